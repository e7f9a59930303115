// Anisotropic linear elasticity on vector CG1 spaces (tetrahedra, and triangles in plane strain): the stiffness operator of a general
// rank-4 tensor C, the per-cell stress sigma = C : (eps(u) - eps*) with its von Mises projection load, and the eigenstrain load.
//
// The reference lists the material as a to-do ("anisotropy needs rank 4 tensor", INTEGRATION.md, "differs from the reference").
// Material (fs_aniso_material, include/fenicssolver_amd.h): a table of symmetric 6x6 matrices D in the tensor order of fs_p1_cell.h
// (xx, yy, zz, xy, xz, yz) acting on (e_xx, e_yy, e_zz, 2 e_xy, 2 e_xz, 2 e_yz), D_IJ = C_ikjl with I = (i,k), J = (j,l); one table
// index per cell; optionally one rotation R per cell whose columns are the material axes in global coordinates.
//
// The kernels never rotate C.  With g_a the gradient of the barycentric function a and V the cell volume (area),
//   K_ab[i][j] = V sum_kl g_a[k] C_ikjl g_b[l],
// and for C_global = (R x R x R x R) C the same block is R Gamma R^T with Gamma built from the rotated gradients R^T g_a, R^T g_b and
// the material-axes C: 72 B of frame per source cell instead of a rotated 168-B tensor.  Contraction per source:
//   T[I][j] = sum_l D[I][J(j,l)] g_b[l]  (6x3),   Gamma[i][j] = sum_k g_a[k] T[I(i,k)][j]   - 81 FMAs.
// Plane strain runs the same code with g[2] = 0 (the compiler drops the dead terms and loads); D must be monoclinic about z and a
// frame a rotation about z, which the host side checks, so that sigma_xz = sigma_yz = 0.
//
// Kernels (no atomics: two assemblies of one state give the same bits):
//   k_assemble_aniso_gather   one thread per STORED block sums its (cell, a, b) sources of the inverse slot table in ascending order,
//       as k_assemble_p1_elasticity_gather does, sources in groups of four: 4 vertex records (24 B each), the 4-B table index, the
//       168-B table row (the same address across a wave when the regions are few) and, FRAME, the 72-B rotation.
//   k_aniso_cell_stress       sigma = C : (eps(u) + s eps*) per cell, 6 doubles (4 in plane strain): the tensor storage.
//   k_aniso_von_mises_load    b_a = int vm lambda_a dx from the stored stress, lane = vertex of the scalar CG1 space, its incidences in
//       ascending cell order (the walk of k_von_mises_load), 2-D deviator convention of the isotropic kernel included.
//   k_p1_stress_force_gather  (fs_p1_cell.h) the eigenstrain load from the stored C : eps*.
#include "fs_common.h"
#include "fs_kernels.h"
#include "fs_p1_cell.h"
#include <math.h>

// tensor storage index of the component (i, k)
__host__ __device__ constexpr int an_voigt(int i, int k) { return i == k ? i : i + k + 2; }
// position of D[I][J] in the stored upper triangle (row-major)
__host__ __device__ constexpr int an_tri(int I, int J) { return I <= J ? I * 6 - I * (I - 1) / 2 + (J - I) : J * 6 - J * (J - 1) / 2 + (I - J); }

struct aniso_dev {
    const double* table;      // [n_materials][21]
    const int32_t* index;     // [n_cells] or nullptr
    const double* frame;      // [n_cells][9] or nullptr
    int64_t identity;         // index == nullptr: 1 when the table has one row per cell, 0 when it has one row
};
__device__ __forceinline__ int64_t an_material(const aniso_dev& M, int64_t c) { return M.index ? (int64_t)M.index[c] : c * M.identity; }

__device__ __forceinline__ void an_load_frame(const double* __restrict__ frame, int64_t c, double (&R)[3][3]) {
    const double* f = frame + 9 * c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = f[3 * i + j];
}

// ---- K: one thread per stored block --------------------------------------------------------------------------------------------
template <int TD, bool ADD, bool FRAME>
__global__ void __launch_bounds__(FS_BLOCK) k_assemble_aniso_gather(int64_t n_entries, const int32_t* __restrict__ ptr,
                                                                    const int32_t* __restrict__ src, const int32_t* __restrict__ cells,
                                                                    const double* __restrict__ xyz4, const aniso_dev M, int mass_mode,
                                                                    double mass_value, const double* __restrict__ mass_cell, int64_t plane,
                                                                    double* __restrict__ val, const box_snap bx) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; e < n_entries; e += stride) {
        double acc[TD][TD];
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int j = 0; j < TD; ++j) acc[i][j] = 0.0;
        const int32_t q1 = ptr[e + 1];
        // sources in groups of four: their indices, then their cell records and table indices, go out before the first coordinate load
        constexpr int PF = 4;
        for (int32_t q0 = ptr[e]; q0 < q1; q0 += PF) {
            int32_t sc[PF];
            int4 vc[PF];
            int64_t mi[PF];
#pragma unroll
            for (int u = 0; u < PF; ++u) sc[u] = q0 + u < q1 ? src[q0 + u] : -1;
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int64_t c = sc[u] >= 0 ? p1_source_cell<TD>(sc[u]) : 0;
                vc[u] = sc[u] >= 0 ? reinterpret_cast<const int4*>(cells)[c] : make_int4(0, 0, 0, 0);
                mi[u] = sc[u] >= 0 ? an_material(M, c) : 0;
            }
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                if (q0 + u >= q1) break;
                int64_t c;
                int a, b;
                p1_source<TD>(sc[u], c, a, b);
                const int4 v4 = vc[u];
                const double* __restrict__ Dm = M.table + 21 * mi[u];
                double ga[3], gb[3], vol, mvol;
                if constexpr (TD == 3) {
                    const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
                    const tet_geom t = tet_geometry_box(xyz4, v, bx);
                    vol = t.adet * (1.0 / 6.0);
                    mvol = t.adet * (1.0 / 120.0);
                    P1_GRAD_TET(t, a, ga);
                    P1_GRAD_TET(t, b, gb);
                } else {
                    const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
                    vol = t.area;
                    mvol = t.area * (1.0 / 12.0);
                    double g2[2];
                    p1_grad(t, a, g2); ga[0] = g2[0]; ga[1] = g2[1]; ga[2] = 0.0;
                    p1_grad(t, b, g2); gb[0] = g2[0]; gb[1] = g2[1]; gb[2] = 0.0;
                }
                double R[3][3];
                if constexpr (FRAME) {       // gradients into the material axes: ghat = R^T g
                    an_load_frame(M.frame, c, R);
                    double ha[3], hb[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        ha[k] = R[0][k] * ga[0] + R[1][k] * ga[1] + R[2][k] * ga[2];
                        hb[k] = R[0][k] * gb[0] + R[1][k] * gb[1] + R[2][k] * gb[2];
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) { ga[k] = ha[k]; gb[k] = hb[k]; }
                }
                double T[6][3];
#pragma unroll
                for (int I = 0; I < 6; ++I)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        T[I][j] = Dm[an_tri(I, an_voigt(j, 0))] * gb[0] + Dm[an_tri(I, an_voigt(j, 1))] * gb[1] + Dm[an_tri(I, an_voigt(j, 2))] * gb[2];
                double G[3][3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        G[i][j] = ga[0] * T[an_voigt(i, 0)][j] + ga[1] * T[an_voigt(i, 1)][j] + ga[2] * T[an_voigt(i, 2)][j];
                if constexpr (FRAME) {       // back to the global axes: R G R^T
                    double W[3][3];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) W[i][j] = R[i][0] * G[0][j] + R[i][1] * G[1][j] + R[i][2] * G[2][j];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) G[i][j] = W[i][0] * R[j][0] + W[i][1] * R[j][1] + W[i][2] * R[j][2];
                }
                double ms = 0.0;
                if (mass_mode != FS_COEF_NONE) ms = (a == b ? 2.0 : 1.0) * (mass_mode == FS_COEF_CONST ? mass_value : mass_cell[c]) * mvol;
#pragma unroll
                for (int i = 0; i < TD; ++i)
#pragma unroll
                    for (int j = 0; j < TD; ++j) {
                        double x = vol * G[i][j];
                        if (i == j) x += ms;
                        acc[i][j] += x;
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int j = 0; j < TD; ++j) {
                const int64_t idx = (int64_t)(i * TD + j) * plane + e;
                val[idx] = ADD ? val[idx] + acc[i][j] : acc[i][j];
            }
    }
}

// ---- the per-cell stress -------------------------------------------------------------------------------------------------------
// sigma = C : (eps(u) + eig_scale eps*); u == nullptr: eps(u) = 0; eig == nullptr: eps* = 0.  Plane strain: the out-of-plane shears
// of the strain are zero, and those of the stress vanish for the materials the host side lets through.
template <int TD, bool FRAME>
__global__ void __launch_bounds__(FS_BLOCK) k_aniso_cell_stress(int64_t nc, const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                                const double* __restrict__ u, const aniso_dev M,
                                                                const double* __restrict__ eig, double eig_scale, const box_snap bx,
                                                                double* __restrict__ out) {
    constexpr int NE = TD == 3 ? 6 : 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += stride) {
        double e[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) e[k] = 0.0;
        if (u) {
            const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
            p1_strain<TD>(v4, xyz4, u, bx, e);
        }
        if (eig) {
#pragma unroll
            for (int k = 0; k < NE; ++k) e[k] += eig_scale * eig[NE * c + k];
        }
        // the symmetric tensor in full
        double E[3][3];
        E[0][0] = e[0]; E[1][1] = e[1]; E[2][2] = e[2];
        E[0][1] = E[1][0] = e[3];
        E[0][2] = E[2][0] = TD == 3 ? e[NE - 2] : 0.0;
        E[1][2] = E[2][1] = TD == 3 ? e[NE - 1] : 0.0;
        double R[3][3];
        if constexpr (FRAME) {               // into the material axes: R^T E R
            an_load_frame(M.frame, c, R);
            double W[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) W[i][j] = R[0][i] * E[0][j] + R[1][i] * E[1][j] + R[2][i] * E[2][j];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) E[i][j] = W[i][0] * R[0][j] + W[i][1] * R[1][j] + W[i][2] * R[2][j];
        }
        const double ev[6] = {E[0][0], E[1][1], E[2][2], 2.0 * E[0][1], 2.0 * E[0][2], 2.0 * E[1][2]};
        const double* __restrict__ Dm = M.table + 21 * an_material(M, c);
        double sv[6];
#pragma unroll
        for (int I = 0; I < 6; ++I) {
            double s = 0.0;
#pragma unroll
            for (int J = 0; J < 6; ++J) s += Dm[an_tri(I, J)] * ev[J];
            sv[I] = s;
        }
        double S[3][3];
        S[0][0] = sv[0]; S[1][1] = sv[1]; S[2][2] = sv[2];
        S[0][1] = S[1][0] = sv[3]; S[0][2] = S[2][0] = sv[4]; S[1][2] = S[2][1] = sv[5];
        if constexpr (FRAME) {               // back: R S R^T
            double W[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) W[i][j] = R[i][0] * S[0][j] + R[i][1] * S[1][j] + R[i][2] * S[2][j];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) S[i][j] = W[i][0] * R[j][0] + W[i][1] * R[j][1] + W[i][2] * R[j][2];
        }
        out[NE * c + 0] = S[0][0]; out[NE * c + 1] = S[1][1]; out[NE * c + 2] = S[2][2]; out[NE * c + 3] = S[0][1];
        if constexpr (TD == 3) { out[NE * c + 4] = S[0][2]; out[NE * c + 5] = S[1][2]; }
    }
}

// ---- right-hand side of the von Mises projection from the stored stress ---------------------------------------------------------
template <int TD>
__global__ void __launch_bounds__(FS_BLOCK) k_aniso_von_mises_load(int64_t n_rows, int64_t n_slices, const int64_t* __restrict__ inc_slice_ptr,
                                                                   const int32_t* __restrict__ inc_cell, const int32_t* __restrict__ cells,
                                                                   const double* __restrict__ xyz4, const double* __restrict__ sig,
                                                                   double* __restrict__ b) {
    constexpr int NE = TD == 3 ? 6 : 4;
    const int lane = threadIdx.x & 63;
    int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (; s < n_slices; s += stride) {
        const int64_t row = s * FS_SLICE + lane;
        const int64_t ibase = inc_slice_ptr[s];
        const int iwidth = (int)((inc_slice_ptr[s + 1] - ibase) >> 6);
        double acc = 0.0;
        for (int j = 0; j < iwidth; ++j) {
            const int32_t q = inc_cell[ibase + (int64_t)j * FS_SLICE + lane];
            if (q < 0) continue;
            const int64_t c = TD == 3 ? q >> 2 : q / 3;
            const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
            const double* __restrict__ sc = sig + NE * c;
            if constexpr (TD == 3) {
                const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
                const tet_geom t = tet_geometry(xyz4, v);
                const double p = (sc[0] + sc[1] + sc[2]) * (1.0 / 3.0);
                const double d0 = sc[0] - p, d1 = sc[1] - p, d2 = sc[2] - p;
                const double ss = d0 * d0 + d1 * d1 + d2 * d2 + 2.0 * (sc[3] * sc[3] + sc[4] * sc[4] + sc[5] * sc[5]);
                acc += 0.25 * (t.adet * (1.0 / 6.0)) * sqrt(1.5 * ss);
            } else {
                // the reference's expression with dimension 2: the 2x2 tensor less tr / 3 (k_von_mises_load_tri)
                const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
                const double pm = (sc[0] + sc[1]) * (1.0 / 3.0);
                const double ss = (sc[0] - pm) * (sc[0] - pm) + (sc[1] - pm) * (sc[1] - pm) + 2.0 * sc[3] * sc[3];
                acc += t.area * (1.0 / 3.0) * sqrt(1.5 * ss);
            }
        }
        if (row < n_rows) b[row] = acc;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the material on the device, checked first: nothing is enqueued for a material that is refused
struct aniso_store {
    dbuf<double> table, frame;
    dbuf<int32_t> index;
    aniso_dev dev;
};

static int aniso_upload(const fs_aniso_material* mat, const fs_mesh_s* m, aniso_store& st, hipStream_t s, const char* who) {
    FS_REQUIRE(mat, "%s: null material", who);
    FS_REQUIRE(mat->n_materials >= 1 && mat->stiffness, "%s: the material needs n_materials >= 1 (got %lld) and a stiffness table", who,
               (long long)mat->n_materials);
    const int64_t nm = mat->n_materials, nc = m->nc;
    double dmax = 0.0;
    for (int64_t k = 0; k < 21 * nm; ++k) {
        FS_REQUIRE(isfinite(mat->stiffness[k]), "%s: material %lld has a stiffness entry that is not finite", who, (long long)(k / 21));
        dmax = fmax(dmax, fabs(mat->stiffness[k]));
    }
    if (mat->material_of_cell) {
        for (int64_t c = 0; c < nc; ++c)
            FS_REQUIRE(mat->material_of_cell[c] >= 0 && mat->material_of_cell[c] < nm,
                       "%s: cell %lld (device order) has material index %d outside 0 .. %lld", who, (long long)c, mat->material_of_cell[c],
                       (long long)(nm - 1));
    } else {
        FS_REQUIRE(nm == 1 || nm == nc, "%s: without material_of_cell the table holds 1 material or one per cell (%lld), got %lld", who,
                   (long long)nc, (long long)nm);
    }
    if (mat->frame)
        for (int64_t k = 0; k < 9 * nc; ++k)
            FS_REQUIRE(isfinite(mat->frame[k]), "%s: the frame of cell %lld (device order) is not finite", who, (long long)(k / 9));
    if (m->tdim == 2) {
        // plane strain: monoclinic about z (no coupling of the in-plane strains and e_zz with the out-of-plane shear stresses) ...
        for (int64_t k = 0; k < nm; ++k)
            for (int I = 0; I < 4; ++I)
                for (int J = 4; J < 6; ++J)
                    FS_REQUIRE(fabs(mat->stiffness[21 * k + an_tri(I, J)]) <= 1e-12 * dmax,
                               "%s: plane strain needs a material that is monoclinic about z; material %lld has D[%d][%d] = %g", who,
                               (long long)k, I, J, mat->stiffness[21 * k + an_tri(I, J)]);
        // ... and frames that keep z
        if (mat->frame)
            for (int64_t c = 0; c < nc; ++c) {
                const double* R = mat->frame + 9 * c;
                FS_REQUIRE(fabs(R[2]) <= 1e-12 && fabs(R[5]) <= 1e-12 && fabs(R[6]) <= 1e-12 && fabs(R[7]) <= 1e-12 && fabs(R[8] - 1.0) <= 1e-12,
                           "%s: plane strain needs frames that are rotations about z; cell %lld (device order) has another", who, (long long)c);
            }
    }
    FS_CHECK(st.table.alloc(21 * nm));
    FS_CHECK(st.table.upload(mat->stiffness, 21 * nm, s));
    if (mat->material_of_cell) {
        FS_CHECK(st.index.alloc(nc));
        FS_CHECK(st.index.upload(mat->material_of_cell, nc, s));
    }
    if (mat->frame) {
        FS_CHECK(st.frame.alloc(9 * nc));
        FS_CHECK(st.frame.upload(mat->frame, 9 * nc, s));
    }
    st.dev.table = st.table.p;
    st.dev.index = st.index.p;
    st.dev.frame = st.frame.p;
    st.dev.identity = (!mat->material_of_cell && nm == nc && nm > 1) ? 1 : 0;
    return FS_OK;
}

static int aniso_upload_eigenstrain(const double* eig, const fs_mesh_s* m, dbuf<double>& store, hipStream_t s, const char* who) {
    if (!eig) return FS_OK;
    const int ne = m->tdim == 3 ? 6 : 4;
    for (int64_t k = 0; k < ne * m->nc; ++k)
        FS_REQUIRE(isfinite(eig[k]), "%s: the eigenstrain of cell %lld (device order) is not finite", who, (long long)(k / ne));
    return fs_upload_cell_rows(store, eig, ne, m->nc, s);
}

// sigma = C : (eps(u) + scale eps*) of every cell into out (device)
static void aniso_launch_stress(const fs_space_s* sp, const double* u, const aniso_dev& M, const double* eig, double scale, double* out,
                                hipStream_t s) {
    const fs_mesh_s* m = sp->mesh;
    const box_snap bx = make_box_snap(m);
    fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
        fs_dispatch_bool(M.frame != nullptr, [&](auto FRAME) {
            hipLaunchKernelGGL((k_aniso_cell_stress<decltype(TD)::value, decltype(FRAME)::value>), dim3(fs_grid_for(m->nc)), dim3(FS_BLOCK), 0, s, m->nc,
                               m->cells.p, m->xyz.p, u, M, eig, scale, bx, out);
        });
    });
}

extern "C" int fs_assemble_anisotropic(fs_matrix_t A, const fs_aniso_material* mat, const fs_coef* mass, int add) {
    const char* who = "fs_assemble_anisotropic";
    FS_REFUSE_DG(A, "fs_assemble_anisotropic");
    FS_CHECK(fs_require_init());
    FS_REQUIRE(A, "%s: null matrix", who);
    fs_space_s* sp = A->space;
    FS_CHECK(fs_require_solid_space(sp, who));
    FS_REQUIRE(A->bs == sp->ncomp, "%s: the matrix is not on a vector space", who);
    fs_mesh_s* m = sp->mesh;
    const int mmode = mass ? mass->mode : FS_COEF_NONE;
    FS_REQUIRE(mmode == FS_COEF_NONE || mmode == FS_COEF_CONST || mmode == FS_COEF_CELL, "%s: mass coefficient must be constant or per cell", who);
    FS_REQUIRE(mmode != FS_COEF_CONST || isfinite(mass->value), "%s: the mass coefficient %g is not finite", who, mass->value);
    FS_REQUIRE(mmode != FS_COEF_CELL || mass->data, "%s: coefficient data pointer is null", who);
    hipStream_t s = fs_rt().stream;
    aniso_store st;
    FS_CHECK(aniso_upload(mat, m, st, s, who));
    dbuf<double> mstore;
    if (mmode == FS_COEF_CELL) FS_CHECK(fs_upload_cell_rows(mstore, mass->data, 1, m->nc, s));
    const box_snap bx = make_box_snap(m);
    const double mval = mmode == FS_COEF_CONST ? mass->value : 0.0;
    int rc = FS_OK;
    fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
        fs_dispatch_bool(add != 0, [&](auto ADD) {
            fs_dispatch_bool(st.dev.frame != nullptr, [&](auto FRAME) {
                rc = p1_launch_blocks(sp, s, k_assemble_aniso_gather<decltype(TD)::value, decltype(ADD)::value, decltype(FRAME)::value>, st.dev, mmode,
                                      mval, mstore.p, sp->sell_entries, A->val.p, bx);
            });
        });
    });
    FS_CHECK(rc);
    // (no wait, as fs_assemble_matrix: the host arrays were consumed by the uploads, the stores go back to the pool in stream order)
    return FS_OK;
}

extern "C" int fs_anisotropic_stress(fs_space_t space, fs_vector_t u, const fs_aniso_material* mat, const double* eigenstrain,
                                     double* cell_stress_out, fs_space_t p1_space, fs_vector_t vm_rhs) {
    const char* who = "fs_anisotropic_stress";
    FS_REFUSE_DG_SPACE(space, "fs_anisotropic_stress");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    fs_space_s* sp = space;
    FS_CHECK(fs_require_solid_space(sp, who));
    fs_mesh_s* m = sp->mesh;
    if (u) FS_CHECK(fs_require_displacement(u, sp, who));
    FS_REQUIRE((p1_space != nullptr) == (vm_rhs != nullptr), "%s: the von Mises load needs both the scalar CG1 space and its vector", who);
    if (vm_rhs) {
        FS_REFUSE_DG_SPACE(p1_space, "fs_anisotropic_stress");
        FS_REQUIRE(p1_space->mesh == m, "%s: the two spaces live on different meshes", who);
        FS_REQUIRE(p1_space->ncomp == 1 && p1_space->degree == 1, "%s: the target is the scalar CG1 space of the mesh", who);
        FS_REQUIRE_TABLES(p1_space, who);
        FS_REQUIRE(vm_rhs->d.n >= p1_space->n_dofs_owned, "%s: vector too short", who);
    }
    hipStream_t s = fs_rt().stream;
    aniso_store st;
    FS_CHECK(aniso_upload(mat, m, st, s, who));
    dbuf<double> estore, sstore;
    FS_CHECK(aniso_upload_eigenstrain(eigenstrain, m, estore, s, who));
    const int ne = m->tdim == 3 ? 6 : 4;
    FS_CHECK(sstore.alloc(ne * m->nc));
    aniso_launch_stress(sp, u ? u->d.p : nullptr, st.dev, estore.p, -1.0, sstore.p, s);
    if (vm_rhs) {
        fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
            hipLaunchKernelGGL(k_aniso_von_mises_load<decltype(TD)::value>, dim3(fs_grid_for(p1_space->n_slices * 64, FS_BLOCK, 8192)), dim3(FS_BLOCK), 0,
                               s, p1_space->n_nodes_owned, p1_space->n_slices, p1_space->inc_slice_ptr.p, p1_space->inc_cell.p, m->cells.p, m->xyz.p,
                               sstore.p, vm_rhs->d.p);
        });
    }
    FS_KERNEL_CHECK();
    if (cell_stress_out) FS_CHECK(sstore.download(cell_stress_out, ne * m->nc, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_assemble_anisotropic_load(fs_space_t space, const fs_aniso_material* mat, const double* eigenstrain, fs_vector_t b, int add) {
    const char* who = "fs_assemble_anisotropic_load";
    FS_REFUSE_DG_SPACE(space, "fs_assemble_anisotropic_load");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    fs_space_s* sp = space;
    FS_CHECK(fs_require_solid_space(sp, who));
    fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(eigenstrain && b, "%s: null pointer", who);
    FS_REQUIRE(b->d.n >= sp->n_dofs_owned, "%s: vector too short", who);
    hipStream_t s = fs_rt().stream;
    aniso_store st;
    FS_CHECK(aniso_upload(mat, m, st, s, who));
    dbuf<double> estore, sstore;
    FS_CHECK(aniso_upload_eigenstrain(eigenstrain, m, estore, s, who));
    FS_CHECK(sstore.alloc((m->tdim == 3 ? 6 : 4) * m->nc));
    aniso_launch_stress(sp, nullptr, st.dev, estore.p, 1.0, sstore.p, s);        // C : eps*
    const box_snap bx = make_box_snap(m);
    int rc = FS_OK;
    fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
        fs_dispatch_bool(add != 0, [&](auto ADD) {
            rc = p1_launch_nodes(sp, s, k_p1_stress_force_gather<decltype(TD)::value, decltype(ADD)::value>, sstore.p, bx, b->d.p);
        });
    });
    FS_CHECK(rc);
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}
