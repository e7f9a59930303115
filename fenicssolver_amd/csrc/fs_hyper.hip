// Compressible neo-Hookean hyperelasticity on vector CG1 spaces (tetrahedra, and triangles in plane strain): the tangent
// stiffness, the internal force and the stored energy at a displaced state, on the device.  The other energies of
// fs_assemble_hyperelastic (St Venant-Kirchhoff, Mooney-Rivlin, Yeoh) and the Cauchy stress of all four are in fs_hyper_models.hip;
// this file keeps the neo-Hookean expression order and with it the bits.
//
// Stands in for the two UFL derivatives of FenicsSolver/NonlinearElasticitySolver.py:41-98 that solve(F == 0, u, bcs, J=J)
// assembles at every Newton iterate:
//   F = I + grad u,  J = det F,  psi = mu/2 (tr F^T F - 3) - mu ln J + lambda/2 (ln J)^2,
//   P = d psi / dF = mu (F - F^-T) + lambda ln J F^-T.
// A P1 displacement has a constant gradient per cell, so every integrand is constant per cell.  With g_a the reference gradients
// of the barycentric functions, V the cell volume (area) and G_a = F^-T g_a:
//   internal force   f_a = V P g_a
//   tangent block    K_ab[i][k] = V (lambda G_a[i] G_b[k] + (mu - lambda ln J) G_a[k] G_b[i] + delta_ik mu g_a . g_b)
// At u = 0, G = g and ln J = 0 exactly, and the block is the expression of the linear operator (k_assemble_p1_elasticity_gather,
// k_assemble_tri_elasticity_gather) term for term: the two operators agree bit for bit there.
//
// Kernels (no atomics anywhere: two assemblies of one state give the same bits):
//   k_hyper_tangent_gather / k_hyper_tangent_tri_gather  one thread per STORED block sums its (cell, a, b) sources of the inverse
//       slot table in ascending order, as the linear gather does, and rebuilds F, F^-1 and ln J of the source cell: 4 vertex
//       records (24 B) + 4 displacements (24 B) + the 16-B cell record per source, about 400 fp64 flops.
//   k_hyper_force_gather / k_hyper_force_tri_gather      one thread per owned node over the sources of its diagonal block (the
//       cells around the node, ascending), P g_a per cell.
//   k_hyper_cells + k_cell_tally_finish (fs_p1_cell.h)   energy V psi per cell and the cells with J <= 0 (or not finite): per-
//       workgroup partials (p1_cell_tally), then one fixed-order sum.
#include "fs_common.h"
#include "fs_kernels.h"
#include "fs_p1_cell.h"
#include <math.h>

// ---- kinematics ----------------------------------------------------------------------------------------------------------
// F = I + sum_a u_a g_a^T, its cofactor matrix (F^-T = cof / J) and J
// (ld_kinematics of fs_large_deformation.hip computes the same F but sums the vertices into an accumulator that starts at 0, where
// this file groups them ((a0 + a1) + a2) + a3: the two round differently, so each file keeps its own.)
__device__ __forceinline__ void hyper_kin3(const tet_geom& t, const double (&uv)[4][3], double (&F)[3][3], double (&FiT)[3][3],
                                           double& J) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            F[i][j] = (i == j ? 1.0 : 0.0) + (((uv[0][i] * t.g[0][j] + uv[1][i] * t.g[1][j]) + uv[2][i] * t.g[2][j]) + uv[3][i] * t.g[3][j]);
    double c[3][3];
    c[0][0] = F[1][1] * F[2][2] - F[1][2] * F[2][1];
    c[0][1] = F[1][2] * F[2][0] - F[1][0] * F[2][2];
    c[0][2] = F[1][0] * F[2][1] - F[1][1] * F[2][0];
    c[1][0] = F[0][2] * F[2][1] - F[0][1] * F[2][2];
    c[1][1] = F[0][0] * F[2][2] - F[0][2] * F[2][0];
    c[1][2] = F[0][1] * F[2][0] - F[0][0] * F[2][1];
    c[2][0] = F[0][1] * F[1][2] - F[0][2] * F[1][1];
    c[2][1] = F[0][2] * F[1][0] - F[0][0] * F[1][2];
    c[2][2] = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    J = F[0][0] * c[0][0] + F[0][1] * c[0][1] + F[0][2] * c[0][2];
    const double inv = 1.0 / J;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) FiT[i][j] = c[i][j] * inv;
}

__device__ __forceinline__ void hyper_kin2(const tri_geom& t, const double (&uv)[3][2], double (&F)[2][2], double (&FiT)[2][2],
                                           double& J) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) F[i][j] = (i == j ? 1.0 : 0.0) + ((uv[0][i] * t.g[0][j] + uv[1][i] * t.g[1][j]) + uv[2][i] * t.g[2][j]);
    J = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    const double inv = 1.0 / J;
    FiT[0][0] = F[1][1] * inv;  FiT[0][1] = -F[1][0] * inv;
    FiT[1][0] = -F[0][1] * inv; FiT[1][1] = F[0][0] * inv;
}

__device__ __forceinline__ void load_disp3(const double* __restrict__ u, const int32_t (&v)[4], double (&uv)[4][3]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) uv[a][k] = u[3 * (int64_t)v[a] + k];
}

__device__ __forceinline__ void load_disp2(const double* __restrict__ u, int4 v4, double (&uv)[3][2]) {
    const int32_t v[3] = {v4.x, v4.y, v4.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double2 p = reinterpret_cast<const double2*>(u)[v[a]];
        uv[a][0] = p.x; uv[a][1] = p.y;
    }
}

// ---- tangent: tetrahedra -------------------------------------------------------------------------------------------------
// Same source walk as k_assemble_p1_elasticity_gather (source index = cell * 16 + a * 4 + b, groups of four with their cell
// records fetched first).  ms0 is the linear kernel's mass term, passed as a run-time 0 so that the diagonal sum below is the
// same expression (and the same rounding) as there.
template <bool ADD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_hyper_tangent_gather(int64_t n_entries, const int32_t* __restrict__ ptr,
                                                                   const int32_t* __restrict__ src, const int32_t* __restrict__ cells,
                                                                   const double* __restrict__ xyz4, const double* __restrict__ u,
                                                                   double mu0, double lambda0, const double2* __restrict__ lame_cell,
                                                                   double ms0, int64_t plane, double* __restrict__ val, const box_snap bx) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; e < n_entries; e += stride) {
        double acc[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        const int32_t q1 = ptr[e + 1];
        constexpr int PF = 4;
        for (int32_t q0 = ptr[e]; q0 < q1; q0 += PF) {
          int32_t sc[PF];
          int4 vc[PF];
          double2 lc[PF];
#pragma unroll
          for (int w = 0; w < PF; ++w) sc[w] = q0 + w < q1 ? src[q0 + w] : -1;
#pragma unroll
          for (int w = 0; w < PF; ++w) {
            vc[w] = sc[w] >= 0 ? reinterpret_cast<const int4*>(cells)[p1_source_cell<3>(sc[w])] : make_int4(0, 0, 0, 0);
            if (CELL) lc[w] = sc[w] >= 0 ? lame_cell[p1_source_cell<3>(sc[w])] : make_double2(0.0, 0.0);
          }
#pragma unroll
          for (int w = 0; w < PF; ++w) {
            if (q0 + w >= q1) break;
            int64_t c;
            int a, b;
            p1_source<3>(sc[w], c, a, b);
            const int4 v4 = vc[w];
            const double mu = CELL ? lc[w].x : mu0, lambda = CELL ? lc[w].y : lambda0;
            const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
            const tet_geom t = tet_geometry_box(xyz4, v, bx);
            const double vol = t.adet * (1.0 / 6.0);
            double uv[4][3], F[3][3], FiT[3][3], J;
            load_disp3(u, v, uv);
            hyper_kin3(t, uv, F, FiT, J);
            const double m2 = mu - lambda * log(J);
            double ga[3], gb[3];
            P1_GRAD_TET(t, a, ga);
            P1_GRAD_TET(t, b, gb);
            double Ga[3], Gb[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                Ga[i] = FiT[i][0] * ga[0] + FiT[i][1] * ga[1] + FiT[i][2] * ga[2];
                Gb[i] = FiT[i][0] * gb[0] + FiT[i][1] * gb[1] + FiT[i][2] * gb[2];
            }
            const double gg = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double x = vol * (lambda * Ga[i] * Gb[j] + m2 * Ga[j] * Gb[i]);
                    if (i == j) x += vol * mu * gg + ms0;
                    acc[i][j] += x;
                }
          }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int64_t idx = (int64_t)(i * 3 + j) * plane + e;
                val[idx] = ADD ? val[idx] + acc[i][j] : acc[i][j];
            }
    }
}

// ---- tangent: triangles (plane strain), source index = cell * 9 + a * 3 + b, as k_assemble_tri_elasticity_gather -------------
template <bool ADD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_hyper_tangent_tri_gather(int64_t n_entries, const int32_t* __restrict__ ptr,
                                                                       const int32_t* __restrict__ src, const int32_t* __restrict__ cells,
                                                                       const double* __restrict__ xyz4, const double* __restrict__ u,
                                                                       double mu0, double lambda0, const double2* __restrict__ lame_cell,
                                                                       double ms0, int64_t plane, double* __restrict__ val) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; e < n_entries; e += stride) {
        double acc[2][2] = {{0, 0}, {0, 0}};
        const int32_t q1 = ptr[e + 1];
        for (int32_t q = ptr[e]; q < q1; ++q) {
            int64_t c;
            int a, b;
            p1_source<2>(src[q], c, a, b);
            const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
            const double2 ml = CELL ? lame_cell[c] : make_double2(mu0, lambda0);
            const double mu = ml.x, lambda = ml.y;
            const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
            double uv[3][2], F[2][2], FiT[2][2], J;
            load_disp2(u, v4, uv);
            hyper_kin2(t, uv, F, FiT, J);
            const double m2 = mu - lambda * log(J);
            double ga[2], gb[2];
            p1_grad(t, a, ga);
            p1_grad(t, b, gb);
            double Ga[2], Gb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                Ga[i] = FiT[i][0] * ga[0] + FiT[i][1] * ga[1];
                Gb[i] = FiT[i][0] * gb[0] + FiT[i][1] * gb[1];
            }
            const double gg = ga[0] * gb[0] + ga[1] * gb[1];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    double x = t.area * (lambda * Ga[i] * Gb[j] + m2 * Ga[j] * Gb[i]);
                    if (i == j) x += t.area * mu * gg + ms0;
                    acc[i][j] += x;
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t idx = (int64_t)(i * 2 + j) * plane + e;
                val[idx] = ADD ? val[idx] + acc[i][j] : acc[i][j];
            }
    }
}

// ---- internal force ------------------------------------------------------------------------------------------------------
// thread per owned node r: the sources of its diagonal block are (c, a, a) for every cell c holding the node, ascending in c
template <bool ADD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_hyper_force_gather(int64_t n_rows, const int64_t* __restrict__ slice_ptr,
                                                                 const int32_t* __restrict__ sell_col, const int32_t* __restrict__ gptr,
                                                                 const int32_t* __restrict__ gsrc, const int32_t* __restrict__ cells,
                                                                 const double* __restrict__ xyz4, const double* __restrict__ u,
                                                                 double mu0, double lambda0, const double2* __restrict__ lame_cell,
                                                                 const box_snap bx, double* __restrict__ f) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_rows; r += stride) {
        const int64_t e = p1_diag_entry(r, slice_ptr, sell_col);
        double acc[3] = {0.0, 0.0, 0.0};
        if (e >= 0) {
            constexpr int PF = 4;
            const int32_t q1 = gptr[e + 1];
            for (int32_t q0 = gptr[e]; q0 < q1; q0 += PF) {
              int32_t sc[PF];
              int4 vc[PF];
              double2 lc[PF];
#pragma unroll
              for (int w = 0; w < PF; ++w) sc[w] = q0 + w < q1 ? gsrc[q0 + w] : -1;
#pragma unroll
              for (int w = 0; w < PF; ++w) {
                vc[w] = sc[w] >= 0 ? reinterpret_cast<const int4*>(cells)[p1_source_cell<3>(sc[w])] : make_int4(0, 0, 0, 0);
                if (CELL) lc[w] = sc[w] >= 0 ? lame_cell[p1_source_cell<3>(sc[w])] : make_double2(0.0, 0.0);
              }
#pragma unroll
              for (int w = 0; w < PF; ++w) {
                if (q0 + w >= q1) break;
                int64_t c;
                int a, b;
                p1_source<3>(sc[w], c, a, b);
                const int4 v4 = vc[w];
                const double mu = CELL ? lc[w].x : mu0, lambda = CELL ? lc[w].y : lambda0;
                const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
                const tet_geom t = tet_geometry_box(xyz4, v, bx);
                const double vol = t.adet * (1.0 / 6.0);
                double uv[4][3], F[3][3], FiT[3][3], J;
                load_disp3(u, v, uv);
                hyper_kin3(t, uv, F, FiT, J);
                const double ll = lambda * log(J);
                double ga[3];
                P1_GRAD_TET(t, a, ga);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < 3; ++j) s += (mu * (F[i][j] - FiT[i][j]) + ll * FiT[i][j]) * ga[j];
                    acc[i] += vol * s;
                }
              }
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) f[3 * r + i] = ADD ? f[3 * r + i] + acc[i] : acc[i];
    }
}

template <bool ADD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_hyper_force_tri_gather(int64_t n_rows, const int64_t* __restrict__ slice_ptr,
                                                                     const int32_t* __restrict__ sell_col, const int32_t* __restrict__ gptr,
                                                                     const int32_t* __restrict__ gsrc, const int32_t* __restrict__ cells,
                                                                     const double* __restrict__ xyz4, const double* __restrict__ u,
                                                                     double mu0, double lambda0, const double2* __restrict__ lame_cell,
                                                                     double* __restrict__ f) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_rows; r += stride) {
        const int64_t e = p1_diag_entry(r, slice_ptr, sell_col);
        double acc[2] = {0.0, 0.0};
        if (e >= 0) {
            for (int32_t q = gptr[e]; q < gptr[e + 1]; ++q) {
                int64_t c;
                int a, b;
                p1_source<2>(gsrc[q], c, a, b);
                const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
                const double2 ml = CELL ? lame_cell[c] : make_double2(mu0, lambda0);
                const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
                double uv[3][2], F[2][2], FiT[2][2], J;
                load_disp2(u, v4, uv);
                hyper_kin2(t, uv, F, FiT, J);
                const double ll = ml.y * log(J);
                double ga[2];
                p1_grad(t, a, ga);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < 2; ++j) s += (ml.x * (F[i][j] - FiT[i][j]) + ll * FiT[i][j]) * ga[j];
                    acc[i] += t.area * s;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) f[2 * r + i] = ADD ? f[2 * r + i] + acc[i] : acc[i];
    }
}

// ---- energy and inverted cells -------------------------------------------------------------------------------------------
// psi = mu/2 (tr C - 3) - mu ln J + lambda/2 (ln J)^2 with tr C - d = 2 tr H + H : H (H = grad u: no cancellation at small
// strain); 2-D keeps the reference's "- 3" (Identity(2) with the 3-D constant).  A cell counts as inverted when J <= 0 or J is
// not finite.  Partials per workgroup: the energy in part_e, (count, smallest device cell index) in part (p1_cell_tally).
template <int TD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_hyper_cells(int64_t nc, const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                          const double* __restrict__ u, double mu0, double lambda0,
                                                          const double2* __restrict__ lame_cell, const box_snap bx,
                                                          double* __restrict__ part_e, int64_t* __restrict__ part) {
    double en = 0.0;
    int64_t n_bad[1] = {0}, first = INT64_MAX;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += stride) {
        const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
        const double2 ml = CELL ? lame_cell[c] : make_double2(mu0, lambda0);
        double J, trH = 0.0, HH = 0.0, vol;
        if (TD == 3) {
            const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
            const tet_geom t = tet_geometry_box(xyz4, v, bx);
            vol = t.adet * (1.0 / 6.0);
            double uv[4][3], F[3][3], FiT[3][3];
            load_disp3(u, v, uv);
            hyper_kin3(t, uv, F, FiT, J);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double h = F[i][j] - (i == j ? 1.0 : 0.0);
                    if (i == j) trH += h;
                    HH += h * h;
                }
        } else {
            const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
            vol = t.area;
            double uv[3][2], F[2][2], FiT[2][2];
            load_disp2(u, v4, uv);
            hyper_kin2(t, uv, F, FiT, J);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const double h = F[i][j] - (i == j ? 1.0 : 0.0);
                    if (i == j) trH += h;
                    HH += h * h;
                }
        }
        if (!(J > 0.0) || !isfinite(J)) {
            ++n_bad[0];
            first = c < first ? c : first;
            continue;
        }
        const double lj = log(J);
        const double ic3 = (2.0 * trH + HH) + (TD == 3 ? 0.0 : -1.0);
        en += vol * (0.5 * ml.x * ic3 - ml.x * lj + 0.5 * ml.y * lj * lj);
    }
    p1_cell_tally<1, true>(n_bad, first, en, part, part_e);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
extern "C" int fs_assemble_hyperelastic(fs_space_t space, fs_matrix_t K, fs_vector_t r, fs_vector_t u, const fs_hyper_form* form,
                                        int what, fs_hyper_info* info) {
    FS_REFUSE_DG_SPACE(space, "fs_assemble_hyperelastic"); FS_REFUSE_DG(K, "fs_assemble_hyperelastic");
    FS_REQUIRE(space && u && form, "fs_assemble_hyperelastic: null pointer");
    FS_REQUIRE((what & ~(FS_HYPER_TANGENT | FS_HYPER_FORCE | FS_HYPER_ENERGY)) == 0, "fs_assemble_hyperelastic: unknown bits in what (%d)", what);
    FS_REQUIRE(form->model == FS_HYPER_NEO_HOOKEAN || form->model == FS_HYPER_ST_VENANT_KIRCHHOFF || form->model == FS_HYPER_MOONEY_RIVLIN ||
                   form->model == FS_HYPER_YEOH,
               "fs_assemble_hyperelastic: unknown energy model %d (FS_HYPER_NEO_HOOKEAN, _ST_VENANT_KIRCHHOFF, _MOONEY_RIVLIN, _YEOH)", form->model);
    const char* who = "fs_assemble_hyperelastic";
    fs_space_s* sp = space;
    fs_mesh_s* m = sp->mesh;
    FS_CHECK(fs_require_solid_space(sp, who));
    FS_CHECK(fs_require_displacement(u, sp, who));
    FS_CHECK(fs_require_tangent_force(what & FS_HYPER_TANGENT, K, what & FS_HYPER_FORCE, r, sp, who));
    FS_REQUIRE(!(what & FS_HYPER_ENERGY) || info, "fs_assemble_hyperelastic: the energy needs an info struct");
    if (form->model != FS_HYPER_NEO_HOOKEAN) return fs_hyper_models_assemble(sp, K, r, u, form, what, info);      // fs_hyper_models.hip
    FS_REQUIRE(form->lame.mode == FS_COEF_NONE || form->lame.mode == FS_COEF_CELL_LAME,
               "fs_assemble_hyperelastic: the Lame coefficient is FS_COEF_NONE (mu / lambda) or FS_COEF_CELL_LAME");
    FS_REQUIRE(form->lame.mode == FS_COEF_CELL_LAME || (form->mu > 0.0 && form->lambda >= 0.0 && isfinite(form->mu) && isfinite(form->lambda)),
               "fs_assemble_hyperelastic: mu > 0 and lambda >= 0 are required (mu = %g, lambda = %g)", form->mu, form->lambda);
    hipStream_t s = fs_rt().stream;
    dbuf<double> lstore;
    const bool cellw = form->lame.mode == FS_COEF_CELL_LAME;
    if (cellw) {
        FS_REQUIRE(form->lame.data, "fs_assemble_hyperelastic: per-cell Lame data pointer is null");
        for (int64_t c = 0; c < m->nc; ++c) {
            const double mc = form->lame.data[2 * c], lc = form->lame.data[2 * c + 1];
            FS_REQUIRE(mc > 0.0 && lc >= 0.0 && isfinite(mc) && isfinite(lc),
                       "fs_assemble_hyperelastic: cell %lld (device order) has mu = %g, lambda = %g: mu > 0 and lambda >= 0 are required",
                       (long long)c, mc, lc);
        }
        FS_CHECK(fs_upload_cell_rows(lstore, form->lame.data, 2, m->nc, s));
    }
    const double2* lc = reinterpret_cast<const double2*>(lstore.p);
    FS_CHECK(p1_gather_map(sp, s));          // ahead of the first launch, also where only the energy is asked for
    const box_snap bx = make_box_snap(m);
    const double mu = form->mu, lambda = form->lambda, ms0 = 0.0;
    int rc = FS_OK;
    // the tetrahedron's kernels take the box snap, the triangle's do not: two names, selected with the dimension
    fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
        fs_dispatch_bool(form->add != 0, [&](auto ADD) {
            fs_dispatch_bool(cellw, [&](auto CELL) {
                constexpr bool a = decltype(ADD)::value, c = decltype(CELL)::value;
                if (rc == FS_OK && (what & FS_HYPER_TANGENT)) {
                    if constexpr (decltype(TD)::value == 3)
                        rc = p1_launch_blocks(sp, s, k_hyper_tangent_gather<a, c>, u->d.p, mu, lambda, lc, ms0, sp->sell_entries, K->val.p, bx);
                    else
                        rc = p1_launch_blocks(sp, s, k_hyper_tangent_tri_gather<a, c>, u->d.p, mu, lambda, lc, ms0, sp->sell_entries, K->val.p);
                }
                if (rc == FS_OK && (what & FS_HYPER_FORCE)) {
                    if constexpr (decltype(TD)::value == 3) rc = p1_launch_nodes(sp, s, k_hyper_force_gather<a, c>, u->d.p, mu, lambda, lc, bx, r->d.p);
                    else rc = p1_launch_nodes(sp, s, k_hyper_force_tri_gather<a, c>, u->d.p, mu, lambda, lc, r->d.p);
                }
            });
        });
    });
    FS_CHECK(rc);
    if (info) {
        fs_cell_tally<1, true> tally;
        FS_CHECK(tally.alloc());
        fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
            fs_dispatch_bool(cellw, [&](auto CELL) {
                hipLaunchKernelGGL((k_hyper_cells<decltype(TD)::value, decltype(CELL)::value>), dim3(tally.nb), dim3(FS_BLOCK), 0, s, m->nc,
                                   m->cells.p, m->xyz.p, u->d.p, mu, lambda, lc, bx, tally.part_sum.p, tally.part.p);
            });
        });
        FS_KERNEL_CHECK();
        FS_CHECK(tally.finish(s));
        FS_CHECK(tally.get(s));
        info->energy = tally.sum;
        info->n_inverted = tally.n[0];
        info->first_inverted_cell = fs_first_cell(m, tally.n[0], tally.n[1]);
    }
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}
