// Geometric (initial-stress) stiffness of a linear-elastic prestress on vector CG1 spaces (tetrahedra, and triangles in plane
// strain): the K_G of the linear buckling pencil (K + lambda K_G) phi = 0.
//
// The reference has no buckling path ("differs from the reference"); the formulation is the classical one of
// eigenvalue buckling (Cook, Malkus, Plesha & Witt, "Concepts and Applications of FEA", ch. 18).  A P1 displacement u0 has a constant
// gradient per cell, so the Cauchy stress of the static solution is constant per cell,
//   sigma_c = lambda tr(eps) I + 2 mu eps,  eps = sym grad u0,
// and with g_a the gradients of the barycentric functions and V the cell volume (area)
//   K_G[(a,i),(b,j)] = delta_ij s_ab,   s_ab = sum over the cells holding a and b of V g_a . sigma_c g_b.
// Every node-pair block is s_ab times the identity.  It is stored as an ordinary block matrix of the space (off-diagonal block entries
// exactly 0.0), so fs_spmv, fs_matrix_get_csr and fs_apply_dirichlet take it unchanged; the eigensolver reads a compact copy of one
// double per node pair (k_pencil_compact, fs_eigen.hip).  Plane strain: sigma_zz = lambda tr(eps) is recorded but does not enter K_G
// (the in-plane gradients have no z component).
//
// Kernels (no atomics: two assemblies of one state give the same bits):
//   k_geometric_stiffness_gather  one thread per STORED block sums its (cell, a, b) sources of the inverse slot table in ascending
//       order, as the linear gather and k_hyper_tangent_gather do, and rebuilds the stress of the source cell: 4 vertex records
//       (24 B) + 4 displacements (24 B) + the 16-B cell record per source.
//   k_cell_stress                 the per-cell stress record, 6 doubles (xx, yy, zz, xy, xz, yz) or 4 in plane strain (xx, yy, zz,
//       xy): the tensor storage of fs_p1_cell.h.
#include "fs_common.h"
#include "fs_kernels.h"
#include "fs_p1_cell.h"
#include <math.h>

// sigma = lambda tr(e) I + 2 mu e in the tensor storage (plane strain: e[2] = 0 on entry, s[2] = lambda tr)
template <int TD>
__device__ __forceinline__ void gs_stress(const double (&e)[TD == 3 ? 6 : 4], double mu, double lambda, double (&s)[TD == 3 ? 6 : 4]) {
    const double ltr = lambda * ((e[0] + e[1]) + e[2]);
    const double m2 = 2.0 * mu;
    s[0] = ltr + m2 * e[0];
    s[1] = ltr + m2 * e[1];
    s[2] = ltr + m2 * e[2];
#pragma unroll
    for (int k = 3; k < (TD == 3 ? 6 : 4); ++k) s[k] = m2 * e[k];
}

// ---- K_G: one thread per stored block ------------------------------------------------------------------------------------------
template <int TD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_geometric_stiffness_gather(int64_t n_entries, const int32_t* __restrict__ ptr,
                                                                         const int32_t* __restrict__ src, const int32_t* __restrict__ cells,
                                                                         const double* __restrict__ xyz4, const double* __restrict__ u,
                                                                         double mu0, double lambda0, const double2* __restrict__ lame_cell,
                                                                         int64_t plane, double* __restrict__ val, const box_snap bx) {
    constexpr int NE = TD == 3 ? 6 : 4;
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; e < n_entries; e += stride) {
        double acc = 0.0;
        const int32_t q1 = ptr[e + 1];
        for (int32_t q = ptr[e]; q < q1; ++q) {
            int64_t c;
            int a, b;
            p1_source<TD>(src[q], c, a, b);
            const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
            const double2 ml = CELL ? lame_cell[c] : make_double2(mu0, lambda0);
            double eps[NE], sig[NE], ga[TD], gb[TD], w[TD], vol;
            if constexpr (TD == 3) {
                const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
                const tet_geom t = tet_geometry_box(xyz4, v, bx);
                vol = t.adet * (1.0 / 6.0);
                p1_strain_of(t, v, u, eps);
                P1_GRAD_TET(t, a, ga);
                P1_GRAD_TET(t, b, gb);
            } else {
                const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
                vol = t.area;
                p1_strain_of(t, v4, u, eps);
                p1_grad(t, a, ga);
                p1_grad(t, b, gb);
            }
            gs_stress<TD>(eps, ml.x, ml.y, sig);
            p1_sym_mul<TD>(sig, gb, w);
            double d = 0.0;
#pragma unroll
            for (int i = 0; i < TD; ++i) d += ga[i] * w[i];
            acc += vol * d;
        }
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int j = 0; j < TD; ++j) val[(int64_t)(i * TD + j) * plane + e] = i == j ? acc : 0.0;
    }
}

// ---- the per-cell stress record ------------------------------------------------------------------------------------------------
template <int TD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_cell_stress(int64_t nc, const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                          const double* __restrict__ u, double mu0, double lambda0,
                                                          const double2* __restrict__ lame_cell, const box_snap bx, double* __restrict__ out) {
    constexpr int NE = TD == 3 ? 6 : 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += stride) {
        const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
        const double2 ml = CELL ? lame_cell[c] : make_double2(mu0, lambda0);
        double eps[NE], sig[NE];
        if constexpr (TD == 3) {
            const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
            const tet_geom t = tet_geometry_box(xyz4, v, bx);
            p1_strain_of(t, v, u, eps);
        } else {
            const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
            p1_strain_of(t, v4, u, eps);
        }
        gs_stress<TD>(eps, ml.x, ml.y, sig);
#pragma unroll
        for (int k = 0; k < NE; ++k) out[NE * c + k] = sig[k];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int fs_assemble_geometric_stiffness(fs_space_t space, double mu, double lambda, const double* lame_cells, fs_vector_t u,
                                               fs_matrix_t KG, double* cell_stress_out) {
    FS_REFUSE_DG_SPACE(space, "fs_assemble_geometric_stiffness"); FS_REFUSE_DG(KG, "fs_assemble_geometric_stiffness");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(space && u && KG, "fs_assemble_geometric_stiffness: null pointer");
    fs_space_s* sp = space;
    FS_CHECK(fs_require_solid_space(sp, "fs_assemble_geometric_stiffness"));
    fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(KG->space == sp && KG->bs == sp->ncomp, "fs_assemble_geometric_stiffness: the matrix is not on this space");
    FS_CHECK(fs_require_displacement(u, sp, "fs_assemble_geometric_stiffness"));
    const bool cellw = lame_cells != nullptr;
    FS_REQUIRE(cellw || (isfinite(mu) && isfinite(lambda)), "fs_assemble_geometric_stiffness: mu = %g, lambda = %g are not finite", mu, lambda);
    hipStream_t s = fs_rt().stream;
    dbuf<double> lstore, sstore;
    if (cellw) {
        for (int64_t c = 0; c < m->nc; ++c)
            FS_REQUIRE(isfinite(lame_cells[2 * c]) && isfinite(lame_cells[2 * c + 1]),
                       "fs_assemble_geometric_stiffness: cell %lld (device order) has mu = %g, lambda = %g", (long long)c, lame_cells[2 * c],
                       lame_cells[2 * c + 1]);
        FS_CHECK(fs_upload_cell_rows(lstore, lame_cells, 2, m->nc, s));
    }
    const double2* lc = reinterpret_cast<const double2*>(lstore.p);
    FS_CHECK(p1_gather_map(sp, s));          // ahead of the allocation below, as it was
    const box_snap bx = make_box_snap(m);
    const int ne = m->tdim == 3 ? 6 : 4;
    if (cell_stress_out) FS_CHECK(sstore.alloc(ne * m->nc));
    int rc = FS_OK;
    fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
        fs_dispatch_bool(cellw, [&](auto CELL) {
            constexpr int td = decltype(TD)::value;
            constexpr bool c = decltype(CELL)::value;
            rc = p1_launch_blocks(sp, s, k_geometric_stiffness_gather<td, c>, u->d.p, mu, lambda, lc, sp->sell_entries, KG->val.p, bx);
            if (rc == FS_OK && cell_stress_out)
                hipLaunchKernelGGL((k_cell_stress<td, c>), dim3(fs_grid_for(m->nc)), dim3(FS_BLOCK), 0, s, m->nc, m->cells.p, m->xyz.p, u->d.p, mu,
                                   lambda, lc, bx, sstore.p);
        });
    });
    FS_CHECK(rc);
    FS_KERNEL_CHECK();
    if (cell_stress_out) FS_CHECK(sstore.download(cell_stress_out, ne * m->nc, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}
