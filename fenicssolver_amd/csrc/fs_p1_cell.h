// P1 cell helpers shared by the solid-mechanics kernel files (fs_hyper.hip, fs_buckling.hip, fs_large_deformation.hip,
// fs_plasticity.hip, fs_viscoelasticity.hip): the gather-map source decode, the diagonal-block lookup, the gradient pick, the strain of a P1 cell,
// symmetric tensor times vector, the stored-stress force gather, the per-cell tally and the host pieces every such solver repeats
// (space check, committed / trial buffer pair, first-cell number).
//
// Tensor storage: 3-D (xx, yy, zz, xy, xz, yz), plane strain (xx, yy, zz, xy) - tensor components, not engineering shears.
// Nothing here sets fp contraction: a helper takes the default of the file, and a caller's "#pragma clang fp contract(off)" region
// does not reach into it.
#pragma once
#include "fs_p1_geometry.h"

// ---- gather-map sources ------------------------------------------------------------------------------------------------------
// source index = cell * 16 + a * 4 + b on tetrahedra, cell * 9 + a * 3 + b on triangles
template <int TD>
__device__ __forceinline__ int32_t p1_source_cell(int32_t sidx) { return TD == 3 ? sidx >> 4 : sidx / 9; }

template <int TD>
__device__ __forceinline__ void p1_source(int32_t sidx, int64_t& c, int& a, int& b) {
    c = p1_source_cell<TD>(sidx);
    if constexpr (TD == 3) {
        a = (sidx >> 2) & 3; b = sidx & 3;
    } else {
        const int ab = sidx - (int32_t)(c * 9);
        a = ab / 3; b = ab - 3 * a;
    }
}

// the stored (SELL) entry of the diagonal block of row r, -1 if the row has none; its sources are (c, a, a) for every cell c holding
// the node, ascending in c
__device__ __forceinline__ int64_t p1_diag_entry(int64_t r, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col) {
    const int64_t sp0 = slice_ptr[r >> 6];
    const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
    const int64_t base = sp0 + (r & 63);
    for (int k = 0; k < width; ++k)
        if (sell_col[base + (int64_t)k * FS_SLICE] == (int32_t)r) return base + (int64_t)k * FS_SLICE;
    return -1;
}

// ---- gradient pick -----------------------------------------------------------------------------------------------------------
// g_a for a run-time a: a select chain, never an index into t.g (that would put the register array into scratch).
// The tetrahedron's chain is a macro, to be expanded where the tet_geom is a local: the kernels' bits depend on it.  g_0 is the sum
// -(g_1 + g_2 + g_3) of products, and whether the compiler contracts that sum depends on where it ends up relative to the chain; as
// a function taking the geometry by reference the chain is optimised on its own first, and the 3-D force gathers round g_0 differently.
#define P1_GRAD_TET(T_, A_, OUT_)                                                                                       \
    _Pragma("unroll") for (int k_ = 0; k_ < 3; ++k_)(OUT_)[k_] =                                                        \
        (A_) == 0 ? (T_).g[0][k_] : (A_) == 1 ? (T_).g[1][k_] : (A_) == 2 ? (T_).g[2][k_] : (T_).g[3][k_]
// the triangle reads the components first: a chain over the members of a referenced tri_geom ends as one load through a selected
// address, and the struct leaves the registers
__device__ __forceinline__ double p1_pick(int a, double x0, double x1, double x2) { return a == 0 ? x0 : (a == 1 ? x1 : x2); }
__device__ __forceinline__ void p1_grad(const tri_geom& t, int a, double (&g)[2]) {
    g[0] = p1_pick(a, t.g[0][0], t.g[1][0], t.g[2][0]);
    g[1] = p1_pick(a, t.g[0][1], t.g[1][1], t.g[2][1]);
}

// g_a and the volume (area) of the cell v4
template <int TD>
__device__ __forceinline__ void p1_weighted_grad(int4 v4, const double* __restrict__ xyz4, const box_snap& bx, int a, double (&ga)[TD],
                                                 double& vol) {
    if constexpr (TD == 3) {
        const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
        const tet_geom t = tet_geometry_box(xyz4, v, bx);
        vol = t.adet * (1.0 / 6.0);
        P1_GRAD_TET(t, a, ga);
    } else {
        const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
        vol = t.area;
        p1_grad(t, a, ga);
    }
}

// y = S x for a stored symmetric tensor: 3-D S = [[s0, s3, s4], [s3, s1, s5], [s4, s5, s2]], plane strain the in-plane part
// [[s0, s3], [s3, s1]]
template <int TD>
__device__ __forceinline__ void p1_sym_mul(const double (&s)[TD == 3 ? 6 : 4], const double (&x)[TD], double (&y)[TD]) {
    if constexpr (TD == 3) {
        y[0] = s[0] * x[0] + s[3] * x[1] + s[4] * x[2];
        y[1] = s[3] * x[0] + s[1] * x[1] + s[5] * x[2];
        y[2] = s[4] * x[0] + s[5] * x[1] + s[2] * x[2];
    } else {
        y[0] = s[0] * x[0] + s[3] * x[1];
        y[1] = s[3] * x[0] + s[1] * x[1];
    }
}

// ---- strain and stress ---------------------------------------------------------------------------------------------------------
// sym grad u of the P1 displacement u on the cell v4, in the tensor storage (plane strain: e_zz = 0)
template <int TD>
__device__ __forceinline__ void p1_strain(int4 v4, const double* __restrict__ xyz4, const double* __restrict__ u, const box_snap& bx,
                                          double (&e)[TD == 3 ? 6 : 4]) {
    if constexpr (TD == 3) {
        const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
        const tet_geom t = tet_geometry_box(xyz4, v, bx);
        double H[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) H[i][j] = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double ua = u[3 * (int64_t)v[a] + i];
#pragma unroll
                for (int j = 0; j < 3; ++j) H[i][j] += ua * t.g[a][j];
            }
        e[0] = H[0][0]; e[1] = H[1][1]; e[2] = H[2][2];
        e[3] = 0.5 * (H[0][1] + H[1][0]); e[4] = 0.5 * (H[0][2] + H[2][0]); e[5] = 0.5 * (H[1][2] + H[2][1]);
    } else {
        const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
        const int32_t v[3] = {v4.x, v4.y, v4.z};
        double H[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double2 ua = reinterpret_cast<const double2*>(u)[v[a]];
            H[0][0] += ua.x * t.g[a][0]; H[0][1] += ua.x * t.g[a][1];
            H[1][0] += ua.y * t.g[a][0]; H[1][1] += ua.y * t.g[a][1];
        }
        e[0] = H[0][0]; e[1] = H[1][1]; e[2] = 0.0; e[3] = 0.5 * (H[0][1] + H[1][0]);
    }
}

// f_a = int B^T sigma dx = sum over the cells around the node of V sigma g_a, from a per-cell stress array sig[nc][NE]
template <int TD, bool ADD>
__global__ void __launch_bounds__(FS_BLOCK) k_p1_stress_force_gather(int64_t n_rows, const int64_t* __restrict__ slice_ptr,
                                                                     const int32_t* __restrict__ sell_col, const int32_t* __restrict__ gptr,
                                                                     const int32_t* __restrict__ gsrc, const int32_t* __restrict__ cells,
                                                                     const double* __restrict__ xyz4, const double* __restrict__ sig,
                                                                     const box_snap bx, double* __restrict__ f) {
    constexpr int NE = TD == 3 ? 6 : 4;
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_rows; r += stride) {
        double acc[TD];
#pragma unroll
        for (int i = 0; i < TD; ++i) acc[i] = 0.0;
        const int64_t e = p1_diag_entry(r, slice_ptr, sell_col);
        if (e >= 0) {
            const int32_t q1 = gptr[e + 1];
            for (int32_t q = gptr[e]; q < q1; ++q) {
                int64_t c;
                int a, b;
                p1_source<TD>(gsrc[q], c, a, b);
                const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
                double s[NE], ga[TD], w[TD], vol;
                const double2* sc = reinterpret_cast<const double2*>(sig + NE * c);
#pragma unroll
                for (int j = 0; j < NE; j += 2) {
                    const double2 x = sc[j >> 1];
                    s[j] = x.x; s[j + 1] = x.y;
                }
                p1_weighted_grad<TD>(v4, xyz4, bx, a, ga, vol);
                p1_sym_mul<TD>(s, ga, w);
#pragma unroll
                for (int i = 0; i < TD; ++i) acc[i] += vol * w[i];
            }
        }
#pragma unroll
        for (int i = 0; i < TD; ++i) f[TD * r + i] = ADD ? f[TD * r + i] + acc[i] : acc[i];
    }
}

// ---- cell tally ----------------------------------------------------------------------------------------------------------------
// Per-thread counts n[N], a smallest cell index and (SUM) one fp64 sum, reduced over the workgroup in a fixed order: the shuffle-down
// tree inside a wave, then the waves in index order.  Thread 0 writes the partials of the workgroup: part[k][gridDim.x] for count
// k, part[N][gridDim.x] for the smallest index, part_sum[gridDim.x].  k_cell_tally_finish sums them in workgroup order.
template <int N, bool SUM>
__device__ __forceinline__ void p1_cell_tally(int64_t (&n)[N], int64_t first, double sum, int64_t* __restrict__ part,
                                              double* __restrict__ part_sum) {
    __shared__ double ss[SUM ? FS_BLOCK / 64 : 1];
    __shared__ int64_t sn[N + 1][FS_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        if (SUM) sum += __shfl_down(sum, off, 64);
#pragma unroll
        for (int k = 0; k < N; ++k) n[k] += __shfl_down(n[k], off, 64);
        const int64_t o = __shfl_down(first, off, 64);
        first = o < first ? o : first;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        if (SUM) ss[wave] = sum;
#pragma unroll
        for (int k = 0; k < N; ++k) sn[k][wave] = n[k];
        sn[N][wave] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0;
        int64_t tn[N], tf = INT64_MAX;
#pragma unroll
        for (int k = 0; k < N; ++k) tn[k] = 0;
        for (int w = 0; w < FS_BLOCK / 64; ++w) {
            if (SUM) ts += ss[w];
#pragma unroll
            for (int k = 0; k < N; ++k) tn[k] += sn[k][w];
            tf = sn[N][w] < tf ? sn[N][w] : tf;
        }
        if (SUM) part_sum[blockIdx.x] = ts;
#pragma unroll
        for (int k = 0; k < N; ++k) part[(int64_t)k * gridDim.x + blockIdx.x] = tn[k];
        part[(int64_t)N * gridDim.x + blockIdx.x] = tf;
    }
}

// one thread: out[k] = the counts, out[N] = the smallest index, out_sum[0] = the sum, over the nb workgroups in index order
template <int N, bool SUM>
__global__ void k_cell_tally_finish(int nb, const int64_t* __restrict__ part, const double* __restrict__ part_sum,
                                    int64_t* __restrict__ out, double* __restrict__ out_sum) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double ts = 0.0;
    int64_t tn[N], tf = INT64_MAX;
#pragma unroll
    for (int k = 0; k < N; ++k) tn[k] = 0;
    for (int b = 0; b < nb; ++b) {
        if (SUM) ts += part_sum[b];
#pragma unroll
        for (int k = 0; k < N; ++k) tn[k] += part[(int64_t)k * nb + b];
        tf = part[(int64_t)N * nb + b] < tf ? part[(int64_t)N * nb + b] : tf;
    }
    if (SUM) out_sum[0] = ts;
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = tn[k];
    out[N] = tf;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the spaces these solvers are written for: vector CG1 on tetrahedra or triangles, one rank
static inline int fs_require_vector_cg1(const fs_space_s* sp, const char* who) {
    FS_REFUSE_DG_SPACE(sp, who);
    FS_REQUIRE(sp, "%s: null space", who);
    const fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(sp->degree == 1 && ((m->tdim == 3 && sp->ncomp == 3) || (m->tdim == 2 && sp->ncomp == 2)),
               "%s: vector CG1 spaces on tetrahedra or triangles only (this space: CG%d with %d components on a %d-D mesh)", who, sp->degree,
               sp->ncomp, m->tdim);
    FS_REQUIRE(m->n_owned == m->nv && sp->n_nodes_owned == sp->n_nodes_local, "%s: the space has ghost nodes (several ranks): not supported", who);
    return FS_OK;
}

// one field of a per-cell history: the committed state and the trial state of the last evaluation
struct fs_history_pair {
    dbuf<double> committed, trial;
    int alloc(int64_t n) {
        FS_CHECK(committed.alloc(n));
        return trial.alloc(n);
    }
    int zero(hipStream_t s) {
        FS_CHECK(committed.zero(s));
        return trial.zero(s);
    }
    int commit(hipStream_t s) {              // trial -> committed
        if (trial.n) FS_HIP(hipMemcpyAsync(committed.p, trial.p, (size_t)trial.n * sizeof(double), hipMemcpyDeviceToDevice, s));
        return FS_OK;
    }
    const dbuf<double>& pick(bool trial_) const { return trial_ ? trial : committed; }
};

// the first flagged cell of a tally (a device cell index, meaningful when n_flagged > 0) in the caller's numbering; -1: none
static inline int64_t fs_first_cell(const fs_mesh_s* m, int64_t n_flagged, int64_t first) {
    if (n_flagged <= 0) return -1;
    return m->cell_order.empty() ? first : m->cell_order[first];
}
