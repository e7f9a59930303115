// P1 cell helpers shared by the solid-mechanics kernel files (fs_hyper.hip, fs_hyper_models.hip, fs_hyper_dynamics.hip,
// fs_buckling.hip, fs_anisotropic.hip, fs_large_deformation.hip, fs_plasticity.hip, fs_viscoelasticity.hip).
// Device side: the gather-map source decode, the diagonal-block lookup, the gradient pick, the strain of a P1 cell, symmetric tensor
// times vector, the stored-stress force gather and the per-cell tally.
// Host side, the body every entry point of these files shares: the checks of the space and of the handles (fs_require_*), the upload
// of a checked per-cell table, the two launch shapes of the gathers (p1_launch_blocks, p1_launch_nodes - they own the grids, the
// leading arguments and the lazy build of the gather map), the cell tally's buffers (fs_cell_tally), the committed / trial buffer
// pair and the space binding of a per-cell history, and the first-cell number.
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
// sym grad u of the P1 displacement u on a cell whose geometry is at hand, in the tensor storage (plane strain: e_zz = 0)
__device__ __forceinline__ void p1_strain_of(const tet_geom& t, const int32_t (&v)[4], const double* __restrict__ u, double (&e)[6]) {
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
}

__device__ __forceinline__ void p1_strain_of(const tri_geom& t, int4 v4, const double* __restrict__ u, double (&e)[4]) {
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

// ... and on the cell v4
template <int TD>
__device__ __forceinline__ void p1_strain(int4 v4, const double* __restrict__ xyz4, const double* __restrict__ u, const box_snap& bx,
                                          double (&e)[TD == 3 ? 6 : 4]) {
    if constexpr (TD == 3) {
        const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
        p1_strain_of(tet_geometry_box(xyz4, v, bx), v, u, e);
    } else {
        p1_strain_of(tri_geometry2(xyz4, v4.x, v4.y, v4.z), v4, u, e);
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

// ---- host side: the checks of an entry point ------------------------------------------------------------------------------------
// `who` is the name of the C entry point, as its messages give it.
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

// ... with the slot table that the gather map inverts: what an entry point that launches a gather asks of its space
static inline int fs_require_solid_space(const fs_space_s* sp, const char* who) {
    FS_CHECK(fs_require_vector_cg1(sp, who));
    FS_REQUIRE(sp->slots.p, "%s: vector space without slot table", who);
    return FS_OK;
}

static inline int fs_require_displacement(const fs_vector_s* u, const fs_space_s* sp, const char* who) {
    FS_REQUIRE(u->d.n >= sp->n_dofs_local, "%s: displacement vector shorter than the space's dofs", who);
    return FS_OK;
}

// the outputs of a tangent / internal-force assembly: K where the tangent is asked for, r where the force is
static inline int fs_require_tangent_force(bool tangent, const fs_matrix_s* K, bool force, const fs_vector_s* r, const fs_space_s* sp,
                                           const char* who) {
    FS_REQUIRE(!tangent || (K && K->space == sp), "%s: the tangent needs a matrix on this space", who);
    FS_REQUIRE(!force || (r && r->d.n >= sp->n_dofs_owned), "%s: the internal force needs a vector of the space's owned dofs", who);
    return FS_OK;
}

// a per-cell table [nc][width] whose rows the caller has checked, on the device
static inline int fs_upload_cell_rows(dbuf<double>& store, const double* rows, int width, int64_t nc, hipStream_t s) {
    FS_CHECK(store.alloc((int64_t)width * nc));
    return store.upload(rows, (int64_t)width * nc, s);
}

// ---- host side: the two launch shapes --------------------------------------------------------------------------------------------
// Every gather of these files is launched one of two ways, and reads the gather map (the inverse of the slot table, built on the
// first use of a space and kept by it).  The two helpers below build it when it is missing, so no caller needs to.  Some callers
// still call p1_gather_map themselves, to keep the build where it was in the stream: fs_assemble_viscoelastic outside the events
// that time its passes, fs_hyper_dyn_* because k_hdyn_step is not launched through a helper, and the hyperelastic, plasticity and
// geometric-stiffness entry points ahead of a per-cell pass or an allocation that used to follow the build (for these the place
// does not matter to the result; it keeps the order of launches of a space's first call what it was).
static inline int p1_gather_map(fs_space_s* sp, hipStream_t s) { return sp->gmap_ptr.p ? (int)FS_OK : fs_space_build_gather_map(sp, s); }

// one thread per STORED block: kernel(sell_entries, gmap_ptr, gmap_src, cells, xyz, tail...)
template <class K, class... Tail>
static inline int p1_launch_blocks(fs_space_s* sp, hipStream_t s, K kernel, Tail... tail) {
    FS_CHECK(p1_gather_map(sp, s));
    const fs_mesh_s* m = sp->mesh;
    hipLaunchKernelGGL(kernel, dim3(fs_grid_for(sp->sell_entries, FS_BLOCK, 1 << 16)), dim3(FS_BLOCK), 0, s, sp->sell_entries, sp->gmap_ptr.p,
                       sp->gmap_src.p, m->cells.p, m->xyz.p, tail...);
    FS_KERNEL_CHECK();
    return FS_OK;
}

// one thread per owned node: kernel(n_nodes_owned, slice_ptr, sell_col, gmap_ptr, gmap_src, cells, xyz, tail...)
template <class K, class... Tail>
static inline int p1_launch_nodes(fs_space_s* sp, hipStream_t s, K kernel, Tail... tail) {
    FS_CHECK(p1_gather_map(sp, s));
    const fs_mesh_s* m = sp->mesh;
    hipLaunchKernelGGL(kernel, dim3(fs_grid_for(sp->n_nodes_owned, FS_BLOCK, 8192)), dim3(FS_BLOCK), 0, s, sp->n_nodes_owned, sp->slice_ptr.p,
                       sp->sell_col.p, sp->gmap_ptr.p, sp->gmap_src.p, m->cells.p, m->xyz.p, tail...);
    FS_KERNEL_CHECK();
    return FS_OK;
}

// ---- host side: the cell tally ---------------------------------------------------------------------------------------------------
#define FS_CELL_TALLY_BLOCKS 1024      // workgroups of a per-cell pass: its partials are summed in this order, so the number is fixed

// The buffers of p1_cell_tally / k_cell_tally_finish<N, SUM>: the per-cell kernel is launched on nb workgroups with part.p (and
// part_sum.p), finish() sums the partials, get() brings n[0 .. N - 1] (the counts), n[N] (the smallest index) and sum to the host.
// A pass that sums in one mode only (hm_cells_pass: the energy, not with the stress) holds the SUM buffers and finishes with S = false.
template <int N, bool SUM>
struct fs_cell_tally {
    static constexpr int nb = FS_CELL_TALLY_BLOCKS;
    dbuf<double> part_sum, out_sum;          // empty without SUM.  (Declared first: the pool gets the blocks back in the order out,
    dbuf<int64_t> part, out;                 //  part, out_sum, part_sum, and hands them out again in the order of alloc().)
    int64_t n[N + 1] = {};
    double sum = 0.0;
    int alloc() {
        if (SUM) FS_CHECK(part_sum.alloc(nb));
        FS_CHECK(part.alloc((N + 1) * nb));
        if (SUM) FS_CHECK(out_sum.alloc(1));
        return out.alloc(N + 1);
    }
    template <bool S = SUM> int finish(hipStream_t s) {
        hipLaunchKernelGGL((k_cell_tally_finish<N, S>), dim3(1), dim3(64), 0, s, nb, part.p, part_sum.p, out.p, out_sum.p);
        FS_KERNEL_CHECK();
        return FS_OK;
    }
    template <bool S = SUM> int get(hipStream_t s) {
        if (S) FS_CHECK(out_sum.download(&sum, 1, s));
        return out.download(n, N + 1, s);
    }
};

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

// what a per-cell history knows of the space it was created on
struct fs_cell_history {
    fs_space_s* space = nullptr;
    int tdim = 3;
    int ne = 6;                          // stored tensor components (4 in plane strain)
    int64_t nc = 0;
    void bind(fs_space_s* sp) {
        space = sp;
        tdim = sp->mesh->tdim;
        ne = tdim == 3 ? 6 : 4;
        nc = sp->mesh->nc;
    }
    bool owns(const fs_space_s* sp, const fs_mesh_s* m) const { return space == sp && nc == m->nc; }
};

// the first flagged cell of a tally (a device cell index, meaningful when n_flagged > 0) in the caller's numbering; -1: none
static inline int64_t fs_first_cell(const fs_mesh_s* m, int64_t n_flagged, int64_t first) {
    if (n_flagged <= 0) return -1;
    return m->cell_order.empty() ? first : m->cell_order[first];
}
