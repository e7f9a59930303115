// Frictionless unilateral contact against a rigid obstacle, and bilateral sliding supports, on vector CG1 spaces (tetrahedra, and
// triangles in plane strain): the per-node change of basis and the active-set update of LinearElasticitySolver.solve_contact.
//
// The reference lists the boundary condition as not implemented ("differs from the reference"); the method is the
// primal-dual active-set strategy (Hintermueller, Ito & Kunisch, SIAM J. Optim. 13 (2002); Wriggers, "Computational Contact
// Mechanics", ch. 6).  Every constrained node a carries a unit normal n_a.  With k = d - 1 the last axis, s = sgn(n_k) (sgn(0) = +1)
// and v = n + s e_k, the Householder reflector
//   H_a = I - tau v v^T,   tau = 2 / v^T v,
// is symmetric, its own inverse, formed without cancellation for every n, and H_a e_k = sigma_a n_a with sigma_a = -s.  In the
// rotated unknowns u' = H u (H = blockdiag(H_a), the identity on every other node) the normal displacement of node a is the single
// dof u'[d a + k] = sigma_a n_a . u_a, so the constraint n_a . u_a = g_a is a component Dirichlet condition of K' = H K H, b' = H b:
// what fs_apply_dirichlet already does.
//
// Kernels (no atomics on floating-point data: two calls give the same bits):
//   k_rotate_matrix   one wavefront per slice, lane = node row, the row / entry walk of k_dirichlet_sell: the owner of block (a, b)
//       reads its bs x bs planes and writes H_a A_ab H_b.  Blocks with neither node framed are not written.
//   k_rotate_vector   one thread per framed node.
//   k_contact_update  one thread per candidate (consecutive candidates of a slice: consecutive lanes, consecutive entries): the row
//       product of the NORMAL dof only, rho = (K' u' - b')[d a + k], summed in storage order; lambda = -sigma rho, the penetration
//       p = sigma u'[d a + k] - g, and the next flag active ? lambda > 0 : p > 0.  The numbers of changed and of active flags are
//       counted with integer atomics; the last workgroup stores them into two words of pinned host memory.
#include "fs_common.h"
#include "fs_kernels.h"
#include <math.h>
#include <vector>

struct fs_contact_s {
    fs_space_s* space = nullptr;
    int bs = 3;
    int64_t n = 0;                 // framed nodes (candidates and bilateral ones)
    dbuf<int32_t> node;            // [n] ascending
    dbuf<int32_t> frame_of;        // [n_nodes_local] index into node, -1: not framed
    dbuf<double> v;                // [n][4]: the reflector's vector (v_x, v_y, v_z, tau); plane strain: (v_x, v_y, 0, tau)
    dbuf<double> sigma;            // [n] -sgn(n_k)
    dbuf<double> g;                // [n] clearance (contact) or prescribed normal displacement (bilateral)
    dbuf<uint8_t> bilateral;       // [n]
    dbuf<int32_t> active;          // [n]
    dbuf<double> lambda, pen;      // [n] of the last update
    dbuf<int32_t> tally;           // [3]: changed, active, workgroups through; zero between calls
    int* h_counts = nullptr;       // pinned, mapped: [0] changed, [1] active
    int* d_counts = nullptr;
    ~fs_contact_s() {
        if (h_counts) (void)hipHostFree(h_counts);
    }
};

// x <- H x for the reflector (v, tau) in q
template <int BS>
__device__ __forceinline__ void ct_reflect(const double4 q, double (&x)[BS]) {
    const double vv[3] = {q.x, q.y, q.z};
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < BS; ++i) d += vv[i] * x[i];
    d *= q.w;
#pragma unroll
    for (int i = 0; i < BS; ++i) x[i] -= d * vv[i];
}

template <int BS>
__global__ void __launch_bounds__(FS_BLOCK) k_rotate_matrix(int64_t n_rows, int64_t n_slices, const int64_t* __restrict__ slice_ptr,
                                                            const int32_t* __restrict__ sell_col, double* __restrict__ val, int64_t plane,
                                                            const int32_t* __restrict__ frame_of, const double4* __restrict__ refl) {
    const int lane = threadIdx.x & 63;
    int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (; s < n_slices; s += stride) {
        const int64_t r = s * FS_SLICE + lane;
        if (r >= n_rows) continue;
        const int64_t base = slice_ptr[s] + lane;
        const int width = (int)((slice_ptr[s + 1] - slice_ptr[s]) >> 6);
        const int32_t fa = frame_of[r];
        double4 qa = make_double4(0.0, 0.0, 0.0, 0.0);
        if (fa >= 0) qa = refl[fa];
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            const int32_t c = sell_col[e];
            if (c < 0) continue;
            const int32_t fb = frame_of[c];
            if (fa < 0 && fb < 0) continue;
            double B[BS][BS];
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) B[i][j] = val[(int64_t)(i * BS + j) * plane + e];
            if (fa >= 0) {                      // H_a B: every column reflected
#pragma unroll
                for (int j = 0; j < BS; ++j) {
                    double x[BS];
#pragma unroll
                    for (int i = 0; i < BS; ++i) x[i] = B[i][j];
                    ct_reflect<BS>(qa, x);
#pragma unroll
                    for (int i = 0; i < BS; ++i) B[i][j] = x[i];
                }
            }
            if (fb >= 0) {                      // B H_b: every row reflected
                const double4 qb = refl[fb];
#pragma unroll
                for (int i = 0; i < BS; ++i) ct_reflect<BS>(qb, B[i]);
            }
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) val[(int64_t)(i * BS + j) * plane + e] = B[i][j];
        }
    }
}

template <int BS>
__global__ void __launch_bounds__(FS_BLOCK) k_rotate_vector(int64_t n, const int32_t* __restrict__ node, const double4* __restrict__ refl,
                                                            double* __restrict__ x) {
    int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; f < n; f += stride) {
        double* xa = x + (int64_t)BS * node[f];
        double t[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) t[i] = xa[i];
        ct_reflect<BS>(refl[f], t);
#pragma unroll
        for (int i = 0; i < BS; ++i) xa[i] = t[i];
    }
}

// The grid covers the candidates once, whole waves (the ballots need every lane of a wave here together).
template <int BS>
__global__ void __launch_bounds__(FS_BLOCK) k_contact_update(int64_t n, const int32_t* __restrict__ node, const int64_t* __restrict__ slice_ptr,
                                                             const int32_t* __restrict__ sell_col, const double* __restrict__ val, int64_t plane,
                                                             const double* __restrict__ u, const double* __restrict__ b,
                                                             const double* __restrict__ sigma, const double* __restrict__ g,
                                                             const uint8_t* __restrict__ bilateral, int32_t* __restrict__ active,
                                                             double* __restrict__ lambda, double* __restrict__ pen, int32_t* __restrict__ tally,
                                                             int* __restrict__ host_counts) {
    __shared__ int lds[2][FS_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool changed = false, now = false;
    if (f < n) {
        const int64_t r = node[f];
        const int64_t sl = r >> 6;
        const int64_t base = slice_ptr[sl] + (r & 63);
        const int width = (int)((slice_ptr[sl + 1] - slice_ptr[sl]) >> 6);
        constexpr int K = BS - 1;
        double rho = 0.0;
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            const int32_t c = sell_col[e];
            if (c < 0) continue;
#pragma unroll
            for (int j = 0; j < BS; ++j) rho += val[(int64_t)(K * BS + j) * plane + e] * u[(int64_t)c * BS + j];
        }
        rho -= b[r * BS + K];
        const double sg = sigma[f];
        const double lam = -sg * rho;
        const double p = sg * u[r * BS + K] - g[f];
        const bool was = active[f] != 0;
        now = bilateral[f] ? true : (was ? lam > 0.0 : p > 0.0);
        changed = now != was;
        lambda[f] = lam;
        pen[f] = p;
        active[f] = now ? 1 : 0;
    }
    const int wave = threadIdx.x >> 6;
    const int nch = __popcll(__ballot(changed)), nac = __popcll(__ballot(now));
    if ((threadIdx.x & 63) == 0) {
        lds[0][wave] = nch;
        lds[1][wave] = nac;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int tc = 0, ta = 0;
#pragma unroll
        for (int w = 0; w < FS_BLOCK / 64; ++w) {
            tc += lds[0][w];
            ta += lds[1][w];
        }
        __hip_atomic_fetch_add(&tally[0], tc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&tally[1], ta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int through = __hip_atomic_fetch_add(&tally[2], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (through == (int)gridDim.x - 1) {     // the last workgroup: every other one added its share before it counted
            fs_host_store(&host_counts[0], __hip_atomic_load(&tally[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            fs_host_store(&host_counts[1], __hip_atomic_load(&tally[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
            for (int i = 0; i < 3; ++i) __hip_atomic_store(&tally[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static int ct_require_cg1_vector(const fs_space_s* sp, const char* who) {
    FS_REQUIRE(sp->family == FS_FAMILY_CG && sp->degree == 1 && (sp->ncomp == 2 || sp->ncomp == 3) && sp->ncomp == sp->mesh->tdim,
               "%s: built for vector CG1 spaces with 2 (triangles) or 3 (tetrahedra) components", who);
    FS_REQUIRE(!sp->halo.active, "%s: runs on one rank", who);
    return FS_OK;
}

extern "C" int fs_contact_create(fs_space_t space, int64_t n, const int32_t* nodes, const double* normals, const double* values,
                                 const int32_t* bilateral, const int32_t* active, fs_contact_t* out) {
    FS_REFUSE_DG_SPACE(space, "fs_contact_create");
    FS_CHECK(fs_require_init());
    FS_REQUIRE(space && out && n > 0 && nodes && normals && values && bilateral && active, "fs_contact_create: null pointer or empty node list");
    fs_space_s* sp = space;
    FS_CHECK(ct_require_cg1_vector(sp, "fs_contact_create"));
    const int bs = sp->ncomp, K = bs - 1;
    FS_REQUIRE(n <= sp->n_nodes_owned, "fs_contact_create: %lld nodes listed, the space has %lld", (long long)n, (long long)sp->n_nodes_owned);
    std::vector<int32_t> frame_of((size_t)sp->n_nodes_local, -1), act((size_t)n);
    std::vector<double> refl(4 * (size_t)n, 0.0), sigma((size_t)n);
    std::vector<uint8_t> bil((size_t)n);
    for (int64_t f = 0; f < n; ++f) {
        FS_REQUIRE(nodes[f] >= 0 && nodes[f] < sp->n_nodes_owned, "fs_contact_create: node %d outside [0,%lld)", nodes[f], (long long)sp->n_nodes_owned);
        FS_REQUIRE(f == 0 || nodes[f] > nodes[f - 1], "fs_contact_create: the node list must be strictly ascending (entry %lld)", (long long)f);
        double nn = 0.0;
        for (int i = 0; i < bs; ++i) nn += normals[bs * f + i] * normals[bs * f + i];
        FS_REQUIRE(isfinite(nn) && nn > 0.0, "fs_contact_create: node %d has a zero or non-finite normal", nodes[f]);
        FS_REQUIRE(isfinite(values[f]), "fs_contact_create: node %d has a non-finite value", nodes[f]);
        const double inv = 1.0 / sqrt(nn);
        double v[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < bs; ++i) v[i] = normals[bs * f + i] * inv;
        const double s = v[K] < 0.0 ? -1.0 : 1.0;
        v[K] += s;
        double vv = 0.0;
        for (int i = 0; i < bs; ++i) vv += v[i] * v[i];
        for (int i = 0; i < 3; ++i) refl[4 * f + i] = v[i];
        refl[4 * f + 3] = 2.0 / vv;
        sigma[f] = -s;
        bil[f] = bilateral[f] ? 1 : 0;
        act[f] = (bilateral[f] || active[f]) ? 1 : 0;
        frame_of[nodes[f]] = (int32_t)f;
    }
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    hipStream_t s = fs_rt().stream;
    fs_contact_s* c = new fs_contact_s;
    struct guard { fs_contact_s* c; ~guard() { delete c; } } gd{c};
    c->space = sp;
    c->bs = bs;
    c->n = n;
    FS_CHECK(c->node.alloc(n)); FS_CHECK(c->frame_of.alloc(sp->n_nodes_local)); FS_CHECK(c->v.alloc(4 * n)); FS_CHECK(c->sigma.alloc(n));
    FS_CHECK(c->g.alloc(n)); FS_CHECK(c->bilateral.alloc(n)); FS_CHECK(c->active.alloc(n)); FS_CHECK(c->lambda.alloc(n));
    FS_CHECK(c->pen.alloc(n)); FS_CHECK(c->tally.alloc(3));
    FS_CHECK(c->node.upload(nodes, n, s)); FS_CHECK(c->frame_of.upload(frame_of.data(), sp->n_nodes_local, s));
    FS_CHECK(c->v.upload(refl.data(), 4 * n, s)); FS_CHECK(c->sigma.upload(sigma.data(), n, s)); FS_CHECK(c->g.upload(values, n, s));
    FS_CHECK(c->bilateral.upload(bil.data(), n, s)); FS_CHECK(c->active.upload(act.data(), n, s));
    FS_CHECK(c->lambda.zero(s)); FS_CHECK(c->pen.zero(s)); FS_CHECK(c->tally.zero(s));
    FS_HIP(hipHostMalloc((void**)&c->h_counts, 4 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->h_counts, 0, 4 * sizeof(int));
    FS_HIP(hipHostGetDevicePointer((void**)&c->d_counts, c->h_counts, 0));
    FS_HIP(hipStreamSynchronize(s));
    gd.c = nullptr;
    *out = c;
    return FS_OK;
}

extern "C" int fs_contact_destroy(fs_contact_t c) {
    delete c;
    return FS_OK;
}

extern "C" int fs_contact_get(fs_contact_t c, int32_t* active, double* lambda, double* penetration) {
    FS_REQUIRE(c, "fs_contact_get: null state");
    hipStream_t s = fs_rt().stream;
    if (active) FS_CHECK(c->active.download(active, c->n, s));
    if (lambda) FS_CHECK(c->lambda.download(lambda, c->n, s));
    if (penetration) FS_CHECK(c->pen.download(penetration, c->n, s));
    return FS_OK;
}

extern "C" int fs_matrix_rotate_nodes(fs_matrix_t A, fs_contact_t frames) {
    FS_REFUSE_DG(A, "fs_matrix_rotate_nodes");
    FS_CHECK(fs_require_init());
    FS_REQUIRE(A && frames, "fs_matrix_rotate_nodes: null pointer");
    FS_REQUIRE(A->space == frames->space && A->bs == frames->bs && !A->taylor_hood, "fs_matrix_rotate_nodes: the matrix is not on the frames' space");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    fs_space_s* sp = A->space;
    hipStream_t s = fs_rt().stream;
    fs_dispatch_int<2, 3>(A->bs, [&](auto BS) {
        hipLaunchKernelGGL(k_rotate_matrix<decltype(BS)::value>, dim3(fs_grid_for(sp->n_slices * 64, FS_BLOCK, 8192)), dim3(FS_BLOCK), 0, s,
                           sp->n_nodes_owned, sp->n_slices, sp->slice_ptr.p, sp->sell_col.p, A->val.p, sp->sell_entries, frames->frame_of.p,
                           reinterpret_cast<const double4*>(frames->v.p));
    });
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_vector_rotate_nodes(fs_vector_t x, fs_contact_t frames) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(x && frames, "fs_vector_rotate_nodes: null pointer");
    FS_REQUIRE(x->d.n >= frames->space->n_dofs_owned, "fs_vector_rotate_nodes: the vector has %lld entries, the space %lld owned dofs", (long long)x->d.n,
               (long long)frames->space->n_dofs_owned);
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    hipStream_t s = fs_rt().stream;
    fs_dispatch_int<2, 3>(frames->bs, [&](auto BS) {
        hipLaunchKernelGGL(k_rotate_vector<decltype(BS)::value>, dim3(fs_grid_for(frames->n)), dim3(FS_BLOCK), 0, s, frames->n, frames->node.p,
                           reinterpret_cast<const double4*>(frames->v.p), x->d.p);
    });
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_contact_update(fs_contact_t state, fs_matrix_t Kprime, fs_vector_t uprime, fs_vector_t bprime, int32_t* counts) {
    FS_REFUSE_DG(Kprime, "fs_contact_update");
    FS_CHECK(fs_require_init());
    FS_REQUIRE(state && Kprime && uprime && bprime && counts, "fs_contact_update: null pointer");
    fs_space_s* sp = state->space;
    FS_REQUIRE(Kprime->space == sp && Kprime->bs == state->bs && !Kprime->taylor_hood, "fs_contact_update: the matrix is not on the state's space");
    FS_REQUIRE(uprime->d.n >= sp->n_dofs_local, "fs_contact_update: u' has %lld entries, the space %lld dofs", (long long)uprime->d.n, (long long)sp->n_dofs_local);
    FS_REQUIRE(bprime->d.n >= sp->n_dofs_owned, "fs_contact_update: b' has %lld entries, the space %lld owned dofs", (long long)bprime->d.n,
               (long long)sp->n_dofs_owned);
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    hipStream_t s = fs_rt().stream;
    const int grid = (int)((state->n + FS_BLOCK - 1) / FS_BLOCK);
    fs_dispatch_int<2, 3>(state->bs, [&](auto BS) {
        hipLaunchKernelGGL(k_contact_update<decltype(BS)::value>, dim3(grid), dim3(FS_BLOCK), 0, s, state->n, state->node.p, sp->slice_ptr.p, sp->sell_col.p,
                           Kprime->val.p, sp->sell_entries, uprime->d.p, bprime->d.p, state->sigma.p, state->g.p, state->bilateral.p, state->active.p,
                           state->lambda.p, state->pen.p, state->tally.p, state->d_counts);
    });
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    counts[0] = state->h_counts[0];
    counts[1] = state->h_counts[1];
    return FS_OK;
}
