// Discontinuous P1 (DG1) scalar spaces: cell-block storage, upwind SIPG advection-diffusion assembly, the block product,
// BiCGStab with block-Jacobi and the right-hand side of the L2 projection onto CG1 (ScalarTransportDGSolver.py).
//
// A DG1 operator couples a cell only with itself and with the d+1 cells across its facets, so its structure is fixed by the
// cell-facet adjacency: no symbolic phase, no sparsity pattern.  Dof (K, a) = (d+1) K + a in device cell order.
//
// Storage (fs_matrix_s::val of a DG matrix): (d+2) slots of (d+1) x (d+1) blocks per cell, slot 0 the diagonal block, slot k+1
// the block that couples with the neighbour across facet k (the facet opposite local vertex k).  Entry (slot s, row a, column b)
// of cell K lives at ((s (d+1) + a) (d+1) + b) * nc + K: the cell index runs fastest, so the 64 lanes of a wave (64 consecutive
// cells) load 512 contiguous bytes per entry.  Slots of boundary facets hold zeros and are never read by the product.
//
// Every kernel here gives one work item one cell (and writes only that cell's rows): no atomics, the same bits on every run.
#include "fs_common.h"
#include "fs_p1_geometry.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>

namespace {

constexpr int DG_GRID_MAX = 1024;   // workgroups of the reducing kernels: partial sums [n_sums][DG_GRID_MAX], summed in a fixed order

// ---- geometry ------------------------------------------------------------------------------------------------------------
// gradients of the barycentric basis (3-vectors; z = 0 on triangles), measure, h = 2 circumradius (fs_assemble.hip's h)
template <int D>
struct dg_cell {
    int32_t v[D + 1];
    double g[D + 1][3];
    double vol;
    double h;
};

template <int D>
__device__ __forceinline__ void dg_load_cell(const int32_t* __restrict__ cells, const double* __restrict__ xyz4, int64_t K,
                                             dg_cell<D>& c) {
    const int4 cv = reinterpret_cast<const int4*>(cells)[K];
    c.v[0] = cv.x; c.v[1] = cv.y; c.v[2] = cv.z;
    if constexpr (D == 3) {
        c.v[3] = cv.w;
        const int32_t vv[4] = {cv.x, cv.y, cv.z, cv.w};
        const tet_geom t = tet_geometry(xyz4, vv);
        for (int a = 0; a < 4; ++a)
            for (int d = 0; d < 3; ++d) c.g[a][d] = t.g[a][d];
        c.vol = t.adet / 6.0;
        double x[4][3];
        for (int a = 0; a < 4; ++a) load_vertex(xyz4, vv[a], x[a]);
        auto dist = [&](int p, int q) {
            return sqrt((x[p][0] - x[q][0]) * (x[p][0] - x[q][0]) + (x[p][1] - x[q][1]) * (x[p][1] - x[q][1]) +
                        (x[p][2] - x[q][2]) * (x[p][2] - x[q][2]));
        };
        const double aA = dist(0, 1) * dist(2, 3), bB = dist(0, 2) * dist(1, 3), cC = dist(0, 3) * dist(1, 2);
        const double prod = (aA + bB + cC) * (aA + bB - cC) * (aA - bB + cC) * (-aA + bB + cC);
        c.h = 2.0 * sqrt(prod > 0.0 ? prod : 0.0) / (4.0 * t.adet);
    } else {
        const tri_geom t = tri_geometry2(xyz4, cv.x, cv.y, cv.z);
        for (int a = 0; a < 3; ++a) { c.g[a][0] = t.g[a][0]; c.g[a][1] = t.g[a][1]; c.g[a][2] = 0.0; }
        c.vol = t.area;
        double x[3][2];
        for (int a = 0; a < 3; ++a) { x[a][0] = xyz4[4 * (int64_t)c.v[a]]; x[a][1] = xyz4[4 * (int64_t)c.v[a] + 1]; }
        auto dist = [&](int p, int q) { return sqrt((x[p][0] - x[q][0]) * (x[p][0] - x[q][0]) + (x[p][1] - x[q][1]) * (x[p][1] - x[q][1])); };
        c.h = dist(0, 1) * dist(1, 2) * dist(2, 0) / (2.0 * t.area);
    }
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

struct dg_form_dev {
    double k;          // conductivity = capacity * diffusivity
    double c;          // capacity
    double beta[3];
    double alpha;
    double op;         // coefficient of c a(T, v)
    double mass;       // coefficient of int T v dx
};

// One work item per cell K writes its block row: slot 0 (cell term, its own side of the d+1 facet terms, outflow, HTC facet mass,
// mass term) and slot k+1 (the cross terms with neighbour k), and optionally its d+1 entries of b (body source, facet loads).
// fcell_ptr / f_local / f_h / f_g: the listed boundary facets of every cell (CSR by cell, ascending local facet).
template <int D>
__global__ void __launch_bounds__(FS_BLOCK) k_dg_assemble(int64_t nc, const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                          const int32_t* __restrict__ nbr, const uint8_t* __restrict__ plus, dg_form_dev F,
                                                          const int32_t* __restrict__ fcell_ptr, const int32_t* __restrict__ f_local,
                                                          const double* __restrict__ f_h, const double* __restrict__ f_g,
                                                          const double* __restrict__ source, int add, double* __restrict__ val,
                                                          double* __restrict__ b) {
    constexpr int L = D + 1;
    const int64_t K = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (K >= nc) return;
    dg_cell<D> C;
    dg_load_cell<D>(cells, xyz4, K, C);
    double Ad[L][L];
    double bl[L];
    // cell term: k vol g_a.g_b - c (vol / (d+1)) beta.g_a, mass (vol / ((d+1)(d+2))) (1 + delta_ab)
    const double mK = C.vol / (double)(L * (L + 1));
    for (int a = 0; a < L; ++a) {
        const double adv = F.c * (C.vol / (double)L) * dot3(F.beta, C.g[a]);
        for (int b2 = 0; b2 < L; ++b2)
            Ad[a][b2] = F.op * (F.k * C.vol * dot3(C.g[a], C.g[b2]) - adv) + F.mass * mK * (a == b2 ? 2.0 : 1.0);
        bl[a] = 0.0;
    }
    if (source) {
        double f[L], fs = 0.0;
        for (int a = 0; a < L; ++a) { f[a] = source[K * L + a]; fs += f[a]; }
        for (int a = 0; a < L; ++a) bl[a] += mK * (fs + f[a]);
    }
    const uint8_t pl = plus[K];
    for (int k = 0; k < L; ++k) {
        const double gn = sqrt(dot3(C.g[k], C.g[k]));
        double n[3] = {-C.g[k][0] / gn, -C.g[k][1] / gn, -C.g[k][2] / gn};
        const double area = (double)D * C.vol * gn;
        const double mf = area / (double)(D * L);          // int_F phi_a phi_b = mf (1 + delta_ab) on the facet's vertices
        const double If = area / (double)D;                // int_F phi_a
        const double bn = dot3(F.beta, n);
        const double bout = bn > 0.0 ? bn : 0.0, bin = bn < 0.0 ? -bn : 0.0;
        const int32_t N = nbr[(int64_t)k * nc + K];
        double* vs = val + (int64_t)(k + 1) * L * L * nc + K;
        if (N < 0) {
            for (int a = 0; a < L; ++a)
                for (int b2 = 0; b2 < L; ++b2) {
                    if (a != k && b2 != k) Ad[a][b2] += F.op * F.c * bout * mf * (a == b2 ? 2.0 : 1.0);
                    if (!add) vs[(int64_t)(a * L + b2) * nc] = 0.0;
                }
            continue;
        }
        dg_cell<D> Nc;
        dg_load_cell<D>(cells, xyz4, N, Nc);
        const double hp = ((pl >> k) & 1) ? C.h : Nc.h;
        const double pen = F.k * F.alpha / hp;
        double gan[L], gbn[L];
        for (int a = 0; a < L; ++a) { gan[a] = dot3(C.g[a], n); gbn[a] = dot3(Nc.g[a], n); }
        for (int a = 0; a < L; ++a)
            for (int b2 = 0; b2 < L; ++b2) {
                const double Ia = a != k ? If : 0.0, Ib = b2 != k ? If : 0.0;
                const double mab = (a != k && b2 != k) ? mf * (a == b2 ? 2.0 : 1.0) : 0.0;
                Ad[a][b2] += F.op * ((pen + F.c * bout) * mab - 0.5 * F.k * (gan[a] * Ib + gan[b2] * Ia));
            }
        // the neighbour's local vertex c lies on the facet unless it is its vertex opposite; it matches K's vertex of the same id
        for (int a = 0; a < L; ++a) {
            const double Ia = a != k ? If : 0.0;
            for (int c2 = 0; c2 < L; ++c2) {
                bool on = false;
                for (int e = 0; e < L; ++e) on |= (e != k && C.v[e] == Nc.v[c2]);
                const double Ic = on ? If : 0.0;
                const double mac = (a != k && on) ? mf * (C.v[a] == Nc.v[c2] ? 2.0 : 1.0) : 0.0;
                const double v = F.op * (-(pen + F.c * bin) * mac + 0.5 * F.k * (gan[a] * Ic - gbn[c2] * Ia));
                double* e = vs + (int64_t)(a * L + c2) * nc;
                *e = add ? *e + v : v;
            }
        }
    }
    // listed boundary facets: HTC facet mass (h) and loads (g at the cell's vertices: int_F g phi_a = sum_b M_F[a][b] g_b)
    if (fcell_ptr) {
        for (int32_t i = fcell_ptr[K]; i < fcell_ptr[K + 1]; ++i) {
            const int k = f_local[i];
            const double gn = sqrt(dot3(C.g[k], C.g[k]));
            const double mf = (double)D * C.vol * gn / (double)(D * L);
            const double h = f_h ? f_h[i] : 0.0;
            double gs = 0.0;
            if (f_g)
                for (int e = 0; e < L; ++e) gs += e != k ? f_g[(int64_t)i * L + e] : 0.0;
            for (int a = 0; a < L; ++a) {
                if (a == k) continue;
                for (int b2 = 0; b2 < L; ++b2)
                    if (b2 != k) Ad[a][b2] += h * mf * (a == b2 ? 2.0 : 1.0);
                if (f_g) bl[a] += mf * (gs + f_g[(int64_t)i * L + a]);
            }
        }
    }
    for (int a = 0; a < L; ++a)
        for (int b2 = 0; b2 < L; ++b2) {
            double* e = val + (int64_t)(a * L + b2) * nc + K;
            *e = add ? *e + Ad[a][b2] : Ad[a][b2];
        }
    if (b)
        for (int a = 0; a < L; ++a) b[K * L + a] = add ? b[K * L + a] + bl[a] : bl[a];
}

// ---- block reductions (fixed grid, fixed order: deterministic) ------------------------------------------------------------
static_assert(FS_BLOCK / FS_WAVE == 4, "dg_block_sums adds the partial sums of four waves");
template <int NS>
__device__ __forceinline__ void dg_block_sums(double (&v)[NS], double* __restrict__ partials) {
    __shared__ double red[NS][FS_BLOCK / FS_WAVE];
#pragma unroll
    for (int s = 0; s < NS; ++s)
        for (int off = FS_WAVE / 2; off > 0; off >>= 1) v[s] += __shfl_down(v[s], off, FS_WAVE);
    const int lane = threadIdx.x & (FS_WAVE - 1), w = threadIdx.x / FS_WAVE;
    if (lane == 0)
        for (int s = 0; s < NS; ++s) red[s][w] = v[s];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int s = 0; s < NS; ++s) partials[s * DG_GRID_MAX + blockIdx.x] = ((red[s][0] + red[s][1]) + red[s][2]) + red[s][3];
}

// y_K = sum over slots of A_{K,s} x_{nbr(K,s)} for the cells [0, nc) (grid-stride); NDOT fused sums: dot(u, y) and/or dot(y, y)
template <int D, bool DOT_U, bool DOT_Y>
__global__ void __launch_bounds__(FS_BLOCK) k_dg_spmv(int64_t nc, const double* __restrict__ val, const int32_t* __restrict__ nbr,
                                                      const double* __restrict__ x, double* __restrict__ y, const double* __restrict__ u,
                                                      double* __restrict__ partials, const int* __restrict__ done) {
    constexpr int L = D + 1;
    constexpr int NS = (DOT_U ? 1 : 0) + (DOT_Y ? 1 : 0);
    if (done && *done) return;
    double sums[NS > 0 ? NS : 1] = {};
    for (int64_t K = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; K < nc; K += (int64_t)gridDim.x * blockDim.x) {
        double acc[L];
        double xs[L];
        for (int b = 0; b < L; ++b) xs[b] = x[K * L + b];
        for (int a = 0; a < L; ++a) {
            double t = 0.0;
            for (int b = 0; b < L; ++b) t += val[(int64_t)(a * L + b) * nc + K] * xs[b];
            acc[a] = t;
        }
        for (int k = 0; k < L; ++k) {
            const int32_t N = nbr[(int64_t)k * nc + K];
            if (N < 0) continue;
            for (int b = 0; b < L; ++b) xs[b] = x[(int64_t)N * L + b];
            const double* vs = val + (int64_t)(k + 1) * L * L * nc + K;
            for (int a = 0; a < L; ++a) {
                double t = 0.0;
                for (int b = 0; b < L; ++b) t += vs[(int64_t)(a * L + b) * nc] * xs[b];
                acc[a] += t;
            }
        }
        for (int a = 0; a < L; ++a) {
            y[K * L + a] = acc[a];
            if constexpr (DOT_U) sums[0] += u[K * L + a] * acc[a];
            if constexpr (DOT_Y) sums[NS - 1] += acc[a] * acc[a];
        }
    }
    if constexpr (NS > 0) {
        double v[NS];
        for (int s = 0; s < NS; ++s) v[s] = sums[s];
        dg_block_sums<NS>(v, partials);
    }
}

// ---- BiCGStab state (device) ------------------------------------------------------------------------------------------------
struct dg_state {
    double rho, alpha, omega, beta;
    double rr, bb, tol2;
    double rrp, bbp, tol2p;  // the same in the preconditioned norm (||M^-1 r||, pnorm only)
    double last[5];  // the sums of the last finalisation (diagnostics)
    int done;        // 1: converged, 2: breakdown
    int iter;
};

// sum of the partials of `nblocks` workgroups in a fixed order (one workgroup): out[s] for s < ns
__device__ __forceinline__ void dg_sum_partials(const double* __restrict__ partials, int nblocks, int ns, double* out) {
    __shared__ double sh[FS_BLOCK];
    for (int s = 0; s < ns; ++s) {
        double t = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += FS_BLOCK) t += partials[s * DG_GRID_MAX + i];
        sh[threadIdx.x] = t;
        __syncthreads();
        for (int w = FS_BLOCK / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[s] = sh[0];
        __syncthreads();
    }
}

__device__ __forceinline__ bool dg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and inf

// which: 0 start (rho = rhat.r = r.r, bb), 1 alpha, 2 omega, 3 rho / beta / residual
__global__ void k_dg_finalize(dg_state* st, const double* __restrict__ partials, int nblocks, int which, double* __restrict__ hist,
                              double rtol2, double atol2) {
    if (which != 0 && st->done) return;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    dg_sum_partials(partials, nblocks, which == 1 ? 1 : which == 0 ? 5 : which == 2 ? 2 : 3, s);
    if (threadIdx.x != 0) return;
    for (int i = 0; i < 5; ++i) st->last[i] = s[i];
    if (which == 0) {
        st->rho = s[0];
        st->rr = s[2];
        st->bb = s[1];
        st->tol2 = fmax(rtol2 * s[1], atol2);
        st->rrp = s[4];
        st->bbp = s[3];
        st->tol2p = fmax(rtol2 * s[3], atol2);
        st->iter = 0;
        st->omega = 1.0;
        st->done = (s[2] <= st->tol2 && s[4] <= st->tol2p) ? 1 : 0;
        if (hist) hist[0] = s[2];
    } else if (which == 1) {
        const double a = st->rho / s[0];
        if (!(s[0] != 0.0) || !dg_finite(a)) { st->done = 2; return; }
        st->alpha = a;
    } else if (which == 2) {
        // t = A M^-1 s = 0: s is already the residual; omega = 0 makes the next beta infinite (breakdown) unless it converged
        st->omega = s[1] != 0.0 ? s[0] / s[1] : 0.0;
        if (!dg_finite(st->omega)) st->done = 2;
    } else {
        st->iter += 1;
        st->rr = s[1];
        st->rrp = s[2];
        if (hist) hist[st->iter] = s[1];
        if (s[1] <= st->tol2 && s[2] <= st->tol2p) { st->done = 1; return; }
        const double beta = (s[0] / st->rho) * (st->alpha / st->omega);
        if (!(s[0] != 0.0) || !(st->omega != 0.0) || !dg_finite(beta) || !dg_finite(s[1])) { st->done = 2; return; }
        st->beta = beta;
        st->rho = s[0];
    }
}

// z_K = M_K^-1 w_K (Minv in the layout of one block slot)
template <int L>
__device__ __forceinline__ void dg_apply_minv(const double* __restrict__ minv, int64_t nc, int64_t K, const double (&w)[L], double (&z)[L]) {
    for (int a = 0; a < L; ++a) {
        double t = 0.0;
        for (int b = 0; b < L; ++b) t += minv[(int64_t)(a * L + b) * nc + K] * w[b];
        z[a] = t;
    }
}

// The stopping test measures ||r||_2 and, with pnorm (FS_NORM_PRECONDITIONED), also ||M^-1 r||_2 (both must pass; without pnorm the
// second pair of sums is zero)
// mode 0: start   r = b - y (y = A x, or b when x0 = 0), rhat = r, p = r, phat = M^-1 r; sums rhat.r, b.b, r.r, |M^-1 b|^2, |M^-1 r|^2
// mode 1: s = r - alpha v, shat = M^-1 s                       (s stored in r)
// mode 2: x += alpha phat + omega shat, r = s - omega t; sums rhat.r, r.r, |M^-1 r|^2
// mode 3: p = r + beta (p - omega v), phat = M^-1 p
template <int D>
__global__ void __launch_bounds__(FS_BLOCK) k_dg_update(int mode, int64_t nc, const double* __restrict__ minv, dg_state* st,
                                                        double* __restrict__ x, double* __restrict__ r, double* __restrict__ rhat,
                                                        double* __restrict__ p, double* __restrict__ phat, double* __restrict__ v,
                                                        double* __restrict__ shat, const double* __restrict__ t, const double* __restrict__ b,
                                                        const double* __restrict__ y, double* __restrict__ partials, int pnorm) {
    constexpr int L = D + 1;
    if (mode != 0 && st->done) return;
    const double alpha = st->alpha, omega = st->omega, beta = st->beta;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int64_t K = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; K < nc; K += (int64_t)gridDim.x * blockDim.x) {
        double w[L], z[L];
        const int64_t o = K * L;
        if (mode == 0) {
            double bl[L], zb[L];
            for (int a = 0; a < L; ++a) {
                bl[a] = b[o + a];
                w[a] = y ? bl[a] - y[o + a] : bl[a];
                r[o + a] = w[a]; rhat[o + a] = w[a]; p[o + a] = w[a];
                s0 += w[a] * w[a];
            }
            dg_apply_minv<L>(minv, nc, K, w, z);
            if (pnorm) dg_apply_minv<L>(minv, nc, K, bl, zb);
            for (int a = 0; a < L; ++a) {
                phat[o + a] = z[a];
                s1 += bl[a] * bl[a];
                s2 += w[a] * w[a];
                if (pnorm) { s3 += zb[a] * zb[a]; s4 += z[a] * z[a]; }
            }
        } else if (mode == 1) {
            for (int a = 0; a < L; ++a) { w[a] = r[o + a] - alpha * v[o + a]; r[o + a] = w[a]; }
            dg_apply_minv<L>(minv, nc, K, w, z);
            for (int a = 0; a < L; ++a) shat[o + a] = z[a];
        } else if (mode == 2) {
            for (int a = 0; a < L; ++a) {
                x[o + a] += alpha * phat[o + a] + omega * shat[o + a];
                w[a] = r[o + a] - omega * t[o + a];
                r[o + a] = w[a];
                s0 += rhat[o + a] * w[a];
            }
            if (pnorm) dg_apply_minv<L>(minv, nc, K, w, z);
            for (int a = 0; a < L; ++a) {
                s1 += w[a] * w[a];
                if (pnorm) s2 += z[a] * z[a];
            }
        } else {
            for (int a = 0; a < L; ++a) { w[a] = r[o + a] + beta * (p[o + a] - omega * v[o + a]); p[o + a] = w[a]; }
            dg_apply_minv<L>(minv, nc, K, w, z);
            for (int a = 0; a < L; ++a) phat[o + a] = z[a];
        }
    }
    if (mode == 0 || mode == 2) {
        double vv[5] = {s0, s1, s2, s3, s4};
        dg_block_sums<5>(vv, partials);
    }
}

// block Jacobi: the inverse of every diagonal block (Gauss-Jordan with partial pivoting, fp64); point Jacobi: 1 / the diagonal;
// none: identity.  A zero pivot leaves a zero block row (the solve then breaks down and says so).
template <int D>
__global__ void __launch_bounds__(FS_BLOCK) k_dg_precond(int64_t nc, const double* __restrict__ val, int pc, double* __restrict__ minv,
                                                         int* __restrict__ singular) {
    constexpr int L = D + 1;
    const int64_t K = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (K >= nc) return;
    double M[L][L], I[L][L];
    for (int a = 0; a < L; ++a)
        for (int b = 0; b < L; ++b) { M[a][b] = val[(int64_t)(a * L + b) * nc + K]; I[a][b] = a == b ? 1.0 : 0.0; }
    if (pc == 2) {
        for (int c = 0; c < L; ++c) {
            int piv = c;
            for (int r = c + 1; r < L; ++r)
                if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
            if (M[piv][c] == 0.0) { *singular = 1; for (int a = 0; a < L; ++a) for (int b = 0; b < L; ++b) I[a][b] = 0.0; break; }
            if (piv != c)
                for (int b = 0; b < L; ++b) {
                    double t = M[c][b]; M[c][b] = M[piv][b]; M[piv][b] = t;
                    t = I[c][b]; I[c][b] = I[piv][b]; I[piv][b] = t;
                }
            const double inv = 1.0 / M[c][c];
            for (int b = 0; b < L; ++b) { M[c][b] *= inv; I[c][b] *= inv; }
            for (int r = 0; r < L; ++r) {
                if (r == c) continue;
                const double f = M[r][c];
                for (int b = 0; b < L; ++b) { M[r][b] -= f * M[c][b]; I[r][b] -= f * I[c][b]; }
            }
        }
    } else if (pc == 1) {
        for (int a = 0; a < L; ++a) {
            if (M[a][a] == 0.0) *singular = 1;
            I[a][a] = M[a][a] != 0.0 ? 1.0 / M[a][a] : 0.0;
        }
    }
    for (int a = 0; a < L; ++a)
        for (int b = 0; b < L; ++b) minv[(int64_t)(a * L + b) * nc + K] = I[a][b];
}

// Dirichlet rows -> identity rows, b_i = g (one work item per listed dof; the host list holds each dof once)
template <int D>
__global__ void k_dg_dirichlet(int64_t n, const int32_t* __restrict__ dofs, const double* __restrict__ g, int64_t nc, double* __restrict__ val,
                               double* __restrict__ b) {
    constexpr int L = D + 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t dof = dofs[i], K = dof / L;
    const int a = (int)(dof % L);
    if (val)
        for (int s = 0; s < L + 1; ++s)
            for (int c = 0; c < L; ++c) val[((int64_t)(s * L + a) * L + c) * nc + K] = (s == 0 && c == a) ? 1.0 : 0.0;
    if (b) b[dof] = g[i];
}

// ||w||^2 and (pnorm) ||M^-1 w||^2 partials of w = b - y
template <int D>
__global__ void __launch_bounds__(FS_BLOCK) k_dg_resid(int64_t nc, const double* __restrict__ minv, int pnorm, const double* __restrict__ b,
                                                       const double* __restrict__ y, double* __restrict__ partials) {
    constexpr int L = D + 1;
    double s = 0.0, sp = 0.0;
    for (int64_t K = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; K < nc; K += (int64_t)gridDim.x * blockDim.x) {
        double w[L], z[L];
        for (int a = 0; a < L; ++a) w[a] = b[K * L + a] - y[K * L + a];
        if (pnorm) dg_apply_minv<L>(minv, nc, K, w, z);
        for (int a = 0; a < L; ++a) {
            s += w[a] * w[a];
            if (pnorm) sp += z[a] * z[a];
        }
    }
    double v[2] = {s, sp};
    dg_block_sums<2>(v, partials);
}

__global__ void k_dg_sum(const double* __restrict__ partials, int nblocks, int ns, double* __restrict__ out) {
    double s[5];
    dg_sum_partials(partials, nblocks, ns, s);
    if (threadIdx.x == 0)
        for (int i = 0; i < ns; ++i) out[i] = s[i];
}

// b_i = sum over the cells around vertex i, ascending, of (M_K T_K)_a with a = i's local index: vol / ((d+1)(d+2)) (sum T_K + T_Ka)
template <int D>
__global__ void __launch_bounds__(FS_BLOCK) k_dg_projection(int64_t nv, const int32_t* __restrict__ vptr, const int32_t* __restrict__ vinc,
                                                            const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                            const double* __restrict__ T, double* __restrict__ b) {
    constexpr int L = D + 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    double acc = 0.0;
    for (int32_t j = vptr[i]; j < vptr[i + 1]; ++j) {
        const int64_t K = vinc[j] >> 2;
        const int a = vinc[j] & 3;
        dg_cell<D> C;
        dg_load_cell<D>(cells, xyz4, K, C);
        double s = 0.0;
        for (int e = 0; e < L; ++e) s += T[K * L + e];
        acc += C.vol / (double)(L * (L + 1)) * (s + T[K * L + a]);
    }
    b[i] = acc;
}

int dg_dim(const fs_space_s* sp) { return sp->mesh->tdim; }

int dg_grid(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + FS_BLOCK - 1) / FS_BLOCK, DG_GRID_MAX)); }

// '+' flags from one key per cell: on every interior facet '+' is the cell with the larger key
void dg_plus_from_keys(fs_space_s* sp, const std::vector<int64_t>& key, std::vector<uint8_t>& plus) {
    const int64_t nc = sp->mesh->nc;
    const int L = dg_dim(sp) + 1;
    plus.assign(nc, 0);
    for (int64_t K = 0; K < nc; ++K)
        for (int k = 0; k < L; ++k) {
            const int32_t N = sp->dg_nbr_host[k * nc + K];
            if (N >= 0 && key[K] > key[N]) plus[K] |= (uint8_t)(1u << k);
        }
}

}  // namespace

// ---- space ------------------------------------------------------------------------------------------------------------------
int fs_dg_space_create(fs_mesh_s* mesh, int degree, int ncomp, fs_space_t* out) {
    if (degree != 1 || ncomp != 1) {
        fs_set_error("fs_space_create: DG spaces are scalar and of degree 1 (degree=%d ncomp=%d)", degree, ncomp);
        return FS_ERR_UNSUPPORTED;
    }
    FS_REQUIRE(mesh->n_owned == mesh->nv, "fs_space_create: DG spaces run on one rank (the mesh has ghost vertices)");
    hipStream_t s = fs_rt().stream;
    const int D = mesh->tdim, L = D + 1;
    const int64_t nc = mesh->nc, nv = mesh->nv;
    FS_REQUIRE(nc > 0 && (int64_t)L * nc < (int64_t)INT32_MAX, "fs_space_create: %lld cells do not fit a DG space", (long long)nc);
    std::vector<int32_t> cells((size_t)nc * 4);
    FS_CHECK(mesh->cells.download(cells.data(), nc * 4, s));
    // facets as sorted vertex tuples, bucketed by their smallest vertex, matched inside each bucket
    std::vector<int32_t> cnt(nv + 1, 0);
    auto facet = [&](int64_t K, int k, int32_t (&f)[3]) {
        int m = 0;
        for (int e = 0; e < L; ++e)
            if (e != k) f[m++] = cells[K * 4 + e];
        if (D == 2) f[2] = -1;
        std::sort(f, f + D);
    };
    for (int64_t K = 0; K < nc; ++K)
        for (int k = 0; k < L; ++k) {
            int32_t f[3];
            facet(K, k, f);
            FS_REQUIRE(f[0] >= 0 && f[D - 1] < nv, "fs_space_create: cell %lld names a vertex outside the mesh", (long long)K);
            cnt[f[0] + 1]++;
        }
    for (int64_t i = 0; i < nv; ++i) cnt[i + 1] += cnt[i];
    std::vector<int64_t> ent((size_t)nc * L);
    {
        std::vector<int32_t> pos(cnt.begin(), cnt.end() - 1);
        for (int64_t K = 0; K < nc; ++K)
            for (int k = 0; k < L; ++k) {
                int32_t f[3];
                facet(K, k, f);
                ent[pos[f[0]]++] = K * L + k;
            }
    }
    fs_space_s* sp = new fs_space_s();
    sp->mesh = mesh;
    sp->family = FS_FAMILY_DG;
    sp->degree = 1;
    sp->ncomp = 1;
    sp->ndof_cell = L;
    sp->dg_nbr_host.assign((size_t)L * nc, -1);
    int64_t bad = -1;
    for (int64_t i = 0; i < nv && bad < 0; ++i) {
        const int64_t b0 = cnt[i], b1 = cnt[i + 1];
        std::vector<std::pair<int64_t, int64_t>> keyed;
        keyed.reserve(b1 - b0);
        for (int64_t j = b0; j < b1; ++j) {
            int32_t f[3];
            facet(ent[j] / L, (int)(ent[j] % L), f);
            keyed.emplace_back(((int64_t)f[1] << 32) | (uint32_t)(f[2] + 1), ent[j]);
        }
        std::sort(keyed.begin(), keyed.end());
        for (size_t j = 0; j < keyed.size();) {
            size_t e = j + 1;
            while (e < keyed.size() && keyed[e].first == keyed[j].first) ++e;
            if (e - j > 2) { bad = keyed[j].second / L; break; }
            if (e - j == 2) {
                const int64_t p = keyed[j].second, q = keyed[j + 1].second;
                sp->dg_nbr_host[(p % L) * nc + p / L] = (int32_t)(q / L);
                sp->dg_nbr_host[(q % L) * nc + q / L] = (int32_t)(p / L);
            }
            j = e;
        }
    }
    if (bad >= 0) {
        delete sp;
        fs_set_error("fs_space_create: a facet of cell %lld is shared by more than two cells", (long long)bad);
        return FS_ERR_INVALID;
    }
    for (int64_t i = 0; i < (int64_t)L * nc; ++i) sp->dg_interior_sides += sp->dg_nbr_host[i] >= 0;
    // vertex -> (cell, local vertex) incidences, ascending by cell: the gather of the projection's right-hand side
    std::vector<int32_t> vptr(nv + 1, 0), vinc((size_t)nc * L);
    for (int64_t K = 0; K < nc; ++K)
        for (int a = 0; a < L; ++a) vptr[cells[K * 4 + a] + 1]++;
    for (int64_t i = 0; i < nv; ++i) vptr[i + 1] += vptr[i];
    {
        std::vector<int32_t> pos(vptr.begin(), vptr.end() - 1);
        for (int64_t K = 0; K < nc; ++K)
            for (int a = 0; a < L; ++a) vinc[pos[cells[K * 4 + a]]++] = (int32_t)(K * 4 + a);
    }
    std::vector<int64_t> key(nc);
    for (int64_t K = 0; K < nc; ++K) key[K] = -(int64_t)(mesh->cell_order.empty() ? K : mesh->cell_order[K]);
    std::vector<uint8_t> plus;
    dg_plus_from_keys(sp, key, plus);
    sp->n_nodes_local = sp->n_nodes_owned = sp->n_dofs_local = sp->n_dofs_owned = (int64_t)L * nc;
    int rc = sp->dg_nbr.alloc((int64_t)L * nc);
    if (rc == FS_OK) rc = sp->dg_nbr.upload(sp->dg_nbr_host.data(), (int64_t)L * nc, s);
    if (rc == FS_OK) rc = sp->dg_plus.alloc(nc);
    if (rc == FS_OK) rc = sp->dg_plus.upload(plus.data(), nc, s);
    if (rc == FS_OK) rc = sp->dg_vptr.alloc(nv + 1);
    if (rc == FS_OK) rc = sp->dg_vptr.upload(vptr.data(), nv + 1, s);
    if (rc == FS_OK) rc = sp->dg_vinc.alloc((int64_t)L * nc);
    if (rc == FS_OK) rc = sp->dg_vinc.upload(vinc.data(), (int64_t)L * nc, s);
    if (rc != FS_OK) {
        delete sp;
        return rc;
    }
    *out = sp;
    return FS_OK;
}

extern "C" int fs_space_dg_set_plus_key(fs_space_t space, const int64_t* key) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(space && key, "fs_space_dg_set_plus_key: null pointer");
    if (space->family != FS_FAMILY_DG) {
        fs_set_error("fs_space_dg_set_plus_key: not a DG space");
        return FS_ERR_UNSUPPORTED;
    }
    const int64_t nc = space->mesh->nc;
    std::vector<int64_t> k(key, key + nc);
    std::vector<uint8_t> plus;
    dg_plus_from_keys(space, k, plus);
    return space->dg_plus.upload(plus.data(), nc, fs_rt().stream);
}

// ---- matrix -----------------------------------------------------------------------------------------------------------------
int fs_dg_matrix_create(fs_space_s* space, fs_matrix_t* out) {
    const int L = dg_dim(space) + 1;
    fs_matrix_s* A = new fs_matrix_s();
    A->space = space;
    A->bs = 1;
    int rc = A->val.alloc((int64_t)(L + 1) * L * L * space->mesh->nc);
    if (rc == FS_OK) rc = A->val.zero(fs_rt().stream);
    if (rc == FS_OK && hipStreamSynchronize(fs_rt().stream) != hipSuccess) rc = FS_ERR_HIP;
    if (rc != FS_OK) {
        delete A;
        return rc;
    }
    *out = A;
    return FS_OK;
}

int64_t fs_dg_matrix_nnz(const fs_space_s* sp) {
    const int64_t L = dg_dim(sp) + 1;
    return L * L * sp->mesh->nc + L * L * sp->dg_interior_sides;
}

// sorted-column CSR in dof order, the zero slots of boundary facets left out (a host-side export for tests)
int fs_dg_matrix_get_csr(fs_matrix_s* A, int32_t* rowptr, int32_t* colidx, double* vals) {
    fs_space_s* sp = A->space;
    const int L = dg_dim(sp) + 1;
    const int64_t nc = sp->mesh->nc, nnz = fs_dg_matrix_nnz(sp);
    FS_REQUIRE(nnz < (int64_t)INT32_MAX, "fs_matrix_get_csr: nnz exceeds int32");
    std::vector<double> v;
    if (vals) {
        v.resize(A->val.n);
        FS_CHECK(A->val.download(v.data(), A->val.n, fs_rt().stream));
    }
    int64_t pos = 0;
    if (rowptr) rowptr[0] = 0;
    for (int64_t K = 0; K < nc; ++K) {
        std::pair<int32_t, int> blocks[5];
        int nb = 0;
        blocks[nb++] = {(int32_t)K, 0};
        for (int k = 0; k < L; ++k) {
            const int32_t N = sp->dg_nbr_host[(int64_t)k * nc + K];
            if (N >= 0) blocks[nb++] = {N, k + 1};
        }
        std::sort(blocks, blocks + nb);
        for (int a = 0; a < L; ++a) {
            for (int j = 0; j < nb; ++j)
                for (int c = 0; c < L; ++c, ++pos) {
                    if (colidx) colidx[pos] = blocks[j].first * L + c;
                    if (vals) vals[pos] = v[((int64_t)(blocks[j].second * L + a) * L + c) * nc + K];
                }
            if (rowptr) rowptr[K * L + a + 1] = (int32_t)pos;
        }
    }
    return FS_OK;
}

int fs_dg_apply_dirichlet(fs_matrix_s* A, fs_vector_s* b, int64_t n, const int32_t* dofs, const double* vals, int symmetric) {
    if (symmetric) {
        fs_set_error("fs_apply_dirichlet: DG matrices take Dirichlet rows as identity rows (symmetric = 0)");
        return FS_ERR_UNSUPPORTED;
    }
    fs_space_s* sp = A->space;
    FS_REQUIRE(!b || b->d.n >= sp->n_dofs_owned, "fs_apply_dirichlet: b shorter than the owned dofs");
    // later entries win on duplicates
    std::map<int32_t, double> last;
    for (int64_t i = 0; i < n; ++i) {
        FS_REQUIRE(dofs[i] >= 0 && dofs[i] < sp->n_dofs_owned, "fs_apply_dirichlet: dof %d outside [0,%lld)", dofs[i], (long long)sp->n_dofs_owned);
        last[dofs[i]] = vals[i];
    }
    std::vector<int32_t> d;
    std::vector<double> g;
    d.reserve(last.size());
    g.reserve(last.size());
    for (const auto& e : last) { d.push_back(e.first); g.push_back(e.second); }
    hipStream_t s = fs_rt().stream;
    dbuf<int32_t> dd;
    dbuf<double> dg;
    const int64_t m = (int64_t)d.size();
    FS_CHECK(dd.alloc(m));
    FS_CHECK(dg.alloc(m));
    FS_CHECK(dd.upload(d.data(), m, s));
    FS_CHECK(dg.upload(g.data(), m, s));
    const int grid = (int)((m + FS_BLOCK - 1) / FS_BLOCK);
    if (dg_dim(sp) == 3)
        hipLaunchKernelGGL(k_dg_dirichlet<3>, dim3(grid), dim3(FS_BLOCK), 0, s, m, dd.p, dg.p, sp->mesh->nc, A->val.p, b ? b->d.p : nullptr);
    else
        hipLaunchKernelGGL(k_dg_dirichlet<2>, dim3(grid), dim3(FS_BLOCK), 0, s, m, dd.p, dg.p, sp->mesh->nc, A->val.p, b ? b->d.p : nullptr);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// ---- assembly ---------------------------------------------------------------------------------------------------------------
extern "C" int fs_assemble_dg_transport(fs_matrix_t A, fs_vector_t b, const fs_dg_form* form) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(A && form, "fs_assemble_dg_transport: null pointer");
    fs_space_s* sp = A->space;
    if (sp->family != FS_FAMILY_DG) {
        fs_set_error("fs_assemble_dg_transport: the matrix is not on a DG space");
        return FS_ERR_UNSUPPORTED;
    }
    fs_mesh_s* m = sp->mesh;
    const int D = m->tdim, L = D + 1;
    const int64_t nc = m->nc;
    FS_REQUIRE(!b || b->d.n >= sp->n_dofs_owned, "fs_assemble_dg_transport: b shorter than the dofs");
    FS_REQUIRE(form->n_facets >= 0 && (form->n_facets == 0 || (form->facet_cell && form->facet_local)),
               "fs_assemble_dg_transport: bad facet list");
    FS_REQUIRE(std::isfinite(form->conductivity) && std::isfinite(form->capacity) && std::isfinite(form->alpha) &&
                   std::isfinite(form->operator_scale) && std::isfinite(form->mass_scale),
               "fs_assemble_dg_transport: coefficients must be finite");
    hipStream_t s = fs_rt().stream;
    dg_form_dev F;
    F.k = form->conductivity;
    F.c = form->capacity;
    for (int d = 0; d < 3; ++d) F.beta[d] = d < D ? form->velocity[d] : 0.0;
    F.alpha = form->alpha;
    F.op = form->operator_scale;
    F.mass = form->mass_scale;
    // listed boundary facets grouped by cell, ascending local facet (stable: the caller's order among duplicates)
    dbuf<int32_t> d_ptr, d_loc;
    dbuf<double> d_h, d_g, d_src;
    const int64_t nf = form->n_facets;
    if (nf > 0 && (form->facet_h || (b && form->facet_g))) {
        std::vector<int64_t> ord(nf);
        for (int64_t i = 0; i < nf; ++i) {
            FS_REQUIRE(form->facet_cell[i] >= 0 && form->facet_cell[i] < nc && form->facet_local[i] >= 0 && form->facet_local[i] < L,
                       "fs_assemble_dg_transport: facet %lld names cell %d / local facet %d", (long long)i, form->facet_cell[i],
                       form->facet_local[i]);
            FS_REQUIRE(sp->dg_nbr_host[(int64_t)form->facet_local[i] * nc + form->facet_cell[i]] < 0,
                       "fs_assemble_dg_transport: facet %lld is not on the boundary", (long long)i);
            ord[i] = i;
        }
        std::stable_sort(ord.begin(), ord.end(), [&](int64_t p, int64_t q) {
            return form->facet_cell[p] != form->facet_cell[q] ? form->facet_cell[p] < form->facet_cell[q] : form->facet_local[p] < form->facet_local[q];
        });
        std::vector<int32_t> ptr(nc + 1, 0), loc(nf);
        std::vector<double> h(form->facet_h ? nf : 0), g(b && form->facet_g ? nf * L : 0);
        for (int64_t j = 0; j < nf; ++j) {
            const int64_t i = ord[j];
            ptr[form->facet_cell[i] + 1]++;
            loc[j] = form->facet_local[i];
            if (!h.empty()) h[j] = form->facet_h[i];
            if (!g.empty())
                for (int e = 0; e < L; ++e) g[j * L + e] = form->facet_g[i * L + e];
        }
        for (int64_t K = 0; K < nc; ++K) ptr[K + 1] += ptr[K];
        FS_CHECK(d_ptr.alloc(nc + 1));
        FS_CHECK(d_ptr.upload(ptr.data(), nc + 1, s));
        FS_CHECK(d_loc.alloc(nf));
        FS_CHECK(d_loc.upload(loc.data(), nf, s));
        if (!h.empty()) { FS_CHECK(d_h.alloc(nf)); FS_CHECK(d_h.upload(h.data(), nf, s)); }
        if (!g.empty()) { FS_CHECK(d_g.alloc(nf * L)); FS_CHECK(d_g.upload(g.data(), nf * L, s)); }
    }
    if (b && form->source) {
        FS_CHECK(d_src.alloc(nc * L));
        FS_CHECK(d_src.upload(form->source, nc * L, s));
    }
    const int grid = (int)((nc + FS_BLOCK - 1) / FS_BLOCK);
#define FS_DG_ASM_ARGS dim3(grid), dim3(FS_BLOCK), 0, s, nc, m->cells.p, m->xyz.p, sp->dg_nbr.p, sp->dg_plus.p, F, d_ptr.p, d_loc.p, d_h.p, \
                       d_g.p, d_src.p, form->add, A->val.p, b ? b->d.p : nullptr
    if (D == 3)
        hipLaunchKernelGGL(k_dg_assemble<3>, FS_DG_ASM_ARGS);
    else
        hipLaunchKernelGGL(k_dg_assemble<2>, FS_DG_ASM_ARGS);
#undef FS_DG_ASM_ARGS
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// ---- product ----------------------------------------------------------------------------------------------------------------
int64_t fs_dg_spmv_bytes(const fs_space_s* sp) {
    // algorithmic traffic: every block value once, the neighbour table, x of the cell and its neighbours, y
    const int64_t L = dg_dim(sp) + 1, nc = sp->mesh->nc;
    return (L + 1) * L * L * 8 * nc + L * 4 * nc + 2 * L * 8 * nc;
}

int fs_dg_spmv_dev(fs_matrix_s* A, const double* x, double* y, hipStream_t s) {
    const fs_space_s* sp = A->space;
    const int64_t nc = sp->mesh->nc;
    const int grid = (int)std::min<int64_t>((nc + FS_BLOCK - 1) / FS_BLOCK, 65535);
    if (dg_dim(sp) == 3)
        hipLaunchKernelGGL((k_dg_spmv<3, false, false>), dim3(grid), dim3(FS_BLOCK), 0, s, nc, A->val.p, sp->dg_nbr.p, x, y, nullptr, nullptr, nullptr);
    else
        hipLaunchKernelGGL((k_dg_spmv<2, false, false>), dim3(grid), dim3(FS_BLOCK), 0, s, nc, A->val.p, sp->dg_nbr.p, x, y, nullptr, nullptr, nullptr);
    FS_KERNEL_CHECK();
    return FS_OK;
}

int fs_dg_spmv(fs_matrix_s* A, fs_vector_s* x, fs_vector_s* y) {
    const fs_space_s* sp = A->space;
    FS_REQUIRE(x->d.n >= sp->n_dofs_local && y->d.n >= sp->n_dofs_owned, "fs_spmv: x / y shorter than the dofs (%lld)", (long long)sp->n_dofs_local);
    hipStream_t s = fs_rt().stream;
    FS_CHECK(fs_dg_spmv_dev(A, x->d.p, y->d.p, s));
    FS_HIP(hipStreamSynchronize(s));
    fs_set_last_product_kind(6);
    return FS_OK;
}

// ---- BiCGStab, right-preconditioned by the inverse diagonal blocks ------------------------------------------------------------
namespace {
struct dg_ws {
    dbuf<double> minv, r, rhat, p, phat, v, shat, t, partials, hist, sums;
    dbuf<dg_state> st;
    dbuf<int> flag;
};
}  // namespace

int fs_dg_krylov_solve(fs_matrix_s* A, fs_vector_s* bv, fs_vector_s* xv, const fs_krylov_opts* opts, fs_krylov_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    fs_space_s* sp = A->space;
    if (opts->method != FS_KSP_BICGSTAB) {
        fs_set_error("fs_krylov_solve: DG operators are not symmetric: use FS_KSP_BICGSTAB");
        return FS_ERR_UNSUPPORTED;
    }
    FS_REQUIRE(opts->precond == FS_PC_NONE || opts->precond == FS_PC_JACOBI || opts->precond == FS_PC_BLOCK_JACOBI,
               "fs_krylov_solve: unknown preconditioner %d", opts->precond);
    FS_REQUIRE(opts->max_iter > 0 && opts->rtol >= 0.0 && opts->atol >= 0.0, "fs_krylov_solve: bad tolerances");
    const int D = dg_dim(sp), L = D + 1;
    const int64_t nc = sp->mesh->nc, n = sp->n_dofs_owned;
    FS_REQUIRE(bv->d.n >= n && xv->d.n >= n, "fs_krylov_solve: b/x shorter than the dofs (%lld)", (long long)n);
    hipStream_t s = fs_rt().stream;
    dg_ws w;
    FS_CHECK(w.minv.alloc((int64_t)L * L * nc));
    for (dbuf<double>* q : {&w.r, &w.rhat, &w.p, &w.phat, &w.v, &w.shat, &w.t}) FS_CHECK(q->alloc(n));
    FS_CHECK(w.partials.alloc(5 * DG_GRID_MAX));
    FS_CHECK(w.hist.alloc((int64_t)opts->max_iter + 1));
    FS_CHECK(w.sums.alloc(2));   // true ||r||^2, ||M^-1 r||^2
    FS_CHECK(w.st.alloc(1));
    FS_CHECK(w.flag.alloc(1));
    FS_CHECK(w.flag.zero(s));
    FS_CHECK(w.st.zero(s));
    const int pc = opts->precond == FS_PC_BLOCK_JACOBI ? 2 : opts->precond == FS_PC_JACOBI ? 1 : 0;
    // FS_NORM_PRECONDITIONED: the stopping test on ||M^-1 r|| <= rtol ||M^-1 b|| - the inverse diagonal blocks put the unit
    // Dirichlet rows and the physical rows (of scale c kappa h) on one scale; without a preconditioner it is the plain norm
    const int pnorm = (opts->norm_type == FS_NORM_PRECONDITIONED && pc != 0) ? 1 : 0;
    const int gcell = (int)((nc + FS_BLOCK - 1) / FS_BLOCK);
    const int gred = dg_grid(nc);
    double* x = xv->d.p;
    const double* b = bv->d.p;
    int* done = &w.st.p->done;
    const double rtol2 = opts->rtol * opts->rtol, atol2 = opts->atol * opts->atol;

    if (D == 3) hipLaunchKernelGGL(k_dg_precond<3>, dim3(gcell), dim3(FS_BLOCK), 0, s, nc, A->val.p, pc, w.minv.p, w.flag.p);
    else hipLaunchKernelGGL(k_dg_precond<2>, dim3(gcell), dim3(FS_BLOCK), 0, s, nc, A->val.p, pc, w.minv.p, w.flag.p);
    FS_KERNEL_CHECK();
    const double* y0 = nullptr;     // A x0 of the pass (nullptr: x0 = 0, r = b)
    auto update = [&](int mode) {
        if (D == 3)
            hipLaunchKernelGGL(k_dg_update<3>, dim3(gred), dim3(FS_BLOCK), 0, s, mode, nc, w.minv.p, w.st.p, x, w.r.p, w.rhat.p, w.p.p, w.phat.p,
                               w.v.p, w.shat.p, w.t.p, b, y0, w.partials.p, pnorm);
        else
            hipLaunchKernelGGL(k_dg_update<2>, dim3(gred), dim3(FS_BLOCK), 0, s, mode, nc, w.minv.p, w.st.p, x, w.r.p, w.rhat.p, w.p.p, w.phat.p,
                               w.v.p, w.shat.p, w.t.p, b, y0, w.partials.p, pnorm);
    };
    auto finalize = [&](int which) {
        hipLaunchKernelGGL(k_dg_finalize, dim3(1), dim3(FS_BLOCK), 0, s, w.st.p, w.partials.p, gred, which, w.hist.p, rtol2, atol2);
    };
    auto product = [&](const double* in, double* out, const double* u, bool dot_y) {
        if (D == 3) {
            if (dot_y) hipLaunchKernelGGL((k_dg_spmv<3, true, true>), dim3(gred), dim3(FS_BLOCK), 0, s, nc, A->val.p, sp->dg_nbr.p, in, out, u, w.partials.p, done);
            else hipLaunchKernelGGL((k_dg_spmv<3, true, false>), dim3(gred), dim3(FS_BLOCK), 0, s, nc, A->val.p, sp->dg_nbr.p, in, out, u, w.partials.p, done);
        } else {
            if (dot_y) hipLaunchKernelGGL((k_dg_spmv<2, true, true>), dim3(gred), dim3(FS_BLOCK), 0, s, nc, A->val.p, sp->dg_nbr.p, in, out, u, w.partials.p, done);
            else hipLaunchKernelGGL((k_dg_spmv<2, true, false>), dim3(gred), dim3(FS_BLOCK), 0, s, nc, A->val.p, sp->dg_nbr.p, in, out, u, w.partials.p, done);
        }
    };
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
    FS_HIP(hipEventCreate(&e0));
    FS_HIP(hipEventCreate(&e1));
    FS_HIP(hipEventCreate(&e2));
    FS_HIP(hipEventCreate(&e3));
    std::vector<double> hist;       // ||n(r)||^2 of every iteration, the passes one after the other (each starts with its true residual)
    const int batch = opts->batch > 0 ? opts->batch : 32;
    int launched = 0, timed = 0, total_iter = 0;
    double spmv_ms = 0.0, update_ms = 0.0, true_rr = 0.0, true_rrp = 0.0, prev_true = HUGE_VAL;
    bool met = false;
    dg_state hs{};
    int rc = FS_OK;
    // The recurrence residual of BiCGStab drifts from the true one on ill-conditioned operators (the penalty of the SIPG form):
    // when the recurrence has converged and the true residual has not, the iteration restarts from x (r = b - A x), as long as a
    // pass lowers the true residual by at least a factor 2 - until fp64 gives no more.  Converged means: the TRUE residual met
    // the tolerance.  The host polls the device state every `batch` iterations through the library's pinned staging buffer.
    for (int pass = 0; pass < 16 && rc == FS_OK; ++pass) {
        if (pass > 0 || opts->nonzero_guess) {
            FS_CHECK(fs_dg_spmv_dev(A, x, w.t.p, s));
            y0 = w.t.p;
        } else {
            FS_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), s));
            y0 = nullptr;
        }
        update(0);
        finalize(0);
        FS_KERNEL_CHECK();
        FS_CHECK(w.st.download(&hs, 1, s));
        while (!hs.done && launched < opts->max_iter) {
            const int nb = std::min(batch, opts->max_iter - launched);
            for (int i = 0; i < nb; ++i) {
                const bool time_it = i == 0;
                if (time_it) (void)hipEventRecord(e0, s);
                product(w.phat.p, w.v.p, w.rhat.p, false);          // v = A phat, rhat.v
                if (time_it) (void)hipEventRecord(e1, s);
                finalize(1);                                        // alpha
                update(1);                                          // s = r - alpha v, shat = M^-1 s
                product(w.shat.p, w.t.p, w.r.p, true);              // t = A shat, t.s, t.t
                finalize(2);                                        // omega
                if (time_it) (void)hipEventRecord(e2, s);
                update(2);                                          // x, r = s - omega t, rhat.r, n(r).n(r)
                if (time_it) (void)hipEventRecord(e3, s);
                finalize(3);                                        // rho, beta, ||r||
                update(3);                                          // p, phat = M^-1 p
            }
            launched += nb;
            if (hipGetLastError() != hipSuccess) { fs_set_error("fs_krylov_solve: DG iteration launch failed"); rc = FS_ERR_HIP; break; }
            FS_CHECK(w.st.download(&hs, 1, s));
            float a = 0.f, c = 0.f;
            if (hipEventElapsedTime(&a, e0, e1) == hipSuccess) spmv_ms += a;
            if (hipEventElapsedTime(&c, e2, e3) == hipSuccess) update_ms += c;
            ++timed;
        }
        total_iter += hs.iter;
        if (rc != FS_OK) break;
        {
            std::vector<double> h((size_t)hs.iter + 1);
            FS_CHECK(w.hist.download(h.data(), hs.iter + 1, s));
            hist.insert(hist.end(), h.begin(), h.end());
        }
        // true residual
        FS_CHECK(fs_dg_spmv_dev(A, x, w.t.p, s));
        if (D == 3) hipLaunchKernelGGL(k_dg_resid<3>, dim3(gred), dim3(FS_BLOCK), 0, s, nc, w.minv.p, pnorm, b, w.t.p, w.partials.p);
        else hipLaunchKernelGGL(k_dg_resid<2>, dim3(gred), dim3(FS_BLOCK), 0, s, nc, w.minv.p, pnorm, b, w.t.p, w.partials.p);
        hipLaunchKernelGGL(k_dg_sum, dim3(1), dim3(FS_BLOCK), 0, s, w.partials.p, gred, 2, w.sums.p);
        FS_KERNEL_CHECK();
        double tr[2] = {0.0, 0.0};
        FS_CHECK(w.sums.download(tr, 2, s));
        true_rr = tr[0];
        true_rrp = tr[1];
        met = true_rr <= hs.tol2 && (!pnorm || true_rrp <= hs.tol2p);
        // progress: the larger of the two relative misses
        const double miss = std::max(hs.tol2 > 0.0 ? true_rr / hs.tol2 : 0.0, pnorm && hs.tol2p > 0.0 ? true_rrp / hs.tol2p : 0.0);
        // a breakdown (rhat.v = 0 or omega = 0: advection-dominated operators) restarts too - with a new shadow residual rhat -
        // provided the pass iterated at all and lowered the true residual
        const bool restartable = hs.done == 1 || (hs.done == 2 && hs.iter > 0);
        if (!restartable || met || !(miss < 0.25 * prev_true) || launched >= opts->max_iter) break;
        prev_true = miss;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipEventDestroy(e2);
    (void)hipEventDestroy(e3);
    if (rc != FS_OK) return rc;
    int singular = 0;
    FS_CHECK(w.flag.download(&singular, 1, s));
    fs_krylov_set_history(hist);
    fs_set_last_product_kind(6);
    const double bnorm = std::sqrt(hs.bb);
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->iterations = total_iter;
        stats->converged = met ? 1 : hs.done == 2 ? -1 : 0;
        stats->bnorm = bnorm;
        stats->rel_residual = bnorm > 0.0 ? std::sqrt(hs.rr) / bnorm : 0.0;
        stats->true_rel_residual = bnorm > 0.0 ? std::sqrt(true_rr) / bnorm : 0.0;
        stats->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->spmv_ms = timed ? spmv_ms / timed : 0.0;
        stats->update_ms = timed ? update_ms / timed : 0.0;
        stats->spmv_bytes = fs_dg_spmv_bytes(sp);
        stats->launches = launched;
        stats->product_kind = 6;
    }
    if (singular && pc != 0) {
        fs_set_error("fs_krylov_solve: a diagonal block of the DG operator is singular");
        return FS_ERR_NUMERIC;
    }
    if (hs.done == 2 && !met) {
        fs_set_error("fs_krylov_solve: BiCGStab breakdown on the DG operator after %d iterations (rho %.3e alpha %.3e omega %.3e "
                     "||r||^2 %.3e ||b||^2 %.3e, last sums %.3e %.3e)", hs.iter, hs.rho, hs.alpha, hs.omega, hs.rr, hs.bb, hs.last[0], hs.last[1]);
        return FS_ERR_NUMERIC;
    }
    return FS_OK;
}

// ---- projection onto CG1 ----------------------------------------------------------------------------------------------------
extern "C" int fs_assemble_dg_projection(fs_space_t V_dg, fs_vector_t x, fs_space_t V_cg1, fs_vector_t b) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(V_dg && x && V_cg1 && b, "fs_assemble_dg_projection: null pointer");
    if (V_dg->family != FS_FAMILY_DG || V_cg1->family != FS_FAMILY_CG || V_cg1->degree != 1 || V_cg1->ncomp != 1) {
        fs_set_error("fs_assemble_dg_projection: needs a DG1 space and a scalar CG1 space");
        return FS_ERR_UNSUPPORTED;
    }
    FS_REQUIRE(V_dg->mesh == V_cg1->mesh, "fs_assemble_dg_projection: the two spaces must be on the same mesh");
    fs_mesh_s* m = V_dg->mesh;
    FS_REQUIRE(x->d.n >= V_dg->n_dofs_owned && b->d.n >= m->nv, "fs_assemble_dg_projection: vector too short");
    hipStream_t s = fs_rt().stream;
    const int grid = (int)((m->nv + FS_BLOCK - 1) / FS_BLOCK);
    if (m->tdim == 3)
        hipLaunchKernelGGL(k_dg_projection<3>, dim3(grid), dim3(FS_BLOCK), 0, s, m->nv, V_dg->dg_vptr.p, V_dg->dg_vinc.p, m->cells.p, m->xyz.p, x->d.p, b->d.p);
    else
        hipLaunchKernelGGL(k_dg_projection<2>, dim3(grid), dim3(FS_BLOCK), 0, s, m->nv, V_dg->dg_vptr.p, V_dg->dg_vinc.p, m->cells.p, m->xyz.p, x->d.p, b->d.p);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}
