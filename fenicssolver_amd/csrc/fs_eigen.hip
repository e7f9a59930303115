// Block eigensolver of libfsamd.so (gfx950, fp64): the lowest modes of K phi = lambda M phi by LOBPCG.
//
// Stands in for SLEPcEigenSolver (FenicsSolver/LinearElasticitySolver.py:283-310).  The reference asks SLEPc for its default,
// the largest-magnitude eigenpair of the stiffness alone; this solver computes the physically meaningful problem instead: the
// n_modes smallest eigenvalues of the pencil (K, M) restricted to the free dofs ("differs from the reference").
//
// Blocks of vectors are column-major: column j of a block at base + j * ld, so each column is a plain vector that the V-cycle
// (fs_amg_apply_dev) and fs_spmv take.  The hot path is three kernels:
//   k_sell_spmv_multi  Y = A X for MC columns at a time on the node-block SELL storage; every 3 x 3 (2 x 2) block of values is
//                      loaded once per chunk of columns, and every column is summed in the order of k_sell_spmv, so each column
//                      of Y equals fs_spmv of that column bit for bit.  Constrained rows are stored as 0.
//   k_block_gram       G = X^T Y: per-workgroup partials of 8 x 8 tiles, then one fixed-order sum (deterministic).
//   k_block_combine    Y = X C + Z D with the small coefficient matrices read as wave-uniform (scalar) loads.
// The driver (robust LOBPCG: Knyazev 2001; Duersch, Shao, Yang & Gu, SISC 2018) keeps the basis S = [X P W] and the blocks
// K S and M S, updates them by combinations, and solves the dense Rayleigh-Ritz problem on the host (cyclic Jacobi: the library
// links no LAPACK).
//
// The iteration itself (lobpcg()) is written for a pencil A x = theta B x and serves two entry points: fs_eigen_solve with
// (A, B) = (K, M), and fs_buckling_solve - linear buckling, (K + lambda K_G) phi = 0 - with (A, B) = (K_G, K), whose lowest theta = nu
// are the smallest positive lambda = -1 / nu.  There K S and K_G S of the same columns come from one pass over the pattern:
//   k_sell_spmv_pencil  both products for MC columns, K_G read from a copy of one double per node pair (k_pencil_compact).
#include "fs_common.h"
#include "fs_kernels.h"
#include <math.h>
#include <chrono>
#include <algorithm>

#define FS_GRAM_T 8            // gram tile: 8 x 8 entries per thread
#define FS_COMBINE_Q 8         // output columns per pass of k_block_combine
#define FS_EIGEN_DROP 1e-14    // a column whose M-norm falls below 1e-7 of its norm before the projections is dropped
#define FS_EIGEN_REFRESH 10    // K X and M X are recomputed from X every this many iterations: the combinations drift by about
                               // eps |K| / lambda_1 per iteration, which at 5 M DOF stalls the residuals near 1e-6

// ---- Y = A X for MC columns ----------------------------------------------------------------------------------------------
// The slice walk and the order of summation per row are those of k_sell_spmv<BS, 0, *> (fs_krylov_stream.inc): entry by entry,
// and inside an entry column j = 0 .. BS-1 of the block, each term one fma into the row's accumulator.  Padding entries (value 0,
// a safe column) and the clamped columns of DIA slices are multiplied in exactly as there.
template <int BS, int MC>
__global__ void __launch_bounds__(FS_BLOCK) k_sell_spmv_multi(int64_t n_rows, int64_t n_cols, int64_t n_slices,
                                                              const int64_t* __restrict__ slice_ptr,
                                                              const int32_t* __restrict__ sell_col,
                                                              const int32_t* __restrict__ dia_ptr,
                                                              const int32_t* __restrict__ dia_off,
                                                              const double* __restrict__ val, int64_t plane,
                                                              const int32_t* __restrict__ order,
                                                              const double* __restrict__ X, int64_t ldx,
                                                              double* __restrict__ Y, int64_t ldy,
                                                              const uint8_t* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t n_chunks = (n_slices + 3) >> 2;
    const int32_t cmax = (int32_t)(n_cols - 1);
    for (chunk_iter it = xcd_chunks(n_chunks); it.cur < it.end; it.cur += it.step) {
        const int64_t q = __builtin_amdgcn_readfirstlane((int)(it.cur * 4 + wave));
        if (q >= n_slices) continue;
        const int64_t s = order ? __builtin_amdgcn_readfirstlane(order[q]) : q;
        const int64_t base = slice_ptr[s];
        const int width = (int)((slice_ptr[s + 1] - base) >> 6);
        const int32_t dp = dia_ptr[s];
        const int64_t r = s * FS_SLICE + lane;
        const int32_t* __restrict__ cp = sell_col + base + lane;
        const double* __restrict__ vp = val + base + lane;
        const int32_t* __restrict__ op = nullptr;
        const int32_t* __restrict__ op2 = nullptr;
        bool hi = false;
        if (dp >= 0) {
            const int split = dia_off[dp];
            op = dia_off + dp + 1;
            op2 = op + (split < FS_SLICE ? width : 0);
            hi = lane >= split;
        }
        double acc[MC][BS];
#pragma unroll
        for (int c = 0; c < MC; ++c)
#pragma unroll
            for (int i = 0; i < BS; ++i) acc[c][i] = 0.0;
        for (int k = 0; k < width; ++k) {
            int64_t col;
            if (dp >= 0) {
                col = r + (hi ? op2[k] : op[k]);
                col = col < 0 ? 0 : (col > cmax ? cmax : col);
            } else {
                col = fs_col_decode(cp[(int64_t)k * FS_SLICE]);
            }
            double v[BS * BS];
#pragma unroll
            for (int e = 0; e < BS * BS; ++e) v[e] = vp[(int64_t)e * plane + (int64_t)k * FS_SLICE];
            double xv[MC][BS];
#pragma unroll
            for (int c = 0; c < MC; ++c)
#pragma unroll
                for (int j = 0; j < BS; ++j) xv[c][j] = X[(int64_t)c * ldx + col * BS + j];
#pragma unroll
            for (int c = 0; c < MC; ++c)
#pragma unroll
                for (int j = 0; j < BS; ++j)
#pragma unroll
                    for (int i = 0; i < BS; ++i) acc[c][i] += v[i * BS + j] * xv[c][j];
        }
        if (r < n_rows) {
#pragma unroll
            for (int i = 0; i < BS; ++i) {
                const bool off = mask && mask[r * BS + i];
#pragma unroll
                for (int c = 0; c < MC; ++c) Y[(int64_t)c * ldy + r * BS + i] = off ? 0.0 : acc[c][i];
            }
        }
    }
}

// ---- Y_K = K X and Y_G = K_G X for MC columns in one pass over the pattern ------------------------------------------------------
// The buckling pencil (fs_buckling_solve) needs both products of the same columns.  K_G's node-pair blocks are s I (fs_buckling.hip),
// so it is read from a compact copy gs of one double per stored block (k_pencil_compact) in the layout of one value plane: 8 B per
// block where the block storage streams 72 B (32 B in 2-D).  The column index and the MC x BS values of X are gathered once for both
// halves.  Walk, clamping, padding and mask are those of k_sell_spmv_multi.
//   K half:   the statements of k_sell_spmv_multi, so every column equals fs_spmv_multi(K) bit for bit.
//   K_G half: one fma per entry, row component and column.  k_sell_spmv_multi on the block storage adds the same fma and BS - 1 more
//             with an exact 0.0 factor, which leave a finite sum unchanged (at most they turn a -0 into +0): the two agree as numbers
//             for finite X, not in the sign of a zero.
// Registers (BS = 3, MC = 8): 2 x 24 accumulators, 24 values of X, 9 + 1 matrix values, all fp64 - twice the accumulators of
// k_sell_spmv_multi<3, 8>; the compiler's count is in DESIGN.md.  No LDS.
template <int BS, int MC>
__global__ void __launch_bounds__(FS_BLOCK) k_sell_spmv_pencil(int64_t n_rows, int64_t n_cols, int64_t n_slices,
                                                               const int64_t* __restrict__ slice_ptr,
                                                               const int32_t* __restrict__ sell_col,
                                                               const int32_t* __restrict__ dia_ptr,
                                                               const int32_t* __restrict__ dia_off,
                                                               const double* __restrict__ val, int64_t plane,
                                                               const double* __restrict__ gs,
                                                               const int32_t* __restrict__ order,
                                                               const double* __restrict__ X, int64_t ldx,
                                                               double* __restrict__ YK, double* __restrict__ YG, int64_t ldy,
                                                               const uint8_t* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t n_chunks = (n_slices + 3) >> 2;
    const int32_t cmax = (int32_t)(n_cols - 1);
    for (chunk_iter it = xcd_chunks(n_chunks); it.cur < it.end; it.cur += it.step) {
        const int64_t q = __builtin_amdgcn_readfirstlane((int)(it.cur * 4 + wave));
        if (q >= n_slices) continue;
        const int64_t s = order ? __builtin_amdgcn_readfirstlane(order[q]) : q;
        const int64_t base = slice_ptr[s];
        const int width = (int)((slice_ptr[s + 1] - base) >> 6);
        const int32_t dp = dia_ptr[s];
        const int64_t r = s * FS_SLICE + lane;
        const int32_t* __restrict__ cp = sell_col + base + lane;
        const double* __restrict__ vp = val + base + lane;
        const double* __restrict__ gp = gs + base + lane;
        const int32_t* __restrict__ op = nullptr;
        const int32_t* __restrict__ op2 = nullptr;
        bool hi = false;
        if (dp >= 0) {
            const int split = dia_off[dp];
            op = dia_off + dp + 1;
            op2 = op + (split < FS_SLICE ? width : 0);
            hi = lane >= split;
        }
        double acc[MC][BS], accg[MC][BS];
#pragma unroll
        for (int c = 0; c < MC; ++c)
#pragma unroll
            for (int i = 0; i < BS; ++i) acc[c][i] = accg[c][i] = 0.0;
        for (int k = 0; k < width; ++k) {
            int64_t col;
            if (dp >= 0) {
                col = r + (hi ? op2[k] : op[k]);
                col = col < 0 ? 0 : (col > cmax ? cmax : col);
            } else {
                col = fs_col_decode(cp[(int64_t)k * FS_SLICE]);
            }
            double v[BS * BS];
#pragma unroll
            for (int e = 0; e < BS * BS; ++e) v[e] = vp[(int64_t)e * plane + (int64_t)k * FS_SLICE];
            const double g = gp[(int64_t)k * FS_SLICE];
            double xv[MC][BS];
#pragma unroll
            for (int c = 0; c < MC; ++c)
#pragma unroll
                for (int j = 0; j < BS; ++j) xv[c][j] = X[(int64_t)c * ldx + col * BS + j];
#pragma unroll
            for (int c = 0; c < MC; ++c)
#pragma unroll
                for (int j = 0; j < BS; ++j)
#pragma unroll
                    for (int i = 0; i < BS; ++i) acc[c][i] += v[i * BS + j] * xv[c][j];
#pragma unroll
            for (int c = 0; c < MC; ++c)
#pragma unroll
                for (int i = 0; i < BS; ++i) accg[c][i] += g * xv[c][i];
        }
        if (r < n_rows) {
#pragma unroll
            for (int i = 0; i < BS; ++i) {
                const bool off = mask && mask[r * BS + i];
#pragma unroll
                for (int c = 0; c < MC; ++c) {
                    YK[(int64_t)c * ldy + r * BS + i] = off ? 0.0 : acc[c][i];
                    YG[(int64_t)c * ldy + r * BS + i] = off ? 0.0 : accg[c][i];
                }
            }
        }
    }
}

// gs[e] = s of the stored block e of a matrix whose blocks are s I, and the check that they are: *bad becomes 1 where a diagonal
// entry differs from s (or is a NaN) or an off-diagonal entry is not 0.0.  Every writer stores the same 1.
template <int BS>
__global__ void __launch_bounds__(FS_BLOCK) k_pencil_compact(int64_t n_entries, const double* __restrict__ val, int64_t plane,
                                                             double* __restrict__ gs, int* __restrict__ bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += stride) {
        const double s = val[e];
        bool ok = s == s;
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) {
                const double x = val[(int64_t)(i * BS + j) * plane + e];
                ok = ok && (i == j ? x == s : x == 0.0);
            }
        gs[e] = s;
        if (!ok) *bad = 1;
    }
}

// ---- G = X^T Y ------------------------------------------------------------------------------------------------------------
// blockIdx.y: one 8 x 8 tile of G; blockIdx.x: one of nrb row groups (rows blockIdx.x * 256 + t, stride nrb * 256).  Each tile
// entry's partial of the group goes to partials[entry * nrb + group]; k_block_gram_finish adds them in group order.  The grid
// depends on (n, p, q) only, so a call gives the same bits every time.
__global__ void __launch_bounds__(FS_BLOCK) k_block_gram(int64_t n, const double* __restrict__ X, int64_t ldx, int p,
                                                         const double* __restrict__ Y, int64_t ldy, int q,
                                                         double* __restrict__ partials, int nrb) {
    __shared__ double red[FS_BLOCK / 64][FS_GRAM_T * FS_GRAM_T];
    const int ntq = (q + FS_GRAM_T - 1) / FS_GRAM_T;
    const int a0 = (blockIdx.y / ntq) * FS_GRAM_T, b0 = (blockIdx.y % ntq) * FS_GRAM_T;
    const int na = min(FS_GRAM_T, p - a0), nb = min(FS_GRAM_T, q - b0);
    double acc[FS_GRAM_T][FS_GRAM_T];
#pragma unroll
    for (int a = 0; a < FS_GRAM_T; ++a)
#pragma unroll
        for (int b = 0; b < FS_GRAM_T; ++b) acc[a][b] = 0.0;
    const int64_t stride = (int64_t)nrb * FS_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * FS_BLOCK + threadIdx.x; i < n; i += stride) {
        double xa[FS_GRAM_T], yb[FS_GRAM_T];
#pragma unroll
        for (int a = 0; a < FS_GRAM_T; ++a) xa[a] = a < na ? X[(int64_t)(a0 + a) * ldx + i] : 0.0;
#pragma unroll
        for (int b = 0; b < FS_GRAM_T; ++b) yb[b] = b < nb ? Y[(int64_t)(b0 + b) * ldy + i] : 0.0;
#pragma unroll
        for (int a = 0; a < FS_GRAM_T; ++a)
#pragma unroll
            for (int b = 0; b < FS_GRAM_T; ++b) acc[a][b] = fma(xa[a], yb[b], acc[a][b]);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < FS_GRAM_T; ++a)
#pragma unroll
        for (int b = 0; b < FS_GRAM_T; ++b) {
            double v = acc[a][b];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) red[wave][a * FS_GRAM_T + b] = v;
        }
    __syncthreads();
    if (threadIdx.x < FS_GRAM_T * FS_GRAM_T) {
        const int a = threadIdx.x / FS_GRAM_T, b = threadIdx.x % FS_GRAM_T;
        if (a < na && b < nb) {
            const double t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
            partials[((int64_t)(a0 + a) * q + (b0 + b)) * nrb + blockIdx.x] = t;
        }
    }
}

__global__ void k_block_gram_finish(int64_t entries, const double* __restrict__ partials, int nrb, double* __restrict__ G) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= entries) return;
    double t = 0.0;
    for (int g = 0; g < nrb; ++g) t += partials[e * nrb + g];
    G[e] = t;
}

// ---- Y = X C + Z D --------------------------------------------------------------------------------------------------------
// X: n x p, C: p x q row-major; Z: n x r, D: r x q (r = 0: no second term).  One row per thread; the output columns in passes
// of FS_COMBINE_Q.  Y must not overlap X or Z.
__global__ void __launch_bounds__(FS_BLOCK) k_block_combine(int64_t n, const double* __restrict__ X, int64_t ldx, int p,
                                                            const double* __restrict__ Cm, const double* __restrict__ Z,
                                                            int64_t ldz, int r, const double* __restrict__ Dm,
                                                            double* __restrict__ Y, int64_t ldy, int q) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        for (int j0 = 0; j0 < q; j0 += FS_COMBINE_Q) {
            double out[FS_COMBINE_Q];
#pragma unroll
            for (int j = 0; j < FS_COMBINE_Q; ++j) out[j] = 0.0;
            for (int a = 0; a < p; ++a) {
                const double x = X[(int64_t)a * ldx + i];
                const double* __restrict__ c = Cm + (int64_t)a * q + j0;
#pragma unroll
                for (int j = 0; j < FS_COMBINE_Q; ++j)
                    if (j0 + j < q) out[j] = fma(x, c[j], out[j]);
            }
            for (int a = 0; a < r; ++a) {
                const double z = Z[(int64_t)a * ldz + i];
                const double* __restrict__ d = Dm + (int64_t)a * q + j0;
#pragma unroll
                for (int j = 0; j < FS_COMBINE_Q; ++j)
                    if (j0 + j < q) out[j] = fma(z, d[j], out[j]);
            }
#pragma unroll
            for (int j = 0; j < FS_COMBINE_Q; ++j)
                if (j0 + j < q) Y[(int64_t)(j0 + j) * ldy + i] = out[j];
        }
    }
}

// ---- start block, masks, Jacobi ----------------------------------------------------------------------------------------
__device__ __forceinline__ double fs_seed_uniform(uint64_t seed, int64_t col, int64_t i) {
    uint64_t h = seed ^ ((uint64_t)col * 0xD1B54A32D192ED03ull) ^ ((uint64_t)i * 0x9E3779B97F4A7C15ull);   // splitmix64
    h += 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    h ^= h >> 31;
    return (double)(h >> 11) * (1.0 / 9007199254740992.0) - 0.5;
}
__global__ void k_block_seed(int64_t n, double* __restrict__ X, int64_t ld, int m, uint64_t seed, const uint8_t* __restrict__ mask) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        for (int c = 0; c < m; ++c) X[(int64_t)c * ld + i] = mask[i] ? 0.0 : fs_seed_uniform(seed, c, i);
}
__global__ void k_mask_set(int64_t count, const int32_t* __restrict__ idx, int64_t n, uint8_t* __restrict__ mask) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count && idx[e] >= 0 && idx[e] < n) mask[idx[e]] = 1;
}
// Y = dinv .* X per column (the Jacobi preconditioner), 0 on constrained rows
__global__ void k_block_scale(int64_t n, const double* __restrict__ dinv, const double* __restrict__ X, int64_t ldx,
                              double* __restrict__ Y, int64_t ldy, int m, const uint8_t* __restrict__ mask) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        for (int c = 0; c < m; ++c) Y[(int64_t)c * ldy + i] = mask[i] ? 0.0 : dinv[i] * X[(int64_t)c * ldx + i];
}
__global__ void k_block_mask(int64_t n, double* __restrict__ X, int64_t ld, int m, const uint8_t* __restrict__ mask) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (mask[i])
            for (int c = 0; c < m; ++c) X[(int64_t)c * ld + i] = 0.0;
}
// 1 / diagonal of a block matrix (0 where the diagonal is not positive: such rows are constrained or the pencil is not SPD)
template <int BS>
__global__ void k_block_dinv(int64_t n_rows, int64_t n_slices, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col,
                             const int32_t* __restrict__ dia_ptr, const int32_t* __restrict__ dia_off, const double* __restrict__ val,
                             int64_t plane, double* __restrict__ dinv) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t s = r / FS_SLICE;
    const int lane = (int)(r % FS_SLICE);
    const int64_t base = slice_ptr[s];
    const int width = (int)((slice_ptr[s + 1] - base) >> 6);
    const int32_t dp = dia_ptr[s];
    double d[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) d[i] = 0.0;
    for (int k = 0; k < width; ++k) {
        bool diag;
        if (dp >= 0) {
            const int split = dia_off[dp];
            const int32_t* op = dia_off + dp + 1;
            const int32_t o = lane >= split ? op[(split < FS_SLICE ? width : 0) + k] : op[k];
            diag = o == 0;
        } else {
            diag = sell_col[base + (int64_t)k * FS_SLICE + lane] == (int32_t)r;
        }
        if (diag)
#pragma unroll
            for (int i = 0; i < BS; ++i) d[i] = val[(int64_t)(i * BS + i) * plane + base + (int64_t)k * FS_SLICE + lane];
    }
#pragma unroll
    for (int i = 0; i < BS; ++i) dinv[r * BS + i] = d[i] > 0.0 ? 1.0 / d[i] : 0.0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
namespace {

struct blk {
    double* p = nullptr;
    int64_t ld = 0;
    double* col(int j) const { return p + (int64_t)j * ld; }
};

template <int BS, int MC>
void launch_multi(const fs_matrix_s* A, const double* X, int64_t ldx, double* Y, int64_t ldy, const uint8_t* mask, hipStream_t s) {
    const fs_space_s* sp = A->space;
    int64_t g = std::min<int64_t>((sp->n_slices + 3) / 4, 1024);
    g = (g + 7) & ~(int64_t)7;
    hipLaunchKernelGGL((k_sell_spmv_multi<BS, MC>), dim3((unsigned)g), dim3(FS_BLOCK), 0, s, sp->n_nodes_owned, sp->n_nodes_local, sp->n_slices,
                       sp->slice_ptr.p, sp->sell_col.p, sp->dia_ptr.p, sp->dia_off.p, A->val.p, sp->sell_entries, sp->slice_order.p, X, ldx, Y, ldy,
                       mask);
}
template <int BS>
void block_product_bs(const fs_matrix_s* A, int m, const double* X, int64_t ldx, double* Y, int64_t ldy, const uint8_t* mask, hipStream_t s) {
    int c = 0;
    for (; c + 8 <= m; c += 8) launch_multi<BS, 8>(A, X + c * ldx, ldx, Y + c * ldy, ldy, mask, s);
    if (c + 4 <= m) { launch_multi<BS, 4>(A, X + c * ldx, ldx, Y + c * ldy, ldy, mask, s); c += 4; }
    if (c + 2 <= m) { launch_multi<BS, 2>(A, X + c * ldx, ldx, Y + c * ldy, ldy, mask, s); c += 2; }
    if (c < m) launch_multi<BS, 1>(A, X + c * ldx, ldx, Y + c * ldy, ldy, mask, s);
}
// Y = A X for m columns (chunks of 8, 4, 2, 1)
int block_product(const fs_matrix_s* A, int m, const double* X, int64_t ldx, double* Y, int64_t ldy, const uint8_t* mask, hipStream_t s) {
    if (m <= 0) return FS_OK;
    if (A->bs == 3) block_product_bs<3>(A, m, X, ldx, Y, ldy, mask, s);
    else if (A->bs == 2) block_product_bs<2>(A, m, X, ldx, Y, ldy, mask, s);
    else FS_REQUIRE(false, "block product: block size %d (2 or 3 expected)", A->bs);
    FS_KERNEL_CHECK();
    return FS_OK;
}

template <int BS, int MC>
void launch_pencil(const fs_matrix_s* K, const double* gs, const double* X, int64_t ldx, double* YK, double* YG, int64_t ldy,
                   const uint8_t* mask, hipStream_t s) {
    const fs_space_s* sp = K->space;
    int64_t g = std::min<int64_t>((sp->n_slices + 3) / 4, 1024);
    g = (g + 7) & ~(int64_t)7;
    hipLaunchKernelGGL((k_sell_spmv_pencil<BS, MC>), dim3((unsigned)g), dim3(FS_BLOCK), 0, s, sp->n_nodes_owned, sp->n_nodes_local, sp->n_slices,
                       sp->slice_ptr.p, sp->sell_col.p, sp->dia_ptr.p, sp->dia_off.p, K->val.p, sp->sell_entries, gs, sp->slice_order.p, X, ldx,
                       YK, YG, ldy, mask);
}
template <int BS>
void pencil_product_bs(const fs_matrix_s* K, const double* gs, int m, const double* X, int64_t ldx, double* YK, double* YG, int64_t ldy,
                       const uint8_t* mask, hipStream_t s) {
    int c = 0;
    for (; c + 8 <= m; c += 8) launch_pencil<BS, 8>(K, gs, X + c * ldx, ldx, YK + c * ldy, YG + c * ldy, ldy, mask, s);
    if (c + 4 <= m) { launch_pencil<BS, 4>(K, gs, X + c * ldx, ldx, YK + c * ldy, YG + c * ldy, ldy, mask, s); c += 4; }
    if (c + 2 <= m) { launch_pencil<BS, 2>(K, gs, X + c * ldx, ldx, YK + c * ldy, YG + c * ldy, ldy, mask, s); c += 2; }
    if (c < m) launch_pencil<BS, 1>(K, gs, X + c * ldx, ldx, YK + c * ldy, YG + c * ldy, ldy, mask, s);
}
// YK = K X and YG = K_G X for m columns (chunks of 8, 4, 2, 1), K_G by its compact copy gs
int pencil_product(const fs_matrix_s* K, const double* gs, int m, const double* X, int64_t ldx, double* YK, double* YG, int64_t ldy,
                   const uint8_t* mask, hipStream_t s) {
    if (m <= 0) return FS_OK;
    if (K->bs == 3) pencil_product_bs<3>(K, gs, m, X, ldx, YK, YG, ldy, mask, s);
    else if (K->bs == 2) pencil_product_bs<2>(K, gs, m, X, ldx, YK, YG, ldy, mask, s);
    else FS_REQUIRE(false, "pencil product: block size %d (2 or 3 expected)", K->bs);
    FS_KERNEL_CHECK();
    return FS_OK;
}
// gs = the compact copy of KG (one double per stored block); refuses a matrix whose blocks are not s I.  Synchronises.
int pencil_compact(const fs_matrix_s* KG, dbuf<double>& gs, const char* who, hipStream_t s) {
    const fs_space_s* sp = KG->space;
    dbuf<int> bad;
    FS_CHECK(gs.alloc(sp->sell_entries));
    FS_CHECK(bad.alloc(1));
    FS_CHECK(bad.zero(s));
    const int grid = fs_grid_for(sp->sell_entries);
    if (KG->bs == 3) hipLaunchKernelGGL(k_pencil_compact<3>, dim3(grid), dim3(FS_BLOCK), 0, s, sp->sell_entries, KG->val.p, sp->sell_entries, gs.p, bad.p);
    else hipLaunchKernelGGL(k_pencil_compact<2>, dim3(grid), dim3(FS_BLOCK), 0, s, sp->sell_entries, KG->val.p, sp->sell_entries, gs.p, bad.p);
    FS_KERNEL_CHECK();
    int h = 0;
    FS_CHECK(bad.download(&h, 1, s));
    FS_REQUIRE(h == 0, "%s: a node-pair block of the geometric stiffness is not a multiple of the identity (was a Dirichlet condition "
               "applied to it, or is an entry not finite?)", who);
    return FS_OK;
}

struct gram_ws {
    dbuf<double> partials, G;
};
// G (host, p x q row-major) = X^T Y over n rows; synchronises
int block_gram(gram_ws& W, int64_t n, const double* X, int64_t ldx, int p, const double* Y, int64_t ldy, int q, double* G, hipStream_t s) {
    if (p <= 0 || q <= 0) return FS_OK;
    const int tiles = ((p + FS_GRAM_T - 1) / FS_GRAM_T) * ((q + FS_GRAM_T - 1) / FS_GRAM_T);
    int nrb = (int)std::min<int64_t>((n + 16 * FS_BLOCK - 1) / (16 * FS_BLOCK), std::max(8, 2048 / tiles));
    nrb = std::max(nrb, 1);
    const int64_t entries = (int64_t)p * q;
    if (W.partials.n < entries * nrb) FS_CHECK(W.partials.alloc(entries * nrb));
    if (W.G.n < entries) FS_CHECK(W.G.alloc(entries));
    hipLaunchKernelGGL(k_block_gram, dim3(nrb, tiles), dim3(FS_BLOCK), 0, s, n, X, ldx, p, Y, ldy, q, W.partials.p, nrb);
    hipLaunchKernelGGL(k_block_gram_finish, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, entries, W.partials.p, nrb, W.G.p);
    FS_KERNEL_CHECK();
    return W.G.download(G, entries, s);
}

// Y = X C + Z D (C: p x q, D: r x q, host, row-major); the coefficients go up through the staging buffer (synchronises)
int block_combine(dbuf<double>& coef, int64_t n, const double* X, int64_t ldx, int p, const double* C, const double* Z, int64_t ldz, int r,
                  const double* D, double* Y, int64_t ldy, int q, hipStream_t s) {
    if (q <= 0) return FS_OK;
    const int64_t nc = (int64_t)p * q + (int64_t)r * q;
    if (coef.n < nc) FS_CHECK(coef.alloc(nc));
    std::vector<double> h((size_t)nc);
    std::copy(C, C + (size_t)p * q, h.begin());
    if (r) std::copy(D, D + (size_t)r * q, h.begin() + (size_t)p * q);
    FS_CHECK(coef.upload(h.data(), nc, s));
    hipLaunchKernelGGL(k_block_combine, dim3(fs_grid_for(n)), dim3(FS_BLOCK), 0, s, n, X, ldx, p, coef.p, Z, ldz, r, coef.p + (int64_t)p * q, Y,
                       ldy, q);
    FS_KERNEL_CHECK();
    return FS_OK;
}

// ---- dense symmetric algebra on the host (n <= 3 * 40) --------------------------------------------------------------------
// cyclic Jacobi: A (n x n, row-major, symmetric) -> eigenvalues w (ascending) and eigenvectors V (columns, row-major n x n)
void jacobi_eigen(std::vector<double> A, int n, std::vector<double>& w, std::vector<double>& V) {
    V.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, tot = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const double a = A[(size_t)i * n + j] * A[(size_t)i * n + j];
                tot += a;
                if (i != j) off += a;
            }
        if (off <= 1e-32 * tot || off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; ++k) {       // A = J^T A J
                    const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                    A[(size_t)k * n + p] = c * akp - sn * akq;
                    A[(size_t)k * n + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
                    A[(size_t)p * n + k] = c * apk - sn * aqk;
                    A[(size_t)q * n + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
                    V[(size_t)k * n + p] = c * vkp - sn * vkq;
                    V[(size_t)k * n + q] = sn * vkp + c * vkq;
                }
            }
    }
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return A[(size_t)a * n + a] < A[(size_t)b * n + b]; });
    std::vector<double> V2((size_t)n * n);
    w.resize(n);
    for (int j = 0; j < n; ++j) {
        w[j] = A[(size_t)idx[j] * n + idx[j]];
        for (int k = 0; k < n; ++k) V2[(size_t)k * n + j] = V[(size_t)k * n + idx[j]];
    }
    V.swap(V2);
}

// A c = theta B c (B SPD): theta ascending, C (n x n row-major, columns B-orthonormal).  false: B is not positive definite.
bool gen_eigen(const std::vector<double>& A, const std::vector<double>& B, int n, std::vector<double>& theta, std::vector<double>& Cout) {
    std::vector<double> L((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double d = B[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0.0)) return false;
        L[(size_t)j * n + j] = sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double t = B[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) t -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = t / L[(size_t)j * n + j];
        }
    }
    // Y = L^-1 A, then Atil = Y L^-T
    std::vector<double> Y(A), At((size_t)n * n);
    for (int c = 0; c < n; ++c)
        for (int i = 0; i < n; ++i) {
            double t = Y[(size_t)i * n + c];
            for (int k = 0; k < i; ++k) t -= L[(size_t)i * n + k] * Y[(size_t)k * n + c];
            Y[(size_t)i * n + c] = t / L[(size_t)i * n + i];
        }
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < n; ++i) {      // At[r][i] = (Y L^-T)[r][i]: solve L z = Y[r,:]^T
            double t = Y[(size_t)r * n + i];
            for (int k = 0; k < i; ++k) t -= L[(size_t)i * n + k] * At[(size_t)r * n + k];
            At[(size_t)r * n + i] = t / L[(size_t)i * n + i];
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) At[(size_t)i * n + j] = At[(size_t)j * n + i] = 0.5 * (At[(size_t)i * n + j] + At[(size_t)j * n + i]);
    std::vector<double> Q;
    jacobi_eigen(At, n, theta, Q);
    Cout.assign((size_t)n * n, 0.0);           // C = L^-T Q
    for (int c = 0; c < n; ++c)
        for (int i = n - 1; i >= 0; --i) {
            double t = Q[(size_t)i * n + c];
            for (int k = i + 1; k < n; ++k) t -= L[(size_t)k * n + i] * Cout[(size_t)k * n + c];
            Cout[(size_t)i * n + c] = t / L[(size_t)i * n + i];
        }
    return true;
}

// Cholesky-QR coefficients with column dropping: T (k x k', row-major) with (U T)^T M (U T) = I for the Gram G = U^T M U.  A column
// whose M-norm after removing the kept ones falls below sqrt(drop) of ref[j] (its M-norm before any projection, squared) is dropped.
std::vector<double> chol_qr(const std::vector<double>& G, int k, const std::vector<double>& ref, double drop, int* kept) {
    std::vector<std::vector<double>> T;
    for (int j = 0; j < k; ++j) {
        std::vector<double> t((size_t)k, 0.0);
        t[j] = 1.0;
        for (const auto& ti : T) {              // t -= <t, ti>_G ti  (modified Gram-Schmidt in the G inner product)
            double d = 0.0;
            for (int a = 0; a < k; ++a)
                for (int b = 0; b < k; ++b) d += t[a] * G[(size_t)a * k + b] * ti[b];
            for (int a = 0; a < k; ++a) t[a] -= d * ti[a];
        }
        double nn = 0.0;
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b) nn += t[a] * G[(size_t)a * k + b] * t[b];
        if (!(nn > drop * ref[j]) || !(nn > 0.0)) continue;
        const double sc = 1.0 / sqrt(nn);
        for (auto& x : t) x *= sc;
        T.push_back(std::move(t));
    }
    *kept = (int)T.size();
    std::vector<double> out((size_t)k * T.size());
    for (size_t c = 0; c < T.size(); ++c)
        for (int a = 0; a < k; ++a) out[(size_t)a * T.size() + c] = T[c][a];
    return out;
}

// durations of one phase, collected after the stream synchronised
struct phase_time {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    double ms = 0.0;
    void start(hipStream_t s) {
        if (used + 2 > ev.size()) {
            hipEvent_t a, b;
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            ev.push_back(a);
            ev.push_back(b);
        }
        (void)hipEventRecord(ev[used], s);
    }
    void stop(hipStream_t s) {
        (void)hipEventRecord(ev[used + 1], s);
        used += 2;
    }
    void collect() {
        for (size_t i = 0; i + 1 < used; i += 2) {
            float t = 0.f;
            if (hipEventSynchronize(ev[i + 1]) == hipSuccess && hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) ms += t;
        }
        used = 0;
    }
    ~phase_time() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
};

// basis S and its products with the two matrices of the pencil A x = theta B x (AS = A S, BS = B S): 3 blocks of cap columns each
struct triple {
    dbuf<double> store;
    blk S, AS, BS;
    int alloc(int64_t ld, int cap) {
        FS_CHECK(store.alloc(3 * ld * cap));
        S.p = store.p; AS.p = store.p + ld * cap; BS.p = store.p + 2 * ld * cap;
        S.ld = AS.ld = BS.ld = ld;
        return FS_OK;
    }
};

// The pencil A x = theta B x of one LOBPCG run: A symmetric, B symmetric positive definite on the free dofs.
//   fs_eigen_solve:     A = K (+ shift M), B = M; the Jacobi diagonal is A's; B is well conditioned.
//   fs_buckling_solve:  A = K_G, B = K;           the Jacobi diagonal is B's; B is not.
struct lobpcg_pencil {
    const fs_matrix_s* A = nullptr;
    const fs_matrix_s* B = nullptr;
    const fs_matrix_s* D = nullptr;     // the matrix whose diagonal the Jacobi preconditioner inverts (no V-cycle given)
    const double* gs = nullptr;         // compact copy of A (k_pencil_compact): A S and B S of the same columns in one pass
                                        // (k_sell_spmv_pencil, B as its K); nullptr: two passes of k_sell_spmv_multi
    bool recompute_b = false;           // B S of freshly orthonormalised columns by a product, not by the combination
    const char* who = "";               // for error messages
};
struct lobpcg_stats {
    int iterations = 0, n_converged = 0;
    double max_rel_residual = 0.0, solve_ms = 0.0, block_product_ms = 0.0, gram_ms = 0.0, precond_ms = 0.0;
};

}  // namespace

extern "C" int fs_spmv_multi(fs_matrix_t A, int m, const fs_vector_t* X, fs_vector_t* Y) {
    FS_REFUSE_DG(A, "fs_spmv_multi");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(A && X && Y && m >= 1, "fs_spmv_multi: bad arguments");
    FS_REQUIRE(A->bs == 2 || A->bs == 3, "fs_spmv_multi: block size %d (2 or 3 expected)", A->bs);
    fs_space_s* sp = A->space;
    FS_REQUIRE(!sp->halo.active, "fs_spmv_multi: a decomposed space (several ranks) is not supported");
    const int64_t nl = sp->n_dofs_local, no = sp->n_dofs_owned, ld = (nl + 1) & ~(int64_t)1;
    for (int j = 0; j < m; ++j) {
        FS_REQUIRE(X[j] && Y[j], "fs_spmv_multi: null vector");
        FS_REQUIRE(X[j]->d.n >= nl && Y[j]->d.n >= no, "fs_spmv_multi: vector %d too short", j);
    }
    hipStream_t s = fs_rt().stream;
    dbuf<double> xb, yb;
    FS_CHECK(xb.alloc(ld * m));
    FS_CHECK(yb.alloc(ld * m));
    for (int j = 0; j < m; ++j) FS_HIP(hipMemcpyAsync(xb.p + j * ld, X[j]->d.p, nl * sizeof(double), hipMemcpyDeviceToDevice, s));
    FS_CHECK(block_product(A, m, xb.p, ld, yb.p, ld, nullptr, s));
    for (int j = 0; j < m; ++j) FS_HIP(hipMemcpyAsync(Y[j]->d.p, yb.p + j * ld, no * sizeof(double), hipMemcpyDeviceToDevice, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_vector_gram(int p, const fs_vector_t* X, int q, const fs_vector_t* Y, double* G) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(X && Y && G && p >= 1 && q >= 1, "fs_vector_gram: bad arguments");
    FS_REQUIRE(X[0], "fs_vector_gram: null vector");
    const int64_t n = X[0]->d.n, ld = (n + 1) & ~(int64_t)1;
    for (int j = 0; j < p; ++j) FS_REQUIRE(X[j] && X[j]->d.n == n, "fs_vector_gram: X[%d] is null or of another length", j);
    for (int j = 0; j < q; ++j) FS_REQUIRE(Y[j] && Y[j]->d.n == n, "fs_vector_gram: Y[%d] is null or of another length", j);
    hipStream_t s = fs_rt().stream;
    dbuf<double> xb, yb;
    FS_CHECK(xb.alloc(ld * p));
    FS_CHECK(yb.alloc(ld * q));
    for (int j = 0; j < p; ++j) FS_HIP(hipMemcpyAsync(xb.p + j * ld, X[j]->d.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (int j = 0; j < q; ++j) FS_HIP(hipMemcpyAsync(yb.p + j * ld, Y[j]->d.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    gram_ws W;
    return block_gram(W, n, xb.p, ld, p, yb.p, ld, q, G, s);
}

namespace {

// what fs_eigen_solve and fs_buckling_solve check alike: the space, one rank, the block, the constrained list, the vectors
int lobpcg_check(const lobpcg_pencil& P, fs_amg_t precond, int64_t n_constrained, const int32_t* constrained, int nm, int block, double tol,
                 int max_iter, fs_vector_t* modes, int* m_out) {
    FS_REQUIRE(P.A->space == P.B->space, "%s: the two matrices must share their space", P.who);
    FS_REQUIRE(P.A->bs == P.B->bs && (P.A->bs == 2 || P.A->bs == 3), "%s: block size %d (2 or 3 expected)", P.who, P.A->bs);
    const fs_space_s* sp = P.A->space;
    FS_REQUIRE(!sp->halo.active && fs_rt().n_ranks == 1, "%s: several ranks are not supported", P.who);
    const int m = block > 0 ? block : std::min(2 * nm, nm + 8);
    const int64_t n = sp->n_dofs_owned;
    FS_REQUIRE(nm >= 1 && nm <= 32 && m >= nm && m <= 40, "%s: n_modes %d / block %d out of range", P.who, nm, m);
    FS_REQUIRE(n_constrained >= 0 && (n_constrained == 0 || constrained), "%s: bad constrained list", P.who);
    FS_REQUIRE(n - n_constrained > m, "%s: %lld dofs, %lld constrained: too few for a block of %d", P.who, (long long)n,
               (long long)n_constrained, m);
    FS_REQUIRE(tol > 0.0 && max_iter >= 1, "%s: tol and max_iter must be positive", P.who);
    if (precond) FS_REQUIRE(fs_amg_rows(precond) == n, "%s: the preconditioner has %lld rows, the matrices %lld", P.who, (long long)fs_amg_rows(precond), (long long)n);
    for (int j = 0; j < nm; ++j) FS_REQUIRE(modes[j] && modes[j]->d.n >= n, "%s: mode vector %d missing or too short", P.who, j);
    *m_out = m;
    return FS_OK;
}

// The m lowest Ritz pairs of the pencil P on the dofs outside `constrained`, iterated until the first nm columns meet
// ||A x - theta B x||_2 <= tol |theta| ||B x||_2 on products recomputed from X.  theta[m] ascending; modes[nm] B-orthonormal.
int lobpcg(const lobpcg_pencil& P, fs_amg_t precond, int64_t n_constrained, const int32_t* constrained, int nm, int m, double tol, int max_iter,
           uint64_t seed, std::vector<double>& theta, fs_vector_t* modes, lobpcg_stats* stats) {
    const fs_space_s* sp = P.A->space;
    const int64_t n = sp->n_dofs_owned, ld = (n + 1) & ~(int64_t)1;
    *stats = lobpcg_stats();
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = fs_rt().stream;

    dbuf<uint8_t> mask;
    dbuf<int32_t> cidx;
    dbuf<double> dinv, coef, Rb;
    FS_CHECK(mask.alloc(n));
    FS_CHECK(mask.zero(s));
    if (n_constrained) {
        FS_CHECK(cidx.alloc(n_constrained));
        FS_CHECK(cidx.upload(constrained, n_constrained, s));
        hipLaunchKernelGGL(k_mask_set, dim3((unsigned)((n_constrained + 255) / 256)), dim3(256), 0, s, n_constrained, cidx.p, n, mask.p);
    }
    if (!precond) {
        FS_CHECK(dinv.alloc(n));
        if (P.D->bs == 3)
            hipLaunchKernelGGL(k_block_dinv<3>, dim3((unsigned)((sp->n_nodes_owned + 255) / 256)), dim3(256), 0, s, sp->n_nodes_owned, sp->n_slices,
                               sp->slice_ptr.p, sp->sell_col.p, sp->dia_ptr.p, sp->dia_off.p, P.D->val.p, sp->sell_entries, dinv.p);
        else
            hipLaunchKernelGGL(k_block_dinv<2>, dim3((unsigned)((sp->n_nodes_owned + 255) / 256)), dim3(256), 0, s, sp->n_nodes_owned, sp->n_slices,
                               sp->slice_ptr.p, sp->sell_col.p, sp->dia_ptr.p, sp->dia_off.p, P.D->val.p, sp->sell_entries, dinv.p);
    }
    const int cap = 3 * m;
    triple A_, T_;
    FS_CHECK(A_.alloc(ld, cap));
    FS_CHECK(T_.alloc(ld, cap));
    FS_CHECK(Rb.alloc(ld * m));
    triple* A = &A_;
    triple* T = &T_;
    gram_ws gw;
    phase_time t_prod, t_gram, t_pre;
    const int grid = fs_grid_for(n);

    auto prod_with = [&](const fs_matrix_s* B, const blk& out, int c0, int k) -> int {      // out = B S for columns [c0, c0 + k)
        t_prod.start(s);
        FS_CHECK(block_product(B, k, A->S.col(c0), ld, out.col(c0), ld, mask.p, s));
        t_prod.stop(s);
        return FS_OK;
    };
    auto prod_a = [&](int c0, int k) { return prod_with(P.A, A->AS, c0, k); };
    auto prod_b = [&](int c0, int k) { return prod_with(P.B, A->BS, c0, k); };
    auto prod_ab = [&](int c0, int k) -> int {                   // A S and B S of the same columns: one pass where A has its compact copy
        if (!P.gs) {
            FS_CHECK(prod_a(c0, k));
            return prod_b(c0, k);
        }
        t_prod.start(s);
        FS_CHECK(pencil_product(P.B, P.gs, k, A->S.col(c0), ld, A->BS.col(c0), A->AS.col(c0), ld, mask.p, s));
        t_prod.stop(s);
        return FS_OK;
    };
    // after orthonormalize(): A S of the new columns, and B S again where the combination of an ill-conditioned B S is not kept
    auto prod_new = [&](int c0, int k) { return P.recompute_b ? prod_ab(c0, k) : prod_a(c0, k); };
    auto gram = [&](const double* X, int p, const double* Y, int q, std::vector<double>& G) -> int {
        G.assign((size_t)p * q, 0.0);
        t_gram.start(s);
        const int rc = block_gram(gw, n, X, ld, p, Y, ld, q, G.data(), s);
        t_gram.stop(s);
        return rc;
    };
    // columns [c0, c0 + k) of the blocks of `from` -> columns [o0, o0 + q) of `to`: times Cm (+ columns [z0, z0 + r) times Dm).
    // nb = 3: S, B S and A S; nb = 2: S and B S only (A S of those columns is not formed yet)
    auto combine = [&](int nb, triple* from, int c0, int k, const std::vector<double>& Cm, int z0, int r, const std::vector<double>* Dm,
                       triple* to, int o0, int q) -> int {
        const blk* fb[3] = {&from->S, &from->BS, &from->AS};
        const blk* tb[3] = {&to->S, &to->BS, &to->AS};
        for (int b = 0; b < nb; ++b)
            FS_CHECK(block_combine(coef, n, fb[b]->col(c0), ld, k, Cm.data(), r ? fb[b]->col(z0) : nullptr, ld, r, r ? Dm->data() : nullptr,
                                   tb[b]->col(o0), ld, q, s));
        return FS_OK;
    };
    // B-orthonormalise columns [u0, u0 + k) of S (with B S) against columns [0, u0) (B-orthonormal already) and among themselves:
    // Cholesky-QR applied twice, collapsed columns dropped; *kept = columns left.  Only S and B S are combined, and A S of these
    // columns is computed afterwards by a product, never by a combination (rounding in A U T grows with |T| |A|, which stalls the
    // residuals of large problems).  For the mass matrix as B, well conditioned, the combined B S is kept; for a stiffness matrix as B
    // (P.recompute_b) the same rounding applies to it, and prod_new() forms B S of the kept columns again with A S.
    auto orthonormalize = [&](int u0, int k, int* kept) -> int {
        std::vector<double> H, G;
        for (int pass = 0; pass < 2 && k > 0; ++pass) {
            std::vector<double> ref((size_t)k, 0.0);
            std::vector<double> Ik((size_t)k * k, 0.0);
            for (int j = 0; j < k; ++j) Ik[(size_t)j * k + j] = 1.0;
            if (u0 > 0) {
                FS_CHECK(gram(A->BS.col(0), u0, A->S.col(u0), k, H));        // H = S0^T B U
                std::vector<double> nH(H.size());
                for (size_t e = 0; e < H.size(); ++e) nH[e] = -H[e];
                FS_CHECK(combine(2, A, u0, k, Ik, 0, u0, &nH, T, u0, k));     // U - S0 H
                for (int j = 0; j < k; ++j)
                    for (int i = 0; i < u0; ++i) ref[j] += H[(size_t)i * k + j] * H[(size_t)i * k + j];
            } else {
                FS_CHECK(combine(2, A, u0, k, Ik, 0, 0, nullptr, T, u0, k));
            }
            FS_CHECK(gram(T->S.col(u0), k, T->BS.col(u0), k, G));
            for (int i = 0; i < k; ++i)
                for (int j = 0; j < i; ++j) G[(size_t)i * k + j] = G[(size_t)j * k + i] = 0.5 * (G[(size_t)i * k + j] + G[(size_t)j * k + i]);
            for (int j = 0; j < k; ++j) ref[j] += G[(size_t)j * k + j];
            int kk = 0;
            std::vector<double> Tc = chol_qr(G, k, ref, FS_EIGEN_DROP, &kk);
            if (kk) FS_CHECK(combine(2, T, u0, k, Tc, 0, 0, nullptr, A, u0, kk));
            k = kk;
        }
        *kept = k;
        return FS_OK;
    };

    theta.assign((size_t)m, 0.0);
    std::vector<double> rel((size_t)m, 0.0);
    // Rayleigh-Ritz on S = A[0, nS) (B-orthonormal): X <- S C_x.  The new P spans the [P W] parts of the active Ritz vectors, taken
    // B-orthonormal to C_x in coefficient space (Hetmaniuk & Lehoucq 2006; Duersch et al. 2018), so that [X P] stays B-orthonormal and
    // every combination has coefficients of norm about 1.  Returns the new P count.
    auto rayleigh_ritz = [&](int nS, const std::vector<int>& act, int* pk) -> int {
        std::vector<double> GA, GB, th, Cfull;
        FS_CHECK(gram(A->S.col(0), nS, A->AS.col(0), nS, GA));
        FS_CHECK(gram(A->S.col(0), nS, A->BS.col(0), nS, GB));
        for (int i = 0; i < nS; ++i)
            for (int j = 0; j < i; ++j) {
                GA[(size_t)i * nS + j] = GA[(size_t)j * nS + i] = 0.5 * (GA[(size_t)i * nS + j] + GA[(size_t)j * nS + i]);
                GB[(size_t)i * nS + j] = GB[(size_t)j * nS + i] = 0.5 * (GB[(size_t)i * nS + j] + GB[(size_t)j * nS + i]);
            }
        if (!gen_eigen(GA, GB, nS, th, Cfull)) {
            fs_set_error("%s: the Gram matrix of the basis is not positive definite", P.who);
            return FS_ERR_NUMERIC;
        }
        std::vector<double> Cx((size_t)nS * m);
        for (int i = 0; i < nS; ++i)
            for (int j = 0; j < m; ++j) Cx[(size_t)i * m + j] = Cfull[(size_t)i * nS + j];
        FS_CHECK(combine(3, A, 0, nS, Cx, 0, 0, nullptr, T, 0, m));
        *pk = 0;
        const int a = (int)act.size();
        if (nS > m && a) {
            // Z = the [P W] rows of the active Ritz coefficients; Z <- Z - C_x (C_x^T B Z), then B-orthonormal (twice, with drops)
            std::vector<double> Z((size_t)nS * a, 0.0), BZ, Zref((size_t)a, 0.0);
            for (int i = m; i < nS; ++i)
                for (int j = 0; j < a; ++j) Z[(size_t)i * a + j] = Cfull[(size_t)i * nS + act[j]];
            int na = a;
            for (int pass = 0; pass < 2 && na > 0; ++pass) {
                auto bmul = [&](const std::vector<double>& Y, int q) {          // B Y (nS x q)
                    std::vector<double> out((size_t)nS * q, 0.0);
                    for (int i = 0; i < nS; ++i)
                        for (int k2 = 0; k2 < nS; ++k2) {
                            const double b = GB[(size_t)i * nS + k2];
                            for (int j = 0; j < q; ++j) out[(size_t)i * q + j] += b * Y[(size_t)k2 * q + j];
                        }
                    return out;
                };
                BZ = bmul(Z, na);
                std::vector<double> H((size_t)m * na, 0.0);
                for (int c = 0; c < m; ++c)
                    for (int i = 0; i < nS; ++i)
                        for (int j = 0; j < na; ++j) H[(size_t)c * na + j] += Cx[(size_t)i * m + c] * BZ[(size_t)i * na + j];
                std::vector<double> ref((size_t)na, 0.0);
                for (int j = 0; j < na; ++j) {
                    for (int i = 0; i < nS; ++i) ref[j] += Z[(size_t)i * na + j] * BZ[(size_t)i * na + j];
                }
                for (int i = 0; i < nS; ++i)
                    for (int j = 0; j < na; ++j)
                        for (int c = 0; c < m; ++c) Z[(size_t)i * na + j] -= Cx[(size_t)i * m + c] * H[(size_t)c * na + j];
                BZ = bmul(Z, na);
                std::vector<double> Gz((size_t)na * na, 0.0);
                for (int a1 = 0; a1 < na; ++a1)
                    for (int b1 = 0; b1 < na; ++b1)
                        for (int i = 0; i < nS; ++i) Gz[(size_t)a1 * na + b1] += Z[(size_t)i * na + a1] * BZ[(size_t)i * na + b1];
                for (int i = 0; i < na; ++i)
                    for (int j = 0; j < i; ++j) Gz[(size_t)i * na + j] = Gz[(size_t)j * na + i] = 0.5 * (Gz[(size_t)i * na + j] + Gz[(size_t)j * na + i]);
                int kk = 0;
                std::vector<double> Tz = chol_qr(Gz, na, ref, FS_EIGEN_DROP, &kk);
                std::vector<double> Zn((size_t)nS * kk, 0.0);
                for (int i = 0; i < nS; ++i)
                    for (int c = 0; c < kk; ++c)
                        for (int j = 0; j < na; ++j) Zn[(size_t)i * kk + c] += Z[(size_t)i * na + j] * Tz[(size_t)j * kk + c];
                Z.swap(Zn);
                na = kk;
            }
            if (na) FS_CHECK(combine(3, A, 0, nS, Z, 0, 0, nullptr, T, m, na));
            *pk = na;
        }
        for (int j = 0; j < m; ++j) theta[j] = th[j];
        std::swap(A, T);
        return FS_OK;
    };

    // start: seeded block, B-orthonormal, Ritz vectors of its span
    hipLaunchKernelGGL(k_block_seed, dim3(grid), dim3(FS_BLOCK), 0, s, n, A->S.p, ld, m, seed, mask.p);
    FS_KERNEL_CHECK();
    FS_CHECK(prod_b(0, m));
    int kept = 0, pk = 0;
    FS_CHECK(orthonormalize(0, m, &kept));
    FS_REQUIRE(kept == m, "%s: the start block is rank deficient (%d of %d columns)", P.who, kept, m);
    FS_CHECK(prod_new(0, m));
    FS_CHECK(rayleigh_ritz(m, std::vector<int>(), &pk));

    const bool debug = getenv("FS_EIGEN_DEBUG") != nullptr;      // per iteration: theta / relative residual of the wanted columns
    bool fresh = false, converged = false;
    int stats_restarts = 0;
    int it = 0;
    std::vector<double> G, Lm((size_t)m * m, 0.0), Im((size_t)m * m, 0.0);
    for (int j = 0; j < m; ++j) Im[(size_t)j * m + j] = 1.0;
    const int64_t ldr = ld;
    for (;;) {
        // R = A X - B X Theta and the norms of the stopping test
        for (int j = 0; j < m; ++j) Lm[(size_t)j * m + j] = -theta[j];
        FS_CHECK(block_combine(coef, n, A->AS.col(0), ld, m, Im.data(), A->BS.col(0), ld, m, Lm.data(), Rb.p, ldr, m, s));
        std::vector<double> RR, MM;
        FS_CHECK(gram(Rb.p, m, Rb.p, m, RR));
        FS_CHECK(gram(A->BS.col(0), m, A->BS.col(0), m, MM));
        std::vector<int> act;
        int nconv = 0;
        double worst = 0.0;
        for (int j = 0; j < m; ++j) {
            const double den = fabs(theta[j]) * sqrt(std::max(MM[(size_t)j * m + j], 0.0));
            rel[j] = den > 0.0 ? sqrt(std::max(RR[(size_t)j * m + j], 0.0)) / den : INFINITY;
            if (j < nm) {
                worst = std::max(worst, rel[j]);
                nconv += rel[j] <= tol;
            }
            if (!(rel[j] <= tol)) act.push_back(j);
        }
        stats->n_converged = nconv;
        stats->max_rel_residual = worst;
        if (debug) {
            fprintf(stderr, "[fs_eigen] it %d%s pk %d:", it, fresh ? " (fresh)" : "", pk);
            for (int j = 0; j < nm; ++j) fprintf(stderr, " %.6e/%.1e", theta[j], rel[j]);
            fprintf(stderr, "\n");
        }
        if (nconv == nm) {
            if (fresh) { converged = true; break; }
            // the combinations drift: recompute A X and B X from X and test again
            FS_CHECK(prod_ab(0, m));
            fresh = true;
            continue;
        }
        fresh = false;
        if (it >= max_iter) break;
        ++it;
        // W = T R on the active columns, after P
        const int a = (int)act.size(), w0 = m + pk;
        t_pre.start(s);
        for (int j = 0; j < a; ++j) {
            double* rj = Rb.p + (int64_t)act[j] * ldr;
            double* wj = A->S.col(w0 + j);
            if (precond) FS_CHECK(fs_amg_apply_dev(precond, rj, wj, s));
            else hipLaunchKernelGGL(k_block_scale, dim3(grid), dim3(FS_BLOCK), 0, s, n, dinv.p, rj, ldr, wj, ld, 1, mask.p);
        }
        if (precond) hipLaunchKernelGGL(k_block_mask, dim3(grid), dim3(FS_BLOCK), 0, s, n, A->S.col(w0), ld, a, mask.p);
        FS_KERNEL_CHECK();
        t_pre.stop(s);
        FS_CHECK(prod_b(w0, a));
        int k = 0;
        FS_CHECK(orthonormalize(w0, a, &k));
        FS_CHECK(prod_new(w0, k));
        const int rc = rayleigh_ritz(w0 + k, act, &pk);
        if (rc == FS_ERR_NUMERIC) {
            // [X P W] lost its B-orthonormality: restart from the Ritz vectors of X alone, without P
            FS_CHECK(prod_ab(0, m));
            FS_CHECK(rayleigh_ritz(m, std::vector<int>(), &pk));
            ++stats_restarts;
        } else if (rc != FS_OK) {
            return rc;
        }
        if (it % FS_EIGEN_REFRESH == 0) FS_CHECK(prod_ab(0, m));
        t_prod.collect();
        t_gram.collect();
        t_pre.collect();
    }
    for (int j = 0; j < nm; ++j) FS_HIP(hipMemcpyAsync(modes[j]->d.p, A->S.col(j), n * sizeof(double), hipMemcpyDeviceToDevice, s));
    FS_HIP(hipStreamSynchronize(s));
    t_prod.collect();
    t_gram.collect();
    t_pre.collect();
    stats->iterations = it;
    stats->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->block_product_ms = t_prod.ms;
    stats->gram_ms = t_gram.ms;
    stats->precond_ms = t_pre.ms;
    (void)converged;
    if (stats_restarts && getenv("FS_EIGEN_DEBUG")) fprintf(stderr, "[fs_eigen] %d restarts without P\n", stats_restarts);
    return FS_OK;
}

}  // namespace

extern "C" int fs_eigen_solve(fs_matrix_t K, fs_matrix_t M, fs_amg_t precond, int64_t n_constrained, const int32_t* constrained,
                              const fs_eigen_opts* opts, double* eigenvalues, fs_vector_t* modes, fs_eigen_stats* stats) {
    FS_REFUSE_DG(K, "fs_eigen_solve"); FS_REFUSE_DG(M, "fs_eigen_solve");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(K && M && opts && eigenvalues && modes && stats, "fs_eigen_solve: null pointer");
    lobpcg_pencil P;
    P.A = K; P.B = M; P.D = K; P.who = "fs_eigen_solve";
    int m = 0;
    FS_CHECK(lobpcg_check(P, precond, n_constrained, constrained, opts->n_modes, opts->block, opts->tol, opts->max_iter, modes, &m));
    memset(stats, 0, sizeof(*stats));
    std::vector<double> theta;
    lobpcg_stats st;
    const int rc = lobpcg(P, precond, n_constrained, constrained, opts->n_modes, m, opts->tol, opts->max_iter, (uint64_t)opts->seed, theta, modes, &st);
    stats->iterations = st.iterations; stats->n_converged = st.n_converged; stats->max_rel_residual = st.max_rel_residual;
    stats->solve_ms = st.solve_ms; stats->block_product_ms = st.block_product_ms; stats->gram_ms = st.gram_ms; stats->precond_ms = st.precond_ms;
    FS_CHECK(rc);
    for (int j = 0; j < opts->n_modes; ++j) eigenvalues[j] = theta[j] - opts->shift;
    return FS_OK;
}

// ---- linear buckling ---------------------------------------------------------------------------------------------------------
// (K + lambda K_G) phi = 0 as the lowest end of K_G phi = nu K phi: the most negative nu are the smallest positive lambda = -1 / nu.
// K is the SPD "B" of the Rayleigh-Ritz, K_G the indefinite "A"; the V-cycle (or the Jacobi diagonal) is K's.
extern "C" int fs_spmv_multi_pencil(fs_matrix_t K, fs_matrix_t KG, int m, const fs_vector_t* X, fs_vector_t* YK, fs_vector_t* YG) {
    FS_REFUSE_DG(K, "fs_spmv_multi_pencil"); FS_REFUSE_DG(KG, "fs_spmv_multi_pencil");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(K && KG && X && YK && YG && m >= 1, "fs_spmv_multi_pencil: bad arguments");
    FS_REQUIRE(K->space == KG->space && K->bs == KG->bs, "fs_spmv_multi_pencil: K and K_G must share their space");
    FS_REQUIRE(K->bs == 2 || K->bs == 3, "fs_spmv_multi_pencil: block size %d (2 or 3 expected)", K->bs);
    fs_space_s* sp = K->space;
    FS_REQUIRE(!sp->halo.active, "fs_spmv_multi_pencil: a decomposed space (several ranks) is not supported");
    const int64_t nl = sp->n_dofs_local, no = sp->n_dofs_owned, ld = (nl + 1) & ~(int64_t)1;
    for (int j = 0; j < m; ++j) {
        FS_REQUIRE(X[j] && YK[j] && YG[j], "fs_spmv_multi_pencil: null vector");
        FS_REQUIRE(X[j]->d.n >= nl && YK[j]->d.n >= no && YG[j]->d.n >= no, "fs_spmv_multi_pencil: vector %d too short", j);
    }
    hipStream_t s = fs_rt().stream;
    dbuf<double> gs, xb, yk, yg;
    FS_CHECK(pencil_compact(KG, gs, "fs_spmv_multi_pencil", s));
    FS_CHECK(xb.alloc(ld * m));
    FS_CHECK(yk.alloc(ld * m));
    FS_CHECK(yg.alloc(ld * m));
    for (int j = 0; j < m; ++j) FS_HIP(hipMemcpyAsync(xb.p + j * ld, X[j]->d.p, nl * sizeof(double), hipMemcpyDeviceToDevice, s));
    FS_CHECK(pencil_product(K, gs.p, m, xb.p, ld, yk.p, yg.p, ld, nullptr, s));
    for (int j = 0; j < m; ++j) {
        FS_HIP(hipMemcpyAsync(YK[j]->d.p, yk.p + j * ld, no * sizeof(double), hipMemcpyDeviceToDevice, s));
        FS_HIP(hipMemcpyAsync(YG[j]->d.p, yg.p + j * ld, no * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// the fused product against the two block products it replaces, for m columns of a seeded block: HIP events around reps launches
// of each after 3 warm-up launches, the mean per product pair in milliseconds
extern "C" int fs_spmv_multi_pencil_benchmark(fs_matrix_t K, fs_matrix_t KG, int m, int reps, double* fused_ms, double* two_pass_ms) {
    FS_REFUSE_DG(K, "fs_spmv_multi_pencil_benchmark"); FS_REFUSE_DG(KG, "fs_spmv_multi_pencil_benchmark");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(K && KG && fused_ms && two_pass_ms && m >= 1 && m <= 40 && reps >= 1, "fs_spmv_multi_pencil_benchmark: bad arguments");
    FS_REQUIRE(K->space == KG->space && K->bs == KG->bs && (K->bs == 2 || K->bs == 3), "fs_spmv_multi_pencil_benchmark: K and K_G must "
               "share a space of block size 2 or 3");
    fs_space_s* sp = K->space;
    FS_REQUIRE(!sp->halo.active, "fs_spmv_multi_pencil_benchmark: a decomposed space (several ranks) is not supported");
    const int64_t nl = sp->n_dofs_local, ld = (nl + 1) & ~(int64_t)1;
    hipStream_t s = fs_rt().stream;
    dbuf<double> gs, xb, yk, yg;
    dbuf<uint8_t> none;
    FS_CHECK(pencil_compact(KG, gs, "fs_spmv_multi_pencil_benchmark", s));
    FS_CHECK(xb.alloc(ld * m));
    FS_CHECK(yk.alloc(ld * m));
    FS_CHECK(yg.alloc(ld * m));
    FS_CHECK(none.alloc(nl));
    FS_CHECK(none.zero(s));
    hipLaunchKernelGGL(k_block_seed, dim3(fs_grid_for(nl)), dim3(FS_BLOCK), 0, s, nl, xb.p, ld, m, (uint64_t)2024, none.p);
    FS_KERNEL_CHECK();
    hipEvent_t e0, e1;
    FS_HIP(hipEventCreate(&e0));
    FS_HIP(hipEventCreate(&e1));
    int rc = FS_OK;
    for (int variant = 0; variant < 2 && rc == FS_OK; ++variant) {
        for (int i = -3; i < reps && rc == FS_OK; ++i) {
            if (i == 0) (void)hipEventRecord(e0, s);
            if (variant == 0) {
                rc = pencil_product(K, gs.p, m, xb.p, ld, yk.p, yg.p, ld, nullptr, s);
            } else {
                rc = block_product(K, m, xb.p, ld, yk.p, ld, nullptr, s);
                if (rc == FS_OK) rc = block_product(KG, m, xb.p, ld, yg.p, ld, nullptr, s);
            }
        }
        (void)hipEventRecord(e1, s);
        float t = 0.f;
        if (rc == FS_OK && (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)) {
            fs_set_error("fs_spmv_multi_pencil_benchmark: the event timing failed");
            rc = FS_ERR_HIP;
        }
        *(variant == 0 ? fused_ms : two_pass_ms) = (double)t / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

extern "C" int fs_buckling_solve(fs_matrix_t K, fs_matrix_t KG, fs_amg_t precond, int64_t n_constrained, const int32_t* constrained,
                                 const fs_buckling_opts* opts, double* factors, fs_vector_t* modes, fs_buckling_stats* stats) {
    FS_REFUSE_DG(K, "fs_buckling_solve"); FS_REFUSE_DG(KG, "fs_buckling_solve");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(K && KG && opts && factors && modes && stats, "fs_buckling_solve: null pointer");
    lobpcg_pencil P;
    P.A = KG; P.B = K; P.D = K; P.recompute_b = true; P.who = "fs_buckling_solve";
    int m = 0;
    const int nm = opts->n_modes;
    FS_CHECK(lobpcg_check(P, precond, n_constrained, constrained, nm, opts->block, opts->tol, opts->max_iter, modes, &m));
    memset(stats, 0, sizeof(*stats));
    hipStream_t s = fs_rt().stream;
    dbuf<double> gs;
    FS_CHECK(pencil_compact(KG, gs, "fs_buckling_solve", s));      // always: the check that every block of K_G is s I
    if (opts->two_pass == 0) P.gs = gs.p;
    std::vector<double> nu;
    lobpcg_stats st;
    const int rc = lobpcg(P, precond, n_constrained, constrained, nm, m, opts->tol, opts->max_iter, (uint64_t)opts->seed, nu, modes, &st);
    stats->iterations = st.iterations; stats->n_converged = st.n_converged; stats->max_rel_residual = st.max_rel_residual;
    stats->solve_ms = st.solve_ms; stats->block_product_ms = st.block_product_ms; stats->gram_ms = st.gram_ms; stats->precond_ms = st.precond_ms;
    FS_CHECK(rc);
    int n_negative = 0;
    for (int j = 0; j < m; ++j) n_negative += nu[j] < 0.0;
    stats->n_negative = n_negative;
    for (int j = 0; j < nm; ++j) factors[j] = nu[j] < 0.0 ? -1.0 / nu[j] : 0.0;
    if (st.n_converged == nm && n_negative < nm) {
        fs_set_error("fs_buckling_solve: the reference load produces only %d buckling mode(s)", n_negative);
        return FS_ERR_NUMERIC;
    }
    return FS_OK;
}
