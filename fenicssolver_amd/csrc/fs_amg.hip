// Smoothed-aggregation algebraic multigrid for libfsamd.so (gfx950).
//
// Replaces what SolverBase.solve_amg() asks of PETSc (FenicsSolver/SolverBase.py:643-672):
//   PETScPreconditioner("petsc_amg")  = GAMG smoothed aggregation with the rigid-body near-null space
//                                       of build_nullspace() (:674-706),
//   mg_levels_ksp_type chebyshev + mg_levels_pc_type jacobi (2 steps, bounds 0.1/1.1 of the
//   estimated largest eigenvalue of D^-1 A), CG outside.
//
// Everything but the final dense factorisation of the (<= a few hundred dof) coarsest operator runs
// on the device:
//   strength graph -> MIS(2) aggregation (Bell/Dalton/Olson: roots are a distance-2 maximal
//   independent set found with hashed 64-bit keys, deterministic) -> per-aggregate QR of the near-null
//   space (tentative prolongator T, coarse near-null space R) -> P = (I - 4/(3 lmax) D^-1 A) T ->
//   A_c = P^T A P.
// The two sparse products are row-wise SpGEMMs: one workgroup (or wave) per output row, the distinct
// columns of a row found with an LDS hash, the numeric pass accumulating into an LDS-resident row
// (this is where the 160 KB LDS of a CDNA4 CU pays: a 6x6-block coarse row of ~100 blocks is 29 KB).
// Level matrices are block CSR (block = dofs of a node: 1, 3 on the fine level, nb = 6 on the
// coarse levels of elasticity).  The fine level's SpMV is the tuned SELL/DIA kernel.
#include "fs_kernels.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <chrono>
#include <stdlib.h>
#include <cmath>
#include <vector>


// ---- block CSR -----------------------------------------------------------------------------------
struct bcsr {
    int64_t nrows = 0, ncols = 0;   // in blocks
    int br = 1, bc = 1;
    int64_t nnz = 0;                // blocks
    dbuf<int32_t> rowptr, col;
    dbuf<double> val;               // [nnz][br][bc]
    dbuf<float> val32;              // the same rounded to fp32 (levels >= 1 and transfer operators of a finished hierarchy: what the
                                    // V-cycle streams; the fp64 values stay for the set-up of the next level and for inspection)
};

struct amg_level {
    int64_t nn = 0;       // nodes
    int bs = 1;           // dofs per node
    int64_t n = 0;        // dofs
    int nb = 1;           // near-null-space vectors = dofs per node of the next level
    bcsr A;
    bcsr P;               // nn x n_agg, blocks bs x nb
    int64_t n_agg = 0;
    dbuf<int32_t> agg;    // [nn] aggregate of every node, -1 = in none (no strong coupling); inspection hook (fs_amg_level_get, which = 4)
    dbuf<int32_t> pt_ptr, pt_entry, pt_row;   // transpose index of P (entries sorted by column)
    dbuf<double> rt_val;  // R = P^T blocks [nb][bs] in pt order: the restriction streams them contiguously
    dbuf<float> rt_val32; // rounded to fp32 (the SAME rounded numbers as P.val32: R stays the exact transpose of P)
    dbuf<double> dinv;    // [n]
    dbuf<uint8_t> ident;  // [n] scalar row has no off-diagonal value (eliminated Dirichlet dof)
    dbuf<double> B;       // near-null space [n][nb]
    double lmax = 2.0;    // largest eigenvalue of D^-1 A (estimate)
    double gersh = 2.0;   // Gershgorin bound of it
    dbuf<double> x, b, r, d, t;   // work vectors (levels > 0 own x and b)
};

struct fs_amg_s {
    fs_matrix_s* fine = nullptr;
    std::vector<amg_level*> lv;
    dbuf<double> cinv;          // dense inverse of the coarsest operator (row-major), empty = Chebyshev
    int64_t nc = 0;
    double setup_ms = 0.0;
    double op_complexity = 1.0, grid_complexity = 1.0;
    int smooth_steps = 2;
    dbuf<double> partials, sums;
    // PCG vectors
    dbuf<double> pr, pz, pp, pw;
    // DISTRIBUTED fine level under replicated coarse levels (fs_amg_attach_distributed_fine): the hierarchy was built on the
    // undecomposed operator (every rank the same), `fine` is swapped for this rank's rows of the decomposed operator and dist0
    // holds the level-0 pieces for those rows - P rows + transpose index, dinv, work vectors; level 1 and below stay replicated
    amg_level* dist0 = nullptr;
    fs_space_s* dist_space = nullptr;      // the decomposed space dist0 was built for (a later matrix on it may be re-attached)
    ~fs_amg_s() {
        for (amg_level* l : lv) delete l;
        delete dist0;
    }
};

static void amg_tick(const char* what);

// ---- small utilities --------------------------------------------------------------------------------
static int scan_exclusive(int32_t* d_in, int32_t* d_out, int64_t count, hipStream_t s) {
    size_t tb = 0;
    FS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_in, d_out, (int)count, s));
    dbuf<uint8_t> tmp;
    FS_CHECK(tmp.alloc((int64_t)tb + 16));
    FS_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, d_in, d_out, (int)count, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

static int sort_pairs(int32_t* k_in, int32_t* k_out, int32_t* v_in, int32_t* v_out, int64_t count, hipStream_t s) {
    size_t tb = 0;
    FS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, k_in, k_out, v_in, v_out, (int)count, 0, 32, s));
    dbuf<uint8_t> tmp;
    FS_CHECK(tmp.alloc((int64_t)tb + 16));
    FS_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, k_in, k_out, v_in, v_out, (int)count, 0, 32, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

static int read_i32(const int32_t* d, int32_t* h, hipStream_t s) {
    FS_HIP(hipMemcpyAsync(h, d, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

__global__ void k_iota(int32_t* v, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) v[i] = (int32_t)i;
}

// out[a] = first position p in sorted keys[0..n) with keys[p] >= a, a = 0..n_bins
__global__ void k_lower_bounds(const int32_t* __restrict__ keys, int64_t n, int64_t n_bins, int32_t* __restrict__ out) {
    int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; a <= n_bins; a += stride) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < (int32_t)a) lo = mid + 1; else hi = mid;
        }
        out[a] = (int32_t)lo;
    }
}

__global__ void k_expand_rows(const int32_t* __restrict__ rowptr, int64_t nrows, int32_t* __restrict__ rowidx) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nrows; i += stride)
        for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) rowidx[e] = (int32_t)i;
}

__global__ void k_gather_i32(const int32_t* __restrict__ src, const int32_t* __restrict__ idx, int64_t n, int32_t* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = src[idx[i]];
}

// B[i][c] = raw[c][i], or the constant of component (i % bs) when no vectors are given
__global__ void k_nullspace_layout(int64_t n, int nb, int bs, const double* __restrict__ raw, double* __restrict__ B) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; t < n * nb; t += stride) {
        const int64_t i = t / nb;
        const int c = (int)(t - i * nb);
        B[t] = raw ? raw[(int64_t)c * n + i] : ((int)(i % bs) == c ? 1.0 : 0.0);
    }
}

// The six rigid-body modes of SolverBase.build_nullspace (SolverBase.py:674-706) from the node coordinates, in the
// [dof][6] layout of the near-null space: translations, then (-y, x, 0), (z, 0, -x), (0, -z, y).  The reference
// orthonormalises them globally; the tentative prolongator orthonormalises per aggregate anyway, so the span is what
// matters.  Saves the 6 n doubles a host-built basis has to cross PCIe (245 MB at configs[2]).
// CG2 spaces: node i >= nv is the mid-point of edge i - nv (owned vertices first, then the owned edges in table order).
__global__ void k_rigid_body_modes(int64_t n_nodes, int64_t nv, const int32_t* __restrict__ edges, const double* __restrict__ xyz4,
                                   double* __restrict__ B) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n_nodes; i += stride) {
        double x, y, z;
        if (i < nv) {
            x = xyz4[4 * i]; y = xyz4[4 * i + 1]; z = xyz4[4 * i + 2];
        } else {
            const int64_t a = edges[2 * (i - nv)], b = edges[2 * (i - nv) + 1];
            x = 0.5 * (xyz4[4 * a] + xyz4[4 * b]); y = 0.5 * (xyz4[4 * a + 1] + xyz4[4 * b + 1]); z = 0.5 * (xyz4[4 * a + 2] + xyz4[4 * b + 2]);
        }
        double* b = B + i * 18;
        const double rows[3][6] = {{1, 0, 0, -y, z, 0}, {0, 1, 0, x, 0, -z}, {0, 0, 1, 0, -x, y}};
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 6; ++k) b[c * 6 + k] = rows[c][k];
    }
}

// ---- level 0: block CSR copy of the SELL/DIA matrix -------------------------------------------------
template <int BS>
__global__ void k_amg_extract(int64_t n_rows, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ rowptr,
                              const int32_t* __restrict__ sell_col, const double* __restrict__ val, int64_t plane,
                              double* __restrict__ out) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_rows; r += stride) {
        const int64_t sp0 = slice_ptr[r >> 6];
        const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
        const int64_t base = sp0 + (r & 63);
        int64_t o = rowptr[r];
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            if (sell_col[e] < 0) continue;     // structural entries come in ascending column order
            for (int i = 0; i < BS; ++i)
                for (int j = 0; j < BS; ++j) out[(o * BS + i) * BS + j] = val[(int64_t)(i * BS + j) * plane + e];
            ++o;
        }
    }
}

// rank-local block of a distributed matrix: entries whose column is a ghost node are dropped
__global__ void k_count_owned_cols(int64_t nn, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci, int32_t* __restrict__ cnt) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r <= nn; r += stride) {
        int32_t c = 0;
        if (r < nn)
            for (int32_t e = rp[r]; e < rp[r + 1]; ++e) c += ci[e] < nn ? 1 : 0;
        cnt[r] = c;
    }
}
__global__ void k_compact_owned_cols(int64_t nn, int bs2, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                     const double* __restrict__ val, const int32_t* __restrict__ nrp, int32_t* __restrict__ nci,
                                     double* __restrict__ nval) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < nn; r += stride) {
        int64_t o = nrp[r];
        for (int32_t e = rp[r]; e < rp[r + 1]; ++e) {
            if (ci[e] >= nn) continue;
            nci[o] = ci[e];
            for (int q = 0; q < bs2; ++q) nval[o * bs2 + q] = val[(int64_t)e * bs2 + q];
            ++o;
        }
    }
}

// maximum of a non-negative double over all threads into one word (positive doubles order like their bit patterns): the wave's
// maximum first, and a look at the word before the atomic - one atomic per THREAD on one address was half a million of them
__device__ __forceinline__ void fs_atomic_max_positive(unsigned long long* word, double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    if ((threadIdx.x & 63) == 0 && bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, bits);
}

// per node: 1/diag, identity-row flags, Gershgorin ratio (max over the block row, atomically maxed), block norm:
// 16 lanes per node striding over the values of its block row (contiguous in memory); bs <= 6 (1, 3 or 6 on every level)
__global__ void __launch_bounds__(FS_BLOCK) k_amg_diag_grp(int64_t nn, int bs, const int32_t* __restrict__ rp,
                                                           const int32_t* __restrict__ ci, const double* __restrict__ val,
                                                           double* __restrict__ dinv, uint8_t* __restrict__ ident,
                                                           double* __restrict__ dnorm, unsigned long long* __restrict__ gersh_bits) {
    const int sub = threadIdx.x & 15;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 4;
    const int bb = bs * bs;
    double gmax = 0.0;
    for (; i < nn; i += stride) {
        const int32_t e0 = rp[i];
        const int total = (rp[i + 1] - e0) * bb;
        const double* row = val + (int64_t)e0 * bb;
        double d[6] = {0, 0, 0, 0, 0, 0}, off[6] = {0, 0, 0, 0, 0, 0}, dn = 0.0;
        for (int idx = sub; idx < total; idx += 16) {
            const int e = idx / bb, rem = idx - e * bb;
            const int r = rem / bs, c = rem - r * bs;
            const double v = row[idx];
            const bool diag = ci[e0 + e] == (int32_t)i;
            const bool on_diag = diag && c == r;
            const double a = on_diag ? 0.0 : fabs(v);
#pragma unroll
            for (int rr = 0; rr < 6; ++rr) {
                if (rr == r) {
                    off[rr] += a;
                    if (on_diag) d[rr] = v;
                }
            }
            if (diag) dn += v * v;
        }
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                d[rr] += __shfl_xor(d[rr], o, 16);        // one lane holds the entry, the others 0
                off[rr] += __shfl_xor(off[rr], o, 16);
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) dn += __shfl_xor(dn, o, 16);
        double dm = 0.0, om = 0.0;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr)
            if (rr == sub) { dm = d[rr]; om = off[rr]; }
        if (sub < bs) {
            dinv[i * bs + sub] = dm != 0.0 ? 1.0 / dm : 1.0;
            ident[i * bs + sub] = om == 0.0 ? 1 : 0;
            if (dm != 0.0) gmax = fmax(gmax, (fabs(dm) + om) / fabs(dm));
        }
        if (sub == 0) dnorm[i] = sqrt(dn);
    }
    fs_atomic_max_positive(gersh_bits, gmax);
}

// strength graph: j != i strong iff ||A_ij||_F^2 > theta^2 ||A_ii||_F ||A_jj||_F (and > 0)
// 16 lanes per node.  Small blocks (COOP = false): a lane per entry of the block row, the strong entries keep their
// order through the ballot of the group.  Large blocks (6x6): the group sums one block after the other together
// (butterfly: every lane holds the same bits) and its first lane writes.
template <bool FILL, bool COOP>
__global__ void __launch_bounds__(FS_BLOCK) k_strength_grp(int64_t nn, int bs, const int32_t* __restrict__ rp,
                                                           const int32_t* __restrict__ ci, const double* __restrict__ val,
                                                           const double* __restrict__ dnorm, double theta2,
                                                           int32_t* __restrict__ cnt, const int32_t* __restrict__ sptr,
                                                           int32_t* __restrict__ scol, double* __restrict__ sw) {
    const int sub = threadIdx.x & 15;
    const int shift = threadIdx.x & 48;                    // first lane of the group inside its wave
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 4;
    const int bb = bs * bs;
    for (; i < nn; i += stride) {
        const int32_t e0 = rp[i], e1 = rp[i + 1];
        const int32_t o = FILL ? sptr[i] : 0;
        const double di = dnorm[i];
        int32_t n = 0;
        if (COOP) {
            for (int32_t e = e0; e < e1; ++e) {
                const int32_t j = ci[e];
                if (j == (int32_t)i) continue;
                const double* blk = val + (int64_t)e * bb;
                double f = 0.0;
                for (int q = sub; q < bb; q += 16) f += blk[q] * blk[q];
#pragma unroll
                for (int w = 8; w > 0; w >>= 1) f += __shfl_xor(f, w, 16);
                if (f > 0.0 && f > theta2 * di * dnorm[j]) {
                    if (FILL && sub == 0) { scol[o + n] = j; sw[o + n] = f; }
                    ++n;
                }
            }
        } else {
            for (int32_t base = e0; base < e1; base += 16) {
                const int32_t e = base + sub;
                bool strong = false;
                int32_t j = 0;
                double f = 0.0;
                if (e < e1) {
                    j = ci[e];
                    if (j != (int32_t)i) {
                        const double* blk = val + (int64_t)e * bb;
                        for (int q = 0; q < bb; ++q) f += blk[q] * blk[q];
                        strong = f > 0.0 && f > theta2 * di * dnorm[j];
                    }
                }
                const unsigned m = (unsigned)((__ballot(strong) >> shift) & 0xffffull);
                if (FILL && strong) {
                    const int at = o + n + __popc(m & ((1u << sub) - 1u));
                    scol[at] = j;
                    sw[at] = f;
                }
                n += __popc(m);
            }
        }
        if (!FILL && sub == 0) cnt[i] = n;
    }
}

// ---- MIS(2) ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t amg_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// key = state(2 bits: 2 root, 1 undecided, 0 out) | hash(30) | index(32)
__global__ void k_mis_init(int64_t nn, const int32_t* __restrict__ sptr, unsigned long long* __restrict__ key) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nn; i += stride) {
        const unsigned long long st = sptr[i + 1] > sptr[i] ? 1ULL : 0ULL;
        key[i] = (st << 62) | ((unsigned long long)(amg_hash((uint32_t)i) & 0x3fffffffU) << 32) | (unsigned long long)i;
    }
}
__global__ void k_mis_max(int64_t nn, const int32_t* __restrict__ sptr, const int32_t* __restrict__ scol,
                          const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nn; i += stride) {
        unsigned long long m = in[i];
        for (int32_t e = sptr[i]; e < sptr[i + 1]; ++e) {
            const unsigned long long v = in[scol[e]];
            m = v > m ? v : m;
        }
        out[i] = m;
    }
}
__global__ void k_mis_update(int64_t nn, unsigned long long* __restrict__ key, const unsigned long long* __restrict__ m2,
                             int32_t* __restrict__ undecided) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int32_t left = 0;
    for (; i < nn; i += stride) {
        const unsigned long long k = key[i];
        if ((k >> 62) != 1ULL) continue;
        const unsigned long long m = m2[i];
        if ((uint32_t)m == (uint32_t)i) key[i] = (k & ~(3ULL << 62)) | (2ULL << 62);
        else if ((m >> 62) == 2ULL) key[i] = k & ~(3ULL << 62);
        else ++left;
    }
    // (the wave's count first: one atomic per thread on one word is half a million of them per round)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) left += __shfl_xor(left, off, 64);
    if (left && (threadIdx.x & 63) == 0) atomicAdd(undecided, left);
}
__global__ void k_agg_rootflag(int64_t nn, const unsigned long long* __restrict__ key, int32_t* __restrict__ flag) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i <= nn; i += stride) flag[i] = (i < nn && (key[i] >> 62) == 2ULL) ? 1 : 0;
}
__global__ void k_agg_pass1(int64_t nn, const int32_t* __restrict__ sptr, const int32_t* __restrict__ scol,
                            const unsigned long long* __restrict__ key, const int32_t* __restrict__ rootid,
                            int32_t* __restrict__ agg1) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nn; i += stride) {
        int32_t a = -1;
        if ((key[i] >> 62) == 2ULL) a = rootid[i];
        else
            for (int32_t e = sptr[i]; e < sptr[i + 1]; ++e) {
                const int32_t j = scol[e];
                if ((key[j] >> 62) == 2ULL) { a = rootid[j]; break; }   // at most one root neighbour
            }
        agg1[i] = a;
    }
}
__global__ void k_agg_pass2(int64_t nn, const int32_t* __restrict__ sptr, const int32_t* __restrict__ scol,
                            const double* __restrict__ sw, const int32_t* __restrict__ agg1, int32_t* __restrict__ agg) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nn; i += stride) {
        int32_t a = agg1[i];
        if (a < 0) {
            double best = -1.0;
            for (int32_t e = sptr[i]; e < sptr[i + 1]; ++e) {   // ascending j: ties go to the smaller index
                const int32_t aj = agg1[scol[e]];
                if (aj >= 0 && sw[e] > best * (1.0 + 1e-6)) { best = sw[e]; a = aj; }   // noise must not break ties
            }
        }
        agg[i] = a;
    }
}
__global__ void k_agg_sortkey(int64_t nn, const int32_t* __restrict__ agg, int32_t n_agg, int32_t* __restrict__ key,
                              int32_t* __restrict__ has) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i <= nn; i += stride) {
        if (i < nn) key[i] = agg[i] >= 0 ? agg[i] : n_agg;
        has[i] = (i < nn && agg[i] >= 0) ? 1 : 0;
    }
}

// ---- tentative prolongator: QR of the near-null space over every aggregate ---------------------------
// T [nn][bs][nb] (rows of isolated nodes stay 0), Bc [n_agg][nb][nb] = R
__global__ void k_tentative(int64_t n_agg, int bs, int nb, const int32_t* __restrict__ agg_ptr,
                            const int32_t* __restrict__ members, const double* __restrict__ B,
                            const uint8_t* __restrict__ ident, double* __restrict__ T, double* __restrict__ Bc) {
    int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; a < n_agg; a += stride) {
        const int32_t m0 = agg_ptr[a], m1 = agg_ptr[a + 1];
        for (int32_t m = m0; m < m1; ++m) {
            const int64_t i = members[m];
            for (int r = 0; r < bs; ++r)
                for (int c = 0; c < nb; ++c)
                    T[(i * bs + r) * nb + c] = ident[i * bs + r] ? 0.0 : B[(i * bs + r) * nb + c];
        }
        double* R = Bc + a * nb * nb;
        for (int q = 0; q < nb * nb; ++q) R[q] = 0.0;
        for (int c = 0; c < nb; ++c) {
            double orig = 0.0;
            for (int32_t m = m0; m < m1; ++m) {
                const int64_t i = members[m];
                for (int r = 0; r < bs; ++r) { const double v = T[(i * bs + r) * nb + c]; orig += v * v; }
            }
            for (int k = 0; k < c; ++k) {
                double dot = 0.0;
                for (int32_t m = m0; m < m1; ++m) {
                    const int64_t i = members[m];
                    for (int r = 0; r < bs; ++r) dot += T[(i * bs + r) * nb + k] * T[(i * bs + r) * nb + c];
                }
                R[k * nb + c] = dot;
                for (int32_t m = m0; m < m1; ++m) {
                    const int64_t i = members[m];
                    for (int r = 0; r < bs; ++r) T[(i * bs + r) * nb + c] -= dot * T[(i * bs + r) * nb + k];
                }
            }
            double nrm = 0.0;
            for (int32_t m = m0; m < m1; ++m) {
                const int64_t i = members[m];
                for (int r = 0; r < bs; ++r) { const double v = T[(i * bs + r) * nb + c]; nrm += v * v; }
            }
            const bool live = nrm > 1e-16 * orig && nrm > 0.0;   // (1e-8)^2: column not in the span of the others
            nrm = sqrt(nrm);
            R[c * nb + c] = live ? nrm : 0.0;
            const double sc = live ? 1.0 / nrm : 0.0;
            if (!live)
                for (int k = 0; k < c; ++k) R[k * nb + c] = 0.0;
            for (int32_t m = m0; m < m1; ++m) {
                const int64_t i = members[m];
                for (int r = 0; r < bs; ++r) T[(i * bs + r) * nb + c] *= sc;
            }
        }
    }
}

// the same with one wave per aggregate: a lane owns the rows lane, lane + 64, ... of the aggregate (nobody else
// touches them), the column products are butterfly sums over the wave - every lane holds the same bits
__device__ __forceinline__ double wave_sum_all(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(64) k_tentative_wave(int64_t n_agg, int bs, int nb, const int32_t* __restrict__ agg_ptr,
                                                       const int32_t* __restrict__ members, const double* __restrict__ B,
                                                       const uint8_t* __restrict__ ident, double* __restrict__ T,
                                                       double* __restrict__ Bc) {
    const int lane = threadIdx.x;
    for (int64_t a = blockIdx.x; a < n_agg; a += gridDim.x) {
        const int32_t m0 = agg_ptr[a];
        const int n_rows = (agg_ptr[a + 1] - m0) * bs;
        double* R = Bc + a * nb * nb;
        for (int q = lane; q < nb * nb; q += 64) R[q] = 0.0;
        for (int t = lane; t < n_rows; t += 64) {
            const int64_t row = (int64_t)members[m0 + t / bs] * bs + t % bs;
            for (int c = 0; c < nb; ++c) T[row * nb + c] = ident[row] ? 0.0 : B[row * nb + c];
        }
        for (int c = 0; c < nb; ++c) {
            double part = 0.0;
            for (int t = lane; t < n_rows; t += 64) {
                const int64_t row = (int64_t)members[m0 + t / bs] * bs + t % bs;
                const double v = T[row * nb + c];
                part += v * v;
            }
            const double orig = wave_sum_all(part);
            for (int k = 0; k < c; ++k) {
                part = 0.0;
                for (int t = lane; t < n_rows; t += 64) {
                    const int64_t row = (int64_t)members[m0 + t / bs] * bs + t % bs;
                    part += T[row * nb + k] * T[row * nb + c];
                }
                const double dot = wave_sum_all(part);
                if (lane == 0) R[k * nb + c] = dot;
                for (int t = lane; t < n_rows; t += 64) {
                    const int64_t row = (int64_t)members[m0 + t / bs] * bs + t % bs;
                    T[row * nb + c] -= dot * T[row * nb + k];
                }
            }
            part = 0.0;
            for (int t = lane; t < n_rows; t += 64) {
                const int64_t row = (int64_t)members[m0 + t / bs] * bs + t % bs;
                const double v = T[row * nb + c];
                part += v * v;
            }
            double nrm = wave_sum_all(part);
            const bool live = nrm > 1e-16 * orig && nrm > 0.0;   // (1e-8)^2: column not in the span of the others
            nrm = sqrt(nrm);
            const double sc = live ? 1.0 / nrm : 0.0;
            if (lane == 0) {
                R[c * nb + c] = live ? nrm : 0.0;
                if (!live)
                    for (int k = 0; k < c; ++k) R[k * nb + c] = 0.0;
            }
            for (int t = lane; t < n_rows; t += 64) {
                const int64_t row = (int64_t)members[m0 + t / bs] * bs + t % bs;
                T[row * nb + c] *= sc;
            }
        }
    }
}

// T as block CSR: one block per aggregated node
__global__ void k_t_fill(int64_t nn, int bsnb, const int32_t* __restrict__ agg, const int32_t* __restrict__ tptr,
                         const double* __restrict__ T, int32_t* __restrict__ tcol, double* __restrict__ tval) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nn; i += stride) {
        if (agg[i] < 0) continue;
        const int64_t e = tptr[i];
        tcol[e] = agg[i];
        for (int q = 0; q < bsnb; ++q) tval[e * bsnb + q] = T[i * bsnb + q];
    }
}

// P = T - omega D^-1 (A T), in place on the values of AT (pattern of AT contains agg(i): the diagonal is structural)
// 16 lanes per node over the values of its row of P
__global__ void __launch_bounds__(FS_BLOCK) k_smooth_p_grp(int64_t nn, int bs, int nb, const int32_t* __restrict__ rp,
                                                           const int32_t* __restrict__ ci, double* __restrict__ val,
                                                           const double* __restrict__ dinv, const int32_t* __restrict__ agg,
                                                           const double* __restrict__ T, double omega) {
    const int sub = threadIdx.x & 15;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 4;
    const int bb = bs * nb;
    for (; i < nn; i += stride) {
        const int32_t e0 = rp[i];
        const int total = (rp[i + 1] - e0) * bb;
        double* row = val + (int64_t)e0 * bb;
        const int32_t mine = agg[i];
        for (int idx = sub; idx < total; idx += 16) {
            const int e = idx / bb, rem = idx - e * bb;
            const int r = rem / nb;
            double v = -omega * dinv[i * bs + r] * row[idx];
            if (ci[e0 + e] == mine) v += T[i * bb + rem];
            row[idx] = v;
        }
    }
}

// ---- row-wise SpGEMM ----------------------------------------------------------------------------------
// Output row I expands the rows lk[q] of the right matrix, q in [lptr[I], lptr[I+1]).
// Symbolic: distinct columns through an LDS hash; COUNT writes the row length, otherwise the sorted columns.
template <bool COUNT>
__global__ void k_spgemm_symbolic(int64_t n_out, const int32_t* __restrict__ lptr, const int32_t* __restrict__ lk,
                                  const int32_t* __restrict__ rptr, const int32_t* __restrict__ rcol, int cap,
                                  int32_t* __restrict__ rowlen, const int32_t* __restrict__ optr,
                                  int32_t* __restrict__ ocol, int32_t* __restrict__ overflow) {
    extern __shared__ int32_t lds_i[];
    int32_t* keys = lds_i;            // [cap]
    int32_t* list = lds_i + cap;      // [cap]
    __shared__ int32_t used;
    const int lane16 = threadIdx.x & 15, grp = threadIdx.x >> 4, ngrp = blockDim.x >> 4;
    for (int64_t I = blockIdx.x; I < n_out; I += gridDim.x) {
        for (int t = threadIdx.x; t < cap; t += blockDim.x) keys[t] = -1;
        if (threadIdx.x == 0) used = 0;
        __syncthreads();
        for (int32_t q = lptr[I] + grp; q < lptr[I + 1]; q += ngrp) {
            const int32_t k = lk[q];
            for (int32_t p = rptr[k] + lane16; p < rptr[k + 1]; p += 16) {
                const int32_t J = rcol[p];
                uint32_t h = ((uint32_t)J * 2654435761U) % (uint32_t)cap;
                int probes = 0;
                while (true) {
                    const int32_t old = atomicCAS(&keys[h], -1, J);
                    if (old == -1 || old == J) break;
                    h = h + 1 == (uint32_t)cap ? 0 : h + 1;
                    if (++probes >= cap) { atomicExch(overflow, 1); break; }
                }
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < cap; t += blockDim.x)
            if (keys[t] >= 0) list[atomicAdd(&used, 1)] = keys[t];
        __syncthreads();
        const int n = used;
        if (COUNT) {
            if (threadIdx.x == 0) rowlen[I] = n;
        } else {
            const int32_t o = optr[I];
            for (int t = threadIdx.x; t < n; t += blockDim.x) {
                const int32_t key = list[t];
                int rank = 0;
                for (int u = 0; u < n; ++u) rank += list[u] < key ? 1 : 0;
                ocol[o + rank] = key;
            }
        }
        __syncthreads();
    }
}

// Numeric: C_row(I) = sum_q L_q * Rrow(lk[q]); L_q = left block lval[lidx[q]] (br x bk), used transposed when
// TRANS (stored bk x br).  The row is accumulated in LDS ([len][br][bc]); within one q all items hit distinct
// addresses, consecutive q are separated by a barrier: no atomics, fixed summation order.
#define FS_SPGEMM_STAGE 64
template <bool TRANS>
__global__ void k_spgemm_numeric(int64_t n_out, int maxlen, int br, int bk, int bc, const int32_t* __restrict__ lptr,
                                 const int32_t* __restrict__ lk, const int32_t* __restrict__ lidx,
                                 const double* __restrict__ lval, const int32_t* __restrict__ rptr,
                                 const int32_t* __restrict__ rcol, const double* __restrict__ rval,
                                 const int32_t* __restrict__ optr, const int32_t* __restrict__ ocol,
                                 double* __restrict__ oval) {
    extern __shared__ double acc[];
    const int rc = br * bc;
    // the row's output columns are staged once, so the binary search of every product runs in LDS.  (Staging the
    // whole lookup - right rows, product positions - ahead of the accumulation rounds was tried: the 20 KB of extra
    // LDS per workgroup cost more occupancy than the shorter dependency chains gained, 2x slower.)
    int32_t* scol = reinterpret_cast<int32_t*>(acc + (size_t)maxlen * rc);
    // (right row, its start, its length, left block) of the next FS_SPGEMM_STAGE products, fetched by as many lanes
    // at once: the three dependent loads lk -> rptr -> row would otherwise sit in front of every accumulation round
    int32_t* stage = scol + maxlen;
    for (int64_t I = blockIdx.x; I < n_out; I += gridDim.x) {
        const int32_t o0 = optr[I];
        const int len = optr[I + 1] - o0;
        for (int t = threadIdx.x; t < len * rc; t += blockDim.x) acc[t] = 0.0;
        for (int t = threadIdx.x; t < len; t += blockDim.x) scol[t] = ocol[o0 + t];
        const int32_t q_end = lptr[I + 1];
        for (int32_t q0 = lptr[I]; q0 < q_end; q0 += FS_SPGEMM_STAGE) {
            const int nq = min(FS_SPGEMM_STAGE, q_end - q0);
            __syncthreads();
            if ((int)threadIdx.x < nq) {
                const int32_t q = q0 + threadIdx.x;
                const int32_t k = lk[q];
                const int32_t r0 = rptr[k];
                stage[4 * threadIdx.x + 0] = r0;
                stage[4 * threadIdx.x + 1] = rptr[k + 1] - r0;
                stage[4 * threadIdx.x + 2] = lidx ? lidx[q] : q;
            }
            __syncthreads();
            for (int j = 0; j < nq; ++j) {
                const int32_t r0 = stage[4 * j + 0];
                const int items = stage[4 * j + 1] * rc;
                const double* L = lval + (int64_t)stage[4 * j + 2] * br * bk;
                for (int it = threadIdx.x; it < items; it += blockDim.x) {
                    const int p = it / rc, e = it - p * rc;
                    const int r = e / bc, c = e - r * bc;
                    const int32_t J = rcol[r0 + p];
                    const double* Rb = rval + (int64_t)(r0 + p) * bk * bc;
                    double v = 0.0;
                    for (int m = 0; m < bk; ++m) v += (TRANS ? L[m * br + r] : L[r * bk + m]) * Rb[m * bc + c];
                    int lo = 0, hi = len;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (scol[mid] < J) lo = mid + 1; else hi = mid;
                    }
                    acc[lo * rc + e] += v;
                }
                if (j + 1 < nq) __syncthreads();
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < len * rc; t += blockDim.x) oval[(int64_t)o0 * rc + t] = acc[t];
        __syncthreads();
    }
}

// The same product with one wave per output row and the block shape known at compile time.  The wave is cut into
// G = 64 >> gl_log2 groups of lanes; group g takes the products q = g, g + G, ... of the row and accumulates them in
// its own copy of the row (LDS), a lane owning one column c of one right block and running over the BR rows itself:
// one column search, BK right values and BR*BK left values (the same addresses over the group) per BR results.  No
// barrier separates the products: a group sits inside one wave, whose LDS accesses complete in issue order.  The
// copies are added in the order g = 0..G-1 at the end, so the summation order is a function of the operands alone.
template <bool TRANS, int BR, int BK, int BC>
__global__ void __launch_bounds__(64) k_spgemm_numeric_wave(int64_t n_out, int maxlen, int gl_log2,
                                                            const int32_t* __restrict__ lptr, const int32_t* __restrict__ lk,
                                                            const int32_t* __restrict__ lidx, const double* __restrict__ lval,
                                                            const int32_t* __restrict__ rptr, const int32_t* __restrict__ rcol,
                                                            const double* __restrict__ rval, const int32_t* __restrict__ optr,
                                                            const int32_t* __restrict__ ocol, double* __restrict__ oval) {
    extern __shared__ double acc[];
    constexpr int RC = BR * BC;
    const int G = 64 >> gl_log2, gl = 1 << gl_log2;
    const int lane = threadIdx.x, g = lane >> gl_log2, sub = lane & (gl - 1);
    const size_t copy = (size_t)maxlen * RC;
    int32_t* scol = reinterpret_cast<int32_t*>(acc + (size_t)G * copy);
    int32_t* stage = scol + maxlen;
    double* mine = acc + (size_t)g * copy;
    for (int64_t I = blockIdx.x; I < n_out; I += gridDim.x) {
        const int32_t o0 = optr[I];
        const int len = optr[I + 1] - o0;
        for (int k = 0; k < G; ++k)
            for (int t = lane; t < len * RC; t += 64) acc[k * copy + t] = 0.0;
        for (int t = lane; t < len; t += 64) scol[t] = ocol[o0 + t];
        const int32_t q_end = lptr[I + 1];
        for (int32_t q0 = lptr[I]; q0 < q_end; q0 += 64) {
            const int nq = min(64, q_end - q0);
            __syncthreads();
            if (lane < nq) {
                const int32_t q = q0 + lane;
                const int32_t k = lk[q];
                const int32_t r0 = rptr[k];
                stage[4 * lane + 0] = r0;
                stage[4 * lane + 1] = rptr[k + 1] - r0;
                stage[4 * lane + 2] = lidx ? lidx[q] : q;
            }
            __syncthreads();
            for (int j = g; j < nq; j += G) {
                const int32_t r0 = stage[4 * j + 0];
                const int items = stage[4 * j + 1] * BC;
                const double* L = lval + (int64_t)stage[4 * j + 2] * BR * BK;
                double Lr[BR * BK];
#pragma unroll
                for (int t = 0; t < BR * BK; ++t) Lr[t] = L[t];
                for (int it = sub; it < items; it += gl) {
                    const int p = it / BC, c = it - p * BC;
                    const int32_t J = rcol[r0 + p];
                    const double* Rb = rval + (int64_t)(r0 + p) * BK * BC + c;
                    double rv[BK];
#pragma unroll
                    for (int m = 0; m < BK; ++m) rv[m] = Rb[m * BC];
                    int lo = 0, hi = len;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (scol[mid] < J) lo = mid + 1; else hi = mid;
                    }
                    double* a = mine + lo * RC + c;
#pragma unroll
                    for (int r = 0; r < BR; ++r) {
                        double v = 0.0;
#pragma unroll
                        for (int m = 0; m < BK; ++m) v += (TRANS ? Lr[m * BR + r] : Lr[r * BK + m]) * rv[m];
                        a[r * BC] += v;
                    }
                }
            }
        }
        __syncthreads();
        for (int t = lane; t < len * RC; t += 64) {
            double v = acc[t];
            for (int k = 1; k < G; ++k) v += acc[k * copy + t];
            oval[(int64_t)o0 * RC + t] = v;
        }
        __syncthreads();
    }
}

template <bool TRANS, int BR, int BK, int BC>
static int launch_spgemm_wave(int64_t n_out, int maxlen, double items_per_product, const int32_t* lptr, const int32_t* lk,
                              const int32_t* lidx, const double* lval, const bcsr& R, bcsr* C, hipStream_t s) {
    int gl_log2 = 3;                                            // 8 lanes per product at least
    while (gl_log2 < 6 && (1 << gl_log2) < items_per_product) ++gl_log2;
    const size_t copy = (size_t)maxlen * BR * BC * sizeof(double);
    while (gl_log2 < 6 && (64 >> gl_log2) * copy > 24 * 1024) ++gl_log2;   // keep several waves per CU resident
    const size_t lds = (size_t)(64 >> gl_log2) * copy + (size_t)maxlen * sizeof(int32_t) + 64 * 4 * sizeof(int32_t);
    FS_REQUIRE(lds <= 160 * 1024 - 512, "AMG setup: a product row of %d blocks (%dx%d) exceeds the LDS accumulator", maxlen, BR, BC);
    auto kern = k_spgemm_numeric_wave<TRANS, BR, BK, BC>;
    if (lds > 64 * 1024) FS_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = (int)std::min<int64_t>(n_out, 1 << 20);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, s, n_out, maxlen, gl_log2, lptr, lk, lidx, lval, R.rowptr.p, R.col.p,
                       R.val.p, C->rowptr.p, C->col.p, C->val.p);
    FS_KERNEL_CHECK();
    return FS_OK;
}

// dead coarse dofs (near-null-space column not representable on an aggregate): unit diagonal
__global__ void k_fix_dead(int64_t nn, int bs, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                           double* __restrict__ val) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nn; i += stride)
        for (int32_t e = rp[i]; e < rp[i + 1]; ++e)
            if (ci[e] == (int32_t)i)
                for (int r = 0; r < bs; ++r)
                    if (val[((int64_t)e * bs + r) * bs + r] == 0.0) val[((int64_t)e * bs + r) * bs + r] = 1.0;
}

// ---- solve phase kernels ------------------------------------------------------------------------------
// y = A x (MODE 0) or y = b - A x (MODE 1); thread per scalar row
template <int BS, int MODE>
__global__ void __launch_bounds__(FS_BLOCK) k_bcsr_spmv(int64_t n, const int32_t* __restrict__ rp,
                                                        const int32_t* __restrict__ ci, const double* __restrict__ val,
                                                        const double* __restrict__ x, const double* __restrict__ b,
                                                        double* __restrict__ y) {
    int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; row < n; row += stride) {
        const int64_t i = row / BS;
        const int r = (int)(row - i * BS);
        double acc = 0.0;
        for (int32_t e = rp[i]; e < rp[i + 1]; ++e) {
            const double* blk = val + ((int64_t)e * BS + r) * BS;
            const double* xj = x + (int64_t)ci[e] * BS;
#pragma unroll
            for (int c = 0; c < BS; ++c) acc += blk[c] * xj[c];
        }
        y[row] = MODE ? b[row] - acc : acc;
    }
}

// the same with G lanes per scalar row (coarse levels: few, long rows - a thread per row walks 30-250 entries one
// dependent load after the other and fills a fraction of the chip: 39 us for a 4 K-row level, latency only)
template <int BS, int MODE, int G>
__global__ void __launch_bounds__(FS_BLOCK) k_bcsr_spmv_grp(int64_t n, const int32_t* __restrict__ rp,
                                                            const int32_t* __restrict__ ci, const double* __restrict__ val,
                                                            const double* __restrict__ x, const double* __restrict__ b,
                                                            double* __restrict__ y) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = gid / G;
    const int lg = (int)(gid - row * G);
    double acc = 0.0;
    if (row < n) {
        const int64_t i = row / BS;
        const int r = (int)(row - i * BS);
        for (int32_t e = rp[i] + lg; e < rp[i + 1]; e += G) {
            const double* blk = val + ((int64_t)e * BS + r) * BS;
            const double* xj = x + (int64_t)ci[e] * BS;
#pragma unroll
            for (int c = 0; c < BS; ++c) acc += blk[c] * xj[c];
        }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, G);      // fixed order: reproducible
    if (lg == 0 && row < n) y[row] = MODE ? b[row] - acc : acc;
}

template <typename T> struct fs_pair_of;
template <> struct fs_pair_of<double> { typedef double2 type; };
template <> struct fs_pair_of<float> { typedef float2 type; };

// the same with one wave per NODE (block row) of a level with large blocks: the lanes stride over the contiguous values
// of the block row (coalesced 8-byte loads; the per-scalar-row kernels read 48-byte pieces 288 bytes apart and lean on
// the caches for the rest of the line: 3.5 TB/s on the 0.9 GB level-1 operator of configs[2]), every lane keeps BS
// partial sums, butterfly reduction, lanes 0..BS-1 write
template <int BS, int MODE, typename VT = double>
__global__ void __launch_bounds__(FS_BLOCK) k_bcsr_spmv_node(int64_t nn, const int32_t* __restrict__ rp,
                                                             const int32_t* __restrict__ ci, const VT* __restrict__ val,
                                                             const double* __restrict__ x, const double* __restrict__ b,
                                                             double* __restrict__ y) {
    constexpr int BB = BS * BS;
    const int lane = threadIdx.x & 63;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (; i < nn; i += stride) {
        const int32_t e0 = rp[i];
        const int total = (rp[i + 1] - e0) * BB;
        const VT* row = val + (int64_t)e0 * BB;
        double acc[BS];
#pragma unroll
        for (int r = 0; r < BS; ++r) acc[r] = 0.0;
        if (BS == 6 && sizeof(VT) == 4) {
            // fp32 values of 6 x 6 blocks: a lane takes TWO rows of one block - 48 bytes, three 16-byte loads (a row alone is three 8-byte
            // loads: 110 us per level-1 product of configs[2], 4.1 TB/s) - and the block's six values of x once for both
            const float4* row4 = reinterpret_cast<const float4*>(row);
            const int parts = (rp[i + 1] - e0) * 3;
            for (int idx = lane; idx < parts; idx += 64) {
                const int e = idx / 3, r2 = idx - e * 3;
                const double2* xv = reinterpret_cast<const double2*>(x + (int64_t)ci[e0 + e] * BS);
                const float4 a0 = row4[(int64_t)idx * 3], a1 = row4[(int64_t)idx * 3 + 1], a2 = row4[(int64_t)idx * 3 + 2];
                const double2 x0 = xv[0], x1 = xv[1], x2 = xv[2];
                // the terms of a row in the order of the one-row-per-lane form: pairs (0, 1), (2, 3), (4, 5)
                double v0 = 0.0, v1 = 0.0;
                v0 += (double)a0.x * x0.x + (double)a0.y * x0.y;
                v0 += (double)a0.z * x1.x + (double)a0.w * x1.y;
                v0 += (double)a1.x * x2.x + (double)a1.y * x2.y;
                v1 += (double)a1.z * x0.x + (double)a1.w * x0.y;
                v1 += (double)a2.x * x1.x + (double)a2.y * x1.y;
                v1 += (double)a2.z * x2.x + (double)a2.w * x2.y;
#pragma unroll
                for (int rr = 0; rr < 3; ++rr)
                    if (rr == r2) { acc[2 * rr] += v0; acc[2 * rr + 1] += v1; }
            }
        } else if (BS % 2 == 0) {           // a lane takes one row of one block: BS/2 16-byte (fp32 values: 8-byte) loads of values, BS/2 16-byte loads of x
            constexpr int HP = BS / 2;
            typedef typename fs_pair_of<VT>::type VT2;
            const VT2* row2 = reinterpret_cast<const VT2*>(row);
            const int parts = (rp[i + 1] - e0) * BS;
            for (int idx = lane; idx < parts; idx += 64) {
                const int e = idx / BS, r = idx - e * BS;
                const double2* xv = reinterpret_cast<const double2*>(x + (int64_t)ci[e0 + e] * BS);
                double v = 0.0;
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    const VT2 a = row2[(int64_t)idx * HP + h];
                    const double2 xx = xv[h];
                    v += (double)a.x * xx.x + (double)a.y * xx.y;
                }
#pragma unroll
                for (int rr = 0; rr < BS; ++rr)
                    if (rr == r) acc[rr] += v;
            }
        } else {
            for (int idx = lane; idx < total; idx += 64) {
                const int e = idx / BB, rem = idx - e * BB;
                const int r = rem / BS, c = rem - r * BS;
                const double v = (double)row[idx] * x[(int64_t)ci[e0 + e] * BS + c];
#pragma unroll
                for (int rr = 0; rr < BS; ++rr)
                    if (rr == r) acc[rr] += v;
            }
        }
        double mine = 0.0;
#pragma unroll
        for (int rr = 0; rr < BS; ++rr) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[rr] += __shfl_xor(acc[rr], o, 64);
            if (rr == lane) mine = acc[rr];
        }
        if (lane < BS) y[i * BS + lane] = MODE ? b[i * BS + lane] - mine : mine;
    }
}

// xf += P xc ; thread per fine scalar row
__global__ void k_prolong_add(int64_t n_f, int br, int bc, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                              const double* __restrict__ val, const double* __restrict__ xc, double* __restrict__ xf) {
    int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; row < n_f; row += stride) {
        const int64_t i = row / br;
        const int r = (int)(row - i * br);
        double acc = 0.0;
        for (int32_t e = rp[i]; e < rp[i + 1]; ++e) {
            const double* blk = val + ((int64_t)e * br + r) * bc;
            const double* xj = xc + (int64_t)ci[e] * bc;
            for (int c = 0; c < bc; ++c) acc += blk[c] * xj[c];
        }
        xf[row] += acc;
    }
}

// the same for a known block shape: 16 lanes per fine node stride over the values of its block row
template <int BR, int BC, typename VT = double>
__global__ void __launch_bounds__(FS_BLOCK) k_prolong_add_grp(int64_t nn_f, const int32_t* __restrict__ rp,
                                                              const int32_t* __restrict__ ci, const VT* __restrict__ val,
                                                              const double* __restrict__ xc, double* __restrict__ xf) {
    constexpr int BB = BR * BC;
    const int sub = threadIdx.x & 15;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 4;
    for (; i < nn_f; i += stride) {
        const int32_t e0 = rp[i];
        const int total = (rp[i + 1] - e0) * BB;
        const VT* row = val + (int64_t)e0 * BB;
        double acc[BR];
#pragma unroll
        for (int r = 0; r < BR; ++r) acc[r] = 0.0;
        if (BC % 2 == 0) {           // a lane takes one row of one block: BC/2 16-byte (fp32 values: 8-byte) loads of values, BC/2 16-byte loads of xc
            constexpr int HP = BC / 2;
            typedef typename fs_pair_of<VT>::type VT2;
            const VT2* row2 = reinterpret_cast<const VT2*>(row);
            const int parts = (rp[i + 1] - e0) * BR;
            for (int idx = sub; idx < parts; idx += 16) {
                const int e = idx / BR, r = idx - e * BR;
                const double2* xv = reinterpret_cast<const double2*>(xc + (int64_t)ci[e0 + e] * BC);
                double v = 0.0;
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    const VT2 a = row2[(int64_t)idx * HP + h];
                    const double2 xx = xv[h];
                    v += (double)a.x * xx.x + (double)a.y * xx.y;
                }
#pragma unroll
                for (int rr = 0; rr < BR; ++rr)
                    if (rr == r) acc[rr] += v;
            }
        } else {
            for (int idx = sub; idx < total; idx += 16) {
                const int e = idx / BB, rem = idx - e * BB;
                const int r = rem / BC, c = rem - r * BC;
                const double v = (double)row[idx] * xc[(int64_t)ci[e0 + e] * BC + c];
#pragma unroll
                for (int rr = 0; rr < BR; ++rr)
                    if (rr == r) acc[rr] += v;
            }
        }
        double mine = 0.0;
#pragma unroll
        for (int rr = 0; rr < BR; ++rr) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc[rr] += __shfl_xor(acc[rr], o, 16);
            if (rr == sub) mine = acc[rr];
        }
        if (sub < BR) xf[i * BR + sub] += mine;
    }
}

// R blocks: rt[q][c][r] = P[pt_entry[q]][r][c]
__global__ void k_transpose_blocks(int64_t nq, int br, int bc, const int32_t* __restrict__ pt_entry,
                                   const double* __restrict__ val, double* __restrict__ rt) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int bb = br * bc;
    for (; t < nq * bb; t += stride) {
        const int64_t q = t / bb;
        const int e = (int)(t - q * bb);
        const int c = e / br, r = e - c * br;
        rt[t] = val[(int64_t)pt_entry[q] * bb + r * bc + c];
    }
}

// out = P^T rf : one wave per coarse node; lanes stride over the entries of the column (contiguous R blocks),
// each lane accumulates its nb partial sums, fixed-order shuffle reduction
template <int BR, int BC, typename VT = double>
__global__ void __launch_bounds__(FS_BLOCK) k_restrict(int64_t nn_c, const int32_t* __restrict__ pt_ptr,
                                                        const int32_t* __restrict__ pt_row, const VT* __restrict__ rt,
                                                        const double* __restrict__ rf, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    int64_t I = (int64_t)blockIdx.x * (FS_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * (FS_BLOCK / 64);
    for (; I < nn_c; I += stride) {
        double acc[BC];
#pragma unroll
        for (int c = 0; c < BC; ++c) acc[c] = 0.0;
        for (int32_t q = pt_ptr[I] + lane; q < pt_ptr[I + 1]; q += 64) {
            const double* rr = rf + (int64_t)pt_row[q] * BR;
            double rv[BR];
#pragma unroll
            for (int r = 0; r < BR; ++r) rv[r] = rr[r];
            double blk[BR * BC];
            if ((BR * BC) % 2 == 0) {     // blocks are 16-byte (fp32: 8-byte) aligned
                typedef typename fs_pair_of<VT>::type VT2;
                const VT2* b2 = reinterpret_cast<const VT2*>(rt + (int64_t)q * BR * BC);
#pragma unroll
                for (int h = 0; h < BR * BC / 2; ++h) { const VT2 t = b2[h]; blk[2 * h] = (double)t.x; blk[2 * h + 1] = (double)t.y; }
            } else {
#pragma unroll
                for (int h = 0; h < BR * BC; ++h) blk[h] = (double)rt[(int64_t)q * BR * BC + h];
            }
#pragma unroll
            for (int c = 0; c < BC; ++c)
#pragma unroll
                for (int r = 0; r < BR; ++r) acc[c] += blk[c * BR + r] * rv[r];
        }
#pragma unroll
        for (int c = 0; c < BC; ++c) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_down(acc[c], off, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < BC; ++c) out[I * BC + c] = acc[c];
        }
    }
}

// d = scale * dinv*r ; x = (ADD ? x : 0) + d
template <bool ADD>
__global__ void k_cheb_first(int64_t n, const double* __restrict__ dinv, const double* __restrict__ r,
                             double* __restrict__ d, double* __restrict__ x, double scale) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double v = scale * dinv[i] * r[i];
        d[i] = v;
        x[i] = ADD ? x[i] + v : v;
    }
}
// d = c1 d + c2 dinv*r ; x += d
__global__ void k_cheb_next(int64_t n, const double* __restrict__ dinv, const double* __restrict__ r,
                            double* __restrict__ d, double* __restrict__ x, double c1, double c2) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double v = c1 * d[i] + c2 * dinv[i] * r[i];
        d[i] = v;
        x[i] += v;
    }
}
// the same two with the residual r = b - t formed on the fly (level 0: t = A x comes from the SELL product)
template <bool ADD>
__global__ void k_cheb_first_bt(int64_t n, const double* __restrict__ dinv, const double* __restrict__ b, const double* __restrict__ t,
                                double* __restrict__ d, double* __restrict__ x, double scale) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double v = scale * dinv[i] * (b[i] - t[i]);
        d[i] = v;
        x[i] = ADD ? x[i] + v : v;
    }
}
__global__ void k_cheb_next_bt(int64_t n, const double* __restrict__ dinv, const double* __restrict__ b, const double* __restrict__ t,
                               double* __restrict__ d, double* __restrict__ x, double c1, double c2) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double v = c1 * d[i] + c2 * dinv[i] * (b[i] - t[i]);
        d[i] = v;
        x[i] += v;
    }
}
__global__ void k_amg_sub(int64_t n, const double* __restrict__ b, const double* t, double* r) {   // r may alias t
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) r[i] = b[i] - t[i];
}
// y = a x + b y
__global__ void k_amg_axpby(int64_t n, double a, const double* __restrict__ x, double b, double* __restrict__ y) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) y[i] = a * x[i] + b * y[i];
}
__global__ void k_amg_scale_dinv(int64_t n, const double* __restrict__ dinv, double* __restrict__ v, double s) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) v[i] *= s * (dinv ? dinv[i] : 1.0);
}
__global__ void k_amg_div_dinv(int64_t n, const double* __restrict__ dinv, const double* __restrict__ v, double* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = v[i] / dinv[i];
}

__global__ void k_amg_seed(int64_t n, double* __restrict__ v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) v[i] = (double)(amg_hash((uint32_t)i * 2654435761U + 12345U) & 0xffffff) / 8388608.0 - 1.0;
}
// x = Cinv b, one wave per row
__global__ void k_dense_apply(int64_t n, const double* __restrict__ M, const double* __restrict__ b, double* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (; row < n; row += stride) {
        double acc = 0.0;
        for (int64_t c = lane; c < n; c += 64) acc += M[row * n + c] * b[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) x[row] = acc;
    }
}

// ---- host: products ------------------------------------------------------------------------------------
// C = L R with the left operand given as (lptr, lk, lidx, lval): plain block CSR (lidx = nullptr, TRANS=false)
// or the transpose index of P (TRANS=true).  wg = threads per output row.
static int spgemm(int64_t n_out, int64_t n_cols, int br, int bk, int bc, bool trans, const int32_t* lptr, const int32_t* lk,
                  const int32_t* lidx, const double* lval, const bcsr& R, int wg, bcsr* C, hipStream_t s) {
    C->nrows = n_out; C->ncols = n_cols; C->br = br; C->bc = bc;
    FS_CHECK(C->rowptr.alloc(n_out + 1));
    dbuf<int32_t> rowlen, flag;
    FS_CHECK(rowlen.alloc(n_out + 1));
    FS_CHECK(rowlen.zero(s));
    FS_CHECK(flag.alloc(1));
    const int grid = (int)std::min<int64_t>(n_out, 1 << 16);
    int cap = wg == 64 ? 256 : 1024;
    while (true) {
        FS_CHECK(flag.zero(s));
        hipLaunchKernelGGL(k_spgemm_symbolic<true>, dim3(grid), dim3(wg), (size_t)cap * 2 * sizeof(int32_t), s, n_out, lptr, lk, R.rowptr.p, R.col.p, cap, rowlen.p, (const int32_t*)nullptr, (int32_t*)nullptr, flag.p);
        FS_KERNEL_CHECK();
        int32_t of = 0;
        FS_CHECK(read_i32(flag.p, &of, s));
        if (!of) break;
        cap *= 2;
        FS_REQUIRE(cap <= 8192, "AMG setup: a product row has more than 8192 distinct columns");
    }
    amg_tick("    spgemm count");
    FS_CHECK(scan_exclusive(rowlen.p, C->rowptr.p, n_out + 1, s));
    int32_t nnz = 0;
    FS_CHECK(read_i32(C->rowptr.p + n_out, &nnz, s));
    C->nnz = nnz;
    FS_CHECK(C->col.alloc(nnz));
    FS_CHECK(C->val.alloc((int64_t)nnz * br * bc));
    amg_tick("    spgemm alloc");
    hipLaunchKernelGGL(k_spgemm_symbolic<false>, dim3(grid), dim3(wg), (size_t)cap * 2 * sizeof(int32_t), s, n_out, lptr, lk, R.rowptr.p, R.col.p, cap, (int32_t*)nullptr, C->rowptr.p, C->col.p, flag.p);
    FS_KERNEL_CHECK();
    amg_tick("    spgemm fill");
    // longest row -> LDS of the numeric pass
    int32_t maxlen = 0;
    {
        size_t tb = 0;
        dbuf<int32_t> mx;
        FS_CHECK(mx.alloc(1));
        FS_HIP(hipcub::DeviceReduce::Max(nullptr, tb, rowlen.p, mx.p, (int)n_out, s));
        dbuf<uint8_t> tmp;
        FS_CHECK(tmp.alloc((int64_t)tb + 16));
        FS_HIP(hipcub::DeviceReduce::Max(tmp.p, tb, rowlen.p, mx.p, (int)n_out, s));
        FS_CHECK(read_i32(mx.p, &maxlen, s));
    }
    amg_tick("    spgemm maxlen");
    maxlen = std::max(1, maxlen);
    const double items = (double)R.nnz / (double)std::max<int64_t>(1, R.nrows) * bc;   // lanes one product can use
    bool done = false;
#define FS_SPGEMM_SHAPE(T, BR_, BK_, BC_)                                                                          \
    if (!done && trans == T && br == BR_ && bk == BK_ && bc == BC_) {                                              \
        FS_CHECK((launch_spgemm_wave<T, BR_, BK_, BC_>(n_out, maxlen, items, lptr, lk, lidx, lval, R, C, s)));      \
        done = true;                                                                                                \
    }
    static const bool old_numeric = getenv("FS_AMG_SPGEMM_BLOCK") != nullptr;
    if (!old_numeric) {
        FS_SPGEMM_SHAPE(false, 3, 3, 6) FS_SPGEMM_SHAPE(true, 6, 3, 6) FS_SPGEMM_SHAPE(false, 6, 6, 6) FS_SPGEMM_SHAPE(true, 6, 6, 6)
        FS_SPGEMM_SHAPE(false, 1, 1, 1) FS_SPGEMM_SHAPE(true, 1, 1, 1) FS_SPGEMM_SHAPE(false, 3, 3, 3) FS_SPGEMM_SHAPE(true, 3, 3, 3)
    }
#undef FS_SPGEMM_SHAPE
    if (!done) {       // any other block shape: a workgroup per row, shapes at run time
        const size_t lds = (size_t)maxlen * br * bc * sizeof(double) + (size_t)maxlen * sizeof(int32_t) +
                           (size_t)FS_SPGEMM_STAGE * 4 * sizeof(int32_t);
        FS_REQUIRE(lds <= 160 * 1024 - 512, "AMG setup: a product row of %d blocks (%dx%d) exceeds the LDS accumulator", maxlen, br, bc);
        if (lds > 64 * 1024) {
            if (trans) FS_HIP(hipFuncSetAttribute((const void*)k_spgemm_numeric<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            else FS_HIP(hipFuncSetAttribute((const void*)k_spgemm_numeric<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        if (trans)
            hipLaunchKernelGGL(k_spgemm_numeric<true>, dim3(grid), dim3(wg), lds, s, n_out, maxlen, br, bk, bc, lptr, lk, lidx, lval, R.rowptr.p, R.col.p, R.val.p, C->rowptr.p, C->col.p, C->val.p);
        else
            hipLaunchKernelGGL(k_spgemm_numeric<false>, dim3(grid), dim3(wg), lds, s, n_out, maxlen, br, bk, bc, lptr, lk, lidx, lval, R.rowptr.p, R.col.p, R.val.p, C->rowptr.p, C->col.p, C->val.p);
        FS_KERNEL_CHECK();
    }
    FS_HIP(hipStreamSynchronize(s));
    amg_tick("    spgemm numeric");
    return FS_OK;
}

// ---- fp32 storage of what the V-cycle streams below the fine level ------------------------------------------------------------
// The V-cycle is a PRECONDITIONER: CG outside works on the fp64 operator with fp64 vectors and stops on the fp64 residual.  Its
// coarse operators (0.9 GB at level 1 of configs[2], four products per cycle) and its transfer operators are streamed once per
// use and bound by HBM, so they are kept rounded to fp32 - half the bytes; vectors, diagonals, eigenvalue bounds and every
// accumulation stay fp64 (a value is widened as it is loaded).  R is rounded from the same numbers as P (it stays P^T exactly) and a
// symmetric A_l stays symmetric up to what the two summation orders of the Galerkin product differed by before rounding.
// fs_set_option("amg_coarse_fp32", 0) / FS_AMG_FP32=0: fp64 storage throughout (round-4 behaviour).
static int g_amg_fp32 = -1;
void fs_amg_set_coarse_fp32(int on) { g_amg_fp32 = on ? 1 : 0; }
static bool amg_fp32() {
    if (g_amg_fp32 < 0) {
        const char* e = getenv("FS_AMG_FP32");
        g_amg_fp32 = (e && e[0] == '0') ? 0 : 1;
    }
    return g_amg_fp32 != 0;
}

__global__ void k_round_to_f32(int64_t n, const double* __restrict__ src, float* __restrict__ dst) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (float)src[i];
}
static int round_to_f32(const dbuf<double>& src, int64_t count, dbuf<float>& dst, hipStream_t s) {
    FS_CHECK(dst.alloc(std::max<int64_t>(count, 1)));
    if (count > 0) hipLaunchKernelGGL(k_round_to_f32, dim3(fs_grid_for(count, FS_BLOCK, 16384)), dim3(FS_BLOCK), 0, s, count, src.p, dst.p);
    FS_KERNEL_CHECK();
    return FS_OK;
}
// the level operator: only where the wave-per-node product (6 x 6 blocks) streams it
static bool level_uses_node_waves(const amg_level* L) {
    static const bool no_node = getenv("FS_AMG_NO_NODE_WAVES") != nullptr;
    return !no_node && L->bs == 6 && L->nn > 0 && L->A.nnz >= 4 * L->nn;
}
static int level_operator_to_f32(amg_level* L, hipStream_t s) {
    if (!amg_fp32() || !level_uses_node_waves(L)) return FS_OK;
    return round_to_f32(L->A.val, L->A.nnz * 36, L->A.val32, s);
}
// the transfer operators of a level: the block shapes with a templated restriction / prolongation
static int level_transfers_to_f32(amg_level* L, hipStream_t s) {
    if (!amg_fp32() || L->P.nnz <= 0) return FS_OK;
    if (!((L->P.br == 3 || L->P.br == 6) && L->P.bc == 6)) return FS_OK;
    const int64_t count = L->P.nnz * L->P.br * L->P.bc;
    FS_CHECK(round_to_f32(L->P.val, count, L->P.val32, s));
    return round_to_f32(L->rt_val, count, L->rt_val32, s);
}

static int coarse_level_spmv(amg_level* L, const double* x, const double* b, double* y, int mode, hipStream_t s);
static int level_spmv(fs_amg_s* M, int l, const double* x, const double* b, double* y, int mode, hipStream_t s) {
    amg_level* L = (l == 0 && M->dist0) ? M->dist0 : M->lv[l];
    if (l == 0) {
        if (mode == 0) return fs_spmv_dev(M->fine, x, y, s);
        FS_CHECK(fs_spmv_dev(M->fine, x, L->t.p, s));
        hipLaunchKernelGGL(k_amg_sub, dim3(fs_grid_for(L->n)), dim3(FS_BLOCK), 0, s, L->n, b, L->t.p, y);
        return FS_OK;
    }
    return coarse_level_spmv(L, x, b, y, mode, s);
}

// y = A_l x (mode 0) or b - A_l x (mode 1) on the level's own block CSR
static int coarse_level_spmv(amg_level* L, const double* x, const double* b, double* y, int mode, hipStream_t s) {
    // 6x6 blocks: a wave per node over the contiguous block row
    if (level_uses_node_waves(L)) {
        const int gg = fs_grid_for(L->nn * 64, FS_BLOCK, 1 << 20);
        if (L->A.val32.p) {
            if (mode) hipLaunchKernelGGL((k_bcsr_spmv_node<6, 1, float>), dim3(gg), dim3(FS_BLOCK), 0, s, L->nn, L->A.rowptr.p, L->A.col.p, L->A.val32.p, x, b, y);
            else hipLaunchKernelGGL((k_bcsr_spmv_node<6, 0, float>), dim3(gg), dim3(FS_BLOCK), 0, s, L->nn, L->A.rowptr.p, L->A.col.p, L->A.val32.p, x, b, y);
        } else {
            if (mode) hipLaunchKernelGGL((k_bcsr_spmv_node<6, 1>), dim3(gg), dim3(FS_BLOCK), 0, s, L->nn, L->A.rowptr.p, L->A.col.p, L->A.val.p, x, b, y);
            else hipLaunchKernelGGL((k_bcsr_spmv_node<6, 0>), dim3(gg), dim3(FS_BLOCK), 0, s, L->nn, L->A.rowptr.p, L->A.col.p, L->A.val.p, x, b, y);
        }
        return FS_OK;
    }
    // long rows on few nodes: 16 lanes per scalar row
    static const bool no_grp = getenv("FS_AMG_NO_ROW_GROUPS") != nullptr;
    if (!no_grp && L->nn > 0 && L->A.nnz >= 8 * L->nn && L->n <= ((int64_t)1 << 22)) {
        const int gg = (int)((L->n * 16 + FS_BLOCK - 1) / FS_BLOCK);
#define FS_BCSR_GRP dim3(gg), dim3(FS_BLOCK), 0, s, L->n, L->A.rowptr.p, L->A.col.p, L->A.val.p, x, b, y
        if (L->bs == 1) { if (mode) hipLaunchKernelGGL((k_bcsr_spmv_grp<1, 1, 16>), FS_BCSR_GRP); else hipLaunchKernelGGL((k_bcsr_spmv_grp<1, 0, 16>), FS_BCSR_GRP); return FS_OK; }
        if (L->bs == 3) { if (mode) hipLaunchKernelGGL((k_bcsr_spmv_grp<3, 1, 16>), FS_BCSR_GRP); else hipLaunchKernelGGL((k_bcsr_spmv_grp<3, 0, 16>), FS_BCSR_GRP); return FS_OK; }
        if (L->bs == 6) { if (mode) hipLaunchKernelGGL((k_bcsr_spmv_grp<6, 1, 16>), FS_BCSR_GRP); else hipLaunchKernelGGL((k_bcsr_spmv_grp<6, 0, 16>), FS_BCSR_GRP); return FS_OK; }
#undef FS_BCSR_GRP
    }
    const int g = fs_grid_for(L->n, FS_BLOCK, 8192);
#define FS_BCSR_ARGS dim3(g), dim3(FS_BLOCK), 0, s, L->n, L->A.rowptr.p, L->A.col.p, L->A.val.p, x, b, y
    if (L->bs == 1) { if (mode) hipLaunchKernelGGL((k_bcsr_spmv<1, 1>), FS_BCSR_ARGS); else hipLaunchKernelGGL((k_bcsr_spmv<1, 0>), FS_BCSR_ARGS); }
    else if (L->bs == 3) { if (mode) hipLaunchKernelGGL((k_bcsr_spmv<3, 1>), FS_BCSR_ARGS); else hipLaunchKernelGGL((k_bcsr_spmv<3, 0>), FS_BCSR_ARGS); }
    else if (L->bs == 6) { if (mode) hipLaunchKernelGGL((k_bcsr_spmv<6, 1>), FS_BCSR_ARGS); else hipLaunchKernelGGL((k_bcsr_spmv<6, 0>), FS_BCSR_ARGS); }
    else { fs_set_error("AMG: unsupported block size %d", L->bs); return FS_ERR_UNSUPPORTED; }
#undef FS_BCSR_ARGS
    return FS_OK;
}

// setup-time SpMV on the level's own block CSR (level 0 included)
static int bcsr_spmv_setup(amg_level* L, const double* x, double* y, hipStream_t s) {
    if (L->nn > 0 && L->A.nnz >= 8 * L->nn && L->n <= ((int64_t)1 << 22)) {      // long rows: 16 lanes per scalar row
        const int gg = (int)((L->n * 16 + FS_BLOCK - 1) / FS_BLOCK);
#define FS_BCSR_GRP dim3(gg), dim3(FS_BLOCK), 0, s, L->n, L->A.rowptr.p, L->A.col.p, L->A.val.p, x, (const double*)nullptr, y
        if (L->bs == 1) { hipLaunchKernelGGL((k_bcsr_spmv_grp<1, 0, 16>), FS_BCSR_GRP); return FS_OK; }
        if (L->bs == 3) { hipLaunchKernelGGL((k_bcsr_spmv_grp<3, 0, 16>), FS_BCSR_GRP); return FS_OK; }
        if (L->bs == 6) { hipLaunchKernelGGL((k_bcsr_spmv_grp<6, 0, 16>), FS_BCSR_GRP); return FS_OK; }
#undef FS_BCSR_GRP
    }
    const int g = fs_grid_for(L->n, FS_BLOCK, 8192);
#define FS_BCSR_ARGS dim3(g), dim3(FS_BLOCK), 0, s, L->n, L->A.rowptr.p, L->A.col.p, L->A.val.p, x, (const double*)nullptr, y
    if (L->bs == 1) hipLaunchKernelGGL((k_bcsr_spmv<1, 0>), FS_BCSR_ARGS);
    else if (L->bs == 3) hipLaunchKernelGGL((k_bcsr_spmv<3, 0>), FS_BCSR_ARGS);
    else if (L->bs == 6) hipLaunchKernelGGL((k_bcsr_spmv<6, 0>), FS_BCSR_ARGS);
    else { fs_set_error("AMG: unsupported block size %d", L->bs); return FS_ERR_UNSUPPORTED; }
#undef FS_BCSR_ARGS
    return FS_OK;
}

// set-up products of a level >= 1: the product of the V-cycle where the level is one of 6 x 6 blocks (a wave per node over the
// fp32 values: 15 power-iteration steps on level 1 of configs[2] 4.4 -> ms), else the per-row kernels above
static int coarse_product(amg_level* L, const double* x, double* y, hipStream_t s) {
    if (level_uses_node_waves(L)) return coarse_level_spmv(L, x, nullptr, y, 0, s);
    return bcsr_spmv_setup(L, x, y, s);
}

static int dot_host(fs_amg_s* M, const double* x, const double* y, int64_t n, double* out, hipStream_t s) {
    const int g = fs_grid_for(n, FS_BLOCK, 1024);
    hipLaunchKernelGGL(k_dot_partial, dim3(g), dim3(FS_BLOCK), 0, s, x, y, n, M->partials.p);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(FS_SUM_BLOCK), 0, s, M->partials.p, g, 1, M->sums.p);
    FS_KERNEL_CHECK();
    FS_CHECK(M->sums.download(out, 1, s));
    return FS_OK;
}

// largest eigenvalue of D^-1 A by power iteration (deterministic start)
static int estimate_lmax(fs_amg_s* M, amg_level* L, int steps, hipStream_t s) {
    // level 0: the tuned SELL/DIA product of the fine matrix (332 us at configs[2]) instead of the block-CSR copy
    // (607 us); its input carries the ghost entries of a decomposed space, which stay zero (rank-local block)
    const bool fine = L == M->lv[0] && M->fine != nullptr;
    const int64_t nloc = fine ? M->fine->space->n_dofs_local : L->n;
    dbuf<double> v, w;
    FS_CHECK(v.alloc(nloc));
    FS_CHECK(w.alloc(nloc));
    FS_CHECK(v.zero(s));
    FS_CHECK(w.zero(s));
    hipLaunchKernelGGL(k_amg_seed, dim3(fs_grid_for(L->n)), dim3(FS_BLOCK), 0, s, L->n, v.p);
    // No normalisation and no host round trip inside the loop (round 1: one synchronising dot per step, 21 + 19 ms of the
    // 160 ms set-up at configs[2], most of it latency on the small levels): the iterate grows by at most the Gershgorin
    // bound per step, 1e300 is far away for any sensible step count.  The estimate is the Rayleigh quotient of the
    // last iterate, (v, A v) / (v, D v) - that of D^-1/2 A D^-1/2 at D^1/2 v - whose error is the square of the
    // iterate's, so half the steps of a norm ratio do (two dots and one scaling, once).
    const double growth = L->gersh > 1.0 ? L->gersh : 1.0;
    int safe = steps;
    while (safe > 1 && safe * log10(growth) > 250.0) --safe;
    // the fine products through the row dictionary where the rows repeat (uniform boxes: 60 instead of 328 us at configs[2])
    struct dict_guard { bool on = false; ~dict_guard() { if (on) fs_dict_end(); } } dict_scope;
    static const bool lmax_dict = !(getenv("FS_AMG_LMAX_DICT") && getenv("FS_AMG_LMAX_DICT")[0] == '0');
    if (fine && lmax_dict) {
        dict_scope.on = true;
        FS_CHECK(fs_dict_begin(M->fine, s));
    }
    for (int it = 0; it + 1 < safe; ++it) {
        if (fine) FS_CHECK(fs_spmv_dev(M->fine, v.p, w.p, s));
        else FS_CHECK(coarse_product(L, v.p, w.p, s));
        hipLaunchKernelGGL(k_amg_scale_dinv, dim3(fs_grid_for(L->n)), dim3(FS_BLOCK), 0, s, L->n, L->dinv.p, w.p, 1.0);
        std::swap(v.p, w.p);
    }
    if (fine) FS_CHECK(fs_spmv_dev(M->fine, v.p, w.p, s));
    else FS_CHECK(coarse_product(L, v.p, w.p, s));
    double num = 0.0, den = 0.0;
    FS_CHECK(dot_host(M, v.p, w.p, L->n, &num, s));
    hipLaunchKernelGGL(k_amg_div_dinv, dim3(fs_grid_for(L->n)), dim3(FS_BLOCK), 0, s, L->n, L->dinv.p, v.p, w.p);
    FS_CHECK(dot_host(M, v.p, w.p, L->n, &den, s));
    const double lam = den > 0.0 ? num / den : 0.0;
    L->lmax = (lam > 0.0 && lam == lam && lam < 1e300) ? std::min(1.1 * lam, L->gersh) : L->gersh;
    if (getenv("FS_AMG_DEBUG")) fprintf(stderr, "[fs_amg_setup]   lambda_max(D^-1 A) ~ %.6f after %d steps (Gershgorin %.4f)\n", lam, safe, L->gersh);
    return FS_OK;
}

// FS_AMG_DEBUG=1: per-phase wall time of the setup on stderr
static void amg_tick(const char* what) {
    static std::chrono::steady_clock::time_point last;
    static const bool debug = getenv("FS_AMG_DEBUG") != nullptr;
    if (!debug) return;
    (void)hipStreamSynchronize(fs_rt().stream);
    const auto now = std::chrono::steady_clock::now();
    if (what) fprintf(stderr, "[fs_amg_setup] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
}

// ---- host: one coarsening step.  Returns *stop = 1 when no useful coarse level results ------------------
// transpose index of L->P (nn x n_agg blocks): entries sorted by column (stable: ascending fine row inside a column), R = P^T
// blocks in that order
static int build_p_transpose(amg_level* L, int64_t nn, int64_t n_agg, int bs, int nb, hipStream_t s) {
    const int64_t pn = L->P.nnz;
    const int g = fs_grid_for(nn);
    dbuf<int32_t> k2, ids, prow;
    FS_CHECK(k2.alloc(std::max<int64_t>(pn, 1))); FS_CHECK(ids.alloc(std::max<int64_t>(pn, 1))); FS_CHECK(prow.alloc(std::max<int64_t>(pn, 1)));
    FS_CHECK(L->pt_entry.alloc(std::max<int64_t>(pn, 1))); FS_CHECK(L->pt_row.alloc(std::max<int64_t>(pn, 1))); FS_CHECK(L->pt_ptr.alloc(n_agg + 1));
    hipLaunchKernelGGL(k_iota, dim3(fs_grid_for(pn)), dim3(FS_BLOCK), 0, s, ids.p, pn);
    hipLaunchKernelGGL(k_expand_rows, dim3(g), dim3(FS_BLOCK), 0, s, L->P.rowptr.p, nn, prow.p);
    if (pn > 0) FS_CHECK(sort_pairs(L->P.col.p, k2.p, ids.p, L->pt_entry.p, pn, s));
    hipLaunchKernelGGL(k_lower_bounds, dim3(fs_grid_for(n_agg + 1)), dim3(FS_BLOCK), 0, s, k2.p, pn, (int64_t)n_agg, L->pt_ptr.p);
    hipLaunchKernelGGL(k_gather_i32, dim3(fs_grid_for(pn)), dim3(FS_BLOCK), 0, s, prow.p, L->pt_entry.p, pn, L->pt_row.p);
    FS_CHECK(L->rt_val.alloc(std::max<int64_t>(pn * bs * nb, 1)));
    hipLaunchKernelGGL(k_transpose_blocks, dim3(fs_grid_for(pn * bs * nb, FS_BLOCK, 8192)), dim3(FS_BLOCK), 0, s, pn, bs, nb, L->pt_entry.p, L->P.val.p, L->rt_val.p);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

static int coarsen(fs_amg_s* M, amg_level* L, double theta, int eig_steps, amg_level** out, hipStream_t s) {
    *out = nullptr;
    const int64_t nn = L->nn;
    const int bs = L->bs, nb = L->nb;
    const int g = fs_grid_for(nn, FS_BLOCK, 8192);
    // diagonal quantities
    dbuf<double> dnorm;
    dbuf<unsigned long long> gbits;
    FS_CHECK(dnorm.alloc(nn));
    FS_CHECK(gbits.alloc(1));
    FS_CHECK(gbits.zero(s));
    FS_CHECK(L->dinv.alloc(L->n));
    FS_CHECK(L->ident.alloc(L->n));
    FS_REQUIRE(bs <= 6, "AMG setup: block size %d (the diagonal kernel keeps six rows per lane)", bs);
    hipLaunchKernelGGL(k_amg_diag_grp, dim3(fs_grid_for(nn * 16, FS_BLOCK, 65536)), dim3(FS_BLOCK), 0, s, nn, bs, L->A.rowptr.p, L->A.col.p, L->A.val.p, L->dinv.p, L->ident.p, dnorm.p, gbits.p);
    FS_KERNEL_CHECK();
    unsigned long long hb = 0;
    FS_HIP(hipMemcpyAsync(&hb, gbits.p, 8, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    memcpy(&L->gersh, &hb, 8);
    if (!(L->gersh > 0.0)) L->gersh = 2.0;
    FS_CHECK(estimate_lmax(M, L, eig_steps, s));
    amg_tick("  diag+lmax");
    if (nb <= 0) return FS_OK;   // coarsest level: only the smoother data

    // strength graph
    dbuf<int32_t> scnt, sptr, scol;
    dbuf<double> sw;
    FS_CHECK(scnt.alloc(nn + 1));
    FS_CHECK(scnt.zero(s));
    FS_CHECK(sptr.alloc(nn + 1));
#define FS_STRENGTH_ARGS dim3(fs_grid_for(nn * 16, FS_BLOCK, 65536)), dim3(FS_BLOCK), 0, s, nn, bs, L->A.rowptr.p, L->A.col.p, L->A.val.p, dnorm.p, theta * theta
    if (bs >= 4) hipLaunchKernelGGL((k_strength_grp<false, true>), FS_STRENGTH_ARGS, scnt.p, (const int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr);
    else hipLaunchKernelGGL((k_strength_grp<false, false>), FS_STRENGTH_ARGS, scnt.p, (const int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr);
    FS_KERNEL_CHECK();
    FS_CHECK(scan_exclusive(scnt.p, sptr.p, nn + 1, s));
    int32_t snnz = 0;
    FS_CHECK(read_i32(sptr.p + nn, &snnz, s));
    if (snnz == 0) return FS_OK;
    FS_CHECK(scol.alloc(snnz));
    FS_CHECK(sw.alloc(snnz));
    if (bs >= 4) hipLaunchKernelGGL((k_strength_grp<true, true>), FS_STRENGTH_ARGS, (int32_t*)nullptr, sptr.p, scol.p, sw.p);
    else hipLaunchKernelGGL((k_strength_grp<true, false>), FS_STRENGTH_ARGS, (int32_t*)nullptr, sptr.p, scol.p, sw.p);
#undef FS_STRENGTH_ARGS
    FS_KERNEL_CHECK();

    amg_tick("  strength");
    // MIS(2)
    dbuf<unsigned long long> key, m1, m2;
    dbuf<int32_t> undecided;
    FS_CHECK(key.alloc(nn)); FS_CHECK(m1.alloc(nn)); FS_CHECK(m2.alloc(nn));
    FS_CHECK(undecided.alloc(1));
    hipLaunchKernelGGL(k_mis_init, dim3(g), dim3(FS_BLOCK), 0, s, nn, sptr.p, key.p);
    for (int round = 0;; ++round) {
        FS_REQUIRE(round < 200, "AMG setup: MIS(2) did not terminate");
        FS_CHECK(undecided.zero(s));
        hipLaunchKernelGGL(k_mis_max, dim3(g), dim3(FS_BLOCK), 0, s, nn, sptr.p, scol.p, key.p, m1.p);
        hipLaunchKernelGGL(k_mis_max, dim3(g), dim3(FS_BLOCK), 0, s, nn, sptr.p, scol.p, m1.p, m2.p);
        hipLaunchKernelGGL(k_mis_update, dim3(g), dim3(FS_BLOCK), 0, s, nn, key.p, m2.p, undecided.p);
        FS_KERNEL_CHECK();
        int32_t left = 0;
        FS_CHECK(read_i32(undecided.p, &left, s));
        if (left == 0) break;
    }
    amg_tick("  mis2");
    // aggregates
    dbuf<int32_t> flag, rootid, agg1, agg;
    FS_CHECK(flag.alloc(nn + 1)); FS_CHECK(rootid.alloc(nn + 1)); FS_CHECK(agg1.alloc(nn)); FS_CHECK(agg.alloc(nn));
    hipLaunchKernelGGL(k_agg_rootflag, dim3(g), dim3(FS_BLOCK), 0, s, nn, key.p, flag.p);
    FS_CHECK(scan_exclusive(flag.p, rootid.p, nn + 1, s));
    int32_t n_agg = 0;
    FS_CHECK(read_i32(rootid.p + nn, &n_agg, s));
    if (n_agg == 0 || (int64_t)n_agg * nb >= L->n) return FS_OK;   // no reduction
    hipLaunchKernelGGL(k_agg_pass1, dim3(g), dim3(FS_BLOCK), 0, s, nn, sptr.p, scol.p, key.p, rootid.p, agg1.p);
    hipLaunchKernelGGL(k_agg_pass2, dim3(g), dim3(FS_BLOCK), 0, s, nn, sptr.p, scol.p, sw.p, agg1.p, agg.p);
    FS_KERNEL_CHECK();
    // member lists
    dbuf<int32_t> skey, skey2, sval, members, agg_ptr, has, tptr;
    FS_CHECK(skey.alloc(nn)); FS_CHECK(skey2.alloc(nn)); FS_CHECK(sval.alloc(nn)); FS_CHECK(members.alloc(nn));
    FS_CHECK(agg_ptr.alloc(n_agg + 1)); FS_CHECK(has.alloc(nn + 1)); FS_CHECK(tptr.alloc(nn + 1));
    hipLaunchKernelGGL(k_agg_sortkey, dim3(g), dim3(FS_BLOCK), 0, s, nn, agg.p, n_agg, skey.p, has.p);
    hipLaunchKernelGGL(k_iota, dim3(g), dim3(FS_BLOCK), 0, s, sval.p, nn);
    FS_CHECK(sort_pairs(skey.p, skey2.p, sval.p, members.p, nn, s));
    hipLaunchKernelGGL(k_lower_bounds, dim3(fs_grid_for(n_agg + 1)), dim3(FS_BLOCK), 0, s, skey2.p, nn, (int64_t)n_agg, agg_ptr.p);
    FS_CHECK(scan_exclusive(has.p, tptr.p, nn + 1, s));
    int32_t n_t = 0;
    FS_CHECK(read_i32(tptr.p + nn, &n_t, s));

    amg_tick("  aggregates");
    // tentative prolongator + coarse near-null space
    amg_level* C = new amg_level();
    C->nn = n_agg; C->bs = nb; C->n = (int64_t)n_agg * nb; C->nb = nb;
    dbuf<double> T;
    FS_CHECK(T.alloc(L->n * nb));
    FS_CHECK(T.zero(s));
    FS_CHECK(C->B.alloc(C->n * nb));
    static const bool serial_qr = getenv("FS_AMG_SERIAL_QR") != nullptr;
    if (serial_qr)
        hipLaunchKernelGGL(k_tentative, dim3(fs_grid_for(n_agg, 64, 8192)), dim3(64), 0, s, (int64_t)n_agg, bs, nb, agg_ptr.p, members.p, L->B.p, L->ident.p, T.p, C->B.p);
    else
        hipLaunchKernelGGL(k_tentative_wave, dim3((unsigned)std::min<int64_t>(n_agg, 1 << 20)), dim3(64), 0, s, (int64_t)n_agg, bs, nb, agg_ptr.p, members.p, L->B.p, L->ident.p, T.p, C->B.p);
    FS_KERNEL_CHECK();
    bcsr Tm;
    Tm.nrows = nn; Tm.ncols = n_agg; Tm.br = bs; Tm.bc = nb; Tm.nnz = n_t;
    FS_CHECK(Tm.col.alloc(n_t));
    FS_CHECK(Tm.val.alloc((int64_t)n_t * bs * nb));
    hipLaunchKernelGGL(k_t_fill, dim3(g), dim3(FS_BLOCK), 0, s, nn, bs * nb, agg.p, tptr.p, T.p, Tm.col.p, Tm.val.p);
    FS_KERNEL_CHECK();
    std::swap(Tm.rowptr.p, tptr.p); std::swap(Tm.rowptr.n, tptr.n);

    amg_tick("  tentative");
    // P = (I - omega D^-1 A) T
    FS_CHECK(spgemm(nn, n_agg, bs, bs, nb, false, L->A.rowptr.p, L->A.col.p, nullptr, L->A.val.p, Tm, 64, &L->P, s));
    const double omega = 4.0 / (3.0 * L->lmax);
    hipLaunchKernelGGL(k_smooth_p_grp, dim3(fs_grid_for(nn * 16, FS_BLOCK, 65536)), dim3(FS_BLOCK), 0, s, nn, bs, nb, L->P.rowptr.p, L->P.col.p, L->P.val.p, L->dinv.p, agg.p, T.p, omega);
    FS_KERNEL_CHECK();
    L->n_agg = n_agg;
    amg_tick("  smoothed P");
    // transpose index of P
    FS_CHECK(build_p_transpose(L, nn, n_agg, bs, nb, s));
    FS_CHECK(level_transfers_to_f32(L, s));
    amg_tick("  transpose");
    // A_c = P^T (A P)
    {
        bcsr AP;
        FS_CHECK(spgemm(nn, n_agg, bs, bs, nb, false, L->A.rowptr.p, L->A.col.p, nullptr, L->A.val.p, L->P, bs * nb >= 36 ? FS_BLOCK : 64, &AP, s));
        // few, long output rows on the coarser levels (4 192 rows of ~150 blocks of 6x6 at level 2 of configs[2]): a larger
        // workgroup shortens the serial loop over the products of a row
        const int wg_rap = n_agg < 32768 ? 1024 : 512;
        FS_CHECK(spgemm(n_agg, n_agg, nb, bs, nb, true, L->pt_ptr.p, L->pt_row.p, L->pt_entry.p, L->P.val.p, AP, wg_rap, &C->A, s));
    }
    amg_tick("  RAP");
    hipLaunchKernelGGL(k_fix_dead, dim3(fs_grid_for(n_agg)), dim3(FS_BLOCK), 0, s, (int64_t)n_agg, nb, C->A.rowptr.p, C->A.col.p, C->A.val.p);
    FS_KERNEL_CHECK();
    FS_CHECK(level_operator_to_f32(C, s));
    FS_HIP(hipStreamSynchronize(s));
    L->agg.swap(agg);
    *out = C;
    return FS_OK;
}

// dense inverse of the coarsest operator on the host (Gauss-Jordan, partial pivoting)
static int coarse_inverse(fs_amg_s* M, amg_level* L, hipStream_t s) {
    const int64_t n = L->n, nn = L->nn;
    const int bs = L->bs;
    std::vector<int32_t> rp(nn + 1), ci(L->A.nnz);
    std::vector<double> va((size_t)L->A.nnz * bs * bs);
    FS_CHECK(L->A.rowptr.download(rp.data(), nn + 1, s));
    FS_CHECK(L->A.col.download(ci.data(), L->A.nnz, s));
    FS_CHECK(L->A.val.download(va.data(), (int64_t)va.size(), s));
    std::vector<double> a((size_t)n * n, 0.0), inv((size_t)n * n, 0.0);
    for (int64_t i = 0; i < nn; ++i)
        for (int32_t e = rp[i]; e < rp[i + 1]; ++e)
            for (int r = 0; r < bs; ++r)
                for (int c = 0; c < bs; ++c) a[(size_t)(i * bs + r) * n + (size_t)ci[e] * bs + c] = va[((size_t)e * bs + r) * bs + c];
    for (int64_t i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
    for (int64_t k = 0; k < n; ++k) {
        int64_t piv = k;
        double best = fabs(a[(size_t)k * n + k]);
        for (int64_t i = k + 1; i < n; ++i)
            if (fabs(a[(size_t)i * n + k]) > best) { best = fabs(a[(size_t)i * n + k]); piv = i; }
        if (!(best > 0.0)) { fs_set_error("AMG setup: coarsest operator is singular"); return FS_ERR_NUMERIC; }
        if (piv != k)
            for (int64_t c = 0; c < n; ++c) {
                std::swap(a[(size_t)k * n + c], a[(size_t)piv * n + c]);
                std::swap(inv[(size_t)k * n + c], inv[(size_t)piv * n + c]);
            }
        const double d = 1.0 / a[(size_t)k * n + k];
        for (int64_t c = 0; c < n; ++c) { a[(size_t)k * n + c] *= d; inv[(size_t)k * n + c] *= d; }
        for (int64_t i = 0; i < n; ++i) {
            if (i == k) continue;
            const double f = a[(size_t)i * n + k];
            if (f == 0.0) continue;
            for (int64_t c = 0; c < n; ++c) {
                a[(size_t)i * n + c] -= f * a[(size_t)k * n + c];
                inv[(size_t)i * n + c] -= f * inv[(size_t)k * n + c];
            }
        }
    }
    FS_CHECK(M->cinv.alloc(n * n));
    FS_CHECK(M->cinv.upload(inv.data(), n * n, s));
    M->nc = n;
    return FS_OK;
}

// ---- C-ABI: setup ---------------------------------------------------------------------------------------
extern "C" int fs_amg_setup(fs_matrix_t A, int n_nullspace, const double* nullspace, const fs_amg_opts* opts,
                            fs_amg_t* out) {
    FS_REFUSE_DG(A, "fs_amg_setup");
    FS_CHECK(fs_require_init());
    FS_REQUIRE(A && out, "fs_amg_setup: null pointer");
    fs_space_s* sp = A->space;
    // Multi-GPU: the hierarchy is built on this rank's diagonal block (ghost columns dropped) - the subdomain solver
    // of a non-overlapping additive Schwarz preconditioner; fs_amg_apply then expects zero ghost entries in z.
    const bool local_block = sp->n_nodes_local > sp->n_nodes_owned;
    FS_REQUIRE(A->bs == 1 || A->bs == 3, "fs_amg_setup: block size %d", A->bs);
    const bool rigid = !nullspace && opts && opts->rigid_body_modes != 0;
    FS_REQUIRE(!rigid || (A->bs == 3 && sp->mesh->tdim == 3 && (sp->degree == 1 || sp->edges.p)),
               "fs_amg_setup: rigid-body modes are built for 3-vector CG1 / CG2 spaces on tetrahedra");
    const int nb = nullspace ? n_nullspace : (rigid ? 6 : A->bs);
    FS_REQUIRE(nb == 1 || nb == 3 || nb == 6, "fs_amg_setup: %d near-null-space vectors (1, 3 or 6 are built)", nb);
    // the transfers of level 0 are blocks of bs x nb: the V-cycle has a restriction for 1 x 1, 3 x 3, 3 x 6 (and 6 x 6 below) only -
    // any other pair would pass the set-up through the run-time-shaped SpGEMM and fail in the first fs_amg_apply
    FS_REQUIRE((A->bs == 1 && nb == 1) || (A->bs == 3 && (nb == 3 || nb == 6)),
               "fs_amg_setup: %d near-null-space vectors for a matrix of %d x %d blocks: no restriction is built for %d x %d transfer blocks "
               "(1 vector for scalar matrices, 3 or 6 for 3 x 3 blocks)", nb, A->bs, A->bs, A->bs, nb);
    // 0 = default 0.05; negative = keep every coupling above the summation-order noise (1e-8)
    const double theta = (!opts || opts->strength_threshold == 0.0) ? 0.05 : std::max(opts->strength_threshold, 1e-8);
    const int max_levels = opts && opts->max_levels > 0 ? opts->max_levels : 10;
    const int coarse_size = opts && opts->coarse_size > 0 ? opts->coarse_size : 500;
    const int eig_steps = opts && opts->eig_steps > 0 ? opts->eig_steps : 15;
    hipStream_t s = fs_rt().stream;
    const auto t0 = std::chrono::steady_clock::now();
    amg_tick(nullptr);
#define tick amg_tick

    fs_amg_s* M = new fs_amg_s();
    M->fine = A;
    M->smooth_steps = opts && opts->smoother_steps > 0 ? opts->smoother_steps : 2;
    int rc = FS_OK;
    auto fail = [&](int code) { delete M; return code; };
    if ((rc = M->partials.alloc(FS_MAX_PARTIAL_BLOCKS * 4)) != FS_OK) return fail(rc);
    if ((rc = M->sums.alloc(8)) != FS_OK) return fail(rc);

    amg_level* L0 = new amg_level();
    M->lv.push_back(L0);
    L0->nn = sp->n_nodes_owned; L0->bs = A->bs; L0->n = sp->n_dofs_owned; L0->nb = nb;
    L0->A.nrows = L0->A.ncols = L0->nn; L0->A.br = L0->A.bc = A->bs; L0->A.nnz = sp->nnz_nodes;
    if ((rc = L0->A.rowptr.alloc(L0->nn + 1)) != FS_OK) return fail(rc);
    if ((rc = L0->A.col.alloc(sp->nnz_nodes)) != FS_OK) return fail(rc);
    if ((rc = L0->A.val.alloc(sp->nnz_nodes * A->bs * A->bs)) != FS_OK) return fail(rc);
    if (hipMemcpyAsync(L0->A.rowptr.p, sp->rowptr.p, (size_t)(L0->nn + 1) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(L0->A.col.p, sp->colidx.p, (size_t)sp->nnz_nodes * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        fs_set_error("fs_amg_setup: device copy failed");
        return fail(FS_ERR_HIP);
    }
    fs_dispatch_int<1, 3>(A->bs, [&](auto BS) {
        hipLaunchKernelGGL(k_amg_extract<decltype(BS)::value>, dim3(fs_grid_for(L0->nn)), dim3(FS_BLOCK), 0, s, L0->nn, sp->slice_ptr.p, sp->rowptr.p, sp->sell_col.p, A->val.p, sp->sell_entries, L0->A.val.p);
    });
    // near-null space [n][nb] (the caller's layout is [nb][n]: transposed on the device)
    {
        if ((rc = L0->B.alloc(L0->n * nb)) != FS_OK) return fail(rc);
        dbuf<double> raw;
        if (nullspace) {
            if ((rc = raw.alloc(L0->n * nb)) != FS_OK) return fail(rc);
            if ((rc = raw.upload(nullspace, L0->n * nb, s)) != FS_OK) return fail(rc);
        }
        if (rigid)
            hipLaunchKernelGGL(k_rigid_body_modes, dim3(fs_grid_for(L0->nn, FS_BLOCK, 8192)), dim3(FS_BLOCK), 0, s, L0->nn,
                               sp->degree == 1 ? L0->nn : sp->mesh->n_owned, sp->degree == 1 ? (const int32_t*)nullptr : sp->edges.p,
                               sp->mesh->xyz.p, L0->B.p);
        else
            hipLaunchKernelGGL(k_nullspace_layout, dim3(fs_grid_for(L0->n * nb, FS_BLOCK, 8192)), dim3(FS_BLOCK), 0, s, L0->n, nb, A->bs, (const double*)raw.p, L0->B.p);
        if (hipStreamSynchronize(s) != hipSuccess) { fs_set_error("fs_amg_setup: near-null-space upload failed"); return fail(FS_ERR_HIP); }
    }
    if (local_block) {
        const int bs2 = A->bs * A->bs;
        dbuf<int32_t> cnt, nrp, nci;
        dbuf<double> nval;
        if ((rc = cnt.alloc(L0->nn + 1)) != FS_OK || (rc = nrp.alloc(L0->nn + 1)) != FS_OK) return fail(rc);
        hipLaunchKernelGGL(k_count_owned_cols, dim3(fs_grid_for(L0->nn + 1)), dim3(FS_BLOCK), 0, s, L0->nn, L0->A.rowptr.p, L0->A.col.p, cnt.p);
        if ((rc = scan_exclusive(cnt.p, nrp.p, L0->nn + 1, s)) != FS_OK) return fail(rc);
        int32_t kept = 0;
        if ((rc = read_i32(nrp.p + L0->nn, &kept, s)) != FS_OK) return fail(rc);
        if ((rc = nci.alloc(std::max<int64_t>(kept, 1))) != FS_OK || (rc = nval.alloc(std::max<int64_t>(kept, 1) * bs2)) != FS_OK) return fail(rc);
        hipLaunchKernelGGL(k_compact_owned_cols, dim3(fs_grid_for(L0->nn)), dim3(FS_BLOCK), 0, s, L0->nn, bs2, L0->A.rowptr.p, L0->A.col.p,
                           L0->A.val.p, nrp.p, nci.p, nval.p);
        if (hipStreamSynchronize(s) != hipSuccess) { fs_set_error("fs_amg_setup: compaction of the local block failed"); return fail(FS_ERR_HIP); }
        L0->A.rowptr.swap(nrp);
        L0->A.col.swap(nci);
        L0->A.val.swap(nval);
        L0->A.nnz = kept;
    }
    tick("extract+nullspace");
    double nnz_scalar0 = (double)L0->A.nnz * A->bs * A->bs, nnz_total = nnz_scalar0, n_total = (double)L0->n;
    while (true) {
        amg_level* L = M->lv.back();
        const bool last = (int)M->lv.size() >= max_levels || L->n <= coarse_size;
        if (last) L->nb = 0;
        amg_level* C = nullptr;
        if ((rc = coarsen(M, L, theta, eig_steps, &C, s)) != FS_OK) return fail(rc);
        tick("coarsen level");
        if (!C) { L->nb = 0; break; }
        M->lv.push_back(C);
        nnz_total += (double)C->A.nnz * C->bs * C->bs;
        n_total += (double)C->n;
    }
    M->op_complexity = nnz_total / nnz_scalar0;
    M->grid_complexity = n_total / (double)L0->n;
    // work vectors
    for (size_t l = 0; l < M->lv.size(); ++l) {
        amg_level* L = M->lv[l];
        if ((rc = L->r.alloc(L->n)) != FS_OK || (rc = L->d.alloc(L->n)) != FS_OK || (rc = L->t.alloc(L->n)) != FS_OK) return fail(rc);
        if (l > 0 && ((rc = L->x.alloc(L->n)) != FS_OK || (rc = L->b.alloc(L->n)) != FS_OK)) return fail(rc);
    }
    amg_level* Lc = M->lv.back();
    if (Lc->n <= 2500 && M->lv.size() > 1) {
        if ((rc = coarse_inverse(M, Lc, s)) != FS_OK) return fail(rc);
    }
    tick("vectors + coarse inverse");
    FS_HIP(hipStreamSynchronize(s));
    M->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = M;
    return FS_OK;
}

// ---- distributed fine level under the replicated hierarchy ----------------------------------------------------------------
__global__ void k_sel_row_lengths(int64_t n_sel, const int32_t* __restrict__ sel, const int32_t* __restrict__ rowptr, int32_t* __restrict__ len) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i <= n_sel; i += stride) len[i] = i < n_sel ? rowptr[sel[i] + 1] - rowptr[sel[i]] : 0;
}
__global__ void k_sel_copy_rows(int64_t n_sel, const int32_t* __restrict__ sel, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                const double* __restrict__ val, int bb, const int32_t* __restrict__ new_ptr, int32_t* __restrict__ new_col,
                                double* __restrict__ new_val) {
    const int lane = threadIdx.x & 63;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (; i < n_sel; i += stride) {
        const int32_t s0 = rowptr[sel[i]], len = rowptr[sel[i] + 1] - s0, d0 = new_ptr[i];
        for (int32_t e = lane; e < len; e += 64) new_col[d0 + e] = col[s0 + e];
        for (int64_t e = lane; e < (int64_t)len * bb; e += 64) new_val[(int64_t)d0 * bb + e] = val[(int64_t)s0 * bb + e];
    }
}
__global__ void k_sel_gather_dofs(int64_t n_sel, const int32_t* __restrict__ sel, int bs, const double* __restrict__ src, double* __restrict__ dst) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n_sel * bs; i += stride) dst[i] = src[(int64_t)sel[i / bs] * bs + i % bs];
}

// M was set up on the UNDECOMPOSED operator (the same on every rank).  A_local holds this rank's rows of the decomposed operator
// (halo plan on its space); owned_global_nodes[i] = number, in the undecomposed space, of local owned node i.  From now on the
// V-cycle smooths, restricts and prolongs level 0 on this rank's rows only - ghost entries refreshed before every fine product,
// the restricted right-hand side summed over the ranks - and applies levels >= 1 as they are: the preconditioner of one GPU,
// with the fine-level work divided by the number of ranks.  fs_amg_solve then runs CG on the decomposed operator.
extern "C" int fs_amg_attach_distributed_fine(fs_amg_t M, fs_matrix_t A_local, int64_t n_owned_nodes, const int32_t* owned_global_nodes) {
    FS_REFUSE_DG(A_local, "fs_amg_attach_distributed_fine");
    FS_CHECK(fs_require_init());
    FS_REQUIRE(M && A_local && owned_global_nodes, "fs_amg_attach_distributed_fine: null pointer");
    FS_REQUIRE(M->lv.size() >= 2, "fs_amg_attach_distributed_fine: the hierarchy has a single level");
    amg_level* G = M->lv[0];
    fs_space_s* sp = A_local->space;
    if (M->dist0) {
        // a hierarchy kept over several solves (same operator key): the caller's CURRENT matrix on the same decomposed space takes
        // the place of the one attached first - the level-0 pieces (P rows, diagonal) belong to the hierarchy, not to that matrix
        FS_REQUIRE(sp == M->dist_space && A_local->bs == G->bs && n_owned_nodes == sp->n_nodes_owned,
                   "fs_amg_attach_distributed_fine: a distributed fine level is attached already, on another space");
        M->fine = A_local;
        return FS_OK;
    }
    FS_REQUIRE(A_local->bs == G->bs && n_owned_nodes == sp->n_nodes_owned, "fs_amg_attach_distributed_fine: %lld owned nodes of block size %d do not match the space (%lld, %d)",
               (long long)n_owned_nodes, A_local->bs, (long long)sp->n_nodes_owned, G->bs);
    hipStream_t s = fs_rt().stream;
    const int bs = G->bs, nb = G->P.bc, bb = bs * nb;
    const int64_t nn = n_owned_nodes;
    amg_level* D = new amg_level();
    int rc = FS_OK;
    auto fail = [&](int code) { delete D; return code; };
    D->nn = nn; D->bs = bs; D->n = nn * bs; D->nb = G->nb; D->lmax = G->lmax; D->gersh = G->gersh; D->n_agg = G->n_agg;
    dbuf<int32_t> sel, len;
    if ((rc = sel.alloc(std::max<int64_t>(nn, 1))) != FS_OK || (rc = len.alloc(nn + 1)) != FS_OK) return fail(rc);
    if ((rc = sel.upload(owned_global_nodes, nn, s)) != FS_OK) return fail(rc);
    for (int64_t i = 0; i < nn; ++i)
        if (owned_global_nodes[i] < 0 || owned_global_nodes[i] >= G->nn) {
            fs_set_error("fs_amg_attach_distributed_fine: node %lld names global node %d of %lld", (long long)i, owned_global_nodes[i], (long long)G->nn);
            return fail(FS_ERR_INVALID);
        }
    // this rank's rows of P
    D->P.nrows = nn; D->P.ncols = G->P.ncols; D->P.br = G->P.br; D->P.bc = G->P.bc;
    if ((rc = D->P.rowptr.alloc(nn + 1)) != FS_OK) return fail(rc);
    hipLaunchKernelGGL(k_sel_row_lengths, dim3(fs_grid_for(nn + 1)), dim3(FS_BLOCK), 0, s, nn, sel.p, G->P.rowptr.p, len.p);
    if ((rc = scan_exclusive(len.p, D->P.rowptr.p, nn + 1, s)) != FS_OK) return fail(rc);
    int32_t pn = 0;
    if ((rc = read_i32(D->P.rowptr.p + nn, &pn, s)) != FS_OK) return fail(rc);
    D->P.nnz = pn;
    if ((rc = D->P.col.alloc(std::max<int64_t>(pn, 1))) != FS_OK || (rc = D->P.val.alloc(std::max<int64_t>((int64_t)pn * bb, 1))) != FS_OK) return fail(rc);
    hipLaunchKernelGGL(k_sel_copy_rows, dim3(fs_grid_for(nn * 64, FS_BLOCK, 16384)), dim3(FS_BLOCK), 0, s, nn, sel.p, G->P.rowptr.p, G->P.col.p, G->P.val.p, bb,
                       D->P.rowptr.p, D->P.col.p, D->P.val.p);
    if ((rc = build_p_transpose(D, nn, G->n_agg, bs, nb, s)) != FS_OK) return fail(rc);
    if (G->P.val32.p && (rc = level_transfers_to_f32(D, s)) != FS_OK) return fail(rc);     // the same storage as the replicated level 0
    // diagonal and work vectors of the local rows
    if ((rc = D->dinv.alloc(std::max<int64_t>(D->n, 1))) != FS_OK || (rc = D->r.alloc(std::max<int64_t>(D->n, 1))) != FS_OK ||
        (rc = D->d.alloc(std::max<int64_t>(D->n, 1))) != FS_OK || (rc = D->t.alloc(std::max<int64_t>(D->n, 1))) != FS_OK) return fail(rc);
    hipLaunchKernelGGL(k_sel_gather_dofs, dim3(fs_grid_for(D->n)), dim3(FS_BLOCK), 0, s, nn, sel.p, bs, G->dinv.p, D->dinv.p);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    M->dist0 = D;
    M->dist_space = sp;
    M->fine = A_local;
    // (the CG vectors are sized for the space they multiply with: re-allocated by the next fs_amg_solve)
    M->pr.release(); M->pz.release(); M->pp.release(); M->pw.release();
    return FS_OK;
}

extern "C" int fs_amg_destroy(fs_amg_t M) {
    delete M;
    return FS_OK;
}

extern "C" int fs_amg_info(fs_amg_t M, int* n_levels, double* operator_complexity, double* grid_complexity, double* setup_ms) {
    FS_REQUIRE(M, "fs_amg_info: null handle");
    if (n_levels) *n_levels = (int)M->lv.size();
    if (operator_complexity) *operator_complexity = M->op_complexity;
    if (grid_complexity) *grid_complexity = M->grid_complexity;
    if (setup_ms) *setup_ms = M->setup_ms;
    return FS_OK;
}

extern "C" int fs_amg_level_info(fs_amg_t M, int level, int64_t* n_nodes, int* block_size, int64_t* nnz_blocks,
                                 int64_t* p_nnz_blocks, int* p_block_cols, double* lambda_max) {
    FS_REQUIRE(M && level >= 0 && level < (int)M->lv.size(), "fs_amg_level_info: bad level");
    amg_level* L = M->lv[level];
    if (n_nodes) *n_nodes = L->nn;
    if (block_size) *block_size = L->bs;
    if (nnz_blocks) *nnz_blocks = L->A.nnz;
    if (p_nnz_blocks) *p_nnz_blocks = L->P.nnz;
    if (p_block_cols) *p_block_cols = L->P.bc;
    if (lambda_max) *lambda_max = L->lmax;
    return FS_OK;
}

extern "C" int fs_amg_level_get(fs_amg_t M, int level, int which, int32_t* rowptr, int32_t* col, double* val) {
    FS_REQUIRE(M && level >= 0 && level < (int)M->lv.size(), "fs_amg_level_get: bad level");
    amg_level* L = M->lv[level];
    const bcsr& X = which == 0 ? L->A : L->P;
    hipStream_t s = fs_rt().stream;
    if (which == 2) {
        FS_REQUIRE(val, "fs_amg_level_get: null pointer");
        return L->B.download(val, L->B.n, s);
    }
    if (which == 3) {       // the dense inverse the V-cycle applies on the coarsest level (k_dense_apply); val == NULL only asks for it
        FS_REQUIRE(level == (int)M->lv.size() - 1, "fs_amg_level_get: the dense inverse belongs to the coarsest level %d, not to level %d",
                   (int)M->lv.size() - 1, level);
        if (!M->cinv.p) {
            fs_set_error("fs_amg_level_get: the hierarchy has no dense inverse (%lld rows on its coarsest level %d: Chebyshev sweeps)",
                         (long long)L->n, level);
            return FS_ERR_UNSUPPORTED;
        }
        return val ? M->cinv.download(val, M->nc * M->nc, s) : FS_OK;
    }
    if (which == 4) {       // the aggregate of every node of a level with a prolongator, -1 = in none
        FS_REQUIRE(col, "fs_amg_level_get: null pointer");
        FS_REQUIRE(L->P.nnz > 0 && L->agg.p, "fs_amg_level_get: level %d has no prolongator, hence no aggregates", level);
        return L->agg.download(col, L->nn, s);
    }
    FS_REQUIRE(which == 0 || which == 1, "fs_amg_level_get: which = %d (0 to 4)", which);
    FS_REQUIRE(X.nnz > 0, "fs_amg_level_get: level %d has no such operator", level);
    if (rowptr) FS_CHECK(X.rowptr.download(rowptr, X.nrows + 1, s));
    if (col) FS_CHECK(X.col.download(col, X.nnz, s));
    if (val) FS_CHECK(X.val.download(val, X.nnz * X.br * X.bc, s));
    return FS_OK;
}

// ---- V-cycle ----------------------------------------------------------------------------------------------
static int smooth(fs_amg_s* M, int l, double* x, const double* b, bool zero_guess, hipStream_t s) {
    // distributed fine level: this rank's rows, the ghost entries of x refreshed before every product - the smoother IS the
    // undecomposed one (same operator, same diagonal, same eigenvalue bound)
    const bool dist = l == 0 && M->dist0 != nullptr;
    amg_level* L = dist ? M->dist0 : M->lv[l];
    const double up = 1.1 * L->lmax, lo = 0.1 * L->lmax;
    const double theta = 0.5 * (up + lo), delta = 0.5 * (up - lo), sigma = theta / delta;
    double rho = 1.0 / sigma;
    const int g = fs_grid_for(L->n, FS_BLOCK, 2048);
    const double* r = b;
    const bool fine = l == 0;       // level 0: the product comes from the SELL kernel, b - A x is formed inside the update
    if (!zero_guess) {
        if (fine) {
            if (dist) FS_CHECK(fs_halo_exchange_dev(M->fine->space, x, s));
            FS_CHECK(level_spmv(M, l, x, b, L->t.p, 0, s));
            hipLaunchKernelGGL(k_cheb_first_bt<true>, dim3(g), dim3(FS_BLOCK), 0, s, L->n, L->dinv.p, b, L->t.p, L->d.p, x, 1.0 / theta);
        } else {
            FS_CHECK(level_spmv(M, l, x, b, L->r.p, 1, s));
            r = L->r.p;
            hipLaunchKernelGGL(k_cheb_first<true>, dim3(g), dim3(FS_BLOCK), 0, s, L->n, L->dinv.p, r, L->d.p, x, 1.0 / theta);
        }
    } else {
        hipLaunchKernelGGL(k_cheb_first<false>, dim3(g), dim3(FS_BLOCK), 0, s, L->n, L->dinv.p, r, L->d.p, x, 1.0 / theta);
    }
    for (int k = 1; k < M->smooth_steps; ++k) {
        const double rho_new = 1.0 / (2.0 * sigma - rho);
        if (fine) {
            if (dist) FS_CHECK(fs_halo_exchange_dev(M->fine->space, x, s));
            FS_CHECK(level_spmv(M, l, x, b, L->t.p, 0, s));
            hipLaunchKernelGGL(k_cheb_next_bt, dim3(g), dim3(FS_BLOCK), 0, s, L->n, L->dinv.p, b, L->t.p, L->d.p, x, rho_new * rho, 2.0 * rho_new / delta);
        } else {
            FS_CHECK(level_spmv(M, l, x, b, L->r.p, 1, s));
            hipLaunchKernelGGL(k_cheb_next, dim3(g), dim3(FS_BLOCK), 0, s, L->n, L->dinv.p, L->r.p, L->d.p, x, rho_new * rho, 2.0 * rho_new / delta);
        }
        rho = rho_new;
    }
    return FS_OK;
}

static int vcycle(fs_amg_s* M, int l, double* x, const double* b, hipStream_t s) {
    const bool dist = l == 0 && M->dist0 != nullptr;
    amg_level* L = dist ? M->dist0 : M->lv[l];
    const int last = (int)M->lv.size() - 1;
    if (l == last) {
        if (M->cinv.p && l > 0) {
            hipLaunchKernelGGL(k_dense_apply, dim3(fs_grid_for(L->n, 4, 2048)), dim3(FS_BLOCK), 0, s, L->n, M->cinv.p, b, x);
            return FS_OK;
        }
        FS_CHECK(smooth(M, l, x, b, true, s));
        for (int k = 0; k < (l > 0 ? 4 : 0); ++k) FS_CHECK(smooth(M, l, x, b, false, s));
        return FS_OK;
    }
    amg_level* C = M->lv[l + 1];
    FS_CHECK(smooth(M, l, x, b, true, s));
    if (dist) FS_CHECK(fs_halo_exchange_dev(M->fine->space, x, s));
    FS_CHECK(level_spmv(M, l, x, b, L->r.p, 1, s));
    {
        const int rg = fs_grid_for(C->nn, FS_BLOCK / 64, 16384);
#define FS_RESTRICT_ARGS32 dim3(rg), dim3(FS_BLOCK), 0, s, C->nn, L->pt_ptr.p, L->pt_row.p, L->rt_val32.p, L->r.p, C->b.p
#define FS_RESTRICT_ARGS dim3(rg), dim3(FS_BLOCK), 0, s, C->nn, L->pt_ptr.p, L->pt_row.p, L->rt_val.p, L->r.p, C->b.p
        if (L->rt_val32.p && L->P.br == 3 && L->P.bc == 6) hipLaunchKernelGGL((k_restrict<3, 6, float>), FS_RESTRICT_ARGS32);
        else if (L->rt_val32.p && L->P.br == 6 && L->P.bc == 6) hipLaunchKernelGGL((k_restrict<6, 6, float>), FS_RESTRICT_ARGS32);
        else if (L->P.br == 1 && L->P.bc == 1) hipLaunchKernelGGL((k_restrict<1, 1>), FS_RESTRICT_ARGS);
        else if (L->P.br == 3 && L->P.bc == 3) hipLaunchKernelGGL((k_restrict<3, 3>), FS_RESTRICT_ARGS);
        else if (L->P.br == 3 && L->P.bc == 6) hipLaunchKernelGGL((k_restrict<3, 6>), FS_RESTRICT_ARGS);
        else if (L->P.br == 6 && L->P.bc == 6) hipLaunchKernelGGL((k_restrict<6, 6>), FS_RESTRICT_ARGS);
        else { fs_set_error("AMG: restriction for %dx%d blocks is not built", L->P.br, L->P.bc); return FS_ERR_UNSUPPORTED; }
#undef FS_RESTRICT_ARGS
#undef FS_RESTRICT_ARGS32
    }
    // distributed fine level: every rank restricted its own rows; the coarse right-hand side is their sum, on every rank
    if (dist) FS_CHECK(fs_comm_allreduce_dev(C->b.p, (int)C->n, s));
    FS_CHECK(vcycle(M, l + 1, C->x.p, C->b.p, s));
    if (L->P.val32.p && L->P.br == 3 && L->P.bc == 6)
        hipLaunchKernelGGL((k_prolong_add_grp<3, 6, float>), dim3(fs_grid_for(L->nn * 16, FS_BLOCK, 65536)), dim3(FS_BLOCK), 0, s, L->nn, L->P.rowptr.p, L->P.col.p, L->P.val32.p, C->x.p, x);
    else if (L->P.val32.p && L->P.br == 6 && L->P.bc == 6)
        hipLaunchKernelGGL((k_prolong_add_grp<6, 6, float>), dim3(fs_grid_for(L->nn * 16, FS_BLOCK, 65536)), dim3(FS_BLOCK), 0, s, L->nn, L->P.rowptr.p, L->P.col.p, L->P.val32.p, C->x.p, x);
    else if (L->P.br == 3 && L->P.bc == 6)
        hipLaunchKernelGGL((k_prolong_add_grp<3, 6>), dim3(fs_grid_for(L->nn * 16, FS_BLOCK, 65536)), dim3(FS_BLOCK), 0, s, L->nn, L->P.rowptr.p, L->P.col.p, L->P.val.p, C->x.p, x);
    else if (L->P.br == 6 && L->P.bc == 6)
        hipLaunchKernelGGL((k_prolong_add_grp<6, 6>), dim3(fs_grid_for(L->nn * 16, FS_BLOCK, 65536)), dim3(FS_BLOCK), 0, s, L->nn, L->P.rowptr.p, L->P.col.p, L->P.val.p, C->x.p, x);
    else
        hipLaunchKernelGGL(k_prolong_add, dim3(fs_grid_for(L->n, FS_BLOCK, 8192)), dim3(FS_BLOCK), 0, s, L->n, L->P.br, L->P.bc, L->P.rowptr.p, L->P.col.p, L->P.val.p, C->x.p, x);
    FS_CHECK(smooth(M, l, x, b, false, s));
    return FS_OK;
}

int fs_amg_apply_dev(fs_amg_s* M, const double* r, double* z, hipStream_t s) {
    return vcycle(M, 0, z, r, s);
}

extern "C" int fs_amg_apply(fs_amg_t M, fs_vector_t r, fs_vector_t z) {
    FS_REQUIRE(M && r && z, "fs_amg_apply: null pointer");
    amg_level* L0 = M->dist0 ? M->dist0 : M->lv[0];
    FS_REQUIRE(r->d.n >= L0->n && z->d.n >= M->fine->space->n_dofs_local, "fs_amg_apply: vector too short");
    hipStream_t s = fs_rt().stream;
    FS_CHECK(vcycle(M, 0, z->d.p, r->d.p, s));
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// ---- PCG preconditioned by one V-cycle (PETSc KSPCG + PCGAMG) ------------------------------------------------
int64_t fs_amg_rows(const fs_amg_s* amg) { return amg && !amg->lv.empty() ? (amg->dist0 ? amg->dist0->n : amg->lv[0]->n) : 0; }

extern "C" int fs_amg_solve(fs_amg_t M, fs_vector_t b, fs_vector_t x, const fs_krylov_opts* opts, fs_krylov_stats* stats) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_REQUIRE(M && b && x && opts && stats, "fs_amg_solve: null pointer");
    amg_level* L0 = M->dist0 ? M->dist0 : M->lv[0];
    const int64_t n = L0->n;
    fs_space_s* sp = M->fine->space;
    FS_REQUIRE(b->d.n >= n && x->d.n >= sp->n_dofs_local, "fs_amg_solve: vector too short");
    hipStream_t s = fs_rt().stream;
    if (M->pr.n < n) {
        FS_CHECK(M->pr.alloc(n));
        FS_CHECK(M->pz.alloc(sp->n_dofs_local));
        FS_CHECK(M->pp.alloc(sp->n_dofs_local));
        FS_CHECK(M->pw.alloc(n));
        FS_CHECK(M->pz.zero(s));
        FS_CHECK(M->pp.zero(s));
    }
    memset(stats, 0, sizeof(*stats));
    const auto t0 = std::chrono::steady_clock::now();
    const int g = fs_grid_for(n, FS_BLOCK, 2048);
    // the fine operator of a uniform box has a few dozen distinct (block) rows: its products - four per V-cycle and one per CG
    // iteration - then run from class numbers + class rows instead of streaming 72 B per stored block (fs_krylov.hip, k_dict_spmv3);
    // found from the values, every row verified, dropped when this solve returns
    struct dict_guard { ~dict_guard() { fs_dict_end(); } } dict_scope;
    FS_CHECK(fs_dict_begin(M->fine, s));
    stats->row_classes = 0;
    // Multi-GPU: CG on the distributed operator (halo exchange before each product, dots reduced over the ranks),
    // preconditioned by the rank-local hierarchies (additive Schwarz, no overlap)
    auto dot_host = [&](fs_amg_s* Mm, const double* xx, const double* yy, int64_t nn, double* out, hipStream_t ss) -> int {
        const int gg = fs_grid_for(nn, FS_BLOCK, 1024);
        hipLaunchKernelGGL(k_dot_partial, dim3(gg), dim3(FS_BLOCK), 0, ss, xx, yy, nn, Mm->partials.p);
        hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(FS_SUM_BLOCK), 0, ss, Mm->partials.p, gg, 1, Mm->sums.p);
        FS_KERNEL_CHECK();
        FS_CHECK(fs_comm_allreduce_dev(Mm->sums.p, 1, ss));
        FS_CHECK(Mm->sums.download(out, 1, ss));
        return FS_OK;
    };
    const bool pnorm = opts->norm_type == FS_NORM_PRECONDITIONED;
    double bb = 0.0;
    FS_CHECK(dot_host(M, b->d.p, b->d.p, n, &bb, s));
    stats->bnorm = sqrt(bb);
    if (!opts->nonzero_guess) FS_HIP(hipMemsetAsync(x->d.p, 0, (size_t)n * sizeof(double), s));
    // r = b - A x
    if (opts->nonzero_guess) {
        FS_CHECK(fs_halo_exchange_dev(sp, x->d.p, s));
        FS_CHECK(fs_spmv_dev(M->fine, x->d.p, M->pw.p, s));
        hipLaunchKernelGGL(k_amg_sub, dim3(g), dim3(FS_BLOCK), 0, s, n, b->d.p, M->pw.p, M->pr.p);
    } else {
        FS_HIP(hipMemcpyAsync(M->pr.p, b->d.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    double ref2 = bb;   // reference for the relative test
    if (pnorm) {
        FS_CHECK(vcycle(M, 0, M->pz.p, b->d.p, s));
        FS_CHECK(dot_host(M, M->pz.p, M->pz.p, n, &ref2, s));
    }
    const double thr2 = std::max(opts->rtol * opts->rtol * ref2, opts->atol * opts->atol);
    double rho = 0.0, rho_old = 1.0, res2 = 0.0, tr2 = 0.0;
    int it = 0, conv = 0;
    const int max_iter = opts->max_iter > 0 ? opts->max_iter : 1000;
    // one CG pass from the residual in pr (beta = 0 on its first step); rc != FS_OK on a failed call
    auto cg_pass = [&]() -> int {
        bool first = true;
        for (;; ++it) {
            if (!pnorm) {
                FS_CHECK(dot_host(M, M->pr.p, M->pr.p, n, &res2, s));
                if (!(res2 == res2)) { conv = -1; return FS_OK; }
                if (res2 <= thr2) { conv = 1; return FS_OK; }
                if (it >= max_iter) return FS_OK;
            }
            FS_CHECK(vcycle(M, 0, M->pz.p, M->pr.p, s));
            FS_CHECK(dot_host(M, M->pr.p, M->pz.p, n, &rho, s));
            if (pnorm) {
                FS_CHECK(dot_host(M, M->pz.p, M->pz.p, n, &res2, s));
                if (!(res2 == res2)) { conv = -1; return FS_OK; }
                if (res2 <= thr2) { conv = 1; return FS_OK; }
                if (it >= max_iter) return FS_OK;
            }
            if (!(rho > 0.0)) { conv = -1; return FS_OK; }
            const double beta = first ? 0.0 : rho / rho_old;
            first = false;
            hipLaunchKernelGGL(k_amg_axpby, dim3(g), dim3(FS_BLOCK), 0, s, n, 1.0, M->pz.p, beta, M->pp.p);   // p = z + beta p
            FS_CHECK(fs_halo_exchange_dev(sp, M->pp.p, s));
            FS_CHECK(fs_spmv_dev(M->fine, M->pp.p, M->pw.p, s));
            double pw = 0.0;
            FS_CHECK(dot_host(M, M->pp.p, M->pw.p, n, &pw, s));
            if (!(pw > 0.0)) { conv = -1; return FS_OK; }
            const double alpha = rho / pw;
            hipLaunchKernelGGL(k_amg_axpby, dim3(g), dim3(FS_BLOCK), 0, s, n, alpha, M->pp.p, 1.0, x->d.p);     // x += alpha p
            hipLaunchKernelGGL(k_amg_axpby, dim3(g), dim3(FS_BLOCK), 0, s, n, -alpha, M->pw.p, 1.0, M->pr.p);   // r -= alpha w
            rho_old = rho;
        }
    };
    for (int pass = 0;; ++pass) {
        conv = 0;
        FS_CHECK(cg_pass());
        FS_KERNEL_CHECK();
        // true residual b - A x
        FS_CHECK(fs_halo_exchange_dev(sp, x->d.p, s));
        FS_CHECK(fs_spmv_dev(M->fine, x->d.p, M->pw.p, s));
        hipLaunchKernelGGL(k_amg_sub, dim3(g), dim3(FS_BLOCK), 0, s, n, b->d.p, M->pw.p, M->pw.p);
        FS_CHECK(dot_host(M, M->pw.p, M->pw.p, n, &tr2, s));
        // the recurrence residual drifts from b - A x on ill-conditioned operators (thin cantilevers): continue
        // from the true residual, as the Jacobi-CG path does (fs_krylov.hip)
        if (conv != 1 || pnorm || tr2 <= 4.0 * thr2 || pass >= 2 || it >= max_iter) break;
        FS_HIP(hipMemcpyAsync(M->pr.p, M->pw.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (fs_p2p_reduce_enabled()) FS_CHECK(fs_p2p_check(s));      // a peer-to-peer wait timed out: the numbers below mean nothing
    stats->iterations = it;
    stats->converged = conv;
    stats->row_classes = fs_dict_classes();
    stats->rel_residual = ref2 > 0.0 ? sqrt(res2 / ref2) : 0.0;
    stats->true_rel_residual = bb > 0.0 ? sqrt(tr2 / bb) : 0.0;
    stats->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->spmv_bytes = sp->nnz_nodes * M->fine->bs * M->fine->bs * 12 + n * 20;
    if (conv < 0) {
        fs_set_error("fs_amg_solve: breakdown at iteration %d (rho %g, residual^2 %g)", it, rho, res2);
        return FS_ERR_NUMERIC;
    }
    return FS_OK;
}

void fs_amg_preload() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(k_iota));
    (void)hipGetLastError();
}
