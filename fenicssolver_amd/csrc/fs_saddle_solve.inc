// Part of fs_saddle.hip (included at its end, one translation unit): fs_saddle_solve, the restarted FGMRES of the Taylor-Hood and
// the large-deformation block systems - its kernels, the two block preconditioners (sd_precond: Cahouet-Chabard; sd_precond_ld:
// block_upper) and the host side.  fs_saddle_solve at the end reads top to bottom:
// checks -> ws_acquire -> set_up -> capture_precond_graph -> while (run_cycle) -> fill_stats.
// (DESIGN.md section 3.11 says which function owns the workspace, the graph, the hand-over and the knobs.)

// ---- FGMRES with the block-triangular preconditioner ---------------------------------------------------------
__global__ void k_sd_diag(int64_t n_nodes, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col,
                          const double* __restrict__ val, int64_t plane, double* __restrict__ dinv) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_nodes; r += stride) {
        const int64_t sp0 = slice_ptr[r >> 6];
        const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
        const int64_t base = sp0 + (r & 63);
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            if (sell_col[e] != (int32_t)r) continue;
            for (int i = 0; i < 4; ++i) {
                const double d = val[(int64_t)(i * 4 + i) * plane + e];
                dinv[r * 4 + i] = d != 0.0 ? 1.0 / d : 0.0;     // pressure rows have no diagonal: 0
            }
            break;
        }
    }
}
// zu = (ADD ? zu : 0) + dinv * (r - t) on velocity components; pressure components of zu are set to 0
template <bool FIRST>
__global__ void k_sd_vel_sweep(int64_t n, const double* __restrict__ dinv, const double* __restrict__ r,
                               const double* __restrict__ t, double* __restrict__ z) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if ((i & 3) == 3) { z[i] = 0.0; continue; }
        z[i] = FIRST ? dinv[i] * r[i] : z[i] + dinv[i] * (r[i] - t[i]);
    }
}
// Chebyshev step on the velocity block (Jacobi-scaled): d = c2 d + c1 dinv (r - t), z += d; FIRST: d = c1 dinv r, z = d.
// Pressure components of z and d stay 0.
template <bool FIRST>
__global__ void k_sd_vel_cheb(int64_t n, const double* __restrict__ dinv, const double* __restrict__ r,
                              const double* __restrict__ t, double* __restrict__ d, double* __restrict__ z, double c1, double c2) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if ((i & 3) == 3) { z[i] = 0.0; d[i] = 0.0; continue; }
        const double v = FIRST ? c1 * dinv[i] * r[i] : c2 * d[i] + c1 * dinv[i] * (r[i] - t[i]);
        d[i] = v;
        z[i] = FIRST ? v : z[i] + v;
    }
}
// v <- dinv * t on velocity components, 0 on pressure components (power iteration of D^-1 A)
__global__ void k_sd_vel_scale(int64_t n, const double* __restrict__ dinv, const double* __restrict__ t, double* __restrict__ v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) v[i] = (i & 3) == 3 ? 0.0 : dinv[i] * t[i];
}
__global__ void k_sd_seed(int64_t n, double* __restrict__ v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        uint32_t x = (uint32_t)i * 2654435761U + 12345U;
        x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
        v[i] = (i & 3) == 3 ? 0.0 : (double)(x & 0xffffff) / 8388608.0 - 1.0;
    }
}
// rp[v] = r[4v+3] - (D z_u)[v]: only the continuity rows of the block matrix are needed here, i.e. the three value
// planes (3,0..2) of the vertex-node rows (numbered first) - 2 % of the traffic of a full SpMV.  One thread per row.
__global__ void __launch_bounds__(FS_BLOCK) k_sd_pressure_rows(int64_t nv, const int64_t* __restrict__ slice_ptr,
                                                               const int32_t* __restrict__ sell_col, const double* __restrict__ val,
                                                               int64_t plane, const double* __restrict__ z,
                                                               const double* __restrict__ r, double* __restrict__ rp) {
    // One workgroup per slice of 64 vertex rows, lane = row (every load of a wave is one contiguous 512-byte line of
    // the slice), the entries of the up to 65-block-wide rows dealt round-robin to the four waves, partial sums through
    // LDS: a thread per row walks 65 dependent entries on a third of the chip (75 us at configs[4]), 16 lanes per row read
    // 32 bytes per line (65 us).
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t n_sl = (nv + 63) >> 6;
    for (int64_t s = blockIdx.x; s < n_sl; s += gridDim.x) {
        const int64_t v = s * 64 + lane;
        const int64_t sp0 = slice_ptr[s];
        const int width = (int)((slice_ptr[s + 1] - sp0) >> 6);
        const int64_t base = sp0 + lane;
        double acc = 0.0;
        for (int k = w; k < width; k += 4) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            const int32_t c = sell_col[e];
            if (c < 0) continue;
            const double* zc = z + 4 * (int64_t)c;
            acc += val[12 * plane + e] * zc[0] + val[13 * plane + e] * zc[1] + val[14 * plane + e] * zc[2];
        }
        part[w][lane] = acc;
        __syncthreads();
        if (w == 0 && v < nv) rp[v] = r[4 * v + 3] - ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]));
        __syncthreads();
    }
}
// z[4v+3] = c1*p1[v] + c2*p2[v] for vertices; dummy pressure slots z = r; rows flagged as identity z = r
__global__ void k_sd_scatter_p(int64_t n_nodes, int64_t nv, double c1, const double* __restrict__ p1, double c2,
                               const double* __restrict__ p2, const double* __restrict__ r, const uint8_t* __restrict__ ident,
                               double* __restrict__ z) {
    int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; v < n_nodes; v += stride) {
        double out;
        if (v >= nv || ident[v]) out = r[4 * v + 3];
        else out = (p1 ? c1 * p1[v] : 0.0) + c2 * p2[v];
        z[4 * v + 3] = out;
    }
}
// pressure rows that are identity rows (Dirichlet pressure): the row has a unit (3,3) diagonal entry
__global__ void k_sd_ident_p(int64_t nv, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col,
                             const double* __restrict__ val, int64_t plane, uint8_t* __restrict__ ident) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < nv; r += stride) {
        const int64_t sp0 = slice_ptr[r >> 6];
        const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
        const int64_t base = sp0 + (r & 63);
        uint8_t f = 0;
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            if (sell_col[e] == (int32_t)r) { f = val[15 * plane + e] != 0.0 ? 1 : 0; break; }
        }
        ident[r] = f;
    }
}
__global__ void k_sd_scale_to(int64_t n, double a, const double* __restrict__ x, double* __restrict__ y) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) y[i] = a * x[i];
}
__global__ void k_sd_sub(int64_t n, const double* __restrict__ b, const double* t, double* r) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) r[i] = b[i] - t[i];
}

// Chebyshev step for M x = b with Jacobi: d = c2 d + c1 dinv (b - t), x += d   (FIRST: d = c1 dinv b, x = d)
template <bool FIRST>
__global__ void k_sd_cheb(int64_t n, const double* __restrict__ dinv, const double* __restrict__ b, const double* __restrict__ t,
                          double* __restrict__ d, double* __restrict__ x, double c1, double c2) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double v = FIRST ? c1 * dinv[i] * b[i] : c2 * d[i] + c1 * dinv[i] * (b[i] - t[i]);
        d[i] = v;
        x[i] = FIRST ? v : x[i] + v;
    }
}
// 1/diag of a scalar SELL matrix
__global__ void k_sd_scalar_dinv(int64_t n_rows, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col,
                                 const double* __restrict__ val, double* __restrict__ dinv) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_rows; r += stride) {
        const int64_t sp0 = slice_ptr[r >> 6];
        const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
        const int64_t base = sp0 + (r & 63);
        double d = 1.0;
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            if (sell_col[e] == (int32_t)r) { d = val[e]; break; }
        }
        dinv[r] = d != 0.0 ? 1.0 / d : 1.0;
    }
}
// dots[j] partials of w . V_j for j < nvec (one launch; block b writes partial[j*gridDim + b])
// gate (may be null): the launch is a no-op when *gate == 0 - the second Gram-Schmidt pass is enqueued unconditionally
// and the device decides whether it runs, so the host never waits for the first pass.
// Eight basis vectors per sweep over the rows: eight independent load streams per lane and one block reduction for
// the eight sums (a sweep per vector is latency-bound: 20 rows per thread, then a barrier).
#define SD_DOT_GROUP 8
__global__ void __launch_bounds__(FS_BLOCK) k_sd_multi_dot(int64_t n, const double* __restrict__ w, const double* const* __restrict__ V,
                                                           int nvec, int with_self, double* __restrict__ partial,
                                                           const double* __restrict__ gate) {
    __shared__ double lds[SD_DOT_GROUP][FS_BLOCK / 64];
    if (gate && *gate == 0.0) return;
    const int total = nvec + with_self;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int j0 = 0; j0 < total; j0 += SD_DOT_GROUP) {
        const double* vp[SD_DOT_GROUP];
        double acc[SD_DOT_GROUP];
#pragma unroll
        for (int c = 0; c < SD_DOT_GROUP; ++c) {
            vp[c] = j0 + c < nvec ? V[j0 + c] : w;      // the extra "vector" is w itself: ||w||^2
            acc[c] = 0.0;
        }
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
            const double wi = w[i];
#pragma unroll
            for (int c = 0; c < SD_DOT_GROUP; ++c) acc[c] += wi * vp[c][i];
        }
#pragma unroll
        for (int c = 0; c < SD_DOT_GROUP; ++c) {
            double t = acc[c];
            for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
            if (lane == 0) lds[c][wave] = t;
        }
        __syncthreads();
        if (threadIdx.x < SD_DOT_GROUP && j0 + (int)threadIdx.x < total) {
            double t = 0.0;
            for (int q = 0; q < FS_BLOCK / 64; ++q) t += lds[threadIdx.x][q];
            partial[(int64_t)(j0 + threadIdx.x) * gridDim.x + blockIdx.x] = t;
        }
        __syncthreads();
    }
}
// sums[j] = sum_b partial[j*nblk + b]   (one workgroup per j, fixed order)
__global__ void __launch_bounds__(FS_BLOCK) k_sd_multi_sum(const double* __restrict__ partial, int nblk, double* __restrict__ sums,
                                                           const double* __restrict__ gate) {
    __shared__ double lds4[4];
    if (gate && *gate == 0.0) return;
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) acc += partial[(int64_t)blockIdx.x * nblk + b];
    const double t = fs_block_sum(acc, lds4);
    if (threadIdx.x == 0) sums[blockIdx.x] = t;
}
// w -= sum_j h[j] V_j
__global__ void k_sd_multi_axpy(int64_t n, double* __restrict__ w, const double* const* __restrict__ V, const double* __restrict__ h,
                                int nvec, const double* __restrict__ gate) {
    if (gate && *gate == 0.0) return;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        double acc = w[i];
        for (int j = 0; j < nvec; ++j) acc -= h[j] * V[j][i];
        w[i] = acc;
    }
}

// ---- Arnoldi bookkeeping on the device: the Hessenberg column, the Givens rotations and the residual recurrence are
// advanced by single-thread kernels between the vector kernels, so one FGMRES iteration is a fixed launch sequence with
// no host read in it.  ctl = {need second pass, hh^2, 1/hh, |gamma_{k+1}|, hh, second passes run in this cycle}.
enum { SD_NEED2 = 0, SD_HH2 = 1, SD_SCALE = 2, SD_RES = 3, SD_HH = 4, SD_NPASS2 = 5, SD_CTL = 8 };
// column k of H (stride m) += the projections of this pass; Pythagoras for the new norm; the DGKS criterion: a second pass unless
// more than half of ||w||^2 is left (eta^2 = 0.5).  With eta^2 = 0.1 the ratio hh^2 / ||w||^2 sat between 0.1 and 0.45 in almost every
// iteration, the second pass hardly ever ran and every single pass multiplied the loss of orthogonality by about 3: |V^T V - I| of
// 1e-13 to 8e-10 after 20 iterations (tests/test_gpu_saddle_replay.py, DESIGN.md).
__global__ void k_sd_hess_pass(const double* __restrict__ hdev, int k, int m, double* __restrict__ H, double* __restrict__ ctl, int pass) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (pass > 0 && ctl[SD_NEED2] == 0.0) return;
    double removed = 0.0;
    for (int j = 0; j <= k; ++j) {
        const double h = hdev[j];
        H[(size_t)j * m + k] = (pass > 0 ? H[(size_t)j * m + k] : 0.0) + h;
        removed += h * h;
    }
    const double before = hdev[k + 1];
    const double hh2 = before - removed;
    ctl[SD_HH2] = hh2;
    if (pass == 0) {
        ctl[SD_NEED2] = hh2 > 0.5 * before ? 0.0 : 1.0;
        ctl[SD_NPASS2] += ctl[SD_NEED2];
    }
}
// host_out (mapped, coherent host memory): {|gamma_{k+1}|, hh, serial}; the serial number is written last, after a
// system-scope fence, and the host spins on it - no runtime call is involved in the hand-over
__global__ void k_sd_givens(int k, int m, double* __restrict__ H, double* __restrict__ cs, double* __restrict__ sn,
                            double* __restrict__ gam, double* __restrict__ ctl, volatile double* host_out, double serial) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double hh2 = ctl[SD_HH2];
    const double hh = hh2 > 0.0 ? sqrt(hh2) : 0.0;
    ctl[SD_HH] = hh;
    ctl[SD_SCALE] = hh > 0.0 ? 1.0 / hh : 0.0;
    H[(size_t)(k + 1) * m + k] = hh;
    for (int j = 0; j < k; ++j) {
        const double a = H[(size_t)j * m + k], c = H[(size_t)(j + 1) * m + k];
        H[(size_t)j * m + k] = cs[j] * a + sn[j] * c;
        H[(size_t)(j + 1) * m + k] = -sn[j] * a + cs[j] * c;
    }
    const double a = H[(size_t)k * m + k], c = H[(size_t)(k + 1) * m + k];
    const double d = sqrt(a * a + c * c);
    cs[k] = d > 0.0 ? a / d : 1.0;
    sn[k] = d > 0.0 ? c / d : 0.0;
    H[(size_t)k * m + k] = d;
    H[(size_t)(k + 1) * m + k] = 0.0;
    gam[k + 1] = -sn[k] * gam[k];
    gam[k] = cs[k] * gam[k];
    ctl[SD_RES] = fabs(gam[k + 1]);
    host_out[0] = ctl[SD_RES];
    host_out[1] = hh;
    __threadfence_system();
    host_out[2] = serial;
}
__global__ void k_sd_cycle_init(int m, double res, double* __restrict__ gam, double* __restrict__ ctl) {
    for (int i = threadIdx.x; i <= m; i += blockDim.x) gam[i] = i == 0 ? res : 0.0;
    if (threadIdx.x == 0) ctl[SD_NPASS2] = 0.0;
}
// y = -(H(0:k,0:k))^-1 gamma   (the sign lets k_sd_multi_axpy, which subtracts, add Z y to x)
__global__ void k_sd_backsolve(int k, int m, const double* __restrict__ H, const double* __restrict__ gam, double* __restrict__ y) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = k - 1; i >= 0; --i) {
        double v = -gam[i];
        for (int j = i + 1; j < k; ++j) v -= H[(size_t)i * m + j] * y[j];
        const double d = H[(size_t)i * m + i];
        y[i] = d != 0.0 ? v / d : 0.0;
    }
}
__global__ void k_sd_scale_dev(int64_t n, const double* __restrict__ a, const double* __restrict__ x, double* __restrict__ y) {
    const double f = *a;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) y[i] = f * x[i];
}

// replicated pressure problem: owned entries <-> the global vector by global vertex id
__global__ void k_sd_to_global(int64_t nvo, const int64_t* __restrict__ gid, const double* __restrict__ local, double* __restrict__ global) {
    int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; v < nvo; v += stride) global[gid[v]] = local[v];
}
__global__ void k_sd_from_global(int64_t nvo, const int64_t* __restrict__ gid, const double* __restrict__ global, double* __restrict__ local) {
    int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; v < nvo; v += stride) local[v] = global[gid[v]];
}

// ---- the host side: knobs, workspace, preconditioners, cycle, fs_saddle_solve -------------------------------------------------------
constexpr int SD_DOT_BLOCKS = 512;      // grid of k_sd_multi_dot

// The debugging knobs.  FS_SADDLE_TRACE is read once per process, by the first cycle; the others by every call.
struct saddle_env {
    const bool timing = getenv("FS_SADDLE_TIMING") != nullptr;     // per-iteration host times, with a synchronisation after every part
    const bool sync = getenv("FS_SADDLE_SYNC") != nullptr;         // the synchronisations of `timing` without its report
    const bool graph = getenv("FS_SADDLE_GRAPH") != nullptr;       // the Cahouet-Chabard preconditioner replayed as a captured graph
    const bool debug = getenv("FS_SADDLE_DEBUG") != nullptr;       // one line per solve
    // per-iteration GPU time (events) beside the host's enqueue and wait times, without extra syncs
    static bool trace() { static const bool on = getenv("FS_SADDLE_TRACE") != nullptr; return on; }
};

// Every buffer of the workspace is sized by these: the operator's owned rows, the restart length, the local dofs, the owned
// vertices (pressure buffers) and the pressure space's local dofs.
struct saddle_key {
    int64_t n; int m; int64_t nl, nv, npl;
    bool operator==(const saddle_key& o) const { return n == o.n && m == o.m && nl == o.nl && nv == o.nv && npl == o.npl; }
};

// The device-side Arnoldi state in one allocation: H | cs | sn | gamma | y | ctl
struct arnoldi_state {
    double *H, *cs, *sn, *gamma, *y, *ctl;
    arnoldi_state(double* p, int m) : H(p), cs(H + (size_t)(m + 1) * m), sn(cs + m), gamma(sn + m), y(gamma + m + 1), ctl(y + m) {}
    static int64_t size(int m) { return (int64_t)(m + 1) * m + 4 * (int64_t)m + 1 + SD_CTL; }
};

struct saddle_ws {
    const saddle_key key;
    explicit saddle_ws(const saddle_key& k) : key(k), V(k.m + 1), Z(k.m) {}
    dbuf<double> partials, sums, dinv, t, r, w, mdinv, md, mt, hdev, cd, gin, gout;
    dbuf<double> pg_in, pg_out;      // the replicated (global) pressure right-hand side / correction on several ranks
    double vel_lmax = 0.0;   // largest eigenvalue of D^-1 A on the velocity block (Chebyshev sweeps)
    dbuf<const double*> vptr, zptr;
    dbuf<double> hs;            // arnoldi_state
    double* h_poll = nullptr;   // pinned, mapped, coherent: 2 slots x {|gamma|, hh, serial, -}
    double* d_poll = nullptr;   // the same memory as the device sees it
    double serial = 0.0;
    dbuf<uint8_t> ident;
    fs_vector_s rp, p1, p2;
    fs_vector_s ldt, ldz;       // block_upper: the velocity residual / correction on the vector CG1 space of a0
    dbuf<double> ldy, ldjy;     // block_upper: (0, z_p) and J (0, z_p)
    int64_t ld_nvec = -1;       // block_upper: n_nodes * tdim the velocity buffers were sized for
    int kuse = -1;              // columns used by the last FGMRES cycle (fs_saddle_last_cycle), -1: no cycle yet
    std::vector<dbuf<double>> V, Z;      // m + 1 basis vectors (owned rows), m preconditioned vectors (local rows: inputs of a product)
    ~saddle_ws() { if (h_poll) (void)hipHostFree(h_poll); }
};
// the workspace of fs_saddle_solve (kept between calls: a Newton / time loop solves many systems of one size; read by fs_saddle_last_cycle)
static saddle_ws* g_ws = nullptr;

static int ws_build(saddle_ws& W, hipStream_t s) {
    const saddle_key& k = W.key;
    const int m = k.m;
    FS_CHECK(W.partials.alloc(std::max<int64_t>(FS_MAX_PARTIAL_BLOCKS, (int64_t)(m + 3) * SD_DOT_BLOCKS)));
    FS_CHECK(W.sums.alloc(8));
    FS_CHECK(W.dinv.alloc(k.n));
    FS_CHECK(W.t.alloc(k.n));
    FS_CHECK(W.r.alloc(k.n));
    FS_CHECK(W.w.alloc(k.n));
    FS_CHECK(W.cd.alloc(k.n));
    FS_CHECK(W.gin.alloc(k.n));
    FS_CHECK(W.gout.alloc(k.nl));
    FS_CHECK(W.gout.zero(s));
    FS_CHECK(W.ident.alloc(k.nv));
    FS_CHECK(W.mdinv.alloc(k.nv));
    FS_CHECK(W.md.alloc(k.nv));
    FS_CHECK(W.mt.alloc(k.nv));
    FS_CHECK(W.hdev.alloc(m + 3));
    FS_CHECK(W.vptr.alloc(m + 3));
    FS_CHECK(W.zptr.alloc(m + 3));
    FS_CHECK(W.hs.alloc(arnoldi_state::size(m)));
    FS_HIP(hipHostMalloc((void**)&W.h_poll, 8 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    memset(W.h_poll, 0, 8 * sizeof(double));
    FS_HIP(hipHostGetDevicePointer((void**)&W.d_poll, W.h_poll, 0));
    FS_CHECK(W.rp.d.alloc(k.nv));
    FS_CHECK(W.p1.d.alloc(k.npl));
    FS_CHECK(W.p2.d.alloc(k.npl));
    FS_CHECK(W.p1.d.zero(s));          // ghost entries stay zero: the pressure solves are rank-local blocks
    FS_CHECK(W.p2.d.zero(s));
    for (auto& v : W.V) FS_CHECK(v.alloc(k.n));
    for (auto& z : W.Z) {              // Z_k is the input of an operator product: owned + ghost entries
        FS_CHECK(z.alloc(k.nl));
        FS_CHECK(z.zero(s));
    }
    std::vector<const double*> hp(m + 1);
    for (int j = 0; j <= m; ++j) hp[j] = W.V[j].p;
    FS_HIP(hipMemcpyAsync(W.vptr.p, hp.data(), (size_t)(m + 1) * sizeof(double*), hipMemcpyHostToDevice, s));
    FS_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < m; ++j) hp[j] = W.Z[j].p;
    FS_HIP(hipMemcpyAsync(W.zptr.p, hp.data(), (size_t)m * sizeof(double*), hipMemcpyHostToDevice, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}
// the workspace for `key`: the kept one, or a fresh one after dropping one of another size; a build that fails leaves none behind
static int ws_acquire(const saddle_key& key, hipStream_t s, saddle_ws** out) {
    if (g_ws && !(g_ws->key == key)) { delete g_ws; g_ws = nullptr; }
    if (!g_ws) {
        g_ws = new saddle_ws(key);
        const int rc = ws_build(*g_ws, s);
        if (rc != FS_OK) { delete g_ws; g_ws = nullptr; return rc; }
    }
    g_ws->kuse = -1;
    *out = g_ws;
    return FS_OK;
}
// block_upper: (0, z_p), J (0, z_p) and the velocity residual / correction on the vector CG1 space of a0, sized on first use
static int ws_acquire_block_upper(saddle_ws& W, const fs_space_s* sp, hipStream_t s) {
    const int64_t nvec = sp->n_nodes_owned * sp->mesh->tdim;
    if (W.ldy.n == W.key.n && W.ld_nvec == nvec) return FS_OK;
    W.ld_nvec = -1;
    FS_CHECK(W.ldy.alloc(W.key.n));
    FS_CHECK(W.ldjy.alloc(W.key.n));
    FS_CHECK(W.ldt.d.alloc(nvec));
    FS_CHECK(W.ldz.d.alloc(nvec));
    FS_CHECK(W.ldz.d.zero(s));
    W.ld_nvec = nvec;
    return FS_OK;
}

static int sd_dot(saddle_ws& W, const double* x, const double* y, int64_t n, double* out, hipStream_t s) {
    const int g = fs_grid_for(n, FS_BLOCK, 1024);
    hipLaunchKernelGGL(k_dot_partial, dim3(g), dim3(FS_BLOCK), 0, s, x, y, n, W.partials.p);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(FS_SUM_BLOCK), 0, s, W.partials.p, g, 1, W.sums.p);
    FS_KERNEL_CHECK();
    FS_CHECK(fs_comm_allreduce_dev(W.sums.p, 1, s));      // no-op on one rank
    FS_CHECK(W.sums.download(out, 1, s));
    return FS_OK;
}

// p2 = Mp^-1 rp on nv rows: the Jacobi-scaled P1 mass matrix has its spectrum in [1/2, 5/2] (Wathen 1987), so 5 Chebyshev
// steps reduce the error by 1e-2 with no reduction and no host synchronisation: a fixed linear operator
static int sd_mass_chebyshev(fs_matrix_s* Mp, saddle_ws& W, int64_t nv, hipStream_t s) {
    const int gq = fs_grid_for(nv, FS_BLOCK, 2048);
    const double lo = 0.5, up = 2.5, theta = 0.5 * (up + lo), delta = 0.5 * (up - lo), sigma = theta / delta;
    double rho_c = 1.0 / sigma;
    hipLaunchKernelGGL(k_sd_cheb<true>, dim3(gq), dim3(FS_BLOCK), 0, s, nv, W.mdinv.p, W.rp.d.p, (const double*)nullptr, W.md.p, W.p2.d.p, 1.0 / theta, 0.0);
    for (int k = 1; k < 5; ++k) {
        FS_CHECK(fs_spmv_dev(Mp, W.p2.d.p, W.mt.p, s));
        const double rho_new = 1.0 / (2.0 * sigma - rho_c);
        hipLaunchKernelGGL(k_sd_cheb<false>, dim3(gq), dim3(FS_BLOCK), 0, s, nv, W.mdinv.p, W.rp.d.p, W.mt.p, W.md.p, W.p2.d.p, 2.0 * rho_new / delta, rho_new * rho_c);
        rho_c = rho_new;
    }
    return FS_OK;
}

// z = P^-1 r
static int sd_precond(fs_matrix_s* J, fs_matrix_s* Kp, fs_amg_s* Kp_amg, fs_matrix_s* Mp, const fs_saddle_opts* o, saddle_ws& W,
                      const double* r, double* z, int* inner_its, hipStream_t s) {
    fs_space_s* sp = J->space;
    const int64_t n = sp->n_dofs_owned, nv = sp->mesh->n_owned;      // owned vertices = pressure unknowns of this rank
    const int g = fs_grid_for(n, FS_BLOCK, 4096);
    const int sweeps = o->velocity_sweeps > 0 ? o->velocity_sweeps : 1;
    if (sweeps == 1) {
        hipLaunchKernelGGL(k_sd_vel_sweep<true>, dim3(g), dim3(FS_BLOCK), 0, s, n, W.dinv.p, r, (const double*)nullptr, z);
    } else {
        // plain Jacobi sweeps are not a convergent iteration on P2 blocks (lambda_max(D^-1 A) > 2, an even number of
        // sweeps is even indefinite): Chebyshev polynomial in D^-1 A on [lambda_max/8, 1.1 lambda_max] instead
        const double up = 1.1 * W.vel_lmax, lo = W.vel_lmax / 8.0;
        const double theta = 0.5 * (up + lo), delta = 0.5 * (up - lo), sigma = theta / delta;
        double rho_c = 1.0 / sigma;
        hipLaunchKernelGGL(k_sd_vel_cheb<true>, dim3(g), dim3(FS_BLOCK), 0, s, n, W.dinv.p, r, (const double*)nullptr, W.cd.p, z, 1.0 / theta, 0.0);
        for (int k = 1; k < sweeps; ++k) {
            FS_CHECK(fs_halo_exchange_dev(sp, z, s));
            FS_CHECK(fs_spmv_dev(J, z, W.t.p, s));
            const double rho_new = 1.0 / (2.0 * sigma - rho_c);
            hipLaunchKernelGGL(k_sd_vel_cheb<false>, dim3(g), dim3(FS_BLOCK), 0, s, n, W.dinv.p, r, W.t.p, W.cd.p, z, 2.0 * rho_new / delta, rho_new * rho_c);
            rho_c = rho_new;
        }
    }
    // the continuity rows couple to the velocities of ghost nodes.  Multi-GPU: the two pressure solves below act on
    // this rank's diagonal block (ghost columns see zeros) - a non-overlapping additive Schwarz step with the AMG
    // V-cycle / Chebyshev iteration as subdomain solver, no communication inside
    FS_CHECK(fs_halo_exchange_dev(sp, z, s));
    hipLaunchKernelGGL(k_sd_pressure_rows, dim3((unsigned)std::min<int64_t>((nv + 63) / 64, 65535)), dim3(FS_BLOCK), 0, s, nv, sp->slice_ptr.p, sp->sell_col.p,
                       J->val.p, sp->sell_entries, z, r, W.rp.d.p);
    FS_KERNEL_CHECK();
    fs_krylov_opts ko;
    memset(&ko, 0, sizeof(ko));
    ko.method = FS_KSP_CG;
    ko.precond = FS_PC_JACOBI;
    ko.rtol = o->inner_rtol > 0.0 ? o->inner_rtol : 1e-2;
    ko.max_iter = 500;
    ko.diagonal_scale = 1;
    ko.norm_type = FS_NORM_UNPRECONDITIONED;
    fs_krylov_stats ks;
    const bool transient = o->inv_dt > 0.0 && Kp;
    if (transient) {
        if (Kp_amg && fs_rt().n_ranks == 1) {          // one V-cycle: a fixed linear operator, spectrally equivalent to Kp^-1
            FS_CHECK(fs_amg_apply_dev(Kp_amg, W.rp.d.p, W.p1.d.p, s));
        } else if (Kp_amg && fs_amg_rows(Kp_amg) != nv) {
            // Several GPUs, hierarchy of the GLOBAL pressure Laplacian held by every rank: the pressure space is small
            // (85 184 unknowns at configs[4]), so the Schur-complement solve is replicated - the owned residuals are
            // summed into the global vector (one all-reduce, 0.7 MB), every rank applies the same V-cycle and keeps
            // its own entries.  Same operator, hence same FGMRES iteration counts, as on one GPU; a block-Jacobi
            // K_p^-1 (rank-local hierarchies) loses the smooth pressure modes that dominate at small dt and
            // FGMRES(60) stagnates at 2e-5 with 2 and 4 ranks.
            const int64_t ng = fs_amg_rows(Kp_amg);
            FS_REQUIRE(sp->mesh->gid.p, "fs_saddle_solve: the mesh carries no global vertex ids (fs_mesh_set_global_ids)");
            if (W.pg_in.n != ng) { FS_CHECK(W.pg_in.alloc(ng)); FS_CHECK(W.pg_out.alloc(ng)); }
            FS_CHECK(W.pg_in.zero(s));
            hipLaunchKernelGGL(k_sd_to_global, dim3(fs_grid_for(nv)), dim3(FS_BLOCK), 0, s, nv, sp->mesh->gid.p, W.rp.d.p, W.pg_in.p);
            FS_CHECK(fs_comm_allreduce_dev(W.pg_in.p, (int)ng, s));
            FS_CHECK(fs_amg_apply_dev(Kp_amg, W.pg_in.p, W.pg_out.p, s));
            hipLaunchKernelGGL(k_sd_from_global, dim3(fs_grid_for(nv)), dim3(FS_BLOCK), 0, s, nv, sp->mesh->gid.p, W.pg_out.p, W.p1.d.p);
        } else if (Kp_amg) {
            // several GPUs with a hierarchy of this rank's diagonal block only: K_p^-1 as a global solve - CG on the
            // distributed operator with the local V-cycles as (additive Schwarz) preconditioner, to 1e-2; FGMRES
            // tolerates the varying operator
            fs_krylov_opts ao = ko;
            ao.rtol = o->inner_rtol > 0.0 ? o->inner_rtol : 1e-2;
            ao.max_iter = 60;
            ao.norm_type = FS_NORM_UNPRECONDITIONED;
            const int rc_in = fs_amg_solve(Kp_amg, &W.rp, &W.p1, &ao, &ks);
            if (rc_in != FS_OK && rc_in != FS_ERR_NUMERIC) return rc_in;
            *inner_its += ks.iterations;
        } else {
            FS_CHECK(fs_krylov_solve(Kp, &W.rp, &W.p1, &ko, &ks));
            *inner_its += ks.iterations;
        }
    }
    FS_CHECK(sd_mass_chebyshev(Mp, W, nv, s));
    const double r2 = o->density * o->density;
    hipLaunchKernelGGL(k_sd_scatter_p, dim3(fs_grid_for(sp->n_nodes_owned)), dim3(FS_BLOCK), 0, s, sp->n_nodes_owned, nv,
                       r2 * o->inv_dt, transient ? W.p1.d.p : (const double*)nullptr, r2 * o->kinematic_viscosity, W.p2.d.p, r,
                       W.ident.p, z);
    FS_KERNEL_CHECK();
    FS_CHECK(fs_halo_exchange_dev(sp, z, s));      // ghost pressures for the operator product that follows
    return FS_OK;
}

// ---- block_upper: the large-deformation preconditioner on a CG1 block-4 operator ---------------------------------------------
// rp[v] = r[4v+3]
__global__ void k_ld_take_p(int64_t nv, const double* __restrict__ r, double* __restrict__ rp) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) rp[v] = r[4 * v + 3];
}
// y = (0, 0, 0, z_p) per vertex: z_p = c p[v], or r_p on identity pressure rows
__global__ void k_ld_put_p(int64_t nv, double c, const double* __restrict__ p, const double* __restrict__ r, const uint8_t* __restrict__ ident,
                           double* __restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
        y[4 * v] = 0.0; y[4 * v + 1] = 0.0; y[4 * v + 2] = 0.0; y[4 * v + 3] = ident[v] ? r[4 * v + 3] : c * p[v];
    }
}
// t[v*d + i] = r[4v+i] - jy[4v+i], i < d
__global__ void k_ld_take_v(int64_t nv, int d, const double* __restrict__ r, const double* __restrict__ jy, double* __restrict__ t) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride)
        for (int i = 0; i < d; ++i) t[v * d + i] = r[4 * v + i] - jy[4 * v + i];
}
// z = (zv, [r dummy slot], y_p)
__global__ void k_ld_put_z(int64_t nv, int d, const double* __restrict__ zv, const double* __restrict__ y, const double* __restrict__ r,
                           double* __restrict__ z) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
        for (int i = 0; i < d; ++i) z[4 * v + i] = zv[v * d + i];
        if (d == 2) z[4 * v + 2] = r[4 * v + 2];
        z[4 * v + 3] = y[4 * v + 3];
    }
}
// pressure rows of the reduced operator that are identity rows: a unit (3,3) diagonal and nothing else in block-row 3
__global__ void k_ld_ident_p(int64_t nv, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col,
                             const double* __restrict__ val, int64_t plane, uint8_t* __restrict__ ident) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nv; r += stride) {
        const int64_t sp0 = slice_ptr[r >> 6];
        const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
        const int64_t base = sp0 + (r & 63);
        bool id = true;
        for (int k = 0; k < width && id; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            const int32_t col = sell_col[e];
            if (col < 0) continue;                       // padding
            const bool diag = col == (int32_t)r;
            for (int j = 0; j < 4; ++j)
                if (val[(12 + j) * plane + e] != ((diag && j == 3) ? 1.0 : 0.0)) id = false;
        }
        ident[r] = id ? 1 : 0;
    }
}

// z = [A J_vp; 0 S]^-1 r: z_p = S^-1 r_p, then z_v = A^-1 (r_v - J_vp z_p)
static int sd_precond_ld(fs_matrix_s* J, fs_matrix_s* Mp, const fs_saddle_opts* o, saddle_ws& W, const double* r, double* z, int* inner_its,
                         hipStream_t s) {
    fs_space_s* sp = J->space;
    const int64_t nv = sp->n_nodes_owned;
    const int d = sp->mesh->tdim;
    const int gq = fs_grid_for(nv, FS_BLOCK, 2048);
    hipLaunchKernelGGL(k_ld_take_p, dim3(gq), dim3(FS_BLOCK), 0, s, nv, r, W.rp.d.p);
    FS_CHECK(sd_mass_chebyshev(Mp, W, nv, s));
    hipLaunchKernelGGL(k_ld_put_p, dim3(gq), dim3(FS_BLOCK), 0, s, nv, 1.0 / o->schur_scale, W.p2.d.p, r, W.ident.p, W.ldy.p);
    FS_CHECK(fs_spmv_dev(J, W.ldy.p, W.ldjy.p, s));
    hipLaunchKernelGGL(k_ld_take_v, dim3(gq), dim3(FS_BLOCK), 0, s, nv, d, r, W.ldjy.p, W.ldt.d.p);
    FS_KERNEL_CHECK();
    if (o->a0_amg) {
        FS_CHECK(fs_amg_apply_dev(o->a0_amg, W.ldt.d.p, W.ldz.d.p, s));
    } else {
        fs_krylov_opts ko;
        memset(&ko, 0, sizeof(ko));
        ko.method = FS_KSP_CG;
        ko.precond = FS_PC_JACOBI;
        ko.rtol = o->a0_rtol > 0.0 ? o->a0_rtol : 1e-2;
        ko.max_iter = 500;
        ko.norm_type = FS_NORM_UNPRECONDITIONED;
        fs_krylov_stats ks;
        const int rc = fs_krylov_solve(o->a0, &W.ldt, &W.ldz, &ko, &ks);
        if (rc != FS_OK && rc != FS_ERR_NUMERIC) return rc;
        *inner_its += ks.iterations;
    }
    hipLaunchKernelGGL(k_ld_put_z, dim3(gq), dim3(FS_BLOCK), 0, s, nv, d, W.ldz.d.p, W.ldy.p, r, z);
    FS_KERNEL_CHECK();
    return FS_OK;
}

// ---- one call: what it fixes, what it carries, its pieces -------------------------------------------------------------------------
using sd_clock = std::chrono::steady_clock;
static double sd_ms(sd_clock::time_point a, sd_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// constant after the checks: the handles, the sizes, the knobs
struct saddle_plan {
    fs_matrix_s *J, *Kp;
    fs_amg_s* Kp_amg;
    fs_matrix_s* Mp;
    fs_vector_s *b, *x;
    const fs_saddle_opts* o;
    fs_space_s* sp;
    hipStream_t s;
    bool ld, multi;      // block_upper; several ranks
    int64_t n;           // owned rows
    int m, max_iter, g;  // restart length, iteration limit, grid of the vector kernels
    saddle_env env;
};

// The Cahouet-Chabard preconditioner captured as a graph (FS_SADDLE_GRAPH): ~55 small launches (AMG V-cycle on the pressure
// Laplacian, Chebyshev mass solve), a fixed sequence on fixed buffers once its input / output are staged in gin / gout.  Measured on
// MI355X / ROCm 7.2 (round 1): replay and direct launches both take 0.35 ms - the enqueue costs the host only 0.1 ms, it is not
// launch-bound - so direct launches stay the default.  exec != nullptr: the graph is in use.
struct precond_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    precond_graph() = default;
    precond_graph(const precond_graph&) = delete;
    precond_graph& operator=(const precond_graph&) = delete;
    void drop_graph() { if (graph) (void)hipGraphDestroy(graph); graph = nullptr; }
    ~precond_graph() { if (exec) (void)hipGraphExecDestroy(exec); drop_graph(); }
};

// what a solve carries from cycle to cycle
struct saddle_run {
    int it = 0, conv = 0, inner = 0, j_product_kind = 0;
    double res = 0.0, thr = 0.0;
    double t[4] = {0.0, 0.0, 0.0, 0.0};      // FS_SADDLE_TIMING [ms]: preconditioner enqueued, ... run, product, orthogonalisation
    precond_graph graph;
};

static int check_arguments(fs_matrix_s* J, fs_matrix_s* Kp, fs_matrix_s* Mp, fs_vector_s* b, fs_vector_s* x, const fs_saddle_opts* o,
                           const fs_krylov_stats* stats) {
    FS_REQUIRE(J && Mp && b && x && o && stats, "fs_saddle_solve: null pointer");
    fs_space_s* sp = J->space;
    if (o->block_upper != 0) {
        FS_REQUIRE(J->bs == 4 && sp->degree == 1 && fs_rt().n_ranks == 1 && sp->n_nodes_owned == sp->n_nodes_local,
                   "fs_saddle_solve: block_upper needs the CG1 block-4 operator of fs_assemble_large_deformation on one rank");
        FS_REQUIRE(o->a0 && o->a0->space->mesh == sp->mesh && o->a0->space->ncomp == sp->mesh->tdim &&
                   o->a0->space->degree == 1, "fs_saddle_solve: block_upper needs a0 on the vector CG1 space of the same mesh");
        FS_REQUIRE(o->schur_scale > 0.0 && isfinite(o->schur_scale), "fs_saddle_solve: block_upper needs schur_scale > 0");
        FS_REQUIRE(!o->a0_amg || fs_amg_rows(o->a0_amg) == o->a0->space->n_dofs_owned, "fs_saddle_solve: a0_amg is not a hierarchy of a0");
    } else {
        FS_REQUIRE(J->bs == 4 && sp->degree == 2, "fs_saddle_solve: the operator must be a Taylor-Hood block matrix");
    }
    const int64_t nv = sp->mesh->n_owned;
    FS_REQUIRE(Mp->bs == 1 && Mp->space->n_dofs_owned == nv && (!Kp || (Kp->bs == 1 && Kp->space->n_dofs_owned == nv)),
               "fs_saddle_solve: the pressure operators must live on the CG1 space of the same mesh");
    FS_REQUIRE(b->d.n >= sp->n_dofs_owned && x->d.n >= sp->n_dofs_local, "fs_saddle_solve: vector too short");
    return FS_OK;
}

// what depends on the values of the operators and on b: the two diagonals, the identity pressure rows, vel_lmax, ||b||, the start
static int set_up(const saddle_plan& P, saddle_run& R, saddle_ws& W, fs_krylov_stats* stats) {
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    const int64_t n = P.n, nv = W.key.nv;
    const int g = P.g;
    {
        fs_space_s* q = P.Mp->space;
        hipLaunchKernelGGL(k_sd_scalar_dinv, dim3(fs_grid_for(nv)), dim3(FS_BLOCK), 0, s, nv, q->slice_ptr.p, q->sell_col.p, P.Mp->val.p, W.mdinv.p);
    }
    hipLaunchKernelGGL(k_sd_diag, dim3(fs_grid_for(sp->n_nodes_owned)), dim3(FS_BLOCK), 0, s, sp->n_nodes_owned, sp->slice_ptr.p, sp->sell_col.p, P.J->val.p, sp->sell_entries, W.dinv.p);
    if (P.ld)
        hipLaunchKernelGGL(k_ld_ident_p, dim3(fs_grid_for(nv)), dim3(FS_BLOCK), 0, s, nv, sp->slice_ptr.p, sp->sell_col.p, P.J->val.p, sp->sell_entries, W.ident.p);
    else
        hipLaunchKernelGGL(k_sd_ident_p, dim3(fs_grid_for(nv)), dim3(FS_BLOCK), 0, s, nv, sp->slice_ptr.p, sp->sell_col.p, P.J->val.p, sp->sell_entries, W.ident.p);
    FS_KERNEL_CHECK();
    if (P.o->velocity_sweeps > 1) {
        // lambda_max(D^-1 A) of the velocity block: 12 power iterations from a hashed start
        hipLaunchKernelGGL(k_sd_seed, dim3(g), dim3(FS_BLOCK), 0, s, n, W.w.p);
        double lam = 1.0;
        for (int it = 0; it < 12; ++it) {
            double nn = 0.0;
            FS_CHECK(sd_dot(W, W.w.p, W.w.p, n, &nn, s));
            nn = sqrt(nn);
            if (!(nn > 0.0)) break;
            if (it > 0) lam = nn;
            hipLaunchKernelGGL(k_sd_scale_to, dim3(g), dim3(FS_BLOCK), 0, s, n, 1.0 / nn, W.w.p, W.Z[0].p);
            FS_CHECK(fs_halo_exchange_dev(sp, W.Z[0].p, s));
            FS_CHECK(fs_spmv_dev(P.J, W.Z[0].p, W.t.p, s));
            hipLaunchKernelGGL(k_sd_vel_scale, dim3(g), dim3(FS_BLOCK), 0, s, n, W.dinv.p, W.t.p, W.w.p);
        }
        W.vel_lmax = lam;
    }
    double bb = 0.0;
    FS_CHECK(sd_dot(W, P.b->d.p, P.b->d.p, n, &bb, s));
    stats->bnorm = sqrt(bb);
    if (!P.o->nonzero_guess) FS_HIP(hipMemsetAsync(P.x->d.p, 0, (size_t)sp->n_dofs_local * sizeof(double), s));
    R.thr = std::max(P.o->rtol * stats->bnorm, P.o->atol);
    return FS_OK;
}

// FS_SADDLE_GRAPH: G owns the graph from the capture on; a capture or an instantiation that fails leaves it empty (direct launches)
static int capture_precond_graph(const saddle_plan& P, saddle_ws& W, precond_graph& G) {
    const bool transient_kp = P.o->inv_dt > 0.0 && P.Kp != nullptr;     // an inner CG on Kp (no hierarchy given) cannot be captured
    if (!P.env.graph || (transient_kp && !P.Kp_amg) || P.multi || P.ld) return FS_OK;
    FS_HIP(hipStreamSynchronize(P.s));
    if (hipStreamBeginCapture(P.s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return FS_OK;
    }
    int dummy = 0;
    const int rc_cap = sd_precond(P.J, P.Kp, P.Kp_amg, P.Mp, P.o, W, W.gin.p, W.gout.p, &dummy, P.s);
    const hipError_t e_end = hipStreamEndCapture(P.s, &G.graph);
    if (rc_cap != FS_OK || e_end != hipSuccess || !G.graph ||
        hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0) != hipSuccess) {
        G.drop_graph();
        G.exec = nullptr;      // (a failed instantiation made none)
        (void)hipGetLastError();
    }
    return FS_OK;
}

// FS_SADDLE_TIMING: back-to-back cost of the preconditioner, graph replay vs direct launches, and of the block product
static void time_precond_back_to_back(const saddle_plan& P, saddle_ws& W, const precond_graph& G) {
    hipStream_t s = P.s;
    int dummy = 0;
    (void)hipStreamSynchronize(s);
    auto t0g = sd_clock::now();
    if (G.exec) for (int rep = 0; rep < 20; ++rep) (void)hipGraphLaunch(G.exec, s);
    (void)hipStreamSynchronize(s);
    auto t1g = sd_clock::now();
    for (int rep = 0; rep < 20; ++rep) (void)sd_precond(P.J, P.Kp, P.Kp_amg, P.Mp, P.o, W, W.gin.p, W.gout.p, &dummy, s);
    (void)hipStreamSynchronize(s);
    auto t2g = sd_clock::now();
    for (int rep = 0; rep < 20; ++rep) (void)fs_spmv_dev(P.J, W.gin.p, W.w.p, s);
    (void)hipStreamSynchronize(s);
    auto t3g = sd_clock::now();
    (void)fs_spmv_dev(P.J, W.gin.p, W.w.p, s);
    (void)hipStreamSynchronize(s);
    auto t4g = sd_clock::now();
    fprintf(stderr, "[fs_saddle_solve] block SpMV: %.3f ms each back to back (x20), %.3f ms for a single launch + sync\n",
            sd_ms(t2g, t3g) / 20, sd_ms(t3g, t4g));
    fprintf(stderr, "[fs_saddle_solve] preconditioner x20 back to back: graph %.3f ms each, direct %.3f ms each\n",
            sd_ms(t0g, t1g) / 20, sd_ms(t1g, t2g) / 20);
}

// Z_k = P^-1 V_k: the captured graph, block_upper or Cahouet-Chabard
static int apply_precond(const saddle_plan& P, saddle_run& R, saddle_ws& W, int k) {
    hipStream_t s = P.s;
    if (R.graph.exec) {
        FS_HIP(hipMemcpyAsync(W.gin.p, W.V[k].p, (size_t)P.n * sizeof(double), hipMemcpyDeviceToDevice, s));
        FS_HIP(hipGraphLaunch(R.graph.exec, s));
        FS_HIP(hipMemcpyAsync(W.Z[k].p, W.gout.p, (size_t)P.n * sizeof(double), hipMemcpyDeviceToDevice, s));
    } else if (P.ld) {
        FS_CHECK(sd_precond_ld(P.J, P.Mp, P.o, W, W.V[k].p, W.Z[k].p, &R.inner, s));
    } else {
        FS_CHECK(sd_precond(P.J, P.Kp, P.Kp_amg, P.Mp, P.o, W, W.V[k].p, W.Z[k].p, &R.inner, s));
    }
    return FS_OK;
}

// The hand-over of an iteration's result.  k_sd_givens writes {|gamma_{k+1}|, hh, serial} into one of two slots of mapped host
// memory, the serial number last; the host, which runs one iteration ahead of the GPU, spins on it.  hipEventSynchronize is not
// used: a wait of ~1 ms leaves the runtime's active-wait window and blocks on an interrupt, and that wake-up was measured to take
// 25-65 ms once or twice per solve (MI355X, ROCm 7.2; FS_SADDLE_TRACE).
struct handover {
    saddle_ws& W;
    int slot = 0, pending = -1, pending_k = -1;      // the slot of the next iteration; slot and iteration of the one not yet read
    double expect[2] = {0.0, 0.0};
    // the slot (as the device sees it) for the iteration about to be enqueued; W.serial is its serial number
    double* arm() {
        W.serial += 1.0;
        expect[slot] = W.serial;
        return W.d_poll + 4 * slot;
    }
    void posted(int k) { pending = slot; pending_k = k; slot ^= 1; }
    // waits for the pending iteration: its index, |gamma_{k+1}| and hh
    int harvest(hipStream_t s, int* k, double* rk, double* hk) {
        volatile double* hp = W.h_poll + 4 * pending;
        const auto t_spin = sd_clock::now();
        for (uint64_t spin = 0; hp[2] != expect[pending]; ++spin) {
            __builtin_ia32_pause();
            if ((spin & 0xfffff) == 0xfffff) {          // every ~10 ms: a failed launch or a hung device must not spin for ever
                const hipError_t q = hipStreamQuery(s);
                if (q != hipSuccess && q != hipErrorNotReady) FS_HIP(q);
                if (q == hipSuccess && hp[2] != expect[pending]) { fs_set_error("fs_saddle_solve: the iteration result never arrived"); return FS_ERR_HIP; }
                if (std::chrono::duration<double>(sd_clock::now() - t_spin).count() > 120.0) { fs_set_error("fs_saddle_solve: device timeout"); return FS_ERR_HIP; }
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        *rk = hp[0];
        *hk = hp[1];
        *k = pending_k;
        pending = -1;
        return FS_OK;
    }
};

// host time points of one iteration: before the preconditioner, after its enqueue, after it has run (only the knobs `timing` and
// `sync` wait for it), after the product
struct iter_clock { sd_clock::time_point A, B, C, D; };

// One FGMRES iteration is a fixed launch sequence: the Hessenberg column, the rotations and the residual recurrence live on the
// device.  Preconditioner, product, the two gated Gram-Schmidt passes, Givens (which posts the result), the next basis vector.
static int enqueue_iteration(const saddle_plan& P, saddle_run& R, saddle_ws& W, const arnoldi_state& A, handover& hand, int k, iter_clock& c) {
    hipStream_t s = P.s;
    const int64_t n = P.n;
    const int m = P.m, g = P.g;
    const bool dbg = P.env.timing || P.env.sync;
    c.A = sd_clock::now();
    FS_CHECK(apply_precond(P, R, W, k));
    c.B = c.A;
    if (dbg) { c.B = sd_clock::now(); (void)hipStreamSynchronize(s); }
    c.C = sd_clock::now();
    FS_CHECK(fs_spmv_dev(P.J, W.Z[k].p, W.w.p, s));
    R.j_product_kind = fs_last_product_kind();
    if (dbg) (void)hipStreamSynchronize(s);
    c.D = sd_clock::now();
    // classical Gram-Schmidt with one fused multi-dot launch per pass; the last pointer of the list is w itself,
    // so the pass also returns ||w||^2 before the projection.  The second pass runs unless more than half of ||w||^2
    // is left (DGKS criterion, decided on the device) - in nearly every iteration on these systems: |V^T V - I| stays
    // within 1000 times that of two full passes on the host (tests/test_gpu_saddle_replay.py).
    for (int pass = 0; pass < 2; ++pass) {
        const double* gate = pass ? A.ctl + SD_NEED2 : nullptr;
        hipLaunchKernelGGL(k_sd_multi_dot, dim3(SD_DOT_BLOCKS), dim3(FS_BLOCK), 0, s, n, W.w.p, W.vptr.p, k + 1, 1, W.partials.p, gate);
        hipLaunchKernelGGL(k_sd_multi_sum, dim3(k + 2), dim3(FS_BLOCK), 0, s, W.partials.p, SD_DOT_BLOCKS, W.hdev.p, gate);
        // every rank issues the reduction of both passes: whether the second pass counts is decided on the
        // device, from reduced numbers, hence identically on all ranks
        if (P.multi) FS_CHECK(fs_comm_allreduce_dev(W.hdev.p, k + 2, s));
        hipLaunchKernelGGL(k_sd_hess_pass, dim3(1), dim3(1), 0, s, W.hdev.p, k, m, A.H, A.ctl, pass);
        hipLaunchKernelGGL(k_sd_multi_axpy, dim3(g), dim3(FS_BLOCK), 0, s, n, W.w.p, W.vptr.p, W.hdev.p, k + 1, gate);
    }
    double* const post = hand.arm();
    hipLaunchKernelGGL(k_sd_givens, dim3(1), dim3(1), 0, s, k, m, A.H, A.cs, A.sn, A.gamma, A.ctl, post, W.serial);
    hipLaunchKernelGGL(k_sd_scale_dev, dim3(g), dim3(FS_BLOCK), 0, s, n, A.ctl + SD_SCALE, W.w.p, W.V[k + 1].p);
    FS_KERNEL_CHECK();
    return FS_OK;
}

// FS_SADDLE_TRACE: one event per iteration of a cycle beside the host's enqueue and wait times; the events go on every exit
struct cycle_trace {
    const bool on;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    std::vector<double> t_enq, t_wait;
    cycle_trace(bool on_, int m, hipStream_t s_) : on(on_), s(s_) {
        if (!on) return;
        ev.resize(m + 1);
        for (auto& e : ev) (void)hipEventCreate(&e);
        (void)hipEventRecord(ev[0], s);
    }
    cycle_trace(const cycle_trace&) = delete;
    cycle_trace& operator=(const cycle_trace&) = delete;
    ~cycle_trace() { for (auto& e : ev) (void)hipEventDestroy(e); }
    void enqueued(int k) { if (on) (void)hipEventRecord(ev[k + 1], s); }
    // iteration begun at t_begin, enqueued at t_enqueued, the result of the one before it read by now
    void harvested(sd_clock::time_point t_begin, sd_clock::time_point t_enqueued) {
        if (!on) return;
        t_enq.push_back(sd_ms(t_begin, t_enqueued));
        t_wait.push_back(sd_ms(t_enqueued, sd_clock::now()));
    }
    void report() {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        for (size_t q = 0; q < t_enq.size(); ++q) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[q], ev[q + 1]);
            fprintf(stderr, "[fs_saddle_trace] k=%2zu gpu %.3f ms  host enqueue %.3f ms  host wait %.3f ms\n", q, ms, t_enq[q], t_wait[q]);
        }
    }
};

// One cycle: the true residual and the stopping test on it, up to m iterations, x += Z y.  *more: another cycle is wanted.
static int run_cycle(const saddle_plan& P, saddle_run& R, saddle_ws& W, bool* more) {
    hipStream_t s = P.s;
    const int64_t n = P.n;
    const int m = P.m, g = P.g;
    const arnoldi_state A(W.hs.p, m);
    *more = false;
    // r = b - J x
    FS_CHECK(fs_halo_exchange_dev(P.sp, P.x->d.p, s));
    FS_CHECK(fs_spmv_dev(P.J, P.x->d.p, W.t.p, s));
    hipLaunchKernelGGL(k_sd_sub, dim3(g), dim3(FS_BLOCK), 0, s, n, P.b->d.p, W.t.p, W.r.p);
    double rr = 0.0;
    FS_CHECK(sd_dot(W, W.r.p, W.r.p, n, &rr, s));
    R.res = sqrt(rr);
    if (!(R.res == R.res)) { R.conv = -1; return FS_OK; }
    if (R.res <= R.thr) { R.conv = 1; return FS_OK; }
    if (R.it >= P.max_iter) return FS_OK;
    hipLaunchKernelGGL(k_sd_scale_to, dim3(g), dim3(FS_BLOCK), 0, s, n, 1.0 / R.res, W.r.p, W.V[0].p);
    hipLaunchKernelGGL(k_sd_cycle_init, dim3(1), dim3(64), 0, s, m, R.res, A.gamma, A.ctl);
    // The host runs one iteration ahead of the GPU and reads |gamma| of iteration k-1 after it has enqueued iteration k, so the
    // queue never drains; the price is at most one iteration enqueued beyond convergence, whose column is simply not used in
    // the update.
    int kuse = 0;
    bool stop = false;
    cycle_trace trace(saddle_env::trace(), m, s);
    handover hand{W};
    auto harvest = [&]() -> int {
        int k_read = -1;
        double rk = 0.0, hk = 0.0;
        FS_CHECK(hand.harvest(s, &k_read, &rk, &hk));
        R.res = rk;
        kuse = k_read + 1;
        if (!(rk == rk)) { R.conv = -1; stop = true; }
        else if (rk <= R.thr || !(hk > 0.0)) stop = true;
        return FS_OK;
    };
    for (int k = 0; k < m && R.it + k < P.max_iter && !stop; ++k) {
        iter_clock c;
        FS_CHECK(enqueue_iteration(P, R, W, A, hand, k, c));
        trace.enqueued(k);
        const auto t_enqueued = sd_clock::now();
        if (P.env.timing) {
            (void)hipStreamSynchronize(s);
            R.t[0] += sd_ms(c.A, c.B);
            R.t[1] += sd_ms(c.A, c.C);
            R.t[2] += sd_ms(c.C, c.D);
            R.t[3] += sd_ms(c.D, sd_clock::now());
        }
        if (hand.pending >= 0) FS_CHECK(harvest());
        trace.harvested(c.A, t_enqueued);
        if (!stop) hand.posted(k);
    }
    trace.report();
    if (!stop && hand.pending >= 0) FS_CHECK(harvest());
    R.it += kuse;
    W.kuse = kuse;
    if (R.conv < 0) return FS_OK;
    // y = H^-1 gamma ; x += Z y   (the first kuse columns)
    hipLaunchKernelGGL(k_sd_backsolve, dim3(1), dim3(1), 0, s, kuse, m, A.H, A.gamma, A.y);
    hipLaunchKernelGGL(k_sd_multi_axpy, dim3(g), dim3(FS_BLOCK), 0, s, n, P.x->d.p, W.zptr.p, A.y, kuse, (const double*)nullptr);
    FS_KERNEL_CHECK();
    *more = kuse != 0;
    return FS_OK;
}

static int fill_stats(const saddle_plan& P, const saddle_run& R, sd_clock::time_point t0, fs_krylov_stats* stats) {
    const int it = R.it;
    stats->iterations = it;
    stats->converged = R.conv;
    if (fs_p2p_reduce_enabled()) FS_CHECK(fs_p2p_check(P.s));      // a peer-to-peer wait timed out: the numbers below mean nothing
    stats->row_classes = 0;
    if (P.ld) stats->product_kind = R.j_product_kind;      // the kernel family of the operator products J z
    stats->rel_residual = stats->bnorm > 0.0 ? R.res / stats->bnorm : 0.0;
    stats->true_rel_residual = stats->rel_residual;
    stats->solve_ms = sd_ms(t0, sd_clock::now());
    stats->spmv_bytes = P.sp->nnz_nodes * 16 * 12 + P.n * 20;
    if (P.env.debug) fprintf(stderr, "[fs_saddle_solve] %d outer iterations, %d inner CG iterations, %.1f ms%s\n", it, R.inner, stats->solve_ms, R.graph.exec ? " (preconditioner as hipGraph)" : "");
    if (P.env.timing) fprintf(stderr, "[fs_saddle_solve] per iteration [ms]: precond enqueue %.3f, precond done %.3f, spmv %.3f, orthogonalisation %.3f\n", R.t[0] / std::max(it, 1), R.t[1] / std::max(it, 1), R.t[2] / std::max(it, 1), R.t[3] / std::max(it, 1));
    if (R.conv < 0) {
        fs_set_error("fs_saddle_solve: breakdown at iteration %d", it);
        return FS_ERR_NUMERIC;
    }
    return FS_OK;
}

extern "C" int fs_saddle_solve(fs_matrix_t J, fs_matrix_t Kp, fs_amg_t Kp_amg, fs_matrix_t Mp, fs_vector_t b, fs_vector_t x,
                               const fs_saddle_opts* o, fs_krylov_stats* stats) {
    FS_REFUSE_DG(J, "fs_saddle_solve"); FS_REFUSE_DG(Kp, "fs_saddle_solve"); FS_REFUSE_DG(Mp, "fs_saddle_solve");
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_CHECK(check_arguments(J, Kp, Mp, b, x, o, stats));
    fs_space_s* sp = J->space;
    const int64_t n = sp->n_dofs_owned;
    const saddle_plan P{J, Kp, Kp_amg, Mp, b, x, o, sp, fs_rt().stream, o->block_upper != 0, fs_rt().n_ranks > 1, n,
                        o->restart > 0 ? o->restart : 60, o->max_iter > 0 ? o->max_iter : 600, fs_grid_for(n, FS_BLOCK, 4096), {}};
    memset(stats, 0, sizeof(*stats));
    const auto t0 = sd_clock::now();
    saddle_ws* ws = nullptr;
    FS_CHECK(ws_acquire({n, P.m, sp->n_dofs_local, sp->mesh->n_owned, Mp->space->n_dofs_local}, P.s, &ws));
    if (P.ld) FS_CHECK(ws_acquire_block_upper(*ws, sp, P.s));
    saddle_run R;
    FS_CHECK(set_up(P, R, *ws, stats));
    FS_CHECK(capture_precond_graph(P, *ws, R.graph));
    if (P.env.timing && !P.ld) time_precond_back_to_back(P, *ws, R.graph);
    for (bool more = true; more;) FS_CHECK(run_cycle(P, R, *ws, &more));
    return fill_stats(P, R, t0, stats);
}

extern "C" int fs_saddle_last_cycle(fs_saddle_cycle_info* info, double* V, double* Z, double* H, double* cs, double* sn, double* gamma,
                                    double* y) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(info, "fs_saddle_last_cycle: null pointer");
    if (!g_ws || g_ws->kuse < 0) {
        fs_set_error("fs_saddle_last_cycle: no FGMRES cycle has run on the workspace");
        return FS_ERR_UNSUPPORTED;
    }
    saddle_ws& W = *g_ws;
    hipStream_t s = fs_rt().stream;
    const int m = W.key.m, kuse = W.kuse;
    const int64_t n = W.key.n;
    const arnoldi_state A(W.hs.p, m);
    auto get = [&](double* out, const double* src, size_t count) -> int {
        if (out && count) FS_HIP(hipMemcpyAsync(out, src, count * sizeof(double), hipMemcpyDeviceToHost, s));
        return FS_OK;
    };
    double ctl[SD_CTL];
    FS_CHECK(get(ctl, A.ctl, SD_CTL));
    for (int k = 0; k <= kuse; ++k) FS_CHECK(get(V ? V + (size_t)k * n : nullptr, W.V[k].p, (size_t)n));
    for (int k = 0; k < kuse; ++k) FS_CHECK(get(Z ? Z + (size_t)k * n : nullptr, W.Z[k].p, (size_t)n));
    FS_CHECK(get(H, A.H, (size_t)(m + 1) * m));
    FS_CHECK(get(cs, A.cs, (size_t)m));
    FS_CHECK(get(sn, A.sn, (size_t)m));
    FS_CHECK(get(gamma, A.gamma, (size_t)m + 1));
    FS_CHECK(get(y, A.y, (size_t)m));
    FS_HIP(hipStreamSynchronize(s));
    info->restart = m;
    info->columns_used = kuse;
    info->second_passes = (int)ctl[SD_NPASS2];
    info->n_owned = n;
    info->vel_lmax = W.vel_lmax;
    return FS_OK;
}

