// Part of fs_krylov.hip (included there, one translation unit: the kernels share its file-scope state): the Krylov iterations' device side: CG / BiCGStab / pipelined CG update kernels, the one-launch iteration k_dict_cg_iter, the peer-to-peer exchange kernel.
// Split out in round 6 (VERDICT r5: a 5 000-line source); nothing here is compiled on its own.

// ---- CG scalar state on the device ---------------------------------------------------------
// sums[0..2] = gamma=r.z, delta=w.z, rho=r.r of the current iteration (globally reduced)
// ctrl[0] = threshold on rho (max(rtol^2 b.b, atol^2)), ctrl[1] = b.b, ctrl[2] = max_iter (read by the update kernels of a
// captured batch, so that one instantiated graph serves solves with different iteration limits)
// scal[2][2] = (gamma, alpha) of the previous iteration, double-buffered by iteration parity
// status[0] = 0 running / 1 converged / 2 breakdown / 3 max_iter, status[1] = iterations
__global__ void k_set_threshold(const double* __restrict__ bb, double rtol, double atol, double* __restrict__ ctrl) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double t = rtol * rtol * bb[0];
        ctrl[0] = fmax(t, atol * atol);
        ctrl[1] = bb[0];
    }
}
__global__ void k_set_iteration_limit(double* __restrict__ ctrl, int max_iter) {
    if (threadIdx.x == 0 && blockIdx.x == 0) ctrl[2] = (double)max_iter;
}

// FUSED: every workgroup first sums the SpMV's per-WG partials itself (same fixed order as
// k_sum_partials, so all workgroups obtain bit-identical gamma/delta/rho) - saves one launch per
// iteration on a single GPU; with a communicator the sums come from the all-reduced `sums`.
// alpha, beta of the single-reduction recurrences from the reduced sums and the previous iteration's (gamma, alpha).  ONE definition
// for every kernel that needs them - the update kernels, the peer-to-peer exchange kernel that advances the ghost rows of r and
// s on its own, the pipelined recurrence: the ghost copies stay bit-identical to the owner's rows only if all of them apply the
// same bits (ADVICE r3).  false: not SPD / NaN.
__device__ __forceinline__ bool cg_scalars_from(int iter, double gamma, double delta, double rho, double gamma_old, double alpha_old,
                                                 double& alpha, double& beta) {
    beta = 0.0;
    if (iter == 0) {
        alpha = gamma / delta;
    } else {
        beta = gamma / gamma_old;
        alpha = gamma / (delta - beta * gamma / alpha_old);
    }
    return (alpha > 0.0) && (alpha < 1e300) && (rho == rho);
}
__device__ __forceinline__ bool cg_scalars(int iter, double gamma, double delta, double rho, const double* __restrict__ scal,
                                            double& alpha, double& beta) {
    double gamma_old = 0.0, alpha_old = 0.0;
    if (iter != 0) {
        gamma_old = scal[2 * ((iter - 1) & 1) + 0];
        alpha_old = scal[2 * ((iter - 1) & 1) + 1];
    }
    return cg_scalars_from(iter, gamma, delta, rho, gamma_old, alpha_old, alpha, beta);
}

template <bool FUSED>
__global__ void __launch_bounds__(FS_BLOCK) k_cg_update(int64_t n, int iter, int check_only,
                                                        const double* __restrict__ partials, int npart,
                                                        const double* __restrict__ sums,
                                                        const double* __restrict__ ctrl, double* __restrict__ scal,
                                                        int* __restrict__ status, double* __restrict__ hist,
                                                        const double* __restrict__ dinv, double* z,
                                                        const double* __restrict__ w, double* __restrict__ p,
                                                        double* __restrict__ sv, double* __restrict__ x,
                                                        double* __restrict__ r) {
    if (status[0] != 0) return;
    double gamma, delta, rho;
    if (FUSED) {
        __shared__ double lds4[4];
        __shared__ double sh[3];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int i = threadIdx.x; i < npart; i += FS_BLOCK) {
            a0 += partials[i];
            a1 += partials[npart + i];
            a2 += partials[2 * npart + i];
        }
        const double t0 = fs_block_sum(a0, lds4);
        const double t1 = fs_block_sum(a1, lds4);
        const double t2 = fs_block_sum(a2, lds4);
        if (threadIdx.x == 0) { sh[0] = t0; sh[1] = t1; sh[2] = t2; }
        __syncthreads();
        gamma = sh[0]; delta = sh[1]; rho = sh[2];
    } else {
        gamma = sums[0]; delta = sums[1]; rho = sums[2];
    }
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    if (leader) hist[iter] = rho;
    if (rho <= ctrl[0]) {  // every workgroup takes the same branch: inputs are identical
        if (leader) { status[1] = iter; status[0] = 1; }
        return;
    }
    if (check_only) {
        if (leader) { status[1] = iter; status[0] = 3; }
        return;
    }
    double beta, alpha;
    if (!cg_scalars(iter, gamma, delta, rho, scal, alpha, beta)) {  // not SPD / NaN
        if (leader) { status[1] = iter; status[0] = 2; }
        return;
    }
    if (leader) {
        scal[2 * (iter & 1) + 0] = gamma;
        scal[2 * (iter & 1) + 1] = alpha;
    }
    // 16-B vectorised body; n even part as double2, tail scalar
    const int64_t n2 = n >> 1;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double2* z2 = reinterpret_cast<double2*>(z);  // read and written in place: no restrict
    const double2* __restrict__ w2 = reinterpret_cast<const double2*>(w);
    const double2* __restrict__ d2 = reinterpret_cast<const double2*>(dinv);
    double2* __restrict__ p2 = reinterpret_cast<double2*>(p);
    double2* __restrict__ s2 = reinterpret_cast<double2*>(sv);
    double2* __restrict__ x2 = reinterpret_cast<double2*>(x);
    double2* __restrict__ r2 = reinterpret_cast<double2*>(r);
    for (; i < n2; i += stride) {
        const double2 zz = z2[i], ww = w2[i], dd = d2[i];
        double2 pp = p2[i], ss = s2[i], xx = x2[i], rr = r2[i];
        pp.x = zz.x + beta * pp.x;  pp.y = zz.y + beta * pp.y;
        ss.x = ww.x + beta * ss.x;  ss.y = ww.y + beta * ss.y;
        xx.x += alpha * pp.x;       xx.y += alpha * pp.y;
        rr.x -= alpha * ss.x;       rr.y -= alpha * ss.y;
        p2[i] = pp; s2[i] = ss; x2[i] = xx; r2[i] = rr;
        double2 zn; zn.x = dd.x * rr.x; zn.y = dd.y * rr.y;
        z2[i] = zn;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t t = n - 1;
        const double pp = z[t] + beta * p[t];
        const double ss = w[t] + beta * sv[t];
        p[t] = pp; sv[t] = ss;
        x[t] += alpha * pp;
        const double rr = r[t] - alpha * ss;
        r[t] = rr;
        z[t] = dinv[t] * rr;
    }
}

// ---- BiCGStab (non-symmetric operators: advection, ScalarTransportSolver.py:305-311) --------------
// Right-preconditioned (Jacobi) BiCGStab, PETSc KSPBCGS.  Per iteration: two fused SpMV+dots launches and
// three fused vector kernels; rho/alpha/omega, the threshold and the status word live on the device,
// exactly as for CG.  bscal = {rho[parity 0], rho[parity 1], alpha, omega}.
template <int NS>
__device__ __forceinline__ void wg_sum_partials(const double* __restrict__ partials, int npart, double (&out)[NS]) {
    __shared__ double lds4[4];
    __shared__ double sh[NS];
    double a[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) a[j] = 0.0;
    // four trips at a time, their 4 NS loads in flight together (the plain loop waits for every trip's loads before the next
    // trip's go out: four dependent round trips for 1024 partials, and the partials were written by the previous launch on other
    // XCDs - about 0.7 us each); a thread's partials are still added in ascending index: same bits
    for (int i0 = threadIdx.x; i0 < npart; i0 += 4 * FS_BLOCK) {
        double v[4][NS];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = i0 + t * FS_BLOCK;
#pragma unroll
            for (int j = 0; j < NS; ++j) v[t][j] = partials[(int64_t)j * npart + (i < npart ? i : npart - 1)];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (i0 + t * FS_BLOCK < npart) {
#pragma unroll
                for (int j = 0; j < NS; ++j) a[j] += v[t][j];
            }
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double t = fs_block_sum(a[j], lds4);
        if (threadIdx.x == 0) sh[j] = t;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NS; ++j) out[j] = sh[j];
}

static __global__ void __launch_bounds__(FS_BLOCK) k_dot2_partial(const double* __restrict__ a, const double* __restrict__ b,
                                                                  const double* __restrict__ c, const double* __restrict__ d,
                                                                  int64_t n, double* __restrict__ partial) {
    __shared__ double lds4[4];
    double s0 = 0.0, s1 = 0.0;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        s0 += a[i] * b[i];
        s1 += c[i] * d[i];
    }
    const double t0 = fs_block_sum(s0, lds4);
    const double t1 = fs_block_sum(s1, lds4);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = t0;
        partial[gridDim.x + blockIdx.x] = t1;
    }
}

// K1: (rho_new = rhat.r, rr = r.r) -> convergence test, beta, p = r + beta (p - omega v), y = D^-1 p
template <bool FUSED>
__global__ void __launch_bounds__(FS_BLOCK) k_bicg_p(int64_t n, int iter, int check_only,
                                                     const double* __restrict__ partials, int npart,
                                                     const double* __restrict__ sums, const double* __restrict__ ctrl,
                                                     double* __restrict__ bscal, int* __restrict__ status,
                                                     double* __restrict__ hist, const double* __restrict__ dinv,
                                                     const double* __restrict__ r, double* __restrict__ p,
                                                     const double* __restrict__ v, double* __restrict__ y) {
    if (status[0] != 0) return;
    double sm[2];
    if (FUSED) wg_sum_partials<2>(partials, npart, sm);
    else { sm[0] = sums[0]; sm[1] = sums[1]; }
    const double rho_new = sm[0], rr = sm[1];
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    if (leader) hist[iter] = rr;
    if (rr <= ctrl[0]) {
        if (leader) { status[1] = iter; status[0] = 1; }
        return;
    }
    if (check_only) {
        if (leader) { status[1] = iter; status[0] = 3; }
        return;
    }
    double beta = 0.0, omega = 0.0;
    if (iter > 0) {
        const double rho_old = bscal[(iter - 1) & 1];
        const double alpha = bscal[2];
        omega = bscal[3];
        beta = (rho_new / rho_old) * (alpha / omega);
    }
    if (!(rho_new == rho_new) || rho_new == 0.0 || !(beta == beta) || !(fabs(beta) < 1e300)) {
        if (leader) { status[1] = iter; status[0] = 2; }
        return;
    }
    if (leader) bscal[iter & 1] = rho_new;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double pn = iter == 0 ? r[i] : r[i] + beta * (p[i] - omega * v[i]);
        p[i] = pn;
        y[i] = dinv[i] * pn;
    }
}

// K3: alpha = rho / (rhat.v); s = r - alpha v; z = D^-1 s
template <bool FUSED>
__global__ void __launch_bounds__(FS_BLOCK) k_bicg_s(int64_t n, int iter, const double* __restrict__ partials,
                                                     int npart, const double* __restrict__ sums,
                                                     double* __restrict__ bscal, int* __restrict__ status,
                                                     const double* __restrict__ dinv, const double* __restrict__ r,
                                                     const double* __restrict__ v, double* __restrict__ sv,
                                                     double* __restrict__ z) {
    if (status[0] != 0) return;
    double sm[1];
    if (FUSED) wg_sum_partials<1>(partials, npart, sm);
    else sm[0] = sums[0];
    const double rv = sm[0];
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    const double alpha = bscal[iter & 1] / rv;
    if (rv == 0.0 || !(alpha == alpha) || !(fabs(alpha) < 1e300)) {
        if (leader) { status[1] = iter; status[0] = 2; }
        return;
    }
    if (leader) bscal[2] = alpha;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double si = r[i] - alpha * v[i];
        sv[i] = si;
        z[i] = dinv[i] * si;
    }
}

// K5: omega = (t.s)/(t.t); x += alpha y + omega z; r = s - omega t; partial dots (rhat.r, r.r)
template <bool FUSED>
__global__ void __launch_bounds__(FS_BLOCK) k_bicg_x(int64_t n, int iter, const double* __restrict__ partials,
                                                     int npart, const double* __restrict__ sums,
                                                     double* __restrict__ bscal, int* __restrict__ status,
                                                     double* __restrict__ x, const double* __restrict__ y,
                                                     const double* __restrict__ z, double* __restrict__ r,
                                                     const double* __restrict__ sv, const double* __restrict__ t,
                                                     const double* __restrict__ rhat, double* __restrict__ pout) {
    if (status[0] != 0) return;
    double sm[2];
    if (FUSED) wg_sum_partials<2>(partials, npart, sm);
    else { sm[0] = sums[0]; sm[1] = sums[1]; }
    const double ts = sm[0], tt = sm[1];
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    const double omega = tt > 0.0 ? ts / tt : 0.0;   // t = 0 only when s = 0: x + alpha y is already exact
    const double alpha = bscal[2];
    if (!(omega == omega)) {
        if (leader) { status[1] = iter; status[0] = 2; }
        return;
    }
    if (leader) bscal[3] = omega;
    __shared__ double lds4b[4];
    double d0 = 0.0, d1 = 0.0;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        x[i] += alpha * y[i] + omega * z[i];
        const double ri = sv[i] - omega * t[i];
        r[i] = ri;
        d0 += rhat[i] * ri;
        d1 += ri * ri;
    }
    const double t0 = fs_block_sum(d0, lds4b);
    const double t1 = fs_block_sum(d1, lds4b);
    if (threadIdx.x == 0) {
        pout[blockIdx.x] = t0;
        pout[gridDim.x + blockIdx.x] = t1;
    }
}

// ---- CG on the symmetrically scaled system  D^-1/2 A D^-1/2 (PETSc KSPSetDiagonalScale) ------------
// Jacobi-PCG on A is unpreconditioned CG on the scaled operator, for which z == r: the update kernel
// drops the z and D^-1 streams (72 instead of 96 B/DOF per iteration).  rho stays the UNSCALED ||r||^2
// (sum d r^2, computed in the SpMV), so the stopping test is unchanged.
template <bool FUSED, bool NT = false>
__global__ void __launch_bounds__(FS_BLOCK) k_cg_update_scaled(int64_t n, int iter, int check_only,
                                                               const double* __restrict__ partials, int npart,
                                                               const double* __restrict__ sums,
                                                               const double* __restrict__ ctrl,
                                                               double* __restrict__ scal, int* __restrict__ status,
                                                               double* __restrict__ hist, double* __restrict__ r,
                                                               const double* __restrict__ w, double* __restrict__ p,
                                                               double* __restrict__ sv, double* __restrict__ x, int* __restrict__ mirror = nullptr, int r_plain = 0) {
    // mirror (one GPU; may be null): the pinned progress words of k_dict_cg_iter - [0] status once stopped, [1] iteration in progress
    // (the status word is looked at AFTER the first trip's loads have gone out - everything a launch reads first was written by the
    // previous launch on other XCDs, and each dependent load is a round trip of about a microsecond)
    const int st0 = status[0];
    const int st2 = status[2];
    const double it_max = ctrl[2], thresh = ctrl[0];
    const double sc_g0 = scal[0], sc_a0 = scal[1], sc_g1 = scal[2], sc_a1 = scal[3];      // (gamma, alpha) of the two iteration parities
    // NT (vectors larger than the caches, 10 M DOF): non-temporal loads and stores - the probe in tools/probes streams
    // 7.2 instead of 6.4 TB/s that way
    typedef double v2d __attribute__((ext_vector_type(2)));
    struct io {
        static __device__ __forceinline__ double2 ld(const double2* q) {
            if (NT) { const v2d t = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(q)); return make_double2(t.x, t.y); }
            return *q;
        }
        static __device__ __forceinline__ void st(double2* q, const double2& v) {
            if (NT) { v2d t; t.x = v.x; t.y = v.y; __builtin_nontemporal_store(t, reinterpret_cast<v2d*>(q)); }
            else *q = v;
        }
    };
    const int64_t n2 = n >> 1;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const double2* __restrict__ w2 = reinterpret_cast<const double2*>(w);
    double2* __restrict__ p2 = reinterpret_cast<double2*>(p);
    double2* __restrict__ s2 = reinterpret_cast<double2*>(sv);
    double2* __restrict__ x2 = reinterpret_cast<double2*>(x);
    double2* __restrict__ r2 = reinterpret_cast<double2*>(r);
    // the operands of the first trip are requested BEFORE the sums are reduced (at 1 M rows a thread makes two trips and the
    // kernel is latency-bound: the reduction of 3 x 1024 partials and the ten loads of the trip used to be two round trips in a row)
    const bool first_trip = i + stride < n2;
    double2 wa0 = {0.0, 0.0}, wb0 = wa0, pa0 = wa0, sa0 = wa0, xa0 = wa0, ra0 = wa0, pb0 = wa0, sb0 = wa0, xb0 = wa0, rb0 = wa0;
    if (first_trip) {
        const int64_t j = i + stride;
        wa0 = io::ld(&w2[i]); wb0 = io::ld(&w2[j]);
        pa0 = io::ld(&p2[i]); sa0 = io::ld(&s2[i]); xa0 = io::ld(&x2[i]); ra0 = io::ld(&r2[i]);
        pb0 = io::ld(&p2[j]); sb0 = io::ld(&s2[j]); xb0 = io::ld(&x2[j]); rb0 = io::ld(&r2[j]);
    }
    if (st0 != 0) return;
    if (iter < 0) {                 // captured batch: the index of the product that preceded this launch
        iter = st2 - 1;
        check_only = iter >= (int)it_max ? 1 : 0;
    }
    double gamma, delta, rho;
    if (FUSED) {
        double sm[3];
        wg_sum_partials<3>(partials, npart, sm);
        gamma = sm[0]; delta = sm[1]; rho = sm[2];
    } else {
        gamma = sums[0]; delta = sums[1]; rho = sums[2];
    }
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    if (leader) hist[iter] = rho;
    auto stop = [&](int code) {
        if (leader) {
            status[1] = iter; status[0] = code;
            if (mirror) { fs_host_store(mirror + 1, iter); fs_host_store(mirror, code); }
        }
    };
    if (rho <= thresh) { stop(1); return; }
    if (check_only) { stop(3); return; }
    double beta, alpha;
    if (!cg_scalars_from(iter, gamma, delta, rho, ((iter - 1) & 1) ? sc_g1 : sc_g0, ((iter - 1) & 1) ? sc_a1 : sc_a0, alpha, beta)) { stop(2); return; }
    if (leader) {
        scal[2 * (iter & 1) + 0] = gamma;
        scal[2 * (iter & 1) + 1] = alpha;
        if (mirror) fs_host_store(mirror + 1, iter + 1);
    }
    // two strided elements per trip: ten 16-B loads in flight per lane (the kernel is latency-bound at 1 M DOF)
    bool prefetched = first_trip;
    for (; i + stride < n2; i += 2 * stride) {
        const int64_t j = i + stride;
        double2 wa, wb, pa, sa, xa, ra, pb, sb, xb, rb;
        if (prefetched) {
            wa = wa0; wb = wb0; pa = pa0; sa = sa0; xa = xa0; ra = ra0; pb = pb0; sb = sb0; xb = xb0; rb = rb0;
            prefetched = false;
        } else {
            wa = io::ld(&w2[i]); wb = io::ld(&w2[j]);
            pa = io::ld(&p2[i]); sa = io::ld(&s2[i]); xa = io::ld(&x2[i]); ra = io::ld(&r2[i]);
            pb = io::ld(&p2[j]); sb = io::ld(&s2[j]); xb = io::ld(&x2[j]); rb = io::ld(&r2[j]);
        }
        pa.x = ra.x + beta * pa.x;  pa.y = ra.y + beta * pa.y;
        pb.x = rb.x + beta * pb.x;  pb.y = rb.y + beta * pb.y;
        sa.x = wa.x + beta * sa.x;  sa.y = wa.y + beta * sa.y;
        sb.x = wb.x + beta * sb.x;  sb.y = wb.y + beta * sb.y;
        xa.x += alpha * pa.x;       xa.y += alpha * pa.y;
        xb.x += alpha * pb.x;       xb.y += alpha * pb.y;
        ra.x -= alpha * sa.x;       ra.y -= alpha * sa.y;
        rb.x -= alpha * sb.x;       rb.y -= alpha * sb.y;
        // (r_plain, bits: ordinary stores for r / p / s / x where the kernel otherwise streams its stores past the caches; g_upd_r_plain)
        if (r_plain & 2) { p2[i] = pa; p2[j] = pb; } else { io::st(&p2[i], pa); io::st(&p2[j], pb); }
        if (r_plain & 4) { s2[i] = sa; s2[j] = sb; } else { io::st(&s2[i], sa); io::st(&s2[j], sb); }
        if (r_plain & 8) { x2[i] = xa; x2[j] = xb; } else { io::st(&x2[i], xa); io::st(&x2[j], xb); }
        if (r_plain & 1) { r2[i] = ra; r2[j] = rb; } else { io::st(&r2[i], ra); io::st(&r2[j], rb); }
    }
    for (; i < n2; i += stride) {
        const double2 ww = w2[i];
        double2 pp = p2[i], ss = s2[i], xx = x2[i], rr = r2[i];
        pp.x = rr.x + beta * pp.x;  pp.y = rr.y + beta * pp.y;
        ss.x = ww.x + beta * ss.x;  ss.y = ww.y + beta * ss.y;
        xx.x += alpha * pp.x;       xx.y += alpha * pp.y;
        rr.x -= alpha * ss.x;       rr.y -= alpha * ss.y;
        p2[i] = pp; s2[i] = ss; x2[i] = xx; r2[i] = rr;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t t = n - 1;
        const double pp = r[t] + beta * p[t];
        const double ss = w[t] + beta * sv[t];
        p[t] = pp; sv[t] = ss;
        x[t] += alpha * pp;
        r[t] -= alpha * ss;
    }
}

// ---- ONE launch per CG iteration (row-dictionary operators, one GPU) ------------------------------------------------------------
// Launch k does the update of iteration k AND the product of iteration k + 1:
//      s_k = w_k + beta_k s_{k-1};   r_{k+1} = r_k - alpha_k s_k;   p_k = r_k + beta_k p_{k-1};   x_{k+1} = x_k + alpha_k p_k
//      w_{k+1} = A r_{k+1}   with the three sums (r.r, w.r, sum d r^2) of the new pair
// The product needs r_{k+1} on the NEIGHBOUR rows, which other workgroups own: instead of waiting for them (a device-wide barrier
// costs 8 us on the 8 XCDs of gfx950, DESIGN history) every lane recomputes r_{k+1}[j] = r_k[j] - alpha (w_k[j] + beta s_{k-1}[j])
// for the columns its runs touch - the same two fmas the owner applies, hence the same bits - from the OLD r, w, s, which are
// read-only during the launch: r, w, s are double-buffered by iteration parity, p and x are row-local and stay in place.  alpha_k,
// beta_k come from the dot partials launch k - 1 left (summed by every workgroup, as k_cg_update_scaled does).
// Per row: reads r, w, s (neighbour values from L1 / L2), p, x, d, the 2-byte class; writes r, w, s, p, x = 90 B instead of the
// 98 B and two launches of k_dict_spmv + k_cg_update_scaled; 3 x 3.5 vector loads per row for the runs instead of 3.5.
// The iteration number travels on the device (it_ctr[par] read by everybody, it_ctr[par ^ 1] = iter + 1 written by one lane) so
// that a captured batch replays with constant arguments; par = parity of the launch = which buffers are `old`.
// Whole dictionary in LDS only (P1 boxes: the operators whose iteration is launch-bound).
// Measured on MI355X (tools/probes/fused_iter_probe.py, hipGraph batches): 1 M rows: 27.4 us per iteration against 29.9 us for
// the two launches, iterates BIT-IDENTICAL (the same fmas on the same operands, the same partial-sum geometry); 10 M rows: 285 us
// against 187 us - with ONE neighbour vector instead of three (timing ablation, wrong numerics) still 220 us: the row-local
// streams (5 loads, 5 stores per row) reach 4.1 TB/s inside an item-by-item kernel against the 6.5 TB/s of the grid-stride update
// kernel, and three vectors x three mesh planes no longer fit the 4 MB L2 of an XCD.  Hence automatic only where the vectors
// stay in the Infinity Cache (FS_CG_FUSED_MAX_ROWS, default 3 M rows).
#ifdef FS_ITER_TIMING
// (stamp 8 sits between 2 and 3: the prefetch is issued and the status word looked at, the sums are not yet begun)
#define FS_STAMPS 16
__device__ long long g_iter_dbg[FS_STAMPS * 4096];
#define FS_STAMP(k) do { if (threadIdx.x == 0 && it_ctr[par] == 100) g_iter_dbg[FS_STAMPS * blockIdx.x + (k)] = wall_clock64(); } while (0)
#else
#define FS_STAMP(k) do { } while (0)
#endif
// -DFS_ITER_ABLATE_PXD (probe builds only, wrong numerics): the kernel without the loads and stores of p, x and the dot weights - what
// the launch costs without the 40 B per row that do nothing for the recurrence (tools/probes/fused_iter_probe.py with FS_PROBE_LIB;
// profiles/r07_cg_pair_ablation.txt: 18.8 against 21.7 us per launch at 1 M rows)
// -DFS_ITER_ABLATE_RUNS (probe builds only; wrong numerics wherever those runs carry a coefficient): EVERY CENTRE launch drops the runs of
// slots 1 and 7 as ZRUNS does - 2 of the 7 runs a Kuhn-box row multiplies, 29 % of the run loads and of the recomputed-residual fma
// pairs.  Timing ablation of profiles/r10_cg_lines_ablation.txt (tools/probes/fused_iter_probe.py with FS_PROBE_LIB).
#ifdef FS_ITER_ABLATE_RUNS
#define FS_ABLATE_RUNS true
#else
#define FS_ABLATE_RUNS false
#endif
// COMM: a decomposed space - the three sums come reduced over the ranks from `sums` (k_cg_p2p_exchange<true> before this launch put
// them there, stored the neighbours' w into the ghost rows of w_in and advanced the ghost rows of r_out / s_out); the neighbour
// columns of an item may then be ghost columns: n_cols counts them.
// MODE: p and x feed nothing but each other, so their two row-local steps need not run in every launch (option "cg_pair"):
//   FS_ITER_EVERY  p_k = r_k + beta_k p_{k-1}, x_{k+1} = x_k + alpha_k p_k in launch k (90 B per row)
//   FS_ITER_LIGHT  even launches: p and x are not touched (50 B per row); the step of iteration k stays owed
//   FS_ITER_PAIR   odd launches: the owed step of iteration k - 1, then the step of iteration k, in one pass over p and x (90 B per
//                  row).  r_{k-1} is still there: launch k writes r_{k+1} into the buffer that holds it, every lane reads its own rows
//                  of it before it overwrites them, and nobody else reads that buffer during the launch.  alpha_{k-1} is in scal[2 q + 1],
//                  beta_{k-1} in scal[4 + q] (q = (k - 1) & 1), left there by the leader lane of launch k - 1: the bits cg_scalars_from
//                  produced.  The same four fmas on the same operands as two launches of FS_ITER_EVERY: the same bits.
//   A solve that stops in an odd launch still owes x one step: k_cg_pair_flush, enqueued by the host behind the last launch.
// Measured at 1 M rows (kernel trace of the step workload, profiles/r07_cg_pair_trace_*.csv): LIGHT 16.6 us, PAIR 20.8 us, the flush 6.5 us
// once per solve, against 20.2 us per launch of FS_ITER_EVERY; 6.53 -> 6.13 ms per step.  One GPU only: behind the exchange kernel
// (COMM) the LIGHT instantiation needs 132 VGPRs - three waves per SIMD - and COMM stays on FS_ITER_EVERY.
// DTAB: `dvec` is the table of dot weights by row class (row_dict::dtab, every row verified against it bit for bit), copied into LDS behind
// the dictionary, instead of the 8 B per row of the weight vector.
// GUARD (option "cg_guard", one GPU, LIGHT / PAIR launches): r, w, s of both parities have G doubles of zeros in front of row 0 and behind
// row n + 1 (dbuf::alloc_guarded; G covers the smallest and largest run start of the space + the 128 values of an item), so every run
// load of every item is inside the block: H.edge is ignored, no item takes the run-by-run clamped path (eight dependent round trips
// where an ordinary item has two exposed ones), the first item's half round is always asked for before the prologue, n_cols is unused.
// The same bits: a column outside the vector has a zero coefficient - the clamped path adds fma(+0, finite, acc), this one
// fma(+0, 0, acc) (the recomputed residual of a band column is fma(-alpha, fma(beta, 0, 0), 0) = 0), in the same run order.
// CENTRE (with GUARD, where the space has ONE plan of one round whose slot 4 is the run (-1; 3 offsets): the Kuhn box, fs_space_s::dict_centre):
// that run brings x[r - 1 .. r + 2], the lane's own two rows among them, so the z run of slot 0 - whose coefficients are all zero - is
// neither loaded nor multiplied (21 instead of 24 sixteen-byte run loads per item, 42 instead of 48 coefficient reads and fma pairs): the
// new s, the old r and the new r of the own rows are (value.y, next lane's value.x) of slot 4, the same memory words through the same two
// fmas.  Lane 63 has no rows of its own and loads what lane 62 needs.
// Measured at 1 M rows: profiles/r08_cg_guard_ab.txt, r08_cg_guard_trace_*.csv, r08_iter_edge_timeline.txt (DESIGN.md section 3).
// ZRUNS (with CENTRE and DTAB, option "cg_zero_runs"; the host takes it where NO class row of the solve's dictionary holds a coefficient
// above 2^-53 at any position of slots 1 and 7 - row_dict::nz_slots, found from the class table itself): the runs (-(a + b + 1); 2) and
// (a + b; 2) are neither loaded nor multiplied - 15 instead of 21 run loads per item, 30 instead of 42 coefficient reads and fma pairs.
// They are the (0, 1, 1) and (1, 1, 1) diagonals of the Kuhn split, whose P1 stiffness entries vanish on a box with orthogonal edges:
// the pure diffusion operator is the 7-point stencil, and what the assembly leaves there is the rounding of sums that cancel (1.9e-17
// at most on the unit cube, against a unit diagonal).  The two runs are each other's transposes: the operator stays symmetric.  NOT the
// same bits: a row's product loses terms below half an ulp of its diagonal term; iterates equal the seven-run form's to rounding, the
// true residual at the end of a pass is taken with the whole operator.  A mass or reaction term fills those entries and the host keeps
// the seven runs.
// PROLOGUE (every form): the dictionary and the DTAB table go into LDS by direct-to-LDS loads issued first (fs_fill_lds_issue); every wave
// waits for its own with a counted s_waitcnt in front of the ONE barrier of the sums, which publishes them, and in front of the early
// return.  With GUARD nothing between kernel entry and that barrier waits for the first item's run loads: the sums are reduced under
// their flight.  Measured: profiles/r09_iter_prologue_timeline.txt, r09_cg_prologue_ab.txt, r09_cg_prologue_trace_*.csv.
enum { FS_ITER_EVERY = 0, FS_ITER_LIGHT = 1, FS_ITER_PAIR = 2 };
// a 16-byte pair of doubles at base + st doubles + boff bytes (8-byte aligned), through an ordinary pointer or a global-address-space one
typedef const __attribute__((address_space(1))) double* fs_gcd;
typedef double fs_v2du __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ fs_v2du fs_ld_pair(const double* base, int32_t st, uint32_t boff) {
    return *reinterpret_cast<const fs_v2du*>(reinterpret_cast<const char*>(base + st) + boff);
}
__device__ __forceinline__ fs_v2du fs_ld_pair(fs_gcd base, int32_t st, uint32_t boff) {
    return *(const __attribute__((address_space(1))) fs_v2du*)((const __attribute__((address_space(1))) char*)(base + st) + boff);
}
template <int RL, bool COMM, int MODE = FS_ITER_EVERY, bool DTAB = false, bool GUARD = false, bool CENTRE = false, bool ZRUNS = false>
__global__ void __launch_bounds__(FS_BLOCK) k_dict_cg_iter(int64_t n_cols, int64_t n_items, const int4* __restrict__ items,
                                                           const dict_plan_round* __restrict__ plans, const uint16_t* __restrict__ cls,
                                                           const double* __restrict__ dict, int S, int C,
                                                           const double* __restrict__ r_in, const double* __restrict__ w_in,
                                                           const double* __restrict__ s_in, double* __restrict__ r_out,
                                                           double* __restrict__ w_out, double* __restrict__ s_out,
                                                           double* __restrict__ pv, double* __restrict__ xv, const double* __restrict__ dvec,
                                                           const double* __restrict__ part_in, double* __restrict__ part_out, int npart,
                                                           const double* __restrict__ ctrl, double* __restrict__ scal, int* __restrict__ status,
                                                           int* __restrict__ it_ctr, int par, double* __restrict__ hist, int map_xcd,
                                                           const double* __restrict__ sums, int* __restrict__ mirror) {
    // mirror (may be null): two words of PINNED HOST memory - [0] the status word once the recurrence has stopped, [1] the number of
    // the iteration this launch is working on - written by one lane with relaxed system-scope stores (no fence: nothing is ordered
    // against them).  The host enqueues the next launches from what it reads there (fs_krylov_solve) instead of copying the status
    // word back behind every batch, and stops within a few launches of the end instead of a batch and a half after it.
    static_assert(!ZRUNS || (CENTRE && DTAB && RL == 3), "ZRUNS: the Kuhn box with the class table of dot weights");
    // (run j of half round h is dropped: slots 1 and 7)
    constexpr bool DROP17 = ZRUNS || (FS_ABLATE_RUNS && CENTRE);
    auto dropped = [](int h, int j) { return DROP17 && ((h == 0 && j == 1) || (h == 1 && j == 3)); };
    FS_STAMP(0);
    // The launch is latency-bound at the sizes it is used for (a wave has two work items at 1 M rows), and what it reads first was
    // written by the previous launch on other XCDs - every dependent load is a round trip to the Infinity Cache (1 - 2 us).  So
    // everything the prologue needs goes out BEFORE anything is waited for: the dictionary (direct-to-LDS loads: no registers, and
    // nothing it needs depends on anything else), status word, iteration number, threshold, both parities of the previous
    // (gamma, alpha), the twelve dot partials of this thread, the first item's header -> row-local operands, run starts -> first
    // nine or twelve run loads.  (Timeline of the first version, tools/probes: 8.8 of 22.7 us were the prologue.)
    // The dictionary used to go LAST, through registers, behind a wait for everything before it: a second round trip on the way to
    // alpha and beta.  And with GUARD the first item's loads are branch-free (a wave without a first item loads the operands of item
    // 0 - inside the guarded block like every item's - and discards them), so that the wait in front of the sums is a COUNT that
    // leaves the run loads in flight: reduction, barrier and the two divisions run under them.
    extern __shared__ __attribute__((aligned(16))) double sdict[];
    fs_fill_lds_issue(sdict, dict, C * S);
    double* const sdtab = sdict + C * S;         // (DTAB: C dot weights behind the C class rows, by the same road - as an early register
    if (DTAB) fs_fill_lds_issue<4>(sdtab, dvec, C);     // load the compiler sinks them behind the run loads, in front of a wait for everything)
    const int st0 = status[0];
    const int iter = it_ctr[par];
    const double thresh = ctrl[0], it_max = ctrl[2];
    const double sc_g0 = scal[0], sc_a0 = scal[1], sc_g1 = scal[2], sc_a1 = scal[3];
    double sc_b0 = 0.0, sc_b1 = 0.0;
    if (MODE == FS_ITER_PAIR) { sc_b0 = scal[4]; sc_b1 = scal[5]; }
    // (the loads of the prologue go through copies of their pointers the compiler knows nothing about: what it loads through a
    // read-only `restrict` argument it is free to sink behind the early return and the barrier of the sums - behind the status
    // word's round trip, or behind alpha and beta)
    fs_gcd part_pre = (fs_gcd)part_in, r_pre = (fs_gcd)r_in, w_pre = (fs_gcd)w_in, s_pre = (fs_gcd)s_in;
    asm volatile("" : "+s"(part_pre), "+s"(r_pre), "+s"(w_pre), "+s"(s_pre));
    double pl[3][4];
    double sum_g = 0.0, sum_d = 0.0, sum_r = 0.0;
    if (COMM) { sum_g = sums[0]; sum_d = sums[1]; sum_r = sums[2]; }
    else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = threadIdx.x + t * FS_BLOCK;
#pragma unroll
            for (int j = 0; j < 3; ++j) pl[j][t] = part_pre[(int64_t)j * npart + (i < npart ? i : npart - 1)];      // (no branch: twelve loads in flight)
        }
    }
    FS_STAMP(1);
    typedef double v2d __attribute__((ext_vector_type(2)));
    typedef double v2du __attribute__((ext_vector_type(2), aligned(8)));
    __shared__ double lds34[3][4], lds34e[3][4];      // (the sums of the prologue; this launch's own partials at the end)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t n_chunks = (n_items + 3) / 4;
    const int32_t cmax = (int32_t)(n_cols - 1);
    chunk_iter it = xcd_chunks(n_chunks);
    if (!map_xcd) { it.cur = blockIdx.x; it.step = gridDim.x; it.end = n_chunks; }
    struct item_hdr { int32_t first; int nr, edge, rounds; const dict_plan_round* pl; };
    auto decode = [&](int64_t q) {
        const int4 ds = items[__builtin_amdgcn_readfirstlane((int)q)];
        item_hdr H;
        H.first = __builtin_amdgcn_readfirstlane(ds.x);
        H.nr = __builtin_amdgcn_readfirstlane(ds.y) & 0xffff;
        H.edge = __builtin_amdgcn_readfirstlane(ds.y) >> 16;
        H.pl = plans + __builtin_amdgcn_readfirstlane(ds.z);
        H.rounds = __builtin_amdgcn_readfirstlane(ds.w);
        return H;
    };
    // loads of runs [4 h, 4 h + 4) of round rd: scalar base (vector + run start) + one 32-bit byte offset per lane - the `saddr` form
    // of the load, no 64-bit address arithmetic or address registers per load (rows < 2^29)
    // (skip0: slot 0 of the half round is not loaded - the z run of a CENTRE launch; pre: the first item's loads in the prologue)
    auto load_half = [&](const item_hdr& H, int rd, int h, uint32_t boff, v2d (&A)[4], v2d (&Wb)[4], v2d (&Sb)[4], bool skip0 = false, bool pre = false) {
        // (measured and not kept: run starts that need no load - kernel arguments for the plan most items have, or a per-item copy beside
        // the header - and the next item's header asked for an item ahead: with nothing left between header and run loads the
        // compiler schedules 164 - 177 VGPRs (and spills SGPRs into them), two or three waves per SIMD instead of four, and the
        // launch gets slower: 22.9 against 19.0 us at 1 M rows)
        int32_t sts[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sts[j] = __builtin_amdgcn_readfirstlane(H.pl[rd].start[4 * h + j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((skip0 && j == 0) || dropped(h, j)) { A[j] = Wb[j] = Sb[j] = v2d{0.0, 0.0}; continue; }
            const int32_t st = sts[j];
            if (pre) { A[j] = fs_ld_pair(r_pre, st, boff); Wb[j] = fs_ld_pair(w_pre, st, boff); Sb[j] = fs_ld_pair(s_pre, st, boff); }
            else { A[j] = fs_ld_pair(r_in, st, boff); Wb[j] = fs_ld_pair(w_in, st, boff); Sb[j] = fs_ld_pair(s_in, st, boff); }
        }
    };
    // (rp: the own rows of r_{k-1}, PAIR only)
    auto load_own = [&](const item_hdr& H, v2d& pp, v2d& xx, v2d& dd, v2d& rp) {
        const int32_t r = H.first + 2 * lane;
        pp = xx = dd = rp = v2d{0.0, 0.0};
#ifdef FS_ITER_ABLATE_PXD
        dd = v2d{1.0, 1.0};
        return;
#endif
        if (2 * lane + 1 < H.nr) {
            if (MODE != FS_ITER_LIGHT) {
                pp = *reinterpret_cast<const v2du*>(&pv[r]);
                xx = *reinterpret_cast<const v2du*>(&xv[r]);
            }
            if (MODE == FS_ITER_PAIR) rp = *reinterpret_cast<const v2du*>(&r_out[r]);
            if (!DTAB) dd = *reinterpret_cast<const v2du*>(&dvec[r]);
        } else if (2 * lane < H.nr) {
            if (MODE != FS_ITER_LIGHT) { pp.x = pv[r]; xx.x = xv[r]; }
            if (MODE == FS_ITER_PAIR) rp.x = r_out[r];
            if (!DTAB) dd.x = dvec[r];
        }
    };
    // the same for the first item in the GUARD prologue: row by row under the lanes' masks - no two arms that write the same registers
    // (the second arm waits for the first one's loads, and with them for everything asked for before) and no branch on `have`
    auto load_own_pre = [&](const item_hdr& H, bool have, v2d& pp, v2d& xx, v2d& dd, v2d& rp) {
        const int32_t r = H.first + 2 * lane;
        pp = xx = dd = rp = v2d{0.0, 0.0};
#ifdef FS_ITER_ABLATE_PXD
        dd = v2d{1.0, 1.0};
        return;
#endif
        if (have && 2 * lane < H.nr) {
            if (MODE != FS_ITER_LIGHT) { pp.x = pv[r]; xx.x = xv[r]; }
            if (MODE == FS_ITER_PAIR) rp.x = r_out[r];
            if (!DTAB) dd.x = dvec[r];
        }
        if (have && 2 * lane + 1 < H.nr) {
            if (MODE != FS_ITER_LIGHT) { pp.y = pv[r + 1]; xx.y = xv[r + 1]; }
            if (MODE == FS_ITER_PAIR) rp.y = r_out[r + 1];
            if (!DTAB) dd.y = dvec[r + 1];
        }
    };
    // Nothing the first item LOADS depends on alpha, beta: its first twelve run loads and its row-local operands are asked for
    // before the partial sums are reduced (a wave has about two items at 1 M rows; 35.3 -> 27.4 us per iteration with 1024 workgroups)
    item_hdr H0 = {};
    v2d PA[4], PW[4], PS[4], Ppp = {0.0, 0.0}, Pxx = {0.0, 0.0}, Pdd = {0.0, 0.0}, Prp = {0.0, 0.0};
    const bool have0 = it.cur < it.end && it.cur * 4 + wave < n_items;
    // (the vector loads the wave has certainly issued behind the dictionary's and the partials' when it comes to the sums: the run loads)
    constexpr int RUN_LOADS0 = GUARD ? 3 * ((CENTRE ? 3 : 4) - (DROP17 ? 1 : 0)) : 0;
    if (GUARD) {
        H0 = decode(have0 ? it.cur * 4 + wave : 0);
        load_own_pre(H0, have0, Ppp, Pxx, Pdd, Prp);        // (in front of the run loads: those are the LAST loads of every wave)
        load_half(H0, 0, 0, (uint32_t)(H0.first + 2 * lane) * 8u, PA, PW, PS, CENTRE, true);
    } else if (have0) {
        H0 = decode(it.cur * 4 + wave);
        if (!H0.edge) load_half(H0, 0, 0, (uint32_t)(H0.first + 2 * lane) * 8u, PA, PW, PS, CENTRE, true);
        load_own(H0, Ppp, Pxx, Pdd, Prp);
    }
    asm volatile("" ::: "memory");
    FS_STAMP(2);
    if (st0 != 0) {                             // (the no-op launches behind a converged solve: no wave leaves with a load into LDS in flight)
        fs_fill_lds_wait<0>();
        return;
    }
    FS_STAMP(8);
    // (a wait the compiler SEES, in front of the first use of the partials: it takes a direct-to-LDS load for one that may come back
    // out of order, and every wait it inserts itself while it believes one in flight is vmcnt(0).  gfx9 encoding: vmcnt in bits 3:0
    // (+ 15:14), expcnt 6:4 and lgkmcnt 11:8 left at their maxima)
    // (... and the sums may not be begun in front of it: the partials pass through an empty statement behind it)
    if (GUARD && !COMM) {
        __builtin_amdgcn_s_waitcnt(0x0f70 | RUN_LOADS0);
        asm volatile("s_nop 0");                // (the compiler merges a wait with what the NEXT instruction needs - by its book everything)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int j = 0; j < 3; ++j) asm volatile("" : "+v"(pl[j][t]));
        }
    }
    // the three sums of the previous launch's partials, in the order of wg_sum_partials / fs_block_sum (same bits as the update
    // kernel of the two-launch iteration computes), with ONE barrier: a thread's partials in ascending index, the wave's by the
    // shuffle tree, the four waves as (0 + 1) + (2 + 3) by every thread.  The same barrier publishes the dictionary: every wave
    // waits for its own direct-to-LDS loads in front of it (they went out first: at most the run loads are still outstanding).
    double sm[3];
    if (COMM) {
        sm[0] = sum_g; sm[1] = sum_d; sm[2] = sum_r;
        fs_fill_lds_wait<0>();
        __syncthreads();                        // (the dictionary is in LDS)
    } else {                                    // (npart <= 4 x 256: the host launches this kernel with at most 1024 workgroups)
        double a[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if ((int)threadIdx.x + t * FS_BLOCK < npart) {
#pragma unroll
                for (int j = 0; j < 3; ++j) a[j] += pl[j][t];
            }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a[j] += __shfl_down(a[j], off, 64);
            if (lane == 0) lds34[j][wave] = a[j];
        }
        fs_fill_lds_wait<RUN_LOADS0>();
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; ++j) sm[j] = (lds34[j][0] + lds34[j][1]) + (lds34[j][2] + lds34[j][3]);
    }
    FS_STAMP(3);
    const double gamma = sm[0], delta = sm[1], rho = sm[2];
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    if (leader) hist[iter] = rho;
    auto stop = [&](int code) {
        if (leader) {
            status[1] = iter; status[0] = code;
            if (mirror) { fs_host_store(mirror + 1, iter); fs_host_store(mirror, code); }
        }
    };
    if (rho <= thresh) { stop(1); return; }     // every workgroup takes the same branch: the inputs are identical
    if (iter >= (int)it_max) { stop(3); return; }
    double beta, alpha;
    if (!cg_scalars_from(iter, gamma, delta, rho, ((iter - 1) & 1) ? sc_g1 : sc_g0, ((iter - 1) & 1) ? sc_a1 : sc_a0, alpha, beta)) { stop(2); return; }
    if (leader) {
        scal[2 * (iter & 1) + 0] = gamma;
        scal[2 * (iter & 1) + 1] = alpha;
        if (MODE != FS_ITER_EVERY) scal[4 + (iter & 1)] = beta;
        it_ctr[par ^ 1] = iter + 1;
        if (mirror) fs_host_store(mirror + 1, iter + 1);
    }
    const double nalpha = -alpha;
    const double alpha_prev = ((iter - 1) & 1) ? sc_a1 : sc_a0, beta_prev = ((iter - 1) & 1) ? sc_b1 : sc_b0;      // (PAIR)
    FS_STAMP(4);
    double d_rz = 0.0, d_wz = 0.0, d_rr = 0.0;
    // PRE: this item's first half round and row-local operands were loaded before the prologue
    auto do_item = [&](const item_hdr& H, auto pre_tag) {
        constexpr bool PRE = decltype(pre_tag)::value;
        const int32_t r = H.first + 2 * lane;
        const bool ok0 = 2 * lane < H.nr, ok1 = 2 * lane + 1 < H.nr;
        int c0 = -1, c1 = -1;
        if ((H.first & 1) == 0) {
            const uint32_t two = *reinterpret_cast<const uint32_t*>(&cls[r]);
            if (ok0) c0 = (int)(two & 0xffffu);
            if (ok1) c1 = (int)(two >> 16);
        } else {
            if (ok0) c0 = (int)cls[r];
            if (ok1) c1 = (int)cls[r + 1];
        }
        v2d sn0 = {0.0, 0.0}, ro0 = {0.0, 0.0};
        v2d pp, xx, dd, rp;
        if (PRE) { pp = Ppp; xx = Pxx; dd = Pdd; rp = Prp; }
        else load_own(H, pp, xx, dd, rp);
        if (DTAB) { dd.x = sdtab[ok0 ? c0 : 0]; dd.y = sdtab[ok1 ? c1 : 0]; }
        const double* __restrict__ v0 = sdict + (ok0 ? c0 * S : 0);
        const double* __restrict__ v1 = sdict + (ok1 ? c1 * S : 0);
        double a0 = 0.0, a1 = 0.0;
        v2d zi = {0.0, 0.0};
        // one run: its terms in ascending offsets, one fma each (the order and the bits of k_dict_spmv)
        auto run_terms = [&](v2d rn, const double* __restrict__ w0, const double* __restrict__ w1) {
            const double e0 = rn.x, e1 = rn.y;
            const double e2 = fs_from_next_lane(rn.x);
            a0 = fma(w0[0], e0, a0); a1 = fma(w1[0], e1, a1);
            a0 = fma(w0[1], e1, a0); a1 = fma(w1[1], e2, a1);
            if (RL == 3) {
                const double e3 = fs_from_next_lane(rn.y);
                a0 = fma(w0[2], e2, a0); a1 = fma(w1[2], e3, a1);
            }
        };
        if (GUARD || !H.edge) {
            const uint32_t boff = (uint32_t)r * 8u;
            // (CENTRE: one round, known to the host only - with the trip count a constant the compiler schedules the PAIR launch with 172
            // VGPRs, two waves per SIMD; as a loop 114)
            for (int rd = 0; rd < H.rounds; ++rd) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    v2d A[4], Wb[4], Sb[4];
                    const bool skip0 = CENTRE && h == 0;        // (slot 0, the z run: neither loaded nor multiplied)
                    if (PRE && h == 0) {
                        if (rd == 0) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) { A[j] = PA[j]; Wb[j] = PW[j]; Sb[j] = PS[j]; }
                        } else load_half(H, rd, h, boff, A, Wb, Sb);
                    } else load_half(H, rd, h, boff, A, Wb, Sb, skip0);
                    // the new r on these columns: r - alpha (w + beta s), two fmas per value - the owner's operations, the owner's bits
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if ((skip0 && j == 0) || dropped(h, j)) continue;
                        v2d sn;
                        sn.x = fma(beta, Sb[j].x, Wb[j].x); sn.y = fma(beta, Sb[j].y, Wb[j].y);
                        if (!CENTRE && h == 0 && j == 0 && rd == 0) { sn0 = sn; ro0 = A[0]; }
                        // (CENTRE: slot 4 is the run (-1; 3) - columns r - 1, r of this lane, r + 1 the next lane's first: the own two
                        // rows, the same memory words the z run loads, through the same two fmas)
                        if (CENTRE && h == 1 && j == 0) {
                            sn0.x = sn.y; sn0.y = fs_from_next_lane(sn.x);
                            ro0.x = A[0].y; ro0.y = fs_from_next_lane(A[0].x);
                        }
                        A[j].x = fma(nalpha, sn.x, A[j].x); A[j].y = fma(nalpha, sn.y, A[j].y);
                    }
                    if (!CENTRE && h == 0 && rd == 0) zi = A[0];
                    if (CENTRE && h == 1) { zi.x = A[0].y; zi.y = fs_from_next_lane(A[0].x); }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if ((skip0 && j == 0) || dropped(h, j)) continue;
                        run_terms(A[j], v0 + RL * (8 * rd + 4 * h + j), v1 + RL * (8 * rd + 4 * h + j));
                        asm volatile("" ::: "memory");
                    }
                }
            }
        } else {
            // items whose loads could leave [0, n_cols) (first / last mesh plane; 1.4 % of the rows at 10 M): run by run, each value
            // clamped into the vector (a column outside it has a zero coefficient)
            const int n_runs = 8 * H.rounds;
#pragma unroll 1
            for (int g = 0; g < n_runs; ++g) {
                const int32_t c = r + __builtin_amdgcn_readfirstlane(H.pl[g >> 3].start[g & 7]);
                const int32_t ca = c < 0 ? 0 : (c > cmax ? cmax : c), cb = c + 1 < 0 ? 0 : (c + 1 > cmax ? cmax : c + 1);
                v2d rn, sn;
                sn.x = fma(beta, s_in[ca], w_in[ca]); sn.y = fma(beta, s_in[cb], w_in[cb]);
                const double ra = r_in[ca], rb = r_in[cb];
                if (g == 0) { sn0 = sn; ro0.x = ra; ro0.y = rb; }
                rn.x = fma(nalpha, sn.x, ra); rn.y = fma(nalpha, sn.y, rb);
                if (g == 0) zi = rn;
                run_terms(rn, v0 + RL * g, v1 + RL * g);
            }
        }
        // own rows: p, x, and the new s, r, w
        v2d pn = {0.0, 0.0}, xn = {0.0, 0.0};
        if (MODE == FS_ITER_PAIR) {             // the step launch k - 1 left owed, in its operands
            pp.x = fma(beta_prev, pp.x, rp.x); pp.y = fma(beta_prev, pp.y, rp.y);
            xx.x = fma(alpha_prev, pp.x, xx.x); xx.y = fma(alpha_prev, pp.y, xx.y);
        }
        if (MODE != FS_ITER_LIGHT) {
            pn.x = fma(beta, pp.x, ro0.x); pn.y = fma(beta, pp.y, ro0.y);
            xn.x = fma(alpha, pn.x, xx.x); xn.y = fma(alpha, pn.y, xx.y);
        }
        constexpr bool PX =
#ifdef FS_ITER_ABLATE_PXD
            false;
#else
            MODE != FS_ITER_LIGHT;
#endif
        if (ok1) {
            v2d out;
            out.x = a0; out.y = a1;
            *reinterpret_cast<v2du*>(&w_out[r]) = out;
            *reinterpret_cast<v2du*>(&r_out[r]) = zi;
            *reinterpret_cast<v2du*>(&s_out[r]) = sn0;
            if (PX) {
                *reinterpret_cast<v2du*>(&pv[r]) = pn;
                *reinterpret_cast<v2du*>(&xv[r]) = xn;
            }
        } else if (ok0) {
            w_out[r] = a0; r_out[r] = zi.x; s_out[r] = sn0.x;
            if (PX) { pv[r] = pn.x; xv[r] = xn.x; }
        }
        if (!ok0) { a0 = 0.0; zi.x = 0.0; }
        if (!ok1) { a1 = 0.0; zi.y = 0.0; }
        d_rz += zi.x * zi.x + zi.y * zi.y; d_wz += a0 * zi.x + a1 * zi.y; d_rr += dd.x * zi.x * zi.x + dd.y * zi.y * zi.y;
    };
    if (have0) {
        do_item(H0, std::true_type{});
        it.cur += it.step;
    }
    FS_STAMP(5);
    for (; it.cur < it.end; it.cur += it.step) {
        const int64_t q = it.cur * 4 + wave;
        if (q >= n_items) break;
        do_item(decode(q), std::false_type{});
    }
    FS_STAMP(6);
    // this workgroup's three dot partials: fs_block_sum's order (shuffle tree, then (0 + 1) + (2 + 3)), one barrier for the three
    double dsum[3] = {d_rz, d_wz, d_rr};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dsum[j] += __shfl_down(dsum[j], off, 64);
        if (lane == 0) lds34e[j][wave] = dsum[j];
    }
    __syncthreads();
    FS_STAMP(7);
    if (threadIdx.x < 3) part_out[(int64_t)threadIdx.x * npart + blockIdx.x] =
        (lds34e[threadIdx.x][0] + lds34e[threadIdx.x][1]) + (lds34e[threadIdx.x][2] + lds34e[threadIdx.x][3]);
}

// The step a solve of LIGHT / PAIR launches still owes x when the recurrence stops in an odd launch k (convergence, iteration limit,
// breakdown: status[1] = k): x_k = x_{k-1} + alpha_{k-1} (r_{k-1} + beta_{k-1} p_{k-2}), the two fmas launch k - 1 would have applied.
// Not done inside the stopping launch: a workgroup that starts late there sees the status word already set and returns.  k - 1 is even:
// r_{k-1} is in the parity-0 buffer, alpha_{k-1} in scal[1], beta_{k-1} in scal[4].  Decides for itself from the status word (no host
// round trip); p is not written: nothing reads it after the solve.
__global__ void __launch_bounds__(FS_BLOCK) k_cg_pair_flush(int64_t n, const int* __restrict__ status, const double* __restrict__ scal,
                                                            const double* __restrict__ r_prev, const double* __restrict__ p, double* __restrict__ x) {
    const int st0 = status[0], it = status[1];
    const double alpha = scal[1], beta = scal[4];
    if (st0 == 0 || !(it & 1)) return;
    const int64_t n2 = n >> 1;
    const double2* __restrict__ r2 = reinterpret_cast<const double2*>(r_prev);
    const double2* __restrict__ p2 = reinterpret_cast<const double2*>(p);
    double2* __restrict__ x2 = reinterpret_cast<double2*>(x);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        const double2 rr = r2[i], pp = p2[i];
        double2 xx = x2[i];
        xx.x = fma(alpha, fma(beta, pp.x, rr.x), xx.x);
        xx.y = fma(alpha, fma(beta, pp.y, rr.y), xx.y);
        x2[i] = xx;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = fma(alpha, fma(beta, p[n - 1], r_prev[n - 1]), x[n - 1]);
}

// The same update on the rows [0, a) and [b, n) only - the rows a slab sends to its neighbours - so that the halo
// exchange of the new r can start before the bulk of the update and the interior product are even launched (several
// GPUs: sums from the all-reduce).  No side effects: status, history and the scalars are written by the launch on the
// remaining rows, which comes later in the stream and takes the same decisions from the same inputs.
__global__ void __launch_bounds__(FS_BLOCK) k_cg_update_scaled_rows(int64_t a, int64_t b, int64_t n, int iter, int check_only,
                                                                    const double* __restrict__ sums, const double* __restrict__ ctrl,
                                                                    const double* __restrict__ scal, const int* __restrict__ status,
                                                                    double* __restrict__ r, const double* __restrict__ w,
                                                                    double* __restrict__ p, double* __restrict__ sv, double* __restrict__ x) {
    if (status[0] != 0) return;
    const double gamma = sums[0], delta = sums[1], rho = sums[2];
    if (rho <= ctrl[0] || check_only) return;
    double beta, alpha;
    if (!cg_scalars(iter, gamma, delta, rho, scal, alpha, beta)) return;
    const int64_t total = a + (n - b);
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; t < total; t += stride) {
        const int64_t i = t < a ? t : b + (t - a);
        const double pp = r[i] + beta * p[i];
        const double ss = w[i] + beta * sv[i];
        p[i] = pp; sv[i] = ss;
        x[i] += alpha * pp;
        r[i] -= alpha * ss;
    }
}

// ---- the exchange kernel of the peer-to-peer iteration (fs_comm.hip: hipIpc-mapped buffers; protocol in fs_kernels.h) -----------
// Everything of a CG iteration that crosses GPUs, in ONE launch between the product and the update.  What travels is w = A r on
// the rows some neighbour needs - known as soon as the product is through, with no dependence on the sums - and NOT the new
// residual: a rank advances the ghost copies of r and s itself (s_g <- w_g + beta s_g, r_g <- r_g - alpha s_g are row-local and it
// knows alpha, beta), with the operations the owner's update kernel applies to the same rows.
//   1. every workgroup stores its share of w[send rows] straight into the neighbours' receive buffers, the last one through
//      publishes the sequence number of the exchange at every neighbour;
//   2. (meanwhile on the wire) every workgroup sums the product's dot partials itself (same bits everywhere); workgroup 0
//      stores the three sums into slot [me] of the other ranks' all-reduce buffers; every workgroup waits for the other ranks'
//      sums and adds all up in rank order; workgroup 0 leaves the result in `sums` for the update kernel that follows;
//   3. every workgroup waits for the neighbours' sequence numbers and advances its share of the ghost rows with the received w.
// (No workgroup waits before its own stores are counted, so two ranks never wait for each other.)  Any halo plan (send lists
// need not be contiguous, ghosts may be scattered), any block size: rows are dofs here.  Gated by the status word; steps 1 and
// 2 always run together, step 3 only if the iteration goes on - decided from the reduced sums, hence alike on every rank.
// PP: the exchange of the ONE-LAUNCH iteration on a decomposed space (k_dict_cg_iter<3, true> follows): r, w, s are double-buffered by
// iteration parity and that kernel recomputes the new residual on its neighbour columns - ghost columns included - from the OLD r, w,
// s.  So the received w goes into the ghost rows of the current w (pp.w_cur), and the ghost rows of s and r are advanced from the
// current buffers into the next ones (pp.s_cur -> pp.s_nxt, pp.r_cur -> pp.r_nxt): the two fmas of the owner.  The iteration number
// comes from it_ctr[par] (written by the previous iteration kernel).
struct fs_pp_ghosts {
    double* w_cur;
    const double* s_cur;
    double* s_nxt;
    const double* r_cur;
    double* r_nxt;
    const int* it_ctr;
    int par;
};
template <bool PP>
__global__ void __launch_bounds__(FS_BLOCK) k_cg_p2p_exchange(int iter, int check_only, const double* __restrict__ ctrl,
                                                              const double* __restrict__ scal, const int* __restrict__ status,
                                                              double* r, const double* __restrict__ w, double* __restrict__ s_ghost,
                                                              const fs_p2p_rowsred red, const fs_p2p_sendrows snd, const fs_pp_ghosts pp) {
    // (every scalar the launch needs is asked for before the first of them is looked at: each was written by the previous launch,
    // a dependent load is a round trip of about a microsecond, and this kernel sits on the critical path of every iteration)
    const int st0 = status[0], st2 = status[2];
    const double it_max = ctrl[2], thresh = ctrl[0];
    const double sc_g0 = scal[0], sc_a0 = scal[1], sc_g1 = scal[2], sc_a1 = scal[3];
    // sequence numbers of THIS exchange: one past the last executed ones (fs_comm.hip); read by every workgroup at its start,
    // advanced by the last workgroup through each part
    const unsigned long long rseq = *red.d_seq + 1ull, hseq = *snd.d_seq + 1ull;
    const int it_dev = PP ? pp.it_ctr[pp.par] : 0;
    if (st0 != 0) return;
    if (PP) {
        iter = it_dev;
        check_only = iter >= (int)it_max ? 1 : 0;
    } else if (iter < 0) {          // captured batch: the index of the product that preceded this launch
        iter = st2 - 1;
        check_only = iter >= (int)it_max ? 1 : 0;
    }
    const int rslot = (int)(rseq & 1ull), hslot = (int)(hseq & 1ull);
    const int64_t e_first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int t = threadIdx.x;
    // 1. w on the interface rows -> the neighbours
    for (int64_t e = e_first; e < snd.total_send; e += stride) {
        const double wv = w[snd.send_idx[e]];
        int j = 0;
        while (j + 1 < snd.nn && e >= snd.peers[j + 1].send_offset) ++j;
        const fs_p2p_peer q = snd.peers[j];
        fs_p2p_store(q.recv + (int64_t)hslot * q.peer_total + q.recv_offset + (e - q.send_offset), wv);
    }
    fs_p2p_stores_done();
    __syncthreads();
    if (t == 0 && atomicAdd(snd.counter, 1u) == gridDim.x - 1) {
        __hip_atomic_store(snd.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(snd.d_seq, hseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int j = 0; j < snd.nn; ++j) {
            const fs_p2p_peer q = snd.peers[j];
            fs_p2p_publish(q.flags + (int64_t)hslot * q.peer_nn + q.peer_slot, hseq);
        }
    }
    // 2. the sums of all ranks
    double sm[3];
    wg_sum_partials<3>(red.partials, red.npart, sm);
    if (blockIdx.x == 0 && t < red.nr && t != red.me) {
        double* dst = red.peer_buf[t] + ((int64_t)rslot * red.nr + red.me) * 8;
        fs_p2p_store(dst, sm[0]); fs_p2p_store(dst + 1, sm[1]); fs_p2p_store(dst + 2, sm[2]);
        fs_p2p_stores_done();
        fs_p2p_publish(red.peer_flags[t] + (int64_t)rslot * red.nr + red.me, rseq);
    }
    if (t < red.nr && t != red.me) fs_p2p_wait(red.own_flags + (int64_t)rslot * red.nr + t, rseq, red.timeout, red.err);
    __syncthreads();
    __shared__ double tot[3];
    if (t < 3) {
        double a = 0.0;
        for (int q = 0; q < red.nr; ++q)
            a += q == red.me ? sm[t] : fs_p2p_load(red.own_buf + ((int64_t)rslot * red.nr + q) * 8 + t);
        tot[t] = a;
        if (blockIdx.x == 0) red.sums_out[t] = a;
    }
    if (t == 0 && atomicAdd(red.counter, 1u) == gridDim.x - 1) {          // every workgroup has read d_seq and the other ranks' sums
        __hip_atomic_store(red.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(red.d_seq, rseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const double gamma = tot[0], delta = tot[1], rho = tot[2];
    if (rho <= thresh || check_only) return;
    double beta, alpha;
    if (!cg_scalars_from(iter, gamma, delta, rho, ((iter - 1) & 1) ? sc_g1 : sc_g0, ((iter - 1) & 1) ? sc_a1 : sc_a0, alpha, beta)) return;
    // 3. ghost rows: s_g <- w_g + beta s_g, r_g <- r_g - alpha s_g (the two lines of the update kernel)
    if (t < snd.nn) fs_p2p_wait(snd.own_flags + (int64_t)hslot * snd.nn + t, hseq, snd.timeout, snd.err);
    __syncthreads();
    const double* own_recv = snd.own_recv + (int64_t)hslot * snd.recv_stride;
    for (int64_t k = e_first; k < snd.total_recv; k += stride) {
        const int64_t gi = snd.recv_idx ? (int64_t)snd.recv_idx[k] : snd.n_owned + k;
        if (PP) {
            const double wv = fs_p2p_load(own_recv + k);
            pp.w_cur[gi] = wv;
            const double ss = fma(beta, pp.s_cur[gi], wv);
            pp.s_nxt[gi] = ss;
            pp.r_nxt[gi] = fma(-alpha, ss, pp.r_cur[gi]);
        } else {
            const double ss = fs_p2p_load(own_recv + k) + beta * s_ghost[k];
            s_ghost[k] = ss;
            r[gi] -= alpha * ss;
        }
    }
}

// ---- pipelined CG (Ghysels & Vanroose, Parallel Computing 40 (2014)) on the scaled system --------------------------
// The single-reduction recurrence above still has the global sums between the product and the update: on several GPUs the
// 3-double all-reduce (latency, not bandwidth) is paid in full every iteration.  The pipelined recurrence carries two more
// vectors (w = A r, z = A s) so that the sums of iteration i - (r.r, w.r, sum d r^2) of r_i, w_i - are known BEFORE the
// product n_i = A w_i starts and are reduced while it runs:
//      beta = gamma_i / gamma_{i-1},  alpha = gamma_i / (delta_i - beta gamma_i / alpha_{i-1})
//      z = n + beta z;  s = w + beta s;  p = r + beta p;   x += alpha p;  r -= alpha s;  w -= alpha z
// In exact arithmetic the iterates are those of CG.  The update kernel computes the sums of the NEW r, w as it writes
// them (per-workgroup partials, double-buffered by iteration parity because the next launch reads one set while it writes
// the other).  112 instead of 72 B/DOF of vector traffic per iteration: it only pays where a collective is hidden.
// Rows [m0, m1) are updated by this launch; rows [0, m0) and [m1, n) - what a slab sends to its neighbours - were already
// updated by k_pcg_update_rows (so that their exchange could start) and only enter the sums here.
template <bool FUSED, bool NT>
__global__ void __launch_bounds__(FS_BLOCK) k_pcg_update(int64_t n, int64_t m0, int64_t m1, int iter, int check_only,
                                                         double* __restrict__ partials, int npart,
                                                         const double* __restrict__ sums, const double* __restrict__ ctrl,
                                                         double* __restrict__ scal, int* __restrict__ status,
                                                         double* __restrict__ hist, const double* __restrict__ dvec,
                                                         double* __restrict__ r, double* __restrict__ w,
                                                         const double* __restrict__ nv, double* __restrict__ p,
                                                         double* __restrict__ sv, double* __restrict__ z,
                                                         double* __restrict__ x) {
    if (status[0] != 0) return;
    double gamma, delta, rho;
    if (FUSED) {
        double sm[3];
        wg_sum_partials<3>(partials + (int64_t)(iter & 1) * 3 * npart, npart, sm);
        gamma = sm[0]; delta = sm[1]; rho = sm[2];
    } else {
        gamma = sums[0]; delta = sums[1]; rho = sums[2];
    }
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    if (leader) hist[iter] = rho;
    if (rho <= ctrl[0]) {
        if (leader) { status[1] = iter; status[0] = 1; }
        return;
    }
    if (check_only) {
        if (leader) { status[1] = iter; status[0] = 3; }
        return;
    }
    double alpha, beta;
    if (!cg_scalars(iter, gamma, delta, rho, scal, alpha, beta)) {
        if (leader) { status[1] = iter; status[0] = 2; }
        return;
    }
    if (leader) {
        scal[2 * (iter & 1) + 0] = gamma;
        scal[2 * (iter & 1) + 1] = alpha;
    }
    typedef double v2d __attribute__((ext_vector_type(2)));
    struct io {
        static __device__ __forceinline__ v2d ld(const double* q) {
            return NT ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(q)) : *reinterpret_cast<const v2d*>(q);
        }
        static __device__ __forceinline__ void st(double* q, const v2d& v) {
            if (NT) __builtin_nontemporal_store(v, reinterpret_cast<v2d*>(q));
            else *reinterpret_cast<v2d*>(q) = v;
        }
    };
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t npair = (m1 - m0) >> 1;              // m0 is even
    for (int64_t q = tid; q < npair; q += stride) {
        const int64_t i = m0 + 2 * q;
        const v2d nn = io::ld(nv + i), dd = io::ld(dvec + i);
        v2d zz = io::ld(z + i), ss = io::ld(sv + i), pp = io::ld(p + i), ww = io::ld(w + i), rr = io::ld(r + i), xx = io::ld(x + i);
        zz = nn + beta * zz;
        ss = ww + beta * ss;
        pp = rr + beta * pp;
        xx += alpha * pp;
        rr -= alpha * ss;
        ww -= alpha * zz;
        io::st(z + i, zz); io::st(sv + i, ss); io::st(p + i, pp); io::st(x + i, xx); io::st(r + i, rr); io::st(w + i, ww);
        a0 += rr.x * rr.x + rr.y * rr.y;
        a1 += ww.x * rr.x + ww.y * rr.y;
        a2 += dd.x * rr.x * rr.x + dd.y * rr.y * rr.y;
    }
    if (((m1 - m0) & 1) && tid == 0) {
        const int64_t i = m1 - 1;
        const double zz = nv[i] + beta * z[i], ss = w[i] + beta * sv[i], pp = r[i] + beta * p[i];
        z[i] = zz; sv[i] = ss; p[i] = pp;
        x[i] += alpha * pp;
        const double rr = r[i] - alpha * ss, ww = w[i] - alpha * zz;
        r[i] = rr; w[i] = ww;
        a0 += rr * rr; a1 += ww * rr; a2 += dvec[i] * rr * rr;
    }
    // rows already updated by k_pcg_update_rows
    const int64_t extra = m0 + (n - m1);
    for (int64_t t = tid; t < extra; t += stride) {
        const int64_t i = t < m0 ? t : m1 + (t - m0);
        const double rr = r[i], ww = w[i];
        a0 += rr * rr; a1 += ww * rr; a2 += dvec[i] * rr * rr;
    }
    __shared__ double lds4[4];
    const double t0 = fs_block_sum(a0, lds4);
    const double t1 = fs_block_sum(a1, lds4);
    const double t2 = fs_block_sum(a2, lds4);
    if (threadIdx.x == 0) {
        double* out = partials + (int64_t)((iter + 1) & 1) * 3 * npart;
        out[blockIdx.x] = t0;
        out[npart + blockIdx.x] = t1;
        out[2 * npart + blockIdx.x] = t2;
    }
}

// The pipelined update on the rows [0, a) and [b, n) only (sums from the all-reduce): no side effects, the launch on
// the remaining rows takes the same decisions from the same inputs and writes status / history / scalars.
__global__ void __launch_bounds__(FS_BLOCK) k_pcg_update_rows(int64_t a, int64_t b, int64_t n, int iter, int check_only,
                                                              const double* __restrict__ sums, const double* __restrict__ ctrl,
                                                              const double* __restrict__ scal, const int* __restrict__ status,
                                                              double* __restrict__ r, double* __restrict__ w,
                                                              const double* __restrict__ nv, double* __restrict__ p,
                                                              double* __restrict__ sv, double* __restrict__ z, double* __restrict__ x) {
    if (status[0] != 0) return;
    const double gamma = sums[0], delta = sums[1], rho = sums[2];
    if (rho <= ctrl[0] || check_only) return;
    double alpha, beta;
    if (!cg_scalars(iter, gamma, delta, rho, scal, alpha, beta)) return;
    const int64_t total = a + (n - b);
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; t < total; t += stride) {
        const int64_t i = t < a ? t : b + (t - a);
        const double zz = nv[i] + beta * z[i], ss = w[i] + beta * sv[i], pp = r[i] + beta * p[i];
        z[i] = zz; sv[i] = ss; p[i] = pp;
        x[i] += alpha * pp;
        r[i] -= alpha * ss;
        w[i] -= alpha * zz;
    }
}

// sums of the first iterate of a pass: partials (parity 0) of (r.r, w.r, sum d r^2)
__global__ void __launch_bounds__(FS_BLOCK) k_pcg_dots(int64_t n, const double* __restrict__ r, const double* __restrict__ w,
                                                       const double* __restrict__ dvec, double* __restrict__ partials, int npart) {
    __shared__ double lds4[4];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double rr = r[i], ww = w[i];
        a0 += rr * rr; a1 += ww * rr; a2 += dvec[i] * rr * rr;
    }
    const double t0 = fs_block_sum(a0, lds4);
    const double t1 = fs_block_sum(a1, lds4);
    const double t2 = fs_block_sum(a2, lds4);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = t0;
        partials[npart + blockIdx.x] = t1;
        partials[2 * npart + blockIdx.x] = t2;
    }
}

// aval = D^-1/2 A D^-1/2 (copy; the caller's matrix is left untouched), sc = 1/sqrt(diag)
template <int BS>
__global__ void __launch_bounds__(FS_BLOCK) k_scale_copy(int64_t n_rows, int64_t n_slices,
                                                         const int64_t* __restrict__ slice_ptr,
                                                         const int32_t* __restrict__ sell_col,
                                                         const double* __restrict__ val, int64_t plane,
                                                         const double* __restrict__ sc, double* __restrict__ aval) {
    const int lane = threadIdx.x & 63;
    int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (; s < n_slices; s += stride) {
        const int64_t r = s * FS_SLICE + lane;
        const int64_t base = slice_ptr[s] + lane;
        const int width = (int)((slice_ptr[s + 1] - slice_ptr[s]) >> 6);
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            const int32_t c = sell_col[e];
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) {
                    const int64_t idx = (int64_t)(i * BS + j) * plane + e;
                    aval[idx] = (c >= 0 && r < n_rows) ? val[idx] * sc[r * BS + i] * sc[(int64_t)c * BS + j] : 0.0;
                }
        }
    }
}

__global__ void k_pointwise_div(const double* __restrict__ a, const double* __restrict__ b, int64_t n,
                                double* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = a[i] / b[i];
}

// partial of sum d (b - w)^2 ; optionally r = b - w
__global__ void __launch_bounds__(FS_BLOCK) k_residual_scaled(const double* __restrict__ b, const double* __restrict__ w,
                                                              const double* __restrict__ d, int64_t n,
                                                              double* __restrict__ r, double* __restrict__ partial) {
    __shared__ double lds4[4];
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double x = b[i] - w[i];
        if (r) r[i] = x;
        acc += d[i] * x * x;
    }
    const double t = fs_block_sum(acc, lds4);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

template <int BS>
__global__ void k_extract_dinv(int64_t n_rows, const int64_t* __restrict__ slice_ptr,
                               const int32_t* __restrict__ sell_col, const double* __restrict__ val, int64_t plane,
                               int jacobi, double* __restrict__ dinv, int* __restrict__ err,
                               double* __restrict__ dvec = nullptr) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_rows; r += stride) {
        const int64_t sp0 = slice_ptr[r >> 6];
        const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
        const int64_t base = sp0 + (r & 63);
        int kd = -1;
        for (int k = 0; k < width; ++k)
            if (sell_col[base + (int64_t)k * FS_SLICE] == r) { kd = k; break; }
        for (int i = 0; i < BS; ++i) {
            double d = 1.0;
            if (jacobi) {
                d = kd >= 0 ? val[(int64_t)(i * BS + i) * plane + base + (int64_t)kd * FS_SLICE] : 0.0;
                if (!(d != 0.0) || (jacobi == 2 && !(d > 0.0))) { atomicAdd(err, 1); d = 1.0; }
                if (dvec) dvec[r * BS + i] = d;
                d = jacobi == 2 ? 1.0 / sqrt(d) : 1.0 / d;
            }
            dinv[r * BS + i] = d;
        }
    }
}

__global__ void k_pointwise_mul(const double* __restrict__ a, const double* __restrict__ b, int64_t n,
                                double* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = a[i] * b[i];
}

// r = b - w ; partial of r.r
__global__ void __launch_bounds__(FS_BLOCK) k_residual(const double* __restrict__ b, const double* __restrict__ w,
                                                       int64_t n, double* __restrict__ r,
                                                       double* __restrict__ partial) {
    __shared__ double lds4[4];
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const double d = b[i] - w[i];
        if (r) r[i] = d;
        acc += d * d;
    }
    const double t = fs_block_sum(acc, lds4);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// up to four vectors zeroed by ONE launch (the start of a CG pass: p, s, z and x - four memsets of 8 MB each at 1 M rows were four
// launches with their gaps)
__global__ void __launch_bounds__(FS_BLOCK) k_zero4(double* __restrict__ a, int64_t na, double* __restrict__ b, int64_t nb,
                                                    double* __restrict__ c, int64_t nc, double* __restrict__ d, int64_t nd) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double* const ptr[4] = {a, b, c, d};
    const int64_t len[4] = {na, nb, nc, nd};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double* __restrict__ v = ptr[q];
        const int64_t n2 = len[q] >> 1;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) reinterpret_cast<v2d*>(v)[i] = v2d{0.0, 0.0};
        if ((len[q] & 1) && blockIdx.x == 0 && threadIdx.x == 0) v[len[q] - 1] = 0.0;
    }
}

