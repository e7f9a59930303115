// The central-difference ("leapfrog") scheme the explicit solid marchers share (fs_dynamics_explicit.hip: y = K u;
// fs_hyper_dynamics.hip: y = f_int(u)): its constants, its per-row arithmetic, the Dirichlet kernel of u_0 and the part of the state
// object and of the entry points that does not depend on where y comes from.  Header-only, on top of fs_march.h (row table,
// finishing pass, batch driver), which does no floating-point arithmetic of its own: the arithmetic of the scheme is HERE, once.
//
// M a + C v + y(u) = s_f(t) F with the lumped mass m and C = eta_M diag(m).  The state is (u_n, w_n) with w_n = v_{n-1/2}; with
// alpha = eta_M dt / 2 a step n -> n+1 (n >= 1) is, per row,
//   (1 + alpha) w_{n+1/2} = (1 - alpha) w_{n-1/2} + dt (s_f[n] F - y_n) / m,      u_{n+1} = u_n + dt w_{n+1/2},
// and on a Dirichlet row u_{n+1} = g s_g[n+1], w_{n+1/2} = (u_{n+1} - u_n) / dt.  The march starts with
//   a_0 = (s_f[0] F - y_0) / m - eta_M v_0,   w_{1/2} = v_0 + dt/2 a_0,   u_1 = u_0 + dt w_{1/2}
// (the Dirichlet rows of u_0 take g s_g[0] first, those of u_1 by the rule above).  At the state's time point
//   v_n = (w_{n-1/2} + w_{n+1/2}) / 2,   a_n = (w_{n+1/2} - w_{n-1/2}) / dt   (a Dirichlet row: v_n = w_{n-1/2}, a_n = 0),
// and the kinetic energy of the step is E_kin = 1/2 sum_i m_i w_{n+1/2,i}^2.
// The helpers take y as a value and fix the operand order and grouping of every expression: a marcher that calls them gives the
// bits of every other one on the same (u, w, y, m, F).
#pragma once
#include "fs_march.h"
#include <initializer_list>
#include <vector>

// what the kernels take of the scheme, derived from (dt, eta_M) on the host: w+ = c1 w + c2 (s_f F - y) / m
struct fs_leapfrog_consts {
    double dt, idt;
    double c1;                           // (1 - alpha) / (1 + alpha)
    double c2;                           // dt / (1 + alpha)
    double etam;
};

static inline fs_leapfrog_consts fs_leapfrog_consts_of(double dt, double eta_m) {
    const double alpha = 0.5 * eta_m * dt;
    fs_leapfrog_consts c;
    c.dt = dt;
    c.idt = 1.0 / dt;
    c.c1 = (1.0 - alpha) / (1.0 + alpha);
    c.c2 = dt / (1.0 + alpha);
    c.etam = eta_m;
    return c;
}

// ---- the per-row arithmetic --------------------------------------------------------------------------------------------------
// w_{n+1/2} of a free row
__device__ __forceinline__ double fs_leapfrog_w(const fs_leapfrog_consts& c, double w, double y, double m, double f, double sf) {
    return c.c1 * w + c.c2 * ((sf * f - y) / m);
}

struct fs_leapfrog_row {
    double u, w;                         // (u_{n+1}, w_{n+1/2}) of a row
};

// u+ = u + dt w+, and the Dirichlet row (f holds g there)
__device__ __forceinline__ fs_leapfrog_row fs_leapfrog_move(const fs_leapfrog_consts& c, double u, double wn, double f, double sg,
                                                            bool dirichlet) {
    double un = u + c.dt * wn;
    if (dirichlet) {
        un = f * sg;
        wn = (un - u) * c.idt;
    }
    return {un, wn};
}

// (u_n, w_{n-1/2}) -> (u_{n+1}, w_{n+1/2}); sg = s_g[n+1]
__device__ __forceinline__ fs_leapfrog_row fs_leapfrog_step_row(const fs_leapfrog_consts& c, double u, double w, double y, double m, double f,
                                                                double sf, double sg, bool dirichlet) {
    return fs_leapfrog_move(c, u, fs_leapfrog_w(c, w, y, m, f, sf), f, sg, dirichlet);
}

// (u_0, v_0) -> (u_1, w_{1/2}); sg1 = s_g[1]
__device__ __forceinline__ fs_leapfrog_row fs_leapfrog_start_row(const fs_leapfrog_consts& c, double u0, double v0, double y, double m, double f,
                                                                 double sf, double sg1, bool dirichlet) {
    const double a0 = (sf * f - y) / m - c.etam * v0;
    return fs_leapfrog_move(c, u0, v0 + (0.5 * c.dt) * a0, f, sg1, dirichlet);
}

// v_n and a_n from w = w_{n-1/2} and wp = fs_leapfrog_w of the same row
__device__ __forceinline__ double fs_leapfrog_v(double w, double wp, bool dirichlet) { return dirichlet ? w : 0.5 * (w + wp); }
__device__ __forceinline__ double fs_leapfrog_a(const fs_leapfrog_consts& c, double w, double wp, bool dirichlet) {
    return dirichlet ? 0.0 : (wp - w) * c.idt;
}

// the row's term of E_kin
__device__ __forceinline__ double fs_leapfrog_ekin(double m, double wn) { return 0.5 * m * wn * wn; }

// the Dirichlet rows of u_0 take g s_g[0] (a template so that every file that launches it gets its own copy, as k_march_finish)
template <int = 0>
__global__ void __launch_bounds__(FS_BLOCK) k_leapfrog_dirichlet(int64_t n, const double* __restrict__ load, const uint8_t* __restrict__ flag,
                                                                 double sg, double* __restrict__ u) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (flag[i] & FS_MARCH_DIRICHLET) u[i] = load[i] * sg;
}

// ---- the state object and what the entry points share ------------------------------------------------------------------------------
// A marcher derives its state from this one and adds the buffer(s) that hold u and what its y needs.  api: the prefix of its entry
// points ("fs_dyn_explicit"): the refusals name the sibling entry points by it; who: the entry point a message names.  Refusals come
// before uploads: a refused call leaves the state as it was.
struct fs_leapfrog_state : fs_march_batch_state {
    const char* const api;
    fs_leapfrog_consts c = {};
    dbuf<double> w;                      // v_{n-1/2}: updated in place
    dbuf<double> m;                      // lumped mass
    dbuf<double> t0, t1;                 // start: v_0; full_step: v_n, a_n; and what else a marcher hands back per row
    explicit fs_leapfrog_state(const char* api_) : api(api_) {}

    // the row table, the shared buffers and `own` (the marcher's buffers of one double per row), zeroed, and the partial table
    int alloc(int64_t rows, std::initializer_list<dbuf<double>*> own, hipStream_t s) {
        FS_CHECK(alloc_rows(rows, s));
        std::vector<dbuf<double>*> all(own);
        all.insert(all.end(), {&w, &m, &t0, &t1});
        for (dbuf<double>* b : all) {
            FS_CHECK(b->alloc(n));
            FS_CHECK(b->zero(s));
        }
        return alloc_part();
    }

    int configure(const char* who, double dt, double eta_m, const double* mass, const double* load_host, int64_t n_dirichlet,
                  const int32_t* dirichlet_dofs, const double* dirichlet_values) {
        FS_REQUIRE(mass, "%s: null pointer", who);
        FS_REQUIRE(dt > 0.0 && isfinite(dt), "%s: the step length is %g: dt > 0 and finite is required", who, dt);
        FS_REQUIRE(eta_m >= 0.0 && isfinite(eta_m), "%s: the mass damping eta_M is %g: it must be >= 0 and finite", who, eta_m);
        FS_CHECK(fs_march_rows_ok(who, n, mass, nullptr, load_host, n_dirichlet, dirichlet_dofs, dirichlet_values));
        hipStream_t s = fs_rt().stream;
        FS_CHECK(fs_march_rows::configure(who, load_host, n_dirichlet, dirichlet_dofs, dirichlet_values, s));
        FS_CHECK(m.upload(mass, n, s));
        FS_HIP(hipStreamSynchronize(s));
        c = fs_leapfrog_consts_of(dt, eta_m);
        configured = true;
        return FS_OK;
    }

    // u: the buffer that holds u_n
    int set(const char* who, dbuf<double>& u, const double* u_host, const double* w_host, int64_t step_) {
        FS_REQUIRE(u_host && w_host, "%s: null pointer", who);
        FS_REQUIRE(step_ >= 1, "%s: the step counter is %lld: (u_n, v_{n-1/2}) needs n >= 1", who, (long long)step_);
        hipStream_t s = fs_rt().stream;
        FS_CHECK(u.upload(u_host, n, s));
        FS_CHECK(w.upload(w_host, n, s));
        FS_HIP(hipStreamSynchronize(s));
        step = step_;
        return FS_OK;
    }

    int get(dbuf<double>& u, double* u_host, double* w_host, int64_t* step_) {
        hipStream_t s = fs_rt().stream;
        if (u_host) FS_CHECK(u.download(u_host, n, s));
        if (w_host) FS_CHECK(w.download(w_host, n, s));
        FS_HIP(hipStreamSynchronize(s));
        if (step_) *step_ = step;
        return FS_OK;
    }

    // started: the call needs (u_n, v_{n-1/2})
    int ready(const char* who, bool started) const {
        FS_REQUIRE(configured, "%s: the state was not configured (%s_state_configure)", who, api);
        FS_REQUIRE(!started || step >= 1, "%s: the state holds no (u_n, v_{n-1/2}) yet (%s_start or %s_state_set)", who, api, api);
        return FS_OK;
    }

    int start_ok(const char* who, const double* u0, const double* v0, double load_scale0, double dirichlet_scale0,
                 double dirichlet_scale1) const {
        FS_REQUIRE(u0 && v0, "%s: null pointer", who);
        FS_REQUIRE(isfinite(load_scale0) && isfinite(dirichlet_scale0) && isfinite(dirichlet_scale1), "%s: a time factor is not finite", who);
        return FS_OK;
    }

    // u_0 into u with its Dirichlet rows at g s_g[0], v_0 into t0; the marcher forms y from u and launches its start kernel behind it
    int start_fields(dbuf<double>& u, const double* u0, const double* v0, double dirichlet_scale0, hipStream_t s) {
        FS_CHECK(u.upload(u0, n, s));
        FS_CHECK(t0.upload(v0, n, s));
        step = 0;
        hipLaunchKernelGGL(k_leapfrog_dirichlet<>, dim3(fs_march_grid(n)), dim3(FS_BLOCK), 0, s, n, load.p, flag.p, dirichlet_scale0, u.p);
        FS_KERNEL_CHECK();
        return FS_OK;
    }

    // the tail of full_step: (v_n, a_n) are in (t0, t1)
    int full_step_out(double* v_out, double* a_out, hipStream_t s) {
        if (v_out) FS_CHECK(t0.download(v_out, n, s));
        if (a_out) FS_CHECK(t1.download(a_out, n, s));
        FS_HIP(hipStreamSynchronize(s));
        FS_KERNEL_CHECK();
        return FS_OK;
    }
};
