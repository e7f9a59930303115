// Explicit structural dynamics on vector CG1 spaces (tetrahedra, triangles in plane strain): the central-difference marcher of
// ElastodynamicsSolver ('scheme': 'explicit'), on the device.
//
// The reference has no transient structural solver; the model is the textbook one: M a + C v + K u = s_f(t) F with the isotropic
// elasticity operator K, the LUMPED mass m = M 1 (the row sums of the consistent mass, > 0 on CG1) and mass-proportional damping
// C = eta_M diag(m), marched by central differences in the leapfrog form.  The state is (u_n, w_n) with w_n = v_{n-1/2}; with
// y_n = K u_n and alpha = eta_M dt / 2 a step n -> n+1 (n >= 1) is, per row,
//   (1 + alpha) w_{n+1/2} = (1 - alpha) w_{n-1/2} + dt (s_f[n] F - y_n) / m,      u_{n+1} = u_n + dt w_{n+1/2},
// and on a Dirichlet row u_{n+1} = g s_g[n+1], w_{n+1/2} = (u_{n+1} - u_n) / dt.  The march starts with
//   a_0 = (s_f[0] F - y_0) / m - eta_M v_0,   w_{1/2} = v_0 + dt/2 a_0,   u_1 = u_0 + dt w_{1/2}
// (the Dirichlet rows of u_0 take g s_g[0] first, those of u_1 by the rule above).  The discrete energy of the step is
//   E_kin = 1/2 sum_i m_i w_{n+1/2,i}^2,   E_pot = 1/2 u_{n+1}^T y_n,
// and with F = 0 and fixed Dirichlet values E_{n+1/2} - E_{n-1/2} = -eta_M dt v_n^T diag(m) v_n with v_n = (w_{n-1/2} + w_{n+1/2}) / 2.
// A step is therefore NOT a solve: one product with K - the library's own, through the dispatch of fs_spmv (fs_spmv_dev), so box
// and dictionary operators keep their fast products - and one pass over the rows.  fs_dyn_explicit_advance enqueues any number of
// steps back to back; the host touches nothing in between (the time factors of a step travel as kernel arguments).
//
// Kernels (no floating-point atomics: a march gives the same bits however it is split into calls):
//   k_dynx_update   one thread per row, grid-stride over a launch geometry that depends on the number of rows only, 8-byte loads
//       that a wave coalesces into full lines: the update formula, the Dirichlet rows, the receiver samples and the per-workgroup
//       partials of both energy halves.  Per row it reads y, u, w, m, F (8 B each) and one flag byte and writes u and w in place
//       (a row is read and written by its own thread only): 57 B.  A non-finite u makes the next y and with it w and E_kin
//       non-finite, so the finishing pass's check of the energy is also the check of the fields.
//   k_dynx_dirichlet / k_dynx_start   the Dirichlet rows of u_0, then the first step from (u_0, v_0).
//   k_dynx_full_step   v_n and a_n of the state's time point from (w_{n-1/2}, y_n): w+ is recomputed, nothing is stored.
// The row table (load, flags, receivers), the finishing pass, the batch driver and the shared checks: fs_march.h.
#include "fs_march.h"
#include <mutex>

// what the kernels take of the scheme, derived from (dt, eta_M) on the host: w+ = c1 w + c2 (s_f F - y) / m
struct dynx_consts {
    double dt, idt;
    double c1;                           // (1 - alpha) / (1 + alpha)
    double c2;                           // dt / (1 + alpha)
    double etam;
};

struct fs_dyn_explicit_state_s : fs_march_batch_state {
    dynx_consts c = {};
    dbuf<double> u, w;                   // u_n, v_{n-1/2}: updated in place
    dbuf<double> y;                      // K u of the last product
    dbuf<double> m;                      // lumped mass
    dbuf<double> t0, t1;                 // fs_dyn_explicit_start: v_0; fs_dyn_explicit_full_step: v_n, a_n
};

// ---- the start -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FS_BLOCK) k_dynx_dirichlet(int64_t n, const double* __restrict__ load, const uint8_t* __restrict__ flag,
                                                             double sg, double* __restrict__ u) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (flag[i] & FS_MARCH_DIRICHLET) u[i] = load[i] * sg;
}

// u: u_0 in, u_1 out; w: w_{1/2} out
__global__ void __launch_bounds__(FS_BLOCK) k_dynx_start(int64_t n, const double* __restrict__ y, const double* __restrict__ v0,
                                                         const double* __restrict__ m, const double* __restrict__ load,
                                                         const uint8_t* __restrict__ flag, dynx_consts c, double sf, double sg1,
                                                         double* __restrict__ u, double* __restrict__ w) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double fi = load[i], vi = v0[i], ui = u[i];
        const double a0 = (sf * fi - y[i]) / m[i] - c.etam * vi;
        double wn = vi + (0.5 * c.dt) * a0;
        double un = ui + c.dt * wn;
        if (flag[i] & FS_MARCH_DIRICHLET) {
            un = fi * sg1;
            wn = (un - ui) * c.idt;
        }
        u[i] = un;
        w[i] = wn;
    }
}

// ---- one step ----------------------------------------------------------------------------------------------------------------
// part: this step's [2][gridDim.x] partials; trace: this step's [n_rec] samples (nullptr: none wanted)
__global__ void __launch_bounds__(FS_BLOCK) k_dynx_update(int64_t n, const double* __restrict__ y, double* __restrict__ u, double* __restrict__ w,
                                                          const double* __restrict__ m, const double* __restrict__ load,
                                                          const uint8_t* __restrict__ flag, dynx_consts c, double sf, double sg, int n_rec,
                                                          const int32_t* __restrict__ rec, double* __restrict__ trace,
                                                          double* __restrict__ part) {
    __shared__ double lds4[4];
    double ek = 0.0, ep = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double yi = y[i], ui = u[i], wi = w[i], mi = m[i], fi = load[i];
        const uint8_t fl = flag[i];
        double wn = c.c1 * wi + c.c2 * ((sf * fi - yi) / mi);
        double un = ui + c.dt * wn;
        if (fl & FS_MARCH_DIRICHLET) {
            un = fi * sg;
            wn = (un - ui) * c.idt;
        }
        u[i] = un;
        w[i] = wn;
        ek += 0.5 * mi * wn * wn;
        ep += 0.5 * un * yi;
        fs_march_sample(fl, i, un, n_rec, rec, trace);
    }
    fs_march_store_partials(ek, ep, lds4, part);
}

// ---- the full-step velocity and acceleration of the state's time point ------------------------------------------------------------
__global__ void __launch_bounds__(FS_BLOCK) k_dynx_full_step(int64_t n, const double* __restrict__ y, const double* __restrict__ w,
                                                             const double* __restrict__ m, const double* __restrict__ load,
                                                             const uint8_t* __restrict__ flag, dynx_consts c, double sf,
                                                             double* __restrict__ v, double* __restrict__ a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double wi = w[i];
        const double wp = c.c1 * wi + c.c2 * ((sf * load[i] - y[i]) / m[i]);
        const bool dir = flag[i] & FS_MARCH_DIRICHLET;
        v[i] = dir ? wi : 0.5 * (wi + wp);
        a[i] = dir ? 0.0 : (wp - wi) * c.idt;
    }
}

// ---- host side: the state object ---------------------------------------------------------------------------------------------
static int dynx_space_ok(const fs_space_s* sp, const char* who) {
    FS_REQUIRE(sp, "%s: null space", who);
    FS_REQUIRE(!fs_is_dg(sp), "%s: not built for DG spaces (vector CG1 spaces only)", who);
    const fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(sp->degree == 1 && sp->ncomp == m->tdim && sp->ncomp >= 2, "%s: vector CG1 spaces on tetrahedra or triangles only (this "
               "space: CG%d with %d component(s) on a %d-D mesh; a row-sum lumped P2 mass is not positive)", who, sp->degree, sp->ncomp,
               m->tdim);
    return fs_march_one_rank(sp, who);
}

extern "C" int fs_dyn_explicit_state_create(fs_space_t space, fs_dyn_explicit_state_t* out) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(out, "fs_dyn_explicit_state_create: null pointer");
    FS_CHECK(dynx_space_ok(space, "fs_dyn_explicit_state_create"));
    fs_dyn_explicit_state_s* st = new fs_dyn_explicit_state_s();
    st->space = space;
    hipStream_t s = fs_rt().stream;
    int rc = st->alloc_rows(space->n_dofs_owned, s);
    for (dbuf<double>* b : {&st->u, &st->w, &st->y, &st->m, &st->t0, &st->t1})
        if (rc == FS_OK && (rc = b->alloc(st->n)) == FS_OK) rc = b->zero(s);
    if (rc == FS_OK) rc = st->alloc_part();
    return fs_march_create_finish("fs_dyn_explicit_state_create", st, rc, s, out);
}

extern "C" int fs_dyn_explicit_state_destroy(fs_dyn_explicit_state_t st) {
    delete st;
    return FS_OK;
}

extern "C" int fs_dyn_explicit_state_configure(fs_dyn_explicit_state_t st, double dt, double eta_m, const double* mass, const double* load,
                                               int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values) {
    FS_REQUIRE(st && mass, "fs_dyn_explicit_state_configure: null pointer");
    FS_REQUIRE(dt > 0.0 && isfinite(dt), "fs_dyn_explicit_state_configure: the step length is %g: dt > 0 and finite is required", dt);
    FS_REQUIRE(eta_m >= 0.0 && isfinite(eta_m), "fs_dyn_explicit_state_configure: the mass damping eta_M is %g: it must be >= 0 and finite",
               eta_m);
    const int64_t n = st->n;
    FS_CHECK(fs_march_rows_ok("fs_dyn_explicit_state_configure", n, mass, nullptr, load, n_dirichlet, dirichlet_dofs, dirichlet_values));
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->configure("fs_dyn_explicit_state_configure", load, n_dirichlet, dirichlet_dofs, dirichlet_values, s));
    FS_CHECK(st->m.upload(mass, n, s));
    FS_HIP(hipStreamSynchronize(s));
    const double alpha = 0.5 * eta_m * dt;
    st->c.dt = dt;
    st->c.idt = 1.0 / dt;
    st->c.c1 = (1.0 - alpha) / (1.0 + alpha);
    st->c.c2 = dt / (1.0 + alpha);
    st->c.etam = eta_m;
    st->configured = true;
    return FS_OK;
}

extern "C" int fs_dyn_explicit_state_set(fs_dyn_explicit_state_t st, const double* u, const double* w, int64_t step) {
    FS_REQUIRE(st && u && w, "fs_dyn_explicit_state_set: null pointer");
    FS_REQUIRE(step >= 1, "fs_dyn_explicit_state_set: the step counter is %lld: (u_n, v_{n-1/2}) needs n >= 1", (long long)step);
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->u.upload(u, st->n, s));
    FS_CHECK(st->w.upload(w, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    st->step = step;
    return FS_OK;
}

extern "C" int fs_dyn_explicit_state_get(fs_dyn_explicit_state_t st, double* u, double* w, int64_t* step) {
    FS_REQUIRE(st, "fs_dyn_explicit_state_get: null pointer");
    hipStream_t s = fs_rt().stream;
    if (u) FS_CHECK(st->u.download(u, st->n, s));
    if (w) FS_CHECK(st->w.download(w, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    if (step) *step = st->step;
    return FS_OK;
}

extern "C" int fs_dyn_explicit_state_get_work(fs_dyn_explicit_state_t st, double* y) {
    FS_REQUIRE(st && y, "fs_dyn_explicit_state_get_work: null pointer");
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->y.download(y, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

static int dynx_matrix_ok(const fs_matrix_s* K, const fs_dyn_explicit_state_s* st, const char* who) {
    FS_REQUIRE(K && st, "%s: null pointer", who);
    FS_REQUIRE(!fs_is_dg(K->space), "%s: not built for DG matrices", who);
    FS_REQUIRE(K->space == st->space && K->bs == st->space->ncomp, "%s: the state belongs to another space than the matrix", who);
    FS_CHECK(dynx_space_ok(st->space, who));
    FS_REQUIRE(st->configured, "%s: the state was not configured (fs_dyn_explicit_state_configure)", who);
    return FS_OK;
}

extern "C" int fs_dyn_explicit_start(fs_matrix_t K, fs_dyn_explicit_state_t st, const double* u0, const double* v0, double load_scale0,
                                     double dirichlet_scale0, double dirichlet_scale1) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(dynx_matrix_ok(K, st, "fs_dyn_explicit_start"));
    FS_REQUIRE(u0 && v0, "fs_dyn_explicit_start: null pointer");
    FS_REQUIRE(isfinite(load_scale0) && isfinite(dirichlet_scale0) && isfinite(dirichlet_scale1), "fs_dyn_explicit_start: a time factor is "
               "not finite");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    const int g = fs_march_grid(n);
    FS_CHECK(st->u.upload(u0, n, s));
    FS_CHECK(st->t0.upload(v0, n, s));
    st->step = 0;
    hipLaunchKernelGGL(k_dynx_dirichlet, dim3(g), dim3(FS_BLOCK), 0, s, n, st->load.p, st->flag.p, dirichlet_scale0, st->u.p);
    FS_KERNEL_CHECK();
    FS_CHECK(fs_spmv_prepare(K, s));
    FS_CHECK(fs_spmv_dev(K, st->u.p, st->y.p, s));
    FS_KERNEL_CHECK();
    hipLaunchKernelGGL(k_dynx_start, dim3(g), dim3(FS_BLOCK), 0, s, n, st->y.p, st->t0.p, st->m.p, st->load.p, st->flag.p, st->c, load_scale0,
                       dirichlet_scale1, st->u.p, st->w.p);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    st->step = 1;
    return FS_OK;
}

extern "C" int fs_dyn_explicit_advance(fs_matrix_t K, fs_dyn_explicit_state_t st, int64_t n_steps, const double* load_scale,
                                       const double* dirichlet_scale, int64_t n_receivers, const int32_t* receiver_dofs, double* traces,
                                       double* energy, fs_dyn_explicit_info* info) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(dynx_matrix_ok(K, st, "fs_dyn_explicit_advance"));
    FS_REQUIRE(st->step >= 1, "fs_dyn_explicit_advance: the state holds no (u_n, v_{n-1/2}) yet (fs_dyn_explicit_start or "
               "fs_dyn_explicit_state_set)");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    const int g = fs_march_grid(n);
    auto enqueue = [&](int64_t k, double* trace, double* part) {
        FS_CHECK(fs_spmv_dev(K, st->u.p, st->y.p, s));
        hipLaunchKernelGGL(k_dynx_update, dim3(g), dim3(FS_BLOCK), 0, s, n, st->y.p, st->u.p, st->w.p, st->m.p, st->load.p, st->flag.p, st->c,
                           load_scale[k], dirichlet_scale[k], (int)n_receivers, st->rec.p, trace, part);
        ++st->step;
        return (int)FS_OK;
    };
    return fs_march_advance("fs_dyn_explicit_advance", K, st, true, n_steps, load_scale, dirichlet_scale, n_receivers, receiver_dofs, traces,
                            energy, info, enqueue);
}

extern "C" int fs_dyn_explicit_full_step(fs_matrix_t K, fs_dyn_explicit_state_t st, double load_scale_n, double* v_out, double* a_out) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(dynx_matrix_ok(K, st, "fs_dyn_explicit_full_step"));
    FS_REQUIRE(st->step >= 1, "fs_dyn_explicit_full_step: the state holds no (u_n, v_{n-1/2}) yet (fs_dyn_explicit_start or "
               "fs_dyn_explicit_state_set)");
    FS_REQUIRE(isfinite(load_scale_n), "fs_dyn_explicit_full_step: the load factor is not finite");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    FS_CHECK(fs_spmv_prepare(K, s));
    FS_CHECK(fs_spmv_dev(K, st->u.p, st->y.p, s));
    FS_KERNEL_CHECK();
    hipLaunchKernelGGL(k_dynx_full_step, dim3(fs_march_grid(n)), dim3(FS_BLOCK), 0, s, n, st->y.p, st->w.p, st->m.p, st->load.p, st->flag.p, st->c,
                       load_scale_n, st->t0.p, st->t1.p);
    FS_KERNEL_CHECK();
    if (v_out) FS_CHECK(st->t0.download(v_out, n, s));
    if (a_out) FS_CHECK(st->t1.download(a_out, n, s));
    FS_HIP(hipStreamSynchronize(s));
    FS_KERNEL_CHECK();
    return FS_OK;
}
