// Explicit scalar wave propagation on scalar CG1 spaces (tetrahedra, triangles): the time marcher of WaveSolver, on the device.
//
// The reference lists "wave propagation" among its solvers under development (Readme.md) and never delivers one; the model is the
// textbook one: u_tt = div(c^2 grad u) + f, central differences in time, lumped mass.  With the assembled stiffness K (coefficient
// c^2), the lumped mass m_i = int phi_i dx, the lumped first-order absorbing boundary d_i = sum_F c |F| / dim, the load F scaled in
// time by s_f and the Dirichlet values g scaled by s_g, a step n -> n+1 is, with y = K u^n,
//   (m/dt^2 + d/(2 dt)) u^{n+1} = s_f[n] F - y + (2 m/dt^2) u^n - (m/dt^2 - d/(2 dt)) u^{n-1},   u^{n+1}_i = g_i s_g[n+1] on Dirichlet rows,
// and the march starts with a^0 = (s_f[0] F - K u^0 - d v^0) / m, u^1 = u^0 + dt v^0 + dt^2/2 a^0.  The discrete energy of the step is
//   E_kin = 1/2 sum_i m_i ((u^{n+1} - u^n)_i / dt)^2,   E_pot = 1/2 (u^{n+1})^T y.
// A step is therefore NOT a solve: one product with K - the library's own, through the dispatch of fs_spmv (fs_spmv_dev) - and one
// pass over the rows.  fs_wave_advance enqueues any number of steps back to back; the host touches nothing in between (the time
// factors of a step travel as kernel arguments).
//
// Kernels (no floating-point atomics: a march gives the same bits however it is split into calls):
//   k_wave_update   one thread per row, grid-stride over a launch geometry that depends on the number of rows only: the update
//       formula, the Dirichlet rows, the receiver samples and the per-workgroup partials of both energy halves.  Per row it reads y,
//       u^n, u^{n-1}, m, d, F (8 B each) and one flag byte and writes u^{n+1}: 57 B.  A non-finite field value makes
//       m_i ((u^{n+1} - u^n)_i / dt)^2 and with it E_kin non-finite, so the finishing pass's check of the energy is also the check
//       of the field.
//   k_wave_start    the first step from (u^0, v^0).
// The row table (load, flags, receivers), the finishing pass, the batch driver and the shared checks: fs_march.h.
#include "fs_march.h"
#include <mutex>

struct fs_wave_state_s : fs_march_batch_state {
    double dt = 0.0;
    dbuf<double> up, u, w;               // u^{n-1}, u^n, work: rotated by pointer
    dbuf<double> y;                      // K u^n
    dbuf<double> m, d;                   // lumped mass, lumped damping
};

// ---- the first step --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FS_BLOCK) k_wave_start(int64_t n, const double* __restrict__ y, const double* __restrict__ u0,
                                                         const double* __restrict__ v0, const double* __restrict__ m,
                                                         const double* __restrict__ d, const double* __restrict__ load,
                                                         const uint8_t* __restrict__ flag, double dt, double sf, double sg,
                                                         double* __restrict__ u1) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double fi = load[i], vi = v0[i];
        const double a0 = (sf * fi - y[i] - d[i] * vi) / m[i];
        double un = u0[i] + dt * vi + (0.5 * dt * dt) * a0;
        if (flag[i] & FS_MARCH_DIRICHLET) un = fi * sg;
        u1[i] = un;
    }
}

// ---- one step ----------------------------------------------------------------------------------------------------------------
// part: this step's [2][gridDim.x] partials; trace: this step's [n_rec] samples (nullptr: none wanted)
__global__ void __launch_bounds__(FS_BLOCK) k_wave_update(int64_t n, const double* __restrict__ y, const double* __restrict__ u,
                                                          const double* __restrict__ up, const double* __restrict__ m,
                                                          const double* __restrict__ d, const double* __restrict__ load,
                                                          const uint8_t* __restrict__ flag, double idt, double idt2, double hidt,
                                                          double sf, double sg, double* __restrict__ unew, int n_rec,
                                                          const int32_t* __restrict__ rec, double* __restrict__ trace,
                                                          double* __restrict__ part) {
    __shared__ double lds4[4];
    double ek = 0.0, ep = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double yi = y[i], ui = u[i], upi = up[i], mi = m[i], di = d[i], fi = load[i];
        const uint8_t fl = flag[i];
        const double a = mi * idt2, b = di * hidt;
        double un = (sf * fi - yi + 2.0 * a * ui - (a - b) * upi) / (a + b);
        if (fl & FS_MARCH_DIRICHLET) un = fi * sg;
        unew[i] = un;
        const double vel = (un - ui) * idt;
        ek += 0.5 * mi * vel * vel;
        ep += 0.5 * un * yi;
        fs_march_sample(fl, i, un, n_rec, rec, trace);
    }
    fs_march_store_partials(ek, ep, lds4, part);
}

// ---- host side: the state object ---------------------------------------------------------------------------------------------
static int wave_space_ok(const fs_space_s* sp, const char* who) {
    FS_REFUSE_DG_SPACE(sp, who);
    FS_REQUIRE(sp, "%s: null space", who);
    const fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(sp->degree == 1 && sp->ncomp == 1, "%s: scalar CG1 spaces on tetrahedra or triangles only (this space: CG%d with %d components "
               "on a %d-D mesh)", who, sp->degree, sp->ncomp, m->tdim);
    return fs_march_one_rank(sp, who);
}

extern "C" int fs_wave_state_create(fs_space_t space, fs_wave_state_t* out) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(out, "fs_wave_state_create: null pointer");
    FS_CHECK(wave_space_ok(space, "fs_wave_state_create"));
    fs_wave_state_s* st = new fs_wave_state_s();
    st->space = space;
    hipStream_t s = fs_rt().stream;
    int rc = st->alloc_rows(space->n_dofs_owned, s);
    for (dbuf<double>* b : {&st->up, &st->u, &st->w, &st->y, &st->m, &st->d})
        if (rc == FS_OK && (rc = b->alloc(st->n)) == FS_OK) rc = b->zero(s);
    if (rc == FS_OK) rc = st->alloc_part();
    return fs_march_create_finish("fs_wave_state_create", st, rc, s, out);
}

extern "C" int fs_wave_state_destroy(fs_wave_state_t st) {
    delete st;
    return FS_OK;
}

extern "C" int fs_wave_state_configure(fs_wave_state_t st, double dt, const double* mass, const double* damping, const double* load,
                                       int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values) {
    FS_REQUIRE(st && mass, "fs_wave_state_configure: null pointer");
    FS_REQUIRE(dt > 0.0 && isfinite(dt), "fs_wave_state_configure: the step length is %g: dt > 0 and finite is required", dt);
    const int64_t n = st->n;
    FS_CHECK(fs_march_rows_ok("fs_wave_state_configure", n, mass, damping, load, n_dirichlet, dirichlet_dofs, dirichlet_values));
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->configure("fs_wave_state_configure", load, n_dirichlet, dirichlet_dofs, dirichlet_values, s));
    FS_CHECK(st->m.upload(mass, n, s));
    if (damping) FS_CHECK(st->d.upload(damping, n, s));
    else FS_CHECK(st->d.zero(s));
    FS_HIP(hipStreamSynchronize(s));
    st->dt = dt;
    st->configured = true;
    return FS_OK;
}

extern "C" int fs_wave_state_set(fs_wave_state_t st, const double* u_prev, const double* u, int64_t step) {
    FS_REQUIRE(st && u_prev && u, "fs_wave_state_set: null pointer");
    FS_REQUIRE(step >= 1, "fs_wave_state_set: the step counter is %lld: (u^{n-1}, u^n) needs n >= 1", (long long)step);
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->up.upload(u_prev, st->n, s));
    FS_CHECK(st->u.upload(u, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    st->step = step;
    return FS_OK;
}

extern "C" int fs_wave_state_get(fs_wave_state_t st, double* u_prev, double* u, int64_t* step) {
    FS_REQUIRE(st, "fs_wave_state_get: null pointer");
    hipStream_t s = fs_rt().stream;
    if (u_prev) FS_CHECK(st->up.download(u_prev, st->n, s));
    if (u) FS_CHECK(st->u.download(u, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    if (step) *step = st->step;
    return FS_OK;
}

static int wave_matrix_ok(const fs_matrix_s* K, const fs_wave_state_s* st, const char* who) {
    FS_REQUIRE(K && st, "%s: null pointer", who);
    FS_REFUSE_DG(K, who);
    FS_REQUIRE(K->space == st->space && K->bs == 1, "%s: the state belongs to another space than the matrix", who);
    FS_CHECK(wave_space_ok(K->space, who));
    FS_REQUIRE(st->configured, "%s: the state was not configured (fs_wave_state_configure)", who);
    return FS_OK;
}

extern "C" int fs_wave_start(fs_matrix_t K, fs_wave_state_t st, const double* u0, const double* v0, double load_scale0, double dirichlet_scale1) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(wave_matrix_ok(K, st, "fs_wave_start"));
    FS_REQUIRE(u0 && v0, "fs_wave_start: null pointer");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    FS_CHECK(st->up.upload(u0, n, s));
    FS_CHECK(st->w.upload(v0, n, s));
    FS_CHECK(fs_spmv_prepare(K, s));
    FS_CHECK(fs_spmv_dev(K, st->up.p, st->y.p, s));
    FS_KERNEL_CHECK();
    hipLaunchKernelGGL(k_wave_start, dim3(fs_march_grid(n)), dim3(FS_BLOCK), 0, s, n, st->y.p, st->up.p, st->w.p, st->m.p, st->d.p, st->load.p,
                       st->flag.p, st->dt, load_scale0, dirichlet_scale1, st->u.p);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    st->step = 1;
    return FS_OK;
}

extern "C" int fs_wave_advance(fs_matrix_t K, fs_wave_state_t st, int64_t n_steps, const double* load_scale, const double* dirichlet_scale,
                               int64_t n_receivers, const int32_t* receiver_dofs, double* traces, double* energy, fs_wave_info* info) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(wave_matrix_ok(K, st, "fs_wave_advance"));
    FS_REQUIRE(st->step >= 1, "fs_wave_advance: the state holds no (u^{n-1}, u^n) yet (fs_wave_start or fs_wave_state_set)");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    const int g = fs_march_grid(n);
    const double dt = st->dt, idt = 1.0 / dt, idt2 = 1.0 / (dt * dt), hidt = 1.0 / (2.0 * dt);
    auto enqueue = [&](int64_t k, double* trace, double* part) {
        FS_CHECK(fs_spmv_dev(K, st->u.p, st->y.p, s));
        hipLaunchKernelGGL(k_wave_update, dim3(g), dim3(FS_BLOCK), 0, s, n, st->y.p, st->u.p, st->up.p, st->m.p, st->d.p, st->load.p, st->flag.p,
                           idt, idt2, hidt, load_scale[k], dirichlet_scale[k], st->w.p, (int)n_receivers, st->rec.p, trace, part);
        // (u^{n-1}, u^n, work) <- (u^n, u^{n+1}, u^{n-1})
        st->up.swap(st->u);
        st->u.swap(st->w);
        ++st->step;
        return (int)FS_OK;
    };
    return fs_march_advance("fs_wave_advance", K, st, false, n_steps, load_scale, dirichlet_scale, n_receivers, receiver_dofs, traces, energy,
                            info, enqueue);
}
