// Explicit structural dynamics on vector CG1 spaces (tetrahedra, triangles in plane strain): the central-difference marcher of
// ElastodynamicsSolver ('scheme': 'explicit'), on the device.
//
// The reference has no transient structural solver; the model is the textbook one: M a + C v + K u = s_f(t) F with the isotropic
// elasticity operator K, the LUMPED mass m = M 1 (the row sums of the consistent mass, > 0 on CG1) and mass-proportional damping
// C = eta_M diag(m), marched by central differences in the leapfrog form of fs_leapfrog.h - the formulas of the step, of the start
// and of the Dirichlet rows, the constants and the per-row helpers are there - with y_n = K u_n.  The discrete energy of the step is
//   E_kin = 1/2 sum_i m_i w_{n+1/2,i}^2,   E_pot = 1/2 u_{n+1}^T y_n,
// and with F = 0 and fixed Dirichlet values E_{n+1/2} - E_{n-1/2} = -eta_M dt v_n^T diag(m) v_n with v_n = (w_{n-1/2} + w_{n+1/2}) / 2.
// A step is NOT a solve: one product with K - the library's own, through the dispatch of fs_spmv (fs_spmv_dev), so box
// and dictionary operators keep their fast products - and one pass over the rows.  fs_dyn_explicit_advance enqueues any number of
// steps back to back; the host touches nothing in between (the time factors of a step travel as kernel arguments).
//
// Kernels (no floating-point atomics: a march gives the same bits however it is split into calls):
//   k_dynx_update   one thread per row, grid-stride over a launch geometry that depends on the number of rows only, 8-byte loads
//       that a wave coalesces into full lines: the update formula, the Dirichlet rows, the receiver samples and the per-workgroup
//       partials of both energy halves.  Per row it reads y, u, w, m, F (8 B each) and one flag byte and writes u and w in place
//       (a row is read and written by its own thread only): 57 B.  A non-finite u makes the next y and with it w and E_kin
//       non-finite, so the finishing pass's check of the energy is also the check of the fields.
//   k_leapfrog_dirichlet (fs_leapfrog.h) / k_dynx_start   the Dirichlet rows of u_0, then the first step from (u_0, v_0).
//   k_dynx_full_step   v_n and a_n of the state's time point from (w_{n-1/2}, y_n): w+ is recomputed, nothing is stored.
// The row table (load, flags, receivers), the finishing pass and the batch driver: fs_march.h.  The state object and the checks the
// two leapfrog marchers share: fs_leapfrog.h.
#include "fs_leapfrog.h"
#include <mutex>

struct fs_dyn_explicit_state_s : fs_leapfrog_state {
    dbuf<double> u;                      // u_n: updated in place
    dbuf<double> y;                      // K u of the last product
    fs_dyn_explicit_state_s() : fs_leapfrog_state("fs_dyn_explicit") {}
};

// ---- the start -------------------------------------------------------------------------------------------------------------
// u: u_0 in, u_1 out; w: w_{1/2} out
__global__ void __launch_bounds__(FS_BLOCK) k_dynx_start(int64_t n, const double* __restrict__ y, const double* __restrict__ v0,
                                                         const double* __restrict__ m, const double* __restrict__ load,
                                                         const uint8_t* __restrict__ flag, fs_leapfrog_consts c, double sf, double sg1,
                                                         double* __restrict__ u, double* __restrict__ w) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double fi = load[i], vi = v0[i], ui = u[i];
        const fs_leapfrog_row r = fs_leapfrog_start_row(c, ui, vi, y[i], m[i], fi, sf, sg1, flag[i] & FS_MARCH_DIRICHLET);
        u[i] = r.u;
        w[i] = r.w;
    }
}

// ---- one step ----------------------------------------------------------------------------------------------------------------
// part: this step's [2][gridDim.x] partials; trace: this step's [n_rec] samples (nullptr: none wanted)
__global__ void __launch_bounds__(FS_BLOCK) k_dynx_update(int64_t n, const double* __restrict__ y, double* __restrict__ u, double* __restrict__ w,
                                                          const double* __restrict__ m, const double* __restrict__ load,
                                                          const uint8_t* __restrict__ flag, fs_leapfrog_consts c, double sf, double sg,
                                                          int n_rec, const int32_t* __restrict__ rec, double* __restrict__ trace,
                                                          double* __restrict__ part) {
    __shared__ double lds4[4];
    double ek = 0.0, ep = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double yi = y[i], mi = m[i];
        const uint8_t fl = flag[i];
        const fs_leapfrog_row r = fs_leapfrog_step_row(c, u[i], w[i], yi, mi, load[i], sf, sg, fl & FS_MARCH_DIRICHLET);
        u[i] = r.u;
        w[i] = r.w;
        ek += fs_leapfrog_ekin(mi, r.w);
        ep += 0.5 * r.u * yi;
        fs_march_sample(fl, i, r.u, n_rec, rec, trace);
    }
    fs_march_store_partials(ek, ep, lds4, part);
}

// ---- the full-step velocity and acceleration of the state's time point ------------------------------------------------------------
__global__ void __launch_bounds__(FS_BLOCK) k_dynx_full_step(int64_t n, const double* __restrict__ y, const double* __restrict__ w,
                                                             const double* __restrict__ m, const double* __restrict__ load,
                                                             const uint8_t* __restrict__ flag, fs_leapfrog_consts c, double sf,
                                                             double* __restrict__ v, double* __restrict__ a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double wi = w[i];
        const double wp = fs_leapfrog_w(c, wi, y[i], m[i], load[i], sf);
        const bool dir = flag[i] & FS_MARCH_DIRICHLET;
        v[i] = fs_leapfrog_v(wi, wp, dir);
        a[i] = fs_leapfrog_a(c, wi, wp, dir);
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
    return fs_march_create_finish("fs_dyn_explicit_state_create", st, st->alloc(space->n_dofs_owned, {&st->u, &st->y}, s), s, out);
}

extern "C" int fs_dyn_explicit_state_destroy(fs_dyn_explicit_state_t st) {
    delete st;
    return FS_OK;
}

extern "C" int fs_dyn_explicit_state_configure(fs_dyn_explicit_state_t st, double dt, double eta_m, const double* mass, const double* load,
                                               int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values) {
    FS_REQUIRE(st, "fs_dyn_explicit_state_configure: null pointer");
    return st->configure("fs_dyn_explicit_state_configure", dt, eta_m, mass, load, n_dirichlet, dirichlet_dofs, dirichlet_values);
}

extern "C" int fs_dyn_explicit_state_set(fs_dyn_explicit_state_t st, const double* u, const double* w, int64_t step) {
    FS_REQUIRE(st, "fs_dyn_explicit_state_set: null pointer");
    return st->set("fs_dyn_explicit_state_set", st->u, u, w, step);
}

extern "C" int fs_dyn_explicit_state_get(fs_dyn_explicit_state_t st, double* u, double* w, int64_t* step) {
    FS_REQUIRE(st, "fs_dyn_explicit_state_get: null pointer");
    return st->get(st->u, u, w, step);
}

extern "C" int fs_dyn_explicit_state_get_work(fs_dyn_explicit_state_t st, double* y) {
    FS_REQUIRE(st && y, "fs_dyn_explicit_state_get_work: null pointer");
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->y.download(y, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// started: the call needs (u_n, v_{n-1/2})
static int dynx_ready(const fs_matrix_s* K, const fs_dyn_explicit_state_s* st, const char* who, bool started) {
    FS_REQUIRE(K && st, "%s: null pointer", who);
    FS_REQUIRE(!fs_is_dg(K->space), "%s: not built for DG matrices", who);
    FS_REQUIRE(K->space == st->space && K->bs == st->space->ncomp, "%s: the state belongs to another space than the matrix", who);
    FS_CHECK(dynx_space_ok(st->space, who));
    return st->ready(who, started);
}

extern "C" int fs_dyn_explicit_start(fs_matrix_t K, fs_dyn_explicit_state_t st, const double* u0, const double* v0, double load_scale0,
                                     double dirichlet_scale0, double dirichlet_scale1) {
    const char* who = "fs_dyn_explicit_start";
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(dynx_ready(K, st, who, false));
    FS_CHECK(st->start_ok(who, u0, v0, load_scale0, dirichlet_scale0, dirichlet_scale1));
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    FS_CHECK(st->start_fields(st->u, u0, v0, dirichlet_scale0, s));
    FS_CHECK(fs_spmv_prepare(K, s));
    FS_CHECK(fs_spmv_dev(K, st->u.p, st->y.p, s));
    FS_KERNEL_CHECK();
    hipLaunchKernelGGL(k_dynx_start, dim3(fs_march_grid(n)), dim3(FS_BLOCK), 0, s, n, st->y.p, st->t0.p, st->m.p, st->load.p, st->flag.p, st->c,
                       load_scale0, dirichlet_scale1, st->u.p, st->w.p);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    st->step = 1;
    return FS_OK;
}

extern "C" int fs_dyn_explicit_advance(fs_matrix_t K, fs_dyn_explicit_state_t st, int64_t n_steps, const double* load_scale,
                                       const double* dirichlet_scale, int64_t n_receivers, const int32_t* receiver_dofs, double* traces,
                                       double* energy, fs_dyn_explicit_info* info) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(dynx_ready(K, st, "fs_dyn_explicit_advance", true));
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
    FS_CHECK(dynx_ready(K, st, "fs_dyn_explicit_full_step", true));
    FS_REQUIRE(isfinite(load_scale_n), "fs_dyn_explicit_full_step: the load factor is not finite");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    FS_CHECK(fs_spmv_prepare(K, s));
    FS_CHECK(fs_spmv_dev(K, st->u.p, st->y.p, s));
    FS_KERNEL_CHECK();
    hipLaunchKernelGGL(k_dynx_full_step, dim3(fs_march_grid(n)), dim3(FS_BLOCK), 0, s, n, st->y.p, st->w.p, st->m.p, st->load.p, st->flag.p, st->c,
                       load_scale_n, st->t0.p, st->t1.p);
    FS_KERNEL_CHECK();
    return st->full_step_out(v_out, a_out, s);
}
