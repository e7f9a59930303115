// Implicit structural dynamics on vector CG1 / CG2 spaces (tetrahedra, triangles in plane strain): the pointwise kernels of the
// generalized-alpha marcher of ElastodynamicsSolver, on the device.
//
// The reference has no transient structural solver (its solving_dynamics branch subtracts a lagged rho * a inside a static solve);
// the model is the textbook one: M a + C v + K u = s_f(t) F with the isotropic elasticity operator K, the consistent mass M and
// Rayleigh damping C = eta_M M + eta_K K, marched by the Chung-Hulbert generalized-alpha scheme.  With x_{n+1-alpha} =
// (1 - alpha) x_{n+1} + alpha x_n the balance of a step n -> n+1 is
//   M a_{n+1-am} + C v_{n+1-af} + K u_{n+1-af} = s_f(t_n + (1 - af) dt) F
// with the Newmark updates
//   u~ = u_n + dt v_n + dt^2 (1/2 - beta) a_n        v~ = v_n + dt (1 - gamma) a_n
//   a_{n+1} = (u_{n+1} - u~) / (beta dt^2)           v_{n+1} = v~ + gamma dt a_{n+1}.
// Solved for u_{n+1} a step is ONE linear solve with the fixed operator
//   K_eff = c_M M + c_K K,   c_M = (1 - am)/(beta dt^2) + (1 - af) gamma eta_M/(beta dt),   c_K = (1 - af)(1 + gamma eta_K/(beta dt))
// and the right-hand side
//   cv  = (1 - af)(v~ - gamma/(beta dt) u~) + af v_n
//   p   = (1 - am) u~/(beta dt^2) - am a_n - eta_M cv - c_M g_ext
//   q   = -af u_n - eta_K cv - c_K g_ext
//   rhs = s_f F + M p + K q on the free rows,   rhs_i = g_i s_g(t_{n+1}) on the Dirichlet rows,
// where g_ext holds the next Dirichlet values on the Dirichlet dofs and zero elsewhere: subtracting c_M g_ext and c_K g_ext inside
// p and q IS the lifting of the Dirichlet columns of K_eff.  K and M are therefore the operators WITHOUT eliminated rows; K_eff with
// its Dirichlet rows and columns eliminated belongs to the caller, who builds it once per step length and solves with it
// (fs_amg_solve / fs_krylov_solve) between fs_dyn_predict and fs_dyn_correct.  The march starts from M a_0 = s_f(t_0) F - C v_0 -
// K u_0 on the free rows and a_0 = 0 on the Dirichlet rows: fs_dyn_start_rhs forms that right-hand side, the caller solves with the
// eliminated M, fs_dyn_start takes a_0.  Energy on request (two products): E_kin = 1/2 v^T M v, E_pot = 1/2 u^T K u.
//
// Kernels: one thread per row, grid-stride over a launch geometry that depends on the number of rows only (fs_march_grid), 8-byte loads
// that a wave coalesces into full lines; no floating-point atomics, so a march gives the same bits however it is split into calls.
// Bytes per row (fp64 fields, one flag byte):
//   k_dyn_predict   reads u, v, a and the flag, writes p, q; g only on Dirichlet rows: 24 + 1 + 16 = 41 B
//   k_dyn_rhs       reads M p, K q, F (g on a Dirichlet row, whose products are not read) and the flag, writes rhs: 24 + 1 + 8 = 33 B
//   k_dyn_correct   reads u, v, a, x and the flag, writes u, v, a (u~ and v~ are recomputed, not stored): 32 + 1 + 24 = 57 B;
//                   a Dirichlet row takes the same formulas - its u is exact.  A non-finite row is counted with integer atomics (the
//                   count and the first such step do not depend on the order).
//   k_dyn_energy / k_dyn_energy_finish   per-workgroup partials of v . M v and u . K u, summed in a fixed order by one workgroup.
// The row table (load, flags, receivers: a Dirichlet row keeps g_i in the slot of F_i) and the shared checks: fs_march.h.
#include "fs_march.h"
#include <mutex>

// what the kernels take of the scheme: everything is derived from (dt, alpha_m, alpha_f, beta, gamma, eta_M, eta_K) on the host
struct dyn_consts {
    double dt, dt2h;                     // dt, dt^2 (1/2 - beta)
    double dtg;                          // dt (1 - gamma)
    double am, af, etam, etak;
    double ibdt2;                        // 1 / (beta dt^2)
    double gbdt;                         // gamma / (beta dt)
    double gdt;                          // gamma dt
    double um;                           // (1 - am) / (beta dt^2)
    double cm, ck;                       // the coefficients of K_eff
};

struct fs_dyn_state_s : fs_march_rows, fs_march_events<6> {   // ev: predict: 0 [p, q] 1 [products] 2 [rhs] 3; correct: 4 .. 5
    fs_space_s* space = nullptr;
    bool configured = false;
    bool pending = false;                // fs_dyn_start_rhs was called, fs_dyn_start not yet
    int64_t step = -1;                   // the n of (u_n, v_n, a_n); -1: not started
    double par[7] = {};                  // dt, alpha_m, alpha_f, beta, gamma, eta_M, eta_K
    dyn_consts c = {};
    dbuf<double> u, v, a;
    dbuf<double> p, q, mp, kq;           // work: p, q, M p, K q
    dbuf<double> samples;                // [n_receivers] of the last fs_dyn_correct that wanted them
    dbuf<double> part;                   // [2][grid] energy partials, then the two sums
    dbuf<unsigned long long> bad;        // (rows found non-finite since the start, the first step that had one)
    bool timed_predict = false, timed_correct = false;
};

// ---- one step: before the solve ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FS_BLOCK) k_dyn_predict(int64_t n, const double* __restrict__ u, const double* __restrict__ v,
                                                          const double* __restrict__ a, const double* __restrict__ load,
                                                          const uint8_t* __restrict__ flag, dyn_consts c, double sg,
                                                          double* __restrict__ p, double* __restrict__ q) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double ui = u[i], vi = v[i], ai = a[i];
        const double ut = ui + c.dt * vi + c.dt2h * ai;
        const double vt = vi + c.dtg * ai;
        const double cv = (1.0 - c.af) * (vt - c.gbdt * ut) + c.af * vi;
        double pi = c.um * ut - c.am * ai - c.etam * cv;
        double qi = -c.af * ui - c.etak * cv;
        if (flag[i] & FS_MARCH_DIRICHLET) {
            const double g = load[i] * sg;
            pi -= c.cm * g;
            qi -= c.ck * g;
        }
        p[i] = pi;
        q[i] = qi;
    }
}

__global__ void __launch_bounds__(FS_BLOCK) k_dyn_rhs(int64_t n, const double* __restrict__ mp, const double* __restrict__ kq,
                                                      const double* __restrict__ load, const uint8_t* __restrict__ flag, double sf,
                                                      double sg, double* __restrict__ rhs) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double fi = load[i];
        rhs[i] = (flag[i] & FS_MARCH_DIRICHLET) ? fi * sg : sf * fi + mp[i] + kq[i];
    }
}

// ---- one step: after the solve -----------------------------------------------------------------------------------------------
// x = u_{n+1}; trace: this step's [n_rec] samples (nullptr: none wanted); bad = (non-finite rows, the first step with one)
__global__ void __launch_bounds__(FS_BLOCK) k_dyn_correct(int64_t n, double* __restrict__ u, double* __restrict__ v, double* __restrict__ a,
                                                          const double* __restrict__ x, const uint8_t* __restrict__ flag, dyn_consts c,
                                                          int n_rec, const int32_t* __restrict__ rec, double* __restrict__ trace,
                                                          unsigned long long step, unsigned long long* __restrict__ bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned int n_bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double ui = u[i], vi = v[i], ai = a[i], xi = x[i];
        const double ut = ui + c.dt * vi + c.dt2h * ai;
        const double vt = vi + c.dtg * ai;
        const double an = (xi - ut) * c.ibdt2;
        const double vn = vt + c.gdt * an;
        u[i] = xi;
        v[i] = vn;
        a[i] = an;
        if (!(isfinite(xi) && isfinite(vn) && isfinite(an))) ++n_bad;
        fs_march_sample(flag[i], i, xi, n_rec, rec, trace);
    }
    if (n_bad) {
        atomicAdd(&bad[0], (unsigned long long)n_bad);
        atomicMin(&bad[1], step);
    }
}

// ---- the start ---------------------------------------------------------------------------------------------------------------
// p = eta_M v_0, q = u_0 + eta_K v_0: M p + K q = C v_0 + K u_0
__global__ void __launch_bounds__(FS_BLOCK) k_dyn_start_pq(int64_t n, const double* __restrict__ u, const double* __restrict__ v, double etam,
                                                           double etak, double* __restrict__ p, double* __restrict__ q) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double vi = v[i];
        p[i] = etam * vi;
        q[i] = u[i] + etak * vi;
    }
}

__global__ void __launch_bounds__(FS_BLOCK) k_dyn_start_rhs(int64_t n, const double* __restrict__ mp, const double* __restrict__ kq,
                                                            const double* __restrict__ load, const uint8_t* __restrict__ flag, double sf,
                                                            double* __restrict__ rhs) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        rhs[i] = (flag[i] & FS_MARCH_DIRICHLET) ? 0.0 : sf * load[i] - mp[i] - kq[i];
}

__global__ void __launch_bounds__(FS_BLOCK) k_dyn_take_a0(int64_t n, const double* __restrict__ a0, const uint8_t* __restrict__ flag,
                                                          double* __restrict__ a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        a[i] = (flag[i] & FS_MARCH_DIRICHLET) ? 0.0 : a0[i];
}

// ---- energy ------------------------------------------------------------------------------------------------------------------
// part[0][g]: v . M v, part[1][g]: u . K u per workgroup
__global__ void __launch_bounds__(FS_BLOCK) k_dyn_energy(int64_t n, const double* __restrict__ v, const double* __restrict__ mv,
                                                         const double* __restrict__ u, const double* __restrict__ ku,
                                                         double* __restrict__ part) {
    __shared__ double lds4[4];
    double ek = 0.0, ep = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        ek += v[i] * mv[i];
        ep += u[i] * ku[i];
    }
    fs_march_store_partials(ek, ep, lds4, part);
}

// one workgroup: out = (1/2 sum part[0][.], 1/2 sum part[1][.]) in a fixed order
__global__ void __launch_bounds__(FS_BLOCK) k_dyn_energy_finish(int g, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double lds4[4];
    double ek = 0.0, ep = 0.0;
    for (int j = threadIdx.x; j < g; j += FS_BLOCK) {
        ek += part[j];
        ep += part[g + j];
    }
    const double tk = fs_block_sum(ek, lds4);
    const double tp = fs_block_sum(ep, lds4);
    if (threadIdx.x == 0) {
        out[0] = 0.5 * tk;
        out[1] = 0.5 * tp;
    }
}

// ---- host side: the state object ---------------------------------------------------------------------------------------------
static int dyn_space_ok(const fs_space_s* sp, const char* who) {
    FS_REQUIRE(sp, "%s: null space", who);
    FS_REQUIRE(!fs_is_dg(sp), "%s: not built for DG spaces (vector CG1 or CG2 spaces only)", who);
    const fs_mesh_s* m = sp->mesh;
    FS_REQUIRE((sp->degree == 1 || sp->degree == 2) && sp->ncomp == m->tdim && sp->ncomp >= 2, "%s: vector CG1 or CG2 spaces on "
               "tetrahedra or triangles only (this space: CG%d with %d component(s) on a %d-D mesh)", who, sp->degree, sp->ncomp, m->tdim);
    return fs_march_one_rank(sp, who);
}

static int dyn_clear_bad(fs_dyn_state_s* st, hipStream_t s) {
    FS_HIP(hipMemsetAsync(st->bad.p, 0, sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(st->bad.p + 1, 0xff, sizeof(unsigned long long), s));
    return FS_OK;
}

extern "C" int fs_dyn_state_create(fs_space_t space, fs_dyn_state_t* out) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(out, "fs_dyn_state_create: null pointer");
    FS_CHECK(dyn_space_ok(space, "fs_dyn_state_create"));
    fs_dyn_state_s* st = new fs_dyn_state_s();
    st->space = space;
    hipStream_t s = fs_rt().stream;
    int rc = st->alloc_rows(space->n_dofs_owned, s);
    for (dbuf<double>* b : {&st->u, &st->v, &st->a, &st->p, &st->q, &st->mp, &st->kq})
        if (rc == FS_OK && (rc = b->alloc(st->n)) == FS_OK) rc = b->zero(s);
    if (rc == FS_OK && (rc = st->part.alloc(2 * (int64_t)fs_march_grid(st->n) + 2)) == FS_OK && (rc = st->bad.alloc(2)) == FS_OK)
        rc = dyn_clear_bad(st, s);
    return fs_march_create_finish("fs_dyn_state_create", st, rc, s, out);
}

extern "C" int fs_dyn_state_destroy(fs_dyn_state_t st) {
    delete st;
    return FS_OK;
}

extern "C" int fs_dyn_state_configure(fs_dyn_state_t st, double dt, double alpha_m, double alpha_f, double beta, double gamma, double eta_m,
                                      double eta_k, const double* load, int64_t n_dirichlet, const int32_t* dirichlet_dofs,
                                      const double* dirichlet_values) {
    FS_REQUIRE(st, "fs_dyn_state_configure: null pointer");
    FS_REQUIRE(dt > 0.0 && isfinite(dt), "fs_dyn_state_configure: the step length is %g: dt > 0 and finite is required", dt);
    FS_REQUIRE(isfinite(alpha_m) && isfinite(alpha_f) && isfinite(beta) && isfinite(gamma), "fs_dyn_state_configure: the parameters "
               "(alpha_m, alpha_f, beta, gamma) = (%g, %g, %g, %g) are not finite", alpha_m, alpha_f, beta, gamma);
    FS_REQUIRE(alpha_m <= alpha_f && alpha_f <= 0.5 && beta >= 0.25 + 0.5 * (alpha_f - alpha_m), "fs_dyn_state_configure: the parameters "
               "(alpha_m, alpha_f, beta, gamma) = (%g, %g, %g, %g) are outside alpha_m <= alpha_f <= 1/2, beta >= 1/4 + (alpha_f - alpha_m)/2: "
               "the scheme is not unconditionally stable", alpha_m, alpha_f, beta, gamma);
    FS_REQUIRE(eta_m >= 0.0 && eta_k >= 0.0 && isfinite(eta_m) && isfinite(eta_k), "fs_dyn_state_configure: the Rayleigh coefficients "
               "(eta_M, eta_K) = (%g, %g) must be >= 0 and finite", eta_m, eta_k);
    FS_CHECK(fs_march_rows_ok("fs_dyn_state_configure", st->n, nullptr, nullptr, load, n_dirichlet, dirichlet_dofs, dirichlet_values));
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->configure("fs_dyn_state_configure", load, n_dirichlet, dirichlet_dofs, dirichlet_values, s));
    FS_HIP(hipStreamSynchronize(s));
    const double par[7] = {dt, alpha_m, alpha_f, beta, gamma, eta_m, eta_k};
    memcpy(st->par, par, sizeof(par));
    dyn_consts& c = st->c;
    c.dt = dt;
    c.dt2h = dt * dt * (0.5 - beta);
    c.dtg = dt * (1.0 - gamma);
    c.am = alpha_m;
    c.af = alpha_f;
    c.etam = eta_m;
    c.etak = eta_k;
    c.ibdt2 = 1.0 / (beta * dt * dt);
    c.gbdt = gamma / (beta * dt);
    c.gdt = gamma * dt;
    c.um = (1.0 - alpha_m) / (beta * dt * dt);
    c.cm = (1.0 - alpha_m) / (beta * dt * dt) + (1.0 - alpha_f) * gamma * eta_m / (beta * dt);
    c.ck = (1.0 - alpha_f) * (1.0 + gamma * eta_k / (beta * dt));
    st->configured = true;
    return FS_OK;
}

extern "C" int fs_dyn_state_set(fs_dyn_state_t st, const double* u, const double* v, const double* a, int64_t step) {
    FS_REQUIRE(st && u && v && a, "fs_dyn_state_set: null pointer");
    FS_REQUIRE(step >= 0, "fs_dyn_state_set: the step counter is %lld: n >= 0 is required", (long long)step);
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->u.upload(u, st->n, s));
    FS_CHECK(st->v.upload(v, st->n, s));
    FS_CHECK(st->a.upload(a, st->n, s));
    FS_CHECK(dyn_clear_bad(st, s));
    FS_HIP(hipStreamSynchronize(s));
    st->step = step;
    st->pending = false;
    return FS_OK;
}

extern "C" int fs_dyn_state_get(fs_dyn_state_t st, double* u, double* v, double* a, int64_t* step) {
    FS_REQUIRE(st, "fs_dyn_state_get: null pointer");
    hipStream_t s = fs_rt().stream;
    if (u) FS_CHECK(st->u.download(u, st->n, s));
    if (v) FS_CHECK(st->v.download(v, st->n, s));
    if (a) FS_CHECK(st->a.download(a, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    if (step) *step = st->step;
    return FS_OK;
}

extern "C" int fs_dyn_state_get_work(fs_dyn_state_t st, double* p, double* q, double* mp, double* kq) {
    FS_REQUIRE(st, "fs_dyn_state_get_work: null pointer");
    hipStream_t s = fs_rt().stream;
    if (p) FS_CHECK(st->p.download(p, st->n, s));
    if (q) FS_CHECK(st->q.download(q, st->n, s));
    if (mp) FS_CHECK(st->mp.download(mp, st->n, s));
    if (kq) FS_CHECK(st->kq.download(kq, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_dyn_state_info(fs_dyn_state_t st, fs_dyn_info* info) {
    FS_REQUIRE(st && info, "fs_dyn_state_info: null pointer");
    hipStream_t s = fs_rt().stream;
    unsigned long long bad_host[2] = {0, 0};
    FS_CHECK(st->bad.download(bad_host, 2, s));
    FS_HIP(hipStreamSynchronize(s));
    FS_KERNEL_CHECK();
    float ms = 0.0f, ms2 = 0.0f;
    info->predict_ms = info->predict_pointwise_ms = info->correct_ms = 0.0;
    if (st->timed_predict) {
        FS_HIP(hipEventElapsedTime(&ms, st->ev[0], st->ev[3]));
        info->predict_ms = ms;
        FS_HIP(hipEventElapsedTime(&ms, st->ev[0], st->ev[1]));
        FS_HIP(hipEventElapsedTime(&ms2, st->ev[2], st->ev[3]));
        info->predict_pointwise_ms = (double)ms + (double)ms2;
    }
    if (st->timed_correct) {
        FS_HIP(hipEventElapsedTime(&ms, st->ev[4], st->ev[5]));
        info->correct_ms = ms;
    }
    info->n_nonfinite = (int64_t)bad_host[0];
    info->first_nonfinite_step = bad_host[0] ? (int64_t)bad_host[1] : -1;
    info->step = st->step;
    return FS_OK;
}

static int dyn_matrices_ok(const fs_matrix_s* K, const fs_matrix_s* M, const fs_dyn_state_s* st, const char* who) {
    FS_REQUIRE(K && M && st, "%s: null pointer", who);
    FS_REQUIRE(!fs_is_dg(K->space) && !fs_is_dg(M->space), "%s: not built for DG matrices", who);
    FS_REQUIRE(K->space == st->space && M->space == st->space && K->bs == st->space->ncomp && M->bs == st->space->ncomp,
               "%s: the state belongs to another space than the matrices", who);
    FS_CHECK(dyn_space_ok(st->space, who));
    FS_REQUIRE(st->configured, "%s: the state was not configured (fs_dyn_state_configure)", who);
    return FS_OK;
}

// mp = M p, kq = K q through the dispatch of fs_spmv
static int dyn_products(fs_matrix_s* K, fs_matrix_s* M, fs_dyn_state_s* st, const double* p, const double* q, hipStream_t s) {
    FS_CHECK(fs_spmv_prepare(M, s));
    FS_CHECK(fs_spmv_prepare(K, s));
    FS_CHECK(fs_spmv_dev(M, p, st->mp.p, s));
    FS_CHECK(fs_spmv_dev(K, q, st->kq.p, s));
    FS_KERNEL_CHECK();
    return FS_OK;
}

extern "C" int fs_dyn_start_rhs(fs_matrix_t K, fs_matrix_t M, fs_dyn_state_t st, const double* u0, const double* v0, double load_scale0,
                                fs_vector_t rhs) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(dyn_matrices_ok(K, M, st, "fs_dyn_start_rhs"));
    FS_REQUIRE(u0 && v0 && rhs, "fs_dyn_start_rhs: null pointer");
    FS_REQUIRE(rhs->d.n >= st->n, "fs_dyn_start_rhs: the right-hand side has %lld entries, the space %lld dofs", (long long)rhs->d.n, (long long)st->n);
    FS_REQUIRE(isfinite(load_scale0), "fs_dyn_start_rhs: the load factor is not finite");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    const int g = fs_march_grid(n);
    FS_CHECK(st->u.upload(u0, n, s));
    FS_CHECK(st->v.upload(v0, n, s));
    FS_CHECK(st->a.zero(s));
    st->step = -1;
    st->pending = true;
    hipLaunchKernelGGL(k_dyn_start_pq, dim3(g), dim3(FS_BLOCK), 0, s, n, st->u.p, st->v.p, st->c.etam, st->c.etak, st->p.p, st->q.p);
    FS_KERNEL_CHECK();
    FS_CHECK(dyn_products(K, M, st, st->p.p, st->q.p, s));
    hipLaunchKernelGGL(k_dyn_start_rhs, dim3(g), dim3(FS_BLOCK), 0, s, n, st->mp.p, st->kq.p, st->load.p, st->flag.p, load_scale0, rhs->d.p);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_dyn_start(fs_dyn_state_t st, fs_vector_t a0) {
    FS_REQUIRE(st && a0, "fs_dyn_start: null pointer");
    FS_REQUIRE(st->configured, "fs_dyn_start: the state was not configured (fs_dyn_state_configure)");
    FS_REQUIRE(st->pending, "fs_dyn_start: no initial state is waiting for its acceleration (fs_dyn_start_rhs)");
    FS_REQUIRE(a0->d.n >= st->n, "fs_dyn_start: a_0 has %lld entries, the space %lld dofs", (long long)a0->d.n, (long long)st->n);
    hipStream_t s = fs_rt().stream;
    hipLaunchKernelGGL(k_dyn_take_a0, dim3(fs_march_grid(st->n)), dim3(FS_BLOCK), 0, s, st->n, a0->d.p, st->flag.p, st->a.p);
    FS_KERNEL_CHECK();
    FS_CHECK(dyn_clear_bad(st, s));
    FS_HIP(hipStreamSynchronize(s));
    st->step = 0;
    st->pending = false;
    return FS_OK;
}

extern "C" int fs_dyn_predict(fs_matrix_t K, fs_matrix_t M, fs_dyn_state_t st, double load_scale, double dirichlet_scale_next, fs_vector_t rhs) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(dyn_matrices_ok(K, M, st, "fs_dyn_predict"));
    FS_REQUIRE(st->step >= 0, "fs_dyn_predict: the state holds no (u, v, a) yet (fs_dyn_start or fs_dyn_state_set)");
    FS_REQUIRE(rhs, "fs_dyn_predict: null pointer");
    FS_REQUIRE(rhs->d.n >= st->n, "fs_dyn_predict: the right-hand side has %lld entries, the space %lld dofs", (long long)rhs->d.n, (long long)st->n);
    FS_REQUIRE(isfinite(load_scale) && isfinite(dirichlet_scale_next), "fs_dyn_predict: a time factor is not finite");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    const int g = fs_march_grid(n);
    FS_HIP(hipEventRecord(st->ev[0], s));
    hipLaunchKernelGGL(k_dyn_predict, dim3(g), dim3(FS_BLOCK), 0, s, n, st->u.p, st->v.p, st->a.p, st->load.p, st->flag.p, st->c,
                       dirichlet_scale_next, st->p.p, st->q.p);
    FS_HIP(hipEventRecord(st->ev[1], s));
    FS_CHECK(dyn_products(K, M, st, st->p.p, st->q.p, s));
    FS_HIP(hipEventRecord(st->ev[2], s));
    hipLaunchKernelGGL(k_dyn_rhs, dim3(g), dim3(FS_BLOCK), 0, s, n, st->mp.p, st->kq.p, st->load.p, st->flag.p, load_scale, dirichlet_scale_next,
                       rhs->d.p);
    FS_HIP(hipEventRecord(st->ev[3], s));
    FS_KERNEL_CHECK();
    st->timed_predict = true;
    return FS_OK;                                   // nothing returns to the host: the solve that follows is ordered on the same stream
}

extern "C" int fs_dyn_correct(fs_dyn_state_t st, fs_vector_t x, int64_t n_receivers, const int32_t* receiver_dofs, double* samples) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_REQUIRE(st && x, "fs_dyn_correct: null pointer");
    FS_REQUIRE(st->configured, "fs_dyn_correct: the state was not configured (fs_dyn_state_configure)");
    FS_REQUIRE(st->step >= 0, "fs_dyn_correct: the state holds no (u, v, a) yet (fs_dyn_start or fs_dyn_state_set)");
    FS_REQUIRE(x->d.n >= st->n, "fs_dyn_correct: the solution has %lld entries, the space %lld dofs", (long long)x->d.n, (long long)st->n);
    const int64_t n = st->n;
    FS_CHECK(fs_march_receivers_ok("fs_dyn_correct", n, n_receivers, receiver_dofs));
    const bool want = samples && n_receivers > 0;
    hipStream_t s = fs_rt().stream;
    if (want) {
        FS_CHECK(st->set_receivers(n_receivers, receiver_dofs, s));
        if (st->samples.n != n_receivers) FS_CHECK(st->samples.alloc(n_receivers));
    }
    FS_HIP(hipEventRecord(st->ev[4], s));
    hipLaunchKernelGGL(k_dyn_correct, dim3(fs_march_grid(n)), dim3(FS_BLOCK), 0, s, n, st->u.p, st->v.p, st->a.p, x->d.p, st->flag.p, st->c,
                       (int)n_receivers, st->rec.p, want ? st->samples.p : nullptr, (unsigned long long)(st->step + 1), st->bad.p);
    FS_HIP(hipEventRecord(st->ev[5], s));
    FS_KERNEL_CHECK();
    st->timed_correct = true;
    ++st->step;
    if (!want) return FS_OK;                        // nothing to hand back: the step stays in flight
    FS_CHECK(st->samples.download(samples, n_receivers, s));
    FS_HIP(hipStreamSynchronize(s));
    FS_KERNEL_CHECK();
    return FS_OK;
}

extern "C" int fs_dyn_energy(fs_matrix_t K, fs_matrix_t M, fs_dyn_state_t st, double* out) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(dyn_matrices_ok(K, M, st, "fs_dyn_energy"));
    FS_REQUIRE(st->step >= 0, "fs_dyn_energy: the state holds no (u, v, a) yet (fs_dyn_start or fs_dyn_state_set)");
    FS_REQUIRE(out, "fs_dyn_energy: null pointer");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    const int g = fs_march_grid(n);
    FS_CHECK(dyn_products(K, M, st, st->v.p, st->u.p, s));
    hipLaunchKernelGGL(k_dyn_energy, dim3(g), dim3(FS_BLOCK), 0, s, n, st->v.p, st->mp.p, st->u.p, st->kq.p, st->part.p);
    hipLaunchKernelGGL(k_dyn_energy_finish, dim3(1), dim3(FS_BLOCK), 0, s, g, st->part.p, st->part.p + 2 * g);
    FS_KERNEL_CHECK();
    FS_CHECK(fs_staged_copy(out, st->part.p + 2 * g, 2 * sizeof(double), false, s));
    FS_HIP(hipStreamSynchronize(s));
    FS_KERNEL_CHECK();
    return FS_OK;
}
