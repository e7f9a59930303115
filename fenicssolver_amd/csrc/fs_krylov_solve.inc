// Part of fs_krylov.hip (included there, one translation unit: it shares the file-scope state): the host side of fs_krylov_solve - the workspace, the plan of a solve, the state of a pass, one step
// function per iteration form, the one-launch driver, the graph cache.  fs_krylov_solve at the end reads top to bottom:
// validate -> lattice detour -> prepare -> for (;;) { begin pass; iterate; end pass; decide restart } -> un-scale -> stats.
// (DESIGN.md section 3.4.1 says which function owns which iteration form.)

// Everything a captured batch of iterations bakes in, by name.  Every member is 8 bytes wide (no padding): a key is value-initialised,
// filled and compared with memcmp; a fact that does not apply to a form stays zero.  An argument a captured launch gets and that
// can change between two solves MUST be a member here: a graph replayed with a stale argument is silent.
struct graph_key {
    // the operator and its space (heap and pool addresses are handed out again after a free: the serial numbers are the identity)
    const void *A, *aval, *sell_col;
    int64_t n, matrix_serial, space_serial;
    // the vectors of the call and of the workspace
    const void *x, *hist, *z, *w, *p, *s, *z2, *w2, *s2, *sg, *weights, *partials, *status, *ctrl, *scal, *it_ctr;
    // the row-dictionary product: class tables, items and plans, the class count and widths its launch bakes in
    const void *dict_cls, *dict_values, *dict_items, *dict_plans, *items_interior, *items_boundary;
    int64_t dict_ncls, dict_S, dict_C, n_dict_items, map_xcd;
    // the product of a lattice-ordered operator: the tables of the tile product or of k_lat_march, and the geometry
    const void* lat_tab[6];
    int64_t lat_n_tiles, lat_grid, lat_w_tiles, lm_on, lm_PY, lm_ZC;
    // the peer-to-peer exchange: buffers, the generation of the transport, the grid cap of the exchange kernel
    const void *snd_own_recv, *snd_peers, *red_own_buf, *red_peer_buf;
    int64_t p2p_on, p2p_generation, p2p_rows_cap;
    // the shape of the batch and of its launches
    int64_t bsz, box_ahead, iteration_form, igrid, fgrid, vgrid, upd_nt, spmv_nt, mirror;
};

// One batch of iterations captured as a hipGraph (same arguments every iteration: the kernels read their iteration index from the
// device).  Captured and instantiated anew when anything it bakes in changes.
struct graph_cache {
    hipGraphExec_t exec = nullptr;
    graph_key key = {};
    // one(i) -> int enqueues launch i of the batch
    template <class Launch>
    int replay(const graph_key& want, int bsz, hipStream_t s, Launch&& one) {
        if (!exec || memcmp(&want, &key, sizeof(key))) {
            if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
            hipGraph_t graph = nullptr;
            FS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            int rc_cap = FS_OK;
            for (int i = 0; i < bsz && rc_cap == FS_OK; ++i) rc_cap = one(i);
            const hipError_t e_end = hipStreamEndCapture(s, &graph);       // (a launcher that failed: the capture is ended first)
            FS_CHECK(rc_cap);
            FS_HIP(e_end);
            FS_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
            (void)hipGraphDestroy(graph);
            memcpy(&key, &want, sizeof(key));
        }
        FS_HIP(hipGraphLaunch(exec, s));
        return FS_OK;
    }
};

// persistent Krylov workspace: allocation stays out of the timed solve
struct krylov_ws {
    int64_t n = 0, nl = 0;
    int hist_cap = 0;
    dbuf<double> dinv, r, z, w, p, s, partials, sums, ctrl, scal, hist;
    dbuf<double> rhat, t, y, partials2, bsums;   // BiCGStab only (allocated on first use)
    dbuf<double> aval, dvec, bhat, sc_local;     // diagonally scaled CG only
    dbuf<double> pw, pz;                         // pipelined CG only: w = A r (with ghost room: it is the exchanged vector), z = A s
    hipEvent_t ev_upd = nullptr, ev_red = nullptr;   // pipelined CG: update done -> all-reduce on the communication stream -> sums ready
    dbuf<int> d_err;                             // zero-diagonal counter of k_extract_dinv
    int64_t bicg_n = -1;
    dbuf<int> status;
    int* h_status = nullptr;  // pinned: 2 x 4 status ints (double-buffered polls) + [8] zero-diagonal count
    int* h_mirror = nullptr;  // pinned, written by the iteration kernel's leader lane: [0] status once stopped, [1] iteration in progress
    int* d_mirror = nullptr;  // ... its device address
    bool mirror_ok = true;    // false once a wait on it timed out (stores not visible on this system): the copied status word again
    double* h_vals = nullptr; // pinned: the sums [0 .. 8) and the control block [8 .. 12) at the end of a pass
    hipEvent_t poll[2] = {nullptr, nullptr};
    static const int NSAMPLE = 64;
    hipEvent_t ev[NSAMPLE][4];
    int sample_iter[NSAMPLE];   // iteration (within its pass) a sample was taken at
    int sample_span[NSAMPLE];   // launches a sample covers (2: a LIGHT and a PAIR launch of the one-launch iteration, their mean is reported)
    bool sample_live[NSAMPLE];  // false: the sampled launches came after convergence (no-ops)
    bool events = false;
    std::vector<double> last_hist;
    dbuf<double> sg;            // s on the ghost rows, in arrival order (peer-to-peer iteration: a rank advances its ghost r, s itself)
    graph_cache cg_graph;       // a batch of the two- / three-launch iteration (run_graph_batch)
    // one-launch iteration (k_dict_cg_iter): the second set of r, w, s (double-buffered by iteration parity), the iteration
    // counters of the device, its own captured batch
    dbuf<double> z2, w2, s2;
    dbuf<int> it_ctr;
    graph_cache cgf_graph;
};
static krylov_ws g_ws;

static int ws_prepare(krylov_ws& ws, int64_t n, int64_t nl, int max_iter) {
    if (ws.n != n || ws.nl != nl) {
        // (measured and not kept: the vectors of the update set apart by 256 B ... 1 MB so that equal
        // indices fall on different memory channels - no effect; the 100 - 117 us spread of the update kernel at 10 M rows is
        // the box's, not the addresses')
        FS_CHECK(ws.dinv.alloc(n + 2));
        FS_CHECK(ws.r.alloc(n + 2));
        FS_CHECK(ws.z.alloc(nl + 2));
        FS_CHECK(ws.w.alloc(nl + 2));        // (ghost room: the one-launch iteration on a decomposed space reads w and s on ghost columns)
        FS_CHECK(ws.p.alloc(n + 2));
        FS_CHECK(ws.s.alloc(nl + 2));
        ws.n = n;
        ws.nl = nl;
    }
    if (!ws.partials.p) {
        FS_CHECK(ws.partials.alloc(4 * (FS_MAX_PARTIAL_BLOCKS + 8)));
        FS_CHECK(ws.sums.alloc(8));
        FS_CHECK(ws.ctrl.alloc(4));
        FS_CHECK(ws.scal.alloc(8));          // ([4], [5]: beta by iteration parity, k_dict_cg_iter with LIGHT / PAIR launches)
        FS_CHECK(ws.status.alloc(4));
        FS_CHECK(ws.d_err.alloc(1));
        FS_HIP(hipHostMalloc((void**)&ws.h_status, 16 * sizeof(int), hipHostMallocDefault));     // ([12 .. 16): the status word at the end of a pass)
        FS_HIP(hipHostMalloc((void**)&ws.h_vals, 16 * sizeof(double), hipHostMallocDefault));
        if (hipHostMalloc((void**)&ws.h_mirror, 16 * sizeof(int), hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void**)&ws.d_mirror, ws.h_mirror, 0) != hipSuccess) {
            (void)hipGetLastError();
            ws.h_mirror = ws.d_mirror = nullptr;
        }
        FS_HIP(hipEventCreateWithFlags(&ws.poll[0], hipEventDisableTiming));
        FS_HIP(hipEventCreateWithFlags(&ws.poll[1], hipEventDisableTiming));
        FS_HIP(hipEventCreateWithFlags(&ws.ev_upd, hipEventDisableTiming));
        FS_HIP(hipEventCreateWithFlags(&ws.ev_red, hipEventDisableTiming));
        for (int i = 0; i < krylov_ws::NSAMPLE; ++i)
            for (int j = 0; j < 4; ++j) FS_HIP(hipEventCreate(&ws.ev[i][j]));
        ws.events = true;
    }
    if (ws.hist_cap < max_iter + 2) {
        FS_CHECK(ws.hist.alloc(max_iter + 2));
        ws.hist_cap = max_iter + 2;
    }
    return FS_OK;
}

// The environment knobs of a solve, read once (by the first solve of the process).  FS_KRYLOV_DEBUG, FS_COMM_TIMING and
// FS_ITER_TIMING are diagnostics read where they print, on every call, as everywhere else in this file.
struct krylov_env {
    static bool not_zero(const char* name) { const char* v = getenv(name); return !(v && v[0] == '0'); }
    static int number(const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; }
    // FS_SOLVE_TIMING=1: wall-clock laps of the phases of a solve on stderr (each lap synchronises the stream: a diagnostic, it
    // changes what it measures; tools/probes/first_step_probe.py uses it to split the first solve of a process)
    const bool solve_timing = getenv("FS_SOLVE_TIMING") != nullptr;
    const char* const pipelined = getenv("FS_CG_PIPELINED");           // overrides opts->pipelined
    const bool lazy_scale_copy = not_zero("FS_LAZY_SCALE_COPY");
    const char* const fused = getenv("FS_CG_FUSED");                   // overrides option "cg_fused"
    const int64_t fused_max_rows = getenv("FS_CG_FUSED_MAX_ROWS") ? atoll(getenv("FS_CG_FUSED_MAX_ROWS")) : (int64_t)3000000;
    const bool fused_p2p = not_zero("FS_CG_FUSED_P2P");
    const int batch = number("FS_CG_BATCH", 0);
    // kernel durations (stats->spmv_ms / update_ms: the roofline of bench.py) are sampled with HIP events every
    // sample_every-th iteration, 4 events each.  The markers are not free: on the 1 M-DOF solve (293 iterations of 45 us)
    // sampling every 4th iteration costs 0.87 ms per solve (6 %), every 16th 0.4 ms - the default
    const int sample_every = getenv("FS_CG_SAMPLE_EVERY") ? std::max(1, atoi(getenv("FS_CG_SAMPLE_EVERY"))) : 16;
    const char* const update_nt = getenv("FS_UPDATE_NT");
    const char* const graph = getenv("FS_CG_GRAPH");                   // overrides option "cg_graph"
    const bool profiler_attached = getenv("ROCP_TOOL_LIBRARIES") != nullptr;
    const bool halo_early = not_zero("FS_HALO_EARLY");                 // 0 keeps the exchange inside the product
    const int p2p_fuse = number("FS_P2P_FUSE", 1);
    const int p2p_rows_blocks = number("FS_P2P_ROWS_BLOCKS", 128);
    const bool warm = not_zero("FS_WARM");
    const int mirror = number("FS_CG_MIRROR", -1);
};

// Everything decided before the first pass and constant afterwards (prepare_solve fills it in).
struct solve_plan {
    const krylov_env& env;
    fs_matrix_s* A;
    fs_vector_s *b, *x;
    const fs_krylov_opts* opts;
    fs_space_s* sp;
    hipStream_t s;
    int64_t n, nl;
    int bs;
    bool bicg = false, ds = false, pnorm = false, pipelined = false, fuse_sums = false, upd_nt = false;
    int batch = 0, graph_mode = 0;
    const double* aval = nullptr;           // the scaled copy of the values (ds), nullptr: the matrix's own
    int vgrid = 0, pgrid = 0;               // workgroups of the vector updates, of the plain dot products
    int sgrid = 0;                          // dot partials per product (pairs + singles, or interior + boundary on a decomposed space)
    int igrid = 0;                          // workgroups (= dot partials) of the one-launch iteration kernel
    const box_iter_plan_s* BI = nullptr;    // the one-launch iteration in marching-window form (k_box_cg_iter)
    bool fused = false;                     // one launch per iteration on one GPU
    bool fusedp_ok = false;                 // ... behind the exchange kernel on a decomposed space, where the pass uses that exchange
    bool pair_form = false, dtab_form = false, guard_form = false, centre_form = false, zruns_form = false;
    int64_t guard = 0;                      // zeros in front of and behind the six vectors of the guarded form
    std::chrono::steady_clock::time_point t_begin;
};

// The four-event protocol of a duration sample: ev[i][0] .. [1] bracket the product (the whole launch of the one-launch iteration),
// ev[i][2] .. [3] the update.
struct sampler {
    krylov_ws& ws;
    hipStream_t s;
    int n = 0;              // samples taken by this solve
    int step = 16;
    bool on = false;        // a sample is open
    // opens a sample if iteration k of the pass is due one (k < 0: a launch that is being captured) and none is open
    bool begin(int k, int span) {
        if (on || k < 0 || k % step != 1 % step || n >= krylov_ws::NSAMPLE) return false;
        ws.sample_iter[n] = k;
        ws.sample_span[n] = span;
        return on = true;
    }
    int mark(int j) {
        if (on) FS_HIP(hipEventRecord(ws.ev[n][j], s));
        return FS_OK;
    }
    int close() {
        if (!on) return FS_OK;
        FS_HIP(hipEventRecord(ws.ev[n][3], s));
        ++n;
        on = false;
        return FS_OK;
    }
    // one-launch iteration, behind a launch.  LIGHT / PAIR launches: a sample is a PAIR launch and the LIGHT launch behind it,
    // reported as their mean - avg_launch_ms stays the mean launch of the solve
    int launch_done(bool pair, bool last_of_batch) {
        if (!on) return FS_OK;
        if (++ws.sample_span[n] == 2 || !pair || last_of_batch) {
            FS_CHECK(mark(1));
            FS_CHECK(mark(2));
            FS_CHECK(close());
        }
        return FS_OK;
    }
};

// What a pass sets up and the iteration drivers share.
struct pass_state {
    sampler sm;
    // carried from pass to pass
    int total_iters = 0, n_pass = 0, n_launches = 0;
    bool use_guess = false, fusedp_used = false;
    int iteration_form = 0, iteration_runs = 0;
    int h_status[4] = {0, 0, 0, 0};
    double true_rr = 0.0, thresh = 0.0, bb_host = 0.0, prev_true_rr = 1e300;
    // set by begin_pass
    int max_iter = 0, first_sample = 0;
    double* hist_p = nullptr;
    int64_t early_a = 0, early_b = 0;      // rows sent to the neighbours: a prefix [0, early_a) and / or a suffix [early_b, n) (z-slabs)
    int p2p_fuse = 0, p2p_rows_cap = 128;
    bool p2p_ghosts_in = false;            // peer-to-peer iteration: the ghosts of the next product were received by the exchange kernel
    hipStream_t red_stream = nullptr;      // pipelined: the all-reduce of the sums runs here (nullptr: in the compute stream)
    bool graph_sized = false, graphs_allowed = false, fusedp = false, use_graph = false, mirrored = false;
    int* mirror_dev = nullptr;
    int bsz = 0, first_plain = 0;
    // progress of the pass
    int k = 0, slot = 0, pending = -1;
    bool finished = false;
    int seen = 0;
    std::chrono::steady_clock::time_point t_seen;
};

struct lap_timer {
    bool on;
    hipStream_t s;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[fs_krylov timing] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// A scalar CG2 operator on a uniform box (one GPU) is solved in LATTICE order (fs_lattice.hip): values, b and x permuted into
// the solver's shadow of the space, the solve run there (fs_krylov_solve again, on the shadow's handles), x permuted back.
// Automatic (option "lattice_order" = -1, the default): from FS_LATTICE_MIN_ROWS rows on, and only as long as the shadow's solves
// run on the tile product (a shadow whose rows do not fit the tile form - lat_prepare - is given up after its first solve).
// *taken: the solve was done here.
static int solve_in_lattice_order(fs_matrix_s* A, fs_vector_s* b, fs_vector_s* x, const fs_krylov_opts* opts, fs_krylov_stats* stats, bool* taken) {
    fs_space_s* sp = A->space;
    *taken = false;
    if (!(bs_is_scalar_cg2(A) && (g_lattice > 0 || (g_lattice < 0 && sp->n_nodes_owned >= FS_LATTICE_MIN_ROWS)) && sp->lattice_state >= 0)) return FS_OK;
    fs_lattice_shadow* L = nullptr;
    FS_CHECK(fs_lattice_get(sp, &L));
    if (!L) return FS_OK;
    *taken = true;
    const auto t0 = std::chrono::steady_clock::now();
    fs_matrix_s* A2 = nullptr;
    fs_vector_s *b2 = nullptr, *x2 = nullptr;
    FS_CHECK(fs_lattice_enter(L, A, b, x, opts->nonzero_guess != 0, &A2, &b2, &x2));
    // (the shadow matrix has ONE serial and holds another operator's values on every call: the dictionary's marker `these rows
    // do not repeat`, keyed on the serial, must not outlive the matrix it was set for - ADVICE r5)
    if (g_dict.gave_up_on == A2->serial) g_dict.gave_up_on = 0;
    g_lat.ok = false;           // (decided by THIS solve: a flag left by an earlier solve on another space says nothing, ADVICE r5)
    g_lat.judged = false;
    FS_CHECK(fs_krylov_solve(A2, b2, x2, opts, stats));
    FS_CHECK(fs_lattice_leave(L, sp, x));
    FS_HIP(hipStreamSynchronize(fs_rt().stream));
    if (g_lattice < 0 && g_lat.judged && !(g_lat.ok && g_lat.space_serial == A2->space->serial)) {
        // the shadow's rows do not fit the tile form: the space's own numbering from now on, and the shadow (a second copy of
        // the operator's structure and values: several GB at configs[3]) is given back
        sp->lattice_state = -1;
        fs_lattice_release(sp->lattice);
        sp->lattice = nullptr;
    }
    if (stats) {
        stats->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->lattice_order = 1;
    }
    return FS_OK;
}

// ---- prepare: workspace, Jacobi diagonal, threshold, scaled copy and row classes, the iteration form ------------------------

// the vectors of the method, the recurrence, the grids
static int prepare_workspace(solve_plan& P, krylov_ws& ws) {
    const fs_krylov_opts* opts = P.opts;
    fs_space_s* sp = P.sp;
    const int64_t n = P.n, nl = P.nl;
    if (sp->halo.begun) {              // left over from a solve that ended in an error
        FS_CHECK(fs_halo_end_dev(sp, fs_rt().stream));
        sp->halo.begun = false;
    }
    if (P.bicg && (ws.bicg_n != n || ws.y.n != nl + 2)) {
        FS_CHECK(ws.rhat.alloc(n + 2));
        FS_CHECK(ws.t.alloc(n + 2));
        FS_CHECK(ws.y.alloc(nl + 2));
        FS_CHECK(ws.partials2.alloc(4 * (FS_MAX_PARTIAL_BLOCKS + 8)));
        FS_CHECK(ws.bsums.alloc(16));
        ws.bicg_n = n;
    }
    P.ds = !P.bicg && opts->precond == FS_PC_JACOBI && opts->diagonal_scale != 0;
    if (P.ds) {
        if (ws.aval.n != P.A->val.n) FS_CHECK(ws.aval.alloc(P.A->val.n));
        if (ws.dvec.n != n + 2) {
            FS_CHECK(ws.dvec.alloc(n + 2));
            FS_CHECK(ws.bhat.alloc(n + 2));
        }
        if (ws.sc_local.n != nl + 2) FS_CHECK(ws.sc_local.alloc(nl + 2));
    }
    // Pipelined recurrence (k_pcg_update): only when asked for explicitly (> 0).
    const int pipe_opt = P.env.pipelined ? atoi(P.env.pipelined) : opts->pipelined;
    if (pipe_opt > 0 && !P.ds) {
        fs_set_error("fs_krylov_solve: the pipelined recurrence needs CG + Jacobi with diagonal_scale = 1");
        return FS_ERR_UNSUPPORTED;
    }
    // OPT-IN since round 4 (opts->pipelined = 1, FS_CG_PIPELINED=1): in every measurement available the recurrence lost - 69.3
    // against 57.1 us per iteration over RCCL, 58.8 against 38.0 us over the peer-to-peer exchange at 1 M rows per rank
    // (profiles/r03_p2p_self_halo_timings.txt): its 40 B/DOF of extra vector traffic and two more launches cost more than the
    // 3-double all-reduce it hides.  It would pay from an all-reduce latency of about 20 us per iteration upwards (DESIGN.md
    // section 5) - a multi-node communicator, which this library does not target.
    P.pipelined = P.ds && pipe_opt > 0;
    if (P.pipelined) {
        if (ws.pw.n != nl + 2) FS_CHECK(ws.pw.alloc(nl + 2));
        if (ws.pz.n != n + 2) FS_CHECK(ws.pz.alloc(n + 2));
    }
    P.fuse_sums = g_cg_fuse_sums && fs_rt().comm == nullptr;
    P.vgrid = fs_grid_for(n / 2 + 1, FS_BLOCK, g_update_blocks);
    P.pgrid = fs_grid_for(n, FS_BLOCK, FS_MAX_PARTIAL_BLOCKS);
    if (P.A->bs == 1 && sp->n_pairs < 0 && spmv_use_pairs(sp, 1)) FS_CHECK(build_pair_lists(sp, P.s));
    P.sgrid = spmv_partials(sp, P.A->bs);
    return FS_OK;
}

// Jacobi diagonal (the zero-diagonal counter is read back with the first status poll: no extra sync here), ||b||^2 -> threshold
static int prepare_diagonal_and_threshold(solve_plan& P, krylov_ws& ws) {
    const fs_krylov_opts* opts = P.opts;
    fs_matrix_s* A = P.A;
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    const int64_t n = P.n;
    FS_CHECK(ws.d_err.zero(s));
    const int g = fs_grid_for(sp->n_nodes_owned);
    const int jmode = P.ds ? 2 : (opts->precond == FS_PC_JACOBI ? 1 : 0);
    double* dv = P.ds ? ws.dvec.p : nullptr;
    hipLaunchKernelGGL(P.bs == 2 ? k_extract_dinv<2> : (P.bs == 1 ? k_extract_dinv<1> : k_extract_dinv<3>), dim3(g), dim3(FS_BLOCK), 0, s, sp->n_nodes_owned, sp->slice_ptr.p, sp->sell_col.p, A->val.p,
                       sp->sell_entries, jmode, ws.dinv.p, ws.d_err.p, dv);
    FS_KERNEL_CHECK();
    FS_HIP(hipMemcpyAsync(ws.h_status + 8, ws.d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    P.pnorm = opts->norm_type == FS_NORM_PRECONDITIONED;
    if (P.pnorm && !P.ds) {
        fs_set_error("fs_krylov_solve: the preconditioned residual norm needs CG + Jacobi with diagonal_scale = 1");
        return FS_ERR_UNSUPPORTED;
    }
    // ||b||^2 -> threshold.  Preconditioned norm (PETSc's KSPCG default): ||D^-1 b||^2 = sum (dinv_s^2 b)^2,
    // where ws.dinv holds 1/sqrt(d) in scaled mode, and the residual weights become 1/d instead of d.
    if (P.pnorm) {
        hipLaunchKernelGGL(k_pointwise_mul, dim3(fs_grid_for(n)), dim3(FS_BLOCK), 0, s, ws.dinv.p, ws.dinv.p, n, ws.dvec.p);  // 1/d
        hipLaunchKernelGGL(k_pointwise_mul, dim3(fs_grid_for(n)), dim3(FS_BLOCK), 0, s, ws.dvec.p, P.b->d.p, n, ws.bhat.p);  // b/d
        hipLaunchKernelGGL(k_dot_partial, dim3(P.pgrid), dim3(FS_BLOCK), 0, s, ws.bhat.p, ws.bhat.p, n, ws.partials.p);
    } else
        hipLaunchKernelGGL(k_dot_partial, dim3(P.pgrid), dim3(FS_BLOCK), 0, s, P.b->d.p, P.b->d.p, n, ws.partials.p);
    FS_CHECK(fs_comm_sum_allreduce_dev(ws.partials.p, P.pgrid, 1, ws.sums.p + 4, s));
    hipLaunchKernelGGL(k_set_threshold, dim3(1), dim3(64), 0, s, ws.sums.p + 4, opts->rtol, opts->atol, ws.ctrl.p);
    return FS_OK;
}

// diagonally scaled CG: the scaled copy of the values, bhat = D^-1/2 b, the row classes of a scalar operator
static int prepare_scaled_operator(solve_plan& P, krylov_ws& ws) {
    fs_matrix_s* A = P.A;
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    const int64_t n = P.n;
    const int bs = P.bs;
    // the scaled system needs ghost scale factors too: refresh them through the halo
    // (no halo plan: no ghost entries - the factors are read where they are)
    double* sc_local = sp->halo.active ? ws.sc_local.p : ws.dinv.p;
    if (sp->halo.active) {
        FS_HIP(hipMemcpyAsync(sc_local, ws.dinv.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        FS_CHECK(fs_halo_exchange_dev(sp, sc_local, s));
    }
    const int g2 = fs_grid_for(sp->n_slices * 64, FS_BLOCK, 8192);
    const auto scale_copy = [&]() {
        hipLaunchKernelGGL(bs == 2 ? k_scale_copy<2> : (bs == 1 ? k_scale_copy<1> : k_scale_copy<3>), dim3(g2), dim3(FS_BLOCK), 0, s, sp->n_nodes_owned, sp->n_slices, sp->slice_ptr.p, sp->sell_col.p,
                           A->val.p, sp->sell_entries, sc_local, ws.aval.p);
    };
    // scalar operator on one GPU: the scaled copy is written only if somebody is going to read it - a matrix that the kept class
    // table describes (verified on the fly-scaled values, dict_build) is multiplied from the table alone
    const bool lazy_copy = bs == 1 && !sp->halo.active && P.env.lazy_scale_copy;
    if (!lazy_copy) scale_copy();
    hipLaunchKernelGGL(k_pointwise_mul, dim3(fs_grid_for(n)), dim3(FS_BLOCK), 0, s, ws.dinv.p, P.b->d.p, n, ws.bhat.p);
    FS_KERNEL_CHECK();
    P.aval = ws.aval.p;
    if (bs == 1) {
        // a handful of distinct rows (uniform box, constant coefficient)?
        // (with the dot weights of the solve: a table of them by class for the one-launch iteration)
        if (lazy_copy) FS_CHECK(dict_build(A, P.aval, s, A->val.p, sc_local, scale_copy, ws.dvec.p));
        else FS_CHECK(dict_build(A, P.aval, s, nullptr, nullptr, nullptr, ws.dvec.p));
        P.sgrid = spmv_partials(sp, bs);          // (the row-dictionary product has its own launch geometry)
    }
    return FS_OK;
}

// Which iteration form the solve takes, and the vectors of the one-launch forms.
// One launch per iteration (k_dict_cg_iter) where the product is the row-dictionary kernel with the whole dictionary in LDS,
// on one GPU.  Automatic mode: FS_CG_FUSED_MAX_ROWS rows at most (the neighbour values of three vectors instead of one have
// to stay in the L2 of an XCD; measured crossover in DESIGN.md section 3).
static int choose_iteration_form(solve_plan& P, krylov_ws& ws) {
    fs_space_s* sp = P.sp;
    const int fused_opt = P.env.fused ? atoi(P.env.fused) : g_cg_fused;
    const bool fused_common = P.ds && !P.pipelined && P.bs == 1 && fused_opt != 0 &&
                              g_dict.bs == 1 && g_dict.built_for && g_dict.built_for == P.aval && sp->n_dict_items > 0 &&
                              (size_t)g_dict.ncls * g_dict.S * sizeof(double) <= (size_t)FS_DICT_WHOLE_LDS_BYTES &&
                              P.nl < ((int64_t)1 << 29) && sp->dict_run_len == 3 && sp->dict_runs == 8 && (fused_opt > 0 || P.n <= P.env.fused_max_rows);
    // (round 6) P1 boxes from 400 k rows on: the iteration in marching-window form (k_box_cg_iter), with its own launch geometry
    P.BI = (fused_common && !sp->halo.active && P.fuse_sums) ? box_iter_plan_for(sp, g_dict.ncls) : nullptr;
    P.igrid = fused_common ? (P.BI ? P.BI->g.grid : spmv_partials_unsplit(sp, P.bs)) : 0;
    const bool fused_sized = fused_common && 3 * (int64_t)P.igrid * 2 <= (int64_t)ws.partials.n && P.igrid <= 4 * FS_BLOCK;
    P.fused = fused_sized && P.fuse_sums && !sp->halo.active;
    // a decomposed space: the same kernel after the peer-to-peer exchange kernel (two launches per iteration instead of three) - where
    // that exchange is what the iteration uses (decided per pass: pass_state::p2p_fuse); a rank-local choice, the exchange protocol is the same
    P.fusedp_ok = fused_sized && !P.fuse_sums && sp->halo.active && P.env.fused_p2p;
    // k_dict_cg_iter: p and x every second launch (option "cg_pair"), dot weights from the class table where every row agrees with it
    P.pair_form = g_cg_pair != 0;
    P.dtab_form = P.pair_form && g_dict.dtab_ok;
    // ... and on one GPU the six vectors whose neighbour columns it reads with guard bands of zeros (option "cg_guard"): every run load of
    // every item is then inside the block (a lane reads columns first + 2 lane + start + {0, 1}, lane < 64: 130 covers the item's 128
    // values and the second value of a load; a multiple of 32 keeps row 0 on the alignment the block has), no item takes the clamped
    // path.  The bands are zeroed with the block and nothing writes them: every kernel that gets these pointers writes rows of [0, nl + 2).
    P.guard_form = g_cg_guard != 0 && P.pair_form && P.fused && !P.BI;
    P.centre_form = P.guard_form && sp->dict_centre;
    // ... without the runs of slots 1 and 7 where no class row of this solve's dictionary holds a coefficient above 2^-53 there (option
    // "cg_zero_runs"; automatic mode: from cg_zero_runs_min_rows rows on, never below 100 000 - iterates equal to rounding only)
    P.zruns_form = P.centre_form && P.dtab_form && (g_dict.nz_slots & ((1 << 1) | (1 << 7))) == 0 && g_cg_zero_runs != 0 &&
                   (g_cg_zero_runs > 0 || P.n >= std::max<int64_t>(g_cg_zero_runs_min_rows, FS_CG_ZERO_RUNS_FLOOR_ROWS));
    P.guard = P.guard_form ? 32 * ((std::max<int64_t>(-(int64_t)sp->dict_min_start, sp->dict_max_start) + 130 + 31) / 32) : 0;
    if (P.fused || P.fusedp_ok) {
        dbuf<double>* const six[6] = {&ws.z, &ws.w, &ws.s, &ws.z2, &ws.w2, &ws.s2};
        for (dbuf<double>* v : six)
            if (v->n != P.nl + 2 || v->guard != P.guard) {
                if (P.guard) FS_CHECK(v->alloc_guarded(P.nl + 2, P.guard, P.s));
                else FS_CHECK(v->alloc(P.nl + 2));
            }
        if (!ws.it_ctr.p) FS_CHECK(ws.it_ctr.alloc(2));
    }
    return FS_OK;
}

// Batches after the first (which carries the event samples) go out as ONE hipGraphLaunch of 2 x batch kernel nodes
// on cache-resident problems: the gaps between consecutive launches (2 x 2.1 us of a 44 us iteration at 1 M DOF)
// shrink to the graph's own node-to-node latency.  > 0: graphs forced, 0: plain launches, < 0: automatic.
static int choose_graph_mode(const krylov_env& env) {
    // rocprofv3 (ROCm 7.2) segfaults inside hipGraphLaunch once about 10 500 kernel nodes have been replayed under
    // --kernel-trace (168 launches of this 64-node graph; nothing to do with the graph's contents or age - renewing
    // the executable does not help, plain launches of the same kernels trace fine).  With the profiler's tool library
    // in the process the automatic mode therefore falls back to plain launches: the kernels and their durations are
    // the same, only the 2 x 2 us of launch gap per iteration come back.  FS_CG_GRAPH=1 still forces graphs.
    int graph_mode = env.graph ? atoi(env.graph) : g_cg_graph;
    if (graph_mode < 0 && env.profiler_attached) {
        static bool told = false;
        if (!told) fprintf(stderr, "[libfsamd] rocprofiler tool library detected: CG batches go out as plain launches, not hipGraphs\n");
        told = true;
        graph_mode = 0;
    }
    return graph_mode;
}

static int prepare_solve(solve_plan& P, krylov_ws& ws, lap_timer& lap) {
    FS_CHECK(ws_prepare(ws, P.n, P.nl, P.opts->max_iter));
    lap("workspace");
    FS_CHECK(prepare_workspace(P, ws));
    P.t_begin = std::chrono::steady_clock::now();
    FS_CHECK(prepare_diagonal_and_threshold(P, ws));
    lap("diagonal, |b|, threshold");
    if (P.ds) FS_CHECK(prepare_scaled_operator(P, ws));
    lap("scaling + row classes");
    FS_CHECK(choose_iteration_form(P, ws));
    P.batch = P.opts->batch > 0 ? P.opts->batch : (P.env.batch > 0 ? P.env.batch : g_cg_batch);
    P.upd_nt = P.env.update_nt ? P.env.update_nt[0] == '1' : (int64_t)P.sp->n_dofs_owned * 72 > ((int64_t)192 << 20);   // five vectors exceed the caches
    P.graph_mode = choose_graph_mode(P.env);
    return FS_OK;
}

// ---- a pass: fresh recurrences from the current x -----------------------------------------------------------------------------

// pipelined CG: the all-reduce of the sums runs on the communication stream of the halo plan, behind ev_upd, and the
// compute stream waits for ev_red only when the next update needs the sums - the product sits in between.  Without
// a halo plan (a replicated operator) the collective stays in-stream.
static int pcg_reduce(const solve_plan& P, const pass_state& ps, krylov_ws& ws, int parity) {
    hipStream_t q = ps.red_stream ? ps.red_stream : P.s;
    if (ps.red_stream) {
        FS_HIP(hipEventRecord(ws.ev_upd, P.s));
        FS_HIP(hipStreamWaitEvent(ps.red_stream, ws.ev_upd, 0));
    }
    FS_CHECK(fs_comm_sum_allreduce_dev(ws.partials.p + (int64_t)parity * 3 * P.vgrid, P.vgrid, 3, ws.sums.p, q));
    if (ps.red_stream) FS_HIP(hipEventRecord(ws.ev_red, ps.red_stream));
    return FS_OK;
}

// Decomposed space, scaled CG: which rows go out early and whether the peer-to-peer iteration is taken - agreed on by all ranks
// once per halo plan (the collective and its synchronisation), read from the plan afterwards.
static int agree_on_exchange(const solve_plan& P, pass_state& ps, krylov_ws& ws) {
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    const int64_t n = P.n;
    fs_halo_plan& hp = sp->halo;
    if (hp.early < 0) {
        bool ok = P.env.halo_early && spmv_is_split(sp);
        int64_t a = 0, b2 = n;
        for (size_t i = 0; ok && i < hp.neighbors.size(); ++i) {
            if (hp.send_counts[i] <= 0) continue;
            const int64_t first = hp.send_first[i], last = first + hp.send_counts[i];
            if (!hp.send_contiguous[i]) ok = false;
            else if (first == 0) a = std::max(a, last);
            else if (last == n) b2 = std::min(b2, first);
            else ok = false;
        }
        a = (a + 1) & ~(int64_t)1;          // the bulk update works on 16-byte pairs
        ok = ok && a < b2 && (a > 0 || b2 < n);
        // every rank has to take the same path: an exchange begun by one side only would never be matched
        // (+ 1024 per rank with the peer-to-peer exchange on: the kernel of the iteration is gated by the status word,
        // the separate send / receive kernels are not - a mix would leave one side waiting)
        double flag = (ok ? 1.0 : 0.0) + (fs_p2p_fusable(sp) ? 1024.0 : 0.0);
        FS_HIP(hipMemcpyAsync(ws.sums.p + 6, &flag, sizeof(double), hipMemcpyHostToDevice, s));
        FS_CHECK(fs_comm_allreduce_dev(ws.sums.p + 6, 1, s));
        FS_HIP(hipMemcpyAsync(&flag, ws.sums.p + 6, sizeof(double), hipMemcpyDeviceToHost, s));
        FS_HIP(hipStreamSynchronize(s));
        const int nr_all = fs_rt().n_ranks, agreed = (int)(flag + 0.5);
        hp.early = agreed % 1024 == nr_all ? 1 : 0;
        hp.fuse = agreed / 1024 == nr_all ? 1 : 0;
        hp.early_a = a;
        hp.early_b = b2;
        if (getenv("FS_KRYLOV_DEBUG"))
            fprintf(stderr, "[fs_krylov] rank %d: rows [0,%lld) and [%lld,%lld) are sent; early start of the exchange: %s\n", fs_rt().rank,
                    (long long)a, (long long)b2, (long long)n, hp.early == 1 ? "yes" : "no");
    }
    if (hp.early == 1) { ps.early_a = hp.early_a; ps.early_b = hp.early_b; }
    // Peer-to-peer exchange on every rank: the iteration is THREE kernels of the compute stream - the plain product, the
    // exchange kernel (k_cg_p2p_exchange: all-reduce, send, receive), the plain update - instead of seven launches on two
    // streams (step_cg_scaled).  FS_P2P_FUSE=0 keeps the separate send / receive / all-reduce kernels of the same transport around a
    // split product.  Measured alternatives that lost on MI355X: ghost columns read straight from the (uncached,
    // fine-grained) receive buffer by the boundary rows of one merged product (67 instead of 39 us per product at 1 M rows),
    // and the sums posted by the last workgroup of the product (its agent-scope fence in every workgroup writes back the
    // whole L2 of the XCD: + 26 us).
    ps.p2p_rows_cap = P.env.p2p_rows_blocks > 0 ? P.env.p2p_rows_blocks : 128;
    if (hp.fuse == 1 && !P.pipelined && P.env.p2p_fuse) ps.p2p_fuse = 1;
    return FS_OK;
}

// initial state, r0, the pipelined and BiCGStab starts, the iteration limit, how the launches of the pass go out
static int begin_pass(const solve_plan& P, pass_state& ps, krylov_ws& ws) {
    fs_matrix_s* A = P.A;
    fs_space_s* sp = P.sp;
    fs_vector_s *b = P.b, *x = P.x;
    hipStream_t s = P.s;
    const int64_t n = P.n, nl = P.nl;
    FS_CHECK(ws.status.zero(s));
    FS_CHECK(ws.scal.zero(s));
    if (g_cg_poison_p) {          // (a pass sets p_{-1} = 0 itself: the LIGHT launches never write p, the first PAIR launch reads it)
        FS_HIP(hipMemsetAsync(ws.p.p, 0xff, (size_t)ws.p.n * sizeof(double), s));
        g_cg_poison_p = 0;
    }
    // p, s, z and - from a zero guess - x in one launch
    hipLaunchKernelGGL(k_zero4, dim3(fs_grid_for(std::max<int64_t>(nl / 2, 1), FS_BLOCK, 1024)), dim3(FS_BLOCK), 0, s, ws.p.p, ws.p.n, ws.s.p, ws.s.n,
                       ws.z.p, ws.z.n, x->d.p, ps.use_guess ? (int64_t)0 : x->d.n);
    if (sp->halo.active) {          // s on the ghost rows (k_cg_p2p_exchange)
        if (ws.sg.n < nl - n + 2) FS_CHECK(ws.sg.alloc(nl - n + 2));
        FS_CHECK(ws.sg.zero(s));
    }
    // r0 = rhs - A x, or rhs from a zero guess.  Scaled: the unknown xhat = D^1/2 x lives in the caller's x until the final un-scaling,
    // rhs = bhat, r0 in ws.z; otherwise r0 in ws.r and z = D^-1 r0
    const double* const rhs = P.ds ? ws.bhat.p : b->d.p;
    double* const r0 = P.ds ? ws.z.p : ws.r.p;
    if (ps.use_guess) {
        if (P.ds && ps.n_pass == 0) hipLaunchKernelGGL(k_pointwise_div, dim3(fs_grid_for(n)), dim3(FS_BLOCK), 0, s, x->d.p, ws.dinv.p, n, x->d.p);
        FS_HIP(hipMemcpyAsync(ws.z.p, x->d.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        FS_CHECK(fs_halo_exchange_dev(sp, ws.z.p, s));
        launch_spmv<0>(A, ws.z.p, ws.w.p, nullptr, nullptr, nullptr, s, P.aval);
        hipLaunchKernelGGL(k_residual, dim3(P.pgrid), dim3(FS_BLOCK), 0, s, rhs, ws.w.p, n, r0, ws.partials.p);
    } else {
        FS_HIP(hipMemcpyAsync(r0, rhs, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (!P.ds) hipLaunchKernelGGL(k_pointwise_mul, dim3(fs_grid_for(n)), dim3(FS_BLOCK), 0, s, ws.dinv.p, ws.r.p, n, ws.z.p);
    FS_KERNEL_CHECK();
    ps.red_stream = nullptr;
    // (the peer-to-peer all-reduce is a kernel of a few microseconds: it stays in the compute stream, a second stream's two event
    // hops cost more than it hides)
    if (P.pipelined && !P.fuse_sums && sp->halo.active && !fs_p2p_reduce_enabled()) FS_CHECK(fs_halo_comm_stream(sp, &ps.red_stream));
    if (P.pipelined) {
        // r0 sits in ws.z; w0 = A r0, z = 0 (p, s are zero already), sums of (r0, w0)
        FS_CHECK(ws.pz.zero(s));
        FS_CHECK(fs_halo_exchange_dev(sp, ws.z.p, s));
        launch_spmv<0>(A, ws.z.p, ws.pw.p, nullptr, nullptr, nullptr, s, P.aval);
        hipLaunchKernelGGL(k_pcg_dots, dim3(P.vgrid), dim3(FS_BLOCK), 0, s, n, ws.z.p, ws.pw.p, ws.dvec.p, ws.partials.p, P.vgrid);
        FS_KERNEL_CHECK();
        if (!P.fuse_sums) FS_CHECK(pcg_reduce(P, ps, ws, 0));
    }
    if (P.bicg) {
        // rhat = r0; first (rhat.r, r.r) partials; v = 0 (ws.w), p = 0, y = 0
        FS_HIP(hipMemcpyAsync(ws.rhat.p, ws.r.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        FS_CHECK(ws.w.zero(s));
        FS_CHECK(ws.y.zero(s));
        hipLaunchKernelGGL(k_dot2_partial, dim3(P.vgrid), dim3(FS_BLOCK), 0, s, ws.rhat.p, ws.r.p, ws.r.p, ws.r.p, n, ws.partials2.p);
        FS_KERNEL_CHECK();
    }

    // iteration pipeline
    ps.max_iter = P.opts->max_iter - ps.total_iters > 0 ? P.opts->max_iter - ps.total_iters : 1;
    hipLaunchKernelGGL(k_set_iteration_limit, dim3(1), dim3(64), 0, s, ws.ctrl.p, ps.max_iter);
    ps.hist_p = ws.hist.p + ps.total_iters;
    ps.k = 0; ps.slot = 0; ps.pending = -1;
    ps.finished = false;
    ps.first_sample = ps.sm.n;
    ps.early_a = 0; ps.early_b = n;
    ps.p2p_fuse = 0; ps.p2p_rows_cap = 128;
    ps.p2p_ghosts_in = false;
    // (a condition every rank evaluates alike; !fuse_sums: a communicator is up)
    if (P.ds && !P.bicg && !P.fuse_sums && sp->halo.active) FS_CHECK(agree_on_exchange(P, ps, ws));
    // (the peer-to-peer iteration is three kernels and no library call, with its sequence numbers on the device: it is captured the
    // same way; the RCCL iteration is not - ncclSend / ncclRecv / ncclAllReduce are host calls)
    // (automatic mode: every size - the launch gaps are 10 % of an iteration at 1 M rows and still 1.5 % at 10 M)
    ps.graph_sized = P.graph_mode != 0;
    // The FIRST graph a process instantiates costs 9 ms (the runtime's graph machinery; later ones 0.1 ms), twelve times what the
    // graphs save a 300-iteration solve at 1 M rows: the first solve of a process launches its iterations one by one - a
    // one-shot run never pays, a time loop pays in its second step (tools/probes/first_step_probe.py; FS_CG_GRAPH=1 forces graphs)
    // (round 6: fs_init instantiates a two-node graph on a helper thread while the code objects load - the machinery is paid for
    // there, and the first solve of a process goes out in graphs like every other; FS_WARM=0 restores the old rule)
    static bool first_solve_done = P.env.warm;
    ps.graphs_allowed = first_solve_done || P.graph_mode > 0;
    first_solve_done = true;            // (for the passes and solves after this one)
    ps.fusedp = P.fusedp_ok && ps.p2p_fuse && !P.bicg;
    if (ps.fusedp) ps.fusedp_used = true;
    ps.use_graph = P.ds && !P.bicg && !P.pipelined && ps.graph_sized && !P.fused && !ps.fusedp &&
                   ((P.fuse_sums && !sp->halo.active && P.bs == 1) || ps.p2p_fuse);
    // One-launch iteration on one GPU: the host follows the device through two words of pinned memory the kernel's leader lane
    // writes (iteration in progress, status once stopped) and keeps between cg_ahead and cg_ahead + cg_sub launches enqueued.
    // With batches of 32 and the status word copied back behind each, a solve of 293 iterations enqueued 352 launches - the
    // 59 that returned on the status word cost 5.3 us each, 0.31 of a 6.8 ms solve - and ten in-stream copies.
    // (the same for the two-launch iteration on one GPU - streaming products, row-dictionary products above 3 M rows -, whose
    // update kernel writes the words: its batches of 32 left up to 59 x 2 launches behind the last iteration)
    const bool two_launch_1gpu = ps.use_graph && !ps.p2p_fuse && P.fuse_sums && !sp->halo.active;
    ps.mirrored = ((P.fused && !ps.fusedp) || two_launch_1gpu) && ws.d_mirror && ws.mirror_ok && (P.env.mirror >= 0 ? P.env.mirror != 0 : g_cg_mirror != 0);
    ps.mirror_dev = ps.mirrored ? ws.d_mirror : nullptr;
    if (ps.mirrored) {
        volatile int* const hm = ws.h_mirror;
        hm[0] = 0; hm[1] = 0;
    }
    ps.bsz = ps.mirrored ? g_cg_sub : P.batch;
    // the launches that carry the event samples go out one by one before the graphs take over: the first 32 iterations (samples
    // at iterations 1 and 17), or - with the progress words - the first 16 (samples at 1 and 9)
    ps.first_plain = ps.mirrored ? std::min(P.batch, 16) : P.batch;
    ps.sm.step = ps.mirrored ? std::min(P.env.sample_every, 8) : P.env.sample_every;
    ps.seen = 0;
    ps.t_seen = std::chrono::steady_clock::now();
    return FS_OK;
}

// ---- the steps of the two-, three- and many-launch iterations ------------------------------------------------------------------

// k_cg_update_scaled on rows [m0, m0 + nm): sums in the kernel (fuse: npart partials, progress words) or reduced before it,
// non-temporal accesses where the vectors exceed the caches.  it = -1: iteration index and limit from the device (captured launches).
static void launch_update_scaled(const solve_plan& P, const pass_state& ps, krylov_ws& ws, bool fuse, int it, int co, int npart, int64_t m0, int64_t nm) {
    const auto kernel = fuse ? (P.upd_nt ? k_cg_update_scaled<true, true> : k_cg_update_scaled<true, false>)
                             : (P.upd_nt ? k_cg_update_scaled<false, true> : k_cg_update_scaled<false, false>);
    // (the progress words and the plain stores of r are the FUSE = true instantiation's: the other one gets the defaults of its declaration)
    hipLaunchKernelGGL(kernel, dim3(P.vgrid), dim3(FS_BLOCK), 0, P.s, nm, it, co, ws.partials.p, npart, ws.sums.p, ws.ctrl.p, ws.scal.p, ws.status.p, ps.hist_p,
                       ws.z.p + m0, ws.w.p + m0, ws.p.p + m0, ws.s.p + m0, P.x->d.p + m0, fuse ? ps.mirror_dev : nullptr, fuse ? g_upd_r_plain : 0);
}

// plain Jacobi CG: product with its dots, the sums (in the update kernel or by an all-reduce), the update
static int step_cg(const solve_plan& P, pass_state& ps, krylov_ws& ws, int k) {
    hipStream_t s = P.s;
    sampler& sm = ps.sm;
    sm.begin(k, 1);
    FS_CHECK(sm.mark(0));
    FS_CHECK(spmv_overlapped<1>(P.A, ws.z.p, ws.w.p, ws.r.p, ws.partials.p, ws.status.p, s));
    FS_CHECK(sm.mark(1));
    if (!P.fuse_sums) FS_CHECK(fs_comm_sum_allreduce_dev(ws.partials.p, P.sgrid, 3, ws.sums.p, s));
    FS_CHECK(sm.mark(2));
    hipLaunchKernelGGL(P.fuse_sums ? k_cg_update<true> : k_cg_update<false>, dim3(P.vgrid), dim3(FS_BLOCK), 0, s, P.n, k, k == ps.max_iter ? 1 : 0, ws.partials.p, P.sgrid,
                       ws.sums.p, ws.ctrl.p, ws.scal.p, ws.status.p, ps.hist_p, ws.dinv.p, ws.z.p, ws.w.p, ws.p.p, ws.s.p, P.x->d.p, ws.r.p);
    return sm.close();
}

// diagonally scaled CG, two launches on one GPU; over a communicator with the early-halo split of the update.
// k = -1: a launch that is being captured (iteration index and limit from the device)
static int step_cg_scaled(const solve_plan& P, pass_state& ps, krylov_ws& ws, int k) {
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    const int64_t n = P.n;
    sampler& sm = ps.sm;
    sm.begin(k, 1);
    FS_CHECK(sm.mark(0));
    FS_CHECK(spmv_overlapped<3>(P.A, ws.z.p, ws.w.p, ws.dvec.p, ws.partials.p, ws.status.p, s, P.aval));
    FS_CHECK(sm.mark(1));
    const int co = k == ps.max_iter ? 1 : 0;
    if (P.fuse_sums) {
        FS_CHECK(sm.mark(2));
        launch_update_scaled(P, ps, ws, true, k, co, P.sgrid, 0, n);
    } else {
        FS_CHECK(fs_comm_sum_allreduce_dev(ws.partials.p, P.sgrid, 3, ws.sums.p, s));
        FS_CHECK(sm.mark(2));
        // Slabs send a prefix and / or a suffix of their rows: those are updated first and their exchange is
        // started, so that it runs under the rest of the update AND the interior product of the next iteration
        // (the exchange alone used to start only with that product).
        int64_t m0 = 0, m1 = n;
        if (ps.early_a > 0 || ps.early_b < n) {
            hipLaunchKernelGGL(k_cg_update_scaled_rows, dim3(fs_grid_for(ps.early_a + (n - ps.early_b), FS_BLOCK, 256)), dim3(FS_BLOCK), 0, s,
                               ps.early_a, ps.early_b, n, k, co, ws.sums.p, ws.ctrl.p, ws.scal.p, ws.status.p, ws.z.p, ws.w.p, ws.p.p, ws.s.p, P.x->d.p);
            FS_CHECK(fs_halo_begin_dev(sp, ws.z.p, s));
            sp->halo.begun = true;
            m0 = ps.early_a; m1 = ps.early_b;
        }
        launch_update_scaled(P, ps, ws, false, k, co, P.sgrid, m0, m1 - m0);
    }
    return sm.close();
}

// the three-kernel peer-to-peer iteration: the plain product, the exchange kernel (all-reduce, send, receive), the plain update.
// k = -1: a launch that is being captured
static int step_p2p(const solve_plan& P, pass_state& ps, krylov_ws& ws, int k) {
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    sampler& sm = ps.sm;
    const int co = k == ps.max_iter ? 1 : 0;
    fs_p2p_rowsred red = {};
    fs_p2p_sendrows snd = {};
    if (k >= 0 && !ps.p2p_ghosts_in) {          // first iteration of a pass: the plain send and receive kernels
        FS_CHECK(fs_halo_exchange_dev(sp, ws.z.p, s));
        ps.p2p_ghosts_in = true;
    }
    sm.begin(k, 1);
    FS_CHECK(sm.mark(0));
    launch_spmv<3>(P.A, ws.z.p, ws.w.p, ws.dvec.p, ws.partials.p, ws.status.p, s, P.aval);
    FS_CHECK(sm.mark(1));
    FS_CHECK(sm.mark(2));
    const int fgrid = spmv_partials_unsplit(sp, P.bs);
    FS_CHECK(fs_p2p_exchange_args(sp, ws.partials.p, fgrid, ws.sums.p, &red, &snd));
    const int64_t work = std::max(snd.total_send, snd.total_recv);
    hipLaunchKernelGGL((k_cg_p2p_exchange<false>), dim3(fs_grid_for(std::max<int64_t>(work, 1), FS_BLOCK, ps.p2p_rows_cap)), dim3(FS_BLOCK), 0, s,
                       k, co, ws.ctrl.p, ws.scal.p, ws.status.p, ws.z.p, ws.w.p, ws.sg.p, red, snd, fs_pp_ghosts{});
    launch_update_scaled(P, ps, ws, false, k, co, fgrid, 0, P.n);
    return sm.close();
}

// the pipelined recurrence: n = A w under which the sums of (r, w) are reduced (on the second stream where there is one)
static int step_pipelined(const solve_plan& P, pass_state& ps, krylov_ws& ws, int k) {
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    const int64_t n = P.n;
    sampler& sm = ps.sm;
    const int co = k == ps.max_iter ? 1 : 0;
    sm.begin(k, 1);
    // n = A w (its halo was begun behind the previous update), under which the sums of (r, w) are reduced
    FS_CHECK(sm.mark(0));
    FS_CHECK(spmv_overlapped<4>(P.A, ws.pw.p, ws.w.p, nullptr, nullptr, ws.status.p, s, P.aval));
    FS_CHECK(sm.mark(1));
    if (ps.red_stream) FS_HIP(hipStreamWaitEvent(s, ws.ev_red, 0));
    FS_CHECK(sm.mark(2));
    int64_t m0 = 0, m1 = n;
    if (ps.early_a > 0 || ps.early_b < n) {
        hipLaunchKernelGGL(k_pcg_update_rows, dim3(fs_grid_for(ps.early_a + (n - ps.early_b), FS_BLOCK, 256)), dim3(FS_BLOCK), 0, s,
                           ps.early_a, ps.early_b, n, k, co, ws.sums.p, ws.ctrl.p, ws.scal.p, ws.status.p, ws.z.p, ws.pw.p, ws.w.p, ws.p.p, ws.s.p, ws.pz.p, P.x->d.p);
        FS_CHECK(fs_halo_begin_dev(sp, ws.pw.p, s));
        sp->halo.begun = true;
        m0 = ps.early_a; m1 = ps.early_b;
    }
    const auto kernel = P.fuse_sums ? (P.upd_nt ? k_pcg_update<true, true> : k_pcg_update<true, false>) : (P.upd_nt ? k_pcg_update<false, true> : k_pcg_update<false, false>);
    hipLaunchKernelGGL(kernel, dim3(P.vgrid), dim3(FS_BLOCK), 0, s, n, m0, m1, k, co, ws.partials.p, P.vgrid, ws.sums.p, ws.ctrl.p, ws.scal.p, ws.status.p, ps.hist_p,
                       ws.dvec.p, ws.z.p, ws.pw.p, ws.w.p, ws.p.p, ws.s.p, ws.pz.p, P.x->d.p);
    FS_CHECK(sm.close());
    if (!P.fuse_sums) {
        // the halo of the new w goes first on the communication stream (the boundary rows of the next
        // product wait for it), the reduction of the new sums behind it
        // (whether a rank's product is split is a LOCAL property - a thin part may have no interior slice -
        // while the order of halo and reduction on the communicator must be the same everywhere: the
        // exchange is begun here on every rank with a plan, split or not)
        if (!sp->halo.begun && sp->halo.active) {
            FS_CHECK(fs_halo_begin_dev(sp, ws.pw.p, s));
            sp->halo.begun = true;
        }
        FS_CHECK(pcg_reduce(P, ps, ws, (k + 1) & 1));
    }
    return FS_OK;
}

static int step_bicgstab(const solve_plan& P, pass_state& ps, krylov_ws& ws, int k) {
    fs_matrix_s* A = P.A;
    hipStream_t s = P.s;
    const int64_t n = P.n;
    const int vgrid = P.vgrid, sgrid = P.sgrid;
    const bool fuse = P.fuse_sums;
    double* const x = P.x->d.p;
    sampler& sm = ps.sm;
    const int co = k == ps.max_iter ? 1 : 0;
    sm.begin(k, 1);
    // K1: p, y
    if (!fuse) FS_CHECK(fs_comm_sum_allreduce_dev(ws.partials2.p, vgrid, 2, ws.bsums.p, s));
    hipLaunchKernelGGL(fuse ? k_bicg_p<true> : k_bicg_p<false>, dim3(vgrid), dim3(FS_BLOCK), 0, s, n, k, co, ws.partials2.p, vgrid, ws.bsums.p, ws.ctrl.p, ws.scal.p, ws.status.p, ps.hist_p, ws.dinv.p, ws.r.p, ws.p.p, ws.w.p, ws.y.p);
    // K2: v = A y, rhat.v
    FS_CHECK(sm.mark(0));
    FS_CHECK(spmv_overlapped<2>(A, ws.y.p, ws.w.p, ws.rhat.p, ws.partials.p, ws.status.p, s));
    FS_CHECK(sm.mark(1));
    // K3: s, z
    FS_CHECK(sm.mark(2));
    if (!fuse) FS_CHECK(fs_comm_sum_allreduce_dev(ws.partials.p, sgrid, 1, ws.bsums.p + 4, s));
    hipLaunchKernelGGL(fuse ? k_bicg_s<true> : k_bicg_s<false>, dim3(vgrid), dim3(FS_BLOCK), 0, s, n, k, ws.partials.p, sgrid, ws.bsums.p + 4, ws.scal.p, ws.status.p, ws.dinv.p, ws.r.p, ws.w.p, ws.s.p, ws.z.p);
    FS_CHECK(sm.close());
    // K4: t = A z, (t.s, t.t)
    FS_CHECK(spmv_overlapped<2>(A, ws.z.p, ws.t.p, ws.s.p, ws.partials.p, ws.status.p, s));
    // K5: x, r, next (rhat.r, r.r)
    if (!fuse) FS_CHECK(fs_comm_sum_allreduce_dev(ws.partials.p, sgrid, 2, ws.bsums.p + 8, s));
    hipLaunchKernelGGL(fuse ? k_bicg_x<true> : k_bicg_x<false>, dim3(vgrid), dim3(FS_BLOCK), 0, s, n, k, ws.partials.p, sgrid, ws.bsums.p + 8, ws.scal.p, ws.status.p, x, ws.y.p, ws.z.p, ws.r.p, ws.s.p, ws.t.p, ws.rhat.p, ws.partials2.p);
    return FS_OK;
}

// iteration k of the pass in the form the plan and the pass chose (every form but the one-launch iteration)
static int step(const solve_plan& P, pass_state& ps, krylov_ws& ws, int k) {
    if (P.bicg) return step_bicgstab(P, ps, ws, k);
    if (P.pipelined) return step_pipelined(P, ps, ws, k);
    if (ps.p2p_fuse) return step_p2p(P, ps, ws, k);
    return P.ds ? step_cg_scaled(P, ps, ws, k) : step_cg(P, ps, ws, k);
}

// A full batch of the two-launch iteration on one GPU or of the peer-to-peer iteration as ONE graph launch (the steps above
// captured with k = -1).
static int run_graph_batch(const solve_plan& P, pass_state& ps, krylov_ws& ws, int kend) {
    fs_matrix_s* A = P.A;
    fs_space_s* sp = P.sp;
    // everything the captured launches bake in: the vectors of the workspace, the operator's value and
    // structure arrays - and the serial numbers of matrix and space, because a destroyed operator's heap
    // and pool addresses are handed out again (another mesh with the same row count would otherwise replay
    // this graph over column arrays that no longer exist)
    fs_p2p_rowsred red = {};
    fs_p2p_sendrows snd = {};
    const int fgrid = ps.p2p_fuse ? spmv_partials_unsplit(sp, P.bs) : P.sgrid;
    if (ps.p2p_fuse) FS_CHECK(fs_p2p_exchange_args(sp, ws.partials.p, fgrid, ws.sums.p, &red, &snd));
    const bool dict_on = g_dict.built_for && g_dict.built_for == P.aval;
    // (the tile product of a lattice-ordered operator bakes in the list tables, the tile table and the geometry of lat_prepare:
    // those buffers grow - are allocated anew - when another space brings more classes or tiles)
    const bool lat_on = dict_on && g_lat.ok && g_lat.built_for == P.aval && g_lat.space_serial == sp->serial;
    const bool lm_on = lat_on && g_lm.ok && g_lat_march;          // (k_lat_march bakes in its own tables and geometry)
    graph_key key = {};
    key.A = A; key.aval = P.aval; key.sell_col = sp->sell_col.p;
    key.n = P.n; key.matrix_serial = (int64_t)A->serial; key.space_serial = (int64_t)sp->serial;
    key.x = P.x->d.p; key.hist = ps.hist_p; key.z = ws.z.p; key.w = ws.w.p; key.p = ws.p.p; key.s = ws.s.p;
    key.weights = ws.dvec.p; key.partials = ws.partials.p; key.status = ws.status.p;
    if (dict_on) {          // (whether the product is the row-dictionary kernel, with the class count and widths its launch bakes in)
        key.dict_cls = g_dict.cls.p; key.dict_values = g_dict.values.p; key.dict_items = sp->dict_items.p; key.dict_plans = sp->dict_plans.p;
        key.items_interior = sp->halo.items_interior.p; key.items_boundary = sp->halo.items_boundary.p;
        key.dict_ncls = g_dict.ncls; key.dict_S = g_dict.S; key.dict_C = g_dict.C;
    }
    if (lat_on) {
        key.lat_tab[0] = lm_on ? (const void*)g_lm.sl_line.p : (const void*)g_lat.tile_cls.p;
        key.lat_tab[1] = g_lat.cnt.p; key.lat_tab[2] = g_lat.coef.p;
        key.lat_tab[3] = lm_on ? (const void*)g_lm.SL.p : (const void*)g_lat.rel.p;
        key.lat_tab[4] = g_lat.off.p; key.lat_tab[5] = g_lat.relc.p;
        key.lat_n_tiles = g_lat.geom.n_tiles; key.lat_grid = g_lat.geom.grid; key.lat_w_tiles = g_lat.geom.w_tiles;
    }
    if (lm_on) { key.lm_on = 1; key.lm_PY = g_lm.g.PY; key.lm_ZC = g_lm.g.ZC; }
    if (ps.p2p_fuse) {
        key.sg = ws.sg.p;
        key.snd_own_recv = snd.own_recv; key.snd_peers = snd.peers; key.red_own_buf = red.own_buf; key.red_peer_buf = red.peer_buf;
        key.p2p_on = 1; key.p2p_generation = (int64_t)sp->halo.p2p.generation; key.p2p_rows_cap = ps.p2p_rows_cap;
    }
    key.bsz = ps.bsz; key.fgrid = fgrid; key.vgrid = P.vgrid;
    key.upd_nt = P.upd_nt; key.spmv_nt = spmv_nontemporal(sp, P.bs); key.mirror = ps.mirror_dev != nullptr;
    FS_CHECK(ws.cg_graph.replay(key, ps.bsz, P.s, [&](int) { return ps.p2p_fuse ? step_p2p(P, ps, ws, -1) : step_cg_scaled(P, ps, ws, -1); }));
    ps.k = kend;
    return FS_OK;
}

// ---- the one-launch iteration -------------------------------------------------------------------------------------------------

// What the launches of a pass share.  Launch k = update k + product k + 1; buffers [k & 1] are read, [(k + 1) & 1] written.
// Decomposed space (fusedp): the exchange kernel goes first - it reduces the sums of the previous launch's partials over the ranks,
// stores the neighbours' w into the ghost rows of the current w and advances the ghost rows of r and s into the next buffers
struct one_launch {
    double *Z[2], *W[2], *SV[2], *PT[2];
    bool pair, dtab, guarded, centre, zruns;
    size_t lds;
    const double* weights;
    fs_p2p_rowsred red2[2];
    fs_p2p_sendrows snd2[2];
};

static int one_launch_setup(const solve_plan& P, pass_state& ps, krylov_ws& ws, one_launch& L) {
    L.Z[0] = ws.z.p; L.Z[1] = ws.z2.p;
    L.W[0] = ws.w.p; L.W[1] = ws.w2.p;
    L.SV[0] = ws.s.p; L.SV[1] = ws.s2.p;
    L.PT[0] = ws.partials.p; L.PT[1] = ws.partials.p + 3 * (int64_t)P.igrid;
    // (one GPU only: behind the exchange kernel of a decomposed space the LIGHT instantiation compiles to 132 VGPRs, three
    // waves per SIMD instead of the four the launch needs - that form keeps p and x in every launch)
    L.pair = P.pair_form && !ps.fusedp && !P.BI;
    L.dtab = L.pair && P.dtab_form;
    L.guarded = L.pair && P.guard_form;
    L.centre = L.pair && P.centre_form;
    L.zruns = L.centre && L.dtab && P.zruns_form;
    ps.iteration_runs = L.zruns ? 2 : 0;
    ps.iteration_form = (L.pair ? 1 : 0) | (L.dtab ? 2 : 0) | (L.guarded ? 4 : 0) | (L.centre ? 8 : 0);
    L.lds = (size_t)g_dict.ncls * (g_dict.S + (L.dtab ? 1 : 0)) * sizeof(double);
    L.weights = L.dtab ? g_dict.dtab.p : ws.dvec.p;
    if (ps.fusedp)
        for (int c = 0; c < 2; ++c) FS_CHECK(fs_p2p_exchange_args(P.sp, L.PT[c], P.igrid, ws.sums.p, &L.red2[c], &L.snd2[c]));
    return FS_OK;
}

// k_dict_cg_iter<3, TA ...> on the buffers of parity par
template <auto... TA>
static void launch_dict_iter(const solve_plan& P, const pass_state& ps, krylov_ws& ws, const one_launch& L, int par) {
    fs_space_s* sp = P.sp;
    hipLaunchKernelGGL((k_dict_cg_iter<3, TA...>), dim3(P.igrid), dim3(FS_BLOCK), L.lds, P.s, sp->n_nodes_local, sp->n_dict_items, reinterpret_cast<const int4*>(sp->dict_items.p),
                       reinterpret_cast<const dict_plan_round*>(sp->dict_plans.p), g_dict.cls.p, g_dict.values.p, g_dict.S, g_dict.ncls,
                       L.Z[par], L.W[par], L.SV[par], L.Z[par ^ 1], L.W[par ^ 1], L.SV[par ^ 1], ws.p.p, P.x->d.p, L.weights, L.PT[par], L.PT[par ^ 1], P.igrid,
                       ws.ctrl.p, ws.scal.p, ws.status.p, ws.it_ctr.p, par, ps.hist_p, dict_map_xcd(), ws.sums.p, ps.mirror_dev);
}
// the LIGHT (even) or PAIR (odd) launch (launch parity = iteration parity: it_ctr is zeroed at k = 0)
template <bool DT, bool GU, bool CE, bool ZR = false>
static void launch_dict_pair(const solve_plan& P, const pass_state& ps, krylov_ws& ws, const one_launch& L, int par) {
    if (par) launch_dict_iter<false, FS_ITER_PAIR, DT, GU, CE, ZR>(P, ps, ws, L, par);
    else launch_dict_iter<false, FS_ITER_LIGHT, DT, GU, CE, ZR>(P, ps, ws, L, par);
}

template <int AHEAD>
static void launch_box_iter(const solve_plan& P, const pass_state& ps, krylov_ws& ws, const one_launch& L, int par) {
    const box_iter_plan_s* BI = P.BI;
    hipLaunchKernelGGL((k_box_cg_iter<4, 2, AHEAD, 2>), dim3(P.igrid), dim3(6 * 64), BI->lds, P.s, BI->g, g_dict.cls.p, g_dict.values.p, g_dict.ncls, L.Z[par], L.W[par], L.SV[par], L.Z[par ^ 1], L.W[par ^ 1],
                       L.SV[par ^ 1], ws.p.p, P.x->d.p, ws.dvec.p, L.PT[par], L.PT[par ^ 1], P.igrid, ws.ctrl.p, ws.scal.p, ws.status.p, ws.it_ctr.p, par, ps.hist_p, ps.mirror_dev);
}

static void launch_exchange(const solve_plan& P, const pass_state& ps, krylov_ws& ws, const one_launch& L, int par) {
    const int64_t work = std::max(L.snd2[par].total_send, L.snd2[par].total_recv);
    const fs_pp_ghosts pp = {L.W[par], L.SV[par], L.SV[par ^ 1], L.Z[par], L.Z[par ^ 1], ws.it_ctr.p, par};
    hipLaunchKernelGGL((k_cg_p2p_exchange<true>), dim3(fs_grid_for(std::max<int64_t>(work, 1), FS_BLOCK, ps.p2p_rows_cap)), dim3(FS_BLOCK), 0, P.s,
                       0, 0, ws.ctrl.p, ws.scal.p, ws.status.p, (double*)nullptr, L.W[par], (double*)nullptr, L.red2[par], L.snd2[par], pp);
}

// one iteration: the form's kernel on the buffers of parity par
static void launch_iter(const solve_plan& P, const pass_state& ps, krylov_ws& ws, const one_launch& L, int par) {
    if (P.BI && !ps.fusedp) {
        if (P.BI->ahead == 2) launch_box_iter<2>(P, ps, ws, L, par);
        else launch_box_iter<1>(P, ps, ws, L, par);
    } else if (ps.fusedp) {
        launch_exchange(P, ps, ws, L, par);
        launch_dict_iter<true>(P, ps, ws, L, par);
    } else if (!L.pair) launch_dict_iter<false>(P, ps, ws, L, par);
    else if (L.zruns) launch_dict_pair<true, true, true, true>(P, ps, ws, L, par);
    else if (L.centre) { if (L.dtab) launch_dict_pair<true, true, true>(P, ps, ws, L, par); else launch_dict_pair<false, true, true>(P, ps, ws, L, par); }
    else if (L.guarded) { if (L.dtab) launch_dict_pair<true, true, false>(P, ps, ws, L, par); else launch_dict_pair<false, true, false>(P, ps, ws, L, par); }
    else if (L.dtab) launch_dict_pair<true, false, false>(P, ps, ws, L, par);
    else launch_dict_pair<false, false, false>(P, ps, ws, L, par);
}

// product 0 (w_0 = A r_0 and its sums) by the plain product kernel; s_{-1} = p_{-1} = 0 were set by begin_pass
static int one_launch_first_product(const solve_plan& P, pass_state& ps, krylov_ws& ws) {
    hipStream_t s = P.s;
    FS_CHECK(ws.it_ctr.zero(s));
    if (ps.fusedp && !ps.p2p_ghosts_in) {          // the ghost rows of r_0: the plain send and receive kernels
        FS_CHECK(fs_halo_exchange_dev(P.sp, ws.z.p, s));
        ps.p2p_ghosts_in = true;
    }
    if (P.BI && !ps.fusedp) {
        // (the product kernel on the ITERATION's patches and chunks: one dot partial per workgroup of either kernel)
        box_plan_s P0;
        P0.g = P.BI->g; P0.lds = P.BI->lds_product; P0.shape = 0;
        launch_box<3>(&P0, g_dict.cls.p, g_dict.values.p, g_dict.ncls, ws.z.p, ws.w.p, ws.dvec.p, ws.partials.p, ws.status.p, 0, P.igrid, 1, s);
        g_last_product_kind = 3;
    } else
        launch_spmv<3>(P.A, ws.z.p, ws.w.p, ws.dvec.p, ws.partials.p, ws.status.p, s, P.aval, nullptr, 0, 0, 0, 0);
    return FS_OK;
}

// launches [ps.k, kend): a full batch behind the first plain ones as one graph, the rest one by one with the event samples
static int one_launch_batch(const solve_plan& P, pass_state& ps, krylov_ws& ws, const one_launch& L, int kend) {
    fs_space_s* sp = P.sp;
    const int bsz = ps.bsz;
    if (ps.k == 0) FS_CHECK(one_launch_first_product(P, ps, ws));
    if (ps.graph_sized && ps.graphs_allowed && ps.k >= ps.first_plain && kend - ps.k == bsz && kend <= ps.max_iter && (bsz & 1) == 0 && (ps.k & 1) == 0) {
        graph_key key = {};
        key.A = P.A; key.aval = P.aval;
        key.n = P.n; key.matrix_serial = (int64_t)P.A->serial; key.space_serial = (int64_t)sp->serial;
        key.x = P.x->d.p; key.hist = ps.hist_p; key.z = ws.z.p; key.w = ws.w.p; key.p = ws.p.p; key.s = ws.s.p;
        key.z2 = ws.z2.p; key.w2 = ws.w2.p; key.s2 = ws.s2.p; key.weights = L.weights; key.partials = ws.partials.p; key.status = ws.status.p;
        key.ctrl = ws.ctrl.p; key.scal = ws.scal.p; key.it_ctr = ws.it_ctr.p;
        key.dict_cls = g_dict.cls.p; key.dict_values = g_dict.values.p; key.dict_items = sp->dict_items.p; key.dict_plans = sp->dict_plans.p;
        key.dict_ncls = g_dict.ncls; key.dict_S = g_dict.S; key.n_dict_items = sp->n_dict_items; key.map_xcd = dict_map_xcd();
        key.snd_own_recv = L.snd2[0].own_recv; key.red_own_buf = L.red2[0].own_buf;
        if (ps.fusedp) { key.p2p_on = 1; key.p2p_generation = (int64_t)sp->halo.p2p.generation; }
        key.p2p_rows_cap = ps.p2p_rows_cap;
        key.bsz = bsz; key.box_ahead = P.BI ? P.BI->ahead : 0; key.iteration_form = ps.iteration_form | ps.iteration_runs << 8; key.igrid = P.igrid;
        key.mirror = ps.mirror_dev != nullptr;
        FS_CHECK(ws.cgf_graph.replay(key, bsz, P.s, [&](int i) { launch_iter(P, ps, ws, L, i & 1); return FS_OK; }));
        ps.k = kend;
    }
    for (; ps.k < kend; ++ps.k) {
        if (ps.sm.begin(ps.k, 0)) FS_CHECK(ps.sm.mark(0));
        launch_iter(P, ps, ws, L, ps.k & 1);
        FS_CHECK(ps.sm.launch_done(L.pair, ps.k + 1 == kend));
    }
    return FS_OK;
}

// ---- the iterations of a pass, its end ------------------------------------------------------------------------------------------

// The progress words of the device: 0 = go on enqueueing, 1 = enough enqueued (look again), 2 = the recurrence has stopped
static int mirror_look(pass_state& ps, krylov_ws& ws, hipStream_t s, int* what) {
    volatile int* const hm = ws.h_mirror;
    *what = 0;
    if (hm[0] != 0) { *what = 2; return FS_OK; }                  // what is enqueued returns on the status word
    const int done = hm[1];
    if (ps.k - done <= g_cg_ahead) return FS_OK;
    *what = 1;                                                    // enough enqueued: wait for the device to get on
    if (done != ps.seen) { ps.seen = done; ps.t_seen = std::chrono::steady_clock::now(); }
    else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - ps.t_seen).count() > 2.0) {
        // no progress seen for two seconds: the kernel's stores do not reach this host memory while it runs.  The
        // copied status word from here on, for the rest of the process.
        FS_HIP(hipStreamSynchronize(s));
        ws.mirror_ok = false;
        ps.mirrored = false;
        fprintf(stderr, "[libfsamd] CG progress words in pinned memory not updated by the device: polling the status word by copies\n");
    }
    return FS_OK;
}

// Batches of launches until the recurrence stops or the iteration limit is enqueued.  The host polls a status word behind every
// batch, two batches in flight, or follows the progress words (mirrored): the stream never drains.
static int iterate(const solve_plan& P, pass_state& ps, krylov_ws& ws) {
    hipStream_t s = P.s;
    const bool one = P.fused || ps.fusedp;
    one_launch L = {};
    if (one) FS_CHECK(one_launch_setup(P, ps, ws, L));
    while (!ps.finished) {
        if (ps.mirrored && ps.k > 0) {
            int what = 0;
            FS_CHECK(mirror_look(ps, ws, s, &what));
            if (what == 2) break;
            if (what == 1) continue;
        }
        const int kend = (ps.k + ps.bsz < ps.max_iter + 1) ? ps.k + ps.bsz : ps.max_iter + 1;
        const int k_before = ps.k;
        if (one) FS_CHECK(one_launch_batch(P, ps, ws, L, kend));
        else {
            if (ps.use_graph && ps.graphs_allowed && ps.k >= ps.first_plain && kend - ps.k == ps.bsz && kend <= ps.max_iter) FS_CHECK(run_graph_batch(P, ps, ws, kend));
            for (; ps.k < kend; ++ps.k) FS_CHECK(step(P, ps, ws, ps.k));
        }
        FS_KERNEL_CHECK();
        ps.n_launches += ps.k - k_before;
        if (!ps.mirrored) {
            FS_HIP(hipMemcpyAsync(ws.h_status + 4 * ps.slot, ws.status.p, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
            FS_HIP(hipEventRecord(ws.poll[ps.slot], s));
            if (ps.pending >= 0) {
                FS_HIP(hipEventSynchronize(ws.poll[ps.pending]));
                if (ws.h_status[4 * ps.pending] != 0) ps.finished = true;
            }
            ps.pending = ps.slot;
            ps.slot ^= 1;
        }
        if (ps.k > ps.max_iter) ps.finished = true;
    }
    return FS_OK;
}

// what the pass left open, the true residual, the ONE synchronisation of a pass, what the host learns from it
static int end_pass(const solve_plan& P, pass_state& ps, krylov_ws& ws) {
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    const int64_t n = P.n;
    double* const x = P.x->d.p;
    if (sp->halo.begun) {          // the exchange started for a product that is not coming any more
        FS_CHECK(fs_halo_end_dev(sp, s));
        sp->halo.begun = false;
    }
    // pipelined: the reduction enqueued behind the last update still reads the partial sums on the communication stream;
    // nothing of the workspace is touched again before it is through
    if (ps.red_stream) FS_HIP(hipStreamWaitEvent(s, ws.ev_red, 0));
    // LIGHT / PAIR launches: a pass that stopped in an odd launch owes x one step (the kernel looks at the status word itself)
    if (ps.iteration_form & 1) {
        hipLaunchKernelGGL(k_cg_pair_flush, dim3(fs_grid_for(n / 2 + 1, FS_BLOCK, 2048)), dim3(FS_BLOCK), 0, s, n, ws.status.p, ws.scal.p, ws.z.p, ws.p.p, x);
        FS_KERNEL_CHECK();
    }
    // The end of a pass used to be six host synchronisations (stream, status word, sums, control block, the un-scaling of x,
    // the history): 0.68 ms of fixed cost per solve at 1 M rows, a tenth of the whole solve.  Nothing of the true-residual
    // computation depends on what the host learns from the status word, so it is enqueued first and status, sums and control
    // block come back in ONE synchronisation.
    // true residual b - A x (scaled mode: sum d (bhat - Ahat xhat)^2, the same number)
    FS_HIP(hipMemcpyAsync(ws.z.p, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    FS_CHECK(fs_halo_exchange_dev(sp, ws.z.p, s));
    launch_spmv<0>(P.A, ws.z.p, ws.w.p, nullptr, nullptr, nullptr, s, P.aval);
    if (P.ds) hipLaunchKernelGGL(k_residual_scaled, dim3(P.pgrid), dim3(FS_BLOCK), 0, s, ws.bhat.p, ws.w.p, ws.dvec.p, n, (double*)nullptr, ws.partials.p);
    else hipLaunchKernelGGL(k_residual, dim3(P.pgrid), dim3(FS_BLOCK), 0, s, P.b->d.p, ws.w.p, n, (double*)nullptr, ws.partials.p);
    FS_CHECK(fs_comm_sum_allreduce_dev(ws.partials.p, P.pgrid, 1, ws.sums.p + 5, s));
    FS_HIP(hipMemcpyAsync(ws.h_status + 12, ws.status.p, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemcpyAsync(ws.h_vals, ws.sums.p, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemcpyAsync(ws.h_vals + 8, ws.ctrl.p, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    if (fs_p2p_reduce_enabled()) FS_CHECK(fs_p2p_check(s));
    for (int q = 0; q < 4; ++q) ps.h_status[q] = ws.h_status[12 + q];
    const int iters = ps.h_status[1];
    ps.total_iters += iters;
    // launches enqueued after the recurrence stopped return on the status word: their samples time no-ops
    for (int i = ps.first_sample; i < ps.sm.n; ++i) ws.sample_live[i] = ws.sample_iter[i] + ws.sample_span[i] - 1 < iters;
    if (ws.h_status[8] != 0) {
        fs_set_error("fs_krylov_solve: %d zero%s diagonal entries (Jacobi preconditioner undefined)", ws.h_status[8], P.ds ? " or negative" : "");
        return FS_ERR_NUMERIC;
    }
    ps.true_rr = ws.h_vals[5];
    ps.thresh = ws.h_vals[8];
    ps.bb_host = ws.h_vals[9];
    ++ps.n_pass;
    if (getenv("FS_KRYLOV_DEBUG"))
        fprintf(stderr, "[fs_krylov] pass %d: status %d, %d iterations (total %d), true ||r||^2 %.3e, threshold %.3e\n",
                ps.n_pass, ps.h_status[0], ps.h_status[1], ps.total_iters, ps.true_rr, ps.thresh);
    return FS_OK;
}

// The single-reduction recurrences drift on ill-conditioned operators (the recurrence residual can reach the threshold while
// b - A x has not): the true residual is recomputed after every pass and, if it misses the tolerance, the solve
// restarts from the current x (at most 8 passes, iteration budget shared).
static bool restart_wanted(const solve_plan& P, pass_state& ps) {
    const bool recurrence_converged = ps.h_status[0] == 1;
    if (!recurrence_converged || ps.true_rr <= ps.thresh * 1.0201 || ps.n_pass >= 8 || ps.total_iters >= P.opts->max_iter) return false;
    if (ps.true_rr > 0.7 * ps.prev_true_rr) return false;   // no longer improving: attainable accuracy of fp64 reached
    ps.prev_true_rr = ps.true_rr;
    ps.use_guess = true;   // restart: r := b - A x exactly, then continue
    return true;
}

#ifdef FS_ITER_TIMING
static int dump_iter_timing(const solve_plan& P) {
    fs_space_s* sp = P.sp;
    hipStream_t s = P.s;
    const int igrid = P.igrid;
    std::vector<long long> h(FS_STAMPS * 4096);
    FS_HIP(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_iter_dbg), h.size() * sizeof(long long)));
    long long first = h[0], last = 0;
    for (int b = 0; b < igrid; ++b) { first = std::min(first, h[FS_STAMPS * b]); last = std::max(last, h[FS_STAMPS * b + 7]); }
    double mean[9] = {0}, mx[9] = {0};
    for (int b = 0; b < igrid; ++b)
        for (int k2 = 0; k2 < 9; ++k2) { const double v = (h[FS_STAMPS * b + k2] - first) * 0.01; mean[k2] += v / igrid; mx[k2] = std::max(mx[k2], v); }
    fprintf(stderr, "[iter timing, last launch, us from the first workgroup's start] span %.2f;", (last - first) * 0.01);
    for (int k2 = 0; k2 < 9; ++k2) fprintf(stderr, " s%d mean %.2f max %.2f;", k2, mean[k2], mx[k2]);
    fprintf(stderr, "\n");
    // stamps 5 (first item done), 6 (all items done), 7 (partials summed) apart for the workgroups whose chunks hold an edge item
    // (the chunk walk of the kernel: xcd_chunks, or block-strided without the XCD map) and for the rest
    std::vector<int32_t> hi((size_t)sp->n_dict_items * 4);
    FS_CHECK(sp->dict_items.download(hi.data(), (int64_t)hi.size(), s));
    FS_HIP(hipStreamSynchronize(s));
    const int64_t n_chunks = (sp->n_dict_items + 3) / 4, per_xcd = (n_chunks + 7) >> 3;
    int cnt[2] = {0, 0};
    double gm[2][3] = {{0}}, gx[2][3] = {{0}};
    for (int b = 0; b < igrid; ++b) {
        int64_t cur = b, step = igrid, end = n_chunks;
        if (dict_map_xcd()) { cur = (b & 7) * per_xcd + (b >> 3); step = igrid >> 3; end = std::min<int64_t>(((b & 7) + 1) * per_xcd, n_chunks); }
        int e = 0;
        for (; cur < end; cur += step)
            for (int64_t q = 4 * cur; q < std::min<int64_t>(4 * cur + 4, sp->n_dict_items); ++q) e |= (hi[(size_t)q * 4 + 1] >> 16) & 1;
        ++cnt[e];
        for (int k2 = 0; k2 < 3; ++k2) { const double v = (h[FS_STAMPS * b + 5 + k2] - first) * 0.01; gm[e][k2] += v; gx[e][k2] = std::max(gx[e][k2], v); }
    }
    for (int e = 0; e < 2; ++e) {
        fprintf(stderr, "[iter timing] %d workgroups %s an edge item:", cnt[e], e ? "with" : "without");
        for (int k2 = 0; k2 < 3; ++k2) fprintf(stderr, " s%d mean %.2f max %.2f;", 5 + k2, cnt[e] ? gm[e][k2] / cnt[e] : 0.0, gx[e][k2]);
        fprintf(stderr, "\n");
    }
    return FS_OK;
}
#endif

static void fill_stats(const solve_plan& P, const pass_state& ps, const krylov_ws& ws, std::chrono::steady_clock::time_point t_end, fs_krylov_stats* stats) {
    const int iters = ps.total_iters;
    memset(stats, 0, sizeof(*stats));
    const double bb = ps.bb_host;
    stats->iterations = iters;
    // PETSc semantics: converged = the recurrence residual met the tolerance; the recomputed true
    // residual is reported next to it (restarts keep the two together whenever fp64 allows)
    stats->converged = ps.h_status[0] == 2 ? -1 : (ps.h_status[0] == 1 ? 1 : 0);
    stats->bnorm = sqrt(bb);
    stats->rel_residual = bb > 0.0 ? sqrt(ws.last_hist[iters] / bb) : 0.0;
    stats->true_rel_residual = bb > 0.0 ? sqrt(ps.true_rr / bb) : sqrt(ps.true_rr);
    stats->solve_ms = std::chrono::duration<double, std::milli>(t_end - P.t_begin).count();
    double t_spmv = 0.0, t_upd = 0.0;
    int cnt = 0;
    for (int i = 0; i < ps.sm.n; ++i) {
        if (!ws.sample_live[i]) continue;
        float a = 0.f, c = 0.f;
        if (hipEventElapsedTime(&a, ws.ev[i][0], ws.ev[i][1]) != hipSuccess) break;
        if (hipEventElapsedTime(&c, ws.ev[i][2], ws.ev[i][3]) != hipSuccess) break;
        t_spmv += a / (float)ws.sample_span[i];
        t_upd += c;
        ++cnt;
    }
    if (cnt) {
        stats->spmv_ms = t_spmv / cnt;
        stats->update_ms = t_upd / cnt;
    }
    stats->spmv_bytes = P.sp->nnz_nodes * P.bs * P.bs * 12 + P.n * 20;
    stats->row_classes = g_dict.built_for ? g_dict.ncls : 0;
    stats->fused_iteration = ps.fusedp_used ? 2 : (P.fused ? 1 : 0);
    stats->classes_kept = g_dict.built_for && g_dict.kept ? 1 : 0;
    stats->launches = ps.n_launches;
    stats->product_kind = P.fused ? (P.BI ? 3 : 1) : g_last_product_kind;
    g_last_iteration_form = (P.fused || ps.fusedp_used) ? ps.iteration_form : 0;
    g_last_iteration_runs = (P.fused || ps.fusedp_used) ? ps.iteration_runs : 0;
    if (P.fused) stats->update_ms = 0.0;       // (spmv_ms is the whole iteration: one launch)
}

extern "C" int fs_krylov_solve(fs_matrix_t A, fs_vector_t b, fs_vector_t x, const fs_krylov_opts* opts,
                               fs_krylov_stats* stats) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(fs_require_init());
    FS_REQUIRE(A && b && x && opts, "fs_krylov_solve: null pointer");
    if (fs_is_dg(A->space)) return fs_dg_krylov_solve(A, b, x, opts, stats);
    if (opts->method != FS_KSP_CG && opts->method != FS_KSP_BICGSTAB) {
        fs_set_error("fs_krylov_solve: unknown Krylov method %d", opts->method);
        return FS_ERR_UNSUPPORTED;
    }
    row_dict_scope dict_scope;           // the row dictionary describes the values of ONE solve (built by prepare_solve where it applies)
    FS_REQUIRE(A->bs != 4, "fs_krylov_solve: Taylor-Hood block systems are solved by fs_saddle_solve");
    FS_REQUIRE(opts->precond == FS_PC_NONE || opts->precond == FS_PC_JACOBI, "fs_krylov_solve: unknown preconditioner %d", opts->precond);
    FS_REQUIRE(opts->max_iter > 0 && opts->rtol >= 0.0 && opts->atol >= 0.0, "fs_krylov_solve: bad tolerances");
    fs_space_s* sp = A->space;
    FS_REQUIRE(b->d.n >= sp->n_dofs_owned && x->d.n >= sp->n_dofs_owned, "fs_krylov_solve: b/x shorter than the owned dofs (%lld)", (long long)sp->n_dofs_owned);
    bool in_lattice_order = false;
    FS_CHECK(solve_in_lattice_order(A, b, x, opts, stats, &in_lattice_order));
    if (in_lattice_order) return FS_OK;

    static const krylov_env env;
    krylov_ws& ws = g_ws;
    solve_plan P = {env, A, b, x, opts, sp, fs_rt().stream, sp->n_dofs_owned, sp->n_dofs_local, A->bs};
    P.bicg = opts->method == FS_KSP_BICGSTAB;
    lap_timer lap = {env.solve_timing, P.s};
    FS_CHECK(prepare_solve(P, ws, lap));

    pass_state ps = {sampler{ws, P.s}};
    ps.use_guess = opts->nonzero_guess != 0;
    for (;;) {
        FS_CHECK(begin_pass(P, ps, ws));
        FS_CHECK(iterate(P, ps, ws));
        lap("iterations of the pass");
        FS_CHECK(end_pass(P, ps, ws));
        if (!restart_wanted(P, ps)) break;
    }
    if (P.ds) {   // x = D^-1/2 xhat (no synchronisation of its own: the download of the history below waits for it)
        hipLaunchKernelGGL(k_pointwise_mul, dim3(fs_grid_for(P.n)), dim3(FS_BLOCK), 0, P.s, ws.dinv.p, x->d.p, P.n, x->d.p);
        FS_KERNEL_CHECK();
    }
    const int iters = ps.total_iters;
    if (fs_rt().comm && getenv("FS_COMM_TIMING")) {
        double au, hu; long ac, hc;
        fs_comm_host_time(&au, &ac, &hu, &hc, true);
        fprintf(stderr, "[fs_krylov] host time inside RCCL enqueue calls: all-reduce %.1f us x %ld, grouped send/recv %.1f us x %ld; %d iterations in %.1f ms\n",
                ac ? au / ac : 0.0, ac, hc ? hu / hc : 0.0, hc, iters,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - P.t_begin).count());
    }
#ifdef FS_ITER_TIMING
    if (P.fused && getenv("FS_ITER_TIMING")) FS_CHECK(dump_iter_timing(P));
#endif
    ws.last_hist.resize((size_t)iters + 1);
    FS_CHECK(ws.hist.download(ws.last_hist.data(), iters + 1, P.s));
    if (stats) fill_stats(P, ps, ws, std::chrono::steady_clock::now(), stats);
    if (ps.h_status[0] == 2) {
        fs_set_error("fs_krylov_solve: %s breakdown at iteration %d (operator not SPD / rho = 0 / NaN)", P.bicg ? "BiCGStab" : "CG", iters);
        return FS_ERR_NUMERIC;
    }
    return FS_OK;
}

// (the guard bits have an accessor of their own: callers of fs_last_iteration_form compare the word with PAIR | DTAB)
extern "C" int fs_last_iteration_form() { return g_last_iteration_form & 3; }
extern "C" int fs_last_iteration_guard() { return (g_last_iteration_form >> 2) & 3; }
extern "C" int fs_last_iteration_runs() { return g_last_iteration_runs; }
void fs_krylov_set_history(const std::vector<double>& rr) { g_ws.last_hist = rr; }
void fs_set_last_product_kind(int kind) { g_last_product_kind = kind; }

extern "C" int fs_krylov_history(double* out, int capacity, int* count) {
    const int n = (int)g_ws.last_hist.size();
    if (count) *count = n;
    if (out)
        for (int i = 0; i < n && i < capacity; ++i) out[i] = g_ws.last_hist[i];
    return FS_OK;
}

void fs_krylov_preload() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(k_set_threshold));
    (void)hipGetLastError();
}
