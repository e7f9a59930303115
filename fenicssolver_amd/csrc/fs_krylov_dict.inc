// Part of fs_krylov.hip (included there, one translation unit: the kernels share its file-scope state): the row-dictionary form of scalar DIA operators: plans, class tables (k_dict_insert / compact / finish), the work-item product k_dict_spmv.
// Split out in round 6 (VERDICT r5: a 5 000-line source); nothing here is compiled on its own.

// ---- row-dictionary form of a scalar DIA matrix ---------------------------------------------------------------------------------
// On a uniform box mesh with constant coefficients (BASELINE configs[0] / [1] / [3]: BoxMesh, k = 20) the assembled operator has a
// few dozen (P1) to a few hundred (CG2) DISTINCT rows - interior, the 26 kinds of boundary position, the rows next to Dirichlet
// faces - each repeated bit for bit (the box assembly snaps its edge vectors to the grid spacing, fs_assemble.hip, so that rows are
// translation-invariant).  The product then does not have to stream 8 B per entry: every row carries a 2-byte class number and
// the distinct coefficient rows are fetched per work item.  Built per solve from the values the solver is about to multiply with,
// every row verified bit for bit against its class, so it is lossless and needs no knowledge of where the matrix came from.
//
// Round 4: the product is organised by ROWS, not by the 64-row slices of the value storage it no longer reads.
//   * SEGMENTS (once per space, dict_structure_build): maximal runs of consecutive rows whose (col - row) offset sets are nested in
//     one list - on a box mesh a mesh line (CG2: 107 / 108 rows, every line its own list because the edge classes are numbered with
//     different line lengths) or, where all lines share one list (P1), the whole mesh.  Cut into WORK ITEMS of <= 128 rows.
//   * the segment's offset list is cut into RUNS of up to three consecutive offsets (o, o + 1, o + 2).  A lane holds TWO consecutive
//     rows; for a run starting at o its rows need x[r + o .. r + o + 3]: ONE 16-byte load x[r + o], x[r + o + 1] per lane, the
//     other two values are the NEXT lane's load (DPP wave shift, no LDS); lane 63 has no rows of its own - an item is 126 rows -
//     and loads what lane 62 needs (tests/test_gpu_kernels.py multiplies chains of dependent vectors bit for bit against the
//     streaming product).  3.5 vector-memory instructions per row on the Kuhn stencil
//     instead of the 19 of round 3, whose per-CU address path - not HBM - was the limit (0.27 of the peak on 26 B/row).
//   * a RUN PLAN per segment: rounds of 8 runs (start offset, length); slot 0 of round 0 is the run (0; no coefficients) whose
//     load IS z = x[r], x[r + 1] for the fused dots.  A class row holds its coefficients IN PLAN LAYOUT, [round][run][3], zero where
//     a run is shorter or the row has no such entry: the kernel reads them at fixed positions.  Ascending offsets = the storage
//     order of the streaming kernels, one fma each: same summation order, same bits (the extra terms add +0 * x).
//   * per item, the distinct classes of its rows (a mesh line: interior + the two ends) are copied into the wave's own LDS
//     region (sized for the item with the most classes, counted when the classes are found; at most 64 KB per workgroup) - the
//     dictionary itself may have any size (CG2: 350 KB).
//   * items whose loads could leave [0, n_cols) (first / last mesh plane) gather their four values per run one by one, clamped.
// Measured (tools/probes/dict_pair_probe.hip and profiles/r04_*): P1, 10 M rows: 123 -> 64 us.
constexpr int FS_DICT_CAP = 8192;       // hash slots
constexpr int FS_DICT_MAX = 4096;       // distinct rows accepted
constexpr int FS_DICT_ITEM_ROWS = 126;  // rows per work item: two per lane for lanes 0 .. 62; lane 63 only loads (its pair is what lane 62
                                        // needs from `the next lane`: no separate tail loads)
constexpr int FS_DICT_WHOLE_LDS_BYTES = 32 << 10;   // a dictionary up to this size is held whole by every workgroup
constexpr int FS_DICT_LDS_BYTES = 64 << 10;   // per workgroup: 4 waves x (most distinct classes of any item) x (doubles per class row)
constexpr int FS_DICT_ITEMS_PER_WAVE = 4;   // consecutive items a wave takes when it fetches class rows per item
constexpr int FS_DICT3_RUNS = 4;          // runs whose loads the block-row kernel has in flight at a time
constexpr int FS_DICT_MAX_ROUNDS = 8;   // rounds of 8 runs per plan (192 coefficient positions)

struct dict_plan_round {
    int32_t start[8];       // first offset of each run (0 for an empty slot: a harmless load of x[r], x[r + 1])
    uint8_t len[8];         // 0 .. 3
    uint8_t pad[24];
};
static_assert(sizeof(dict_plan_round) == 64, "one 64-byte scalar load per round");
// Rounds of TWELVE runs (fs_space_s::dict_runs = 12: the lattice-ordered shadow of a CG2 box space, fs_lattice.hip - three quarters
// of its mesh lines have 11 runs + the z run, one round instead of two): the same 64 bytes, 12 starts + 12 lengths.  Code that
// takes the number of runs per round at run time reads a round through these two:
struct dict_plan_round12 {
    int32_t start[12];
    uint8_t len[12];
    uint8_t pad[4];
};
static_assert(sizeof(dict_plan_round12) == 64, "one 64-byte scalar load per round");
__host__ __device__ __forceinline__ int32_t dict_run_start(const dict_plan_round* __restrict__ pl, int NR, int g) {
    return reinterpret_cast<const int32_t*>(pl + g / NR)[g % NR];
}
__host__ __device__ __forceinline__ int dict_run_len(const dict_plan_round* __restrict__ pl, int NR, int g) {
    return (int)(reinterpret_cast<const uint8_t*>(pl + g / NR) + 4 * NR)[g % NR];
}

// Coefficient position (plan layout) of the stored entry with offset o, walking the runs of a plan in ascending order from run g on
// (the entries of a row come in ascending offsets, as the runs do): -1 = the plan has no such offset.
__device__ __forceinline__ int dict_slot_of(const dict_plan_round* __restrict__ pl, int n_runs, int RL, int& g, int32_t o, int NR = 8) {
    while (g < n_runs) {
        const int32_t st = dict_run_start(pl, NR, g);
        const int ln = dict_run_len(pl, NR, g);
        if (ln > 0 && o < st + ln) return o >= st ? RL * g + (o - st) : -1;
        ++g;
    }
    return -1;
}

// One row's stored entries (DIA slice storage: value plane k, offset list of the row's piece of its slice), nonzero values only:
// f(position, value), position = slot * nq + q for component q of an entry's nq = bs * bs values (block entry e, component q at
// q * plane + e).  Returns false when an entry has no position in the plan.
// sc (scalar operators only; may be null): the row is walked as D^-1/2 A D^-1/2 - every stored value v at column r + o becomes
// (v sc[r]) sc[r + o], the expression and the bits of k_scale_copy - so that a matrix can be compared with the kept class table of
// its scaled form WITHOUT writing the scaled copy first (the copy is 300 MB of traffic at 1 M rows, and on the row-dictionary path
// nobody reads it).
template <typename F>
__device__ __forceinline__ bool dict_walk_row(int32_t r, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ dia_ptr,
                                              const int32_t* __restrict__ dia_off, const double* __restrict__ val, int nq, int64_t plane,
                                              const dict_plan_round* __restrict__ pl, int n_runs, int RL, F f,
                                              const double* __restrict__ sc = nullptr, int NR = 8) {
    const int32_t sl = r >> 6, ln = r & 63;
    const int64_t base = slice_ptr[sl];
    const int width = (int)((slice_ptr[sl + 1] - base) >> 6);
    const int32_t dp = dia_ptr[sl];
    const int32_t* __restrict__ op = dia_off + dp + 1 + (ln >= dia_off[dp] ? width : 0);
    const double* __restrict__ vp = val + base + ln;
    bool ok = true;
    if (n_runs == 8 && NR == 8 && nq == 1) {
        // one-round plans of scalar operators (P1): the eight run starts and lengths are wave-uniform - in scalar registers, an
        // entry's position is found by comparing its offset with all of them - and the row is taken eight entries at a time,
        // offsets and values of a batch (and whatever f loads) in flight together; the walk below goes entry by entry, two loads
        // and a branch per step of the plan, each waited for
        int32_t st[8], le[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            st[j] = __builtin_amdgcn_readfirstlane(pl->start[j]);
            le[j] = __builtin_amdgcn_readfirstlane((int)pl->len[j]);
        }
        for (int k0 = 0; k0 < width; k0 += 8) {
            int32_t o[8];
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + u < width ? k0 + u : width - 1;        // (clamped: the loads of a short batch stay inside the row)
                o[u] = op[k];
                v[u] = vp[(int64_t)k * FS_SLICE];
            }
            if (sc) {
                const double sr = sc[r];
                double scol[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) scol[u] = sc[v[u] != 0.0 ? r + o[u] : r];       // (a padded position has no column)
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = v[u] * sr * scol[u];
            }
            int slot[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                slot[u] = -1;
#pragma unroll
                for (int j = 1; j < 8; ++j)              // (run 0 is the z run: no coefficients)
                    if (le[j] > 0 && o[u] >= st[j] && o[u] < st[j] + le[j]) slot[u] = RL * j + (o[u] - st[j]);
                if (k0 + u >= width || v[u] == 0.0) slot[u] = -3;         // nothing stored there
                if (slot[u] == -1) ok = false;                           // a value outside the plan
            }
            if (!ok) return false;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (slot[u] >= 0) f(slot[u], v[u]);
        }
        return true;
    }
    int g = 1;                  // run 0 is the z run
    if (nq == 1) {
        // scalar operators with plans of several rounds (CG2; the lattice order's line plans): offsets, values and scale factors of
        // eight entries in flight together, then the walk along the plan for the eight - the entry-by-entry loop below waits for two
        // or three dependent loads per entry (configs[3]: 3.9 ms per solve for the comparison with the kept table)
        for (int k0 = 0; k0 < width; k0 += 8) {
            int32_t o[8];
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + u < width ? k0 + u : width - 1;
                o[u] = op[k];
                v[u] = vp[(int64_t)k * FS_SLICE];
            }
            bool stored[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) stored[u] = k0 + u < width && v[u] != 0.0;
            if (sc) {
                const double sr = sc[r];
                double scol[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) scol[u] = sc[stored[u] ? r + o[u] : r];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = v[u] * sr * scol[u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (stored[u]) {
                    const int slot = dict_slot_of(pl, n_runs, RL, g, o[u], NR);
                    if (slot < 0) return false;
                    f(slot, v[u]);
                }
        }
        return true;
    }
    for (int k = 0; k < width && ok; ++k) {
        int slot = -2;          // not looked up yet
        for (int q = 0; q < nq; ++q) {
            double v = vp[(int64_t)k * FS_SLICE + (int64_t)q * plane];
            if (v == 0.0) continue;
            if (sc) v = v * sc[r] * sc[r + op[k]];
            if (slot == -2) slot = dict_slot_of(pl, n_runs, RL, g, op[k], NR);
            if (slot < 0) { ok = false; break; }
            f(slot * nq + q, v);
        }
    }
    return ok;
}

__device__ __forceinline__ unsigned long long dict_mix(unsigned long long h, int slot, double v) {
    h = (h ^ (unsigned long long)__double_as_longlong(v)) * 1099511628211ull;
    h = (h ^ (unsigned long long)(unsigned)slot) * 1099511628211ull;
    return h ^ (h >> 29);
}

// info[0] = classes found, info[1] = 1: gave up (too many classes), info[2] = rows that differ from their class or do not fit their
// plan (verification), info[3] = most distinct classes in any item, info[4] = rows whose dot weight differs from their class's
// dvec (may be null; scalar operators): the dot weights of the solve, one per row - the row that founds a class leaves its weight in
// slot_d, k_dict_compact numbers it into dtab, k_dict_finish compares every row's weight with dtab[class] bit for bit
// Nearly all rows of such an operator carry the SAME hash, so the table is hit where it hurts: the lanes of a wave are first grouped
// by hash (a wave of interior rows is one group) and only the group's first lane goes to memory, and it looks at the slot with an
// ordinary cached load before any atomic (a slot goes from 0 to its final key once: a key seen there is final, a stale 0 merely
// sends the lane to the compare-and-swap, which returns the truth).
__global__ void __launch_bounds__(FS_BLOCK) k_dict_insert(int64_t n_items, const int4* __restrict__ items, const dict_plan_round* __restrict__ plans,
                                                          const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ dia_ptr,
                                                          const int32_t* __restrict__ dia_off, const double* __restrict__ val, int nq, int64_t plane, int S, int RL,
                                                          unsigned long long* keys, const unsigned long long* keys_cached, double* slot_vals,
                                                          uint16_t* __restrict__ cls_slot, int* info, int NR = 8,
                                                          const double* __restrict__ dvec = nullptr, double* __restrict__ slot_d = nullptr) {
    const int lane = threadIdx.x & 63;
    int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (; q < n_items; q += stride) {
        if (__hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
        const int4 it = items[q];
        const int32_t first = it.x, nr = it.y & 0xffff;
        const dict_plan_round* __restrict__ pl = plans + it.z;
        const int n_runs = NR * it.w;
        for (int half = 0; half < 2; ++half) {
            const int i = half * 64 + lane;
            const bool live = i < nr;
            const int32_t r = first + i;
            unsigned long long h = 1469598103934665603ull;
            bool fits = true;
            if (live) fits = dict_walk_row(r, slice_ptr, dia_ptr, dia_off, val, nq, plane, pl, n_runs, RL, [&](int slot, double v) { h = dict_mix(h, slot, v); }, nullptr, NR);
            if (!h) h = 1ull;
            if (live && !fits) atomicAdd(&info[2], 1);
            int my_slot = 0;
            unsigned long long todo = __ballot(live);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const unsigned long long hl = ((unsigned long long)(unsigned)__shfl((int)(h >> 32), leader, 64) << 32) |
                                              (unsigned long long)(unsigned)__shfl((int)(h & 0xffffffffull), leader, 64);
                const bool mine = live && h == hl;
                int slot = (int)(hl & (FS_DICT_CAP - 1));
                if (lane == leader) {
                    for (int probe = 0; probe < FS_DICT_CAP; ++probe) {
                        unsigned long long old = keys_cached[slot];
                        if (old != hl) {
                            old = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (old == 0ull) old = atomicCAS(&keys[slot], 0ull, hl);
                            if (old == 0ull) {                  // this row is the representative of a new class
                                if (atomicAdd(&info[0], 1) >= FS_DICT_MAX) __hip_atomic_store(&info[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                double* __restrict__ dst = slot_vals + (int64_t)slot * S;       // (zero-filled by the host before the launch)
                                (void)dict_walk_row(r, slice_ptr, dia_ptr, dia_off, val, nq, plane, pl, n_runs, RL, [&](int sl2, double v) { if (sl2 < S) dst[sl2] = v; }, nullptr, NR);
                                if (dvec) slot_d[slot] = dvec[r];
                                break;
                            }
                        }
                        if (old == hl) break;
                        slot = (slot + 1) & (FS_DICT_CAP - 1);
                    }
                }
                slot = __shfl(slot, leader, 64);
                if (mine) my_slot = slot;
                todo &= ~__ballot(mine);
            }
            if (live) cls_slot[r] = (uint16_t)my_slot;
        }
    }
}

// number the occupied slots; values[id][S] = the class rows in plan layout, nnz[id] = their nonzero positions
// info[5] (run_width > 0): bit j set = some class row holds a coefficient above 2^-53 in magnitude in run j of its plan (run_width doubles
// per run; runs from 30 on share bit 30).  The class rows of a scalar operator are rows of D^-1/2 A D^-1/2, unit diagonal: a run whose bit
// stays clear adds less than half an ulp of the diagonal term to any row's product (k_dict_cg_iter, ZRUNS)
__global__ void __launch_bounds__(1024) k_dict_compact(const unsigned long long* __restrict__ keys, const double* __restrict__ slot_vals,
                                                       int S, int32_t* __restrict__ slot2cls, double* __restrict__ values, int32_t* __restrict__ nnz,
                                                       const double* __restrict__ slot_d = nullptr, double* __restrict__ dtab = nullptr,
                                                       int* __restrict__ info = nullptr, int run_width = 0) {
    constexpr int PER = FS_DICT_CAP / 1024;       // consecutive slots per thread
    __shared__ int cnt[1024];
    const int t = threadIdx.x;
    int mine = 0;
    for (int q = 0; q < PER; ++q) mine += keys[t * PER + q] != 0ull;
    cnt[t] = mine;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {       // inclusive scan
        const int v = t >= off ? cnt[t - off] : 0;
        __syncthreads();
        cnt[t] += v;
        __syncthreads();
    }
    int id = cnt[t] - mine;
    for (int q = 0; q < PER; ++q) {
        const int slot = t * PER + q;
        const bool used = keys[slot] != 0ull;
        slot2cls[slot] = used ? id : -1;
        if (used && id < FS_DICT_MAX) {
            int nz = 0, runs = 0;
            for (int k = 0; k < S; ++k) {
                const double v = slot_vals[(int64_t)slot * S + k];
                values[(int64_t)id * S + k] = v;
                nz += v != 0.0;
                if (run_width > 0 && fabs(v) > 0x1p-53) runs |= 1 << (k / run_width < 30 ? k / run_width : 30);
            }
            nnz[id] = nz;
            if (runs) atomicOr(&info[5], runs);
            if (slot_d) dtab[id] = slot_d[slot];
        }
        id += used;
    }
}

// class numbers; EVERY row against its class, bit for bit (a hash collision ends here); the distinct classes of every item counted
__global__ void __launch_bounds__(FS_BLOCK) k_dict_finish(int64_t n_items, const int4* __restrict__ items, const dict_plan_round* __restrict__ plans,
                                                          const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ dia_ptr,
                                                          const int32_t* __restrict__ dia_off, const double* __restrict__ val, int nq, int64_t plane, int S, int RL,
                                                          const int32_t* __restrict__ slot2cls, const double* __restrict__ values,
                                                          const int32_t* __restrict__ nnz, const uint16_t* __restrict__ cls_slot,
                                                          uint16_t* __restrict__ cls, int* info, const double* __restrict__ sc = nullptr, int NR = 8,
                                                          const double* __restrict__ dvec = nullptr, const double* __restrict__ dtab = nullptr) {
    const int lane = threadIdx.x & 63;
    int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    int bad = 0, bad_d = 0, crowded = 0;       // (crowded: most distinct classes of an item so far)
    for (; q < n_items; q += stride) {
        const int4 it = items[q];
        const int32_t first = it.x, nr = it.y & 0xffff;
        const dict_plan_round* __restrict__ pl = plans + it.z;
        const int n_runs = NR * it.w;
        int id2[2] = {-1, -1};
        for (int half = 0; half < 2; ++half) {
            const int i = half * 64 + lane;
            if (i >= nr) continue;
            const int32_t r = first + i;
            const int id = slot2cls[cls_slot[r]];
            cls[r] = (uint16_t)(id < 0 ? 0 : id);
            if (id < 0 || id >= FS_DICT_MAX) { ++bad; continue; }
            id2[half] = id;
            if (dvec) bad_d += __double_as_longlong(dvec[r]) != __double_as_longlong(dtab[id]);
            const double* __restrict__ dv = values + (int64_t)id * S;
            int nz = 0, diff = 0;
            const bool fits = dict_walk_row(r, slice_ptr, dia_ptr, dia_off, val, nq, plane, pl, n_runs, RL, [&](int slot, double v) {
                ++nz;
                diff += slot >= S || __double_as_longlong(v) != __double_as_longlong(dv[slot < S ? slot : 0]);
            }, sc, NR);
            bad += !fits || diff != 0 || nz != nnz[id];
        }
        // distinct classes among the item's rows (what its wave will have to hold in LDS)
        int distinct = 0;
        unsigned long long m0 = __ballot(id2[0] >= 0), m1 = __ballot(id2[1] >= 0);
        while (m0 | m1) {
            const bool from0 = m0 != 0ull;
            const int src = __ffsll((long long)(from0 ? m0 : m1)) - 1;
            const int cv = __shfl(from0 ? id2[0] : id2[1], src, 64);
            m0 &= ~__ballot(id2[0] == cv);
            m1 &= ~__ballot(id2[1] == cv);
            ++distinct;
        }
        crowded = distinct > crowded ? distinct : crowded;
    }
    if (bad) atomicAdd(&info[2], bad);
    if (bad_d) atomicAdd(&info[4], bad_d);
    // (a look before the atomic: nearly every wave holds the same maximum, and 8 000 atomics on one address were most of this
    // kernel's time at 1 M rows)
    if (crowded && lane == 0 && crowded > __hip_atomic_load(&info[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&info[3], crowded);
}

// the next lane's value (DPP wave shift, no LDS); lane 63, which has no next lane, owns no rows
__device__ __forceinline__ double fs_from_next_lane(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// n doubles (n even, both 16-byte aligned) global -> LDS by the whole workgroup: batches of four 16-byte loads per thread, all four
// in flight before the first LDS store (the plain loop `for i: lds[i] = g[i]` compiles to one load - wait - store per trip:
// eight dependent round trips for the 15 KB dictionary of a P1 box, about 4 us at the head of every launch)
__device__ __forceinline__ void fs_fill_lds(double* __restrict__ lds, const double* __restrict__ g, int n) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    const int n2 = n >> 1;
    const v2d* __restrict__ g2 = reinterpret_cast<const v2d*>(g);
    v2d* __restrict__ l2 = reinterpret_cast<v2d*>(lds);
    for (int base = 0; base < n2; base += 4 * FS_BLOCK) {
        v2d t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * FS_BLOCK + (int)threadIdx.x;
            t[u] = g2[i < n2 ? i : n2 - 1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * FS_BLOCK + (int)threadIdx.x;
            if (i < n2) l2[i] = t[u];
        }
    }
}

// The same copy with direct-to-LDS loads (global_load_lds_dwordx4, as fs_box.h uses them: no data registers, no ds_write pass), in two
// halves: ISSUE, which waits for nothing, and WAIT.  The layout stays linear: lane l of wave w moves chunk 256 t + 64 w + l in trip t
// (the LDS side of the instruction is a wave-uniform base + B l); the lanes past the end of a partial last instruction are masked
// off.  B = 16: n even, both sides 16-byte aligned; B = 4: any n (a table of n doubles that need not be even: 2 n chunks).
// Nothing may be scheduled in front of the issue (the wait below counts the vector loads BEHIND it).
template <int B = 16>
__device__ __forceinline__ void fs_fill_lds_issue(double* lds, const double* __restrict__ g, int n) {
    static_assert(B == 16 || B == 4, "dwordx4 or dword");
    const int nc = B == 16 ? n >> 1 : 2 * n;
    const int lane = threadIdx.x & 63;
    const int w64 = __builtin_amdgcn_readfirstlane((int)threadIdx.x & ~63);
    const char* g8 = reinterpret_cast<const char*>(g);
    char* l8 = reinterpret_cast<char*>(lds);
    for (int base = w64; base < nc; base += FS_BLOCK)
        if (base + lane < nc) {             // (the size is an immediate of the instruction: a literal)
            const auto* src = (const __attribute__((address_space(1))) void*)(g8 + (int64_t)(base + lane) * B);
            auto* dst = (__attribute__((address_space(3))) void*)(l8 + base * B);
            if (B == 16) __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
            else __builtin_amdgcn_global_load_lds(src, dst, 4, 0, 0);
        }
    __builtin_amdgcn_sched_barrier(0);
}
// This wave's direct-to-LDS loads have landed: vector loads return in order, so they have once at most AFTER of the vector loads issued
// behind them are outstanding (AFTER must not exceed the number of loads the wave has issued since; 0 is always right).  The compiler
// does not know the LDS side of the builtin: every wave waits for its own loads before the barrier that publishes the copy, and before
// it leaves the kernel.
template <int AFTER>
__device__ __forceinline__ void fs_fill_lds_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AFTER) : "memory");
}

// the same by ONE wave (a class row of n2 16-byte pairs into the wave's LDS region): four loads in flight per lane and batch
__device__ __forceinline__ void fs_wave_copy_pairs(double* __restrict__ lds, const double* __restrict__ g, int n2, int lane) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    const v2d* __restrict__ g2 = reinterpret_cast<const v2d*>(g);
    v2d* __restrict__ l2 = reinterpret_cast<v2d*>(lds);
    for (int base = 0; base < n2; base += 256) {
        v2d t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * 64 + lane;
            t[u] = g2[i < n2 ? i : n2 - 1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * 64 + lane;
            if (i < n2) l2[i] = t[u];
        }
    }
}

// item: x = first row, y = rows (1 .. 126) | edge << 16, z = first plan round, w = rounds.  S = doubles per class row (8 RL per round
// of the longest plan of the space), C = class rows a wave's LDS region holds.  Dynamic LDS: 4 waves x C x S doubles.
// LDSD: the whole dictionary fits the workgroup's LDS (P1: 78 class rows of 24 doubles) - loaded once per workgroup, a row's
// coefficients sit at class * S; otherwise (CG2: 361 rows of 120) each item's classes are copied into its wave's region.
// RL: longest run of the space's plans (coefficient positions per run): 3 on P1 Kuhn meshes (runs of 2, 2, 2, 3, 2, 2, 2), 2 on CG2
// spaces, where 67 % of the runs are one offset long, 32 % two and 0.5 % three (those are cut in two): a third fewer fmas and LDS
// reads on padded positions, one DPP shift per run instead of two.
// NR: runs per plan round (8; 12 on the lattice-ordered shadow of a CG2 box space: twelve 16-byte loads in flight per lane and round)
template <int DOTS, bool LDSD, int RL, int NR = 8>
__global__ void __launch_bounds__(FS_BLOCK) k_dict_spmv(int64_t n_cols, int64_t n_items, const int4* __restrict__ items,
                                                        const dict_plan_round* __restrict__ plans, const uint16_t* __restrict__ cls,
                                                        const double* __restrict__ dict, int S, int C,
                                                        const double* __restrict__ x, double* __restrict__ y,
                                                        const double* __restrict__ rvec, double* __restrict__ partials,
                                                        int* __restrict__ status, int part_base, int part_stride, int bump, int map_xcd) {
    // (the status word is asked for now and looked at after the dictionary's loads have gone out: one round trip instead of two)
    const int st0 = DOTS ? status[0] : 0;
    typedef double v2d __attribute__((ext_vector_type(2)));
    typedef double v2du __attribute__((ext_vector_type(2), aligned(8)));
    extern __shared__ __attribute__((aligned(16))) double sdict[];
    __shared__ double lds4[4];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    double* __restrict__ wl = LDSD ? sdict : sdict + (int64_t)wave * C * S;
    if (LDSD) fs_fill_lds(sdict, dict, C * S);      // (C = number of classes here)
    if (DOTS) {
        if (st0 != 0) return;
        if (bump && blockIdx.x == 0 && threadIdx.x == 0) status[2] += 1;      // see k_sell_spmv
    }
    if (LDSD) __syncthreads();
    double d_rz = 0.0, d_wz = 0.0, d_rr = 0.0;
    // A wave takes K CONSECUTIVE items of a chunk of 4 K: with per-item class rows (!LDSD) neighbouring mesh lines hold the same
    // classes, and a class row already in the wave's region (tagv: lane k knows which class slot k holds) is not fetched again.
    constexpr int K = LDSD ? 1 : FS_DICT_ITEMS_PER_WAVE;
    const int64_t n_chunks = (n_items + 4 * K - 1) / (4 * K);
    const int32_t cmax = (int32_t)(n_cols - 1);
    chunk_iter it = xcd_chunks(n_chunks);
    if (!map_xcd) { it.cur = blockIdx.x; it.step = gridDim.x; it.end = n_chunks; }
    int tagv = -1, rr = 0;
    const unsigned long long cmask = C >= 64 ? ~0ull : ((1ull << C) - 1ull);
    for (; it.cur < it.end; it.cur += it.step)
    for (int kk = 0; kk < K; ++kk) {
        const int64_t q = (it.cur * 4 + wave) * K + kk;
        if (q >= n_items) break;
        const int4 ds = items[__builtin_amdgcn_readfirstlane((int)q)];
        const int32_t first = __builtin_amdgcn_readfirstlane(ds.x);
        const int nr = __builtin_amdgcn_readfirstlane(ds.y) & 0xffff;
        const int edge = __builtin_amdgcn_readfirstlane(ds.y) >> 16;
        const dict_plan_round* __restrict__ pl = plans + __builtin_amdgcn_readfirstlane(ds.z);
        const int rounds = __builtin_amdgcn_readfirstlane(ds.w);
        const int32_t r = first + 2 * lane;
        const bool ok0 = 2 * lane < nr, ok1 = 2 * lane + 1 < nr;
        v2d ri = {0.0, 0.0};
        if (DOTS && DOTS != 4) {
            if (ok1) ri = *reinterpret_cast<const v2du*>(&rvec[r]);
            else if (ok0) ri.x = rvec[r];
        }
        int c0 = -1, c1 = -1;
        if ((first & 1) == 0) {        // (wave-uniform) the two class numbers of a lane in one 4-byte load (the array is padded)
            const uint32_t two = *reinterpret_cast<const uint32_t*>(&cls[r]);
            if (ok0) c0 = (int)(two & 0xffffu);
            if (ok1) c1 = (int)(two >> 16);
        } else {
            if (ok0) c0 = (int)cls[r];
            if (ok1) c1 = (int)cls[r + 1];
        }
        // the x values of the first round are asked for before anything waits for the class numbers.  Items whose accesses could leave
        // [0, n_cols) (first / last rows of the vector) load the two values of a pair one by one, each clamped into x: a column
        // outside the vector has no entry, hence a zero coefficient, and every value inside it is the right one.
        const double* __restrict__ xr = x + r;
        v2d A[NR];
        struct starts8 { int32_t v[NR]; };
        auto read_starts = [&](const dict_plan_round* __restrict__ p) {       // (wave-uniform: one 32-byte scalar load)
            starts8 t;
#pragma unroll
            for (int j = 0; j < NR; ++j) t.v[j] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int32_t*>(p)[j]);
            return t;
        };
        auto load_round = [&](v2d (&buf)[NR], const starts8& st) {
            if (!edge) {
#pragma unroll
                for (int j = 0; j < NR; ++j) buf[j] = *reinterpret_cast<const v2du*>(xr + st.v[j]);
            } else {
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int32_t c = r + st.v[j];
                    buf[j].x = x[c < 0 ? 0 : (c > cmax ? cmax : c)];
                    buf[j].y = x[c + 1 < 0 ? 0 : (c + 1 > cmax ? cmax : c + 1)];
                }
            }
        };
        load_round(A, read_starts(pl));
        // (per-item class rows = CG2: the run starts of a plan are the line's own - 20 MB of plans streamed once per product - and
        // the NEXT round's are asked for a round ahead, so that a round's loads wait for one memory round trip, not two: 196 ->
        // 187 us.  It costs 20 VGPRs (the compiler forms the next round's addresses early): not done where the dictionary sits whole
        // in LDS - P1, one round -, which it took from 6 to 4 waves per SIMD, 68 -> 78 us)
        starts8 st_next = read_starts(pl + ((!LDSD && rounds > 1) ? 1 : 0));
        int b0 = 0, b1 = 0;
        if (LDSD) {
            b0 = ok0 ? c0 * S : 0;
            b1 = ok1 ? c1 * S : 0;
        } else {
            // ---- the classes of this item's rows -> the wave's LDS region (C slots), unless they are there already ----
            unsigned long long inuse = 0ull;
            bool copied = false;
            unsigned long long m0 = __ballot(ok0), m1 = __ballot(ok1);
            while (m0 | m1) {
                const bool from0 = m0 != 0ull;
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)(from0 ? m0 : m1)) - 1);
                const int cv = __builtin_amdgcn_readlane(from0 ? c0 : c1, src);
                const unsigned long long hit = __ballot(tagv == cv) & cmask;
                int slot;
                if (hit) slot = __ffsll((long long)hit) - 1;
                else {
                    // victim: the first slot from the round-robin pointer on that this item does not use (there is one: C is the
                    // largest number of classes any item has)
                    const unsigned long long freeb = ~inuse & cmask, ahead = freeb & ~((1ull << rr) - 1ull);
                    slot = __ffsll((long long)(ahead ? ahead : freeb)) - 1;
                    rr = slot + 1 == C ? 0 : slot + 1;
                    fs_wave_copy_pairs(wl + slot * S, dict + (int64_t)cv * S, S >> 1, lane);
                    if (lane == slot) tagv = cv;
                    copied = true;
                }
                inuse |= 1ull << slot;
                const bool h0 = c0 == cv, h1 = c1 == cv;
                if (h0) b0 = slot * S;
                if (h1) b1 = slot * S;
                m0 &= ~__ballot(h0);
                m1 &= ~__ballot(h1);
            }
            if (copied) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        const double* __restrict__ v0 = wl + b0;
        const double* __restrict__ v1 = wl + b1;
        double a0 = 0.0, a1 = 0.0;
        v2d zi = {0.0, 0.0};
        // (measured and not kept, CG2 n = 107, product 204 us: the next round's loads in flight while this one is multiplied - a
        // second register set, 138 VGPRs, 3 waves per SIMD: 270 us; only the terms a run's length calls for, by wave-uniform branches
        // - most CG2 runs are one or two offsets long - : 339 us, the branches keep the coefficient reads from being batched)
        auto compute_round = [&](const v2d (&buf)[NR], int rd) {
            const double* __restrict__ w0 = v0 + NR * RL * rd;
            const double* __restrict__ w1 = v1 + NR * RL * rd;
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const double e0 = buf[j].x, e1 = buf[j].y;
                const double e2 = fs_from_next_lane(buf[j].x);
                a0 = fma(w0[RL * j], e0, a0);     a1 = fma(w1[RL * j], e1, a1);
                a0 = fma(w0[RL * j + 1], e1, a0); a1 = fma(w1[RL * j + 1], e2, a1);
                if (RL == 3) {
                    const double e3 = fs_from_next_lane(buf[j].y);
                    a0 = fma(w0[RL * j + 2], e2, a0); a1 = fma(w1[RL * j + 2], e3, a1);
                }
                // (the coefficient positions are compile-time constants: left alone the compiler reads all 48 of a round
                // ahead of the first fma - 150 VGPRs, 3 waves per SIMD; a compiler barrier per run keeps it at the run's six)
                asm volatile("" ::: "memory");
            }
        };
        for (int rd = 0; rd < rounds; ++rd) {
            if (rd > 0) {
                if (LDSD) load_round(A, read_starts(pl + rd));
                else {
                    load_round(A, st_next);
                    st_next = read_starts(pl + (rd + 1 < rounds ? rd + 1 : rd));
                }
            }
            compute_round(A, rd);
            if (rd == 0) zi = A[0];
        }
        if (ok1) {
            v2d out;
            out.x = a0; out.y = a1;
            *reinterpret_cast<v2du*>(&y[r]) = out;
        } else if (ok0) y[r] = a0;
        if (!ok0) { a0 = 0.0; zi.x = 0.0; }
        if (!ok1) { a1 = 0.0; zi.y = 0.0; }
        if (DOTS == 1) {
            d_rz += ri.x * zi.x + ri.y * zi.y; d_wz += a0 * zi.x + a1 * zi.y; d_rr += ri.x * ri.x + ri.y * ri.y;
        } else if (DOTS == 2) {
            d_rz += a0 * ri.x + a1 * ri.y; d_wz += a0 * a0 + a1 * a1; d_rr += ri.x * ri.x + ri.y * ri.y;
        } else if (DOTS == 3) {
            d_rz += zi.x * zi.x + zi.y * zi.y; d_wz += a0 * zi.x + a1 * zi.y; d_rr += ri.x * zi.x * zi.x + ri.y * zi.y * zi.y;
        }
        if (!LDSD) __builtin_amdgcn_wave_barrier();            // (the next item's class rows may overwrite this one's)
    }
    if (DOTS && DOTS != 4) {
        const double t0 = fs_block_sum(d_rz, lds4);
        const double t1 = fs_block_sum(d_wz, lds4);
        const double t2 = fs_block_sum(d_rr, lds4);
        if (threadIdx.x == 0) {
            partials[part_base + blockIdx.x] = t0;
            partials[part_stride + part_base + blockIdx.x] = t1;
            partials[2 * part_stride + part_base + blockIdx.x] = t2;
        }
    }
}

