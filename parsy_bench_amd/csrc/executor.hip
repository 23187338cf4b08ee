// Plan construction, upload and launch sequencing (host side of the HIP executor).
#include "executor.hpp"

#include <climits>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "cond.hpp"
#include "device_util.hpp"
#include "errors.hpp"
#include "hip_check.hpp"
#include "plan_fwd.hpp"
#include "plan_util.hpp"
#include "refine.hpp"
#include "feature_states.hpp"

namespace parsy {

const Schedule& plan_schedule(const parsy_plan* plan) { return plan->S; }

int check_plan(const parsy_plan* pl, const char* who, PlanNeeds needs) {
    const std::string w(who);
    if (pl->device < 0) return set_last_error(w + ": plan was built without a device (device < 0)"), -1;
    if (needs == kNeedsDevice) return 0;
    if (pl->solve_only) return set_last_error(w + ": plan was built from L's pattern only (no A pattern)"), -1;
    if (needs == kNeedsA) return 0;
    if (pl->sn_mask_set || pl->piece_mask_set)
        return set_last_error(w + ": plan is restricted by parsy_plan_set_active / _set_active_pieces"), -1;
    if (pl->factor_open) return set_last_error(w + ": a factorization is still open (parsy_factor_begin)"), -1;
    if (pl->levels_open) return set_last_error(w + ": a solve in steps of levels is still open"), -1;
    return 0;
}

int plan_set_perm(parsy_plan* pl, const int* perm) {
    const int n = pl->S.n;
    std::vector<int> p;
    if (perm) {
        p.assign(perm, perm + n);
        std::vector<char> seen((size_t)n, 0);
        for (int v : p) {
            if (v < 0 || v >= n || seen[v])
                return set_last_error("parsy_plan_set_perm: perm is not a permutation of 0..n-1"), -1;
            seen[v] = 1;
        }
    }
    if (pl->d_perm.data()) {
        (void)hipSetDevice(pl->device);
        (void)hipDeviceSynchronize();   // (a call may still read the old one)
        (void)pl->d_perm.reset();
    }
    pl->perm_on_device = false;
    pl->perm.swap(p);
    pl->perm_inv.clear();
    return 0;
}

const std::vector<int>& plan_perm_inverse(parsy_plan* pl) {
    if (pl->perm_inv.size() != pl->perm.size()) {
        pl->perm_inv.resize(pl->perm.size());
        for (size_t i = 0; i < pl->perm.size(); ++i) pl->perm_inv[(size_t)pl->perm[i]] = (int)i;
    }
    return pl->perm_inv;
}

int plan_perm_device(parsy_plan* pl, const int** out) {
    *out = nullptr;
    if (pl->perm.empty()) return 0;
    if (!pl->perm_on_device) {
        PARSY_HIP(pl->d_perm.grow((int64_t)pl->perm.size()));
        PARSY_HIP(hipMemcpy(pl->d_perm.data(), pl->perm.data(), pl->perm.size() * 4, hipMemcpyHostToDevice));
        pl->perm_on_device = true;
    }
    *out = pl->d_perm.data();
    return 0;
}

// ---- n x nrhs operands between the caller's ordering and the plan's own (plan_util.hpp) ----
constexpr int kPermThreads = 256;

// dst[k, q] = src[perm[k], q] (dst leading dimension n; a second copy into dst2 when given)
__global__ __launch_bounds__(kPermThreads) void k_perm_gather(const int* __restrict__ perm,
                                                                     const double* __restrict__ src, int64_t ld, int n,
                                                                     int nrhs, double* __restrict__ dst,
                                                                     double* __restrict__ dst2) {
    const int64_t k = (int64_t)blockIdx.x * kPermThreads + threadIdx.x;
    if (k >= n) return;
    const int64_t s = perm ? perm[k] : k;
    for (int64_t q = blockIdx.y; q < nrhs; q += gridDim.y) {
        const double v = src[s + q * ld];
        dst[k + q * n] = v;
        if (dst2) dst2[k + q * n] = v;
    }
}

// dst[perm[k], q] = beta dst[perm[k], q] + alpha src[k, q] (src leading dimension n)
__global__ __launch_bounds__(kPermThreads) void k_perm_scatter(const int* __restrict__ perm,
                                                                      const double* __restrict__ src, int n, int nrhs,
                                                                      double alpha, double beta, double* __restrict__ dst,
                                                                      int64_t ld) {
    const int64_t k = (int64_t)blockIdx.x * kPermThreads + threadIdx.x;
    if (k >= n) return;
    const int64_t d = perm ? perm[k] : k;
    for (int64_t q = blockIdx.y; q < nrhs; q += gridDim.y) store_y(dst + d + q * ld, alpha, beta, src[k + q * n]);
}

// a thread per row, the columns strided over the grid's y (any nrhs >= 1)
static dim3 perm_grid(int n, int nrhs) {
    return dim3((unsigned)((n + kPermThreads - 1) / kPermThreads), (unsigned)(nrhs < 65535 ? nrhs : 65535));
}

void enqueue_perm_gather(const int* perm, const double* src, int64_t ld, double* dst, double* dst2, int n,
                                       int nrhs, hipStream_t stream) {
    if (n > 0)
        hipLaunchKernelGGL(k_perm_gather, perm_grid(n, nrhs), dim3(kPermThreads), 0, stream, perm, src, ld, n, nrhs, dst,
                           dst2);
}

void enqueue_perm_scatter(const int* perm, const double* src, double alpha, double beta, double* dst,
                                        int64_t ld, int n, int nrhs, hipStream_t stream) {
    if (n > 0)
        hipLaunchKernelGGL(k_perm_scatter, perm_grid(n, nrhs), dim3(kPermThreads), 0, stream, perm, src, n, nrhs, alpha,
                           beta, dst, ld);
}

EventTimer::~EventTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
}

bool EventTimer::start() {
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return false;
    (void)hipEventRecord(e0, nullptr);   // (a failure shows in stop(): the elapsed time cannot be read)
    return true;
}

bool EventTimer::stop(double* seconds) {
    float ms = 0;
    if (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
        hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
        return false;
    if (seconds) *seconds = ms * 1e-3;
    return true;
}

// a pattern or launch array of the plan: the plan owns the block (freed with the plan, or with the launch arrays)
template <typename T>
static int upload(parsy_plan* pl, const std::vector<T>& v, const T*& dptr, bool launch_array) {
    DevicePool& pool = launch_array ? pl->launches : pl->pattern;
    dptr = pool.upload(v);
    return dptr ? 0 : pool_failed(pool);
}

int plan_upload_launches(parsy_plan* pl) {
    if (pl->device < 0) return 0;
    PARSY_HIP(hipSetDevice(pl->device));
    pl->launches.clear();
    pl->levels_open = false;
    const Schedule& S = pl->S;
    if (upload(pl, S.small_list, pl->dp.small_list, true)) return -1;
    if (upload(pl, S.small_ranges, pl->dp.small_ranges, true)) return -1;
    if (upload(pl, S.solve_small_ranges, pl->dp.solve_small_ranges, true)) return -1;
    if (upload(pl, S.bsolve_ranges, pl->dp.bsolve_ranges, true)) return -1;
    if (upload(pl, S.tiles, pl->dp.tiles, true)) return -1;
    if (upload(pl, S.big_tasks, pl->dp.big_tasks, true)) return -1;
    if (upload(pl, S.solve_small_list, pl->dp.solve_small_list, true)) return -1;
    if (upload(pl, S.solve_panels, pl->dp.solve_panels, true)) return -1;
    if (upload(pl, S.solve_mtasks, pl->dp.solve_mtasks, true)) return -1;
    if (upload(pl, S.solve_fix_list, pl->dp.solve_fix_list, true)) return -1;
    if (upload(pl, S.solve_wide_list, pl->dp.solve_wide_list, true)) return -1;
    if (upload(pl, S.bsolve_blocks, pl->dp.bsolve_blocks, true)) return -1;
    if (upload(pl, S.bsolve_below, pl->dp.bsolve_below, true)) return -1;
    (void)pl->bpart.reset();   // (sized by the launch lists)
    pl->dp.bpart = nullptr;
    if (upload(pl, S.bsolve_pairs, pl->dp.bsolve_pairs, true)) return -1;
    if (upload(pl, S.sub_members, pl->dp.sub_members, true) || upload(pl, S.sub_trees, pl->dp.sub_trees, true) ||
        upload(pl, S.sub_slots, pl->dp.sub_slots, true) || upload(pl, S.sub_out_rows, pl->dp.sub_out_rows, true))
        return -1;
    // (trees whose workgroup would not get its LDS: the subtree launches keep the level kernels' form)
    pl->route_rt.sub_ntiers = (!S.sub_tiers.empty() && solve_sub_prepare(S.sub_max_slots) == 0) ? (int)S.sub_tiers.size() : 0;
    {
        auto up = [&](const Schedule::OneLists& O, DevicePattern::OneDev& D) {
            D = DevicePattern::OneDev();
            if (upload(pl, O.sn, D.sn, true) || upload(pl, O.slot0, D.slot0, true) || upload(pl, O.wleft, D.wleft, true) ||
                upload(pl, O.pull_ptr, D.pull_ptr, true) || upload(pl, O.pull_slot, D.pull_slot, true) ||
                upload(pl, O.pull_pos, D.pull_pos, true))
                return -1;
            D.nblocks = (int)O.sn.size();
            D.nslots = std::max<int64_t>(O.nslots, 1);
            return 0;
        };
        if (up(S.one_f, pl->dp.one_f)) return -1;
        if (S.one_b.sn.empty()) pl->dp.one_b = pl->dp.one_f;
        else if (up(S.one_b, pl->dp.one_b)) return -1;
        // (the hand-off buffers are sized by the lists: made again by the next ONE-launch solve; the status word of the
        // last such solve lived in them)
        for (int d = 0; d < 2; ++d) {
            (void)pl->one_y[d].reset();
            pl->one_cap[d] = 0;
            pl->one_calls[d] = 0;
        }
        pl->solve_status_word = nullptr;
    }
    // (the tickets are not counted)
    pl->dp.tickets = pl->launches.alloc<int>(std::max(S.n_chain_launches, 1), false);
    pl->dp.stickets = pl->launches.alloc<int>(std::max(S.n_solve_chain_launches, 1), false);
    if (pl->launches.error() != hipSuccess) return pool_failed(pl->launches);
    // hipMemcpy from pageable memory returns when the data is staged, hipMemset when it is enqueued:
    // both are only ordered against the NULL stream.  The caller's stream may be a non-blocking one,
    // so everything must have landed before the plan is handed out.
    PARSY_HIP(hipDeviceSynchronize());
    return 0;
}

static int plan_upload(parsy_plan* pl) {
    PARSY_HIP(hipSetDevice(pl->device));
    const Schedule& S = pl->S;
    if (upload(pl, S.sn, pl->dp.sn, false)) return -1;
    if (upload(pl, S.csn, pl->dp.csn, false)) return -1;
    if (upload(pl, S.big_entries, pl->dp.big_entries, false)) return -1;
    if (upload(pl, S.upd, pl->dp.upd, false)) return -1;
    if (upload(pl, S.relpos, pl->dp.relpos, false)) return -1;
    if (upload(pl, S.a_dst, pl->dp.a_dst, false)) return -1;
    if (upload(pl, S.rows, pl->dp.rows, false)) return -1;
    if (upload(pl, S.wave_entries, pl->dp.wave_entries, false)) return -1;
    if (upload(pl, S.wave_ptr, pl->dp.wave_ptr, false)) return -1;
    if (upload(pl, S.split_ranges, pl->dp.split_ranges, false)) return -1;
    {
        DevicePool& P = pl->pattern;
        const int64_t nflags = 2 * std::max<int64_t>(S.n_tflags, 1);
        pl->dp.n_tflags = (int)S.n_tflags;
        pl->dp.tile_scratch = P.alloc<double>(std::max<int64_t>(S.n_split_doubles, 1));
        pl->dp.tflags = P.alloc<int>(nflags);
        pl->dp.info = P.alloc<int>(1, false);   // (the two status words are not counted)
        pl->dp.sinfo = P.alloc<int>(1, false);
        if (P.error() != hipSuccess) return pool_failed(P);
        PARSY_HIP(hipMemset(pl->dp.info, 0x7f, sizeof(int)));
        PARSY_HIP(hipMemset(pl->dp.sinfo, 0, sizeof(int)));
        PARSY_HIP(hipMemset(pl->dp.tflags, 0, (size_t)nflags * sizeof(int)));
    }
    {
        // lowest priority: the side stream only fills what the main stream's chain leaves idle
        int prio_least = 0, prio_greatest = 0;
        PARSY_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        PARSY_HIP(hipStreamCreateWithPriority(&pl->side_stream, hipStreamNonBlocking, prio_least));
    }
    PARSY_HIP(hipEventCreateWithFlags(&pl->ev_init, hipEventDisableTiming));
    pl->ev_level_done.resize(std::max(S.nlevels, S.cnlevels) + 1);
    pl->ev_early_done.resize(std::max(S.nlevels, S.cnlevels) + 1);
    for (auto& e : pl->ev_level_done) PARSY_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : pl->ev_early_done) PARSY_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    {
        const char* no = std::getenv("PARSY_NO_OVERLAP");
        pl->overlap = !(no && no[0] == '1');
    }
    PARSY_HIP(hipEventCreate(&pl->ev_f0));
    PARSY_HIP(hipEventCreate(&pl->ev_f1));
    PARSY_HIP(hipEventCreate(&pl->ev_s0));
    PARSY_HIP(hipEventCreate(&pl->ev_s1));
    return plan_upload_launches(pl);
}

parsy_plan* plan_build(const PatternRef& P, const size_t* lC, const int* A2p, const int* A2i,
                       int device) {
    parsy_plan* pl = new parsy_plan;
    int cus = 0;
    if (device >= 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) cus = prop.multiProcessorCount;
        // the schedule sizes its walker batches for 2 resident chain workgroups per CU: if the runtime
        // admits fewer (another register / LDS budget), count the CUs accordingly
        (void)hipSetDevice(device);
        const int per_cu = chain_workgroups_per_cu();
        if (per_cu == 1) cus = cus / 2;
    }
    try {
        build_schedule(P, lC, A2p, A2i, nullptr, pl->S, cus);
    } catch (const std::exception& e) {
        set_last_error(std::string("plan: ") + e.what());
        delete pl;
        return nullptr;
    }
    pl->solve_only = pl->S.solve_only;
    pl->device = device;
    if (device >= 0 && plan_upload(pl) != 0) {
        plan_free(pl);
        return nullptr;
    }
    return pl;
}

void plan_free(parsy_plan* pl) {
    if (!pl) return;
    if (pl->device >= 0) {
        (void)hipSetDevice(pl->device);
        (void)hipDeviceSynchronize();
        for (hipEvent_t e : {pl->ev_f0, pl->ev_f1, pl->ev_s0, pl->ev_s1})
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : pl->pev) (void)hipEventDestroy(e);
        for (hipEvent_t e : pl->ev_level_done) (void)hipEventDestroy(e);
        for (hipEvent_t e : pl->ev_early_done) (void)hipEventDestroy(e);
        if (pl->ev_init) (void)hipEventDestroy(pl->ev_init);
        if (pl->side_stream) (void)hipStreamDestroy(pl->side_stream);
        if (pl->h_stream) (void)hipStreamDestroy(pl->h_stream);
        if (pl->h_copy) (void)hipStreamDestroy(pl->h_copy);
        for (hipEvent_t e : pl->h_band_ev) (void)hipEventDestroy(e);
    }
    delete pl;   // (the pools, the buffers and the feature states free what they hold)
}

static void profile_mark(parsy_plan* pl, int kind, hipStream_t stream, size_t& cursor, int level = -1, int side = 0,
                         int count = 0) {
    if (!pl->profile) return;
    if (cursor >= pl->pev_count.size()) pl->pev_count.resize(cursor + 1, 0);
    pl->pev_count[cursor] = count;
    if (cursor >= pl->pev_level.size()) pl->pev_level.resize(cursor + 1, 0);
    pl->pev_level[cursor] = level >= 0 ? (level << 1) | (side & 1) : -1;
    if (cursor >= pl->pev.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        pl->pev.push_back(e);
    }
    if (cursor >= pl->pev_kind.size()) pl->pev_kind.push_back(kind);
    else pl->pev_kind[cursor] = kind;
    (void)hipEventRecord(pl->pev[cursor], stream);
    ++cursor;
}

// Enqueue the factorization's launches seq[i0, i1) (a solve's: run_route).  The state that orders the two streams (which
// level-completion events have been recorded, which side launches are in flight, the profiling cursor) lives in the plan,
// so that a factorization can be enqueued level by level (parsy_factor_level) with the caller's own work -- the exchange
// step of a multi-device run -- in between: run_begin() resets it, run_end() closes the profiling record.
static void run_begin(parsy_plan* pl) {
    pl->run_cursor = 0;
    pl->run_next_level_event = 0;
    pl->run_early_seen.assign(pl->ev_early_done.size(), 0);
}

static void run_range(parsy_plan* pl, const std::vector<Launch>& seq, size_t i0, size_t i1, double* L, hipStream_t stream) {
    size_t& cursor = pl->run_cursor;
    // TILES_EARLY launches go to the side stream (unless profiling / disabled): they wait for the
    // completion event of the level two below their targets and run beside the main stream's
    // block-column chain; the matching TILES (late) launch waits for them.
    const bool overlap = pl->overlap && !pl->profile && pl->side_stream != nullptr;
    int& next_level_event = pl->run_next_level_event;  // ev_level_done[k] recorded for all k < next_level_event
    std::vector<char>& early_seen = pl->run_early_seen;
    auto record_levels_below = [&](int level) {
        for (; next_level_event < level && next_level_event < (int)pl->ev_level_done.size(); ++next_level_event)
            (void)hipEventRecord(pl->ev_level_done[next_level_event], stream);
    };
    for (size_t li = i0; li < i1; ++li) {
        const Launch& l = seq[li];
        const bool on_side = overlap && l.side;
        if (!on_side) {
            // everything enqueued so far on the main stream belongs to levels < l.level
            if (overlap && is_chol_launch(l.kind)) record_levels_below(l.level);
            // A main-stream launch that touches level t's tiles (NEXT, CHAIN) comes after every side launch
            // enqueued so far whose targets can be at level t: those with a level field <= t (a PUSH writes
            // into EVERY level from its field upwards).  The side stream runs in order, so the latest of them
            // covers the earlier ones; PUSH(t - 1) / TILES(t + 1) (field t + 1) stay free to overlap.
            if (overlap && (l.kind == kLaunchChain || l.kind == kLaunchBig || l.kind == kLaunchDense)) {
                int lw = std::min<int>(l.level, (int)early_seen.size() - 1);
                while (lw >= 0 && !early_seen[lw]) --lw;
                if (lw >= 0) (void)hipStreamWaitEvent(stream, pl->ev_early_done[lw], 0);
            }
        }
        profile_mark(pl, l.kind, stream, cursor, l.level, l.side, l.count);
        switch (l.kind) {
            case kLaunchSmall: launch_chol_small(pl->dp, l.first, l.count, l.lds_bytes, l.stage, l.form == kFormSubtrees, L, stream); break;
            case kLaunchTiles:
            case kLaunchBig:
            case kLaunchDense: {
                const hipStream_t st = on_side ? pl->side_stream : stream;
                if (on_side) {
                    record_levels_below(l.wait_level + 1);
                    (void)hipStreamWaitEvent(st, l.wait_level >= 0 ? pl->ev_level_done[l.wait_level] : pl->ev_init, 0);
                }
                if (l.kind == kLaunchBig) launch_chol_big(pl->dp, l.first, l.count, L, st);
                else if (l.kind == kLaunchDense) launch_chol_dense(pl->dp, l.first, l.count, L, st);
                else launch_chol_tiles(pl->dp, l.first, l.count, L, st);
                if (on_side) {
                    (void)hipEventRecord(pl->ev_early_done[l.level], st);
                    early_seen[l.level] = 1;
                }
                break;
            }
            case kLaunchChain: launch_chol_chain(pl->dp, l.first, l.count, l.ticket, pl->epoch, l.rows_only != 0, L, stream); break;
            default: break;   // (the solves' kinds: enqueued from a route, run_route)
        }
    }
}

static void run_end(parsy_plan* pl, hipStream_t stream) {
    profile_mark(pl, -1, stream, pl->run_cursor);
    if (pl->profile) pl->pev_kind.resize(pl->run_cursor);
}

struct OneBuffers {   // what one ONE-launch solve works through
    double *y = nullptr, *y_next = nullptr;
    int *st = nullptr, *st_next = nullptr;
};

// The buffers of the ONE-launch solves, made by the first of them: per direction two hand-off buffers (forward: one
// slot per entry of the row-id array, backward: one per unknown; kOneMaxRhs right-hand sides), all armed, and two
// {status, ticket} pairs, zero.  Every such solve then works through buffer / pair (its direction's count & 1) and
// leaves the other one armed and zeroed for the next solve of its kind (k_solve_one, k_bsolve_one) -- one
// enqueue per solve, no memset.
static int one_begin(parsy_plan* pl, bool backward, int want, hipStream_t stream, OneBuffers& one) {
    // (a direction's buffers hold `want` = 1, 4 or 8 right-hand sides, the route's capacity class -- nd24k-class: 12.5 MB per
    // right-hand side for the forward slots -- and are made again, larger, when a wider block comes: earlier solves on the
    // stream are complete by then)
    const int d = backward ? 1 : 0;
    DeviceBuf<double>& buf = pl->one_y[d];
    if (want > pl->one_cap[d] && buf.data()) {
        PARSY_HIP(hipStreamSynchronize(stream));
        (void)buf.reset();
        if (pl->solve_status_word) pl->solve_status_word = nullptr;
    }
    if (!buf.data()) {
        pl->one_cap[d] = std::max(pl->one_cap[d], want);
        const size_t len = (size_t)(backward ? pl->S.n : pl->dp.one_f.nslots) * pl->one_cap[d];
        // (the two {status, ticket} pairs, four ints, live behind the two buffers: one allocation)
        static_assert(4 * sizeof(int) == 2 * sizeof(double), "the state words are counted as two doubles");
        if (buf.grow((int64_t)(2 * len + 2)) != hipSuccess) {
            // no room for the hand-off buffers: this plan's solves of that direction go by the level launches from now on
            (void)hipGetLastError();
            pl->one_cap[d] = 0;
            pl->route_rt.one_off[d] = true;
            return 1;
        }
        PARSY_HIP(solve_arm_handoff(buf.data(), (int64_t)(2 * len), stream));
        PARSY_HIP(hipMemsetAsync(buf.data() + 2 * len, 0, 4 * sizeof(int), stream));
        pl->one_calls[d] = 0;
    }
    const size_t len = (size_t)(backward ? pl->S.n : pl->dp.one_f.nslots) * pl->one_cap[d];
    int* state = reinterpret_cast<int*>(buf.data() + 2 * len);
    const unsigned k = pl->one_calls[d]++ & 1u;
    one.y = buf.data() + k * len;
    one.y_next = buf.data() + (k ^ 1u) * len;
    one.st = state + 2 * k;
    one.st_next = state + 2 * (k ^ 1u);
    pl->solve_status_word = one.st;
    return 0;
}

// Argument checks of a device solve (`who`: the C ABI call the messages name).  A solve that starts here abandons one in
// steps of levels that was never finished and reads the gates of its kernel variants, once for all its launches.
static int solve_start(parsy_plan* pl, const char* who, bool args_ok, const char* need, bool starts = true) {
    if (pl->device < 0) {
        set_last_error(std::string(who) + ": plan was built without a device (device < 0)");
        return -1;
    }
    if (!args_ok) {
        set_last_error(std::string(who) + ": need " + need);
        return -1;
    }
    if (starts) {
        pl->levels_open = false;
        pl->gates = read_solve_gates();
    }
    return 0;
}

// The prologue of a solve by level launches, from its route's facts: its own status word and the chain launches' ticket
// counters zeroed (arm_wide: by the route's k_solve_arm_wide launch instead), xscratch grown to `scratch` entries, xt to X
// row-major, the inverse diagonal blocks and the backward partial sums allocated by the first solve that needs them;
// then ev_s0 and, without arm_wide, the first `armed` entries of the hand-off buffer armed.  The chain launches hand x
// over through xscratch itself (solve_arm_handoff) and finish a block column with a product with its inverse diagonal
// block (k_diag_inverse, the route's next launch).
static int solve_prologue(parsy_plan* pl, const SolveRoute& R, hipStream_t stream) {
    const Schedule& S = pl->S;
    pl->solve_status_word = nullptr;
    if (!R.arm_wide) {
        PARSY_HIP(hipMemsetAsync(pl->dp.sinfo, 0, sizeof(int), stream));
        PARSY_HIP(hipMemsetAsync(pl->dp.stickets, 0, (size_t)std::max(S.n_solve_chain_launches, 1) * sizeof(int), stream));
    }
    if (R.use_xt) PARSY_HIP(pl->xt.grow((int64_t)S.n * R.ldq));
    if (R.scratch > 0) PARSY_HIP(pl->xscratch.grow(R.scratch));
    if (R.dinv && !pl->dinv.data()) PARSY_HIP(pl->dinv.grow(std::max<int64_t>(S.n_dslots, 1) * kTile * kTile));
    if (R.bpart && !pl->dp.bpart) {
        PARSY_HIP(pl->bpart.grow((int64_t)S.n_bpart_slots * kTile));
        pl->dp.bpart = pl->bpart.data();
    }
    PARSY_HIP(hipEventRecord(pl->ev_s0, stream));
    if (!R.arm_wide && R.armed > 0) PARSY_HIP(solve_arm_handoff(pl->xscratch.data(), R.armed, stream));
    return 0;
}

// Walk a route: every step's mark in the profiling record (run_begin has opened it; `end`: closed behind the last marked
// step), then the launch function its kernel belongs to, with the launch record or the tier the step runs on.
static void run_route(parsy_plan* pl, const SolveRoute& R, bool backward, const OneBuffers& one, const double* L, double* d_x,
                      int nrhs, int ldx, hipStream_t stream, bool end = true) {
    const Schedule& S = pl->S;
    const DevicePattern& P = pl->dp;
    const std::vector<Launch>& seq = backward ? S.bsolve : S.solve;
    double* const x = R.use_xt ? pl->xt.data() : d_x;
    double *const dinv = pl->dinv.data(), *const xs = pl->xscratch.data();
    const int wait_bias = pl->gates.wait_bias, sub_abl = pl->gates.sub_abl, cap = pl->one_cap[backward ? 1 : 0];
    const int nwide = (int)S.solve_wide_list.size() / 2;
    static const Launch none{};
    for (size_t i = 0; i < R.steps.size(); ++i) {
        const SolveStep& s = R.steps[i];
        if (i == R.tail && end) run_end(pl, stream);
        if (s.kind >= 0) profile_mark(pl, s.kind, stream, pl->run_cursor, s.level, s.side, s.count);
        const Launch& l = s.launch >= 0 ? seq[(size_t)s.launch] : none;
        switch (s.kernel) {
            case kWSolveTiny: case kWSolveSmall: case kWSolveSmallMrhs16: case kWSolveSmallMrhs32: case kWSolveSmallMrhs64:
            case kWSolveSmallMrhs64Halves:
                launch_solve_small(P, s.kernel, l.first, l.count, l.form == kFormSubtrees, L, x, nrhs, ldx, R.ldq, stream);
                break;
            case kWSolveSubMrhs: launch_solve_sub_mrhs(P, S.sub_tiers[(size_t)s.tier], L, x, nrhs, ldx, R.ldq, sub_abl, stream); break;
            case kWBsolveSubMrhs: launch_bsolve_sub_mrhs(P, S.sub_tiers[(size_t)s.tier], L, x, nrhs, ldx, sub_abl, stream); break;
            case kWSolveBlocksMrhsNarrow: case kWSolveBlocksMrhs:
                launch_solve_blocks_mrhs(P, s.kernel, l.task_first, l.task_count, L, dinv, x, xs, nrhs, ldx, R.ldq, l.ticket,
                                         wait_bias, stream);
                break;
            case kWSolveChainW2: case kWSolveChainW4:
                launch_solve_chain(P, s.kernel, l.first, l.count, L, dinv, x, xs, l.ticket, wait_bias, stream);
                break;
            case kWSolvePanel: launch_solve_panel(P, l.first, l.count, L, x, xs, nrhs, ldx, stream); break;
            case kWSolveFixup: launch_solve_fixup(P, l.first, l.count, x, xs, nrhs, ldx, stream); break;
            case kWBsolveBelow: launch_bsolve_below(P, l.first, l.count, L, x, stream); break;
            case kWBsolveChainW: launch_bsolve_chain_w(P, l.task_first, l.task_count, L, dinv, x, xs, l.ticket, wait_bias, stream); break;
            case kWBsolveBlock1: case kWBsolveBlock4: case kWBsolveBlockMrhs1: case kWBsolveBlockMrhs4: case kWBsolveChainMrhs:
            case kWBsolveTiny16: case kWBsolveTiny32: case kWBsolveTinyMrhs:
                launch_bsolve_block(P, s.kernel, l.first, l.count, L, dinv, x, xs, nrhs, ldx, (LaunchForm)l.form, l.ticket, wait_bias,
                                    stream);
                break;
            case kWSolveOne1: case kWSolveOne4: case kWSolveOne8:
                launch_solve_one(P, s.kernel, L, x, nrhs, ldx, one.y, one.y_next, one.st, one.st_next, wait_bias, cap, stream);
                break;
            case kWBsolveOne1: case kWBsolveOne4: case kWBsolveOne8:
                launch_bsolve_one(P, s.kernel, S.n, L, x, nrhs, ldx, one.y, one.y_next, one.st, one.st_next, wait_bias, cap, stream);
                break;
            // (in before the marked steps, out behind them)
            case kWTransposeX: launch_transpose_x(d_x, ldx, pl->xt.data(), R.ldq, S.n, nrhs, i < R.body, stream); break;
            case kWSolveArmWide:
                launch_solve_arm_wide(P, nwide, xs, nrhs, ldx, R.ldq, std::max(S.n_solve_chain_launches, 1), stream);
                break;
            case kWDiagInverse: launch_diag_inverse(P, nwide, L, dinv, stream); break;
            default: break;   // (kWitnessCount: a launch record that enqueues nothing)
        }
    }
    if (R.tail >= R.steps.size() && end) run_end(pl, stream);
}

static int solve_end(parsy_plan* pl, hipStream_t stream) {
    PARSY_HIP(hipGetLastError());
    PARSY_HIP(hipEventRecord(pl->ev_s1, stream));
    pl->have_s = true;
    return 0;
}

// A whole forward / backward solve: the arguments, the gates, the route, one prologue from the route's facts, the steps.
static int solve_whole(parsy_plan* pl, const char* who, bool backward, const double* d_L, double* d_x, int nrhs, int ldx,
                       hipStream_t stream) {
    if (solve_start(pl, who, nrhs >= 1 && ldx >= pl->S.n, "nrhs >= 1 and ldx >= n") != 0) return -1;
    SolveRoute& R = pl->route[backward ? 1 : 0];
    solve_route(pl->S, pl->gates, pl->route_rt, nrhs, ldx, backward, R);
    OneBuffers one;
    if (R.one) {
        const int rc = one_begin(pl, backward, R.one_cap, stream, one);
        if (rc < 0) return -1;
        if (rc > 0) solve_route(pl->S, pl->gates, pl->route_rt, nrhs, ldx, backward, R);   // (no room: by level launches)
    }
    if (R.one) PARSY_HIP(hipEventRecord(pl->ev_s0, stream));
    else if (solve_prologue(pl, R, stream) != 0) return -1;
    run_begin(pl);
    run_route(pl, R, backward, one, d_L, d_x, nrhs, ldx, stream);
    return solve_end(pl, stream);
}

int plan_solve(parsy_plan* pl, const double* d_L, double* d_x, int nrhs, int ldx, hipStream_t stream) {
    return solve_whole(pl, "parsy_solve", false, d_L, d_x, nrhs, ldx, stream);
}

int plan_backsolve(parsy_plan* pl, const double* d_L, double* d_x, int nrhs, int ldx, hipStream_t stream) {
    return solve_whole(pl, "parsy_backsolve", true, d_L, d_x, nrhs, ldx, stream);
}

// A solve in steps of etree levels (the exchange steps of a solve that is distributed above the cut go in between,
// as parsy_factor_level's do for the factorization): the level launches of the plan's active supernodes whose level lies
// in [lev0, lev1).  flags: bit 0 = the first step of a solve (status word, tickets, hand-off buffer, inverse diagonal
// blocks), bit 1 = the last one, bit 2 = backward (levels then go DOWN from step to step).  Level launches only: the
// caller's layout of X, no ONE launch, no bands (a rank's share of the supernodes has neither) -- solve_route_levels.
int plan_solve_levels(parsy_plan* pl, const double* d_L, double* d_x, int nrhs, int ldx, hipStream_t stream, int lev0,
                      int lev1, int flags) {
    const bool first = flags & 1, last = flags & 2, backward = flags & 4;
    if (solve_start(pl, "parsy_solve_levels", nrhs >= 1 && ldx >= pl->S.n && lev0 <= lev1,
                    "nrhs >= 1, ldx >= n and level_begin <= level_end", first) != 0)
        return -1;
    if (!first && (!pl->levels_open || pl->levels_backward != backward || pl->levels_nrhs != nrhs)) {
        set_last_error("parsy_solve_levels: a step without PARSY_SOLVE_FIRST needs an open solve of the same direction and width");
        return -1;
    }
    SolveRoute& R = pl->route[backward ? 1 : 0];
    solve_route_levels(pl->S, pl->gates, pl->route_rt, nrhs, ldx, backward, lev0, lev1, first, last, R);
    if (first) {
        if (solve_prologue(pl, R, stream) != 0) return -1;
        run_begin(pl);
        pl->levels_open = true;
        pl->levels_backward = backward;
        pl->levels_nrhs = nrhs;
    }
    run_route(pl, R, backward, OneBuffers(), d_L, d_x, nrhs, ldx, stream, last);
    if (!last) return 0;
    pl->levels_open = false;
    return solve_end(pl, stream);
}

int plan_collect_profile(parsy_plan* pl) {
    // after a synchronised profiled run: add the elapsed time of each launch to its kind
    if (!pl->profile || pl->pev_kind.size() < 2) return -1;
    for (size_t i = 0; i + 1 < pl->pev_kind.size(); ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pl->pev[i], pl->pev[i + 1]) != hipSuccess) return -1;
        const int k = pl->pev_kind[i];
        if (pl->pev_ms.size() <= i) pl->pev_ms.resize(i + 1, 0.f);
        pl->pev_ms[i] = ms;
        if (k >= 0 && k < PARSY_PROFILE_KINDS) {
            pl->kind_ms[k] += ms;
            pl->kind_launches[k] += 1;
        }
        // factorization launches also per level of the Cholesky view and stream (main / side)
        if (is_chol_launch(k) && i < pl->pev_level.size() && pl->pev_level[i] >= 0) {
            const size_t slot = (size_t)pl->pev_level[i];
            if (pl->level_ms.size() <= slot) pl->level_ms.resize(slot + 1, 0.0);
            pl->level_ms[slot] += ms;
        }
    }
    pl->profiled_runs += 1;
    return 0;
}

int plan_factor_begin(parsy_plan* pl, const double* d_values, double* d_L, hipStream_t stream, bool init) {
    if (pl->device < 0) {
        set_last_error("parsy_factor: plan was built without a device (device < 0)");
        return -1;
    }
    if (pl->solve_only) {
        set_last_error("parsy_factor: plan was built from L's pattern only (solve-only)");
        return -1;
    }
    const Schedule& S = pl->S;
    // flags of earlier factorizations go stale; on wrap-around they are cleared, so that a value left by an
    // early factorization cannot pass for a new one
    if (pl->epoch >= INT_MAX - 4) {
        PARSY_HIP(hipMemsetAsync(pl->dp.tflags, 0, 2 * (size_t)std::max(pl->dp.n_tflags, 1) * sizeof(int), stream));
        pl->epoch = 0;
    }
    pl->epoch += 1;
    PARSY_HIP(hipEventRecord(pl->ev_f0, stream));
    if (init) PARSY_HIP(hipMemsetAsync(d_L, 0, (size_t)S.xsize * sizeof(double), stream));
    // "no failed pivot" = 0x7f7f7f7f (kernels atomicMin the 1-based failing column into it)
    PARSY_HIP(hipMemsetAsync(pl->dp.info, 0x7f, sizeof(int), stream));
    PARSY_HIP(hipMemsetAsync(pl->dp.tickets, 0, (size_t)std::max(S.n_chain_launches, 1) * sizeof(int), stream));
    if (init) launch_scatter_a(d_values, pl->dp.a_dst, d_L, S.nnzA, stream);
    PARSY_HIP(hipEventRecord(pl->ev_init, stream));
    run_begin(pl);
    pl->factor_open = true;
    pl->factor_next_level = 0;
    return 0;
}

// The launches of levels [level0, level1) of the Cholesky view (levels must be passed in ascending order and
// without gaps: each step may enqueue side-stream launches that wait for the completion of the step before it).
int plan_factor_levels(parsy_plan* pl, int level0, int level1, double* d_L, hipStream_t stream) {
    const Schedule& S = pl->S;
    if (!pl->factor_open) {
        set_last_error("parsy_factor_level: no factorization is open (call parsy_factor_begin first)");
        return -1;
    }
    if (level0 != pl->factor_next_level || level1 < level0 || level1 > S.cnlevels) {
        set_last_error("parsy_factor_level: levels must be enqueued in ascending order without gaps");
        return -1;
    }
    if (level1 > level0)
        run_range(pl, S.chol, S.chol_level_begin[(size_t)level0], S.chol_level_begin[(size_t)level1], d_L, stream);
    // (profiling: what the caller does between two steps is not a launch's time)
    profile_mark(pl, -1, stream, pl->run_cursor);
    pl->factor_next_level = level1;
    PARSY_HIP(hipGetLastError());
    return 0;
}

int plan_factor_end(parsy_plan* pl, hipStream_t stream) {
    if (!pl->factor_open) {
        set_last_error("parsy_factor_end: no factorization is open");
        return -1;
    }
    if (pl->factor_next_level != pl->S.cnlevels) {
        set_last_error("parsy_factor_end: not every level has been enqueued");
        return -1;
    }
    run_end(pl, stream);
    // the side stream's last launches belong to this factorization: the caller's stream waits for them
    if (pl->overlap && !pl->profile && pl->side_stream != nullptr) {
        for (size_t k = pl->run_early_seen.size(); k-- > 0;)
            if (pl->run_early_seen[k]) {
                (void)hipStreamWaitEvent(stream, pl->ev_early_done[k], 0);
                break;
            }
    }
    PARSY_HIP(hipGetLastError());
    PARSY_HIP(hipEventRecord(pl->ev_f1, stream));
    pl->have_f = true;
    pl->factor_open = false;
    return 0;
}

// Error path of a caller that enqueues a factorization step by step: whatever was enqueued is allowed to finish
// (caller's stream and the plan's side stream), then the plan is closed again so that a later factorization starts
// clean.  The factor in d_L is partial.
void plan_factor_abort(parsy_plan* pl, hipStream_t stream) {
    if (!pl) return;
    (void)hipStreamSynchronize(stream);
    if (pl->side_stream != nullptr) (void)hipStreamSynchronize(pl->side_stream);
    (void)hipGetLastError();
    if (pl->factor_open) run_end(pl, stream);
    pl->factor_open = false;
    pl->factor_next_level = 0;
}

int plan_factor(parsy_plan* pl, const double* d_values, double* d_L, hipStream_t stream, bool init) {
    if (plan_factor_begin(pl, d_values, d_L, stream, init) != 0) return -1;
    if (plan_factor_levels(pl, 0, pl->S.cnlevels, d_L, stream) != 0) return -1;
    return plan_factor_end(pl, stream);
}

}  // namespace parsy

// (here, where the feature states' types are complete)
parsy_plan::~parsy_plan() = default;
