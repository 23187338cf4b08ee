// Device-resident plan: pattern + schedule in HBM, launch sequencing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/parsy_amd.h"
#include "device_buffer.hpp"
#include "kernels.hpp"
#include "schedule.hpp"

namespace parsy {
struct RefineState;
struct SelinvState;
struct GradState;
struct CondState;
struct ApplyState;
struct UpdownState;
struct RowmodState;
struct EigsState;
}

struct parsy_plan {
    parsy::Schedule S;
    int device = -1;          // < 0: host schedule only
    std::mutex use_mu;        // the drop-in operators hold it across a call: flags, tickets, status and the
                              // host-convenience buffers of a cached plan belong to one call at a time
    bool solve_only = false;  // built from L's pattern alone (no A, no update lists)
    bool sn_mask_set = false, piece_mask_set = false;  // parsy_plan_set_active / _set_active_pieces are in force

    // Device memory (device_buffer.hpp).  What is made with &meter is counted in parsy_plan_info.device_bytes; the
    // feature states below hang their own meters under it.  dp holds the raw views the kernels receive.
    parsy::ByteMeter meter;
    parsy::DevicePool pattern{&meter};    // pattern arrays, flags and status words: made once
    parsy::DevicePool launches{&meter};   // launch arrays and tickets: made again by set_active
    parsy::DevicePattern dp;
    int epoch = 0;            // factorization counter (value the Cholesky chain launches publish / wait for)

    parsy::DeviceBuf<double> dinv{&meter};    // inverse 64x64 diagonal blocks of the wide supernodes (solve)
    parsy::DeviceBuf<double> bpart{&meter};   // dp.bpart: sized by the launch lists, reset with them
    parsy::DeviceBuf<double> xscratch;        // (not counted)
    // ONE-launch solves (Schedule::solve_one): per direction two hand-off buffers (a solve works through the one its
    // predecessor armed and arms the other: no memset between solves) and two {status, ticket} pairs, used in turn
    // forward, backward: two buffers + the two state pairs behind them (four ints = two doubles)
    parsy::DeviceBuf<double> one_y[2] = {parsy::DeviceBuf<double>(&meter), parsy::DeviceBuf<double>(&meter)};
    unsigned one_calls[2] = {0, 0};
    int one_cap[2] = {0, 0};                 // right-hand sides the buffers are made for (1, 4 or 8: grown on demand)
    // The dispatch of the solves (solve_route.hpp): the gates of the running solve, what its route depends on beyond them
    // and the schedule -- a direction whose ONE-launch buffers could not be allocated: level launches from then on; the
    // subtree tiers whose workgroups get their LDS --, and the route itself, forward and backward, made again by every solve
    parsy::SolveGates gates;
    parsy::RouteRuntime route_rt;
    parsy::SolveRoute route[2];
    const int* solve_status_word = nullptr;   // where the last solve left its status (null: dp.sinfo)

    // buffers of the host-buffer calls (capi_hostcalls.hip): A's values, the factor, the right-hand sides; they live as
    // long as the plan and are not counted in device_bytes
    parsy::DeviceBuf<double> h_values_dev, h_L_dev, h_x_dev;
    // host-buffer factorization with the download behind the kernels (parsy_factor_host): its own
    // streams, one event per band of levels, the (offset, length) runs of lValues that are final after each band
    hipStream_t h_stream = nullptr, h_copy = nullptr;
    std::vector<hipEvent_t> h_band_ev;
    bool h_ready = false;                    // the pipelined download's streams, bands and events all exist
    bool levels_open = false, levels_backward = false;   // a solve in steps of levels (plan_solve_levels) is under way
    int levels_nrhs = 0;
    std::vector<int> h_band_level;                                    // last level of every band
    std::vector<std::vector<std::pair<int64_t, int64_t>>> h_band_runs;

    // side stream of the TILES_EARLY launches + the events that order it against the main stream
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_init = nullptr;
    std::vector<hipEvent_t> ev_level_done, ev_early_done;
    bool overlap = true;      // PARSY_NO_OVERLAP=1 (or profiling) runs everything on the caller's stream

    // state of the launch sequence being enqueued (executor.hip run_range): persistent so that a factorization
    // can be enqueued level by level
    size_t run_cursor = 0;
    int run_next_level_event = 0;
    std::vector<char> run_early_seen;
    bool factor_open = false;
    int factor_next_level = 0;

    hipEvent_t ev_f0 = nullptr, ev_f1 = nullptr, ev_s0 = nullptr, ev_s1 = nullptr;
    bool have_f = false, have_s = false;

    // optional per-launch profiling (hipEvents on the launch stream)
    bool profile = false;
    parsy::DeviceBuf<double> xt;    // X with the right-hand sides of a row contiguous (forward solves with many of them;
                                    // not counted)
    std::vector<hipEvent_t> pev;
    std::vector<int> pev_kind;
    std::vector<int> pev_level;     // per mark: level << 1 | side of a factorization launch (-1: other)
    std::vector<int> pev_count;     // per mark: work items of the launch
    std::vector<float> pev_ms;      // per mark: elapsed time in the last collected run (diagnostics)
    std::vector<double> level_ms;   // accumulated ms per (level << 1 | side)
    double kind_ms[PARSY_PROFILE_KINDS] = {};
    int kind_launches[PARSY_PROFILE_KINDS] = {};
    int profiled_runs = 0;
    // the caller's ordering (parsy_plan_set_perm; plan_util.hpp): perm[new] = old (empty: identity) and its device copy,
    // uploaded by the first call that reads it
    std::vector<int> perm;
    std::vector<int> perm_inv;       // its inverse (plan_perm_inverse), made on first use
    parsy::DeviceBuf<int> d_perm{&meter};
    bool perm_on_device = false;     // d_perm holds perm
    // the states of the features, each made by the first call of its kind
    std::unique_ptr<parsy::RefineState> refine;   // A x = b in the caller's ordering (refine.hpp)
    std::unique_ptr<parsy::SelinvState> selinv;   // selected inversion / log-determinant (selinv.hpp)
    std::unique_ptr<parsy::GradState> grad;       // gradients with respect to A's values (grad.hpp)
    std::unique_ptr<parsy::CondState> cond;       // forward error bounds / condition estimate (cond.hpp)
    std::unique_ptr<parsy::ApplyState> apply;     // the factor as an operator (apply.hpp)
    std::unique_ptr<parsy::UpdownState> updown;   // update / downdate of the factor (updown.hpp)
    std::unique_ptr<parsy::RowmodState> rowmod;   // row delete / row add in the factor (rowmod.hpp)
    std::unique_ptr<parsy::EigsState> eigs;       // smallest eigenpairs of A x = lambda M x (eigs.hpp)

    ~parsy_plan();   // (executor.hip, where the state types are complete)
};

namespace parsy {

// Build a plan. A2p/A2i may be null => solve-only plan. device < 0 => no HIP calls.
parsy_plan* plan_build(const PatternRef& P, const size_t* lC, const int* A2p, const int* A2i,
                       int device);
void plan_free(parsy_plan* plan);
int plan_upload_launches(parsy_plan* plan);
int plan_factor(parsy_plan* plan, const double* d_values, double* d_L, hipStream_t stream,
                bool init = true);
int plan_factor_begin(parsy_plan* plan, const double* d_values, double* d_L, hipStream_t stream, bool init);
int plan_factor_levels(parsy_plan* plan, int level0, int level1, double* d_L, hipStream_t stream);
int plan_factor_end(parsy_plan* plan, hipStream_t stream);
void plan_factor_abort(parsy_plan* plan, hipStream_t stream);   // error path: drain, close the open factorization
int plan_solve(parsy_plan* plan, const double* d_L, double* d_x, int nrhs, int ldx,
               hipStream_t stream);
int plan_backsolve(parsy_plan* plan, const double* d_L, double* d_x, int nrhs, int ldx, hipStream_t stream);
int plan_solve_levels(parsy_plan* plan, const double* d_L, double* d_x, int nrhs, int ldx, hipStream_t stream, int lev0,
                      int lev1, int flags);
int plan_collect_profile(parsy_plan* plan);
// What a route of the plan depends on at run time; without a device every subtree tier of the schedule counts as usable.
inline RouteRuntime plan_route_runtime(const parsy_plan* plan) {
    RouteRuntime rt = plan->route_rt;
    if (plan->device < 0) rt.sub_ntiers = (int)plan->S.sub_tiers.size();
    return rt;
}

}  // namespace parsy
