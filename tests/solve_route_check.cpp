// Stand-alone check of the solves' routes (csrc/solve_route.hpp).  test_solve_route_host.py compiles it together with
// solve_route.cpp, schedule.cpp, inspector.cpp and gen.cpp as host C++ with the address and undefined-behaviour sanitizers
// and runs it; nothing of HIP, no device.
// The plans are those of launch_record_check.cpp (a 13 x 13 x 13 7-point grid; between them they hold every launch kind and
// form of the solves), each also with the ONE launch forced and with bands of subtree tiers.  For every plan, several sets
// of gates, the subtree tiers usable or not, the ONE-launch buffers refused or not, both directions and 1 / 3 / 5 / 17 / 65
// right-hand sides, the route is held to:
//   1. every step's launch or tier index is in range, and the steps outside the profiling record are the unmarked ones;
//   2. every launch record of the direction appears at most once;
//   3. the launch function the executor hands a step to serves the step's kernel, and is given what it runs on (the
//      table `serves` below: kernel -> launch kind, or a tier, or neither; direction);
//   4. route_kernels lists exactly the steps that enqueue something;
//   5. a second build into the same SolveRoute allocates nothing (the steps' storage stays where it is).
// And a solve in steps of one level each (solve_route_levels): the prologue is in the first step only, and between them the
// steps hold every record of the direction exactly once.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "gen.hpp"
#include "inspector.hpp"
#include "schedule.hpp"
#include "solve_route.hpp"

using namespace parsy;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: CHECK(%s) [%s]\n", __FILE__, __LINE__, #cond, g_what.c_str()); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

static std::string g_what;

using Env = std::vector<std::pair<const char*, const char*>>;

static Schedule plan_of(const Symbolic& sym, const Env& env) {
    for (const auto& kv : env) setenv(kv.first, kv.second, 1);
    Schedule S;
    build_schedule(pattern_ref(sym), sym.p.data(), sym.A2.p.data(), sym.A2.i.data(), nullptr, S);
    for (const auto& kv : env) unsetenv(kv.first);
    return S;
}

// What the launch function of a kernel is given: a record of this kind (kNoKind: none), a tier, and in which direction.
constexpr int kNoKind = -1;
enum Dir { kFwd = 1, kBwd = 2, kBoth = 3 };
struct Serves {
    int kind = kNoKind;
    bool tier = false;
    int dir = 0;   // 0: no solve launches it through a route
};
static std::vector<Serves> serves_table() {
    std::vector<Serves> t(kWitnessCount);
    for (WitnessKernel k : {kWSolveTiny, kWSolveSmall, kWSolveSmallMrhs16, kWSolveSmallMrhs32, kWSolveSmallMrhs64, kWSolveSmallMrhs64Halves})
        t[k] = {kLaunchSolveSmall, false, kFwd};                                                  // launch_solve_small
    for (WitnessKernel k : {kWSolveBlocksMrhsNarrow, kWSolveBlocksMrhs, kWSolveChainW2, kWSolveChainW4, kWSolvePanel})
        t[k] = {kLaunchSolvePanel, false, kFwd};            // launch_solve_blocks_mrhs, launch_solve_chain, launch_solve_panel
    t[kWSolveFixup] = {kLaunchSolveFixup, false, kFwd};
    t[kWBsolveBelow] = {kLaunchBackBelow, false, kBwd};
    for (WitnessKernel k : {kWBsolveChainW, kWBsolveBlock1, kWBsolveBlock4, kWBsolveBlockMrhs1, kWBsolveBlockMrhs4, kWBsolveChainMrhs,
                            kWBsolveTiny16, kWBsolveTiny32, kWBsolveTinyMrhs})
        t[k] = {kLaunchBackBlock, false, kBwd};                                        // launch_bsolve_chain_w, launch_bsolve_block
    t[kWSolveSubMrhs] = {kLaunchSolveSmall, true, kFwd};   // (the record is optional: a band has none)
    t[kWBsolveSubMrhs] = {kLaunchBackBlock, true, kBwd};
    for (WitnessKernel k : {kWSolveOne1, kWSolveOne4, kWSolveOne8, kWTransposeX}) t[k] = {kNoKind, false, kFwd};
    for (WitnessKernel k : {kWBsolveOne1, kWBsolveOne4, kWBsolveOne8}) t[k] = {kNoKind, false, kBwd};
    for (WitnessKernel k : {kWSolveArmWide, kWDiagInverse}) t[k] = {kNoKind, false, kBoth};
    return t;
}

static bool seen_kernel[kWitnessCount];

// checks 1 - 4 on one route; `used` counts the records of the direction
static void check_route(const Schedule& S, const RouteRuntime& rt, const SolveRoute& R, bool backward, int nrhs,
                        std::vector<int>& used) {
    static const std::vector<Serves> serves = serves_table();
    const std::vector<Launch>& seq = backward ? S.bsolve : S.solve;
    CHECK(R.body <= R.tail && R.tail <= R.steps.size());
    int64_t enqueued = 0;
    for (size_t i = 0; i < R.steps.size(); ++i) {
        const SolveStep& s = R.steps[i];
        const bool marked = i >= R.body && i < R.tail;
        CHECK((s.kind >= 0) == marked);
        CHECK(s.launch >= -1 && s.launch < (int)seq.size());
        CHECK(s.tier >= -1 && s.tier < rt.sub_ntiers && s.tier < (int)S.sub_tiers.size());
        if (s.launch >= 0) {
            const Launch& l = seq[(size_t)s.launch];
            CHECK(++used[(size_t)s.launch] == 1);
            CHECK(s.kind == l.kind && s.level == l.level && s.side == l.side && s.count == l.count);
        }
        if (s.kernel == kWitnessCount) {   // marked only: BACK_BELOW with several right-hand sides (or an empty launch)
            CHECK(marked);
            CHECK(s.launch < 0 || seq[(size_t)s.launch].kind != kLaunchBackBelow || nrhs > 1);
            continue;
        }
        ++enqueued;
        CHECK(s.kernel >= 0 && s.kernel < kWitnessCount);
        seen_kernel[s.kernel] = true;
        const Serves& a = serves[(size_t)s.kernel];
        CHECK(a.dir & (backward ? kBwd : kFwd));
        CHECK((s.tier >= 0) == a.tier);
        if (a.kind == kNoKind) CHECK(s.launch < 0);
        else if (!a.tier) CHECK(s.launch >= 0);
        if (s.launch >= 0) {
            const Launch& l = seq[(size_t)s.launch];
            CHECK(l.kind == a.kind);
            if (a.tier) CHECK(l.form == kFormSubtrees && s.tier == 0 && S.sub_tiers[0].ntrees == l.count);
            // what the chain kernels are given: a chain-form record (its ticket, its tasks)
            const bool chain_kernel = s.kernel == kWSolveBlocksMrhsNarrow || s.kernel == kWSolveBlocksMrhs || s.kernel == kWSolveChainW2 ||
                                      s.kernel == kWSolveChainW4 || s.kernel == kWBsolveChainW || s.kernel == kWBsolveChainMrhs;
            if (chain_kernel) CHECK(l.form == kFormChain);
            if (s.kernel == kWSolvePanel) CHECK(l.form == kFormEach);
            if (s.kernel == kWBsolveBelow || s.kernel == kWBsolveChainW || s.kernel == kWBsolveBlock1) CHECK(nrhs == 1);
        }
        if (R.one) CHECK(marked);
        if (!marked) CHECK(i < R.body ? s.kernel != kWitnessCount : s.kernel == kWTransposeX);
    }
    CHECK(route_kernels(R, nullptr, 0) == enqueued);
    std::vector<int32_t> names((size_t)enqueued + 1, -7);
    CHECK(route_kernels(R, names.data(), enqueued) == enqueued && names[(size_t)enqueued] == -7);
    CHECK(R.use_xt == (R.ldq > 0) && (!R.one || (R.one_cap == 1 || R.one_cap == 4 || R.one_cap == 8)));
    CHECK(!R.one || (!R.use_xt && !R.arm_wide && R.scratch == 0 && R.armed == 0 && nrhs <= R.one_cap));
}

int main() {
    const int nx = 13;
    std::vector<int> Ap, Ai, perm;
    std::vector<double> Ax;
    grid_spd_lower(nx, nx, nx, 7, 0.1, Ap, Ai, Ax);
    grid_nested_dissection(nx, nx, nx, 27, perm);
    const int nrelax[3] = {4, 16, 48};
    const double zrelax[3] = {0.8, 0.1, 0.05};
    Symbolic sym;
    analyze(nx * nx * nx, Ap.data(), Ai.data(), Ax.data(), perm.data(), nrelax, zrelax, sym);

    const std::vector<std::pair<const char*, Env>> variants = {
        {"default", {{"PARSY_SOLVE_ONE", "0"}}},
        {"one", {{"PARSY_SOLVE_ONE", "2"}}},
        {"big", {{"PARSY_SOLVE_ONE", "0"}, {"PARSY_PIECE_WIDTH", "128"}, {"PARSY_BIG_MINK", "16"}, {"PARSY_CHAIN_SPLIT", "2"}}},
        {"unfused", {{"PARSY_SOLVE_ONE", "0"}, {"PARSY_FORCE_UNFUSED", "1"}}},
        {"below", {{"PARSY_SOLVE_ONE", "0"}, {"PARSY_BSOLVE_BELOW", "2"}}},
        {"subtrees", {{"PARSY_SOLVE_ONE", "0"}, {"PARSY_SUBTREES", "2"}}},
        {"bands", {{"PARSY_SOLVE_ONE", "0"}, {"PARSY_SUBTREES", "2"}, {"PARSY_SUB_TIER_MIN_TREES", "2"}}},
        {"one_subtrees", {{"PARSY_SOLVE_ONE", "2"}, {"PARSY_SUBTREES", "2"}}},
    };
    std::vector<std::pair<const char*, SolveGates>> gates(5);
    gates[0].first = "default";
    gates[1].first = "mrhs_min=1", gates[1].second.mrhs_min = 1, gates[1].second.chain_mrhs_min = 1;
    gates[2].first = "backward matrix cores everywhere", gates[2].second.bmrhs_wide_only = false, gates[2].second.bmrhs_wide_blocks = 8,
    gates[2].second.bchain_min_blocks = 4;
    gates[3].first = "xt from 5, few chunks 0, halves 1, no tiers", gates[3].second.xt_min = 5, gates[3].second.xt_min_set = true,
    gates[3].second.mrhs_min = 5, gates[3].second.chain_few_chunks = 0, gates[3].second.small_halves_min = 1, gates[3].second.sub_mrhs_min = 0;
    gates[4].first = "bmrhs_min=1000", gates[4].second.bmrhs_min = 1000, gates[4].second.mrhs_min = 1000;

    bool kind_seen[kLaunchDense + 1] = {}, form_seen[2][3] = {}, band_seen = false, one_seen[2] = {};
    size_t routes = 0, level_steps = 0;
    for (const auto& v : variants) {
        const Schedule S = plan_of(sym, v.second);
        std::string what;
        CHECK(check_schedule(S, what) == 0);
        for (int d = 0; d < 2; ++d)
            for (const Launch& l : d ? S.bsolve : S.solve) kind_seen[l.kind] = true, form_seen[d][l.form] = true;
        for (const auto& g : gates)
            for (int tiers = 0; tiers < 2; ++tiers)
                for (int off = 0; off < 2; ++off)
                    for (int d = 0; d < 2; ++d)
                        for (int nrhs : {1, 3, 5, 17, 65}) {   // (3: the ONE-launch kernels' class of 4)
                            const bool backward = d != 0;
                            RouteRuntime rt;
                            rt.sub_ntiers = tiers ? (int)S.sub_tiers.size() : 0;
                            rt.one_off[0] = rt.one_off[1] = off != 0;
                            g_what = std::string(v.first) + " / " + g.first + " / tiers " + std::to_string(tiers) + " off " + std::to_string(off) +
                                     (backward ? " backward " : " forward ") + std::to_string(nrhs);
                            const int ldx = S.n + 3;
                            SolveRoute R;
                            solve_route(S, g.second, rt, nrhs, ldx, backward, R);
                            std::vector<int> used((backward ? S.bsolve : S.solve).size(), 0);
                            check_route(S, rt, R, backward, nrhs, used);
                            CHECK(!(R.one && off));
                            one_seen[d] |= R.one;
                            for (const SolveStep& s : R.steps) band_seen |= s.tier > 0;
                            // every record is in the route of a solve by level launches, but those the tiers cover
                            if (!R.one && !(tiers && S.sub_cover_level >= 0 && g.second.sub_mrhs_min > 0 && nrhs >= g.second.sub_mrhs_min))
                                for (int u : used) CHECK(u == 1);
                            // 5. built again into the same route: the same steps in the same storage
                            const SolveStep* where = R.steps.data();
                            const std::vector<SolveStep> before = R.steps;
                            solve_route(S, g.second, rt, nrhs, ldx, backward, R);
                            CHECK(R.steps.data() == where && R.steps.size() == before.size());
                            for (size_t i = 0; i < before.size(); ++i)
                                CHECK(R.steps[i].kernel == before[i].kernel && R.steps[i].launch == before[i].launch && R.steps[i].tier == before[i].tier);
                            ++routes;

                            // the same solve in steps of one level each
                            std::fill(used.begin(), used.end(), 0);
                            const int nlev = S.nlevels;
                            SolveRoute first_step;
                            for (int k = 0; k < nlev; ++k) {
                                const int lev = backward ? nlev - 1 - k : k;
                                SolveRoute& Q = k == 0 ? first_step : R;
                                solve_route_levels(S, g.second, rt, nrhs, ldx, backward, lev, lev + 1, k == 0, k == nlev - 1, Q);
                                check_route(S, rt, Q, backward, nrhs, used);
                                CHECK(!Q.one && !Q.use_xt && !Q.arm_wide && Q.tail == Q.steps.size());
                                if (k > 0) CHECK(Q.body == 0 && Q.scratch == 0 && Q.armed == 0 && !Q.bpart && !Q.dinv);
                                for (const SolveStep& s : Q.steps) CHECK(s.tier <= 0);   // (no bands)
                                ++level_steps;
                            }
                            for (int u : used) CHECK(u == 1);
                            CHECK(first_step.dinv == (S.solve_wide_list.size() >= 2) && first_step.body == (first_step.dinv ? 1u : 0u));
                        }
    }
    g_what = "coverage";
    for (int k : {kLaunchBackBelow, kLaunchSolveSmall, kLaunchSolvePanel, kLaunchSolveFixup, kLaunchBackBlock}) CHECK(kind_seen[k]);
    for (int d = 0; d < 2; ++d) CHECK(form_seen[d][kFormEach] && form_seen[d][kFormChain] && form_seen[d][kFormSubtrees]);
    CHECK(band_seen && one_seen[0] && one_seen[1]);
    // every solve kernel a route can name was named by one of them (k_rhs_ones, k_copy_segments: no solve's), but
    // k_solve_small_mrhs<32> and k_bsolve_tiny<32>: no launch of this grid has a widest supernode of 17 .. 32 columns (the
    // catalogue's shapes narrow_lo and narrow_32 have: test_solve_route_host.py)
    static const std::vector<Serves> serves = serves_table();
    for (int k = 0; k < kWitnessCount; ++k)
        if (serves[(size_t)k].dir && !seen_kernel[k] && k != kWSolveSmallMrhs32 && k != kWBsolveTiny32) {
            std::fprintf(stderr, "witness entry %d in no route\n", k);
            CHECK(seen_kernel[k]);
        }
    std::printf("solve_route: %zu routes and %zu level steps consistent, every routed kernel seen\n", routes, level_steps);
    return 0;
}
