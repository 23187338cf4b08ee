// Stand-alone check of the launch records (csrc/schedule.hpp: Launch) and of the rule check_schedule holds them to: a
// field that a record's kind and form do not have keeps its default.  test_launch_record_host.py compiles it together
// with schedule.cpp, inspector.cpp and gen.cpp as host C++ with the address and undefined-behaviour sanitizers and runs
// it; nothing of HIP, no device.
//   1. the plans of a 13 x 13 x 13 7-point grid under geometric nested dissection -- default knobs; with pieces, BIG
//      launches and two chain launches per level; and the variants listed at `variants` for the kinds and forms those
//      two do not schedule on so small a grid -- are consistent (check_schedule == 0), and all ten kinds and all three
//      forms occur among them, in `solve` and `bsolve` too.  (13, not 12: at 12 x 12 x 12 the plan with BIG launches
//      has no DENSE one; one more point per axis is the smallest grid that has.)
//   2. one wrong field at a time, planted in a copy, is reported with a message that names the launch.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "gen.hpp"
#include "inspector.hpp"
#include "schedule.hpp"

using namespace parsy;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

using Env = std::vector<std::pair<const char*, const char*>>;

static Schedule plan_of(const Symbolic& sym, const Env& env) {
    for (const auto& kv : env) setenv(kv.first, kv.second, 1);
    Schedule S;
    build_schedule(pattern_ref(sym), sym.p.data(), sym.A2.p.data(), sym.A2.i.data(), nullptr, S);
    for (const auto& kv : env) unsetenv(kv.first);
    return S;
}

static int64_t check(const Schedule& S, std::string& what) {
    what.clear();
    return check_schedule(S, what);
}

// the first launch of `seq` that `pick` accepts (the plans are chosen so that there is one)
static Launch& find(std::vector<Launch>& seq, const std::function<bool(const Launch&)>& pick) {
    for (Launch& l : seq)
        if (pick(l)) return l;
    std::fprintf(stderr, "no launch to plant the fault in\n");
    std::exit(1);
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

    const Env big = {{"PARSY_PIECE_WIDTH", "128"}, {"PARSY_BIG_MINK", "16"}, {"PARSY_CHAIN_SPLIT", "2"}};
    // The two plans, and what they leave out on this grid: the per-block-column form and SOLVE_FIXUP exist only where a
    // chain launch is refused (PARSY_FORCE_UNFUSED=1); no supernode has the 512 rows below its columns that BACK_BELOW
    // starts from (PARSY_BSOLVE_BELOW=2: from one row on); and 2197 columns are too few for the subtree launches to pay
    // (PARSY_SUBTREES=2 asks for them whatever the size).  A larger grid instead of these knobs would have to be far
    // larger: the subtree launches of the solves start at 2048 eligible supernodes.
    const std::vector<std::pair<const char*, Env>> variants = {
        {"default", {}},
        {"big", big},
        {"unfused", {{"PARSY_FORCE_UNFUSED", "1"}}},
        {"below", {{"PARSY_BSOLVE_BELOW", "2"}}},
        {"subtrees", {{"PARSY_SUBTREES", "2"}}},
    };
    std::vector<Schedule> plans;
    bool kind_seen[kLaunchDense + 1] = {};
    bool form_seen[3][3] = {};   // [chol | solve | bsolve][form]
    bool rows_only_seen[2] = {}, side_seen[2] = {};
    for (const auto& v : variants) {
        plans.push_back(plan_of(sym, v.second));
        const Schedule& S = plans.back();
        std::string what;
        const int64_t bad = check(S, what);
        if (bad != 0) std::fprintf(stderr, "plan %s: %lld violations, first: %s\n", v.first, (long long)bad, what.c_str());
        CHECK(bad == 0);
        int which = 0;
        for (const std::vector<Launch>* seq : {&S.chol, &S.solve, &S.bsolve}) {
            for (const Launch& l : *seq) {
                CHECK(l.kind >= 0 && l.kind <= kLaunchDense && l.form >= 0 && l.form <= 2);
                kind_seen[l.kind] = true;
                form_seen[which][l.form] = true;
                if (l.kind == kLaunchChain) rows_only_seen[l.rows_only != 0] = true;
                if (l.kind == kLaunchBig || l.kind == kLaunchDense) side_seen[l.side != 0] = true;
            }
            ++which;
        }
    }
    for (int k = 0; k <= kLaunchDense; ++k) {
        if (!kind_seen[k]) std::fprintf(stderr, "launch kind %d does not occur\n", k);
        CHECK(kind_seen[k]);
    }
    CHECK(form_seen[0][kFormEach] && form_seen[0][kFormSubtrees]);                            // SMALL
    CHECK(form_seen[1][kFormEach] && form_seen[1][kFormChain] && form_seen[1][kFormSubtrees]);
    CHECK(form_seen[2][kFormEach] && form_seen[2][kFormChain] && form_seen[2][kFormSubtrees]);
    CHECK(rows_only_seen[0] && rows_only_seen[1]);   // both chain launches of a level
    CHECK(side_seen[0] && side_seen[1]);             // NEXT and PUSH

    // ---- planted faults: one wrong field each, in a copy of the plan that has such a launch
    struct Fault {
        const char* name;
        size_t plan;
        std::function<std::string(Schedule&)> plant;   // returns "list[index]" of the launch it changed
    };
    auto tag = [](const char* list, const std::vector<Launch>& seq, const Launch& l) {
        return std::string(list) + "[" + std::to_string(&l - seq.data()) + "]";
    };
    auto kind_is = [](int kind, int form) { return [=](const Launch& l) { return l.kind == kind && l.form == form; }; };
    const std::vector<Fault> faults = {
        {"a ticket on a TILES launch", 1, [&](Schedule& S) {
             Launch& l = find(S.chol, kind_is(kLaunchTiles, kFormEach));
             l.ticket = 1;
             return tag("chol", S.chol, l);
         }},
        {"a task range on a SOLVE_SMALL launch", 0, [&](Schedule& S) {
             Launch& l = find(S.solve, kind_is(kLaunchSolveSmall, kFormEach));
             l.task_first = 0, l.task_count = 1;
             return tag("solve", S.solve, l);
         }},
        {"width_class = 3", 0, [&](Schedule& S) {
             Launch& l = find(S.bsolve, kind_is(kLaunchBackBlock, kFormEach));
             l.width_class = 3;
             return tag("bsolve", S.bsolve, l);
         }},
        {"form = kFormChain on a SMALL launch", 0, [&](Schedule& S) {
             Launch& l = find(S.chol, kind_is(kLaunchSmall, kFormEach));
             l.form = kFormChain;
             return tag("chol", S.chol, l);
         }},
        {"wait_level = 2 on a main-stream launch", 1, [&](Schedule& S) {
             Launch& l = find(S.chol, [](const Launch& q) { return q.kind == kLaunchChain && !q.side; });
             l.wait_level = 2;
             return tag("chol", S.chol, l);
         }},
        {"task_first + task_count past the end of solve_mtasks", 0, [&](Schedule& S) {
             Launch& l = find(S.solve, kind_is(kLaunchSolvePanel, kFormChain));
             l.task_first = (int32_t)S.solve_mtasks.size() - l.task_count + 1;
             return tag("solve", S.solve, l);
         }},
        {"a stage size on a SOLVE_PANEL launch", 2, [&](Schedule& S) {
             Launch& l = find(S.solve, kind_is(kLaunchSolvePanel, kFormEach));
             l.stage = 64;
             return tag("solve", S.solve, l);
         }},
        {"a width on a BACK_BLOCK subtree launch", 4, [&](Schedule& S) {
             Launch& l = find(S.bsolve, kind_is(kLaunchBackBlock, kFormSubtrees));
             l.width = 16;
             return tag("bsolve", S.bsolve, l);
         }},
        {"a solve launch in the factorization's list", 0, [&](Schedule& S) {
             Launch& l = find(S.chol, kind_is(kLaunchSmall, kFormEach));
             l.kind = kLaunchSolveSmall;
             return tag("chol", S.chol, l);
         }},
    };
    for (const Fault& f : faults) {
        Schedule S = plans[f.plan];
        const std::string where = f.plant(S);
        std::string what;
        const int64_t bad = check(S, what);
        if (bad == 0 || what.find(where) == std::string::npos)
            std::fprintf(stderr, "planted: %s in %s -> %lld violations, first: %s\n", f.name, where.c_str(), (long long)bad, what.c_str());
        CHECK(bad != 0);
        CHECK(what.find(where) != std::string::npos);
    }
    std::printf("launch_record: %zu plans consistent, every kind and form seen, %zu planted faults reported\n", plans.size(),
                faults.size());
    return 0;
}
