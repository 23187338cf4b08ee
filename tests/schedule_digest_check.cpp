// Stand-alone digests of whole schedules (csrc/schedule_digest.hpp).  test_schedule_digest_host.py compiles it together with
// schedule.cpp, inspector.cpp and gen.cpp as host C++ with the address and undefined-behaviour sanitizers and runs it;
// nothing of HIP, no device.
// build_schedule on three generated grids -- the tiny2d, mid3d and nd24k workloads of parsy_bench_amd/matrices.py, same
// generator, same ordering, same relaxation -- with compute_units in {0, 32, 256, 304}: a host-only plan always passes 0,
// so the branches that follow the device's size (walker_batch, the cost cap and the member threshold of the subtrees) are
// reached from here only.  Prints one line per (grid, compute_units) with one hash over the field hashes, as
// tools/schedule_digests.py does for plans; with --fields one line per field: what a device plan of 256 compute units must
// reproduce (schedule_digests.py --device).
// Usage: schedule_digest_check [--fields]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gen.hpp"
#include "inspector.hpp"
#include "schedule.hpp"
#include "schedule_digest.hpp"

using namespace parsy;

int main(int argc, char** argv) {
    struct Grid { const char* name; int nx, ny, nz, stencil, leaf; };
    const Grid grids[3] = {{"tiny2d", 12, 12, 1, 5, 8}, {"mid3d", 20, 20, 20, 27, 27}, {"nd24k", 42, 42, 42, 27, 27}};
    const bool fields = argc > 1 && std::strcmp(argv[1], "--fields") == 0;
    const int nrelax[3] = {4, 16, 48};
    const double zrelax[3] = {0.8, 0.1, 0.05};
    for (int g = 0; g < 3; ++g) {
        const Grid& G = grids[g];
        std::vector<int> Ap, Ai, perm;
        std::vector<double> Ax;
        grid_spd_lower(G.nx, G.ny, G.nz, G.stencil, 0.1, Ap, Ai, Ax);
        grid_nested_dissection(G.nx, G.ny, G.nz, G.leaf, perm);
        Symbolic sym;
        analyze(G.nx * G.ny * G.nz, Ap.data(), Ai.data(), Ax.data(), perm.data(), nrelax, zrelax, sym);
        for (int cus : {0, 32, 256, 304}) {
            Schedule S;
            build_schedule(pattern_ref(sym), sym.p.data(), sym.A2.p.data(), sym.A2.i.data(), nullptr, S, cus);
            std::string what;
            if (check_schedule(S, what) != 0) {
                std::fprintf(stderr, "%s, %d compute units: %s\n", G.name, cus, what.c_str());
                return 1;
            }
            Schedule again;   // the same plan built twice: equal in every field
            build_schedule(pattern_ref(sym), sym.p.data(), sym.A2.p.data(), sym.A2.i.data(), nullptr, again, cus);
            const ScheduleDigest d = schedule_digest(S), d2 = schedule_digest(again);
            Fnv1a whole;
            for (size_t f = 0; f < d.size(); ++f) {
                if (d[f].second != d2[f].second) {
                    std::fprintf(stderr, "%s, %d compute units: field %s differs between two builds\n", G.name, cus, d[f].first);
                    return 1;
                }
                whole.value(d[f].second);
                if (fields) std::printf("check %s cus=%d\t%s\t%016llx\n", G.name, cus, d[f].first, (unsigned long long)d[f].second);
            }
            if (!fields) std::printf("%016llx  check %s cus=%d\n", (unsigned long long)whole.h, G.name, cus);
        }
    }
    return 0;
}
