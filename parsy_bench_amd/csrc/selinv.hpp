// Selected inversion: Z = (P A P')^-1 on the stored pattern of L (the Takahashi recurrences), and log det A.
//
// Host schedule (selinv.cpp, plain C++: host-only plans build and check it too) and the device state of a plan that has
// called parsy_selinv_device (selinv_kernels.hip).  L is cut into BLOCK COLUMNS of at most 64 columns (a supernode of
// width w gives ceil(w / 64)).  Block column b (columns j0 .. j0 + wb of supernode s) has R_b = the panel rows below its
// columns (positions p0 = j0 + wb .. r of s's row list: s's later columns, then its off-diagonal rows) and computes
//     T = L_bb^-1,  Y = L(R_b, b) T,  Z(R_b, b) = -Z(R_b, R_b) Y,  Z(b, b) = T'T - Y' Z(R_b, b).
// The parent of a block column is the next block column of its supernode, or the first one of the supernode's etree
// parent; a block column reads only the Z of its ancestors, so the work runs level by level from the root (level 0).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "schedule.hpp"

struct parsy_plan;

namespace parsy {

// Default |R_b| from which a block column takes the tiled path (PARSY_SELINV_TILED_MIN).  Measured on the MI355X
// (profiles/selinv_bench_small.json): every threshold above 0 was slower -- ex15-class 0.72 ms at 0, 0.78 at 32, 1.40 at
// 96, 1.34 all small; nd24k-class 40.7 / 40.8 / 42.7 / 5897 ms; parabolic_fem-class 16.8 / 17.0 / 19.7 / 624 ms.
constexpr int kSelinvTiledMin = 0;

// One block column as the kernels read it.
struct SelinvBc {
    int64_t px;       // offset of the supernode's panel in lValues / Z
    int64_t pi;       // offset of its row ids in lR (and of its row positions in the gather map's cb / mo)
    int32_t r;        // rows of the panel (its leading dimension)
    int32_t j0, wb;   // first column of the block inside the supernode, and its width (<= 64)
    int32_t m;        // |R_b| = r - j0 - wb
    int32_t tslot;    // tiled path: 64 x 64 slot of T in the level's scratch
    int32_t yslot;    // tiled path: first 64 x 64 slot of Y in the level's scratch (tile t: yslot + t)
    int32_t pslot;    // tiled path: first 64 x 64 slot of the partials Y_t' Z_t (tile t: pslot + t)
};

// The pattern's part: the block-column tree, its levels and the gather map.
struct SelinvSchedule {
    int nbc = 0, levels = 0;
    std::vector<int32_t> bc_sn, bc_j;         // per block column, in supernode order: its supernode and block index
    std::vector<int32_t> bc_parent, bc_depth; // parent block column (-1: a root) and depth (root: 0)
    std::vector<int32_t> lvl_ptr, lvl_set;    // block columns per level (levels + 1 / nbc entries), ascending ids
    // Gather map.  The entry Z(rows[p], rows[q]), p >= q positions in supernode s's row list, is at
    //     cb[s.pi + q] + gmap[mo[s.pi + q] + p]
    // cb: start in Z of the column rows[q] in the panel of the supernode K that owns that column; gmap[mo + p]: the
    // position of rows[p] in K's row list (K = s: the identity run of s's own columns; otherwise one run per ancestor K,
    // the positions of s's rows from K's first column on -- the factorization's relative positions).
    std::vector<int64_t> cb, mo;              // per row position (ssize entries)
    std::vector<int32_t> gmap;
    double flops = 0;                         // sum_b 2 |R_b|^2 wb + 4 |R_b| wb^2
};

// A split of the levels into the two kernel paths under one threshold.
struct SelinvSplit {
    int tiled_min = -1;
    std::vector<SelinvBc> bcs;         // level by level: the level's tiled block columns, then its small ones
    std::vector<int32_t> bc_id;        // block column of every descriptor
    std::vector<int32_t> lvl_bc;       // levels + 1: first descriptor of every level
    std::vector<int32_t> lvl_ntiled;   // per level: tiled descriptors
    std::vector<int32_t> tasks;        // (descriptor, 64-row tile of R_b) pairs of the tiled path, level by level
    std::vector<int32_t> lvl_task;     // levels + 1: first task of every level
    int64_t scratch_slots = 0;         // max over the levels of (tiled block columns + 2 x tiles), 64 x 64 doubles each
    int ntiled = 0, launches = 0;
};

// build: false with `what` set when the pattern breaks the containment the map relies on.
bool build_selinv(const Schedule& S, SelinvSchedule& X, std::string& what);
void split_selinv(const Schedule& S, const SelinvSchedule& X, int tiled_min, SelinvSplit& out);
int64_t check_selinv(const Schedule& S, const SelinvSchedule& X, const SelinvSplit& sp, std::string& what);
int selinv_tiled_min();   // PARSY_SELINV_TILED_MIN, read at every call (default kSelinvTiledMin)

struct SelinvState;   // the device state (feature_states.hpp)
SelinvState& selinv_state(parsy_plan* pl);   // (made on first use)

}  // namespace parsy
