// Host schedule of the selected inversion (selinv.hpp): block-column tree, levels, gather map, path split, check.
// Plain C++ over the solve view of the schedule (Schedule::sn, rows, sparent), so host-only plans have it too.
#include "selinv.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../include/parsy_amd.h"
#include "errors.hpp"
#include "plan_fwd.hpp"

namespace parsy {

namespace {

int nblocks(int w) { return (w + kTile - 1) / kTile; }

}  // namespace

int selinv_tiled_min() {
    const char* e = std::getenv("PARSY_SELINV_TILED_MIN");
    if (!e || !*e) return kSelinvTiledMin;
    const long v = std::strtol(e, nullptr, 10);
    return v < 0 ? 0 : v > (1L << 30) ? (1 << 30) : (int)v;
}

bool build_selinv(const Schedule& S, SelinvSchedule& X, std::string& what) {
    X = SelinvSchedule();
    const int ns = S.nsuper;
    std::vector<int32_t> bc0((size_t)ns + 1, 0);
    for (int s = 0; s < ns; ++s) bc0[s + 1] = bc0[s] + nblocks(S.sn[s].w);
    X.nbc = bc0[ns];
    X.bc_sn.resize(X.nbc);
    X.bc_j.resize(X.nbc);
    X.bc_parent.resize(X.nbc);
    X.bc_depth.assign(X.nbc, -1);
    for (int s = 0; s < ns; ++s)
        for (int j = 0; j < nblocks(S.sn[s].w); ++j) {
            const int b = bc0[s] + j;
            X.bc_sn[b] = s;
            X.bc_j[b] = j;
            const int ps = S.sparent[s];
            X.bc_parent[b] = j + 1 < nblocks(S.sn[s].w) ? b + 1 : ps >= 0 ? bc0[ps] : -1;
        }
    // depth of the last block column of every supernode: dlast[s] = dlast[parent] + blocks of the parent (memoised walk)
    std::vector<int> dlast((size_t)ns, -1), chain;
    for (int s = 0; s < ns; ++s) {
        int t = s;
        chain.clear();
        while (t >= 0 && dlast[t] < 0) {
            chain.push_back(t);
            t = S.sparent[t];
            if ((int)chain.size() > ns) return what = "the supernodal etree has a cycle", false;
        }
        for (int k = (int)chain.size() - 1; k >= 0; --k) {
            const int u = chain[k], p = S.sparent[u];
            dlast[u] = p < 0 ? 0 : dlast[p] + nblocks(S.sn[p].w);
        }
    }
    int maxd = -1;
    for (int b = 0; b < X.nbc; ++b) {
        const int s = X.bc_sn[b];
        X.bc_depth[b] = dlast[s] + (nblocks(S.sn[s].w) - 1 - X.bc_j[b]);
        maxd = std::max(maxd, X.bc_depth[b]);
    }
    X.levels = maxd + 1;
    X.lvl_ptr.assign((size_t)X.levels + 1, 0);
    for (int b = 0; b < X.nbc; ++b) X.lvl_ptr[X.bc_depth[b] + 1] += 1;
    for (int l = 0; l < X.levels; ++l) X.lvl_ptr[l + 1] += X.lvl_ptr[l];
    X.lvl_set.resize(X.nbc);
    {
        std::vector<int32_t> fill(X.lvl_ptr.begin(), X.lvl_ptr.end() - 1);
        for (int b = 0; b < X.nbc; ++b) X.lvl_set[fill[X.bc_depth[b]]++] = b;
    }
    // nominal flops
    for (int b = 0; b < X.nbc; ++b) {
        const SnDesc& d = S.sn[X.bc_sn[b]];
        const int j0 = X.bc_j[b] * kTile, wb = std::min(kTile, d.w - j0);
        const double m = d.r - j0 - wb, w = wb;
        X.flops += 2.0 * m * m * w + 4.0 * m * w * w;
    }
    // gather map: identity runs now, ancestor runs grouped by owner (one dense position table per owner)
    std::vector<int32_t> col2sn((size_t)S.n, -1);
    for (int s = 0; s < ns; ++s)
        for (int c = S.sn[s].c0; c < S.sn[s].c0 + S.sn[s].w; ++c) col2sn[c] = s;
    X.cb.assign((size_t)S.ssize, 0);
    X.mo.assign((size_t)S.ssize, 0);
    struct Run { int32_t s, lb; int64_t off; };
    std::vector<std::vector<Run>> by_owner((size_t)ns);
    int64_t len = 0;
    for (int s = 0; s < ns; ++s) {
        const SnDesc& d = S.sn[s];
        for (int q = 0; q < d.w; ++q) {
            X.cb[d.pi + q] = d.px + (int64_t)q * d.r;
            X.mo[d.pi + q] = len;
        }
        len += d.r;
        for (int q = d.w; q < d.r;) {
            const int row = S.rows[d.pi + q];
            const int K = (row >= 0 && row < S.n) ? col2sn[row] : -1;
            if (K < 0) return what = "row id out of range in supernode " + std::to_string(s), false;
            if (K == s) return what = "off-diagonal row inside its own supernode " + std::to_string(s), false;
            const SnDesc& k = S.sn[K];
            int e = q;
            while (e < d.r && S.rows[d.pi + e] < k.c0 + k.w) ++e;
            by_owner[K].push_back({s, q, len});
            for (int t = q; t < e; ++t) {
                X.cb[d.pi + t] = k.px + (int64_t)(S.rows[d.pi + t] - k.c0) * k.r;
                X.mo[d.pi + t] = len - q;
            }
            len += d.r - q;
            q = e;
        }
    }
    X.gmap.assign((size_t)len, -1);
    std::vector<int32_t> where((size_t)S.n, -1);
    for (int s = 0; s < ns; ++s) {
        const SnDesc& d = S.sn[s];
        int64_t off = X.mo[d.pi];
        for (int t = 0; t < d.r; ++t) X.gmap[off + t] = t;
    }
    for (int K = 0; K < ns; ++K) {
        if (by_owner[K].empty()) continue;
        const SnDesc& k = S.sn[K];
        for (int t = 0; t < k.r; ++t) where[S.rows[k.pi + t]] = t;
        for (const Run& R : by_owner[K]) {
            const SnDesc& d = S.sn[R.s];
            for (int t = R.lb; t < d.r; ++t) {
                const int pos = where[S.rows[d.pi + t]];
                if (pos < 0)
                    return what = "row " + std::to_string(S.rows[d.pi + t]) + " of supernode " + std::to_string(R.s) +
                                  " is not in the row list of its ancestor " + std::to_string(K), false;
                X.gmap[R.off + (t - R.lb)] = pos;
            }
        }
        for (int t = 0; t < k.r; ++t) where[S.rows[k.pi + t]] = -1;
    }
    return true;
}

void split_selinv(const Schedule& S, const SelinvSchedule& X, int tiled_min, SelinvSplit& o) {
    o = SelinvSplit();
    o.tiled_min = tiled_min;
    o.lvl_bc.assign((size_t)X.levels + 1, 0);
    o.lvl_ntiled.assign((size_t)X.levels, 0);
    o.lvl_task.assign((size_t)X.levels + 1, 0);
    for (int l = 0; l < X.levels; ++l) {
        int64_t slots = 0;
        for (int pass = 0; pass < 2; ++pass)   // 0: tiled, 1: small
            for (int e = X.lvl_ptr[l]; e < X.lvl_ptr[l + 1]; ++e) {
                const int b = X.lvl_set[e];
                const SnDesc& d = S.sn[X.bc_sn[b]];
                SelinvBc B;
                B.px = d.px;
                B.pi = d.pi;
                B.r = d.r;
                B.j0 = X.bc_j[b] * kTile;
                B.wb = std::min(kTile, d.w - B.j0);
                B.m = d.r - B.j0 - B.wb;
                B.tslot = B.yslot = B.pslot = -1;
                const bool tiled = B.m >= tiled_min;
                if (tiled != (pass == 0)) continue;
                if (tiled) {
                    const int nt = (B.m + kTile - 1) / kTile;
                    B.tslot = o.lvl_ntiled[l]++;
                    B.yslot = (int32_t)(slots);   // counted from the end of the T slots below
                    slots += nt;
                    for (int t = 0; t < nt; ++t) {
                        o.tasks.push_back((int32_t)o.bcs.size());
                        o.tasks.push_back(t);
                    }
                }
                o.bc_id.push_back(b);
                o.bcs.push_back(B);
            }
        o.lvl_bc[l + 1] = (int32_t)o.bcs.size();
        o.lvl_task[l + 1] = (int32_t)(o.tasks.size() / 2);
        const int nt = o.lvl_ntiled[l];
        // slots: T (nt), then Y (slots), then the partials (slots)
        for (int e = o.lvl_bc[l]; e < o.lvl_bc[l] + nt; ++e) {
            o.bcs[e].yslot += nt;
            o.bcs[e].pslot = o.bcs[e].yslot + (int32_t)slots;
        }
        o.scratch_slots = std::max<int64_t>(o.scratch_slots, nt + 2 * slots);
        o.ntiled += nt;
        const bool has_small = o.lvl_bc[l + 1] - o.lvl_bc[l] > nt;
        o.launches += (nt > 0 ? 2 : 0) + (o.lvl_task[l + 1] > o.lvl_task[l] ? 2 : 0) + (has_small ? 1 : 0);
    }
}

int64_t check_selinv(const Schedule& S, const SelinvSchedule& X, const SelinvSplit& sp, std::string& what) {
    int64_t bad = 0;
    auto fail = [&](const std::string& msg) {
        if (bad++ == 0) what = msg;
    };
    // every block column scheduled once, on a deeper level than its parent
    std::vector<int> seen((size_t)X.nbc, 0), level_of((size_t)X.nbc, -1);
    for (int l = 0; l < X.levels; ++l)
        for (int e = sp.lvl_bc[l]; e < sp.lvl_bc[l + 1]; ++e) {
            const int b = sp.bc_id[e];
            if (b < 0 || b >= X.nbc) {
                fail("descriptor " + std::to_string(e) + " names no block column");
                continue;
            }
            seen[b] += 1;
            level_of[b] = l;
        }
    for (int b = 0; b < X.nbc; ++b) {
        if (seen[b] != 1) fail("block column " + std::to_string(b) + " is scheduled " + std::to_string(seen[b]) + " times");
        const int p = X.bc_parent[b];
        if (p >= 0 && level_of[b] >= 0 && level_of[b] <= level_of[p])
            fail("block column " + std::to_string(b) + " is not on a deeper level than its parent " + std::to_string(p));
    }
    // every gather position holds the row id it stands for: per run of positions that share an owner K (the identity
    // run of s's own columns, then one per ancestor), the column bases and the positions of rows[lb ..] in K's list
    std::vector<int32_t> col2sn((size_t)S.n, -1);
    for (int s = 0; s < S.nsuper; ++s)
        for (int c = S.sn[s].c0; c < S.sn[s].c0 + S.sn[s].w; ++c) col2sn[c] = s;
    const int64_t glen = (int64_t)X.gmap.size();
    for (int s = 0; s < S.nsuper; ++s) {
        const SnDesc& d = S.sn[s];
        for (int lb = 0, e; lb < d.r; lb = e) {
            const int row0 = S.rows[d.pi + lb];
            const int K = lb < d.w ? s : (row0 >= 0 && row0 < S.n ? col2sn[row0] : -1);
            if (K < 0 || (lb >= d.w && K == s)) {
                fail("row " + std::to_string(row0) + " of supernode " + std::to_string(s) + " has no ancestor owner");
                break;
            }
            const SnDesc& k = S.sn[K];
            e = lb < d.w ? d.w : lb;
            while (lb >= d.w && e < d.r && S.rows[d.pi + e] < k.c0 + k.w) ++e;
            for (int q = lb; q < e; ++q) {
                const int row = S.rows[d.pi + q];
                if (X.cb[d.pi + q] != k.px + (int64_t)(row - k.c0) * k.r || X.mo[d.pi + q] != X.mo[d.pi + lb]) {
                    fail("map entry of row " + std::to_string(row) + " in supernode " + std::to_string(s) + " is wrong");
                    break;
                }
            }
            for (int p = lb; p < d.r; ++p) {
                const int64_t g = X.mo[d.pi + lb] + p;
                const int pos = (g >= 0 && g < glen) ? X.gmap[g] : -1;
                if (pos < 0 || pos >= k.r || S.rows[k.pi + pos] != S.rows[d.pi + p]) {
                    fail("gather position of row " + std::to_string(S.rows[d.pi + p]) + " for supernode " +
                         std::to_string(s) + " in supernode " + std::to_string(K) + " does not hold that row");
                    break;
                }
            }
        }
    }
    return bad;
}

}  // namespace parsy

using parsy::set_last_error;

extern "C" long long parsy_selinv_check(const parsy_plan* pl) {
    if (!pl) {
        set_last_error("parsy_selinv_check: null plan");
        return -1;
    }
    const parsy::Schedule& S = parsy::plan_schedule(pl);
    parsy::SelinvSchedule X;
    parsy::SelinvSplit sp;
    std::string what;
    if (!parsy::build_selinv(S, X, what)) {
        set_last_error("parsy_selinv_check: " + what);
        return 1;
    }
    parsy::split_selinv(S, X, parsy::selinv_tiled_min(), sp);
    const long long bad = (long long)parsy::check_selinv(S, X, sp, what);
    if (bad) set_last_error("parsy_selinv_check: " + what);
    return bad;
}
