// C ABI, device part: plan API and the drop-in operators (include/parsy_amd.h §1, §2); the host-buffer entry points
// (parsy_*_host) are in capi_hostcalls.hip.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <algorithm>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/parsy_amd.h"
#include "errors.hpp"
#include "hip_check.hpp"
#include "dist.hpp"
#include "executor.hpp"
#include "inspector.hpp"
#include "plan_util.hpp"
#include "refine.hpp"
#include "schedule_digest.hpp"
#include "cond.hpp"
#include "eigs.hpp"
#include "feature_states.hpp"

using parsy::set_last_error;

namespace {

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int pick_device() {
    // PARSY_DEVICE selects the HIP device of the drop-in operators (default 0)
    const char* e = std::getenv("PARSY_DEVICE");
    return e ? std::atoi(e) : 0;
}

// ---- plan cache of the drop-in operators -------------------------------------
// Pattern hash of the drop-in plan cache: 8 bytes per step in four independent lanes (the Flan-class pattern is
// hundreds of MB per call; a byte-at-a-time FNV was a measurable part of the call), folded FNV-style.
uint64_t fnv(uint64_t h, const void* p, size_t bytes) {
    const unsigned char* c = (const unsigned char*)p;
    uint64_t lane[4] = {h, h ^ 0x9E3779B97F4A7C15ULL, h ^ 0xC2B2AE3D27D4EB4FULL, h ^ 0x165667B19E3779F9ULL};
    size_t i = 0;
    for (; i + 32 <= bytes; i += 32)
        for (int k = 0; k < 4; ++k) {
            uint64_t w;
            std::memcpy(&w, c + i + 8 * k, 8);
            lane[k] = (lane[k] ^ w) * 1099511628211ULL;
            lane[k] ^= lane[k] >> 29;
        }
    for (int k = 0; k < 4; ++k) h = (h ^ lane[k]) * 1099511628211ULL;
    for (; i < bytes; ++i) {
        h ^= c[i];
        h *= 1099511628211ULL;
    }
    return h ^ (uint64_t)bytes;
}

struct CacheKey {
    const void* a;
    const void* b;
    const void* c;
    uint64_t hash;
    int n, supNo, kind;
    bool operator<(const CacheKey& o) const {
        return std::tie(a, b, c, hash, n, supNo, kind) < std::tie(o.a, o.b, o.c, o.hash, o.n, o.supNo, o.kind);
    }
};

std::mutex g_mu;
std::map<CacheKey, parsy_plan*> g_plans;

bool validate_partition(int supNo, int nLevels, const int* levelPtr, const int* parPtr,
                        const int* partition, const char* who) {
    if (!levelPtr || !parPtr || !partition || nLevels < 1) {
        set_last_error(std::string(who) + ": null H-level schedule");
        return false;
    }
    std::vector<char> seen(supNo, 0);
    const int nparts = levelPtr[nLevels];
    int cnt = 0;
    for (int q = 0; q < nparts; ++q)
        for (int k = parPtr[q]; k < parPtr[q + 1]; ++k) {
            const int s = partition[k];
            if (s < 0 || s >= supNo || seen[s]) {
                set_last_error(std::string(who) + ": H-level partition is not a permutation of the supernodes");
                return false;
            }
            seen[s] = 1;
            ++cnt;
        }
    if (cnt != supNo) {
        set_last_error(std::string(who) + ": H-level partition does not cover every supernode");
        return false;
    }
    return true;
}

bool validate_levelset(int supNo, int nLevels, const int* levelPtr, const int* levelSet, const char* who) {
    if (!levelPtr || !levelSet || nLevels < 1 || levelPtr[nLevels] != supNo) {
        set_last_error(std::string(who) + ": level set does not cover every supernode");
        return false;
    }
    std::vector<char> seen(supNo, 0);
    for (int k = 0; k < supNo; ++k) {
        const int s = levelSet[k];
        if (s < 0 || s >= supNo || seen[s]) {
            set_last_error(std::string(who) + ": level set is not a permutation of the supernodes");
            return false;
        }
        seen[s] = 1;
    }
    return true;
}

void loud(const char* who) {
    std::fprintf(stderr, "[parsy_amd] %s failed: %s\n", who, parsy_last_error());
}

// The plan of `key`, made by build() on first use (null: build failed, nothing is cached).
template <class Build>
parsy_plan* cached_plan(const CacheKey& key, Build build) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_plans.find(key);
    if (it != g_plans.end()) return it->second;
    parsy_plan* pl = build();
    if (pl) g_plans[key] = pl;
    return pl;
}

// Supernodal etree straight from L's pattern: the parent of a supernode is the supernode of its first below-diagonal row.
void tree_from_pattern(int n, int supNo, const int* super, const size_t* Li_ptr, const int* Li, std::vector<int>& col2sup,
                       std::vector<int>& sparent) {
    col2sup.assign((size_t)n, 0);
    sparent.assign((size_t)supNo, -1);
    for (int s = 0; s < supNo; ++s)
        for (int k = super[s]; k < super[s + 1]; ++k) col2sup[k] = s;
    for (int s = 0; s < supNo; ++s) {
        const int w = super[s + 1] - super[s];
        const size_t b = Li_ptr[super[s]], e = Li_ptr[super[s + 1]];
        if (e - b > (size_t)w) sparent[s] = col2sup[Li[b + w]];
    }
}

parsy_plan* cached_chol_plan(int n, int supNo, const int* blockSet, const size_t* lC,
                             const size_t* Li_ptr, const int* lR, const int* aTree,
                             const int* col2Sup, const int* cT, const int* rT, const int* c,
                             const int* r) {
    uint64_t h = 1469598103934665603ULL;
    h = fnv(h, blockSet, sizeof(int) * (supNo + 1));
    h = fnv(h, lR, sizeof(int) * Li_ptr[n]);
    h = fnv(h, c, sizeof(int) * (n + 1));
    h = fnv(h, r, sizeof(int) * c[n]);            // A's rows and L's row pointers decide where A lands in L
    h = fnv(h, Li_ptr, sizeof(size_t) * (n + 1));
    h = fnv(h, lC, sizeof(size_t) * (n + 1));
    h = fnv(h, aTree, sizeof(int) * supNo);
    return cached_plan(CacheKey{blockSet, lR, c, h, n, supNo, 0}, [&] {
        return parsy_plan_create(n, supNo, blockSet, lC, Li_ptr, lR, aTree, col2Sup, cT, rT, c, r, pick_device());
    });
}

// the PRUNE operator: no etree, no upper pattern; the supernodal etree comes from L's pattern
parsy_plan* cached_chol_plan_prune(int n, int supNo, const int* blockSet, const size_t* lC, const size_t* Li_ptr,
                                   const int* lR, const int* prunePtr, const int* pruneSet, const int* c,
                                   const int* r) {
    uint64_t h = 1469598103934665603ULL;
    h = fnv(h, blockSet, sizeof(int) * (supNo + 1));
    h = fnv(h, lR, sizeof(int) * Li_ptr[n]);
    h = fnv(h, c, sizeof(int) * (n + 1));
    h = fnv(h, r, sizeof(int) * c[n]);
    h = fnv(h, Li_ptr, sizeof(size_t) * (n + 1));
    h = fnv(h, lC, sizeof(size_t) * (n + 1));
    h = fnv(h, prunePtr, sizeof(int) * (supNo + 1));
    h = fnv(h, pruneSet, sizeof(int) * prunePtr[supNo]);
    return cached_plan(CacheKey{blockSet, lR, c, h, n, supNo, 2}, [&]() -> parsy_plan* {
        const int dev = pick_device();
        if (dev >= parsy_device_count()) {
            set_last_error("cholesky_left_par_05_prune: no usable HIP device " + std::to_string(dev) +
                           " (this library has no CPU fallback)");
            return nullptr;
        }
        std::vector<int> col2sup, sparent;
        tree_from_pattern(n, supNo, blockSet, Li_ptr, lR, col2sup, sparent);
        parsy::PatternRef P;
        P.n = n;
        P.nsuper = supNo;
        P.super = blockSet;
        P.col2sup = col2sup.data();
        P.sparent = sparent.data();
        P.i_ptr = Li_ptr;
        P.s = lR;
        P.prunePtr = prunePtr;
        P.pruneSet = pruneSet;
        return parsy::plan_build(P, lC, c, r, dev);
    });
}

parsy_plan* cached_solve_plan(int n, int supNo, const size_t* Lp, const int* Li, const size_t* Li_ptr,
                              const int* sup2col) {
    uint64_t h = 1469598103934665603ULL;
    h = fnv(h, sup2col, sizeof(int) * (supNo + 1));
    h = fnv(h, Li, sizeof(int) * Li_ptr[n]);
    h = fnv(h, Li_ptr, sizeof(size_t) * (n + 1));
    h = fnv(h, Lp, sizeof(size_t) * (n + 1));
    return cached_plan(CacheKey{sup2col, Li, Lp, h, n, supNo, 1}, [&]() -> parsy_plan* {
        std::vector<int> col2sup, sparent;
        tree_from_pattern(n, supNo, sup2col, Li_ptr, Li, col2sup, sparent);
        parsy::PatternRef P;
        P.n = n;
        P.nsuper = supNo;
        P.super = sup2col;
        P.col2sup = col2sup.data();
        P.sparent = sparent.data();
        P.i_ptr = Li_ptr;
        P.s = Li;
        if (parsy_device_count() < 1) {
            set_last_error("no usable HIP device: the BCSC solve has no CPU fallback in this library");
            return nullptr;
        }
        return parsy::plan_build(P, Lp, nullptr, nullptr, pick_device());
    });
}

// The body the three Cholesky operators share: the plan is held for the call (the staging buffers, flags and status of a
// cached plan belong to one call at a time), the factorization runs on host buffers, timing[0..2] = wall time since t0,
// 0, device time.  false (loudly): no plan or the call failed; otherwise *status is parsy_factor_status.
bool dropin_factor(const char* who, parsy_plan* pl, const double* values, double* lValues, double* timing, double t0,
                   int* status) {
    double dev_s = 0;
    std::unique_lock<std::mutex> use;
    if (pl) use = std::unique_lock<std::mutex>(pl->use_mu);
    if (!pl || parsy_factor_host(pl, values, lValues, &dev_s) != 0) {
        loud(who);
        return false;
    }
    if (timing) {
        timing[0] = now_s() - t0;
        timing[1] = 0.0;
        timing[2] = dev_s;
    }
    *status = parsy_factor_status(pl);
    return true;
}

int dropin_solve(const char* who, int n, size_t* Lp, int* Li, double* Lx, size_t* Li_ptr,
                 int* sup2col, int supNo, double* x) {
    if (!Lp || !Li || !x) return 0;  // reference: Triangular_BCSC.h:24
    parsy_plan* pl = cached_solve_plan(n, supNo, Lp, Li, Li_ptr, sup2col);
    std::unique_lock<std::mutex> use;
    if (pl) use = std::unique_lock<std::mutex>(pl->use_mu);
    if (!pl || parsy_solve_host(pl, Lx, x, 1, n, nullptr) != 0) {
        loud(who);
        return 0;
    }
    return 1;
}

}  // namespace

extern "C" {

int parsy_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

parsy_plan* parsy_plan_create(int n, int supNo, const int* blockSet, const size_t* lC,
                              const size_t* Li_ptr, const int* lR, const int* aTree,
                              const int* col2Sup, const int* cT, const int* rT, const int* c,
                              const int* r, int device) {
    if (!blockSet || !lC || !Li_ptr || !lR || !aTree || !col2Sup || !cT || !rT || !c || !r || n < 0 ||
        supNo < 0) {
        set_last_error("parsy_plan_create: null or negative argument");
        return nullptr;
    }
    if (device >= 0 && device >= parsy_device_count()) {
        set_last_error("parsy_plan_create: no usable HIP device " + std::to_string(device) +
                       " (this library has no CPU fallback; pass device < 0 for a host-only schedule)");
        return nullptr;
    }
    parsy::PatternRef P;
    P.n = n;
    P.nsuper = supNo;
    P.super = blockSet;
    P.col2sup = col2Sup;
    P.sparent = aTree;
    P.i_ptr = Li_ptr;
    P.s = lR;
    P.A1p = cT;
    P.A1i = rT;
    return parsy::plan_build(P, lC, c, r, device);
}

parsy_plan* parsy_plan_from_symbolic(const parsy_symbolic* sym, int device) {
    const parsy::Symbolic* S = parsy_symbolic_cxx(sym);
    if (!S) {
        set_last_error("parsy_plan_from_symbolic: null symbolic");
        return nullptr;
    }
    return parsy_plan_create(S->n, S->nsuper, S->super.data(), S->p.data(), S->i_ptr.data(), S->s.data(),
                             S->sparent.data(), S->col2sup.data(), S->A1.p.data(), S->A1.i.data(),
                             S->A2.p.data(), S->A2.i.data(), device);
}

void parsy_plan_destroy(parsy_plan* plan) { parsy::plan_free(plan); }

int parsy_plan_get_info(const parsy_plan* pl, parsy_plan_info* o) {
    if (!pl || !o) return -1;
    const parsy::Schedule& S = pl->S;
    std::memset(o, 0, sizeof(*o));
    o->n = S.n;
    o->nsuper = S.nsuper;
    o->nlevels = S.nlevels;
    o->max_width = S.max_width;
    o->max_rows = S.max_rows;
    o->n_small = S.n_small;
    o->n_big = S.n_big;
    o->chol_launches = (int32_t)S.chol.size() + 1;  // + the A scatter
    o->solve_launches = (int32_t)S.solve.size();
    o->nnzA = S.nnzA;
    o->ssize = S.ssize;
    o->xsize = S.xsize;
    o->nnzL = S.nnzL;
    o->n_updates = (int64_t)S.upd.size();
    o->relpos_len = (int64_t)S.relpos.size();
    o->device_bytes = pl->meter.bytes;
    o->flops_stored = S.flops_stored;
    o->update_flops = S.update_flops;
    o->reread_bytes = S.reread_bytes;
    o->inner_flops = S.inner_flops;
    o->tile_update_flops = S.tile_update_flops;
    o->big_flops = S.big_flops;
    o->big_entries = (int64_t)S.big_entries.size();
    o->big_tasks = (int32_t)S.big_tasks.size();
    o->n_pieces = (int32_t)S.csn.size();
    o->chol_levels = S.cnlevels;
    o->piece_width = S.piece_width;
    o->big_min_k = S.big_min_k;
    // as launched (active supernodes only)
    o->chol_subtrees = (int32_t)S.small_ranges.size() / 2;
    for (size_t b = 0; b + 1 < S.small_ranges.size(); b += 2) o->chol_subtree_supernodes += S.small_ranges[b + 1] - S.small_ranges[b];
    o->solve_subtrees = (int32_t)S.solve_small_ranges.size() / 2;
    for (size_t b = 0; b + 1 < S.solve_small_ranges.size(); b += 2)
        o->solve_subtree_supernodes += S.solve_small_ranges[b + 1] - S.solve_small_ranges[b];
    o->backsolve_launches = (int32_t)S.bsolve.size();
    for (const parsy::Launch& l : S.chol)
        if (l.kind == parsy::kLaunchDense) o->dense_tasks += l.count;
    o->dense_flops = S.dense_flops;
    o->dense_entries = S.n_dense_entries;
    o->solve_one = (S.solve_one ? 1 : 0) | (S.solve_one_back ? 2 : 0) | ((S.solve_one || S.solve_one_back) && S.one_subtrees ? 4 : 0);
    o->solve_one_blocks = S.solve_one ? (int32_t)S.one_f.sn.size() : S.solve_one_back ? (int32_t)S.one_back().sn.size() : 0;
    o->sub_mrhs_trees = (int32_t)S.sub_trees.size();
    o->sub_mrhs_slots = S.sub_max_slots;
    o->sub_mrhs_tiers = (int32_t)S.sub_tiers.size();
    o->sub_mrhs_cover_level = S.sub_cover_level;
    o->dense_strip_entries = S.n_strip_entries;
    for (const parsy::Schedule::SplitDesc& sd : S.split_desc)
        if (sd.nparts > 1) {
            o->split_tiles += 1;
            o->split_parts += sd.nparts;
        }
    return 0;
}

long long parsy_plan_chain_check(const parsy_plan* pl, int slots) {
    if (!pl || slots < 1) {
        set_last_error("parsy_plan_chain_check: null plan or slots < 1");
        return -1;
    }
    return (long long)simulate_chain(pl->S, slots);
}

long long parsy_plan_check(const parsy_plan* pl) {
    if (!pl) {
        set_last_error("parsy_plan_check: null plan");
        return -1;
    }
    std::string what;
    const long long bad = (long long)parsy::check_schedule(pl->S, what);
    if (bad) set_last_error("parsy_plan_check: " + what);
    return bad;
}

// The two masks are independent: the supernode mask restricts the solves (and, while no piece mask is set, the
// factorization: a piece follows its supernode); the piece mask restricts the factorization alone.
int parsy_plan_set_active(parsy_plan* pl, const uint8_t* mask) {
    if (!pl) return -1;
    std::vector<uint8_t> pieces;
    if (pl->piece_mask_set) pieces = pl->S.active_piece;
    parsy::build_launches(pl->S, mask, pl->piece_mask_set ? pieces.data() : nullptr);
    pl->sn_mask_set = mask != nullptr;
    return parsy::plan_upload_launches(pl);
}

int parsy_plan_set_active_pieces(parsy_plan* pl, const uint8_t* piece_mask) {
    if (!pl) return -1;
    std::vector<uint8_t> sn_mask;
    if (pl->sn_mask_set) sn_mask = pl->S.active;
    parsy::build_launches(pl->S, pl->sn_mask_set ? sn_mask.data() : nullptr, piece_mask);
    pl->piece_mask_set = piece_mask != nullptr;
    return parsy::plan_upload_launches(pl);
}

int parsy_plan_pieces(const parsy_plan* pl, int32_t* supernode, int32_t* level, int32_t* col0, int32_t* width,
                      int32_t* rows, int64_t* value_begin, int64_t* value_end) {
    if (!pl) return -1;
    const parsy::Schedule& S = pl->S;
    const int nc = (int)S.csn.size();
    for (int p = 0; p < nc; ++p) {
        const parsy::SnDesc& C = S.csn[(size_t)p];
        const parsy::SnDesc& R = S.sn[(size_t)S.csn_real[(size_t)p]];
        if (supernode) supernode[p] = S.csn_real[(size_t)p];
        if (level) level[p] = S.level_of.empty() ? 0 : S.level_of[(size_t)p];
        if (col0) col0[p] = C.c0;
        if (width) width[p] = C.w;
        if (rows) rows[p] = C.r;
        if (value_begin) value_begin[p] = R.px + (int64_t)C.rbias * R.r;
        if (value_end) value_end[p] = R.px + (int64_t)(C.rbias + C.w) * R.r;
    }
    return nc;
}

int parsy_plan_solve_levels(const parsy_plan* pl, int32_t* level) {
    if (!pl) return -1;
    const parsy::Schedule& S = pl->S;
    if (level)
        for (int l = 0; l < S.nlevels; ++l)
            for (int q = S.levelPtr[(size_t)l]; q < S.levelPtr[(size_t)l + 1]; ++q) level[S.levelSet[(size_t)q]] = l;
    return S.nlevels;
}

// Diagnostics (tools/big_stats.py; not part of the public header): the BIG tasks of the plan as rows of
// (task, launch = 2 * source level + push, K, rows in the row window, rows in the column window, identity map,
// first row of the row window - first row of the column window); returns the number of entries (out may be null).
int64_t parsy_debug_big_entries(const parsy_plan* pl, int32_t* out, int64_t cap) {
    if (!pl) return -1;
    const parsy::Schedule& S = pl->S;
    int64_t n = 0, t = 0;
    for (const parsy::Schedule::BigTask& b : S.big_all) {
        for (int64_t e = b.e0; e < b.e1; ++e, ++n) {
            if (!out || n >= cap) continue;
            const parsy::WaveEntry& E = S.big_entries[(size_t)e];
            int32_t* o = out + 7 * n;
            o[0] = (int32_t)t;
            o[1] = b.src_level * 2 + (b.next ? 0 : 1);
            o[2] = E.K;
            o[3] = E.mn & 255;
            o[4] = (E.mn >> 8) & 255;
            o[5] = ((E.mn >> 16) & 1) != 0;
            o[6] = E.ia - E.ja;
        }
        ++t;
    }
    return n;
}

// Diagnostics (tools/pair_stats.py): as parsy_debug_big_entries with the windows themselves -- rows of (task, launch, K,
// rows, columns, first row of the row window, first row of the column window, source (its rank among the panel
// offsets is all a reader needs: low 32 bits of src / 8 ... high bits), 1 = a dense entry of its task).
int64_t parsy_debug_big_windows(const parsy_plan* pl, int64_t* out, int64_t cap) {
    if (!pl) return -1;
    const parsy::Schedule& S = pl->S;
    int64_t n = 0, t = 0;
    for (const parsy::Schedule::BigTask& b : S.big_all) {
        for (int64_t e = b.e0; e < b.e1; ++e, ++n) {
            if (!out || n >= cap) continue;
            const parsy::WaveEntry& E = S.big_entries[(size_t)e];
            int64_t* o = out + 9 * n;
            o[0] = t;
            o[1] = b.src_level * 2 + (b.next ? 0 : 1);
            o[2] = E.K;
            o[3] = E.mn & 255;
            o[4] = (E.mn >> 8) & 255;
            o[5] = E.ia;
            o[6] = E.ja;
            o[7] = E.src;
            o[8] = e < b.em;
        }
        ++t;
    }
    return n;
}

// Diagnostics (tools/recut_stats.py, tests/test_recut_host.py): the BIG tasks of the plan, in the order of the two exports
// above, as rows of (launch = 2 * source level + push, piece, conflict domain (0: tile cut; from kIntervalDomain on: cut in
// intervals of the target's positions), row0, col0, entries, dense
// entries, issued fragment-chunks, 16-wide k chunks, of which in dense entries).  Issued fragment-chunks: per 16-wide k chunk of an entry the 16 x 16
// fragments that are multiplied -- a dense entry its whole 128 x 128 block (64) and 8 per strip that rides with it, a
// ragged entry those its window touches.
int64_t parsy_debug_big_tasks(const parsy_plan* pl, int64_t* out, int64_t cap) {
    if (!pl) return -1;
    const parsy::Schedule& S = pl->S;
    int64_t n = 0;
    for (const parsy::Schedule::BigTask& b : S.big_all) {
        if (out && n < cap) {
            int64_t frag_chunks = 0, chunks = 0, dense_chunks = 0;
            for (int64_t e = b.e0; e < b.e1; ++e) {
                const parsy::WaveEntry& E = S.big_entries[(size_t)e];
                const int64_t kc = (E.K + 15) / 16, mi = E.mn & 255, nj = (E.mn >> 8) & 255;
                chunks += kc;
                if (e < b.em) dense_chunks += kc;
                frag_chunks += kc * (e < b.em ? 64 + 8 * (parsy::big_strip_rows(E) > 0) + 8 * (parsy::big_strip_cols(E) > 0)
                                              : ((mi + 15) / 16) * ((nj + 15) / 16));
            }
            int64_t* o = out + 10 * n;
            o[0] = b.src_level * 2 + (b.next ? 0 : 1);
            o[1] = b.sn;
            o[2] = b.domain;
            o[3] = b.row0;
            o[4] = b.col0;
            o[5] = b.e1 - b.e0;
            o[6] = b.em - b.e0;
            o[7] = frag_chunks;
            o[8] = chunks;
            o[9] = dense_chunks;
        }
        ++n;
    }
    return n;
}

// Diagnostics: the tasks of the DENSE launches in launch order as rows of (launch index, 8-wide k chunks).
int64_t parsy_debug_dense_tasks(const parsy_plan* pl, int32_t* out, int64_t cap) {
    if (!pl) return -1;
    const parsy::Schedule& S = pl->S;
    int64_t n = 0;
    int li = 0;
    for (const parsy::Launch& l : S.chol) {
        if (l.kind != parsy::kLaunchDense) continue;
        for (int q = l.first; q < l.first + l.count; ++q, ++n)
            if (out && n < cap) {
                out[2 * n] = li;
                out[2 * n + 1] = S.big_tasks[(size_t)q].part;
            }
        ++li;
    }
    return n;
}

// Diagnostics: the launch table of the plan -- which = 0: factorization, 1: forward solve, 2: backward solve -- as one row
// per launch record of parsy::kLaunchFields columns, the fields of parsy::Launch in declaration order (kind, first, count,
// level, side, wait_level, form, rows_only, ticket, lds_bytes, stage, width, width_class, task_first, task_count);
// returns the number of records (out may be null).
int64_t parsy_debug_launches(const parsy_plan* pl, int which, int32_t* out, int64_t cap) {
    if (!pl || which < 0 || which > 2) return -1;
    const parsy::Schedule& S = pl->S;
    const std::vector<parsy::Launch>& seq = which == 0 ? S.chol : which == 1 ? S.solve : S.bsolve;
    for (size_t i = 0; out && i < seq.size() && (int64_t)i < cap; ++i) {
        const parsy::Launch& l = seq[i];
        const int32_t row[parsy::kLaunchFields] = {l.kind, l.first, l.count, l.level, l.side, l.wait_level, l.form, l.rows_only,
                                                   l.ticket, l.lds_bytes, l.stage, l.width, l.width_class, l.task_first, l.task_count};
        std::copy(row, row + parsy::kLaunchFields, out + (size_t)parsy::kLaunchFields * i);
    }
    return (int64_t)seq.size();
}

// Diagnostics: the route of a solve (solve_route.hpp) with the gates the environment sets at this call, as the witness
// indices (parsy_debug_kernel_name) of the launches it enqueues, in order; plans without a device too (device < 0: every
// subtree tier counts as usable).  Returns the number of launches and fills at most cap entries (kernels may be null);
// -1: nrhs < 1 or ldx < n.
int64_t parsy_debug_solve_route(const parsy_plan* pl, int nrhs, int ldx, int backward, int32_t* kernels, int64_t cap) {
    if (!pl || nrhs < 1 || ldx < pl->S.n) return -1;
    parsy::SolveRoute R;
    parsy::solve_route(pl->S, parsy::read_solve_gates(), parsy::plan_route_runtime(pl), nrhs, ldx, backward != 0, R);
    return parsy::route_kernels(R, kernels, cap);
}

// ... and of one step of a solve in steps of levels (parsy_solve_levels_device: level_begin, level_end, flags)
int64_t parsy_debug_solve_route_levels(const parsy_plan* pl, int nrhs, int ldx, int level_begin, int level_end, int flags,
                                       int32_t* kernels, int64_t cap) {
    if (!pl || nrhs < 1 || ldx < pl->S.n || level_begin > level_end) return -1;
    parsy::SolveRoute R;
    parsy::solve_route_levels(pl->S, parsy::read_solve_gates(), parsy::plan_route_runtime(pl), nrhs, ldx, (flags & 4) != 0,
                              level_begin, level_end, (flags & 1) != 0, (flags & 2) != 0, R);
    return parsy::route_kernels(R, kernels, cap);
}

// Diagnostics (tools/schedule_digests.py): the digest of the plan's whole schedule (schedule_digest.hpp) -- one 64-bit hash
// per data member of parsy::Schedule, in declaration order.  Returns the number of fields; out / name (either may be
// null) receive the hash and the member's name of field `field`, where that is one.
int parsy_debug_schedule_digest(const parsy_plan* pl, int field, uint64_t* out, const char** name) {
    if (!pl) return -1;
    const parsy::ScheduleDigest d = parsy::schedule_digest(pl->S, field < 0 ? (1 << 30) : field);   // (no field: the count only)
    if (field >= 0 && field < (int)d.size()) {
        if (out) *out = d[(size_t)field].second;
        if (name) *name = d[(size_t)field].first;
    }
    return (int)d.size();
}

// Diagnostics: the launches of the last collected profiled run as rows of (kind, level << 1 | side, work items, ms).
int64_t parsy_debug_launch_times(const parsy_plan* pl, double* out, int64_t cap) {
    if (!pl) return -1;
    const int64_t n = (int64_t)std::min(pl->pev_ms.size(), pl->pev_kind.size());
    for (int64_t i = 0; out && i < n && i < cap; ++i) {
        out[4 * i] = pl->pev_kind[(size_t)i];
        out[4 * i + 1] = (size_t)i < pl->pev_level.size() ? pl->pev_level[(size_t)i] : -1;
        out[4 * i + 2] = (size_t)i < pl->pev_count.size() ? pl->pev_count[(size_t)i] : 0;
        out[4 * i + 3] = pl->pev_ms[(size_t)i];
    }
    return n;
}

int parsy_factor_begin(parsy_plan* pl, const double* d_values, double* d_lValues, void* stream, int flags) {
    if (!pl || !d_values || !d_lValues) {
        set_last_error("parsy_factor_begin: null argument");
        return -1;
    }
    return parsy::plan_factor_begin(pl, d_values, d_lValues, (hipStream_t)stream, (flags & PARSY_FACTOR_NO_INIT) == 0);
}

int parsy_factor_level(parsy_plan* pl, int level, double* d_lValues, void* stream) {
    if (!pl || !d_lValues) {
        set_last_error("parsy_factor_level: null argument");
        return -1;
    }
    return parsy::plan_factor_levels(pl, level, level + 1, d_lValues, (hipStream_t)stream);
}

int parsy_factor_end(parsy_plan* pl, void* stream) {
    if (!pl) {
        set_last_error("parsy_factor_end: null plan");
        return -1;
    }
    return parsy::plan_factor_end(pl, (hipStream_t)stream);
}

int parsy_factor_device(parsy_plan* pl, const double* d_values, double* d_lValues, void* stream) {
    if (!pl || !d_values || !d_lValues) {
        set_last_error("parsy_factor_device: null argument");
        return -1;
    }
    return parsy::plan_factor(pl, d_values, d_lValues, (hipStream_t)stream);
}

int parsy_factor_device_ex(parsy_plan* pl, const double* d_values, double* d_lValues, void* stream,
                           int flags) {
    if (!pl || !d_values || !d_lValues) {
        set_last_error("parsy_factor_device_ex: null argument");
        return -1;
    }
    return parsy::plan_factor(pl, d_values, d_lValues, (hipStream_t)stream,
                              (flags & PARSY_FACTOR_NO_INIT) == 0);
}

int parsy_factor_status(parsy_plan* pl) {
    if (!pl || pl->device < 0) return -1;
    int v = 0;
    if (hipMemcpy(&v, pl->dp.info, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v >= 0x7f7f7f7f ? 0 : v;  // < 0: an in-launch wait timed out (internal error)
}

int parsy_solve_status(parsy_plan* pl) {
    if (!pl || pl->device < 0) return -1;
    int v = 0;
    const int* word = pl->solve_status_word ? pl->solve_status_word : pl->dp.sinfo;
    if (hipMemcpy(&v, word, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (v < 0) set_last_error("solve: a hand-off wait inside a chain launch timed out; x is not the solution");
    return v < 0 ? -1 : 0;
}

int parsy_solve_device(parsy_plan* pl, const double* d_lValues, double* d_x, int nrhs, int ldx,
                       void* stream) {
    if (!pl || !d_lValues || !d_x) {
        set_last_error("parsy_solve_device: null argument");
        return -1;
    }
    return parsy::plan_solve(pl, d_lValues, d_x, nrhs, ldx, (hipStream_t)stream);
}

double parsy_last_factor_ms(parsy_plan* pl) {
    float ms = -1;
    if (!pl || !pl->have_f) return -1;
    if (hipEventSynchronize(pl->ev_f1) != hipSuccess) return -1;
    if (hipEventElapsedTime(&ms, pl->ev_f0, pl->ev_f1) != hipSuccess) return -1;
    return ms;
}

double parsy_last_solve_ms(parsy_plan* pl) {
    float ms = -1;
    if (!pl || !pl->have_s) return -1;
    if (hipEventSynchronize(pl->ev_s1) != hipSuccess) return -1;
    if (hipEventElapsedTime(&ms, pl->ev_s0, pl->ev_s1) != hipSuccess) return -1;
    return ms;
}

int parsy_plan_profile(parsy_plan* pl, int enable) {
    if (!pl) return -1;
    pl->profile = enable != 0;
    if (enable == 2) {  // reset the accumulators
        for (int k = 0; k < PARSY_PROFILE_KINDS; ++k) pl->kind_ms[k] = 0, pl->kind_launches[k] = 0;
        pl->profiled_runs = 0;
        pl->level_ms.clear();
    }
    return 0;
}

int parsy_plan_profile_collect(parsy_plan* pl) { return pl ? parsy::plan_collect_profile(pl) : -1; }

int parsy_plan_profile_get(parsy_plan* pl, double* kind_ms, int* kind_launches, int* runs) {
    if (!pl) return -1;
    for (int k = 0; k < PARSY_PROFILE_KINDS; ++k) {
        if (kind_ms) kind_ms[k] = pl->kind_ms[k];
        if (kind_launches) kind_launches[k] = pl->kind_launches[k];
    }
    if (runs) *runs = pl->profiled_runs;
    return 0;
}

int parsy_plan_profile_levels(parsy_plan* pl, double* main_ms, double* side_ms) {
    if (!pl) return -1;
    const int nl = pl->S.cnlevels;
    for (int l = 0; l < nl; ++l) {
        const size_t a = (size_t)l << 1, b = a | 1;
        if (main_ms) main_ms[l] = a < pl->level_ms.size() ? pl->level_ms[a] : 0.0;
        if (side_ms) side_ms[l] = b < pl->level_ms.size() ? pl->level_ms[b] : 0.0;
    }
    return nl;
}

int parsy_backsolve_device(parsy_plan* pl, const double* d_lValues, double* d_x, int nrhs, int ldx,
                           void* stream) {
    if (!pl || !d_lValues || !d_x) {
        set_last_error("parsy_backsolve_device: null argument");
        return -1;
    }
    return parsy::plan_backsolve(pl, d_lValues, d_x, nrhs, ldx, (hipStream_t)stream);
}

int parsy_solve_levels_device(parsy_plan* pl, const double* d_lValues, double* d_x, int nrhs, int ldx, void* stream,
                              int level_begin, int level_end, int flags) {
    if (!pl || !d_lValues || !d_x) {
        set_last_error("parsy_solve_levels_device: null argument");
        return -1;
    }
    return parsy::plan_solve_levels(pl, d_lValues, d_x, nrhs, ldx, (hipStream_t)stream, level_begin, level_end, flags);
}

int parsy_copy_segments_device(double* d_dst, const double* d_src, const int64_t* d_dst_off,
                               const int64_t* d_src_off, const int32_t* d_len, int64_t nseg, void* stream) {
    if (nseg < 0 || (nseg > 0 && (!d_dst || !d_src || !d_dst_off || !d_src_off || !d_len))) {
        set_last_error("parsy_copy_segments_device: null argument");
        return -1;
    }
    parsy::launch_copy_segments(d_dst, d_src, d_dst_off, d_src_off, d_len, nseg, (hipStream_t)stream);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int parsy_rhs_ones_device(parsy_plan* pl, const double* d_lValues, double* d_b, void* stream) {
    if (!pl || !d_lValues || !d_b || pl->device < 0) {
        set_last_error("parsy_rhs_ones_device: null argument or plan without a device");
        return -1;
    }
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(hipMemsetAsync(d_b, 0, (size_t)pl->S.n * sizeof(double), (hipStream_t)stream));
    parsy::launch_rhs_ones(pl->dp, pl->S.nsuper, pl->S.max_rows, d_lValues, d_b, (hipStream_t)stream);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int parsy_plan_set_perm(parsy_plan* pl, const int* perm) {
    if (!pl) {
        set_last_error("parsy_plan_set_perm: null plan");
        return -1;
    }
    return parsy::plan_set_perm(pl, perm);
}

int parsy_residual_device(parsy_plan* pl, const double* d_values, const double* d_x, int ldx, const double* d_b, int ldb,
                          double* d_r, int ldr, int nrhs, double* berr, void* stream) {
    if (!pl || !d_values || !d_x || !d_b) {
        set_last_error("parsy_residual_device: null argument");
        return -1;
    }
    return parsy::plan_residual(pl, d_values, d_x, ldx, d_b, ldb, d_r, ldr, nrhs, berr, (hipStream_t)stream);
}

int parsy_solve_spd_device(parsy_plan* pl, const double* d_values, const double* d_lValues, const double* d_b, int ldb,
                           double* d_x, int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, void* stream) {
    return parsy_solve_spd_bounds_device(pl, d_values, d_lValues, d_b, ldb, d_x, ldx, nrhs, max_steps, steps, berr, nullptr,
                                         stream);
}

int parsy_solve_spd_bounds_device(parsy_plan* pl, const double* d_values, const double* d_lValues, const double* d_b, int ldb,
                                  double* d_x, int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, double* ferr,
                                  void* stream) {
    if (!pl || !d_values || !d_lValues || !d_b || !d_x) {
        set_last_error(std::string(ferr ? "parsy_solve_spd_bounds_device" : "parsy_solve_spd_device") + ": null argument");
        return -1;
    }
    return parsy::plan_solve_refined(pl, d_values, d_lValues, d_b, ldb, d_x, ldx, nrhs, max_steps, steps, berr, ferr,
                                     (hipStream_t)stream);
}

int parsy_error_bounds_device(parsy_plan* pl, const double* d_values, const double* d_lValues, const double* d_x, int ldx,
                              const double* d_b, int ldb, int nrhs, double* ferr, double* berr, void* stream) {
    if (!pl || !d_values || !d_lValues || !d_x || !d_b || (!ferr && !berr)) {
        set_last_error("parsy_error_bounds_device: null argument (ferr and berr may not both be NULL)");
        return -1;
    }
    return parsy::plan_error_bounds(pl, d_values, d_lValues, d_x, ldx, d_b, ldb, nrhs, ferr, berr, (hipStream_t)stream);
}

int parsy_rcond_device(parsy_plan* pl, const double* d_values, const double* d_lValues, double* anorm, double* rcond,
                       void* stream) {
    if (!pl || !d_values || !d_lValues || (!anorm && !rcond)) {
        set_last_error("parsy_rcond_device: null argument (anorm and rcond may not both be NULL)");
        return -1;
    }
    return parsy::plan_rcond(pl, d_values, d_lValues, anorm, rcond, (hipStream_t)stream);
}

int parsy_eigs_device(parsy_plan* pl, const double* d_values, const double* d_mvalues, const double* d_lValues, int k,
                      const double* d_x0, int ldx0, int block, double tol, int max_basis, int max_iter, double* lambda,
                      double* d_y, int ldy, double* resid, int32_t* nconv, void* stream) {
    if (!pl || !d_values || !d_lValues || !d_x0 || !lambda || !d_y || !resid || !nconv) {
        set_last_error("parsy_eigs_device: null argument (only d_mvalues may be NULL)");
        return -1;
    }
    return parsy::plan_eigs(pl, d_values, d_mvalues, d_lValues, k, d_x0, ldx0, block, tol, max_basis, max_iter, lambda, d_y,
                            ldy, resid, nconv, (hipStream_t)stream);
}

int parsy_factor_apply_device(parsy_plan* pl, const double* d_lValues, int op, const double* d_x, int ldx, int nrhs,
                              double alpha, double beta, double* d_y, int ldy, void* stream) {
    return parsy::plan_factor_apply(pl, d_lValues, op, d_x, ldx, nrhs, alpha, beta, d_y, ldy, stream);
}

int parsy_factor_apply_get_info(parsy_plan* pl, parsy_apply_info* info) {
    if (!pl || !info) {
        set_last_error("parsy_factor_apply_get_info: null argument");
        return -1;
    }
    if (parsy::apply_ensure_host(pl) != 0) return -1;
    const parsy::ApplyState& A = *pl->apply;
    info->rows = pl->S.n;
    info->occurrences = (int64_t)pl->S.rows.size();
    info->max_occurrences = A.I.max_occurrences;
    info->block_columns = parsy::kApplyBlock;
    info->workspace_bytes = A.ws_need * 8;
    info->device_bytes = A.meter.bytes;
    info->last_op = A.last_op;
    info->last_launches = A.last_launches;
    return 0;
}

int parsy_factor_updown_device(parsy_plan* pl, double* d_lValues, int sign, int k, const int* wp, const int* wi,
                               const double* d_wx, void* stream) {
    return parsy::plan_factor_updown(pl, d_lValues, sign, k, wp, wi, d_wx, stream);
}

int parsy_updown_status(parsy_plan* pl) { return parsy::plan_updown_status(pl); }

int parsy_updown_path(const parsy_plan* pl, int k, const int* wp, const int* wi, int* supernodes, int* first_col) {
    const char* who = "parsy_updown_path";
    if (!pl) {
        set_last_error(std::string(who) + ": null argument");
        return -1;
    }
    parsy::UpdownW W;
    if (parsy::updown_prepare(pl->S, pl->perm, who, k, wp, wi, W) != 0) return -1;
    std::vector<parsy::UpdownNode> path;
    parsy::updown_path(pl->S, W, 0, k, path);
    for (size_t i = 0; i < path.size(); ++i) {
        if (supernodes) supernodes[i] = path[i].sn;
        if (first_col) first_col[i] = path[i].first_col;
    }
    return (int)path.size();
}

int parsy_updown_get_info(parsy_plan* pl, parsy_updown_info* info) {
    if (!pl || !info) {
        set_last_error("parsy_updown_get_info: null argument");
        return -1;
    }
    if (parsy::updown_ensure_host(pl) != 0) return -1;
    const parsy::UpdownState& U = *pl->updown;
    info->path_supernodes = U.path_supernodes;
    info->last_launches = U.last_launches;
    info->last_k = U.last_k;
    info->last_sign = U.last_sign;
    info->block_columns = U.block_columns;
    info->entries_touched = U.entries_touched;
    info->device_bytes = U.meter.bytes;
    return 0;
}

int parsy_factor_rowdel_device(parsy_plan* pl, double* d_lValues, int row, void* stream) {
    return parsy::plan_factor_rowdel(pl, d_lValues, row, stream);
}

int parsy_factor_rowadd_device(parsy_plan* pl, double* d_lValues, int row, int nz, const int* ci, const double* d_cx,
                               void* stream) {
    return parsy::plan_factor_rowadd(pl, d_lValues, row, nz, ci, d_cx, stream);
}

int parsy_rowmod_status(parsy_plan* pl) { return parsy::plan_updown_status(pl); }

int parsy_rowmod_reach(parsy_plan* pl, int row, int* supernodes, int* position, int* height) {
    const char* who = "parsy_rowmod_reach";
    if (!pl) {
        set_last_error(std::string(who) + ": null argument");
        return -1;
    }
    const int p = parsy::rowmod_position(pl->S, parsy::plan_perm_inverse(pl), who, row);
    if (p < 0 || parsy::rowmod_ensure_host(pl) != 0) return -1;
    std::vector<parsy::RowmodNode> reach;
    parsy::rowmod_reach(pl->S, pl->rowmod->I, p, reach);
    for (size_t i = 0; i < reach.size(); ++i) {
        if (supernodes) supernodes[i] = reach[i].sn;
        if (position) position[i] = reach[i].pos;
        if (height) height[i] = reach[i].height;
    }
    return (int)reach.size();
}

int parsy_rowmod_get_info(parsy_plan* pl, parsy_rowmod_info* info) {
    if (!pl || !info) {
        set_last_error("parsy_rowmod_get_info: null argument");
        return -1;
    }
    if (!pl->rowmod) pl->rowmod = std::make_unique<parsy::RowmodState>(&pl->meter);   // (the index only once it is asked for)
    const parsy::RowmodState& R = *pl->rowmod;
    info->last_op = R.last_op;
    info->last_row = R.last_row;
    info->reach_supernodes = R.reach;
    info->heights = R.heights;
    info->row_launches = R.row_launches;
    info->column_launches = R.column_launches;
    info->rotation_launches = R.rotation_launches;
    info->reserved = 0;
    info->entries_read = R.entries_read;
    info->entries_walked = R.entries_walked;
    info->device_bytes = R.meter.bytes;
    return 0;
}

parsy_normal* parsy_normal_create(parsy_plan* pl, int m, const int* Fp, const int* Fi) {
    const char* who = "parsy_normal_create";
    if (!pl || !Fp) {
        set_last_error(std::string(who) + ": null argument");
        return nullptr;
    }
    if (pl->solve_only) {
        set_last_error(std::string(who) + ": plan was built from L's pattern only (no A pattern)");
        return nullptr;
    }
    parsy::NormalIndex I;
    if (parsy::normal_build(pl->S, pl->perm, m, Fp, Fi, I) != 0) return nullptr;
    parsy_normal* h = new parsy_normal();
    h->plan = pl;
    h->device = pl->device;
    h->I = std::move(I);
    return h;
}

void parsy_normal_destroy(parsy_normal* h) {
    if (!h) return;
    if (h->dev.on_device || h->dev.ws.data()) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();   // (a call may still read the index)
    }
    delete h;
}

int parsy_normal_get_info(const parsy_normal* h, parsy_normal_info* info) {
    if (!h || !info) {
        set_last_error("parsy_normal_get_info: null argument");
        return -1;
    }
    const parsy::NormalIndex& I = h->I;
    info->n = I.n, info->m = I.m, info->nnzF = I.nnzF();
    info->longest_list = I.longest_list;
    info->chunked_entries = (int32_t)I.fold_q.size();
    info->chunks = (int32_t)I.chunks();
    info->launches = I.chunks() > 0 ? 2 : 0;
    for (int c = 0; c < parsy::kNormalClasses; ++c) {
        info->border[c] = parsy::kNormalBorder[c];
        info->class_entries[c] = (int64_t)I.cls[c].size();
        info->launches += !I.cls[c].empty();
    }
    info->pairs = I.pairs;
    info->entries_untouched = I.entries_untouched;
    info->device_bytes = h->dev.meter.bytes;
    return 0;
}

int64_t parsy_normal_pairs(const parsy_normal* h, int64_t q, int32_t* a, int32_t* b, int32_t* k) {
    if (!h || q < 0 || q >= h->I.nnzA) {
        set_last_error("parsy_normal_pairs: null handle or q outside 0 .. nnzA - 1");
        return -1;
    }
    const parsy::NormalIndex& I = h->I;
    const int64_t t0 = I.lptr[(size_t)q], len = I.lptr[(size_t)q + 1] - t0;
    for (int64_t t = 0; t < len; ++t) {
        if (a) a[t] = I.ta[(size_t)(t0 + t)];
        if (b) b[t] = I.tb[(size_t)(t0 + t)];
        if (k) k[t] = I.tk[(size_t)(t0 + t)];
    }
    return len;
}

long long parsy_normal_check(const parsy_normal* h) {
    if (!h) {
        set_last_error("parsy_normal_check: null handle");
        return -1;
    }
    return parsy::normal_check(h->I);
}

int parsy_normal_values_device(parsy_normal* h, const double* d_fx, const double* d_w, double beta, const double* d_base,
                               double* d_values, void* stream) {
    return parsy::normal_values(h, d_fx, d_w, beta, d_base, d_values, stream);
}

int parsy_normal_apply_device(parsy_normal* h, int op, const double* d_fx, const double* d_w, const double* d_x, int ldx,
                              int nrhs, double alpha, double beta, double* d_y, int ldy, void* stream) {
    return parsy::normal_apply(h, op, d_fx, d_w, d_x, ldx, nrhs, alpha, beta, d_y, ldy, stream);
}

int parsy_lsq_solve_device(parsy_normal* h, const double* d_fx, const double* d_w, double beta, const double* d_lValues,
                           const double* d_c, int ldc, double* d_x, int ldx, int nrhs, int steps, double* d_r, int ldr,
                           double* d_g, int ldg, void* stream) {
    return parsy::normal_lsq(h, d_fx, d_w, beta, d_lValues, d_c, ldc, d_x, ldx, nrhs, steps, d_r, ldr, d_g, ldg, stream);
}

parsy_reach* parsy_reach_create(parsy_plan* pl, int nrhs, const int* bp, const int* bi, int nx, const int* xi) {
    const char* who = "parsy_reach_create";
    if (!pl || !bp) {
        set_last_error(std::string(who) + ": null argument");
        return nullptr;
    }
    if (pl->sn_mask_set || pl->piece_mask_set) {
        set_last_error(std::string(who) + ": plan is restricted by parsy_plan_set_active / _set_active_pieces");
        return nullptr;
    }
    parsy::ReachIndex I;
    if (parsy::reach_build(pl->S, parsy::plan_perm_inverse(pl), who, nrhs, bp, bi, nx, xi, I) != 0) return nullptr;
    parsy_reach* h = new parsy_reach();
    h->plan = pl;
    h->device = pl->device;
    h->I = std::move(I);
    return h;
}

void parsy_reach_destroy(parsy_reach* h) {
    if (!h) return;
    if (h->dev.on_device) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();   // (a call may still read the index)
    }
    delete h;
}

int parsy_reach_get_info(const parsy_reach* h, parsy_reach_info* info) {
    if (!h || !info) {
        set_last_error("parsy_reach_get_info: null argument");
        return -1;
    }
    const parsy::ReachIndex& I = h->I;
    info->nrhs = I.nrhs, info->nx = I.nx;
    info->fwd_supernodes = (int32_t)I.fwd.sn.size(), info->fwd_pieces = (int32_t)I.fwd.pieces.size();
    info->bwd_supernodes = (int32_t)I.bwd.sn.size(), info->bwd_pieces = (int32_t)I.bwd.pieces.size();
    info->fwd_steps = I.fwd.steps(), info->bwd_steps = I.bwd.steps();
    info->last_op = h->dev.last_op, info->last_kernels = h->dev.last_kernels;
    info->fwd_entries = I.fwd.entries, info->bwd_entries = I.bwd.entries, info->xsize = I.xsize;
    info->device_bytes = h->dev.meter.bytes;
    return 0;
}

int parsy_reach_get(const parsy_reach* h, int32_t* fwd, int32_t* bwd) {
    if (!h) {
        set_last_error("parsy_reach_get: null handle");
        return -1;
    }
    if (fwd) std::copy(h->I.fwd.sn.begin(), h->I.fwd.sn.end(), fwd);
    if (bwd) std::copy(h->I.bwd.sn.begin(), h->I.bwd.sn.end(), bwd);
    return 0;
}

long long parsy_reach_check(const parsy_reach* h) {
    if (!h) {
        set_last_error("parsy_reach_check: null handle");
        return -1;
    }
    return parsy::reach_check(h->plan->S, h->I);
}

int parsy_solve_sparse_device(parsy_reach* h, const double* d_lValues, const double* d_bx, int op, double* d_x, int ldx,
                              void* stream) {
    return parsy::reach_solve(h, d_lValues, d_bx, op, d_x, ldx, stream);
}

void parsy_dropin_reset(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_plans) parsy::plan_free(kv.second);
    g_plans.clear();
}

// ---- drop-in operators ----------------------------------------------------------

bool cholesky_left_par_05(int n, int* c, int* r, double* values, size_t* lC, int* lR, size_t* Li_ptr,
                          double* lValues, int* blockSet, int supNo, double* timing, int* aTree,
                          int* cT, int* rT, int* col2Sup, int nLevels, int* levelPtr, int* levelSet,
                          int nPar, int* parPtr, int* partition, int chunk, int threads,
                          int super_max, int col_max, double* nodCost) {
    (void)levelSet; (void)nPar; (void)chunk; (void)threads; (void)super_max; (void)col_max; (void)nodCost;
    const char* who = "cholesky_left_par_05";
    const double t0 = now_s();
    if (!validate_partition(supNo, nLevels, levelPtr, parPtr, partition, who)) {
        loud(who);
        return false;
    }
    parsy_plan* pl = cached_chol_plan(n, supNo, blockSet, lC, Li_ptr, lR, aTree, col2Sup, cT, rT, c, r);
    int st = 0;
    return dropin_factor(who, pl, values, lValues, timing, t0, &st) && st == 0;
}

bool cholesky_left_par_05_prune(int n, int* c, int* r, double* values, size_t* lC, int* lR, size_t* Li_ptr,
                                double* lValues, int* blockSet, int supNo, double* timing, int* prunePtr,
                                int* pruneSet, int nLevels, int* levelPtr, int* levelSet, int nPar, int* parPtr,
                                int* partition, int chunk, int threads, int super_max, int col_max,
                                double* nodCost) {
    (void)levelSet; (void)nPar; (void)chunk; (void)threads; (void)super_max; (void)col_max; (void)nodCost;
    const char* who = "cholesky_left_par_05_prune";
    const double t0 = now_s();
    if (!c || !r || !values || !lC || !lR || !Li_ptr || !lValues || !blockSet || !prunePtr || !pruneSet || n < 0 ||
        supNo < 0) {
        set_last_error(std::string(who) + ": null or negative argument");
        loud(who);
        return false;
    }
    if (!validate_partition(supNo, nLevels, levelPtr, parPtr, partition, who)) {
        loud(who);
        return false;
    }
    parsy_plan* pl = cached_chol_plan_prune(n, supNo, blockSet, lC, Li_ptr, lR, prunePtr, pruneSet, c, r);
    int st = 0;
    return dropin_factor(who, pl, values, lValues, timing, t0, &st) && st == 0;
}

bool cholesky_left_par_waveFront(int n, int* c, int* r, double* values, size_t* lC, int* lR,
                                 size_t* Li_ptr, double* lValues, int* blockSet, int supNo,
                                 double* timing, int* aTree, int* cT, int* rT, int* col2Sup,
                                 int nLevels, int* levelPtr, int* levelSet, int chunk, int threads,
                                 int super_max, int col_max) {
    (void)chunk; (void)threads; (void)super_max; (void)col_max;
    const char* who = "cholesky_left_par_waveFront";
    const double t0 = now_s();
    if (!validate_levelset(supNo, nLevels, levelPtr, levelSet, who)) {
        loud(who);
        return false;
    }
    parsy_plan* pl = cached_chol_plan(n, supNo, blockSet, lC, Li_ptr, lR, aTree, col2Sup, cT, rT, c, r);
    int st = 0;
    if (!dropin_factor(who, pl, values, lValues, timing, t0, &st)) return false;
    if (st != 0)
        std::fprintf(stderr, "[parsy_amd] %s: non-positive pivot at column %d (the reference ignores LAPACK's info here)\n",
                     who, st);
    return true;
}

int blockedLsolve(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr, int* col2sup,
                  int* sup2col, int supNo, double* x) {
    (void)NNZ; (void)col2sup;
    return dropin_solve("blockedLsolve", n, Lp, Li, Lx, Li_ptr, sup2col, supNo, x);
}

int blockedPrunedLSolve(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr, int* BPSet, int PBSetSize,
                        int* sup2col, int supNo, double* x) {
    (void)NNZ;
    const char* who = "blockedPrunedLSolve";
    if (!Lp || !Li || !x) return 0;  // reference: Triangular_BCSC.h:66
    auto fail = [&](const std::string& what) {
        if (!what.empty()) set_last_error(std::string(who) + ": " + what);
        loud(who);
        return 0;
    };
    if (!Lx || !Li_ptr || !sup2col || PBSetSize < 0 || (PBSetSize > 0 && !BPSet)) return fail("null or negative argument");
    // the list, 0-based and ascending
    std::vector<int> list;
    for (int k = 0; k < PBSetSize; ++k) {
        if (BPSet[k] < 1 || BPSet[k] > supNo)
            return fail("supernode " + std::to_string(BPSet[k]) + " of the list is outside 1 .. supNo");
        list.push_back(BPSet[k] - 1);
    }
    std::sort(list.begin(), list.end());
    if (std::adjacent_find(list.begin(), list.end()) != list.end()) return fail("a supernode is listed twice");
    if (list.empty()) return 1;
    // closed towards the root: the parent of a supernode is the supernode of its first row below the diagonal block
    // (tree_from_pattern), read here for the listed ones alone
    for (int s : list) {
        const size_t w = (size_t)(sup2col[s + 1] - sup2col[s]), b0 = Li_ptr[sup2col[s]], b1 = Li_ptr[sup2col[s + 1]];
        if (b1 - b0 <= w) continue;
        const int par = (int)(std::upper_bound(sup2col, sup2col + supNo + 1, Li[b0 + w]) - sup2col) - 1;
        if (!std::binary_search(list.begin(), list.end(), par))
            return fail("the list is not closed towards the root: supernode " + std::to_string(s + 1) + " is listed, its parent " +
                        std::to_string(par + 1) + " is not");
    }
    parsy_plan* pl = cached_solve_plan(n, supNo, Lp, Li, Li_ptr, sup2col);
    if (!pl) return fail("");
    std::unique_lock<std::mutex> use(pl->use_mu);
    // B and the selected rows: every column of the listed supernodes
    std::vector<int> rows;
    for (int s : list)
        for (int j = sup2col[s]; j < sup2col[s + 1]; ++j) rows.push_back(j);
    const int nr = (int)rows.size();
    const int bp[2] = {0, nr};
    std::vector<double> b((size_t)nr), out((size_t)nr);
    for (int k = 0; k < nr; ++k) b[(size_t)k] = x[rows[(size_t)k]];
    parsy_reach* h = parsy_reach_create(pl, 1, bp, rows.data(), nr, rows.data());
    if (!h) return fail("");
    const int rc = parsy_solve_sparse_host(h, Lx, b.data(), PARSY_SPARSE_GINV, out.data(), nr, nullptr);
    parsy_reach_destroy(h);
    if (rc != 0) return fail("");
    for (int k = 0; k < nr; ++k) x[rows[(size_t)k]] = out[(size_t)k];
    return 1;
}

int leveledBlockedLsolve(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr,
                         int* col2sup, int* sup2col, int supNo, double* x, int levels,
                         int* levelPtr, int* levelSet, int chunk) {
    (void)NNZ; (void)col2sup; (void)chunk;
    if (!Lp || !Li || !x) return 0;
    if (!validate_levelset(supNo, levels, levelPtr, levelSet, "leveledBlockedLsolve")) {
        loud("leveledBlockedLsolve");
        return 0;
    }
    return dropin_solve("leveledBlockedLsolve", n, Lp, Li, Lx, Li_ptr, sup2col, supNo, x);
}

int H2LeveledBlockedLsolve(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr,
                           int* col2sup, int* sup2col, int supNo, double* x, int levels,
                           int* levelPtr, int* levelSet, int parts, int* parPtr, int* partition,
                           int chunk) {
    (void)NNZ; (void)col2sup; (void)chunk; (void)levelSet; (void)parts;
    if (!Lp || !Li || !x) return 0;
    if (!validate_partition(supNo, levels, levelPtr, parPtr, partition, "H2LeveledBlockedLsolve")) {
        loud("H2LeveledBlockedLsolve");
        return 0;
    }
    return dropin_solve("H2LeveledBlockedLsolve", n, Lp, Li, Lx, Li_ptr, sup2col, supNo, x);
}

int H2LeveledBlockedLsolve_Peeled(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr,
                                  int* col2sup, int* sup2col, int supNo, double* x, int levels,
                                  int* levelPtr, int* levelSet, int parts, int* parPtr,
                                  int* partition, int chunk, int threads) {
    (void)NNZ; (void)col2sup; (void)chunk; (void)levelSet; (void)parts; (void)threads;
    if (!Lp || !Li || !x) return 0;
    if (!validate_partition(supNo, levels, levelPtr, parPtr, partition, "H2LeveledBlockedLsolve_Peeled")) {
        loud("H2LeveledBlockedLsolve_Peeled");
        return 0;
    }
    return dropin_solve("H2LeveledBlockedLsolve_Peeled", n, Lp, Li, Lx, Li_ptr, sup2col, supNo, x);
}

}  // extern "C"
