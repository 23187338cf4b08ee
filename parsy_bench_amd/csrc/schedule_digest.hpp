// Digest of a whole Schedule: one 64-bit FNV-1a per data member, in declaration order.  What a change of the schedule
// builder that is meant to leave every schedule as it was is compared by (tools/schedule_digests.py,
// tests/schedule_digest_check.cpp): the launch tables alone can stay equal while a wave entry, a split range or a slot
// number moves.  Plain C++, host code only.
//   - integers and bools are hashed by value, doubles by bit pattern (so the flop accumulators pin the order of their sums);
//   - a vector is hashed with its length, its elements as raw bytes only where the element type has no padding
//     (std::has_unique_object_representations) -- padding bytes are indeterminate -- and member by member otherwise.
#pragma once
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "schedule.hpp"

namespace parsy {

struct Fnv1a {
    uint64_t h = 14695981039346656037ULL;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ULL;
    }
    template <class T>
    void value(const T& v) {
        static_assert(std::is_arithmetic_v<T>, "digest: a scalar is an integer, a bool or a double");
        if constexpr (std::is_same_v<T, bool>) {
            const unsigned char b = v ? 1 : 0;
            bytes(&b, 1);
        } else {
            unsigned char raw[sizeof(T)];   // (a double: its bit pattern)
            std::memcpy(raw, &v, sizeof(T));
            bytes(raw, sizeof(T));
        }
    }
    void value(const Schedule::BigTask& b) {   // (padding between the members: member by member)
        value(b.sn), value(b.row0), value(b.col0), value(b.weight), value(b.e0), value(b.e1), value(b.src_level), value(b.next);
        value(b.sr), value(b.sc), value(b.em), value(b.dweight), value(b.dchunks), value(b.strips), value(b.domain);
    }
    template <class T>
    void vec(const std::vector<T>& v) {
        const uint64_t len = v.size();
        value(len);
        if constexpr (std::is_same_v<T, Schedule::BigTask>) {
            for (const T& x : v) value(x);
        } else {
            static_assert(std::is_same_v<T, double> || std::has_unique_object_representations_v<T>,
                          "digest: this element type has padding -- hash it member by member");
            if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
        }
    }
};

using ScheduleDigest = std::vector<std::pair<const char*, uint64_t>>;

// EVERY data member of Schedule is listed below, in declaration order.  A member added to Schedule changes its size and
// stops the build here until it is listed too (and the size updated).
static_assert(sizeof(Schedule) == 1968,
              "Schedule changed: list every data member in schedule_digest() (schedule_digest.hpp), then update this size");
static_assert(sizeof(Schedule::OneLists) == 176,
              "Schedule::OneLists changed: list every data member in schedule_digest() (schedule_digest.hpp), then update this size");

// (only >= 0: just that field is hashed, the others are listed with 0 -- for a caller that asks field by field)
inline ScheduleDigest schedule_digest(const Schedule& S, int only = -1) {
    ScheduleDigest out;
#define PARSY_DIGEST_SCALAR(m)                                \
    {                                                         \
        Fnv1a f;                                              \
        if (only < 0 || only == (int)out.size()) f.value(S.m); \
        out.push_back({#m, f.h});                             \
    }
#define PARSY_DIGEST_VECTOR(m)                              \
    {                                                       \
        Fnv1a f;                                            \
        if (only < 0 || only == (int)out.size()) f.vec(S.m); \
        out.push_back({#m, f.h});                           \
    }
#define PARSY_DIGEST_ONE(o)                                                                              \
    PARSY_DIGEST_VECTOR(o.sn) PARSY_DIGEST_VECTOR(o.slot0) PARSY_DIGEST_VECTOR(o.wleft) PARSY_DIGEST_SCALAR(o.nslots) \
    PARSY_DIGEST_VECTOR(o.pull_ptr) PARSY_DIGEST_VECTOR(o.pull_slot) PARSY_DIGEST_VECTOR(o.pull_pos) PARSY_DIGEST_VECTOR(o.member)
    PARSY_DIGEST_SCALAR(n) PARSY_DIGEST_SCALAR(nsuper) PARSY_DIGEST_SCALAR(nlevels) PARSY_DIGEST_SCALAR(solve_only)
    PARSY_DIGEST_SCALAR(nnzA) PARSY_DIGEST_SCALAR(ssize) PARSY_DIGEST_SCALAR(xsize) PARSY_DIGEST_SCALAR(nnzL)
    PARSY_DIGEST_SCALAR(max_width) PARSY_DIGEST_SCALAR(max_rows) PARSY_DIGEST_SCALAR(n_small) PARSY_DIGEST_SCALAR(n_big)
    PARSY_DIGEST_SCALAR(n_solve_wide) PARSY_DIGEST_SCALAR(n_dslots) PARSY_DIGEST_SCALAR(n_tflags)
    PARSY_DIGEST_SCALAR(n_chain_launches) PARSY_DIGEST_SCALAR(n_solve_chain_launches) PARSY_DIGEST_SCALAR(walker_batch)
    PARSY_DIGEST_SCALAR(flops_stored) PARSY_DIGEST_SCALAR(update_flops) PARSY_DIGEST_SCALAR(reread_bytes)
    PARSY_DIGEST_SCALAR(tile_update_flops) PARSY_DIGEST_SCALAR(inner_flops)
    PARSY_DIGEST_VECTOR(sn) PARSY_DIGEST_VECTOR(sparent)
    PARSY_DIGEST_VECTOR(csn) PARSY_DIGEST_VECTOR(piece0) PARSY_DIGEST_VECTOR(csn_real)
    PARSY_DIGEST_VECTOR(clevelPtr) PARSY_DIGEST_VECTOR(clevelSet) PARSY_DIGEST_SCALAR(cnlevels)
    PARSY_DIGEST_SCALAR(big_min_k) PARSY_DIGEST_SCALAR(piece_width) PARSY_DIGEST_SCALAR(push_group)
    PARSY_DIGEST_SCALAR(big_super_r) PARSY_DIGEST_SCALAR(big_super_c)
    PARSY_DIGEST_VECTOR(upd) PARSY_DIGEST_VECTOR(upd_src) PARSY_DIGEST_VECTOR(relpos) PARSY_DIGEST_VECTOR(a_dst)
    PARSY_DIGEST_VECTOR(rows) PARSY_DIGEST_VECTOR(wave_entries) PARSY_DIGEST_VECTOR(wave_ptr)
    PARSY_DIGEST_VECTOR(chol_subtree) PARSY_DIGEST_VECTOR(solve_subtree) PARSY_DIGEST_VECTOR(bsolve_subtree)
    PARSY_DIGEST_VECTOR(solve_subtree_all) PARSY_DIGEST_VECTOR(bsolve_subtree_all)
    PARSY_DIGEST_VECTOR(chol_cost) PARSY_DIGEST_VECTOR(solve_cost)
    PARSY_DIGEST_SCALAR(n_chol_subtrees) PARSY_DIGEST_SCALAR(n_solve_subtrees) PARSY_DIGEST_SCALAR(n_bsolve_subtrees)
    PARSY_DIGEST_VECTOR(small_ranges) PARSY_DIGEST_VECTOR(solve_small_ranges) PARSY_DIGEST_VECTOR(bsolve_ranges)
    PARSY_DIGEST_VECTOR(sub_members) PARSY_DIGEST_VECTOR(sub_trees) PARSY_DIGEST_VECTOR(sub_slots)
    PARSY_DIGEST_VECTOR(sub_out_rows) PARSY_DIGEST_VECTOR(sub_tiers)
    PARSY_DIGEST_SCALAR(sub_cover_level) PARSY_DIGEST_SCALAR(sub_max_slots)
    PARSY_DIGEST_VECTOR(small_list) PARSY_DIGEST_VECTOR(tiles)
    PARSY_DIGEST_VECTOR(big_entries) PARSY_DIGEST_VECTOR(big_all) PARSY_DIGEST_VECTOR(big_tasks)
    PARSY_DIGEST_SCALAR(big_flops) PARSY_DIGEST_SCALAR(dense_flops)
    PARSY_DIGEST_SCALAR(n_dense_entries) PARSY_DIGEST_SCALAR(n_strip_entries)
    PARSY_DIGEST_VECTOR(chol)
    PARSY_DIGEST_VECTOR(solve_small_list) PARSY_DIGEST_VECTOR(solve_panels) PARSY_DIGEST_VECTOR(solve_mtasks)
    PARSY_DIGEST_VECTOR(solve_fix_list) PARSY_DIGEST_VECTOR(solve_wide_list) PARSY_DIGEST_VECTOR(solve)
    PARSY_DIGEST_VECTOR(bsolve_pairs) PARSY_DIGEST_VECTOR(bsolve_blocks) PARSY_DIGEST_VECTOR(bsolve_below)
    PARSY_DIGEST_SCALAR(n_bpart_slots) PARSY_DIGEST_VECTOR(bsolve)
    PARSY_DIGEST_SCALAR(solve_one) PARSY_DIGEST_SCALAR(solve_one_back) PARSY_DIGEST_SCALAR(one_subtrees)
    PARSY_DIGEST_SCALAR(one_big) PARSY_DIGEST_SCALAR(one_forced)
    PARSY_DIGEST_ONE(one_f)
    PARSY_DIGEST_ONE(one_b)
    PARSY_DIGEST_VECTOR(active) PARSY_DIGEST_VECTOR(active_piece) PARSY_DIGEST_VECTOR(chol_level_begin)
    PARSY_DIGEST_VECTOR(levelPtr) PARSY_DIGEST_VECTOR(levelSet)
    PARSY_DIGEST_VECTOR(split_ranges) PARSY_DIGEST_VECTOR(tile_split) PARSY_DIGEST_VECTOR(split_desc)
    PARSY_DIGEST_SCALAR(n_split_doubles)
    PARSY_DIGEST_VECTOR(sn_wp0) PARSY_DIGEST_VECTOR(sn_tw0) PARSY_DIGEST_VECTOR(tile_w) PARSY_DIGEST_VECTOR(level_of)
#undef PARSY_DIGEST_ONE
#undef PARSY_DIGEST_VECTOR
#undef PARSY_DIGEST_SCALAR
    return out;
}

}  // namespace parsy
