// Row delete / row add in the factor (rowmod.hpp): the row subtree, the checks of the new column and the pattern rule.
// Host logic, no HIP call.
#include "rowmod.hpp"

#include <algorithm>
#include <string>

#include "errors.hpp"
#include "updown.hpp"

namespace parsy {

namespace {

int refuse(const char* who, const std::string& what) {
    set_last_error(std::string(who) + ": " + what);
    return -1;
}

// whether `row` stands in the row list of D from position `from` on (the lists ascend)
bool holds_row(const Schedule& S, const SnDesc& D, int from, int row) {
    const int32_t* b = S.rows.data() + D.pi + from;
    const int32_t* e = S.rows.data() + D.pi + D.r;
    return std::binary_search(b, e, (int32_t)row);
}

}  // namespace

void rowmod_reach(const Schedule& S, const ApplyIndex& index, int p, std::vector<RowmodNode>& out) {
    out.clear();
    // the positions of p in lR ascend, and so do the supernodes they belong to; the last one is p's own
    int s = 0;
    for (int64_t e = index.ptr[(size_t)p]; e < index.ptr[(size_t)p + 1]; ++e) {
        const int64_t k = index.pos[(size_t)e];
        while (s + 1 < S.nsuper && S.sn[(size_t)s + 1].pi <= k) ++s;
        const SnDesc& D = S.sn[(size_t)s];
        const int pos = (int)(k - D.pi);
        const int ks = pos < D.w ? pos : D.w;
        if (ks > 0) out.push_back(RowmodNode{s, pos, ks, 0});
    }
    // heights: children have smaller indices, so a supernode's height is final when its turn comes
    std::vector<int> where((size_t)S.nsuper, -1);
    for (size_t i = 0; i < out.size(); ++i) where[(size_t)out[i].sn] = (int)i;
    for (size_t i = 0; i < out.size(); ++i) {
        const int par = S.sparent[(size_t)out[i].sn];
        if (par < 0 || par >= S.nsuper || where[(size_t)par] < 0) continue;
        RowmodNode& P = out[(size_t)where[(size_t)par]];
        P.height = std::max(P.height, out[i].height + 1);
    }
}

int64_t rowmod_entries_read(const Schedule& S, const std::vector<RowmodNode>& reach) {
    int64_t e = 0;
    for (const RowmodNode& N : reach) {
        const int64_t ks = N.ks, r = S.sn[(size_t)N.sn].r;
        e += ks * (ks + 1) / 2 + (r - ks) * ks;
    }
    return e;
}

int rowmod_first_below(const Schedule& S, int p) {
    const SnDesc& D = S.sn[(size_t)supernode_of(S, p)];
    const int q = p - D.c0;
    return q + 1 < D.r ? S.rows[(size_t)(D.pi + q + 1)] : -1;
}

int rowmod_position(const Schedule& S, const std::vector<int>& inv, const char* who, int row) {
    const int n = S.n;
    if (row < 0 || row >= n)
        return refuse(who, "row " + std::to_string(row) + " is out of range (n = " + std::to_string(n) + ")");
    return inv.empty() ? row : inv[(size_t)row];
}

int rowadd_prepare(const Schedule& S, const std::vector<int>& inv, const char* who, int row, int nz, const int* ci,
                   RowmodColumn& out) {
    out = RowmodColumn();
    const int n = S.n;
    const int p = rowmod_position(S, inv, who, row);
    if (p < 0) return -1;
    if (nz < 0) return refuse(who, "need nz >= 0");
    if (nz > 0 && !ci) return refuse(who, "null argument");
    std::vector<std::pair<int, int>> col;
    col.reserve((size_t)nz);
    bool diag = false;
    for (int e = 0; e < nz; ++e) {
        const int i = ci[e];
        if (i < 0 || i >= n)
            return refuse(who, "row index " + std::to_string(i) + " of the column is out of range (n = " + std::to_string(n) + ")");
        if (e > 0 && ci[e - 1] >= i)
            return refuse(who, "row indices of the column are unsorted or repeated (row " + std::to_string(i) + ")");
        diag = diag || i == row;
        col.push_back({inv.empty() ? i : inv[(size_t)i], e});
    }
    if (!diag) return refuse(who, "the column has no diagonal entry (row " + std::to_string(row) + ")");
    std::sort(col.begin(), col.end());
    // the pattern rule: (i, p) is a stored entry of L -- i > p in the structure of column p, i < p with p in the row list
    // of i's supernode from i on
    const SnDesc& Dp = S.sn[(size_t)supernode_of(S, p)];
    for (const auto& rc : col) {
        const int i = rc.first;
        bool stored = true;
        if (i > p) {
            stored = holds_row(S, Dp, p - Dp.c0, i);
        } else if (i < p) {
            const SnDesc& Di = S.sn[(size_t)supernode_of(S, i)];
            stored = holds_row(S, Di, i - Di.c0, p);
        }
        if (!stored)
            return refuse(who, "the column of row " + std::to_string(row) + " (row " + std::to_string(p) +
                                   " of the factor's ordering) has a non-zero at row " + std::to_string(ci[rc.second]) +
                                   " (row " + std::to_string(i) + " of the factor's ordering) outside the pattern of L; " +
                                   "the pattern of L does not change");
    }
    out.p = p;
    out.row.reserve(col.size());
    out.src.reserve(col.size());
    for (const auto& rc : col) {
        out.row.push_back(rc.first);
        out.src.push_back(rc.second);
    }
    return 0;
}

}  // namespace parsy
