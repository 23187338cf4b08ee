// Update / downdate of the factor (updown.hpp): the checks of W, the pattern rule and the paths.  Host logic, no HIP call.
#include "updown.hpp"

#include <algorithm>

#include "errors.hpp"

namespace parsy {

// the supernode that holds column j
int supernode_of(const Schedule& S, int j) {
    int lo = 0, hi = S.nsuper - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (S.sn[(size_t)mid].c0 <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

namespace {

int refuse(const char* who, const std::string& what) {
    set_last_error(std::string(who) + ": " + what);
    return -1;
}

}  // namespace

int updown_prepare(const Schedule& S, const std::vector<int>& perm, const char* who, int k, const int* wp, const int* wi,
                   UpdownW& out) {
    out = UpdownW();
    if (k < 0) return refuse(who, "need k >= 0");
    out.ptr.assign((size_t)k + 1, 0);
    if (k == 0) return 0;
    if (!wp) return refuse(who, "null argument");
    if (wp[0] < 0) return refuse(who, "column pointers of W must start at 0 or above and not decrease");
    for (int t = 0; t < k; ++t)
        if (wp[t + 1] < wp[t]) return refuse(who, "column pointers of W must start at 0 or above and not decrease");
    const int nnz = wp[k] - wp[0];
    if (nnz > 0 && !wi) return refuse(who, "null argument");
    const int n = S.n;
    std::vector<int> inv;
    if (!perm.empty()) {
        inv.resize((size_t)n);
        for (int i = 0; i < n; ++i) inv[(size_t)perm[(size_t)i]] = i;
    }
    out.k = k;
    out.row.reserve((size_t)nnz);
    out.src.reserve((size_t)nnz);
    std::vector<std::pair<int, int>> col;
    std::vector<int> stamp((size_t)n, -1);
    for (int t = 0; t < k; ++t) {
        col.clear();
        for (int e = wp[t]; e < wp[t + 1]; ++e) {
            const int i = wi[e];
            if (i < 0 || i >= n)
                return refuse(who, "row index " + std::to_string(i) + " of column " + std::to_string(t) +
                                       " of W is out of range (n = " + std::to_string(n) + ")");
            if (e > wp[t] && wi[e - 1] >= i)
                return refuse(who, "row indices of column " + std::to_string(t) + " of W are unsorted or repeated (row " +
                                       std::to_string(i) + ")");
            col.push_back({inv.empty() ? i : inv[(size_t)i], e});
        }
        std::sort(col.begin(), col.end());
        if (!col.empty()) {
            // the pattern rule: every row in the structure of column j_t of L
            const int jt = col[0].first;
            const SnDesc& D = S.sn[(size_t)supernode_of(S, jt)];
            for (int i = jt - D.c0; i < D.r; ++i) stamp[(size_t)S.rows[(size_t)(D.pi + i)]] = t;
            for (const auto& rc : col)
                if (stamp[(size_t)rc.first] != t)
                    return refuse(who, "column " + std::to_string(t) + " of W has a non-zero at row " +
                                           std::to_string(wi[rc.second]) + " (row " + std::to_string(rc.first) +
                                           " of the factor's ordering) outside the structure of column " +
                                           std::to_string(jt) + " of L; the pattern of L does not change");
        }
        for (const auto& rc : col) {
            out.row.push_back(rc.first);
            out.src.push_back(rc.second);
        }
        out.ptr[(size_t)t + 1] = (int)out.row.size();
    }
    return 0;
}

void updown_path(const Schedule& S, const UpdownW& W, int t0, int t1, std::vector<UpdownNode>& path) {
    path.clear();
    std::vector<std::pair<int, int>> found;   // (supernode, column it is entered at), unordered, with repeats
    for (int t = std::max(t0, 0); t < std::min(t1, W.k); ++t) {
        if (W.ptr[(size_t)t] == W.ptr[(size_t)t + 1]) continue;
        int col = W.row[(size_t)W.ptr[(size_t)t]];
        int s = supernode_of(S, col);
        while (s >= 0) {
            const SnDesc& D = S.sn[(size_t)s];
            found.push_back({s, col});
            const int p = S.sparent[(size_t)s];
            if (p < 0) break;
            // a column of W leaves s with its first non-zero at the first row below s's columns (at the earliest)
            const SnDesc& P = S.sn[(size_t)p];
            col = D.r > D.w ? S.rows[(size_t)(D.pi + D.w)] : P.c0;
            if (col < P.c0 || col >= P.c0 + P.w) col = P.c0;
            s = p;
        }
    }
    std::sort(found.begin(), found.end());
    for (const auto& f : found)
        if (path.empty() || path.back().sn != f.first) path.push_back(UpdownNode{f.first, f.second});   // (the smallest column)
}

int64_t updown_block_columns(const Schedule& S, const std::vector<UpdownNode>& path) {
    int64_t nb = 0;
    for (const UpdownNode& N : path) {
        const SnDesc& D = S.sn[(size_t)N.sn];
        nb += (D.w + kUpdownTile - 1) / kUpdownTile - (N.first_col - D.c0) / kUpdownTile;
    }
    return nb;
}

}  // namespace parsy
