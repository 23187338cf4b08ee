// Normal matrices on the plan's pattern (normal.hpp): the checks of F, the pattern of F F', the pair lists with their
// chunks and classes, the transposed index of F and the check of all of it.  Host logic, no HIP call.
#include "normal.hpp"

#include <algorithm>
#include <climits>

#include "../../include/parsy_amd.h"
#include "errors.hpp"
#include "grad.hpp"

namespace parsy {

namespace {

int refuse(const char* who, const std::string& what) {
    set_last_error(std::string(who) + ": " + what);
    return -1;
}

}  // namespace

int normal_check_f(const char* who, int n, int m, const int* Fp, const int* Fi) {
    if (m < 0) return refuse(who, "need m >= 0");
    if (n < 0) return refuse(who, "need n >= 0");
    if (!Fp) return refuse(who, "null argument");
    if (Fp[0] < 0) return refuse(who, "column pointers of F must start at 0 or above and not decrease");
    for (int k = 0; k < m; ++k)
        if (Fp[k + 1] < Fp[k]) return refuse(who, "column pointers of F must start at 0 or above and not decrease");
    // (Fp holds ints: the int32 limit on nnzF is the type's; a caller whose counts wrapped has decreasing pointers)
    if ((int64_t)Fp[m] - Fp[0] > 0 && !Fi) return refuse(who, "null argument");
    for (int k = 0; k < m; ++k)
        for (int e = Fp[k]; e < Fp[k + 1]; ++e) {
            const int i = Fi[e];
            if (i < 0 || i >= n)
                return refuse(who, "row index " + std::to_string(i) + " of column " + std::to_string(k) +
                                       " of F is out of range (n = " + std::to_string(n) + ")");
            if (e > Fp[k] && Fi[e - 1] >= i)
                return refuse(who, "row indices of column " + std::to_string(k) + " of F are unsorted or repeated (row " +
                                       std::to_string(i) + ")");
        }
    return 0;
}

int64_t normal_pattern(int n, int m, const int* Fp, const int* Fi, int* Ap, int* Ai) {
    const char* who = "parsy_normal_pattern";
    if (normal_check_f(who, n, m, Fp, Fi) != 0) return -1;
    if (!Ap) return refuse(who, "null argument");
    // the transposed index of F, then per column j the union of the rows >= j of the columns of F that hold j
    std::vector<int64_t> rp((size_t)n + 1, 0);
    for (int e = Fp[0]; e < Fp[m]; ++e) rp[(size_t)Fi[e] + 1] += 1;
    for (int i = 0; i < n; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
    std::vector<int> rc((size_t)std::max<int64_t>(rp[(size_t)n], 1));
    {
        std::vector<int64_t> fill(rp.begin(), rp.end() - 1);
        for (int k = 0; k < m; ++k)
            for (int e = Fp[k]; e < Fp[k + 1]; ++e) rc[(size_t)fill[(size_t)Fi[e]]++] = k;
    }
    std::vector<int> stamp((size_t)n, -1), rows;
    int64_t nnz = 0;
    Ap[0] = 0;
    for (int j = 0; j < n; ++j) {
        rows.clear();
        rows.push_back(j);
        stamp[(size_t)j] = j;
        for (int64_t t = rp[(size_t)j]; t < rp[(size_t)j + 1]; ++t) {
            const int k = rc[(size_t)t];
            for (int e = Fp[k + 1] - 1; e >= Fp[k] && Fi[e] > j; --e)
                if (stamp[(size_t)Fi[e]] != j) stamp[(size_t)Fi[e]] = j, rows.push_back(Fi[e]);
        }
        if (nnz + (int64_t)rows.size() > INT_MAX) return refuse(who, "the pattern has more than 2^31 - 1 entries");
        if (Ai) {
            std::sort(rows.begin(), rows.end());
            std::copy(rows.begin(), rows.end(), Ai + nnz);
        }
        nnz += (int64_t)rows.size();
        Ap[j + 1] = (int)nnz;
    }
    return nnz;
}

int normal_build(const Schedule& S, const std::vector<int>& perm, int m, const int* Fp, const int* Fi, NormalIndex& out) {
    const char* who = "parsy_normal_create";
    out = NormalIndex();
    const int n = S.n;
    if (normal_check_f(who, n, m, Fp, Fi) != 0) return -1;
    NormalIndex I;
    I.n = n, I.m = m, I.nnzA = S.nnzA;
    I.perm = perm;
    if (!perm.empty()) {
        I.inv.resize((size_t)n);
        for (int i = 0; i < n; ++i) I.inv[(size_t)perm[(size_t)i]] = i;
    }
    const int base = Fp[0], nnzF = Fp[m] - base;
    I.fp.resize((size_t)m + 1);
    for (int k = 0; k <= m; ++k) I.fp[(size_t)k] = Fp[k] - base;
    I.fi.assign(Fi + (nnzF > 0 ? base : 0), Fi + (nnzF > 0 ? base + nnzF : 0));
    {
        GradPattern P;
        std::string what;
        if (!build_grad_pattern(S, P, what)) return refuse(who, what);
        I.arow.swap(P.row);
        I.acol.swap(P.col);
    }
    // A's pattern by column, rows ascending, with the A2 index of every entry
    std::vector<int64_t> cp((size_t)n + 1, 0);
    for (int64_t q = 0; q < I.nnzA; ++q) cp[(size_t)I.acol[(size_t)q] + 1] += 1;
    for (int j = 0; j < n; ++j) cp[(size_t)j + 1] += cp[(size_t)j];
    std::vector<std::pair<int32_t, int32_t>> centry((size_t)I.nnzA);   // (row, q)
    {
        std::vector<int64_t> fill(cp.begin(), cp.end() - 1);
        for (int64_t q = 0; q < I.nnzA; ++q) centry[(size_t)fill[(size_t)I.acol[(size_t)q]]++] = {I.arow[(size_t)q], (int32_t)q};
        for (int j = 0; j < n; ++j) std::sort(centry.begin() + cp[(size_t)j], centry.begin() + cp[(size_t)j + 1]);
    }
    auto find = [&](int i, int j) -> int64_t {   // the A2 index of (i, j), i >= j, or -1
        auto b = centry.begin() + cp[(size_t)j], e = centry.begin() + cp[(size_t)j + 1];
        auto it = std::lower_bound(b, e, std::make_pair((int32_t)i, (int32_t)-1));
        return it != e && it->first == i ? it->second : -1;
    };
    I.diag.assign((size_t)I.nnzA, 0);
    for (int64_t q = 0; q < I.nnzA; ++q) I.diag[(size_t)q] = I.arow[(size_t)q] == I.acol[(size_t)q];
    // two passes over the pairs of every column, columns ascending: count, then fill; a list is ascending in k by construction
    I.lptr.assign((size_t)I.nnzA + 1, 0);
    std::vector<std::pair<int, int>> col;   // (row in the factor's ordering, position in fx)
    std::vector<int64_t> fill;
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < m; ++k) {
            col.clear();
            for (int e = I.fp[(size_t)k]; e < I.fp[(size_t)k + 1]; ++e)
                col.push_back({I.inv.empty() ? I.fi[(size_t)e] : I.inv[(size_t)I.fi[(size_t)e]], e});
            std::sort(col.begin(), col.end());
            for (size_t y = 0; y < col.size(); ++y)
                for (size_t x = y; x < col.size(); ++x) {
                    const int64_t q = find(col[x].first, col[y].first);
                    if (q < 0) {
                        const int ri = I.fi[(size_t)col[x].second], rj = I.fi[(size_t)col[y].second];
                        return refuse(who, "column " + std::to_string(k) + " of F holds rows " + std::to_string(ri) + " and " +
                                               std::to_string(rj) + " (rows " + std::to_string(col[x].first) + " and " +
                                               std::to_string(col[y].first) +
                                               " of the factor's ordering), which is no stored entry of the plan's pattern "
                                               "of A; the pattern of A does not change");
                    }
                    if (pass == 0) {
                        I.lptr[(size_t)q + 1] += 1;
                    } else {
                        const int64_t t = fill[(size_t)q]++;
                        I.ta[(size_t)t] = col[x].second, I.tb[(size_t)t] = col[y].second, I.tk[(size_t)t] = k;
                    }
                }
        }
        if (pass == 0) {
            for (int64_t q = 0; q < I.nnzA; ++q) I.lptr[(size_t)q + 1] += I.lptr[(size_t)q];
            I.pairs = I.lptr[(size_t)I.nnzA];
            I.ta.resize((size_t)I.pairs), I.tb.resize((size_t)I.pairs), I.tk.resize((size_t)I.pairs);
            fill.assign(I.lptr.begin(), I.lptr.end() - 1);
        }
    }
    // classes and chunks
    for (int64_t q = 0; q < I.nnzA; ++q) {
        const int64_t len = I.lptr[(size_t)q + 1] - I.lptr[(size_t)q];
        I.longest_list = (int32_t)std::max<int64_t>(I.longest_list, std::min<int64_t>(len, INT_MAX));
        I.entries_untouched += len == 0;
        if (len > kNormalChunk) {
            if ((int64_t)I.chunk_len.size() + (len + kNormalChunk - 1) / kNormalChunk > INT_MAX)
                return refuse(who, "more than 2^31 - 1 chunks");
            if (I.fold_ptr.empty()) I.fold_ptr.push_back(0);
            I.fold_q.push_back((int32_t)q);
            for (int64_t t = I.lptr[(size_t)q]; t < I.lptr[(size_t)q + 1]; t += kNormalChunk) {
                I.chunk_off.push_back(t);
                I.chunk_len.push_back((int32_t)std::min<int64_t>(kNormalChunk, I.lptr[(size_t)q + 1] - t));
            }
            I.fold_ptr.push_back((int32_t)I.chunk_len.size());
        } else {
            int c = 0;
            while (len > kNormalBorder[c]) ++c;
            I.cls[c].push_back((int32_t)q);
        }
    }
    if (I.fold_ptr.empty()) I.fold_ptr.push_back(0);
    // the transposed index of F by the caller's row: positions ascending
    I.rptr.assign((size_t)n + 1, 0);
    for (int e = 0; e < nnzF; ++e) I.rptr[(size_t)I.fi[(size_t)e] + 1] += 1;
    for (int i = 0; i < n; ++i) I.rptr[(size_t)i + 1] += I.rptr[(size_t)i];
    I.rpos.resize((size_t)nnzF), I.rcol.resize((size_t)nnzF);
    {
        std::vector<int64_t> f2(I.rptr.begin(), I.rptr.end() - 1);
        for (int k = 0; k < m; ++k)
            for (int e = I.fp[(size_t)k]; e < I.fp[(size_t)k + 1]; ++e) {
                const int64_t t = f2[(size_t)I.fi[(size_t)e]]++;
                I.rpos[(size_t)t] = e, I.rcol[(size_t)t] = k;
            }
    }
    out = std::move(I);
    return 0;
}

long long normal_check(const NormalIndex& I) {
    long long bad = 0;
    const int nnzF = I.nnzF();
    auto prow = [&](int e) { return I.inv.empty() ? I.fi[(size_t)e] : I.inv[(size_t)I.fi[(size_t)e]]; };
    // every triple is a pair of its column on the rows of its entry, every list strictly ascending in k (so no pair
    // twice: a column holds a row once), and there are as many triples as pairs
    int64_t expect = 0;
    for (int k = 0; k < I.m; ++k) {
        const int64_t c = I.fp[(size_t)k + 1] - I.fp[(size_t)k];
        expect += c * (c + 1) / 2;
    }
    bad += expect != I.pairs;
    bad += (int64_t)I.lptr.size() != I.nnzA + 1 || I.lptr[0] != 0 || I.lptr[(size_t)I.nnzA] != I.pairs;
    if (bad) return bad;
    std::vector<char> seen((size_t)I.nnzA, 0);
    for (int64_t q = 0; q < I.nnzA; ++q) {
        if (I.lptr[(size_t)q + 1] < I.lptr[(size_t)q]) return bad + 1;
        for (int64_t t = I.lptr[(size_t)q]; t < I.lptr[(size_t)q + 1]; ++t) {
            const int a = I.ta[(size_t)t], b = I.tb[(size_t)t], k = I.tk[(size_t)t];
            if (k < 0 || k >= I.m || a < I.fp[(size_t)k] || a >= I.fp[(size_t)k + 1] || b < I.fp[(size_t)k] ||
                b >= I.fp[(size_t)k + 1] || a >= nnzF || b >= nnzF) {
                ++bad;
                continue;
            }
            bad += prow(a) != I.arow[(size_t)q] || prow(b) != I.acol[(size_t)q];
            bad += t > I.lptr[(size_t)q] && I.tk[(size_t)t - 1] >= k;
        }
        bad += I.diag[(size_t)q] != (I.arow[(size_t)q] == I.acol[(size_t)q]);
    }
    // every entry in one class that fits its length, or chunked with chunks that tile its list
    for (int c = 0; c < kNormalClasses; ++c)
        for (int32_t q : I.cls[c]) {
            if (q < 0 || q >= I.nnzA || seen[(size_t)q]) {
                ++bad;
                continue;
            }
            seen[(size_t)q] = 1;
            const int64_t len = I.lptr[(size_t)q + 1] - I.lptr[(size_t)q];
            bad += len > kNormalBorder[c] || (c > 0 && len <= kNormalBorder[c - 1]);
        }
    bad += I.fold_ptr.size() != I.fold_q.size() + 1 || I.chunk_off.size() != I.chunk_len.size();
    if (bad) return bad;
    for (size_t f = 0; f < I.fold_q.size(); ++f) {
        const int32_t q = I.fold_q[f];
        if (q < 0 || q >= I.nnzA || seen[(size_t)q]) {
            ++bad;
            continue;
        }
        seen[(size_t)q] = 1;
        int64_t at = I.lptr[(size_t)q];
        bad += I.lptr[(size_t)q + 1] - at <= kNormalChunk;
        for (int32_t c = I.fold_ptr[f]; c < I.fold_ptr[f + 1]; ++c) {
            bad += I.chunk_off[(size_t)c] != at;
            bad += I.chunk_len[(size_t)c] < 1 || I.chunk_len[(size_t)c] > kNormalChunk;
            bad += c + 1 < I.fold_ptr[f + 1] && I.chunk_len[(size_t)c] != kNormalChunk;
            at += I.chunk_len[(size_t)c];
        }
        bad += at != I.lptr[(size_t)q + 1];
    }
    bad += !I.fold_ptr.empty() && I.fold_ptr.back() != (int32_t)I.chunk_len.size();
    for (int64_t q = 0; q < I.nnzA; ++q) bad += !seen[(size_t)q];
    // every position of the row index holds its row, positions ascending, each position once
    bad += (int64_t)I.rptr.size() != (int64_t)I.n + 1 || I.rptr[(size_t)I.n] != nnzF;
    if (bad) return bad;
    for (int i = 0; i < I.n; ++i)
        for (int64_t t = I.rptr[(size_t)i]; t < I.rptr[(size_t)i + 1]; ++t) {
            const int e = I.rpos[(size_t)t], k = I.rcol[(size_t)t];
            if (e < 0 || e >= nnzF || k < 0 || k >= I.m) {
                ++bad;
                continue;
            }
            bad += I.fi[(size_t)e] != i || e < I.fp[(size_t)k] || e >= I.fp[(size_t)k + 1];
            bad += t > I.rptr[(size_t)i] && I.rpos[(size_t)t - 1] >= e;
        }
    return bad;
}

}  // namespace parsy

extern "C" int64_t parsy_normal_pattern(int n, int m, const int* Fp, const int* Fi, int* Ap, int* Ai) {
    return parsy::normal_pattern(n, m, Fp, Fi, Ap, Ai);
}
