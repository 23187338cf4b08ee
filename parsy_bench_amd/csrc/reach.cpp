// The reaches of a sparse right-hand side and of a set of selected rows (reach.hpp): closures, the compact numbering,
// pieces, steps, the launch lists and the gather lists.  Host logic, no HIP call; the arrays of size nsuper it works
// with end with reach_build.
#include "reach.hpp"

#include <algorithm>
#include <string>

#include "errors.hpp"

namespace parsy {

namespace {

int refuse(const char* who, const std::string& what) {
    set_last_error(std::string(who) + ": " + what);
    return -1;
}

// the supernode that holds column j
int column_supernode(const Schedule& S, int j) {
    int lo = 0, hi = S.nsuper - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (S.sn[(size_t)mid].c0 <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

bool has_parent(const Schedule& S, int s) {
    const int p = S.sparent[(size_t)s];
    return p >= 0 && p < S.nsuper && p != s;
}

// mark s and its ancestors (stops at the first one that is marked: its ancestors are)
void close_up(const Schedule& S, int s, std::vector<uint8_t>& in) {
    while (!in[(size_t)s]) {
        in[(size_t)s] = 1;
        if (!has_parent(S, s)) break;
        s = S.sparent[(size_t)s];
    }
}

int pieces_of(int w) { return std::max(1, (w + kSparsePiece - 1) / kSparsePiece); }

// Pieces, steps and launch lists of one set.  ybase / ebase: per supernode of the set its first compact column and its
// first compact entry (indexed by supernode: transient arrays of reach_build).
void build_pass(const Schedule& S, const std::vector<int32_t>& set, const std::vector<int32_t>& ybase,
                const std::vector<int64_t>& ebase, bool backward, int64_t* npart, SparsePass& out) {
    out = SparsePass();
    out.sn = set;
    // children have smaller indices than their parents: a supernode's first step is final when its turn comes
    std::vector<int32_t> first((size_t)S.nsuper, 0);
    int nsteps = 0;
    size_t npieces = 0;
    for (int32_t s : set) {
        const int np = pieces_of(S.sn[(size_t)s].w);
        const int last = first[(size_t)s] + np - 1;
        nsteps = std::max(nsteps, last + 1);
        npieces += (size_t)np;
        if (has_parent(S, s)) {
            int32_t& f = first[(size_t)S.sparent[(size_t)s]];
            f = std::max(f, last + 1);
        }
        const int64_t w = S.sn[(size_t)s].w, r = S.sn[(size_t)s].r;
        out.entries += w * (w + 1) / 2 + (r - w) * w;
    }
    out.step_first.assign((size_t)nsteps + 1, 0);
    for (int32_t s : set)
        for (int k = 0, np = pieces_of(S.sn[(size_t)s].w); k < np; ++k) ++out.step_first[(size_t)(first[(size_t)s] + k) + 1];
    for (int t = 0; t < nsteps; ++t) out.step_first[(size_t)t + 1] += out.step_first[(size_t)t];
    out.pieces.resize(npieces);
    std::vector<int32_t> next(out.step_first.begin(), out.step_first.end() - 1);
    for (int32_t s : set) {
        const SnDesc& D = S.sn[(size_t)s];
        for (int k = 0, np = pieces_of(D.w); k < np; ++k) {
            SparsePiece P{};
            P.px = D.px, P.e0 = ebase[(size_t)s], P.p0 = 0;
            P.r = D.r, P.w = D.w;
            P.c0 = k * kSparsePiece, P.nc = std::min(kSparsePiece, D.w - P.c0);
            P.y0 = ybase[(size_t)s] + P.c0;
            const int below = D.r - (P.c0 + P.nc);
            P.nseg = backward ? (below + kSparseSeg - 1) / kSparseSeg : 0;
            if (backward) P.p0 = *npart, *npart += (int64_t)P.nseg * P.nc;
            out.pieces[(size_t)next[(size_t)(first[(size_t)s] + k)]++] = P;
        }
    }
    out.work_first.assign((size_t)nsteps + 1, 0);
    for (int t = 0; t < nsteps; ++t) {
        for (int32_t i = out.step_first[(size_t)t]; i < out.step_first[(size_t)t + 1]; ++i) {
            const SparsePiece& P = out.pieces[(size_t)i];
            if (!backward) {
                for (int row0 = P.c0 + P.nc; row0 < P.r; row0 += kSparseRows) out.work.push_back(i), out.work.push_back(row0);
            } else {
                const int groups = (P.nc + kSparseCols - 1) / kSparseCols;
                for (int code = 0; code < P.nseg * groups; ++code) out.work.push_back(i), out.work.push_back(code);
            }
        }
        out.work_first[(size_t)t + 1] = (int32_t)(out.work.size() / 2);
    }
}

}  // namespace

int reach_build(const Schedule& S, const std::vector<int>& inv, const char* who, int nrhs, const int* bp, const int* bi, int nx,
                const int* xi, ReachIndex& out) {
    out = ReachIndex();
    const int n = S.n;
    if (nrhs < 1) return refuse(who, "need nrhs >= 1");
    if (!bp) return refuse(who, "null argument");
    if (bp[0] != 0) return refuse(who, "bp must start at 0");
    for (int q = 0; q < nrhs; ++q)
        if (bp[q + 1] < bp[q]) return refuse(who, "bp decreases at column " + std::to_string(q));
    const int nnz = bp[nrhs];
    if (nnz > 0 && !bi) return refuse(who, "null argument");
    for (int q = 0; q < nrhs; ++q)
        for (int t = bp[q]; t < bp[q + 1]; ++t) {
            if (bi[t] < 0 || bi[t] >= n)
                return refuse(who, "row " + std::to_string(bi[t]) + " of column " + std::to_string(q) + " of B is out of range (n = " +
                                       std::to_string(n) + ")");
            if (t > bp[q] && bi[t - 1] >= bi[t])
                return refuse(who, "rows of column " + std::to_string(q) + " of B are unsorted or repeated (row " +
                                       std::to_string(bi[t]) + ")");
        }
    if (xi) {
        if (nx < 1) return refuse(who, "need nx >= 1 with a list of rows");
        std::vector<int> sorted(xi, xi + nx);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.front() < 0 || sorted.back() >= n)
            return refuse(who, "row " + std::to_string(sorted.front() < 0 ? sorted.front() : sorted.back()) +
                                   " of the selected rows is out of range (n = " + std::to_string(n) + ")");
        for (int k = 1; k < nx; ++k)
            if (sorted[(size_t)k - 1] == sorted[(size_t)k])
                return refuse(who, "row " + std::to_string(sorted[(size_t)k]) + " is repeated in the selected rows");
    } else {
        nx = n;
    }
    auto at = [&](int row) { return inv.empty() ? row : inv[(size_t)row]; };

    // the closures
    std::vector<uint8_t> inF((size_t)S.nsuper, 0), inK((size_t)S.nsuper, 0);
    for (int t = 0; t < nnz; ++t) close_up(S, column_supernode(S, at(bi[t])), inF);
    if (xi) {
        for (int k = 0; k < nx; ++k) close_up(S, column_supernode(S, at(xi[k])), inK);
    } else {
        std::fill(inK.begin(), inK.end(), (uint8_t)1);
    }
    // the compact numbering over F u K and the map of the row lists
    std::vector<int32_t> setF, setK, ybase((size_t)S.nsuper, -1);
    std::vector<int64_t> ebase((size_t)S.nsuper, -1);
    int64_t ncomp = 0, nent = 0;
    for (int s = 0; s < S.nsuper; ++s) {
        if (inF[(size_t)s]) setF.push_back(s);
        if (inK[(size_t)s]) setK.push_back(s);
        if (!inF[(size_t)s] && !inK[(size_t)s]) continue;
        ybase[(size_t)s] = (int32_t)ncomp, ebase[(size_t)s] = nent;
        ncomp += S.sn[(size_t)s].w, nent += S.sn[(size_t)s].r;
    }
    out.n = n, out.nrhs = nrhs, out.nx = nx, out.xsize = S.xsize;
    out.ncomp = (int32_t)ncomp, out.nent = nent;
    out.cmap.resize((size_t)nent);
    out.colmask.resize((size_t)ncomp);
    out.entmask.resize((size_t)nent);
    auto compact = [&](int row) {   // (-1: the row's supernode is outside F u K)
        const int t = column_supernode(S, row);
        return ybase[(size_t)t] < 0 ? -1 : ybase[(size_t)t] + (row - S.sn[(size_t)t].c0);
    };
    std::vector<int64_t> count((size_t)ncomp + 1, 0);
    for (int s = 0; s < S.nsuper; ++s) {
        if (ybase[(size_t)s] < 0) continue;
        const SnDesc& D = S.sn[(size_t)s];
        const uint8_t m = (uint8_t)((inF[(size_t)s] ? 1 : 0) | (inK[(size_t)s] ? 2 : 0));
        for (int j = 0; j < D.w; ++j) out.colmask[(size_t)(ybase[(size_t)s] + j)] = m;
        for (int i = 0; i < D.r; ++i) {
            const int c = compact(S.rows[(size_t)(D.pi + i)]);
            if (c < 0) {
                out = ReachIndex();
                return refuse(who, "the etree and the row lists disagree: a row below supernode " + std::to_string(s) +
                                       " belongs to no ancestor of it");
            }
            out.cmap[(size_t)(ebase[(size_t)s] + i)] = c;
            out.entmask[(size_t)(ebase[(size_t)s] + i)] = (uint8_t)(m & 1);
            if ((m & 1) && i >= D.w) ++count[(size_t)c + 1];
        }
    }
    // the forward gather: the occurrences of every column below the columns of the supernodes of F, ascending
    for (int64_t c = 0; c < ncomp; ++c) count[(size_t)c + 1] += count[(size_t)c];
    out.gptr = count;
    out.gpos.resize((size_t)count[(size_t)ncomp]);
    for (int32_t s : setF) {
        const SnDesc& D = S.sn[(size_t)s];
        for (int i = D.w; i < D.r; ++i) {
            const int64_t e = ebase[(size_t)s] + i;
            out.gpos[(size_t)count[(size_t)out.cmap[(size_t)e]]++] = e;
        }
    }
    // B and Xset in the compact numbering
    out.bcol.resize((size_t)nnz), out.bcomp.resize((size_t)nnz);
    for (int q = 0; q < nrhs; ++q)
        for (int t = bp[q]; t < bp[q + 1]; ++t) out.bcol[(size_t)t] = q, out.bcomp[(size_t)t] = compact(at(bi[t]));
    out.xcomp.resize((size_t)nx);
    for (int k = 0; k < nx; ++k) out.xcomp[(size_t)k] = compact(at(xi ? xi[k] : k));
    build_pass(S, setF, ybase, ebase, false, &out.npart, out.fwd);
    build_pass(S, setK, ybase, ebase, true, &out.npart, out.bwd);
    return 0;
}

int reach_kernels(const ReachIndex& I, int op) {
    int k = 3;   // the load, the gather, the clearing
    for (int dir = 0; dir < 2; ++dir) {
        if (op == (dir == 0 ? 2 : 1)) continue;   // (PARSY_SPARSE_GINVT has no forward pass, _GINV no backward one)
        const SparsePass& P = dir == 0 ? I.fwd : I.bwd;
        for (int t = 0; t < P.steps(); ++t) k += 1 + (P.work_first[(size_t)t + 1] > P.work_first[(size_t)t] ? 1 : 0);
    }
    return k;
}

long long reach_check(const Schedule& S, const ReachIndex& I) {
    long long bad = 0;
    for (int dir = 0; dir < 2; ++dir) {
        const SparsePass& P = dir == 0 ? I.fwd : I.bwd;
        const bool backward = dir == 1;
        std::vector<int32_t> in((size_t)S.nsuper, 0), last((size_t)S.nsuper, -1), firsts((size_t)S.nsuper, -1);
        for (size_t k = 0; k < P.sn.size(); ++k) {
            bad += k > 0 && P.sn[k - 1] >= P.sn[k];
            in[(size_t)P.sn[k]] = 1;
        }
        for (int32_t s : P.sn) bad += has_parent(S, s) && !in[(size_t)S.sparent[(size_t)s]];   // closed towards the root
        // pieces: per supernode they tile its columns, one step apart
        std::vector<int32_t> cover((size_t)S.nsuper, 0);
        int64_t work_seen = 0;
        std::vector<int64_t> have(P.pieces.size(), 0);   // panel work per piece, counted inside the piece's own step
        for (int t = 0; t < P.steps(); ++t)
            for (int32_t k = P.work_first[(size_t)t]; k < P.work_first[(size_t)t + 1]; ++k) {
                const int32_t i = P.work[(size_t)2 * k];
                if (i >= P.step_first[(size_t)t] && i < P.step_first[(size_t)t + 1]) ++have[(size_t)i];
                else ++bad;
            }
        for (int t = 0; t < P.steps(); ++t) {
            bad += P.step_first[(size_t)t + 1] <= P.step_first[(size_t)t];   // (no empty step)
            for (int32_t i = P.step_first[(size_t)t]; i < P.step_first[(size_t)t + 1]; ++i) {
                const SparsePiece& Q = P.pieces[(size_t)i];
                // its supernode, through its panel (the panels ascend in lValues)
                int sn = 0;
                for (int lo = 0, hi = S.nsuper - 1; lo <= hi;) {
                    const int mid = (lo + hi) / 2;
                    if (S.sn[(size_t)mid].px <= Q.px) sn = mid, lo = mid + 1;
                    else hi = mid - 1;
                }
                if (S.nsuper < 1 || !in[(size_t)sn] || S.sn[(size_t)sn].px != Q.px || S.sn[(size_t)sn].w != Q.w || S.sn[(size_t)sn].r != Q.r) {
                    ++bad;
                    continue;
                }
                bad += Q.c0 != cover[(size_t)sn] || Q.nc < 1 || Q.nc > kSparsePiece || Q.c0 + Q.nc > Q.w;
                bad += Q.c0 + Q.nc < Q.w && Q.nc != kSparsePiece;
                bad += Q.c0 > 0 && last[(size_t)sn] != t - 1;
                if (Q.c0 == 0) firsts[(size_t)sn] = t;
                cover[(size_t)sn] = Q.c0 + Q.nc, last[(size_t)sn] = t;
                // its panel work
                const int below = Q.r - (Q.c0 + Q.nc);
                const int64_t want = !backward ? (below + kSparseRows - 1) / kSparseRows
                                               : (int64_t)((below + kSparseSeg - 1) / kSparseSeg) * ((Q.nc + kSparseCols - 1) / kSparseCols);
                bad += have[(size_t)i] != want;
                work_seen += have[(size_t)i];
            }
        }
        bad += work_seen != (int64_t)P.work.size() / 2;
        for (int32_t s : P.sn) {
            bad += cover[(size_t)s] != S.sn[(size_t)s].w;
            if (has_parent(S, s)) bad += firsts[(size_t)S.sparent[(size_t)s]] <= last[(size_t)s];   // children first
        }
    }
    for (int32_t c : I.cmap) bad += c < 0 || c >= I.ncomp;
    for (int32_t c : I.xcomp) bad += c < 0 || c >= I.ncomp || !(I.colmask[(size_t)c] & 2);
    for (int32_t c : I.bcomp) bad += c < 0 || c >= I.ncomp || !(I.colmask[(size_t)c] & 1);
    for (int64_t c = 0; c < I.ncomp; ++c)
        for (int64_t e = I.gptr[(size_t)c]; e < I.gptr[(size_t)c + 1]; ++e) {
            bad += e > I.gptr[(size_t)c] && I.gpos[(size_t)e - 1] >= I.gpos[(size_t)e];
            bad += I.cmap[(size_t)I.gpos[(size_t)e]] != c || !I.entmask[(size_t)I.gpos[(size_t)e]];
        }
    return bad;
}

}  // namespace parsy
