// The transpose of the row lists and the tasks of the factor's products (apply.hpp): host logic, no HIP call.
#include "apply.hpp"

#include <algorithm>

#include "../../include/parsy_amd.h"
#include "errors.hpp"
#include "plan_fwd.hpp"

namespace parsy {

void build_apply_index(const Schedule& S, ApplyIndex& I) {
    I = ApplyIndex();
    const int64_t ns = (int64_t)S.rows.size();
    I.ptr.assign((size_t)S.n + 1, 0);
    for (int64_t k = 0; k < ns; ++k) ++I.ptr[(size_t)S.rows[(size_t)k] + 1];
    for (int i = 0; i < S.n; ++i) {
        I.max_occurrences = (int32_t)std::max<int64_t>(I.max_occurrences, I.ptr[(size_t)i + 1]);
        I.ptr[(size_t)i + 1] += I.ptr[(size_t)i];
    }
    I.pos.assign((size_t)ns, 0);
    std::vector<int64_t> next(I.ptr.begin(), I.ptr.end() - 1);
    for (int64_t k = 0; k < ns; ++k) I.pos[(size_t)next[(size_t)S.rows[(size_t)k]]++] = k;   // (ascending k per row)
}

void build_apply_layout(const Schedule& S, const ApplyIndex& I, ApplyLayout& A) {
    A = ApplyLayout();
    std::vector<ApplyOcc> by_pos(S.rows.size());
    A.col.assign((size_t)S.n, ApplyCol{0, 0, 0});
    for (int t = 0; t < S.nsuper; ++t) {
        const SnDesc& D = S.sn[(size_t)t];
        // Y = L X: chunks of columns, 64 rows a task; chunk j reaches the rows from its first column on
        const int nch = (D.w + kApplyChunk - 1) / kApplyChunk;
        const int64_t tbase = A.t_rows;
        A.t_rows += (int64_t)nch * D.r;
        for (int j = 0; j < nch; ++j) {
            const int cb = j * kApplyChunk, ncol = std::min(kApplyChunk, D.w - cb);
            for (int i0 = cb; i0 < D.r; i0 += 64)
                A.l_tasks.push_back(ApplyTaskL{D.px + (int64_t)cb * D.r, tbase + (int64_t)j * D.r, D.r, D.c0 + cb, i0, ncol, cb, 0});
        }
        for (int i = 0; i < D.r; ++i)
            by_pos[(size_t)(D.pi + i)] = ApplyOcc{tbase + i, D.r, std::min(nch, i / kApplyChunk + 1)};
        // Y = L' X: blocks of columns, segments of rows; column c is reached by the segments from c / kApplySeg on
        const int nseg = (D.r + kApplySeg - 1) / kApplySeg;
        const int64_t pbase = A.p_rows;
        A.p_rows += (int64_t)nseg * D.w;
        for (int c = 0; c < D.w; c += kApplyCols) {
            const int nc = std::min(kApplyCols, D.w - c);
            for (int s = c / kApplySeg; s < nseg; ++s)
                A.lt_tasks.push_back(ApplyTaskLt{D.px + (int64_t)c * D.r, pbase + (int64_t)s * D.w + c, D.pi, D.r, c, nc,
                                                 std::max(s * kApplySeg, c / 64 * 64), std::min(D.r, (s + 1) * kApplySeg), 0});
        }
        for (int c = 0; c < D.w; ++c) {
            const int s0 = c / kApplySeg;
            A.col[(size_t)(D.c0 + c)] = ApplyCol{pbase + (int64_t)s0 * D.w + c, D.w, nseg - s0};
        }
    }
    A.occ.resize(I.pos.size());
    for (size_t k = 0; k < I.pos.size(); ++k) A.occ[k] = by_pos[(size_t)I.pos[k]];
}

int64_t apply_workspace_len(const Schedule& S, const ApplyLayout& A) {
    return std::max<int64_t>(1, std::max(A.t_rows, A.p_rows + S.n) * kApplyBlock);
}

}  // namespace parsy

extern "C" int parsy_factor_apply_row_index(const parsy_plan* pl, int64_t* ptr, int64_t* pos) {
    if (!pl || !ptr || !pos) {
        parsy::set_last_error("parsy_factor_apply_row_index: null argument");
        return -1;
    }
    parsy::ApplyIndex I;
    parsy::build_apply_index(parsy::plan_schedule(pl), I);
    std::copy(I.ptr.begin(), I.ptr.end(), ptr);
    std::copy(I.pos.begin(), I.pos.end(), pos);
    return 0;
}
