// The pattern of A as a plan sees it (grad.hpp): host logic, no HIP call.
#include "grad.hpp"

#include <cstdlib>

#include "../../include/parsy_amd.h"
#include "errors.hpp"
#include "plan_fwd.hpp"

namespace parsy {

int grad_mrhs_min() {
    const char* e = std::getenv("PARSY_GRAD_MRHS_MIN");
    if (!e || !*e) return kGradMrhsMin;
    const long v = std::strtol(e, nullptr, 10);
    return v < 1 ? 1 : v > (1L << 30) ? (1 << 30) : (int)v;
}

bool build_grad_pattern(const Schedule& S, GradPattern& P, std::string& what) {
    P = GradPattern();
    P.row.assign((size_t)S.nnzA, 0);
    P.col.assign((size_t)S.nnzA, 0);
    for (int t = 0; t < S.nsuper; ++t) {
        const SnDesc& d = S.sn[t];
        for (int q = d.a0; q < d.a1; ++q) {
            const int64_t v = S.a_dst[q] - d.px;
            if (v < 0 || v >= (int64_t)d.w * d.r) {
                what = "A entry " + std::to_string(q) + " outside its supernode's panel";
                return false;
            }
            const int col = d.c0 + (int)(v / d.r), row = S.rows[d.pi + v % d.r];
            if (row < col || row >= S.n) {
                what = "A2 entry " + std::to_string(q) + " above the diagonal";
                return false;
            }
            P.row[q] = row;
            P.col[q] = col;
            P.offdiag += row != col;
        }
    }
    return true;
}

}  // namespace parsy

extern "C" int64_t parsy_plan_pattern(const parsy_plan* pl, int32_t* row, int32_t* col, int64_t* dst) {
    if (!pl) {
        parsy::set_last_error("parsy_plan_pattern: null plan");
        return -1;
    }
    const parsy::Schedule& S = parsy::plan_schedule(pl);
    if (row || col) {
        parsy::GradPattern P;
        std::string what;
        if (!parsy::build_grad_pattern(S, P, what)) {
            parsy::set_last_error("parsy_plan_pattern: " + what);
            return -1;
        }
        for (int64_t q = 0; q < S.nnzA; ++q) {
            if (row) row[q] = P.row[q];
            if (col) col[q] = P.col[q];
        }
    }
    if (dst)
        for (int64_t q = 0; q < S.nnzA; ++q) dst[q] = S.a_dst[q];
    return S.nnzA;
}
