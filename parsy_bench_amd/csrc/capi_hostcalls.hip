// C ABI, the host-buffer entry points (parsy_*_host): host arrays in, the device calls of the plan, host arrays out.
// No kernel lives here.  A's values, the factor and the right-hand sides are staged in buffers that live as long as the
// plan (h_values_dev, h_L_dev, h_x_dev; the selected inverse in SelinvState::h_z / h_diag); the gradient calls stage in
// buffers of their own, freed on return.  A call owns the staging buffers while it runs: one host-buffer call per plan
// at a time (the drop-in operators hold the plan's use_mu for that).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../include/parsy_amd.h"
#include "errors.hpp"
#include "hip_check.hpp"
#include "executor.hpp"
#include "plan_util.hpp"
#include "refine.hpp"
#include "cond.hpp"
#include "eigs.hpp"
#include "feature_states.hpp"

using parsy::set_last_error;

namespace {

// The refusal of the factorization and the plain solves ("plan has no device"; the other calls refuse through check_plan).
int check_device(const parsy_plan* pl, const char* who) {
    if (pl->device >= 0) return 0;
    set_last_error(std::string(who) + ": plan has no device");
    return -1;
}

// The plan-lifetime staging buffers a call uses, on the device the caller has selected: the factor's always, A's values
// on request (both made once), the right-hand sides' grown to x_len doubles (0: not used, left as it is).
hipError_t stage(parsy_plan* pl, bool values, int64_t x_len) {
    const parsy::Schedule& S = pl->S;
    hipError_t e = pl->h_L_dev.grow(std::max<int64_t>(S.xsize, 1));
    if (e == hipSuccess && values) e = pl->h_values_dev.grow(std::max<int64_t>(S.nnzA, 1));
    if (e == hipSuccess) e = pl->h_x_dev.grow(x_len);
    return e;
}

// The bands of levels of the pipelined host factorization and, per band, the runs of lValues that are final once
// the band is complete (a piece is final after the chain launch of its own level: everything that updates it comes
// from lower levels and is applied before that launch).  Pieces are in column order = lValues order, so consecutive
// pieces of one band are one run; runs separated by less than 128 K doubles are merged (the gap is copied early and
// again with its own band: harmless).  Built once per plan.
void build_download_bands(parsy_plan* pl) {
    const parsy::Schedule& S = pl->S;
    const int nl = S.cnlevels, np = (int)S.csn.size();
    // band boundaries: a band ends with the level at which another eighth of the factor's bytes has become final
    // (few bands = few, long runs: every copy from device to pageable host memory has a fixed cost), the last band
    // with the last level
    {
        std::vector<double> bytes((size_t)nl, 0.0);
        for (int p = 0; p < np; ++p) bytes[(size_t)S.level_of[(size_t)p]] += 8.0 * S.csn[(size_t)p].w * S.csn[(size_t)p].ld;   // (ld = rows of the supernode)
        const double total = 8.0 * (double)S.xsize;
        pl->h_band_level.clear();
        double run = 0, next = total / 8;
        for (int l = 0; l < nl; ++l) {
            run += bytes[(size_t)l];
            if (l == nl - 1 || run >= next) {
                pl->h_band_level.push_back(l);
                while (next <= run) next += total / 8;
            }
        }
    }
    const size_t nb = pl->h_band_level.size();
    pl->h_band_runs.assign(nb, {});
    std::vector<int> band_of((size_t)nl, 0);
    for (size_t b = 0, l = 0; b < nb; ++b)
        for (; (int)l <= pl->h_band_level[b]; ++l) band_of[l] = (int)b;
    const int64_t gap = 131072;
    for (int p = 0; p < np; ++p) {
        const parsy::SnDesc& C = S.csn[(size_t)p];
        const parsy::SnDesc& R = S.sn[(size_t)S.csn_real[(size_t)p]];
        // (a piece's columns are whole columns of its supernode's panel)
        const int64_t a = R.px + (int64_t)C.rbias * R.r, e = R.px + (int64_t)(C.rbias + C.w) * R.r;
        auto& runs = pl->h_band_runs[(size_t)band_of[(size_t)S.level_of[(size_t)p]]];
        if (!runs.empty() && a - (runs.back().first + runs.back().second) <= gap && a >= runs.back().first)
            runs.back().second = std::max(runs.back().second, e - runs.back().first);
        else
            runs.push_back({a, e - a});
    }
}

// The streams, bands and events of the pipelined download, made on its first use.  They are made into locals and handed
// to the plan only when all of them exist: a setup that failed half-way must not leave a plan that "pipelines" over no
// band at all (and downloads nothing).  false: the caller takes the plain form.
bool ensure_pipeline(parsy_plan* pl) {
    if (pl->h_ready) return true;
    hipStream_t hs = nullptr, hc = nullptr;
    std::vector<hipEvent_t> evs;
    bool ok = hipStreamCreateWithFlags(&hs, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&hc, hipStreamNonBlocking) == hipSuccess;
    if (ok) {
        build_download_bands(pl);
        evs.resize(pl->h_band_level.size(), nullptr);
        for (hipEvent_t& e : evs)
            if (ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                e = nullptr;
                ok = false;
            }
        ok = ok && !evs.empty();
    }
    if (!ok) {
        for (hipEvent_t e : evs)
            if (e) (void)hipEventDestroy(e);
        if (hs) (void)hipStreamDestroy(hs);
        if (hc) (void)hipStreamDestroy(hc);
        pl->h_band_level.clear();
        pl->h_band_runs.clear();
        (void)hipGetLastError();
        return false;
    }
    pl->h_stream = hs;
    pl->h_copy = hc;
    pl->h_band_ev = evs;
    pl->h_ready = true;
    return true;
}

// parsy_solve_host / parsy_solve2_host: L and x to the device, the chosen directions with the status read after each,
// x back.  x stays untouched when a status is bad: it would not be the solution.
int solve_staged(parsy_plan* pl, const char* who, const double* lValues, double* x, int nrhs, int ldx, bool forward,
                 bool backward, double* seconds) {
    if (!pl || !lValues || !x) {
        set_last_error(std::string(who) + ": null argument");
        return -1;
    }
    if (check_device(pl, who) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    const int64_t need = (int64_t)ldx * nrhs;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, false, need));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice));
    PARSY_HIP(hipMemcpy(pl->h_x_dev.data(), x, (size_t)need * 8, hipMemcpyHostToDevice));
    double sec = 0;
    auto run = [&](bool back) -> int {
        const int rc = back ? parsy::plan_backsolve(pl, pl->h_L_dev.data(), pl->h_x_dev.data(), nrhs, ldx, nullptr)
                            : parsy::plan_solve(pl, pl->h_L_dev.data(), pl->h_x_dev.data(), nrhs, ldx, nullptr);
        if (rc != 0) return -1;
        PARSY_HIP(hipDeviceSynchronize());
        if (parsy_solve_status(pl) != 0) return -1;
        if (seconds) sec += parsy_last_solve_ms(pl) * 1e-3;   // (the plan's own solve events)
        return 0;
    };
    if (forward && run(false) != 0) return -1;
    if (backward && run(true) != 0) return -1;
    if (seconds) *seconds = sec;
    PARSY_HIP(hipMemcpy(x, pl->h_x_dev.data(), (size_t)need * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Device buffers of one gradient host call, freed when it returns, and the call's timer.
struct Scratch {
    parsy::DevicePool bufs;
    parsy::EventTimer timer;
    double* upload(const double* h, int64_t len, bool copy) {
        double* d = bufs.alloc<double>(std::max<int64_t>(len, 1));
        if (!d) return nullptr;
        if (copy && len > 0 && hipMemcpy(d, h, (size_t)len * 8, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
};

}  // namespace

extern "C" {

int parsy_factor_host(parsy_plan* pl, const double* values, double* lValues, double* seconds) {
    const char* who = "parsy_factor_host";
    if (!pl || !values || !lValues) {
        set_last_error(std::string(who) + ": null argument");
        return -1;
    }
    if (check_device(pl, who) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, true, 0));
    PARSY_HIP(hipMemcpy(pl->h_values_dev.data(), values, (size_t)S.nnzA * 8, hipMemcpyHostToDevice));
    // Small factors take the plain form: kernels, then one download.  Large ones (PARSY_HOST_PIPELINE=0: never): the
    // download of every band of levels runs BEHIND the kernels of the levels above it -- a worker thread copies the runs
    // of lValues that a band has made final while this thread's stream goes on (Flan-class: 19.4 GB at PCIe speed take as
    // long as the kernels; one after the other the call was 0.78 s).
    // (read per call: the tests switch it; PARSY_HOST_PIPELINE=2 takes the pipelined path whatever the size)
    const char* pe = std::getenv("PARSY_HOST_PIPELINE");
    const bool pipeline_on = !(pe && pe[0] == '0'), pipeline_forced = pe && pe[0] == '2';
    if (!pipeline_on || (!pipeline_forced && S.xsize * 8 < (int64_t)256 << 20) || pl->profile || S.cnlevels < 1 ||
        !ensure_pipeline(pl)) {
        if (parsy::plan_factor(pl, pl->h_values_dev.data(), pl->h_L_dev.data(), nullptr) != 0) return -1;
        PARSY_HIP(hipDeviceSynchronize());
        if (seconds) *seconds = parsy_last_factor_ms(pl) * 1e-3;
        PARSY_HIP(hipMemcpy(lValues, pl->h_L_dev.data(), (size_t)S.xsize * 8, hipMemcpyDeviceToHost));
        return 0;
    }
    const size_t nb = pl->h_band_level.size();
    std::atomic<int> recorded{0};
    std::atomic<int> failed{0};
    double* const dL = pl->h_L_dev.data();
    const int device = pl->device;
    std::thread worker([&, dL, device] {
        if (hipSetDevice(device) != hipSuccess) {
            failed = 1;
            return;
        }
        for (size_t b = 0; b < nb; ++b) {
            while (recorded.load(std::memory_order_acquire) <= (int)b && !failed.load()) std::this_thread::yield();
            if (failed.load()) return;
            if (hipEventSynchronize(pl->h_band_ev[b]) != hipSuccess) {
                failed = 1;
                return;
            }
            for (const auto& r : pl->h_band_runs[b])
                if (hipMemcpyAsync(lValues + r.first, dL + r.first, (size_t)r.second * 8, hipMemcpyDeviceToHost, pl->h_copy) !=
                    hipSuccess) {
                    failed = 1;
                    return;
                }
            if (hipStreamSynchronize(pl->h_copy) != hipSuccess) {
                failed = 1;
                return;
            }
        }
    });
    int rc = parsy::plan_factor_begin(pl, pl->h_values_dev.data(), dL, pl->h_stream, true);
    size_t b = 0;
    for (int lev = 0; rc == 0 && lev < S.cnlevels; ++lev) {
        rc = parsy::plan_factor_levels(pl, lev, lev + 1, dL, pl->h_stream);
        if (rc == 0 && b < nb && pl->h_band_level[b] == lev) {
            if (hipEventRecord(pl->h_band_ev[b], pl->h_stream) != hipSuccess) rc = -1;
            ++b;
            recorded.store((int)b, std::memory_order_release);
        }
    }
    if (rc == 0) rc = parsy::plan_factor_end(pl, pl->h_stream);
    if (rc != 0) {
        failed = 1;
        worker.join();
        parsy::plan_factor_abort(pl, pl->h_stream);
        return -1;
    }
    const hipError_t es = hipStreamSynchronize(pl->h_stream);
    worker.join();
    if (es != hipSuccess || failed.load()) {
        set_last_error(std::string(who) + ": the pipelined download failed");
        return -1;
    }
    if (seconds) *seconds = parsy_last_factor_ms(pl) * 1e-3;
    return 0;
}

int parsy_solve_host(parsy_plan* pl, const double* lValues, double* x, int nrhs, int ldx, double* seconds) {
    return solve_staged(pl, "parsy_solve_host", lValues, x, nrhs, ldx, true, false, seconds);
}

int parsy_solve2_host(parsy_plan* pl, const double* lValues, double* x, int nrhs, int ldx, int forward,
                      double* seconds) {
    return solve_staged(pl, "parsy_solve2_host", lValues, x, nrhs, ldx, forward != 0, true, seconds);
}

int parsy_solve_spd_host(parsy_plan* pl, const double* values, const double* lValues, const double* b, int ldb,
                         double* x, int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, double* seconds) {
    return parsy_solve_spd_bounds_host(pl, values, lValues, b, ldb, x, ldx, nrhs, max_steps, steps, berr, nullptr, seconds);
}

int parsy_solve_spd_bounds_host(parsy_plan* pl, const double* values, const double* lValues, const double* b, int ldb,
                                double* x, int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, double* ferr,
                                double* seconds) {
    const char* who = ferr ? "parsy_solve_spd_bounds_host" : "parsy_solve_spd_host";
    if (!pl || !values || !lValues || !b || !x) {
        set_last_error(std::string(who) + ": null argument");
        return -1;
    }
    if (parsy::check_plan(pl, who, parsy::kNeedsDevice) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    if (nrhs < 1 || ldb < S.n || ldx < S.n) {
        set_last_error(std::string(who) + ": need nrhs >= 1 and leading dimensions >= n");
        return -1;
    }
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, true, std::max<int64_t>((int64_t)S.n * nrhs, 1)));
    const size_t row = (size_t)S.n * 8;
    PARSY_HIP(hipMemcpy(pl->h_values_dev.data(), values, (size_t)S.nnzA * 8, hipMemcpyHostToDevice));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice));
    if (S.n > 0) PARSY_HIP(hipMemcpy2D(pl->h_x_dev.data(), row, b, (size_t)ldb * 8, row, nrhs, hipMemcpyHostToDevice));
    parsy::EventTimer timer;
    if (!timer.start()) {
        set_last_error(std::string(who) + ": hipEventCreate failed");
        return -1;
    }
    double* const dx = pl->h_x_dev.data();
    if (parsy::plan_solve_refined(pl, pl->h_values_dev.data(), pl->h_L_dev.data(), dx, S.n, dx, S.n, nrhs, max_steps, steps,
                                  berr, ferr, nullptr) != 0)
        return -1;
    double sec = 0;
    if (!timer.stop(&sec)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    // (max_steps == 0 without steps / berr: nothing synchronised inside the call, so the solves' status is read here)
    if (parsy_solve_status(pl) != 0) return -1;
    if (seconds) *seconds = sec;
    if (S.n > 0) PARSY_HIP(hipMemcpy2D(x, (size_t)ldx * 8, pl->h_x_dev.data(), row, row, nrhs, hipMemcpyDeviceToHost));
    return 0;
}

int parsy_rcond_host(parsy_plan* pl, const double* values, const double* lValues, double* anorm, double* rcond,
                     double* seconds) {
    const char* who = "parsy_rcond_host";
    if (!pl || !values || !lValues || (!anorm && !rcond)) {
        set_last_error(std::string(who) + ": null argument (anorm and rcond may not both be NULL)");
        return -1;
    }
    if (parsy::check_plan(pl, who, parsy::kNeedsDevice) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, true, 0));
    PARSY_HIP(hipMemcpy(pl->h_values_dev.data(), values, (size_t)S.nnzA * 8, hipMemcpyHostToDevice));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice));
    parsy::EventTimer timer;
    if (!timer.start()) {
        set_last_error(std::string(who) + ": hipEventCreate failed");
        return -1;
    }
    double an = 0, rc = 0;
    if (parsy::plan_rcond(pl, pl->h_values_dev.data(), pl->h_L_dev.data(), &an, rcond ? &rc : nullptr, nullptr) != 0)
        return -1;
    if (!timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    if (anorm) *anorm = an;
    if (rcond) *rcond = rc;
    return 0;
}

int parsy_eigs_host(parsy_plan* pl, const double* values, const double* mvalues, const double* lValues, int k,
                    const double* x0, int ldx0, int block, double tol, int max_basis, int max_iter, double* lambda, double* y,
                    int ldy, double* resid, int32_t* nconv, double* seconds) {
    const char* who = "parsy_eigs_host";
    if (!pl || !values || !lValues || !x0 || !lambda || !y || !resid || !nconv) {
        set_last_error(std::string(who) + ": null argument (only mvalues may be NULL)");
        return -1;
    }
    if (parsy::check_plan(pl, who, parsy::kNeedsDevice) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    if (k < 1 || k > parsy::kEigsMaxBasis || block < 1 || block > parsy::kEigsMaxBlock || ldx0 < S.n || ldy < S.n) {
        set_last_error(std::string(who) + ": need 1 <= k <= 128, 1 <= block <= 16 and leading dimensions >= n");
        return -1;
    }
    PARSY_HIP(hipSetDevice(pl->device));
    // x0 and Y share the staging buffer of the right-hand sides; M's values get one that lives as long as the call
    const int64_t nx0 = (int64_t)S.n * block, ny = (int64_t)S.n * k;
    PARSY_HIP(stage(pl, true, std::max<int64_t>(nx0 + ny, 1)));
    parsy::DeviceBuf<double> m_dev;
    if (mvalues) {
        PARSY_HIP(m_dev.grow(std::max<int64_t>(S.nnzA, 1)));
        PARSY_HIP(hipMemcpy(m_dev.data(), mvalues, (size_t)S.nnzA * 8, hipMemcpyHostToDevice));
    }
    const size_t row = (size_t)S.n * 8;
    PARSY_HIP(hipMemcpy(pl->h_values_dev.data(), values, (size_t)S.nnzA * 8, hipMemcpyHostToDevice));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice));
    double *dx0 = pl->h_x_dev.data(), *dy = dx0 + nx0;
    if (S.n > 0) PARSY_HIP(hipMemcpy2D(dx0, row, x0, (size_t)ldx0 * 8, row, block, hipMemcpyHostToDevice));
    parsy::EventTimer timer;
    if (!timer.start()) {
        set_last_error(std::string(who) + ": hipEventCreate failed");
        return -1;
    }
    // (into locals: a refusal or a failure leaves the caller's outputs untouched)
    std::vector<double> lam((size_t)k), res((size_t)k);
    int32_t nc = 0;
    const int rc = parsy::plan_eigs(pl, pl->h_values_dev.data(), mvalues ? m_dev.data() : nullptr, pl->h_L_dev.data(), k, dx0,
                                    S.n, block, tol, max_basis, max_iter, lam.data(), dy, S.n, res.data(), &nc, nullptr);
    if (rc != 0) {
        (void)hipDeviceSynchronize();   // (m_dev is freed on return)
        return rc;
    }
    if (!timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    if (S.n > 0) PARSY_HIP(hipMemcpy2D(y, (size_t)ldy * 8, dy, row, row, k, hipMemcpyDeviceToHost));
    std::copy(lam.begin(), lam.end(), lambda);
    std::copy(res.begin(), res.end(), resid);
    *nconv = nc;
    return 0;
}

int parsy_selinv_host(parsy_plan* pl, const double* lValues, double* z, double* diag, double* seconds) {
    const char* who = "parsy_selinv_host";
    if (!pl || !lValues || !z) {
        set_last_error(std::string(who) + ": null argument");
        return -1;
    }
    if (parsy::check_plan(pl, who, parsy::kNeedsIdle) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    parsy::SelinvState& X = parsy::selinv_state(pl);
    if (hipSetDevice(pl->device) != hipSuccess) {
        set_last_error(std::string(who) + ": hipSetDevice failed");
        return -1;
    }
    if (stage(pl, false, 0) != hipSuccess ||
        X.h_z.grow(std::max<int64_t>(S.xsize, 1)) != hipSuccess ||
        X.h_diag.grow(std::max<int64_t>(S.n, 1)) != hipSuccess) {
        set_last_error(std::string(who) + ": hipMalloc failed");
        return -1;
    }
    if (hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice) != hipSuccess) {
        set_last_error(std::string(who) + ": upload failed");
        return -1;
    }
    parsy::EventTimer timer;
    if (!timer.start()) {
        set_last_error(std::string(who) + ": hipEventCreate failed");
        return -1;
    }
    if (parsy_selinv_device(pl, pl->h_L_dev.data(), X.h_z.data(), nullptr) != 0) return -1;
    if (diag && parsy_inverse_diag_device(pl, X.h_z.data(), X.h_diag.data(), nullptr) != 0) return -1;
    if (!timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    if (hipMemcpy(z, X.h_z.data(), (size_t)S.xsize * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        (diag && S.n > 0 && hipMemcpy(diag, X.h_diag.data(), (size_t)S.n * 8, hipMemcpyDeviceToHost) != hipSuccess)) {
        set_last_error(std::string(who) + ": download failed");
        return -1;
    }
    return 0;
}

int parsy_pattern_outer_host(parsy_plan* pl, const double* lam, int ldl, const double* x, int ldx, int nrhs, double alpha,
                             double beta, double* g, double* seconds) {
    const char* who = "parsy_pattern_outer_host";
    if (!pl || !lam || !x || !g) {
        set_last_error(std::string(who) + ": null argument");
        return -1;
    }
    if (parsy::check_plan(pl, who, parsy::kNeedsA) != 0) return -1;
    const int n = pl->S.n;
    if (nrhs < 1 || ldl < n || ldx < n) {
        set_last_error(std::string(who) + ": need nrhs >= 1 and leading dimensions >= n");
        return -1;
    }
    PARSY_HIP(hipSetDevice(pl->device));
    Scratch sc;
    const int64_t nnz = pl->S.nnzA;
    double* d_lam = sc.upload(lam, (int64_t)ldl * (nrhs - 1) + n, true);
    double* d_x = sc.upload(x, (int64_t)ldx * (nrhs - 1) + n, true);
    double* d_g = sc.upload(g, nnz, beta != 0.0);
    if (!d_lam || !d_x || !d_g || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (parsy_pattern_outer_device(pl, d_lam, ldl, d_x, ldx, nrhs, alpha, beta, d_g, nullptr) != 0) return -1;
    if (!sc.timer.stop(seconds) || (nnz > 0 && hipMemcpy(g, d_g, (size_t)nnz * 8, hipMemcpyDeviceToHost) != hipSuccess)) {
        set_last_error(std::string(who) + ": download failed");
        return -1;
    }
    return 0;
}

int parsy_inverse_pattern_host(parsy_plan* pl, const double* z, double alpha, double beta, int flags, double* g,
                               double* seconds) {
    const char* who = "parsy_inverse_pattern_host";
    if (!pl || !z || !g) {
        set_last_error(std::string(who) + ": null argument");
        return -1;
    }
    if (parsy::check_plan(pl, who, parsy::kNeedsA) != 0) return -1;
    PARSY_HIP(hipSetDevice(pl->device));
    Scratch sc;
    const int64_t nnz = pl->S.nnzA;
    double* d_z = sc.upload(z, pl->S.xsize, true);
    double* d_g = sc.upload(g, nnz, beta != 0.0);
    if (!d_z || !d_g || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (parsy_inverse_pattern_device(pl, d_z, alpha, beta, flags, d_g, nullptr) != 0) return -1;
    if (!sc.timer.stop(seconds) || (nnz > 0 && hipMemcpy(g, d_g, (size_t)nnz * 8, hipMemcpyDeviceToHost) != hipSuccess)) {
        set_last_error(std::string(who) + ": download failed");
        return -1;
    }
    return 0;
}

int parsy_factor_apply_host(parsy_plan* pl, const double* lValues, int op, const double* x, int ldx, int nrhs, double alpha,
                            double beta, double* y, int ldy, double* seconds) {
    const char* who = "parsy_factor_apply_host";
    if (parsy::apply_check_args(pl, who, lValues, op, x, ldx, nrhs, y, ldy) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    const int n = S.n;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, false, 0));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice));
    // X and Y with leading dimension n on the device; Y goes up only when it is read
    Scratch sc;
    const int64_t len = (int64_t)n * nrhs;
    const size_t row = (size_t)n * 8;
    double* d_x = sc.upload(nullptr, len, false);
    double* d_y = sc.upload(nullptr, len, false);
    if (!d_x || !d_y || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (n > 0) {
        PARSY_HIP(hipMemcpy2D(d_x, row, x, (size_t)ldx * 8, row, nrhs, hipMemcpyHostToDevice));
        if (beta != 0.0) PARSY_HIP(hipMemcpy2D(d_y, row, y, (size_t)ldy * 8, row, nrhs, hipMemcpyHostToDevice));
    }
    if (parsy_factor_apply_device(pl, pl->h_L_dev.data(), op, d_x, std::max(n, 1), nrhs, alpha, beta, d_y, std::max(n, 1),
                                  nullptr) != 0)
        return -1;
    if (!sc.timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    // (y stays untouched when a solve's status is bad: it would not be the result)
    if ((op == PARSY_OP_GINV || op == PARSY_OP_GINVT) && parsy_solve_status(pl) != 0) return -1;
    if (n > 0) PARSY_HIP(hipMemcpy2D(y, (size_t)ldy * 8, d_y, row, row, nrhs, hipMemcpyDeviceToHost));
    return 0;
}

int parsy_factor_updown_host(parsy_plan* pl, double* lValues, int sign, int k, const int* wp, const int* wi, const double* wx,
                             double* seconds) {
    const char* who = "parsy_factor_updown_host";
    if (parsy::updown_check_args(pl, who, lValues, sign, k, wp, wi, wx) != 0) return -1;
    {
        // the refusals of W come before the one of a host-only plan, as in the device call
        parsy::UpdownW W;
        if (parsy::updown_prepare(pl->S, pl->perm, who, k, wp, wi, W) != 0) return -1;
    }
    if (parsy::check_plan(pl, who, parsy::kNeedsDevice) != 0) return -1;
    if (seconds) *seconds = 0.0;
    if (k == 0) return parsy_factor_updown_device(pl, nullptr, sign, 0, wp, wi, nullptr, nullptr);
    const parsy::Schedule& S = pl->S;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, false, 0));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice));
    Scratch sc;
    double* d_wx = sc.upload(wx, wp[k], wp[k] > wp[0]);   // (positions in wx count from its start, whatever wp[0] is)
    if (!d_wx || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (parsy_factor_updown_device(pl, pl->h_L_dev.data(), sign, k, wp, wi, d_wx, nullptr) != 0) return -1;
    if (!sc.timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    PARSY_HIP(hipMemcpy(lValues, pl->h_L_dev.data(), (size_t)S.xsize * 8, hipMemcpyDeviceToHost));
    return 0;
}

int parsy_factor_rowdel_host(parsy_plan* pl, double* lValues, int row, double* seconds) {
    const char* who = "parsy_factor_rowdel_host";
    if (parsy::rowdel_check_args(pl, who, lValues, row, nullptr) != 0) return -1;
    if (parsy::check_plan(pl, who, parsy::kNeedsDevice) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, false, 0));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice));
    parsy::EventTimer timer;
    if (!timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (parsy_factor_rowdel_device(pl, pl->h_L_dev.data(), row, nullptr) != 0) return -1;
    if (!timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    PARSY_HIP(hipMemcpy(lValues, pl->h_L_dev.data(), (size_t)S.xsize * 8, hipMemcpyDeviceToHost));
    return 0;
}

int parsy_factor_rowadd_host(parsy_plan* pl, double* lValues, int row, int nz, const int* ci, const double* cx,
                             double* seconds) {
    const char* who = "parsy_factor_rowadd_host";
    {
        // the refusals of the column come before the one of a host-only plan, as in the device call
        parsy::RowmodColumn col;
        if (parsy::rowadd_check_args(pl, who, lValues, row, nz, ci, cx, col) != 0) return -1;
    }
    if (parsy::check_plan(pl, who, parsy::kNeedsDevice) != 0) return -1;
    const parsy::Schedule& S = pl->S;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, false, 0));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)S.xsize * 8, hipMemcpyHostToDevice));
    Scratch sc;
    double* d_cx = sc.upload(cx, nz, true);
    if (!d_cx || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (parsy_factor_rowadd_device(pl, pl->h_L_dev.data(), row, nz, ci, d_cx, nullptr) != 0) return -1;
    if (!sc.timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    PARSY_HIP(hipMemcpy(lValues, pl->h_L_dev.data(), (size_t)S.xsize * 8, hipMemcpyDeviceToHost));
    return 0;
}

// The normal-matrix calls stage in buffers of their own, freed on return; operands go to the device with the leading
// dimension of their row count.
int parsy_normal_values_host(parsy_normal* h, const double* fx, const double* w, double beta, const double* base,
                             double* values, double* seconds) {
    const char* who = "parsy_normal_values_host";
    if (parsy::normal_check_values_args(h, who, fx, values) != 0) return -1;
    PARSY_HIP(hipSetDevice(h->plan->device));
    Scratch sc;
    const int64_t nnz = h->I.nnzA;
    double* d_fx = sc.upload(fx, h->I.nnzF(), true);
    double* d_w = w ? sc.upload(w, h->I.m, true) : nullptr;
    double* d_v = sc.upload(base, nnz, base != nullptr);   // (in place: A0 and the result share the array)
    if (!d_fx || (w && !d_w) || !d_v || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (parsy_normal_values_device(h, d_fx, d_w, beta, base ? d_v : nullptr, d_v, nullptr) != 0) return -1;
    if (!sc.timer.stop(seconds) || (nnz > 0 && hipMemcpy(values, d_v, (size_t)nnz * 8, hipMemcpyDeviceToHost) != hipSuccess)) {
        set_last_error(std::string(who) + ": download failed");
        return -1;
    }
    return 0;
}

int parsy_normal_apply_host(parsy_normal* h, int op, const double* fx, const double* w, const double* x, int ldx, int nrhs,
                            double alpha, double beta, double* y, int ldy, double* seconds) {
    const char* who = "parsy_normal_apply_host";
    if (parsy::normal_check_apply_args(h, who, op, fx, x, ldx, nrhs, y, ldy) != 0) return -1;
    PARSY_HIP(hipSetDevice(h->plan->device));
    const int nx = op == PARSY_NORMAL_F ? h->I.m : h->I.n, ny = op == PARSY_NORMAL_F ? h->I.n : h->I.m;
    Scratch sc;
    double* d_fx = sc.upload(fx, h->I.nnzF(), true);
    double* d_w = w ? sc.upload(w, h->I.m, true) : nullptr;
    double* d_x = sc.upload(nullptr, (int64_t)nx * nrhs, false);
    double* d_y = sc.upload(nullptr, (int64_t)ny * nrhs, false);
    if (!d_fx || (w && !d_w) || !d_x || !d_y || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (nx > 0) PARSY_HIP(hipMemcpy2D(d_x, (size_t)nx * 8, x, (size_t)ldx * 8, (size_t)nx * 8, nrhs, hipMemcpyHostToDevice));
    if (ny > 0 && beta != 0.0)
        PARSY_HIP(hipMemcpy2D(d_y, (size_t)ny * 8, y, (size_t)ldy * 8, (size_t)ny * 8, nrhs, hipMemcpyHostToDevice));
    if (parsy_normal_apply_device(h, op, d_fx, d_w, d_x, std::max(nx, 1), nrhs, alpha, beta, d_y, std::max(ny, 1), nullptr) != 0)
        return -1;
    if (!sc.timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    if (ny > 0) PARSY_HIP(hipMemcpy2D(y, (size_t)ldy * 8, d_y, (size_t)ny * 8, (size_t)ny * 8, nrhs, hipMemcpyDeviceToHost));
    return 0;
}

int parsy_lsq_solve_host(parsy_normal* h, const double* fx, const double* w, double beta, const double* lValues,
                         const double* c, int ldc, double* x, int ldx, int nrhs, int steps, double* r, int ldr, double* g,
                         int ldg, double* seconds) {
    const char* who = "parsy_lsq_solve_host";
    if (parsy::normal_check_lsq_args(h, who, fx, lValues, c, ldc, x, ldx, nrhs, steps, r, ldr, g, ldg) != 0) return -1;
    parsy_plan* pl = h->plan;
    const int n = h->I.n, m = h->I.m;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, false, 0));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)pl->S.xsize * 8, hipMemcpyHostToDevice));
    Scratch sc;
    double* d_fx = sc.upload(fx, h->I.nnzF(), true);
    double* d_w = w ? sc.upload(w, m, true) : nullptr;
    double* d_c = sc.upload(nullptr, (int64_t)m * nrhs, false);
    double* d_x = sc.upload(nullptr, (int64_t)n * nrhs, false);
    double* d_r = r ? sc.upload(nullptr, (int64_t)m * nrhs, false) : nullptr;
    double* d_g = g ? sc.upload(nullptr, (int64_t)n * nrhs, false) : nullptr;
    if (!d_fx || (w && !d_w) || !d_c || !d_x || (r && !d_r) || (g && !d_g) || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (m > 0) PARSY_HIP(hipMemcpy2D(d_c, (size_t)m * 8, c, (size_t)ldc * 8, (size_t)m * 8, nrhs, hipMemcpyHostToDevice));
    if (parsy_lsq_solve_device(h, d_fx, d_w, beta, pl->h_L_dev.data(), d_c, std::max(m, 1), d_x, std::max(n, 1), nrhs, steps,
                               d_r, std::max(m, 1), d_g, std::max(n, 1), nullptr) != 0)
        return -1;
    if (!sc.timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    if (parsy_solve_status(pl) != 0) return -1;
    if (n > 0) PARSY_HIP(hipMemcpy2D(x, (size_t)ldx * 8, d_x, (size_t)n * 8, (size_t)n * 8, nrhs, hipMemcpyDeviceToHost));
    if (r && m > 0) PARSY_HIP(hipMemcpy2D(r, (size_t)ldr * 8, d_r, (size_t)m * 8, (size_t)m * 8, nrhs, hipMemcpyDeviceToHost));
    if (g && n > 0) PARSY_HIP(hipMemcpy2D(g, (size_t)ldg * 8, d_g, (size_t)n * 8, (size_t)n * 8, nrhs, hipMemcpyDeviceToHost));
    return 0;
}

// The factor goes through the plan's staging buffer like every solve's; B's values and the selected rows stage in
// buffers of their own, freed on return.
int parsy_solve_sparse_host(parsy_reach* h, const double* lValues, const double* bx, int op, double* x, int ldx,
                            double* seconds) {
    const char* who = "parsy_solve_sparse_host";
    if (parsy::reach_check_args(h, who, lValues, bx, op, x, ldx) != 0) return -1;
    parsy_plan* pl = h->plan;
    if (parsy::check_plan(pl, who, parsy::kNeedsDevice) != 0) return -1;
    const int nx = h->I.nx, nrhs = h->I.nrhs;
    const int64_t nnz = (int64_t)h->I.bcol.size();
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(stage(pl, false, 0));
    PARSY_HIP(hipMemcpy(pl->h_L_dev.data(), lValues, (size_t)pl->S.xsize * 8, hipMemcpyHostToDevice));
    Scratch sc;
    double* d_bx = sc.upload(bx, nnz, true);
    double* d_x = sc.upload(nullptr, (int64_t)nx * nrhs, false);
    if (!d_bx || !d_x || !sc.timer.start()) {
        set_last_error(std::string(who) + ": device buffers could not be made");
        return -1;
    }
    if (parsy_solve_sparse_device(h, pl->h_L_dev.data(), d_bx, op, d_x, nx, nullptr) != 0) return -1;
    if (!sc.timer.stop(seconds)) {
        set_last_error(std::string(who) + ": timing the call failed");
        return -1;
    }
    PARSY_HIP(hipMemcpy2D(x, (size_t)ldx * 8, d_x, (size_t)nx * 8, (size_t)nx * 8, nrhs, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
