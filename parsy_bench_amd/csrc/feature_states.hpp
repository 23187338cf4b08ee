// The device states of the features whose host schedules are plain C++ (selinv.hpp, grad.hpp, apply.hpp, updown.hpp,
// rowmod.hpp, eigs.hpp, normal.hpp, reach.hpp: those headers are read by host-only translation units too, these structs own device memory).  A plan holds
// each only once one of the feature's device calls has run.
#pragma once
#include "apply.hpp"
#include "device_buffer.hpp"
#include "grad.hpp"
#include "normal.hpp"
#include "reach.hpp"
#include "rowmod.hpp"
#include "selinv.hpp"
#include "updown.hpp"

#include <vector>

namespace parsy {

// Device state of a plan (selinv_kernels.hip): made by the first selinv / logdet call.
struct SelinvState {
    explicit SelinvState(ByteMeter* plan) : meter(plan), diag_meter(plan) {}
    // parsy_selinv_info.device_bytes is the map's and the scratch's share (meter); the diagonal's arrays are counted in
    // the plan's figure only (diag_meter)
    ByteMeter meter, diag_meter;
    bool map_ready = false;          // set when the schedule and the whole map are on the device
    SelinvSchedule X;
    SelinvSplit sp;                  // (tiled_min < 0: the descriptors on the device are not those of a split)
    DevicePool map{&meter};
    int64_t *d_cb = nullptr, *d_mo = nullptr;
    int32_t* d_gmap = nullptr;
    SelinvBc* d_bcs = nullptr;
    int32_t* d_tasks = nullptr;
    int64_t task_cap = 0;            // (descriptor, tile) pairs d_tasks holds
    DeviceBuf<double> d_scr{&meter}; // level scratch: T, Y and partial slots (64 x 64 doubles each)
    bool used = false;               // a call has enqueued work that reads the descriptors / scratch
    // log-determinant and diagonal: per column the offset of its diagonal entry, the reduction's partials and result
    bool diag_ready = false;         // set when both arrays exist
    DevicePool diag{&diag_meter};
    int64_t* d_doff = nullptr;
    double* d_lpart = nullptr;       // kLogParts sums, kLogParts first bad columns (as doubles), then the result pair
    // buffers of parsy_selinv_host (capi_hostcalls.hip), plan-lifetime, not counted: Z and the diagonal
    DeviceBuf<double> h_z, h_diag;
};

struct GradState {
    explicit GradState(ByteMeter* plan) : meter(plan) {}
    ByteMeter meter;                 // parsy_grad_info.device_bytes: everything here, in the plan's figure too
    bool built = false;
    GradPattern P;                   // (row / col are released once they are on the device; offdiag stays)
    bool on_device = false;          // set when both arrays are on the device
    DevicePool pattern{&meter};
    int32_t *d_row = nullptr, *d_col = nullptr;
    DeviceBuf<double> ws{&meter};    // P lambda and P x with the right-hand sides of a row contiguous (2 n pitch doubles)
    DeviceBuf<double> tpart{&meter}; // partial sums and results of parsy_trace_inverse_device
    int last_lanes = 0;              // lanes per entry of the last sampled product (0: none yet, 1: the direct kernel)
};

struct ApplyState {
    explicit ApplyState(ByteMeter* plan) : meter(plan) {}
    ByteMeter meter;                  // parsy_apply_info.device_bytes: everything here, in the plan's figure too
    bool built = false;
    ApplyIndex I;                     // (pos and the layout are released once they are on the device; the counts stay)
    ApplyLayout A;
    int64_t ws_need = 0;              // apply_workspace_len
    int64_t n_l_tasks = 0, n_lt_tasks = 0;
    bool on_device = false;           // set when the five arrays are on the device
    DevicePool index{&meter};
    int64_t* d_ptr = nullptr;
    ApplyOcc* d_occ = nullptr;
    ApplyTaskL* d_l_tasks = nullptr;
    ApplyTaskLt* d_lt_tasks = nullptr;
    ApplyCol* d_col = nullptr;
    DeviceBuf<double> ws{&meter};     // T / partials + staged X of one block of columns
    DeviceBuf<double> sol{&meter};    // n x nrhs operand of the inverse operators
    int last_op = -1, last_launches = 0;
};

struct UpdownState {
    explicit UpdownState(ByteMeter* plan) : meter(plan) {}
    ByteMeter meter;                  // parsy_updown_info.device_bytes: everything here, in the plan's figure too
    bool on_device = false;           // set when the workspace, the table and the status word exist
    DevicePool fixed{&meter};
    double* d_w = nullptr;            // n x kUpdownBlock, the columns of a row contiguous; all zero between calls
    double* d_coef = nullptr;         // kUpdownTile x kUpdownBlock rotations of the block column under way
    int32_t* d_status = nullptr;      // smallest 1-based column whose pivot failed (INT_MAX: none)
    DeviceBuf<int32_t> pattern{&meter};   // of the block of W under way: rows, columns, positions in the caller's values
    DeviceBuf<int64_t> segs{&meter};      // the row lists of a path: prefix sums of their lengths, then their offsets in lR
    bool used = false;                // a call has enqueued work that writes the status word
    int path_supernodes = 0, last_launches = 0, last_k = 0, last_sign = 0;
    int64_t block_columns = 0, entries_touched = 0;
    std::vector<int64_t> walk_segs;   // host copy of segs for plan_updown_walk (lives until the next walk: its upload is asynchronous)
};

struct RowmodDesc {                   // a supernode of the row subtree as the kernels read it
    int64_t px, pi;                   // its panel in lValues, its row list in lR
    int32_t c0, r;                    // first column, rows
    int32_t ks, q;                    // columns that take part, position of p in the row list
};

struct RowmodState {
    explicit RowmodState(ByteMeter* plan) : meter(plan) {}
    ByteMeter meter;                  // parsy_rowmod_info.device_bytes: everything here, in the plan's figure too
    ApplyIndex I;                     // the transpose of the row lists (kept on the host: parsy_rowmod_reach reads it)
    bool built = false;
    bool on_device = false;           // set when the index and both workspaces exist
    DevicePool fixed{&meter};
    int64_t *d_ptr = nullptr, *d_pos = nullptr;   // the device copy of the index
    double* d_t = nullptr;            // one double per entry of lR; all zero between calls
    double* d_y = nullptr;            // n doubles; all zero between calls
    DeviceBuf<RowmodDesc> nodes{&meter};   // of the call under way: T(p) grouped by height
    DeviceBuf<int64_t> segs{&meter};       // prefix sums over T(p): of ks (k_rowdel_zero), of r (k_rowmod_clear)
    DeviceBuf<int32_t> ints{&meter};       // the panel launches' (supernode, first row) pairs; rows and positions of the column
    // of the last device call
    int last_op = 0, last_row = -1;   // 0: none yet, 1: delete, 2: add; the row in the factor's ordering
    int reach = 0, heights = 0, row_launches = 0, column_launches = 0, rotation_launches = 0;
    int64_t entries_read = 0, entries_walked = 0;
};

// Device state of the eigensolver (eigs.hpp, eigs_kernels.hip): made by the first parsy_eigs_device call, grown on demand.
struct EigsState {
    explicit EigsState(ByteMeter* plan) : meter(plan) {}
    ByteMeter meter;                  // parsy_eigs_info.device_bytes: everything here, in the plan's figure too
    DeviceBuf<double> vf_a{&meter};   // A's and M's values on the full symmetric pattern (RefineState's CSR), gathered once
    DeviceBuf<double> vf_m{&meter};   // per call
    DeviceBuf<double> basis{&meter};  // V, A V and (with an M) M V: n x max_basis each, leading dimension n
    DeviceBuf<double> blocks{&meter}; // kEigsBlocks scratch blocks of n x 16
    DeviceBuf<double> gram{&meter};   // the Gram kernel's partials, one p x q tile set per chunk of rows
    DeviceBuf<double> dense{&meter};  // the small matrices the kernels read or write (eigs.hpp: EigsDense)
    DeviceBuf<unsigned long long> part{&meter};   // partial maxima: kRefinePartials per column, two sets
    DeviceBuf<int> ctl{&meter};       // {unused, status of the solves} as refine_solve_enqueue folds it
    // of the last call
    int32_t iterations = 0, restarts = 0, nconv = 0, basis_cols = 0, dropped = 0;
    int64_t solve_columns = 0;
    // host side of the small dense work; each is read by an asynchronous upload and rewritten only behind a wait
    std::vector<double> h_g, h_s, h_st, h_theta, h_c1, h_c2, h_eta;
};

// Device state of a normal-matrix handle (normal.hpp, normal_kernels.hip): made by the handle's first device call.
struct NormalState {
    ByteMeter meter;                  // parsy_normal_info.device_bytes: everything here (a handle's memory is its own: not in
                                      // the plan's figure, the plan may be destroyed first)
    bool on_device = false;           // set when the whole index is on the device
    DevicePool index{&meter};
    int64_t *d_lptr = nullptr, *d_chunk_off = nullptr, *d_rptr = nullptr;
    int32_t *d_ta = nullptr, *d_tb = nullptr, *d_tk = nullptr, *d_chunk_len = nullptr, *d_fold_q = nullptr,
            *d_fold_ptr = nullptr, *d_fp = nullptr, *d_fi = nullptr, *d_rpos = nullptr, *d_rcol = nullptr;
    int32_t* d_cls[kNormalClasses] = {nullptr, nullptr, nullptr};
    uint8_t* d_diag = nullptr;
    double* d_part = nullptr;         // one partial per chunk
    int* d_perm = nullptr;            // the handle's ordering and its inverse (null: identity)
    int* d_inv = nullptr;
    int* d_ctl = nullptr;             // the folded status of the solves of a least-squares call
    DeviceBuf<double> ws{&meter};     // n x nrhs + m x nrhs of parsy_lsq_solve_device
};

// Device state of a sparse-solve handle (reach.hpp, sparse_solve_kernels.hip): made by the handle's first device call.
struct ReachState {
    ByteMeter meter;                  // parsy_reach_info.device_bytes: everything here (a handle's memory is its own: not in
                                      // the plan's figure)
    bool on_device = false;           // set when the index and the three workspaces exist
    DevicePool fixed{&meter};
    SparsePiece *d_fpieces = nullptr, *d_bpieces = nullptr;
    int32_t *d_fwork = nullptr, *d_bwork = nullptr, *d_cmap = nullptr, *d_bcol = nullptr, *d_bcomp = nullptr,
            *d_xcomp = nullptr;
    int64_t *d_gptr = nullptr, *d_gpos = nullptr;
    uint8_t *d_colmask = nullptr, *d_entmask = nullptr;
    // per block of kSparseBlock right-hand sides, the columns of a row contiguous; all zero between calls
    double* d_y = nullptr;            // ncomp rows: b, then y, then x in the compact numbering
    double* d_t = nullptr;            // nent rows: what the panels of F subtract from the rows below them
    double* d_p = nullptr;            // npart rows: the partials of the backward panels
    int last_op = -1, last_kernels = 0;   // of the last device call (-1: none yet)
};

}  // namespace parsy

// A handle: one plan, one pattern of B, one list of selected rows.  The plan is borrowed and must outlive every call of
// the handle.
struct parsy_reach {
    parsy_plan* plan = nullptr;
    int device = -1;                  // the plan's (kept: parsy_reach_destroy may run after the plan is gone)
    parsy::ReachIndex I;
    parsy::ReachState dev;
};

// A handle: one plan, one pattern of F.  The plan is borrowed and must outlive every device call of the handle.
struct parsy_normal {
    parsy_plan* plan = nullptr;
    int device = -1;                  // the plan's (kept: parsy_normal_destroy may run after the plan is gone)
    parsy::NormalIndex I;
    parsy::NormalState dev;
};
