"""The solve catalogue: which solve kernel meets which engineered border, under the componentwise measure.

A plain helper module of the suite in the style of shape_cases.py (no fixtures, no collection hooks).  Three parts:

* `SHAPES`: the shapes the cells work on -- entries of shape_cases.CASES by name, and new ones made for the borders of
  the solve kernels (a last chunk of fewer than four row blocks, rows one over the 128- and 256-row chunks, the staging
  limits of the ONE-launch kernels, the 512-row chunks of k_bsolve_below, levels of one width class only).  All have
  n <= 1000 and are analysed with shape_cases.ZRELAX.
* `predict`: the kernels a solve launches, from the launch tables of a host-only plan (parsy_debug_launches), the plan's
  counters and the gates -- the tests' independent copy of the library's dispatch (csrc/solve_route.cpp) -- so that
  test_solve_cases_host.py pins every cell to its path without a GPU.  test_solve_route_host.py compares it with the
  library's own route (`route`), test_solve_shapes_gpu.py holds both to the kernel witness, cell by cell.
* `CELLS`: name, shape, the variables read when the plan is built and those read per solve, the number of right-hand
  sides, the direction, the witness entries the cell must launch and those it must not, and the border it exists for.

The limit of every cell is shape_cases.limit(n) = n + 1 units of u for rho_solve of every column (shape_cases.py says
where it is from).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

import shape_cases as SC

# variables read when the plan is built / at the start of every solve; a test clears them all before it applies a cell's
PLAN_VARIABLES = ("PARSY_SOLVE_ONE", "PARSY_FORCE_UNFUSED", "PARSY_SUBTREES", "PARSY_SUB_TIER_MIN_TREES")
SOLVE_VARIABLES = ("PARSY_MRHS_MIN", "PARSY_BMRHS_MIN", "PARSY_BMRHS_WIDE_ONLY", "PARSY_BMRHS_WIDE_BLOCKS",
                   "PARSY_BCHAIN_MIN_BLOCKS", "PARSY_SMALL_MRHS_HALVES_MIN", "PARSY_SUB_MRHS_MIN", "PARSY_XT_MIN",
                   "PARSY_CHAIN_FEW_CHUNKS")
VARIABLES = tuple(SC.VARIABLES) + tuple(v for v in PLAN_VARIABLES + SOLVE_VARIABLES if v not in SC.VARIABLES)


# ---------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    name: str
    blocks: tuple
    border: int
    seed: int
    chain: object = False
    intent: str = ""

    @property
    def n(self) -> int:
        return sum(w for w, _ in self.blocks) + self.border


def _from_case(name):
    c = SC.CASE_BY_NAME[name]
    return Shape(name, c.blocks, c.border, c.seed, c.chain, c.intent)


_SUB_BLOCKS = SC.CASE_BY_NAME["subtrees"].blocks

SHAPES = {s.name: s for s in [
    *(_from_case(k) for k in ("narrow_lo", "narrow_hi", "cap_at", "cap_over", "tiles_70", "tiles_130", "tiles_257",
                               "dense_65", "dense_129", "dense_257", "chain", "subtrees")),
    Shape("wide_130", ((130, 170),), 171, 20, intent=
          "width 130 over 300 rows: the third row block holds the last diagonal block (2 columns) and 62 rows below it; "
          "the second 256-row chunk has one row block of 44 rows"),
    Shape("tall_65", ((65, 128), (65, 129), (65, 257)), 258, 21, intent=
          "width 65 (a second block column of one column) over 128, 129 and 257 rows: one over the 128-row chunks of "
          "k_solve_blocks_mrhs and one over two of them / the 256-row chunk of the chains"),
    Shape("below_512", ((65, 511), (65, 513)), 514, 22, intent=
          "width 65 over 511 and 513 rows: one under and one over kBelowRows (a second chunk of one row)"),
    Shape("one_stage", ((64, 55), (64, 56), (64, 57), (64, 63), (64, 64), (64, 65)), 66, 23, intent=
          "55 / 56 / 57 and 63 / 64 / 65 rows below blocks of width 64: both sides of OneStage (3584 and 4096 doubles at "
          "a row stride of rows | 1)"),
    Shape("one_rows", ((20, 255), (33, 256), (64, 257)), 258, 24, intent=
          "255 / 256 / 257 rows below: both sides of kOneRows"),
    Shape("tiny_only", ((1, 7), (2, 39), (15, 33), (16, 17), (16, 38), (9, 1)), 40, 25, intent=
          "a level of widths 1, 2, 9, 15, 16 only: the one-wave kernels' first width class"),
    Shape("narrow_32", ((31, 62), (32, 33), (17, 9), (16, 1), (1, 63), (32, 61)), 64, 26, intent=
          "a level of widths 1, 16, 17, 31, 32 only: the second width class (32) and its lower border"),
    Shape("mixed_257", ((17, 30), (33, 40), (64, 50), (65, 60)), 78, 27, intent=
          "n = 257 = 4 * 64 + 1: a last transpose tile of one row; narrow and wide supernodes"),
    Shape("subtrees_chain", _SUB_BLOCKS, 60, 28, chain=(0, 1, 2, 5, 7, 8, 9, 16, 17, 18, 21, 23, 24, 25, 32, 33, 34), intent=
          "the subtrees entry with runs of chained blocks: subtrees of up to five supernodes, ragged gathers"),
]}
assert all(s.n <= 1000 for s in SHAPES.values())

_BUILT = {}


def build(shape: Shape):
    """(A, S, sym) of a shape, made once per process and left unchanged."""
    from parsy_bench_amd import inspector as I
    if shape.name not in _BUILT:
        A, S = SC.arrow(shape.blocks, shape.border, shape.seed, shape.chain)
        _BUILT[shape.name] = (A, S, I.analyze(A, None, zrelax=SC.ZRELAX))
    return _BUILT[shape.name]


def engineered(shape: Shape):
    """The supernodes the shape is made to have, as (width, rows), the border last (test_updown_gpu._shaped)."""
    return SC.arrow_layout(shape.blocks, shape.border, shape.seed, shape.chain)[1]


def set_env(monkeypatch, env):
    for k in VARIABLES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------
# the prediction
# ---------------------------------------------------------------------------
# predict() is the tests' independent copy of the dispatch, which the library holds in one place, csrc/solve_route.cpp: a
# change to a gate or to a choice there is made here too (a comment there says so).  It cannot drift unnoticed:
# test_solve_route_host.py compares it with the library's route on every point of a grid without a GPU,
# test_solve_shapes_gpu.py holds it to the witness exactly, and test_solve_cases_host.py reads the field order of
# parsy::Launch and the defaults of SolveGates from the headers.
# parsy::Launch in declaration order (schedule.hpp)
LAUNCH_FIELDS = ("kind", "first", "count", "level", "side", "wait_level", "form", "rows_only", "ticket", "lds_bytes", "stage",
                 "width", "width_class", "task_first", "task_count")
KIND, FIRST, COUNT, LEVEL, SIDE, WAIT_LEVEL, FORM, ROWS_ONLY, TICKET, LDS_BYTES, STAGE, WIDTH, WIDTH_CLASS, TASK_FIRST, TASK_COUNT = range(len(LAUNCH_FIELDS))
# the defaults of SolveGates (solve_route.hpp) that _gates mirrors, by the struct's member names
GATE_DEFAULTS = {"mrhs_min": 6, "chain_mrhs_min": 2, "bmrhs_min": 16, "bmrhs_wide_blocks": 128, "bchain_min_blocks": 128,
                 "small_halves_min": 512, "sub_mrhs_min": 6, "xt_min": 16, "chain_few_chunks": 384}
BACK_BELOW, SOLVE_SMALL, SOLVE_PANEL, SOLVE_FIXUP, BACK_BLOCK = 4, 5, 6, 7, 8
EACH, CHAIN, SUBTREES = 0, 1, 2


def launch_tables(plan):
    """(forward, backward): the solve launches of a plan as rows of parsy::Launch's fields."""
    from parsy_bench_amd import _native as N
    lib = N.lib()
    lib.parsy_debug_launches.restype = C.c_int64
    lib.parsy_debug_launches.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    out = []
    for which in (1, 2):
        n = lib.parsy_debug_launches(plan._h, which, None, 0)
        t = np.zeros((n, 15), dtype=np.int32)
        assert lib.parsy_debug_launches(plan._h, which, t.ctypes.data, n) == n
        out.append(t)
    return out


def _names(call):
    """The witness names a route export returns: call(kernels, cap) -> number of launches."""
    from parsy_bench_amd import _native as N
    lib = N.lib()
    n = call(None, 0)
    assert n >= 0, N.last_error()
    k = np.zeros(max(n, 1), dtype=np.int32)
    assert call(k.ctypes.data, n) == n
    return [lib.parsy_debug_kernel_name(int(i)).decode() for i in k[:n]]


def route(plan, nrhs, ldx, forward):
    """The library's own route of a solve (parsy_debug_solve_route, a diagnostic outside the public header): the witness names
    of its launches in enqueue order, with the gates the environment sets now.  Plans without a device too."""
    from parsy_bench_amd import _native as N
    f = N.lib().parsy_debug_solve_route
    f.restype, f.argtypes = C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    return _names(lambda out, cap: f(plan._h, nrhs, ldx, 0 if forward else 1, out, cap))


def route_levels(plan, nrhs, ldx, forward, lev0, lev1, first, last):
    """... of one step of a solve in steps of levels (parsy_debug_solve_route_levels; the flags of parsy_solve_levels_device)."""
    from parsy_bench_amd import _native as N
    f = N.lib().parsy_debug_solve_route_levels
    f.restype, f.argtypes = C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    flags = (1 if first else 0) | (2 if last else 0) | (0 if forward else 4)
    return _names(lambda out, cap: f(plan._h, nrhs, ldx, lev0, lev1, flags, out, cap))


def _gates(env):
    d = GATE_DEFAULTS
    g = {"mrhs_min": d["mrhs_min"], "chain_mrhs_min": d["chain_mrhs_min"], "bmrhs_min": d["bmrhs_min"], "wide_only": True,
         "wide_blocks": d["bmrhs_wide_blocks"], "bchain": d["bchain_min_blocks"], "halves": d["small_halves_min"],
         "sub": d["sub_mrhs_min"], "xt": d["xt_min"], "xt_set": False, "few": d["chain_few_chunks"]}
    m = int(env.get("PARSY_MRHS_MIN", "0"))
    if m > 0:
        g["mrhs_min"], g["chain_mrhs_min"] = m, min(m, 2)
    for key, var in (("bmrhs_min", "PARSY_BMRHS_MIN"), ("wide_blocks", "PARSY_BMRHS_WIDE_BLOCKS"), ("bchain", "PARSY_BCHAIN_MIN_BLOCKS"),
                     ("halves", "PARSY_SMALL_MRHS_HALVES_MIN"), ("sub", "PARSY_SUB_MRHS_MIN"), ("xt", "PARSY_XT_MIN"),
                     ("few", "PARSY_CHAIN_FEW_CHUNKS")):
        if var in env:
            g[key] = int(env[var])
    g["wide_only"] = env.get("PARSY_BMRHS_WIDE_ONLY", "1")[0] != "0"
    g["xt_set"] = "PARSY_XT_MIN" in env
    return g


def predict(info, tables, plan_env, solve_env, nrhs, forward):
    """The witness entries a solve launches (a set), on the launch tables and counters of a plan built under plan_env."""
    g = _gates(solve_env)
    fwd_t, bwd_t = tables
    one = plan_env.get("PARSY_SOLVE_ONE")
    assert one in ("0", "2"), "a cell names its ONE-launch mode"
    size = "1" if nrhs == 1 else "4" if nrhs <= 4 else "8"
    out = set()
    sub_usable = info["sub_mrhs_tiers"] > 0 and g["sub"] > 0 and nrhs >= g["sub"]
    tier0 = info["solve_subtrees"]

    def small(row):
        w, count = int(row[WIDTH]), int(row[COUNT])
        if nrhs < g["mrhs_min"] and w <= 16:
            return "k_solve_tiny<16>"
        if nrhs < g["mrhs_min"]:
            return "k_solve_small"
        if w <= 16:
            return "k_solve_small_mrhs<16>"
        if w <= 32:
            return "k_solve_small_mrhs<32>"
        return "k_solve_small_mrhs<64,true>" if count >= g["halves"] or nrhs <= 32 else "k_solve_small_mrhs<64>"

    def back_block(row):
        cls, count, chain = int(row[WIDTH_CLASS]), int(row[COUNT]), row[FORM] == CHAIN
        if cls == 1 and nrhs >= g["bmrhs_min"]:
            return "k_bsolve_tiny_mrhs"
        if cls and nrhs < g["bmrhs_min"]:
            return "k_bsolve_tiny<16>" if cls == 1 else "k_bsolve_tiny<32>"
        if chain and nrhs > 16 and nrhs >= g["bmrhs_min"] and count >= g["bchain"]:
            return "k_bsolve_chain_mrhs"
        if nrhs >= g["bmrhs_min"] and (not g["wide_only"] or count >= g["wide_blocks"]):
            return "k_bsolve_block_mrhs<4>" if count >= g["wide_blocks"] and nrhs > 16 else "k_bsolve_block_mrhs<1>"
        return "k_bsolve_block<1>" if nrhs == 1 else "k_bsolve_block<4>"

    def run(row):
        kind, form = int(row[KIND]), int(row[FORM])
        if kind == SOLVE_SMALL:
            out.add("k_solve_sub_mrhs" if form == SUBTREES and sub_usable and tier0 == row[COUNT] else small(row))
        elif kind == SOLVE_PANEL:
            if form == CHAIN and nrhs >= g["chain_mrhs_min"]:
                out.add("k_solve_blocks_mrhs<true>" if nrhs <= 16 else "k_solve_blocks_mrhs<false>")
            elif form == CHAIN:
                out.add("k_solve_chain_w<2>" if row[COUNT] <= g["few"] else "k_solve_chain_w<4>")
            else:
                out.add("k_solve_panel")
        elif kind == SOLVE_FIXUP:
            out.add("k_solve_fixup")
        elif kind == BACK_BELOW:
            if nrhs == 1:
                out.add("k_bsolve_below")
        elif kind == BACK_BLOCK:
            if form == CHAIN and nrhs == 1:
                out.add("k_bsolve_chain_w")
            elif form == SUBTREES and sub_usable and tier0 == row[COUNT]:
                out.add("k_bsolve_sub_mrhs")
            else:
                out.add(back_block(row))

    table = fwd_t if forward else bwd_t
    takes_one = one == "2" and info["solve_one"] & (1 if forward else 2) and nrhs <= 8
    if takes_one:
        out.add(("k_solve_one<%s>" if forward else "k_bsolve_one<%s>") % size)
        if info["solve_one"] & 4 and len(table):
            run(table[0] if forward else table[-1])
        return out
    wide = any(r[KIND] == SOLVE_PANEL and r[FORM] == CHAIN for r in fwd_t)   # (solve_wide_list: the chain-form launches)
    fixup = any(r[KIND] == SOLVE_FIXUP for r in fwd_t)
    if wide:
        out.add("k_diag_inverse")
    if forward:
        if g["xt"] > 0 and nrhs >= g["xt"] and nrhs >= g["mrhs_min"] and not fixup and (info["xsize"] >= 150 * info["n"] or g["xt_set"]):
            out.add("k_transpose_x")
        if nrhs >= g["chain_mrhs_min"] and wide and not fixup:
            out.add("k_solve_arm_wide")
    elif nrhs > 1 and wide:
        out.add("k_solve_arm_wide")
    cover = info["sub_mrhs_cover_level"]
    if sub_usable and cover >= 0:
        out.add("k_solve_sub_mrhs" if forward else "k_bsolve_sub_mrhs")
        table = [r for r in table if r[FORM] != SUBTREES and r[LEVEL] > cover]
    for row in table:
        run(row)
    return out


# ---------------------------------------------------------------------------
# the cells
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Cell:
    name: str
    shape: str
    plan_env: dict
    solve_env: dict
    nrhs: int
    direction: str          # "forward" | "backward"
    kernels: tuple          # witness entries the cell must launch
    intent: str
    absent: tuple = ()      # ... and must not
    pair: str = ""          # the <4> / <2> cells of one shape: the other one's name (the two X agree normwise)

    @property
    def forward(self) -> bool:
        return self.direction == "forward"

    @property
    def plan_key(self):
        return (self.shape, tuple(sorted(self.plan_env.items())))


L0 = {"PARSY_SOLVE_ONE": "0"}           # level launches
ONE = {"PARSY_SOLVE_ONE": "2"}          # ONE launch per solve
UNFUSED = {**L0, "PARSY_FORCE_UNFUSED": "1"}
SUB0 = {**L0, "PARSY_SUBTREES": "1", "PARSY_SUB_TIER_MIN_TREES": "0"}
SUB2 = {**L0, "PARSY_SUBTREES": "1", "PARSY_SUB_TIER_MIN_TREES": "2"}
FWD, BWD = "forward", "backward"

NO_XT = {"PARSY_XT_MIN": "0"}           # X stays right-hand-side-major whatever the factor's density
XT6 = {"PARSY_XT_MIN": "6"}             # X row-major from 6 right-hand sides on
W4, W2 = "k_solve_chain_w<4>", "k_solve_chain_w<2>"
DINV = "k_diag_inverse"
M16, M32, M64, M64H = ("k_solve_small_mrhs<16>", "k_solve_small_mrhs<32>", "k_solve_small_mrhs<64>", "k_solve_small_mrhs<64,true>")
BN, BW = "k_solve_blocks_mrhs<true>", "k_solve_blocks_mrhs<false>"


def _pair(shape, intent, extra=()):
    """The forward one-right-hand-side chain of a shape through k_solve_chain_w<4> and through <2>: the same plan, the
    same right-hand side, PARSY_CHAIN_FEW_CHUNKS = 0 and 1000000."""
    a, b = f"w4_{shape}", f"w2_{shape}"
    return [Cell(a, shape, L0, {"PARSY_CHAIN_FEW_CHUNKS": "0"}, 1, FWD, (W4, DINV) + tuple(extra), intent, absent=(W2,), pair=b),
            Cell(b, shape, L0, {"PARSY_CHAIN_FEW_CHUNKS": "1000000"}, 1, FWD, (W2, DINV) + tuple(extra), intent, absent=(W4,), pair=a)]


CELLS = [
    # ---- k_solve_chain_w<4> and <2>: one right-hand side through the forward chain --------------------------------------
    *_pair("dense_65", "a second diagonal block of one column; <4>: one workgroup, two of its four row blocks past the panel"),
    *_pair("dense_129", "two full diagonal blocks hand over inside a workgroup (three in <4>), a third of one column"),
    *_pair("dense_257", "a second 256-row chunk of one row: <4> four diagonal blocks in one workgroup, the fifth polls the armed buffer"),
    *_pair("tiles_70", "widths 65 .. 129 over 1 .. 69 rows: last diagonal blocks of 1, 32, 63, 64 columns with rows below them in the same row block"),
    *_pair("tiles_130", "widths 191 .. 193 over up to 129 rows: chunks of 256 and 65 rows; a border of 130: a third block of 2 columns"),
    *_pair("tiles_257", "width 257 over 65 rows (a second chunk of 66 rows) and a chained pair: three levels of chain launches"),
    *_pair("cap_over", "a border of 400 columns under narrow tall supernodes: the chain's x comes from k_solve_small's atomics", ("k_solve_small",)),
    *_pair("wide_130", "width 130 over 300 rows: the row block of the last diagonal block (2 columns) holds 62 rows below it; a last chunk "
           "of one row block of 44 rows (<4>: three row blocks return at once)"),
    # ---- the width classes of the narrow kernels --------------------------------------------------------------------------
    Cell("tiny_f1", "tiny_only", L0, {}, 1, FWD, ("k_solve_tiny<16>", "k_solve_small"), "widths 1, 2, 9, 15, 16: one wave each; the border of 40 by a workgroup"),
    Cell("tiny_f32", "tiny_only", L0, NO_XT, 32, FWD, (M16, M64H), "widths <= 16 on the matrix cores: exactly two full fragments of 16 right-hand sides", absent=("k_solve_tiny<16>", "k_solve_small", M64)),
    Cell("tiny_f65", "tiny_only", L0, {}, 65, FWD, (M16, M64), "a second pass of one right-hand side", absent=(M64H,)),
    Cell("tiny_b1", "tiny_only", L0, {}, 1, BWD, ("k_bsolve_tiny<16>", "k_bsolve_block<1>"), "widths 1, 2, 9, 15, 16 backward: one wave each"),
    Cell("tiny_b9", "tiny_only", L0, {}, 9, BWD, ("k_bsolve_tiny<16>", "k_bsolve_block<4>"), "nine right-hand sides over eight lanes of passes: a lane takes two"),
    Cell("tiny_b65", "tiny_only", L0, {}, 65, BWD, ("k_bsolve_tiny_mrhs",), "a second lane of passes that holds one right-hand side", absent=("k_bsolve_tiny<16>",)),
    Cell("lo_f9", "narrow_lo", L0, {}, 9, FWD, (M32, M64H), "widths 15, 16, 17 in one launch of the 32 class; 9 right-hand sides"),
    Cell("lo_b5", "narrow_lo", L0, {}, 5, BWD, ("k_bsolve_tiny<32>", "k_bsolve_block<4>"), "widths 1 .. 17 in the second width class of the one-wave kernel"),
    Cell("n32_f32", "narrow_32", L0, NO_XT, 32, FWD, (M32, M64H), "widths 31 and 32, exactly two full fragments; the border of 64: the last count of the one-sweep kernel", absent=(M64,)),
    Cell("n32_f33", "narrow_32", L0, NO_XT, 33, FWD, (M32,), "widths 31 and 32 at the top of the 32 class; 33 right-hand sides: a third fragment of one; the border of 64 by the whole-sweep kernel", absent=(M64H,)),
    Cell("n32_b8", "narrow_32", L0, {}, 8, BWD, ("k_bsolve_tiny<32>",), "widths 31 and 32 by one wave; eight lanes of passes"),
    Cell("hi_f1", "narrow_hi", L0, {}, 1, FWD, ("k_solve_small",), "widths 31, 32, 33, 63, 64 by a workgroup each"),
    Cell("hi_f32", "narrow_hi", L0, NO_XT, 32, FWD, (M64H,), "32: the last count of the halves kernel in one sweep, widths 33, 63, 64", absent=(M64,)),
    Cell("hi_f33", "narrow_hi", L0, NO_XT, 33, FWD, (M64,), "33: the first count of the whole-sweep kernel", absent=(M64H,)),
    Cell("hi_f64", "narrow_hi", L0, NO_XT, 64, FWD, (M64,), "a full pass of 64 right-hand sides over widths 33, 63, 64", absent=(M64H,)),
    Cell("hi_f33_halves", "narrow_hi", L0, {**NO_XT, "PARSY_SMALL_MRHS_HALVES_MIN": "1"}, 33, FWD, (M64H,), "two halves, the second of one right-hand side", absent=(M64,)),
    Cell("hi_f65_halves", "narrow_hi", L0, {**NO_XT, "PARSY_SMALL_MRHS_HALVES_MIN": "1"}, 65, FWD, (M64H,), "two passes in halves, the second pass of one right-hand side", absent=(M64,)),
    Cell("hi_b17", "narrow_hi", L0, {"PARSY_BMRHS_WIDE_ONLY": "0"}, 17, BWD, ("k_bsolve_block_mrhs<1>",), "16 right-hand sides per pass: a second pass of one", absent=("k_bsolve_block<4>",)),
    Cell("hi_b65", "narrow_hi", L0, {"PARSY_BMRHS_WIDE_BLOCKS": "1"}, 65, BWD, ("k_bsolve_block_mrhs<4>",), "64 per pass: a second pass of one; widths 31 .. 64", absent=("k_bsolve_block_mrhs<1>", "k_bsolve_block<4>")),
    Cell("cap_f8", "cap_at", L0, {}, 8, FWD, (M64H, BN, "k_solve_arm_wide", DINV), "w * r == 6144: widths 64, 48, 32, 16 over 32 .. 368 rows below"),
    # ---- the chains with several right-hand sides -------------------------------------------------------------------------
    Cell("tall_f2", "tall_65", L0, {}, 2, FWD, (BN, "k_solve_arm_wide", DINV), "two right-hand sides; 128, 129 and 257 rows below: chunk tasks of 128, 128 + 1 and 2 * 128 + 1 rows", absent=(BW, W2, W4)),
    Cell("tall_f64", "tall_65", L0, NO_XT, 64, FWD, (BW,), "a full pass of exactly 64 right-hand sides through the wide chain, X right-hand-side-major", absent=(BN, "k_transpose_x")),
    Cell("tall_f17", "tall_65", L0, NO_XT, 17, FWD, (BW,), "17: the first count of the wide form, X right-hand-side-major", absent=(BN, "k_transpose_x")),
    Cell("tall_f65", "tall_65", L0, {}, 65, FWD, (BW, "k_transpose_x"), "a second pass of one right-hand side, X row-major (the default of a dense factor)"),
    Cell("tall_b1", "tall_65", L0, {}, 1, BWD, ("k_bsolve_chain_w", DINV), "pairs of block columns of 1 + 64 columns; 128 .. 257 rows below, under kBelowRows", absent=("k_bsolve_below",)),
    Cell("tall_b3", "tall_65", L0, {}, 3, BWD, ("k_bsolve_block<4>", "k_solve_arm_wide", DINV), "the chain form of the light kernel, three of four right-hand sides"),
    Cell("tall_b17", "tall_65", L0, {"PARSY_BCHAIN_MIN_BLOCKS": "1"}, 17, BWD, ("k_bsolve_chain_mrhs",), "17: the first count of the kernel; last block columns of one column"),
    Cell("tall_b65", "tall_65", L0, {"PARSY_BCHAIN_MIN_BLOCKS": "6", "PARSY_BMRHS_WIDE_ONLY": "0"}, 65, BWD, ("k_bsolve_chain_mrhs", "k_bsolve_block_mrhs<1>"),
         "the level of six block columns through the chain kernel, the border's five through k_bsolve_block_mrhs<1>: both in one solve"),
    Cell("t257_b33", "tiles_257", L0, {"PARSY_BMRHS_WIDE_BLOCKS": "1"}, 33, BWD, ("k_bsolve_block_mrhs<4>",), "the chain form, 64 per pass: 33 of them; a last block column of one column",
         absent=("k_bsolve_block_mrhs<1>", "k_bsolve_chain_mrhs")),
    # ---- X row-major ------------------------------------------------------------------------------------------------------
    Cell("xt_chain_6", "chain", L0, XT6, 6, FWD, ("k_transpose_x", M32, M64H, BN), "n = 408 = 6 * 64 + 24; six right-hand sides at a stride of 16: the gate of 6",
         absent=("k_solve_small", "k_solve_tiny<16>")),
    Cell("xt_chain_63", "chain", L0, XT6, 63, FWD, ("k_transpose_x", M64, BW), "63 of a stride of 64: one tile of right-hand sides, not full"),
    Cell("xt_257_16", "mixed_257", L0, XT6, 16, FWD, ("k_transpose_x", M64H, BN), "n = 4 * 64 + 1: a last tile of one row; a full stride of 16"),
    Cell("xt_257_65", "mixed_257", L0, XT6, 65, FWD, ("k_transpose_x", M64, BW), "a second tile of one right-hand side (stride 80) and a last tile of one row"),
    # ---- the ONE-launch kernels -------------------------------------------------------------------------------------------
    Cell("one_stage_f1", "one_stage", ONE, {}, 1, FWD, ("k_solve_one<1>",), "55 .. 65 rows below 64 columns: staged up to 63 rows (4096 doubles)"),
    Cell("one_stage_f8", "one_stage", ONE, {}, 8, FWD, ("k_solve_one<8>",), "eight: the stage of 3584 doubles, 55 rows staged and 56 not"),
    Cell("one_stage_b5", "one_stage", ONE, {}, 5, BWD, ("k_bsolve_one<8>",), "five of eight right-hand sides"),
    Cell("one_rows_f5", "one_rows", ONE, {}, 5, FWD, ("k_solve_one<8>",), "255 .. 257 rows below: never staged; five of eight right-hand sides"),
    Cell("one_rows_b1", "one_rows", ONE, {}, 1, BWD, ("k_bsolve_one<1>",), "255, 256, 257 rows below: both sides of kOneRows"),
    Cell("one_rows_b8", "one_rows", ONE, {}, 8, BWD, ("k_bsolve_one<8>",), "eight: x of 256 rows below is the whole of its LDS"),
    Cell("one_chain_f2", "chain", ONE, {}, 2, FWD, ("k_solve_one<4>",), "six levels, ragged gathers: a block pulls slots of several descendants"),
    Cell("one_chain_b4", "chain", ONE, {}, 4, BWD, ("k_bsolve_one<4>",), "the same tree from the root down"),
    # ---- k_bsolve_below ---------------------------------------------------------------------------------------------------
    Cell("below_b1", "below_512", L0, {}, 1, BWD, ("k_bsolve_below", "k_bsolve_chain_w"), "513 rows below: two chunks, the second of one row; 511: none, the chain streams them itself"),
    # ---- the launches per block column ------------------------------------------------------------------------------------
    Cell("unfused_t130_f3", "tiles_130", UNFUSED, {}, 3, FWD, ("k_solve_panel", "k_solve_fixup"), "three of four right-hand sides; chunks of 256 rows below every block column", absent=(BN, DINV)),
    Cell("unfused_chain_f1", "chain", UNFUSED, {}, 1, FWD, ("k_solve_panel", "k_solve_fixup", "k_solve_small"), "one right-hand side through a deep tree", absent=(W2, W4)),
    # ---- the subtree kernels ----------------------------------------------------------------------------------------------
    Cell("sub_f6", "subtrees", SUB0, {}, 6, FWD, ("k_solve_sub_mrhs", M64H), "40 subtrees of one supernode; six of 16 right-hand sides", absent=(M16,)),
    Cell("sub_b17", "subtrees", SUB0, {}, 17, BWD, ("k_bsolve_sub_mrhs",), "a second group of one right-hand side", absent=("k_bsolve_tiny_mrhs",)),
    Cell("subc_f16_xt", "subtrees_chain", SUB2, XT6, 16, FWD, ("k_solve_sub_mrhs", "k_transpose_x"), "two tiers cover every level; subtrees of several supernodes on X row-major", absent=(M16, M64H)),
    Cell("subc_b17", "subtrees_chain", SUB2, {}, 17, BWD, ("k_bsolve_sub_mrhs",), "both tiers backward, the border's tree first", absent=("k_bsolve_tiny_mrhs", "k_bsolve_block<4>")),
    Cell("subc_f17_level", "subtrees_chain", SUB0, {"PARSY_SUB_MRHS_MIN": "0"}, 17, FWD, (M16,), "the level kernel walks the subtrees' ranges", absent=("k_solve_sub_mrhs",)),
    Cell("subc_f1_level", "subtrees_chain", SUB0, {}, 1, FWD, ("k_solve_tiny<16>",), "one wave walks a subtree of several supernodes", absent=("k_solve_sub_mrhs",)),
    Cell("sub_b16_level", "subtrees", SUB0, {"PARSY_SUB_MRHS_MIN": "0"}, 16, BWD, ("k_bsolve_tiny_mrhs",), "the level kernel on the ranges; the gate of 16: one full fragment", absent=("k_bsolve_sub_mrhs", "k_bsolve_tiny<16>")),
    Cell("subc_b3_level", "subtrees_chain", SUB0, {"PARSY_SUB_MRHS_MIN": "0"}, 3, BWD, ("k_bsolve_tiny<16>",), "one wave walks a subtree from its root down", absent=("k_bsolve_sub_mrhs",)),
    # ---- b = L 1 ----------------------------------------------------------------------------------------------------------
    Cell("rhs_ones", "cap_over", L0, {}, 1, FWD, ("k_rhs_ones",), "parsy_rhs_ones_device: panels of 97 .. 400 rows over two workgroups each"),
]
CELL_BY_NAME = {c.name: c for c in CELLS}
assert len(CELL_BY_NAME) == len(CELLS)


def rhs(shape: Shape, nrhs: int) -> np.ndarray:
    """The right-hand sides of every cell of a shape with that many of them (both tiers take B from here)."""
    return np.random.default_rng(1000 * nrhs + shape.seed).standard_normal((shape.n, nrhs))


def values(shape: Shape, A, sym, scaled: bool) -> np.ndarray:
    """The plain values of a shape, or those of D A D (shape_cases.scaled_values, seed 100 + seed), in the factor's order."""
    return sym.permute_values(SC.scaled_values(A, 100 + shape.seed)) if scaled else sym.A2x


def dense(shape: Shape, S, sym, scaled: bool) -> np.ndarray:
    """The dense symmetric matrix the values belong to, permuted."""
    Sx = SC.scaled(S, 100 + shape.seed) if scaled else S
    return Sx[np.ix_(sym.Perm, sym.Perm)]
