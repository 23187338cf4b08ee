"""The interval cut of conflict domains whose members' rows differ (schedule.cpp: find_conflict_domains, interval_bounds)
on shapes made to order (window_cases.py), on host-only plans: every plan passes parsy_plan_check under PARSY_BIG_RECUT =
0, 1, 2 and 3 and multiplies the products the tile cut multiplies; the intervals, their tasks and the members' blocks in
them are the ones the construction says; the decision and its tail guard are pinned by the issued work of the model.

The model (schedule.hpp: kIssue*): a dense entry (k_chol_dense) issues 2.09 us per 8-wide k chunk whatever its window
holds, a ragged one (k_chol_big) 1.0 us + 0.06 us per 16 x 16 fragment per 16-wide chunk.  A window of at least 70 % of
128 x 128 counts as dense.
"""
import numpy as np
import pytest

import recut_cases as RC
import window_cases as WC
from parsy_bench_amd import api

F = {k: i for i, k in enumerate(WC.TASK_FIELDS)}
ALL_NAMES = WC.NAMES + RC.NAMES
_PLANS = {}


def _plan(monkeypatch, name, knob):
    """(plan, tasks, windows) per (case, knob), made once and never changed."""
    if (name, knob) not in _PLANS:
        case = WC.case_of(name)
        WC.set_env(monkeypatch, case, knob)
        A, S, sym = WC.build(case)
        plan = api.Plan(sym, -1)
        _PLANS[(name, knob)] = (plan, WC.big_tasks(plan), WC.big_windows(plan))
    return _PLANS[(name, knob)]


def _ns(K, m, n, dense):
    """Issued work of one entry by the model, in ns."""
    return -(-K // 8) * 2090 if dense else -(-K // 16) * (1000 + 60 * -(-m // 16) * -(-n // 16))


def _task_ns(tasks, wins):
    out = np.zeros(len(tasks), dtype=np.int64)
    for t, _, K, m, n, _, _, _, dense in wins.tolist():
        out[t] += _ns(K, m, n, dense)
    return out


def _blocks(wins, tasks, K):
    """(row0, col0, rows, columns, ia, ja) of the entries of the source of width K, in task order."""
    return [[int(tasks[t, F["row0"]]), int(tasks[t, F["col0"]]), m, n, ia, ja] for t, _, k, m, n, ia, ja, _, _ in wins.tolist() if k == K]


@pytest.mark.parametrize("knob", WC.KNOBS)
@pytest.mark.parametrize("name", ALL_NAMES)
def test_plan_is_consistent_under_every_knob(monkeypatch, name, knob):
    plan, tasks, wins = _plan(monkeypatch, name, knob)
    assert plan.check() == 0
    assert len(tasks) > 0 and tasks[:, F["entries"]].sum() == len(wins) <= plan.info["big_entries"]
    dom = tasks[:, F["domain"]]
    assert (dom >= 0).all()
    if knob == 0:
        assert not dom.any()
    if knob <= 1:
        assert not (dom >= WC.INTERVAL).any()
    # the products are the same whatever the cut: every pair (i, j), i >= j, of a source's rows x its rows among the
    # target's columns, once -- per (launch, source, K), against the tile cut's
    _, _, tile_wins = _plan(monkeypatch, name, 0)

    def pairs(w):
        out = {}
        for _, launch, K, m, n, ia, ja, src, _ in w.tolist():
            i, j = np.meshgrid(np.arange(ia, ia + m), np.arange(ja, ja + n), indexing="ij")
            out[(launch, src, K)] = out.get((launch, src, K), 0) + int((i >= j).sum())
        return out
    # (strips ride in their block's entry and are not listed as windows: compared without them on both sides)
    if plan.info["dense_strip_entries"] == 0 and _plan(monkeypatch, name, 0)[0].info["dense_strip_entries"] == 0:
        assert pairs(wins) == pairs(tile_wins)


@pytest.mark.parametrize("name", WC.NAMES)
def test_knob_1_leaves_domains_of_differing_rows_on_the_grid(monkeypatch, name):
    """No case here has a domain of one row set that gains from its own order: knob 1's plan is the tile cut's."""
    _, t0, w0 = _plan(monkeypatch, name, 0)
    _, t1, w1 = _plan(monkeypatch, name, 1)
    assert np.array_equal(t0, t1) and np.array_equal(w0, w1)


def test_nested_rows_make_one_interval(monkeypatch):
    """(a) A (K = 136: 9 chunks of 16, 17 of 8) has the 128 even rows of the 256-wide target, B (K = 72: 5 and 9) the 64
    rows = 0 mod 4.  Nobody receives a 129th row: one interval, one task -- A as a full block that straddles the diagonal
    (dense), B as a 64 x 64 window (ragged): 64 * 9 + 16 * 5 = 656 fragment-chunks.
    Tile cut: three tiles of a 64 x 64 window of A and a 32 x 32 one of B each: 3 * (9 * 1.96 + 5 * 1.24) = 71.52 us, the
    longest task 23.84 us.  Intervals: 17 * 2.09 + 5 * 1.96 = 45.33 us in one task: less work, taken with knob 3; a task
    longer than the tile cut's longest and than the launch's 71.52 / 512 us per slot: refused by the guard with knob 2."""
    _, tile, tile_wins = _plan(monkeypatch, "nested", 0)
    assert len(tile) == 3 and _task_ns(tile, tile_wins).tolist() == [23840, 23840, 23840]
    plan, cut, wins = _plan(monkeypatch, "nested", 3)
    assert len(cut) == 1 and cut[0, F["domain"]] == WC.INTERVAL + 1 and cut[0, [F["row0"], F["col0"]]].tolist() == [0, 0]
    assert cut[0, F["entries"]] == 2 and cut[0, F["dense"]] == 1 and cut[0, F["frag_chunks"]] == 64 * 9 + 16 * 5 == 656
    assert _blocks(wins, cut, 136) == [[0, 0, 128, 128, 0, 0]] and _blocks(wins, cut, 72) == [[0, 0, 64, 64, 0, 0]]
    assert wins[wins[:, 2] == 136][0, 8] == 1 and wins[wins[:, 2] == 72][0, 8] == 0
    assert _task_ns(cut, wins).tolist() == [45330] and 45330 < 71520 and 45330 > max(23840, 71520 // 512)
    assert plan.info["dense_tasks"] == 1
    _, guarded, guarded_wins = _plan(monkeypatch, "nested", 2)
    assert np.array_equal(guarded, tile) and np.array_equal(guarded_wins, tile_wins)


def test_the_guard_passes_where_a_tile_task_is_as_long(monkeypatch):
    """(e) The same rows where k_chol_dense takes every entry: a window costs a whole block whatever it holds, so a tile's
    task (A + B) issues what the one interval task issues, (17 + 9) * 2.09 = 54.34 us, and the tile cut has three of them:
    less work and no longer a task -- knob 2 takes the intervals."""
    _, tile, tile_wins = _plan(monkeypatch, "nested_all_dense", 0)
    assert _task_ns(tile, tile_wins).tolist() == [54340] * 3
    for knob in (2, 3):
        _, cut, wins = _plan(monkeypatch, "nested_all_dense", knob)
        assert len(cut) == 1 and cut[0, F["domain"]] == WC.INTERVAL + 1 and cut[0, F["entries"]] == cut[0, F["dense"]] == 2
        assert _task_ns(cut, wins).tolist() == [54340]


def test_a_boundary_off_the_grid(monkeypatch):
    """(b) A (K = 40) has rows 1, 4, 7, .. 433 of the 435-wide target, 145 of them: its 129th row, at position
    1 + 3 * 128 = 385, opens the second interval.  B (K = 48) has the 128 rows 100 .. 227, all before 385 and never a 129th.
    Interval 0 = [0, 385) holds a full block of each, interval 1 = [385, 435) A's last 17 rows: task (0, 0) holds both
    members, (1, 0) and (1, 1) hold A alone."""
    case = WC.CASE_BY_NAME["off_grid"]
    rows_a, rows_b = case.blocks[0][1], case.blocks[1][1]
    assert rows_a[128] == 385 and len(rows_a) == 145 and max(rows_b) < 385 and len(rows_b) == 128 and set(rows_a) & set(rows_b)
    plan, cut, wins = _plan(monkeypatch, "off_grid", 3)
    assert (cut[:, F["domain"]] == WC.INTERVAL + 1).all()
    assert cut[:, [F["row0"], F["col0"]]].tolist() == [[0, 0], [128, 0], [128, 128]] and cut[:, F["entries"]].tolist() == [2, 1, 1]
    assert _blocks(wins, cut, 40) == [[0, 0, 128, 128, 0, 0], [128, 0, 17, 128, 128, 0], [128, 128, 17, 17, 128, 128]]
    assert _blocks(wins, cut, 48) == [[0, 0, 128, 128, 0, 0]]
    # the tile cut had A in runs of 43, 42, 43 and 17 rows and B in runs of 28 and 100: ten tasks, none dense
    _, tile, _ = _plan(monkeypatch, "off_grid", 0)
    assert len(tile) == 10 and not tile[:, F["dense"]].any() and cut[:, F["dense"]].tolist() == [2, 0, 0]


def test_an_interval_ends_at_the_piece_end(monkeypatch):
    """(c) The 512-wide target is four pieces of 128 columns; A has every other row (64 per 128), B every fourth (32).  Into
    the first piece A has 256 rows: without the boundary at T.w = 128 the first interval would run to position 255 and
    hold 128 rows, 64 of them columns.  With it: [0, 128) = the columns, [128, 384) = 128 rows, [384, 512) = 64: tasks
    (0, 0), (1, 0), (2, 0), the middle one a 128 x 64 window of A and a 64 x 32 one of B where the tile cut had two tasks
    of 64 x 64 and 32 x 32.  The second piece (rows from 128 on) has its own domain and intervals: (0, 0), (1, 0).  The
    third and fourth gain nothing and stay on the grid."""
    plan, cut, wins = _plan(monkeypatch, "piece_end", 3)
    assert plan.info["n_pieces"] == 6
    of_sources = cut[:, F["launch"]] >> 1 == 0       # source level 0: A and B (NEXT into the first piece, PUSH into the rest)
    src = cut[of_sources]
    pieces = sorted(set(src[:, F["piece"]].tolist()))
    assert len(pieces) == 4
    by_piece = [src[src[:, F["piece"]] == p] for p in pieces]
    assert [(t[:, F["domain"]] >= WC.INTERVAL).all() for t in by_piece] == [True, True, False, False]
    assert not by_piece[2][:, F["domain"]].any() and not by_piece[3][:, F["domain"]].any()
    assert by_piece[0][:, [F["row0"], F["col0"]]].tolist() == [[0, 0], [128, 0], [256, 0]]
    assert by_piece[1][:, [F["row0"], F["col0"]]].tolist() == [[0, 0], [128, 0]]
    assert set(by_piece[0][:, F["domain"]].tolist()) == set(by_piece[1][:, F["domain"]].tolist()) == {WC.INTERVAL + 1}
    first = np.flatnonzero(of_sources & (cut[:, F["piece"]] == pieces[0]))
    in_first = wins[np.isin(wins[:, 0], first)]
    assert [r[2:7] for r in in_first.tolist()] == [[136, 64, 64, 0, 0], [72, 32, 32, 0, 0], [136, 128, 64, 64, 0], [72, 64, 32, 32, 0],
                                                   [136, 64, 64, 192, 0], [72, 32, 32, 96, 0]]
    # no window crosses the piece's end: columns are rows below T.w, and the rows of column interval 0 are those alone
    assert (in_first[:, 4] <= 64).all() and (in_first[in_first[:, 5] == 0][:, 3] <= 64).all()
    _, tile, _ = _plan(monkeypatch, "piece_end", 0)
    assert len(tile[(tile[:, F["launch"]] >> 1 == 0) & (tile[:, F["piece"]] == pieces[0])]) == 4


def test_a_chain_of_three_is_one_domain(monkeypatch):
    """(d) A has the rows = 0, 1 (mod 4), B = 1, 2, C = 2, 3: A and B share columns, B and C, A and C none -- one domain of
    three row sets, 128 rows each in 256 positions: one interval, one task of three full blocks in update order (the order
    of a tile's entries).  Tile cut 3 * 17 * 1.96 = 99.96 us in three tasks of 33.32; intervals (17 + 9 + 5) * 2.09 =
    64.79 us in one: knob 3 takes it, the guard of knob 2 refuses it."""
    _, tile, tile_wins = _plan(monkeypatch, "chain3", 0)
    assert len(tile) == 3 and (tile[:, F["entries"]] == 3).all() and _task_ns(tile, tile_wins).tolist() == [33320] * 3
    _, cut, wins = _plan(monkeypatch, "chain3", 3)
    assert len(cut) == 1 and cut[0, F["domain"]] == WC.INTERVAL + 1 and cut[0, F["entries"]] == cut[0, F["dense"]] == 3
    assert (wins[:, 3:7] == [128, 128, 0, 0]).all() and sorted(wins[:, 2].tolist()) == [40, 72, 136]
    assert wins[:, 2].tolist() == tile_wins[:3, 2].tolist() and wins[:, 7].tolist() == tile_wins[:3, 7].tolist()
    assert _task_ns(cut, wins).tolist() == [64790]
    _, guarded, guarded_wins = _plan(monkeypatch, "chain3", 2)
    assert np.array_equal(guarded, tile) and np.array_equal(guarded_wins, tile_wins)


def test_no_gain_keeps_the_tile_cut(monkeypatch):
    """recut_cases' "overlap" (the even rows and rows 0 .. 127 of a 256-wide target): the tile cut has B's full block and a
    64 x 64 window of A in its longest task, 9 * 2.09 + 9 * 1.96 = 36.45 us; one interval would hold both as full blocks,
    (17 + 9) * 2.09 = 54.34 us in one task.  Knob 2: the tile cut's plan, array for array."""
    _, tile, tile_wins = _plan(monkeypatch, "overlap", 0)
    assert _task_ns(tile, tile_wins).max() == 36450
    _, cut, wins = _plan(monkeypatch, "overlap", 2)
    assert np.array_equal(tile, cut) and np.array_equal(tile_wins, wins) and not cut[:, F["domain"]].any()
    _, forced, forced_wins = _plan(monkeypatch, "overlap", 3)
    assert len(forced) == 1 and _task_ns(forced, forced_wins).tolist() == [54340]
