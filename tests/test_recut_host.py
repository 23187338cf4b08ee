"""Conflict domains of the BIG launches on shapes made to order (recut_cases.py), on host-only plans: every plan passes
parsy_plan_check with PARSY_BIG_RECUT on and off, the domains that are re-cut are the ones the construction says, and the
issued fragment-chunks are the counts derived from it.

Issued fragment-chunks (parsy_debug_big_tasks): per 16-wide k chunk of an entry the 16 x 16 fragments that are multiplied:
a dense entry (k_chol_dense) its whole 128 x 128 block = 64, and 8 per strip that rides with it; a ragged entry
(k_chol_big) ceil(rows / 16) * ceil(columns / 16).
"""
import numpy as np
import pytest

import recut_cases as RC
from parsy_bench_amd import api

F = {k: i for i, k in enumerate(RC.TASK_FIELDS)}


def _plan(monkeypatch, name, recut):
    case = RC.CASE_BY_NAME[name]
    RC.set_env(monkeypatch, case, recut)
    A, S, sym = RC.build(case)
    plan = api.Plan(sym, -1)
    return plan, RC.big_tasks(plan), RC.big_windows(plan)


@pytest.mark.parametrize("recut", [False, True], ids=["tile", "recut"])
@pytest.mark.parametrize("name", RC.NAMES)
def test_plan_is_consistent(monkeypatch, name, recut):
    plan, tasks, wins = _plan(monkeypatch, name, recut)
    assert plan.check() == 0
    # (big_entries counts the blocks as they are cut; a strip then rides in its block's entry)
    assert len(tasks) > 0 and tasks[:, F["entries"]].sum() == len(wins) <= plan.info["big_entries"]
    assert (len(wins) == plan.info["big_entries"]) == (plan.info["dense_strip_entries"] == 0)
    if not recut:
        assert not tasks[:, F["domain"]].any()
    # the products are the same whatever the cut: every pair (i, j), i >= j, of a source's rows x its rows among the
    # target's columns, once (the plan check holds the flop identity; here the windows themselves, per source)
    _, tile_tasks, tile_wins = _plan(monkeypatch, name, False)

    def pairs(w):
        out = {}
        for _, launch, K, m, n, ia, ja, src, _ in w.tolist():
            i, j = np.meshgrid(np.arange(ia, ia + m), np.arange(ja, ja + n), indexing="ij")
            out[(launch, src, K)] = out.get((launch, src, K), 0) + int((i >= j).sum())
        return out
    # (strips ride in their block's entry and are not listed as windows: compared without them on both sides)
    if plan.info["dense_strip_entries"] == 0:
        assert pairs(wins) == pairs(tile_wins)


def test_one_source_is_cut_in_its_own_order(monkeypatch):
    """(a) The source has 128 rows in the target, rows 0, 2, .. 254 of its 256, all of them columns of the target; K = 136
    is ceil(136 / 16) = 9 chunks of 16.
    Tile cut: a 128-row window of the target holds 64 of the source's rows, so the tiles (0, 0), (1, 0), (1, 1) hold one
    64 x 64 window each: 3 tasks x 4 * 4 fragments x 9 chunks = 432, all ragged (4096 entries are below the 70 % of
    128 x 128 at which a window counts as dense).
    Re-cut: the domain is the source alone, its index has 128 positions = one window: one task, one full 128 x 128 block
    that straddles the diagonal and is multiplied whole by k_chol_dense: 64 fragments x 9 chunks = 576.  More
    fragment-chunks, but less issued work at the measured rates (17 dense chunks of 8 k at 2.09 us = 35.5 us against
    27 ragged chunks of 16 k at 1.0 + 0.06 * 16 us = 52.9 us), which is what decides."""
    _, tile, _ = _plan(monkeypatch, "one_source", False)
    assert len(tile) == 3 and tile[:, F["frag_chunks"]].tolist() == [144, 144, 144] and not tile[:, F["dense"]].any()
    assert tile[:, F["frag_chunks"]].sum() == 3 * 16 * 9 == 432
    plan, cut, wins = _plan(monkeypatch, "one_source", True)
    assert len(cut) == 1 and cut[0, F["domain"]] == 1 and cut[0, [F["row0"], F["col0"]]].tolist() == [0, 0]
    assert cut[0, F["entries"]] == cut[0, F["dense"]] == 1 and wins[0, 2:7].tolist() == [136, 128, 128, 0, 0]
    assert cut[:, F["frag_chunks"]].sum() == 64 * 9 == 576
    assert plan.info["dense_tasks"] == 1 and plan.info["dense_entries"] == 1


def test_two_sources_with_the_same_rows_share_one_domain(monkeypatch):
    """(b) Two sources, K = 136 (9 chunks) and K = 72 (5 chunks), both on rows 0, 2, .. 254 of the target.
    Tile cut: 3 tiles x 2 sources x 16 fragments: 48 * (9 + 5) = 672, ragged.
    Re-cut: they share every column: one domain; both have the same 128 rows: one window, one task with one full block
    per member in update order, both dense: 64 * (9 + 5) = 896."""
    _, tile, _ = _plan(monkeypatch, "same_rows", False)
    assert len(tile) == 3 and tile[:, F["frag_chunks"]].sum() == 48 * (9 + 5) == 672 and not tile[:, F["dense"]].any()
    plan, cut, wins = _plan(monkeypatch, "same_rows", True)
    assert len(cut) == 1 and cut[0, F["domain"]] == 1 and cut[0, F["entries"]] == cut[0, F["dense"]] == 2
    assert cut[:, F["frag_chunks"]].sum() == 64 * (9 + 5) == 896
    assert sorted(wins[:, 2].tolist()) == [72, 136] and (wins[:, 3:7] == [128, 128, 0, 0]).all()
    _, _, tile_wins = _plan(monkeypatch, "same_rows", False)
    # update order: the members of the task come as the sources of a tile do
    assert wins[:, 2].tolist() == tile_wins[:2, 2].tolist()


def test_partial_overlap_keeps_the_tile_cut(monkeypatch):
    """(c) Rows 0, 2, .. 254 and rows 0 .. 127: they share the even columns below 128, so they are one domain, and their
    rows differ, so no window of one index names the same entries of L for both: the plan is the tile cut's."""
    _, tile, tile_wins = _plan(monkeypatch, "overlap", False)
    _, cut, wins = _plan(monkeypatch, "overlap", True)
    assert np.array_equal(tile, cut) and np.array_equal(tile_wins, wins) and not cut[:, F["domain"]].any()


def test_a_source_across_two_pieces(monkeypatch):
    """(d) The target is two pieces of 128 columns.  Into the first the source has 128 rows, 64 of them its columns: the
    re-cut makes one 128 x 64 window of two 64 x 64 ones (the same 8 * 4 fragments, half the chunks).  Into the second
    it has the last 64 rows: one 64 x 64 window either way -- nothing to gain, the tile cut stays.  The push from the first
    piece into the second has the identity map: its tile cut is its own row order already."""
    _, tile, _ = _plan(monkeypatch, "two_pieces", False)
    plan, cut, wins = _plan(monkeypatch, "two_pieces", True)
    assert plan.info["n_pieces"] == 3
    first = cut[cut[:, F["piece"]] == 1]
    assert len(first) == 1 and first[0, F["domain"]] == 1 and first[0, F["frag_chunks"]] == 8 * 4 * 9
    assert tile[tile[:, F["piece"]] == 1][:, F["frag_chunks"]].sum() == 2 * 16 * 9 and len(tile[tile[:, F["piece"]] == 1]) == 2
    assert np.array_equal(tile[tile[:, F["piece"]] == 2], cut[cut[:, F["piece"]] == 2]) and not cut[cut[:, F["piece"]] == 2][:, F["domain"]].any()
    assert [136, 128, 64, 0, 0] in wins[:, 2:7].tolist()


def test_remainders_of_5_16_and_17_rows(monkeypatch):
    """(e) Three sources on the rows = 0, 1, 2 (mod 3) of the target share no column: three domains of one launch and piece,
    inside the same tiles.  133 = 128 + 5 and 144 = 128 + 16 rows: the remainder is at most a strip (16), so its rows under
    the full block join that block's task and ride with it (64 + 8 fragments per chunk; the column strip lies above the
    diagonal), and the corner of the two remainders (one fragment) is a task of its own.  145 = 128 + 17: the remainder
    is a window like any other: three tasks of 8 * 8, 2 * 8 and 2 * 2 fragments."""
    plan, cut, wins = _plan(monkeypatch, "remainders", True)
    assert (cut[:, F["launch"]] == 0).all() and len(set(cut[:, F["piece"]].tolist())) == 1
    by_domain = {int(d): cut[cut[:, F["domain"]] == d] for d in sorted(set(cut[:, F["domain"]].tolist()))}
    assert list(by_domain) == [1, 2, 3]
    K = {int(d): sorted(set(wins[np.isin(wins[:, 0], np.flatnonzero(cut[:, F["domain"]] == d)), 2].tolist())) for d in by_domain}
    assert sorted(k for ks in K.values() for k in ks) == [40, 48, 56] and all(len(ks) == 1 for ks in K.values())
    rem = {40: 5, 48: 16, 56: 17}
    for d, t in by_domain.items():
        k = K[d][0]
        chunks = -(-k // 16)
        if rem[k] <= 16:
            assert t[:, [F["row0"], F["col0"]]].tolist() == [[0, 0], [128, 128]]
            assert t[:, F["entries"]].tolist() == [1, 1] and t[:, F["dense"]].tolist() == [1, 0]
            assert t[:, F["frag_chunks"]].tolist() == [chunks * (64 + 8), chunks * 1]
        else:
            assert t[:, [F["row0"], F["col0"]]].tolist() == [[0, 0], [128, 0], [128, 128]]
            assert t[:, F["frag_chunks"]].tolist() == [chunks * 64, chunks * 2 * 8, chunks * 2 * 2]
    assert plan.info["dense_strip_entries"] == 2
    _, tile, _ = _plan(monkeypatch, "remainders", False)
    assert len(tile) == 10 and (tile[:, F["entries"]] == 3).all()
