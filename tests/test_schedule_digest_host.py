"""The digest of a whole schedule (csrc/schedule_digest.hpp: one hash per data member of parsy::Schedule).  Host only: no device.

tests/schedule_digest_check.cpp is compiled with schedule.cpp, inspector.cpp and gen.cpp as host C++ under the address and
undefined-behaviour sanitizers and run directly: build_schedule for 0, 32, 256 and 304 compute units (a host-only plan
passes 0 only), every plan consistent and equal in every field when built twice.  The other tests read the digest of
host-only plans (parsy_debug_schedule_digest, a diagnostic outside the public header; tools/schedule_digests.py).
No table of expected digests is kept here: schedules change on purpose, the tool compares two trees.
"""
import subprocess
import sys
from pathlib import Path

import pytest

from conftest import problem, shard_masks
from parsy_bench_amd import api

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "parsy_bench_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tools"))
import schedule_digests as SD   # noqa: E402

KNOBS = ("PARSY_BSOLVE_BELOW", "PARSY_SUBTREES", "PARSY_PIECE_WIDTH", "PARSY_BIG_MINK")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def test_digests_under_the_sanitizers(tmp_path):
    from parsy_bench_amd.build import _hipcc
    exe = tmp_path / "schedule_digest_check"
    # (the sanitizers are for the host compilation only: -Xarch_host keeps them off any device pass of the driver)
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-g", "-O0", f"-I{CSRC}", str(ROOT / "tests" / "schedule_digest_check.cpp"),
           *(str(CSRC / s) for s in ("schedule.cpp", "inspector.cpp", "gen.cpp")), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(exe), "--fields"], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    rows = [line.split("\t") for line in ran.stdout.splitlines()]
    assert all(len(r) == 3 and len(r[2]) == 16 for r in rows)
    plans = {r[0] for r in rows}
    assert plans == {f"check {g} cus={c}" for g in ("tiny2d", "mid3d", "nd24k") for c in (0, 32, 256, 304)}
    of = {(r[0], r[1]): r[2] for r in rows}
    assert len(of) == len(rows) and len(rows) % len(plans) == 0
    # the device's size reaches the schedule: the walker batch everywhere, the subtrees where there are any
    assert of["check tiny2d cus=32", "walker_batch"] != of["check tiny2d cus=256", "walker_batch"]
    # (32 units: a sixteenth of the members needed, an eighth of the subtrees aimed at)
    assert any(of["check nd24k cus=32", f] != of["check nd24k cus=304", f] for f in ("chol_subtree", "solve_subtree"))
    # ... and 0 stands for 256 units in everything but the walker batch (64 at both)
    assert all(of["check nd24k cus=0", r[1]] == r[2] for r in rows if r[0] == "check nd24k cus=256")


def test_the_same_plan_twice_gives_equal_digests():
    A, perm, sym = problem("mid3d")
    first, second = api.Plan(sym, -1), api.Plan(sym, -1)
    a, b = SD.digest(first._h), SD.digest(second._h)
    names = [f for f, _ in a]
    assert len(names) == len(set(names)) > 100 and {"wave_entries", "split_ranges", "one_b.member", "level_of"} <= set(names)
    assert a == b


def test_a_backward_solve_knob_moves_backward_solve_fields_only(monkeypatch):
    """PARSY_BSOLVE_BELOW=2 on mid3d (rows below every wide supernode go to BACK_BELOW launches): the chain's groups name
    their slots (bsolve_pairs), the BACK_BELOW tasks and launches appear, their slots are counted -- nothing else moves."""
    A, perm, sym = problem("mid3d")
    plan = api.Plan(sym, -1)
    base = dict(SD.digest(plan._h))
    monkeypatch.setenv("PARSY_BSOLVE_BELOW", "2")
    plan = api.Plan(sym, -1)
    below = dict(SD.digest(plan._h))
    assert {f for f in base if base[f] != below[f]} == {"bsolve_pairs", "bsolve_below", "n_bpart_slots", "bsolve"}


@pytest.mark.parametrize("env", [{}, {"PARSY_SUBTREES": "2", "PARSY_PIECE_WIDTH": "128", "PARSY_BIG_MINK": "32"}])
def test_a_mask_taken_off_restores_every_field(monkeypatch, env):
    """Supernode masks (2 and 3 ranks) and piece masks on lap30 -- as it comes, and with subtrees, pieces and BIG launches
    forced, so that every launch-side list exists: a mask moves launch-side fields, and the plan without the mask is the
    plan as it was built, in every field."""
    A, perm, sym = problem("lap30")
    masks = shard_masks(sym, 2) + shard_masks(sym, 3)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = api.Plan(sym, -1)
    built = SD.digest(plan._h)
    for mask in masks:
        plan.set_active(mask)
        masked = dict(SD.digest(plan._h))
        assert masked["active"] != dict(built)["active"] and masked["wave_entries"] == dict(built)["wave_entries"]
        plan.set_active(None)
        assert SD.digest(plan._h) == built
    D = api.Dist(plan, 3)
    for rank in range(3):
        plan.set_active_pieces(D.mask(rank))
        assert dict(SD.digest(plan._h))["active_piece"] != dict(built)["active_piece"]
        plan.set_active_pieces(None)
        assert SD.digest(plan._h) == built
