"""The launch records of a plan (csrc/schedule.hpp: Launch).  Host only: no device.

tests/launch_record_check.cpp is compiled with schedule.cpp, inspector.cpp and gen.cpp as host C++ under the address and
undefined-behaviour sanitizers and run directly: plans that hold every launch kind and form are consistent, and a wrong
field planted in a record is reported by check_schedule with the launch's name.  The second test reads the launch table
(parsy_debug_launches, a diagnostic outside the public header) of host-only plans and compares it with the plan's counts.
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import problem
from parsy_bench_amd import _native as N

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "parsy_bench_amd" / "csrc"
FIELDS = ("kind", "first", "count", "level", "side", "wait_level", "form", "rows_only", "ticket", "lds_bytes", "stage",
          "width", "width_class", "task_first", "task_count")


def test_records_under_the_sanitizers(tmp_path):
    from parsy_bench_amd.build import _hipcc
    exe = tmp_path / "launch_record_check"
    # (the sanitizers are for the host compilation only: -Xarch_host keeps them off any device pass of the driver)
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-g", "-O0", f"-I{CSRC}", str(ROOT / "tests" / "launch_record_check.cpp"),
           *(str(CSRC / s) for s in ("schedule.cpp", "inspector.cpp", "gen.cpp")), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "launch_record:" in ran.stdout and "planted faults reported" in ran.stdout


@pytest.mark.parametrize("name", ["tiny2d", "small3d", "ex15"])
def test_launch_table_matches_the_plan(name):
    lib = N.lib()
    lib.parsy_debug_launches.restype = C.c_int64
    lib.parsy_debug_launches.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    A, perm, sym = problem(name)
    h = lib.parsy_plan_from_symbolic(sym._handle, -1)
    assert h, N.last_error()
    try:
        pi = N.PlanInfo()
        lib.parsy_plan_get_info(h, C.byref(pi))
        info = pi.as_dict()
        want = (info["chol_launches"] - 1, info["solve_launches"], info["backsolve_launches"])   # (- 1: the A scatter)
        kinds = ({0, 1, 2, 3, 9}, {5, 6, 7}, {4, 8})
        for which in range(3):
            n = lib.parsy_debug_launches(h, which, None, 0)
            assert n == want[which] and n > 0
            t = np.full((n, len(FIELDS)), -7, dtype=np.int32)
            assert lib.parsy_debug_launches(h, which, t.ctypes.data, n) == n
            col = dict(zip(FIELDS, t.T))
            assert set(col["kind"].tolist()) <= kinds[which]
            assert (col["first"] >= 0).all() and (col["count"] > 0).all()
            assert (col["first"].astype(np.int64) + col["count"] < 2 ** 31).all()
            assert ((col["level"] >= 0) & (col["level"] <= max(info["nlevels"], info["chol_levels"]) + 1)).all()
            assert np.isin(col["form"], (0, 1, 2)).all() and (col["wait_level"] >= -1).all()
            # a table shorter than the plan's is filled up to its capacity only
            short = np.full((n, len(FIELDS)), -7, dtype=np.int32)
            assert lib.parsy_debug_launches(h, which, short.ctypes.data, n - 1) == n
            assert (short[:n - 1] == t[:n - 1]).all() and (short[n - 1] == -7).all()
        assert lib.parsy_debug_launches(h, 3, None, 0) == -1
    finally:
        lib.parsy_plan_destroy(h)
