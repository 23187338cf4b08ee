"""Every wait inside a launch goes through csrc/device_wait.hpp: the 2 s bound, its cadence, the look at the status word
and the report are defined there and nowhere else.  Source text only (comments stripped); nothing is compiled.
"""
import re

from test_kernel_witness import CSRC, source_text

HEADER = "device_wait.hpp"
WAITERS = ["chol_kernels.hip", "trsv_bwd_kernels.hip", "trsv_kernels.hip"]   # the sources with a wait inside a launch
SOURCES = sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".hpp", ".cpp"))


def _files_with(pattern, text=source_text):
    return [p.name for p in SOURCES if re.search(pattern, text(p))]


def test_one_bound():
    assert _files_with(r"\bkWaitTicks\s*=") == [HEADER]
    assert re.search(r"constexpr unsigned long long kWaitTicks = 200000000ull;", source_text(CSRC / HEADER))
    # (the two constants it replaces: not even in a comment)
    assert _files_with(r"kSpinTicks|kSolveSpinTicks", text=lambda p: p.read_text()) == []


def test_the_rule_and_the_report_are_in_the_header_only():
    # no source compares a difference of the wall clock with anything (the stamp macros only store the clock)
    assert _files_with(r"wall_clock64\(\)\s*-\s*\w+\s*>") == [HEADER]
    stamp = "#define STAMP(i) do { if (threadIdx.x == 0) g_stamps[i] = wall_clock64(); } while (0)"
    assert not re.search(r"wall_clock64\(\)\s*-\s*\w+\s*>", stamp)
    # status < 0 is written by wait_failed() alone (an atomicMin of a failing column is another matter)
    assert _files_with(r"atomicMin\s*\([^;]*,\s*-1\s*\)") == [HEADER]
    assert len(re.findall(r"atomicMin\s*\(", source_text(CSRC / HEADER))) == 1
    for name in WAITERS:
        text = source_text(CSRC / name)
        assert "wait_failed(info)" in text, name
        assert not re.search(r"\b(gave_up|give_up|wait_lds)\s*=\s*\[", text), f"{name} has a wait lambda of its own"


def _includes(name, seen=None):
    seen = set() if seen is None else seen
    for inc in re.findall(r'#include\s*"([^"]+)"', source_text(CSRC / name)):
        if inc not in seen and (CSRC / inc).exists():
            seen.add(inc)
            _includes(inc, seen)
    return seen


def test_who_waits():
    for name in WAITERS:
        assert HEADER in _includes(name), name
    # a wait inside a launch sleeps between its polls: nobody else does (the other sources are ordered by the stream)
    assert _files_with(r"__builtin_amdgcn_s_sleep") == sorted(WAITERS + [HEADER])


def test_a_loop_that_sleeps_holds_a_budget():
    """Every sleep stands a few lines behind the check of a BoundedWait that ends its loop."""
    sleeps = 0
    for name in WAITERS + [HEADER]:
        lines = source_text(CSRC / name).split("\n")
        for i, line in enumerate(lines):
            if "__builtin_amdgcn_s_sleep" in line:
                sleeps += 1
                before = "\n".join(lines[max(0, i - 12):i])
                assert re.search(r"\.expired(_now)?\(", before), f"{name}:{i + 1}: a sleep without a budget"
        assert name == HEADER or "BoundedWait" in "\n".join(lines) or "wait_lds_counter" in "\n".join(lines), name
    assert sleeps >= 20, sleeps
