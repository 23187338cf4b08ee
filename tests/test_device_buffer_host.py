"""csrc/device_buffer.hpp on its own: tests/device_buffer_check.cpp includes nothing else of the library, is compiled
as host C++ with the address and undefined-behaviour sanitizers and run directly.  It needs no device.

Two programs from the one source.  The first supplies the allocator at compile time as a counting malloc / free that
fails the k-th allocation on request (and aborts on a free of null) and checks growth, failure, the build-into-locals-
then-commit pattern of the ensure_* functions, moves and clear + destructor against the live-block count and the byte
meter; the sanitizer reports any double free or leak.  The second uses the header's own hipMalloc / hipFree pair on a
machine without a device: every allocation returns the error, owners and meter stay empty, and no owner calls hipFree.
"""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SOURCE = ROOT / "tests" / "device_buffer_check.cpp"


def _build_and_run(tmp_path, name, defines):
    from parsy_bench_amd.build import _hipcc
    hipcc = _hipcc()
    rocm = Path(os.environ.get("ROCM_PATH") or Path(hipcc).resolve().parents[1])
    exe = tmp_path / name
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{rocm / 'include'}",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
           f"-I{ROOT / 'parsy_bench_amd' / 'csrc'}", *defines, str(SOURCE), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "device_buffer:" in ran.stdout


def test_owners_against_a_counting_allocator(tmp_path):
    _build_and_run(tmp_path, "device_buffer_fake", [])


def test_owners_on_the_real_pair_without_a_device(tmp_path):
    _build_and_run(tmp_path, "device_buffer_real", ["-DCHECK_REAL_PAIR"])
