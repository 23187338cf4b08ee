"""The kernel witness (include/parsy_amd.h, diagnostics) without a GPU: its table names every factor and solve kernel of the
sources, so that a new kernel cannot land without an entry (and so without the GPU tier's coverage tests noticing it)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "parsy_bench_amd" / "csrc"

SOLVE_SOURCES = "trsv*.hip"
FACTOR_SOURCES = "chol_kernels.hip"


def kernel_names(*patterns):
    """The names of every __global__ function of the sources that match (comments stripped); by default the solve and the
    factor sources."""
    names = set()
    for pattern in patterns or (SOLVE_SOURCES, FACTOR_SOURCES):
        for src in sorted(CSRC.glob(pattern)):
            text = re.sub(r"//[^\n]*|/\*.*?\*/", "", src.read_text(), flags=re.S)
            names |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", text))
    return names


def test_sources_have_solve_kernels():
    names = kernel_names(SOLVE_SOURCES)
    # (the parse itself: a few kernels every solve needs, and nothing that is not a kernel name)
    assert {"k_solve_small_mrhs", "k_bsolve_chain_mrhs", "k_solve_sub_mrhs", "k_transpose_x"} <= names
    assert all(n.startswith("k_") for n in names), names


def test_sources_have_factor_kernels():
    names = kernel_names(FACTOR_SOURCES)
    assert names == {"k_scatter_a", "k_chol_small", "k_chol_tiles", "k_chol_chain", "k_chol_chain_rows", "k_chol_big",
                     "k_chol_dense"}, names
    assert not names & kernel_names(SOLVE_SOURCES)


def test_every_solve_kernel_has_a_witness_entry():
    """(and every factor kernel: the name is from when the table held the solve kernels only)"""
    from parsy_bench_amd import api
    table = api.kernel_launches()
    assert len(table) == len(set(table)), "duplicate witness entries"
    bases = {name.split("<")[0] for name in table}
    names = kernel_names()
    missing = sorted(names - bases)
    assert not missing, f"kernels without a witness entry (kernels.hpp, PARSY_WITNESS_KERNELS): {missing}"
    stale = sorted(bases - names)
    assert not stale, f"witness entries of no kernel in the sources: {stale}"


def test_every_launch_of_a_factor_kernel_bumps_its_entry():
    """Each hipLaunchKernelGGL of chol_kernels.hip has the witness_launch of its own kernel right before it."""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", (CSRC / FACTOR_SOURCES).read_text(), flags=re.S)
    table = re.sub(r"//[^\n]*", "", (CSRC / "kernels.hpp").read_text())
    ident = {name: "kW" + ident for ident, name in re.findall(r'X\((\w+),\s*"(\w+)"\)', table)}
    launches = re.findall(r"(?:witness_launch\((\w+)\);\s*)?hipLaunchKernelGGL\(\s*(\w+)\s*,", text)
    assert len(launches) == 7 and {k for _, k in launches} == kernel_names(FACTOR_SOURCES), launches
    assert all(bump == ident[kernel] for bump, kernel in launches), launches


def test_witness_api_without_a_device():
    from parsy_bench_amd import _native as N, api
    lib = N.lib()
    count = lib.parsy_debug_kernel_count()
    assert count == len(api.kernel_launches()) > 0
    assert lib.parsy_debug_kernel_name(-1) is None and lib.parsy_debug_kernel_name(count) is None
    assert lib.parsy_debug_kernel_launches(count) == 0
    api.reset_kernel_launches()
    seen = api.kernel_launches()
    assert all(isinstance(v, int) and v == 0 for v in seen.values())
    assert "k_solve_small_mrhs<64,true>" in seen and "k_bsolve_block_mrhs<4>" in seen
    assert "k_chol_chain_rows" in seen and "k_scatter_a" in seen
