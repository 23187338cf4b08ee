"""The kernel witness (include/parsy_amd.h, diagnostics) without a GPU: its table names every factor and solve kernel of the
sources, so that a new kernel cannot land without an entry (and so without the GPU tier's coverage tests noticing it), and
every launch of such a kernel goes through launch_witnessed<kernel, entry> (csrc/launch.hpp) with its own entry."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "parsy_bench_amd" / "csrc"

SOLVE_SOURCES = "trsv*.hip"
FACTOR_SOURCES = "chol_kernels.hip"

# the table in its order (solve_route.hpp, PARSY_WITNESS_KERNELS): the solve kernel instantiations, then the factor kernels
SOLVE_ENTRIES = [
    "k_solve_tiny<16>", "k_solve_small", "k_solve_small_mrhs<16>", "k_solve_small_mrhs<32>", "k_solve_small_mrhs<64>",
    "k_solve_small_mrhs<64,true>", "k_solve_panel", "k_diag_inverse", "k_solve_chain_w<2>", "k_solve_chain_w<4>",
    "k_solve_blocks_mrhs<true>", "k_solve_blocks_mrhs<false>", "k_transpose_x", "k_solve_arm_wide", "k_solve_one<1>",
    "k_solve_one<4>", "k_solve_one<8>", "k_bsolve_one<1>", "k_bsolve_one<4>", "k_bsolve_one<8>", "k_bsolve_block<1>",
    "k_bsolve_block<4>", "k_bsolve_block_mrhs<1>", "k_bsolve_block_mrhs<4>", "k_bsolve_chain_mrhs", "k_bsolve_tiny<16>",
    "k_bsolve_tiny<32>", "k_bsolve_tiny_mrhs", "k_bsolve_below", "k_bsolve_chain_w", "k_solve_fixup", "k_rhs_ones",
    "k_copy_segments", "k_solve_sub_mrhs", "k_bsolve_sub_mrhs"]
FACTOR_ENTRIES = ["k_scatter_a", "k_chol_small", "k_chol_tiles", "k_chol_chain", "k_chol_chain_rows", "k_chol_big",
                  "k_chol_dense"]
SOLVE_LAUNCH_SITES = 35   # launch sites of the solve sources; each instantiation is launched at one site

HELPER = r"launch_witnessed<\s*(\w+)\s*(<[^<>]*>)?\s*,\s*(\w+)\s*>\s*\("
BARE = r"hipLaunchKernelGGL\(\s*\(?\s*(\w+)"


def source_text(path):
    """(comments stripped)"""
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", path.read_text(), flags=re.S)


def kernel_names(*patterns):
    """The names of every __global__ function of the sources that match (comments stripped); by default the solve and the
    factor sources."""
    names = set()
    for pattern in patterns or (SOLVE_SOURCES, FACTOR_SOURCES):
        for src in sorted(CSRC.glob(pattern)):
            names |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", source_text(src)))
    return names


def witness_idents():
    """entry name -> its identifier (solve_route.hpp)"""
    table = re.sub(r"//[^\n]*", "", (CSRC / "solve_route.hpp").read_text())
    return {name: "kW" + ident for ident, name in re.findall(r'X\((\w+),\s*"([^"]+)"\)', table)}


def launch_sites(pattern):
    """[(kernel instantiation as the table spells it, witness identifier)] of every launch_witnessed of the sources that
    match; the width classes kTinyWidth / kTinyWidth2 (schedule.hpp) resolved to their values."""
    widths = dict(re.findall(r"constexpr int (kTinyWidth2?) = (\d+);", (CSRC / "schedule.hpp").read_text()))
    assert set(widths) == {"kTinyWidth", "kTinyWidth2"}, widths
    sites = []
    for src in sorted(CSRC.glob(pattern)):
        for kernel, targs, ident in re.findall(HELPER, source_text(src)):
            targs = re.sub(r"\w+", lambda m: widths.get(m.group(0), m.group(0)), re.sub(r"\s+", "", targs))
            sites.append((kernel + targs, ident))
    return sites


def test_sources_have_solve_kernels():
    names = kernel_names(SOLVE_SOURCES)
    # (the full set: a move between the solve sources that loses a kernel or makes one fails here)
    assert names == {
        "k_solve_small", "k_solve_tiny", "k_solve_small_mrhs", "k_solve_panel", "k_solve_chain_w", "k_solve_blocks_mrhs",
        "k_solve_arm_wide", "k_solve_fixup", "k_solve_one", "k_bsolve_one", "k_bsolve_block", "k_bsolve_block_mrhs",
        "k_bsolve_chain_mrhs", "k_bsolve_tiny", "k_bsolve_tiny_mrhs", "k_bsolve_below", "k_bsolve_chain_w",
        "k_diag_inverse", "k_transpose_x", "k_rhs_ones", "k_copy_segments", "k_solve_sub_mrhs", "k_bsolve_sub_mrhs"}, names
    assert all(n.startswith("k_") for n in names), names
    assert names == {e.split("<")[0] for e in SOLVE_ENTRIES}
    # (each kernel in one source only)
    assert sum(len(kernel_names(src.name)) for src in CSRC.glob(SOLVE_SOURCES)) == len(names)


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
    assert not missing, f"kernels without a witness entry (solve_route.hpp, PARSY_WITNESS_KERNELS): {missing}"
    stale = sorted(bases - names)
    assert not stale, f"witness entries of no kernel in the sources: {stale}"


def test_every_launch_of_a_factor_kernel_bumps_its_entry():
    """Each launch of chol_kernels.hip is a launch_witnessed with the entry of its own kernel."""
    ident = witness_idents()
    launches = launch_sites(FACTOR_SOURCES)
    assert len(launches) == 7 and {k for k, _ in launches} == kernel_names(FACTOR_SOURCES), launches
    assert all(bump == ident[kernel] for kernel, bump in launches), launches


def test_every_launch_of_a_solve_kernel_bumps_its_entry():
    """Each launch of the solve sources is a launch_witnessed whose entry is the one named as the kernel INSTANTIATION
    launched there (k_bsolve_block<4> with kWBsolveBlock4); every solve entry of the table has a launch site."""
    ident = witness_idents()
    assert list(ident) == SOLVE_ENTRIES + FACTOR_ENTRIES
    launches = launch_sites(SOLVE_SOURCES)
    assert len(launches) == SOLVE_LAUNCH_SITES, launches
    assert sorted(k for k, _ in launches) == sorted(SOLVE_ENTRIES), launches
    assert len(SOLVE_ENTRIES) == 35
    assert all(bump == ident[kernel] for kernel, bump in launches), launches


def test_no_bare_launch_of_a_witnessed_kernel():
    """No source launches a kernel that has a witness entry but through the helper, and nothing but the helper bumps."""
    witnessed = {e.split("<")[0] for e in witness_idents()}
    assert witnessed == kernel_names()
    for src in sorted(CSRC.iterdir()):
        if src.suffix not in (".hip", ".hpp", ".cpp"):
            continue
        text = source_text(src)
        bare = set(re.findall(BARE, text)) & witnessed
        assert not bare, f"{src.name}: hipLaunchKernelGGL of {sorted(bare)} (use launch_witnessed)"
        assert "<<<" not in text, src.name
        if src.name not in ("launch.hpp", "witness.hip", "solve_route.hpp"):
            assert "witness_launch" not in text, f"{src.name}: witness_launch outside launch_witnessed"
    # (the helper itself: the bump, then the launch of its template argument)
    assert re.search(r"witness_launch\(W\);\s*hipLaunchKernelGGL\(Kernel,", source_text(CSRC / "launch.hpp"))


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
    assert list(seen) == SOLVE_ENTRIES + FACTOR_ENTRIES   # (keys and their order)
