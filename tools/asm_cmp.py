"""Compare the gfx950 device code of two source trees kernel by kernel (no GPU needed): tools/asm_cmp.sh runs this.

asm_cmp.py TREE_A TREE_B WORKDIR
Every parsy_bench_amd/csrc/*.hip of both trees is compiled device-only with the flags of parsy_bench_amd/build.py.  Per
kernel symbol -- wherever in its tree it lives -- three things are compared: the function body (label to .Lfunc_end),
the .amdhsa_kernel descriptor and the kernel's entry of the amdgpu_metadata note (arguments, LDS, scratch, register
counts).  Only what depends on a function's position in its file is normalised: the ordinal in .LBB<n>_ / BB<n>_ /
.Lfunc_end<n> / .LJTI<n>_ (and the padding between a .LBB label and its comment, which has the ordinal's width) and the
numbers of .Ltmp labels.  Lines with the source-text hash (__hip_cuid_), .file and
.ident are dropped.  The other device symbols (functions that are no kernels, globals) are compared as sets of (kind,
symbol) over the whole tree: one that moves between files counts as unchanged, as a kernel does.  Where two files of a
tree define the same kernel (a template of a shared header), the first definition stands for it.
Exit status 0 only if no kernel is in one tree alone, none differs (between the trees, or between two files of one tree
that both define it) and those sets are equal.  A kernel whose body alone differs and holds the same normalised lines in
another order is marked as such (it still counts as different)."""
import difflib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

FLAGS = ["--offload-arch=gfx950", "-munsafe-fp-atomics", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
         "-I", "include", "--cuda-device-only", "-S"]
DROP = ("__hip_cuid_", ".file", ".ident")


def compile_tree(tree: Path, out: Path, hipcc: str):
    """-> {file name: (assembly lines or None when the compile failed, number of warnings)}"""
    out.mkdir(parents=True, exist_ok=True)
    sources = sorted((tree / "parsy_bench_amd" / "csrc").glob("*.hip"))

    def one(src):
        raw = out / (src.stem + ".s")
        r = subprocess.run([hipcc, *FLAGS, *os.environ.get("ASM_CMP_FLAGS", "").split(), str(src), "-o", str(raw)],
                           cwd=tree, capture_output=True, text=True)
        (out / (src.stem + ".warn")).write_text(r.stderr)
        if r.returncode != 0:
            return src.name, (None, 0)
        lines = [l for l in raw.read_text().split("\n") if not any(d in l for d in DROP)]
        return src.name, (lines, r.stderr.count("warning:"))

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(ex.map(one, sources))


def normalise(lines):
    tmp = {}
    out = []
    for l in lines:
        if re.match(r"\.LBB\d+_\d+:", l):   # (a label's comment is padded to a column: the padding has the ordinal's width)
            l = re.sub(r":\s+;", ": ;", l, count=1)
        l = re.sub(r"\.LBB\d+_", ".LBB#_", l)
        l = re.sub(r"\bBB\d+_", "BB#_", l)
        l = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#", l)
        l = re.sub(r"\.LJTI\d+_", ".LJTI#_", l)
        l = re.sub(r"\.Ltmp\d+", lambda m: tmp.setdefault(m.group(0), f".Ltmp#{len(tmp)}"), l)
        out.append(l)
    return out


def parse(lines):
    """-> ({kernel: {"body": [...], "descriptor": [...], "metadata": [...]}}, {(kind, symbol)} of everything else)"""
    types = {}
    for l in lines:
        m = re.match(r"\s*\.type\s+([^,\s]+),@(\w+)", l)
        if m:
            types[m.group(1)] = m.group(2)
    kernels = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            kernels[m.group(1)] = {"descriptor": [x.strip() for x in lines[i:j + 1]]}
            i = j
        i += 1
    for name, parts in kernels.items():
        start = next(k for k, l in enumerate(lines) if l.startswith(name + ":"))
        end = start
        while not re.match(r"\.Lfunc_end\d+:", lines[end]):
            end += 1
        parts["body"] = normalise(lines[start:end + 1])
        parts["metadata"] = []
    # the note: a YAML list of kernels, one "  - " item each, its keys sorted
    if any(".amdgpu_metadata" in l for l in lines):
        a = next(k for k, l in enumerate(lines) if l.strip() == ".amdgpu_metadata")
        b = next(k for k, l in enumerate(lines) if l.strip() == ".end_amdgpu_metadata")
        item = None
        for l in lines[a + 1:b]:
            if l.startswith("  - "):
                item = []
            elif not l.startswith("    "):
                item = None
            if item is not None:
                item.append(l)
                m = re.match(r"\s+\.name:\s+(\S+)$", l)
                if m and l.startswith("    .name:") and m.group(1) in kernels:
                    kernels[m.group(1)]["metadata"] = item
    others = {(kind, sym) for sym, kind in types.items() if sym not in kernels}
    return kernels, others


def main():
    tree_a, tree_b, work = Path(sys.argv[1]).resolve(), Path(sys.argv[2]).resolve(), Path(sys.argv[3])
    hipcc = os.environ.get("HIPCC") or "hipcc"
    rc = 0
    sides = {}
    for side, tree in (("A", tree_a), ("B", tree_b)):
        kernels, others, twice = {}, set(), []
        print(f"tree {side}: {tree}")
        for name, (lines, nwarn) in compile_tree(tree, work / side.lower(), hipcc).items():
            if lines is None:
                print(f"  {name}: compile failed (see {work / side.lower() / (Path(name).stem + '.warn')})")
                rc = 1
                continue
            ks, os_ = parse(lines)
            for k, parts in ks.items():
                # (a template kernel of a shared header is a weak definition in every source that launches it)
                if k in kernels and any(kernels[k][p] != parts[p] for p in ("body", "descriptor", "metadata")):
                    twice.append(k)
                kernels.setdefault(k, dict(parts, file=name))
            others |= {(kind, sym, name) for kind, sym in os_}
            print(f"  {name}: {len(ks)} kernels, {len(lines)} lines of assembly, {len(os_)} other device symbols, "
                  f"{nwarn} warnings")
        print(f"  total: {len(kernels)} kernels")
        if twice:
            print(f"  kernels whose definitions in two files of the tree differ: {sorted(twice)}")
            rc = 1
        sides[side] = (kernels, others)
    (ka, oa), (kb, ob) = sides["A"], sides["B"]
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    print(f"kernels only in A: {len(only_a)}" + "".join(f"\n  {k} ({ka[k]['file']})" for k in only_a))
    print(f"kernels only in B: {len(only_b)}" + "".join(f"\n  {k} ({kb[k]['file']})" for k in only_b))
    differ, same, moved = [], 0, {}
    for k in sorted(set(ka) & set(kb)):
        bad = [p for p in ("body", "descriptor", "metadata") if ka[k][p] != kb[k][p]]
        if bad:
            differ.append((k, bad))
        else:
            same += 1
        if ka[k]["file"] != kb[k]["file"]:
            moved.setdefault((ka[k]["file"], kb[k]["file"]), []).append(k)
    # (a body that differs alone, with the same lines in another order: nothing added or removed, labels included)
    reordered = [k for k, bad in differ if bad == ["body"] and sorted(ka[k]["body"]) == sorted(kb[k]["body"])]
    print(f"kernels that differ: {len(differ)}, of them same instructions in another order: {len(reordered)}")
    for k, bad in differ:
        print(f"  {k} ({ka[k]['file']} -> {kb[k]['file']}): {', '.join(bad)}" + (" (same lines, other order)" if k in reordered else ""))
        for p in bad:
            d = list(difflib.unified_diff(ka[k][p], kb[k][p], "A", "B", lineterm="", n=1))
            print("".join(f"\n    {x}" for x in d[:20])[1:])
    print(f"kernels identical (body, descriptor, metadata): {same}")
    for (fa, fb), ks in sorted(moved.items()):
        print(f"  moved {fa} -> {fb}: {len(ks)}")
    for side, o in (("A", oa), ("B", ob)):
        print(f"other device symbols of {side}: {len(o)}" + "".join(f"\n  {kind} {sym} ({f})" for kind, sym, f in sorted(o)))
    if {x[:2] for x in oa} != {x[:2] for x in ob}:
        print("other device symbols: DIFFERENT")
        rc = 1
    else:
        print("other device symbols: equal")
    if only_a or only_b or differ:
        rc = 1
    print("RESULT:", "identical" if rc == 0 else "DIFFERENT")
    return rc


if __name__ == "__main__":
    sys.exit(main())
