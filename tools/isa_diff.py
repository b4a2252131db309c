"""Compare the gfx950 assembly of two source trees, kernel by kernel (CPU only: it compiles, it runs nothing).

    python tools/isa_diff.py [--keep DIR] [--pool a.hip,b.hip] ... OLD_TREE NEW_TREE [unit.hip ...]
    (no unit named: every .hip unit of _build.py's SOURCES; --keep: leave each kernel's normalised text in DIR/<unit>/{old,new}/ to diff)

Each unit is compiled from both trees with the flags of openmatch_amd/_build.py plus `--cuda-device-only -S`.  Comments, the
.file / .ident lines and the per-compilation __hip_cuid_* symbol are stripped, and the ordinal of the function in its unit is taken out
of local labels (.LBB12_3 -> .LBB_3: templates are emitted in the order the host code first names them, which a change of host code
alone moves).  What is left is split at the kernel symbols -- from a kernel's label to its .size directive, which takes in its
.amdhsa_kernel block of register, scratch and LDS figures -- and the text of each kernel is compared for equality; nothing else is
looked at.  The unit's remaining text (metadata, symbol directives) is one more entry, "<rest>", compared as a sorted list of lines for
the same reason as the labels.  Exit status 0 when every entry of every unit is equal.

--pool: the kernels of the listed units are pooled on each side -- a unit a tree does not have adds nothing -- and matched by symbol, so
a kernel that moved between units is still compared (search.hip against search.hip + search_scan.hip: --pool search.hip,search_scan.hip).
The pooled units leave the unit list, and their "<rest>" entries, which a move is bound to change, are not compared.

A refactor of kernel code that claims "same code as before" is checked with
    git worktree add /tmp/parent HEAD~1 && python tools/isa_diff.py /tmp/parent .
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))


def _build_module():
    spec = importlib.util.spec_from_file_location("om_build", os.path.join(os.path.dirname(HERE), "openmatch_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _build_module()
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={B.ARCH}", "-x", "hip", "-Wno-unused-result"]      # build_native's


def assembly(tree, unit, out):
    src = os.path.join(tree, "openmatch_amd", "csrc", unit)
    r = subprocess.run([B._hipcc()] + FLAGS + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")
    with open(out) as f:
        return f.read()


def kernels(text):
    """{kernel symbol: its normalised text} and "<rest>": everything outside the kernels, lines sorted."""
    lines = []
    for ln in text.splitlines():
        ln = re.sub(r"\s*;.*$", "", ln).rstrip()
        ln = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end)\d+", r".\1", ln)
        if not ln or re.match(r"\s*\.(file|ident)\b", ln) or "__hip_cuid_" in ln:
            continue
        lines.append(ln)
    names = {m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m}
    parts, cur = {"<rest>": []}, "<rest>"
    for ln in lines:
        m = re.match(r"(\S+):$", ln)
        if m and m.group(1) in names:
            cur = m.group(1)
            parts[cur] = []
        parts[cur].append(ln)
        if cur != "<rest>" and re.match(r"\s*\.size\s+" + re.escape(cur) + r"\b", ln):
            cur = "<rest>"
    parts["<rest>"].sort()
    return {k: "\n".join(v) + "\n" for k, v in parts.items()}


def diff_unit(old, new, unit, tmp, keep):
    """unit: a file name, or a tuple of them to pool"""
    pool = unit if isinstance(unit, tuple) else None
    stem = "+".join(os.path.splitext(u)[0] for u in pool or [unit])
    sides = {}
    for side, tree in (("old", old), ("new", new)):
        sides[side] = {}
        for u in pool or [unit]:
            if pool and not os.path.exists(os.path.join(tree, "openmatch_amd", "csrc", u)):
                continue
            parts = kernels(assembly(tree, u, os.path.join(tmp, f"{os.path.splitext(u)[0]}.{side}.s")))
            if pool:
                del parts["<rest>"]
            sides[side].update(parts)
    unit = " + ".join(pool or [unit])
    if keep:
        for side, parts in sides.items():
            os.makedirs(os.path.join(keep, stem, side), exist_ok=True)
            for k, v in parts.items():
                with open(os.path.join(keep, stem, side, k.strip("<>") + ".s"), "w") as f:
                    f.write(v)
    a, b = sides["old"], sides["new"]
    return unit, [(k, "equal" if a.get(k) == b.get(k) else "only old" if k not in b else "only new" if k not in a else "DIFFERENT")
                  for k in sorted(set(a) | set(b))]


def main(argv):
    keep = None
    if argv[:1] == ["--keep"]:
        keep, argv = argv[1], argv[2:]
    pools = []
    while argv[:1] == ["--pool"]:
        pools.append(tuple(argv[1].split(",")))
        argv = argv[2:]
    if len(argv) < 2:
        print(__doc__)
        return 2
    old, new = argv[0], argv[1]
    pooled = {u for p in pools for u in p}
    units = [u for u in argv[2:] or [s for s in B.SOURCES if s.endswith(".hip")] if u not in pooled] + pools
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as ex:
        for unit, rows in ex.map(lambda u: diff_unit(old, new, u, tmp, keep), units):
            wrong = [(k, st) for k, st in rows if st != "equal"]
            bad += len(wrong)
            n_kernels = sum(1 for k, _ in rows if k != "<rest>")
            print(f"{unit}: {n_kernels} kernels, {len(rows) - len(wrong)} of {len(rows)} entries equal", flush=True)
            for k, st in wrong:
                print(f"  {st}: {k}")
    print("every kernel equal" if not bad else f"{bad} entries differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
