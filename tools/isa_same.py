#!/usr/bin/env python3
"""Is the gfx950 device code of the working tree the device code of another revision?  (cross-compiles; no GPU needed)

usage: python tools/isa_same.py <git-rev> [file.hip ...]        (default: the four kernel sources of libbsx)
       python tools/isa_same.py --dirs <dir-a> <dir-b>          every *.hip of the two directories, paired by name
       python tools/isa_same.py --dump-seg <dir>                fill <dir> with the graph-specialised segment modules of the tree this copy of the tool is in

Each file is compiled to assembly twice, from <git-rev> (its csrc/ and include/ extracted into a temporary directory) and from the working tree, with the flags
of tools/kernel_regs.sh.  Per file the sets of .amdhsa_kernel symbols must be equal, and for every symbol the text from its label to its .end_amdhsa_kernel
must be identical.  The comparison is per symbol because the order of the kernels in the file follows their first use in host code and may move; the number
of a function inside its file, which the compiler puts into local labels (.LBB12_3), is therefore taken out.  Prints the differing symbols; exit status 1 if any.

The four sources are what hipcc builds ahead of time.  The segment kernels that run are the ones hipRTC compiles for the loaded graph (gen_seg.cpp: bsx_seg_head,
_k2, _k3, _tail and, where the plan takes k3's per-frame form, bsx_seg_k3f), and their text exists only behind a built library.  For those:
    python tools/isa_same.py --dump-seg seg_here                         here, after build()
    bash tools/ab_worktree.sh <git-rev>                                  the other revision, built under _ab_old/
    python _ab_old/tools/isa_same.py --dump-seg seg_rev                  (a revision from before this mode: run this copy with BSX_ISA_TREE=_ab_old)
    python tools/isa_same.py --dirs seg_rev seg_here
--dump-seg writes api.model_seg_source() of the lite, full and mlkit fixture models, each with BSX_ACT16 unset and =1: six self-contained sources, lite.hip,
lite_act16.hip, ...  A file present in one directory only, and a symbol present in one file only (bsx_seg_k3f is in lite's modules and in no other), count as differences.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.environ.get("BSX_ISA_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = "backscrub_amd/csrc"
DEFAULT = [f"{CSRC}/kernels_{k}.hip" for k in ("img", "seg", "nn", "frame")]
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S"]


def assemble(src, out, include=()):
    r = subprocess.run([HIPCC, *FLAGS, *("-I" + d for d in include), "-o", out, src], stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
    return kernels(open(out).read())


def kernels(asm):
    """{symbol: text from its label to its .end_amdhsa_kernel}"""
    lines = asm.splitlines()
    label = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"([A-Za-z_$][\w$.]*):", l))}
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            text = "\n".join(lines[label[m.group(1)]:end + 1])
            out[m.group(1)] = re.sub(r"(\.L[A-Za-z_]+)\d+", r"\1", text)      # .LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end
    return out


def compare(pairs, name_a, name_b, tmp):
    """pairs: (title, (source, include dirs) of side a, the same of side b) — compiles every source, prints one line per pair and the differing symbols; their number"""
    bad = 0
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        jobs = [(t, pool.submit(assemble, a[0], os.path.join(tmp, f"a{i}.s"), a[1]), pool.submit(assemble, b[0], os.path.join(tmp, f"b{i}.s"), b[1]))
                for i, (t, a, b) in enumerate(pairs)]
        for t, ja, jb in jobs:
            a, b = ja.result(), jb.result()
            diff = sorted((a.keys() ^ b.keys()) | {k for k in a.keys() & b.keys() if a[k] != b[k]})
            print(f"{t}: {len(a)} kernels {name_a}, {len(b)} {name_b}, {len(diff)} differ")
            for k in diff:
                print("  " + (f"only {name_a}" if k not in b else f"only {name_b}" if k not in a else "differs") + ": " + k)
            bad += len(diff)
    return bad


def tree_source(tree, rel):
    src = os.path.join(tree, rel)
    return src, (os.path.dirname(src), os.path.join(tree, "include"))


def dump_seg(dst):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from backscrub_amd import api
    from conftest import model_path
    os.makedirs(dst, exist_ok=True)
    for key in ("lite", "full", "mlkit"):
        for act16 in (False, True):
            os.environ.pop("BSX_ACT16", None)
            if act16:
                os.environ["BSX_ACT16"] = "1"
            src = api.model_seg_source(model_path(key))
            assert src, "no segment kernels for " + key
            with open(os.path.join(dst, key + ("_act16" if act16 else "") + ".hip"), "w") as f:
                f.write(src)
    os.environ.pop("BSX_ACT16", None)
    print("six sources in " + dst)


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    if sys.argv[1] == "--dump-seg" and len(sys.argv) == 3:
        return dump_seg(sys.argv[2])
    with tempfile.TemporaryDirectory() as tmp:
        if sys.argv[1] == "--dirs" and len(sys.argv) == 4:
            da, db = sys.argv[2:]
            fa, fb = ({f for f in os.listdir(d) if f.endswith(".hip")} for d in (da, db))
            for f in sorted(fa ^ fb):
                print(f"{f}: only in {da if f in fa else db}")
            bad = len(fa ^ fb) + compare([(f, (os.path.join(da, f), ()), (os.path.join(db, f), ())) for f in sorted(fa & fb)], "in " + da, "in " + db, tmp)
        else:
            rev, files = sys.argv[1], sys.argv[2:] or DEFAULT
            other = os.path.join(tmp, "rev")
            os.mkdir(other)
            tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, stdout=subprocess.PIPE).stdout
            subprocess.run(["tar", "-x", "-C", other], input=tar, check=True)
            bad = compare([(f, tree_source(other, f), tree_source(ROOT, f)) for f in files], "at " + rev, "here", tmp)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
