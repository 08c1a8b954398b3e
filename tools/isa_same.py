#!/usr/bin/env python3
"""Is the gfx950 device code of the working tree the device code of another revision?  (cross-compiles; no GPU needed)

usage: python tools/isa_same.py <git-rev> [file.hip ...]        (default: the four kernel sources of libbsx)

Each file is compiled to assembly twice, from <git-rev> (its csrc/ and include/ extracted into a temporary directory) and from the working tree, with the flags
of tools/kernel_regs.sh.  Per file the sets of .amdhsa_kernel symbols must be equal, and for every symbol the text from its label to its .end_amdhsa_kernel
must be identical.  The comparison is per symbol because the order of the kernels in the file follows their first use in host code and may move; the number
of a function inside its file, which the compiler puts into local labels (.LBB12_3), is therefore taken out.  Prints the differing symbols; exit status 1 if any.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "backscrub_amd/csrc"
DEFAULT = [f"{CSRC}/kernels_{k}.hip" for k in ("img", "seg", "nn", "frame")]
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S"]


def assemble(tree, rel, out):
    src = os.path.join(tree, rel)
    r = subprocess.run([HIPCC, *FLAGS, "-I" + os.path.dirname(src), "-I" + os.path.join(tree, "include"), "-o", out, src], stderr=subprocess.PIPE, text=True)
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


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev, files = sys.argv[1], sys.argv[2:] or DEFAULT
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        other = os.path.join(tmp, "rev")
        os.mkdir(other)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", other], input=tar, check=True)
        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            jobs = [(f, pool.submit(assemble, other, f, os.path.join(tmp, f"a{i}.s")), pool.submit(assemble, ROOT, f, os.path.join(tmp, f"b{i}.s")))
                    for i, f in enumerate(files)]
            for f, ja, jb in jobs:
                a, b = ja.result(), jb.result()
                diff = sorted((a.keys() ^ b.keys()) | {k for k in a.keys() & b.keys() if a[k] != b[k]})
                print(f"{f}: {len(a)} kernels at {rev}, {len(b)} here, {len(diff)} differ")
                for k in diff:
                    print("  " + ("only at " + rev if k not in b else "only here" if k not in a else "differs") + ": " + k)
                bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
