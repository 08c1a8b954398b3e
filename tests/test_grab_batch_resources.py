"""Compile-time resources and memory instructions of resize_bgr_batch_k, read from the gfx950 assembly hipcc emits without a GPU (as
tests/test_kernel_resources.py reads its kernels).  The kernel is byte work bound by its loads and stores: it must stay out of scratch and LDS, read its descriptor
with scalar loads (the descriptor index is the block's), reach memory through global — not flat — instructions although its pointers come out of a table, and
store a lane's four pixels as one three-dword store in the aligned form."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
ROW = re.compile(r"^(\S+)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)")
CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")


@pytest.fixture(scope="module")
def hipcc():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return HIPCC


def test_the_batch_resize_kernel_uses_no_scratch_and_no_lds(hipcc):
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(CSRC, "kernels_img.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    rows = {}
    for line in r.stdout.splitlines():
        m = ROW.match(line)
        if m and "resize_bgr_batch_k" in m.group(1):
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), lds=int(m.group(4)), scratch=int(m.group(5)))
    assert len(rows) == 1, "one instance of resize_bgr_batch_k is expected: %s" % list(rows)
    for name, row in rows.items():
        assert row["scratch"] == 0, "%s spills %d bytes" % (name, row["scratch"])
        assert row["lds"] == 0, "%s uses %d bytes of LDS" % (name, row["lds"])
        assert row["vgpr"] <= 64, "%s: %d registers — eight waves per SIMD need <= 64" % (name, row["vgpr"])


def test_the_batch_resize_kernel_reads_its_descriptor_as_scalars_and_memory_as_global(hipcc):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, "-I" + os.path.join(CSRC, "build"),
                            "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "kernels_img.hip")],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-1500:]
        lines = open(out).read().splitlines()
    start = [i for i, l in enumerate(lines) if re.match(r"^_ZN\S*resize_bgr_batch_k\S*:", l)]
    assert len(start) == 1, start
    body = []
    for l in lines[start[0]:]:
        body.append(l)
        if "s_endpgm" in l:
            break
    ops = [l.split()[0] for l in body if l.startswith("\t") and l.split()]
    assert not [o for o in ops if o.startswith("flat_")], "pointers read from the descriptor must be used as global pointers"
    assert not [o for o in ops if o.startswith("scratch_") or o.startswith("ds_")]
    # the 64-byte descriptor: scalar loads only (two s_load_dwordx8 or any split of them), no vector load of it followed by a broadcast
    assert sum(int(re.sub(r"\D", "", o[len("s_load_dword"):]) or 1) for o in ops if o.startswith("s_load_dword")) >= 16, [o for o in ops if o.startswith("s_load")]
    assert "v_readfirstlane_b32" not in ops
    assert "global_store_dwordx3" in ops, "the aligned form stores a lane's four pixels at once"
    assert "global_load_dwordx2" in ops, "sample_linear's one 8-byte load per source row"
