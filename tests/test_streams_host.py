"""bsx_step_batch_streams / bsx_reset_streams on a box without a GPU: the library's real host code runs against tests/hip_stub/libhipstub.so (the LD_PRELOAD
interposer of tests/test_device_order.py: two pretend devices, every HIP call logged with the calling thread's current device), driven by
tests/hip_stub/drive_streams.py for a context on device 1 with the caller on device 0.  Asserted:
  * both calls return 0 on every route of the step (plain, YUYV + flip, no mask, YUYV in, own-blur background fused and two-pass, in place), every HIP call
    they make is on device 1, no handle crosses devices, and the caller's device is restored;
  * the ids reach the device through the pinned ring (host -> device copy), whose entries are reused behind their events (no host synchronisation);
  * each refusal — duplicate id, id out of range, negative id, n > n_streams, n < 0, a pending pipelined composite — returns BSX_EINVAL with a message that
    names the offending position and value, and enqueues no HIP call at all; n == 0 returns 0 and enqueues nothing."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, model_path

STUB_DIR = os.path.join(ROOT, "tests", "hip_stub")
STUB = os.path.join(STUB_DIR, "libhipstub.so")
BSX_EINVAL = -1


@pytest.fixture(scope="module")
def stub():
    from backscrub_amd import build
    build.build()
    src = os.path.join(STUB_DIR, "hip_stub.cpp")
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", STUB, src])
    return STUB


@pytest.fixture(scope="module")
def run(stub, tmp_path_factory):
    log = str(tmp_path_factory.mktemp("streams") / "hip.log")
    env = dict(os.environ, LD_PRELOAD=stub, BSX_STUB_LOG=log, BSX_STUB_NDEV="2")
    W, H, n = 640, 480, 4
    r = subprocess.run([sys.executable, os.path.join(STUB_DIR, "drive_streams.py"), model_path("lite"), str(W), str(H), str(n), "1"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "error" not in d, d
    lines = [l.split() for l in open(log).read().splitlines() if l.strip()]
    return d, lines


def _span(d, lines, key):
    a, b = d["calls"][key]["log"]
    return lines[a:b]


OK_CALLS = ["step", "step_subset", "step_yuyv_flip", "step_no_mask", "step_yuyv_in", "step_bgblur", "step_bgblur_flip", "step_in_place_flip", "reset"] + \
    ["step_ring_%d" % i for i in range(6)] + ["after_flush"]


def test_both_calls_run_on_the_contexts_device_only(run):
    d, lines = run
    for key in OK_CALLS:
        c = d["calls"][key]
        assert c["rc"] == 0, (key, c)
        assert c["caller_device"] == 0, "%s: the caller's device was not restored" % key
        span = _span(d, lines, key)
        affine = [l for l in span if l[0] == "affine"]
        assert affine, "%s enqueued nothing" % key
        off = [l for l in affine if int(l[2]) != 1]
        assert not off, "%s: HIP calls made while device 0 was current: %s" % (key, sorted({l[1] for l in off}))
        assert not [l for l in span if l[0] == "MISMATCH"], key
        apis = [l[1] for l in affine]
        assert "hipMemcpyAsync" in apis, "%s: the ids never went to the device" % key
        assert "hipEventRecord" in apis, "%s: the ring entry is not guarded by an event" % key
        assert "hipStreamSynchronize" not in apis and "hipDeviceSynchronize" not in apis, "%s synchronised the host" % key
    assert d["pipelined"] == [0, 0]


def test_the_id_ring_is_allocated_once_and_reused(run):
    d, lines = run
    first = [l[1] for l in _span(d, lines, "step") if l[0] == "affine"]
    assert "hipHostMalloc" in first and "hipEventCreateWithFlags" in first      # lazily, on the first call
    for key in OK_CALLS[1:]:
        apis = [l[1] for l in _span(d, lines, key) if l[0] == "affine"]
        assert "hipHostMalloc" not in apis, key
    for i in range(6):                     # more calls than ring entries: a reused entry is checked with hipEventQuery, never waited on with a sync
        apis = [l[1] for l in _span(d, lines, "step_ring_%d" % i) if l[0] == "affine"]
        assert "hipEventSynchronize" not in apis
    reused = [l[1] for k in ("step_ring_%d" % i for i in range(6)) for l in _span(d, lines, k) if l[0] == "affine"]
    assert "hipEventQuery" in reused


def test_reset_streams_is_one_launch(run):
    d, lines = run
    apis = [l[1] for l in _span(d, lines, "reset") if l[0] == "affine"]
    assert apis.count("hipLaunchKernel") == 1, apis


@pytest.mark.parametrize("key,words", [
    ("dup", ["ids[2] = 0", "repeats ids[0]"]),
    ("out_of_range", ["ids[1] = 4", "out of range"]),
    ("negative", ["ids[1] = -2", "out of range"]),
    ("too_many", ["n = 5", "exceeds", "4 streams"]),
    ("negative_n", ["n = -1", "negative"]),
    ("reset_dup", ["bsx_reset_streams", "ids[1] = 2", "repeats ids[0]"]),
    ("reset_out_of_range", ["bsx_reset_streams", "ids[0] = 7", "out of range"]),
    ("pending", ["pipelined composite is pending"]),
    ("reset_pending", ["pipelined composite is pending"]),
])
def test_refusals_name_the_offending_id_and_enqueue_nothing(run, key, words):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL, c
    for w in words:
        assert w in c["error"], (key, c["error"])
    assert _span(d, lines, key) == [], "%s: a refused call made HIP calls" % key
    assert c["caller_device"] == 0


@pytest.mark.parametrize("key", ["step_empty", "reset_empty"])
def test_an_empty_list_is_a_no_op(run, key):
    d, lines = run
    assert d["calls"][key]["rc"] == 0
    assert _span(d, lines, key) == []


def test_header_and_binding_agree_on_the_new_calls():
    from backscrub_amd import api
    names = {s[0] for s in api.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    for n in ("bsx_step_batch_streams", "bsx_reset_streams"):
        assert n in names and ("BSX_API int %s(" % n) in hdr
