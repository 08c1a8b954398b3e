"""The batch step's host code on a box without a GPU: tools/step_trace.py drives libbsx.so's real host code under tests/hip_stub/libhipstub.so (an LD_PRELOAD
interposer that logs every HIP call with the kernel's name and geometry) for the three reference models and the synthetic DeepLab, at 640x480 and at 642x480
(width % 4 != 0: the tile kernel does not fuse, the step composites as separate passes and the pipeline refuses).  Asserted:
  * bsx_profile_batch times the launches bsx_step_batch makes — same kernels, geometry and order — followed by the one stand-alone blend, per iteration;
  * every refusal of every step entry point returns BSX_EINVAL, names its entry point and enqueues no HIP call — partial overlap with BSX_STEP_BGBLUR on the
    fused and the two-pass route and partial overlap in the id form included;
  * a refusal that follows another entry point's refusal reports its own reason, not the earlier message."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
BSX_EINVAL = -1
LAUNCH = ("hipLaunchKernel", "hipModuleLaunchKernel")


FUSED = "640x480"


@pytest.fixture(scope="module", params=[(m, g) for m in ("lite", "full", "mlkit", "deeplab") for g in (FUSED, "642x480")], ids=lambda p: "%s-%s" % p)
def traces(request):
    from backscrub_amd import build
    build.build()
    from tools import step_trace
    d = step_trace.trace_all(False, 4, only="^%s %s " % request.param)
    assert len(d) == 1, d.keys()
    return dict(list(d.values())[0], fused=request.param[1] == FUSED)


def _launches(trace):
    return [l for l in trace if l.split()[1] in LAUNCH]


def test_profile_times_the_steps_own_launches(traces):
    step = _launches(traces["step"]["trace"])
    prof = traces["profile"]
    assert prof["rc"] > 0 and step, (prof["rc"], prof["error"])
    if traces["fused"]:                                                         # the fused step, then the stand-alone blend of the same buffers
        blend = [l for l in _launches(prof["trace"]) if "blend" in l.split()[2].lower() and "mask" not in l.split()[2]][:1]
        assert len(blend) == 1
        per_iter = step + blend
    else:                                                                       # the unfused step ends with that blend itself
        assert "blend" in step[-1].split()[2].lower()
        per_iter = step
    assert _launches(prof["trace"]) == per_iter * 2                             # two iterations


REFUSALS = {
    "bsx_step_batch_ex": ["null_frames", "null_out", "null_bg", "n0", "n_too_big", "unknown_flag", "bgblur_even", "bgblur_33", "bgblur_in_place",
                          "partial_overlap", "partial_overlap_bgblur_fused", "partial_overlap_bgblur_two_pass", "partial_overlap_no_mask", "pending",
                          "unknown_flag_after_dup"],
    "bsx_step_batch_streams": ["dup", "out_of_range", "negative_id", "n_too_big", "negative_n", "null_ids", "unknown_flag", "null_bg", "partial_overlap",
                               "partial_overlap_bgblur", "pending"],
    "bsx_step_batch_vcam": ["null_frames", "no_mask", "unknown_flag", "bgblur_even", "zero_size", "odd_yuyv", "overlaps_frames", "overlaps_bg", "pending"],
    "bsx_step_batch_pipelined": ["bgblur", "in_place", "partial_overlap", "n_too_big", "null_bg", "unknown_flag", "unaligned", "bgblur_after_dup"],
}
PREFIX = {"bsx_step_batch_ex": "ex_", "bsx_step_batch_streams": "streams_", "bsx_step_batch_vcam": "vcam_", "bsx_step_batch_pipelined": "pipe_"}


def test_every_refusal_names_its_entry_point_and_enqueues_nothing(traces):
    refused = {fn: list(keys) for fn, keys in REFUSALS.items()}
    if traces["fused"]:
        pending = ["pending_process", "pending_step", "pending_profile"]
    else:                                                                       # the pipeline refuses a geometry its fused kernel does not take: nothing pends
        refused = {fn: [k for k in keys if k != "pending"] for fn, keys in refused.items()}
        refused["bsx_step_batch_pipelined"] += ["0", "1", "2"]
        pending = []
    for fn, keys in refused.items():
        for k in keys:
            c = traces[PREFIX[fn] + k]
            assert c["rc"] == BSX_EINVAL, (fn, k, c["rc"])
            assert c["error"].startswith("error: %s: " % fn), (fn, k, c["error"])
            assert c["trace"] == [], (fn, k, c["trace"])
    for k in pending:
        c = traces[k]
        assert c["rc"] == BSX_EINVAL and "pipelined composite is pending" in c["error"] and c["trace"] == [], (k, c)


def test_a_refusal_reports_its_own_reason(traces):
    assert "ids[2] = 0 repeats ids[0]" in traces["streams_dup"]["error"]
    assert "unsupported flags" in traces["ex_unknown_flag_after_dup"]["error"]
    assert "repeats" not in traces["pipe_bgblur_after_dup"]["error"]
    assert traces["pipe_bgblur_after_dup"]["error"].startswith("error: bsx_step_batch_pipelined: ")


def test_the_accepted_routes_still_run(traces):
    """the calls next to the refusals are accepted: in place (plain, with a flip, with YUYV), BGBLUR fused and two-pass, every vcam form"""
    for k in ("ex_in_place", "ex_in_place_flip", "ex_in_place_yuyv", "ex_bgblur25", "ex_bgblur1", "streams_bgblur25", "vcam_up", "vcam_per_tap", "vcam_capture",
              "step_after_refusals") + (("pipe_0", "pipe_1", "pipe_flush") if traces["fused"] else ()):
        assert traces[k]["rc"] == 0 and traces[k]["trace"], (k, traces[k]["error"])
