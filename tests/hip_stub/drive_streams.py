"""Runs UNDER LD_PRELOAD=libhipstub.so (tests/test_streams_host.py starts it): drives bsx_step_batch_streams / bsx_reset_streams of libbsx.so for a context on
device 1 while the caller's current device is 0, through the library's real host code — every route of the step, the refusals, and n == 0.  No torch, no GPU.
Prints one JSON line: per call its return code, bsx_last_error, the caller's device afterwards and the span [first, last) of the HIP call log it produced."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from backscrub_amd import api  # noqa: E402  (module import only: api.lib() would pull torch in)


def load():
    L = C.CDLL(api.lib_path())
    for name, res, args in api.SYMBOLS:
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def log_lines():
    p = os.environ["BSX_STUB_LOG"]
    return len(open(p).read().splitlines()) if os.path.exists(p) else 0


def main():
    model, W, H, n, dev = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    stub = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhipstub.so"))
    L = load()
    msgs = []
    dbg = api.DEBUG_FN(lambda c, m: msgs.append(m.decode(errors="replace")))
    ctx = L.bsx_new(model.encode(), 2, W, H, n, dev, dbg, api.STAGE_FN(), api.STAGE_FN(), api.STAGE_FN(), None)
    if not ctx:
        print(json.dumps({"error": "bsx_new failed: %s" % msgs}))
        return
    # "device" buffers are host memory under the stub
    frames = np.zeros((n, H, W, 3), np.uint8)
    frames2 = np.zeros((n, H, W, 2), np.uint8)
    bg = np.zeros((H, W, 3), np.uint8)
    out = np.zeros((n, H, W, 3), np.uint8)
    out2 = np.zeros((n, H, W, 2), np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    calls = {}

    def run(key, fn):
        first = log_lines()
        rc = fn()
        err = (L.bsx_last_error(ctx) or b"").decode(errors="replace").strip()
        calls[key] = {"rc": rc, "error": err, "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()]}

    def ids(*v):
        return (C.c_int * max(len(v), 1))(*v), len(v)

    def step(key, id_list, flags=0, fr=frames, o=out, b=bg, nn=None):
        a, k = ids(*id_list)
        run(key, lambda: L.bsx_step_batch_streams(ctx, a, p(fr), p(b) if b is not None else None, 0, p(o), k if nn is None else nn, None, flags))

    perm = list(range(n))[::-1]
    # every route of the step with a permutation of the streams, then a subset, then resets
    step("step", perm)
    step("step_subset", [n - 1, 0])
    step("step_yuyv_flip", perm, 1 | 2, o=out2)
    step("step_no_mask", perm, 8)
    step("step_yuyv_in", perm, 16 | 1, fr=frames2, o=out2)
    step("step_bgblur", perm, 25 << 8, b=None)
    step("step_bgblur_flip", perm, (25 << 8) | 4, b=None)
    step("step_in_place_flip", perm, 2, o=frames)
    for i in range(6):                                   # more calls than the ring has entries: entries are reused behind their events
        step("step_ring_%d" % i, [i % n])
    a, k = ids(1, 0)
    run("reset", lambda: L.bsx_reset_streams(ctx, a, k, None))
    # n == 0: nothing happens, nothing is enqueued
    step("step_empty", [])
    run("reset_empty", lambda: L.bsx_reset_streams(ctx, None, 0, None))
    # refusals: validated on the host before anything is enqueued
    step("dup", [0, 1, 0])
    step("out_of_range", [0, n])
    step("negative", [1, -2])
    step("too_many", list(range(n)) + [0], nn=n + 1)
    step("negative_n", [0], nn=-1)
    a, k = ids(2, 2)
    run("reset_dup", lambda: L.bsx_reset_streams(ctx, a, k, None))
    a, k = ids(n + 3)
    run("reset_out_of_range", lambda: L.bsx_reset_streams(ctx, a, k, None))
    rc_pipe = L.bsx_step_batch_pipelined(ctx, p(frames), p(bg), 0, p(out), n, None, 0)
    step("pending", [0])
    a, k = ids(0)
    run("reset_pending", lambda: L.bsx_reset_streams(ctx, a, k, None))
    rc_flush = L.bsx_step_batch_pipelined(ctx, None, None, 0, None, 0, None, 0)
    step("after_flush", [0, 1])
    L.bsx_delete(ctx)
    print(json.dumps({"calls": calls, "pipelined": [rc_pipe, rc_flush], "messages": msgs}))


if __name__ == "__main__":
    main()
