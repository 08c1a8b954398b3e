"""Runs UNDER LD_PRELOAD=libhipstub.so (tests/test_mixed_host.py starts it): drives bsx_step_batch_mixed of libbsx.so for a context on device 1 while the caller's
current device is 0, through the library's real host code — the dense and the id form, every batch flag set, batches with 0, 1 and 2 distinct blur sizes, the
refusals and n == 0.  No torch, no GPU.  Prints one JSON line: per call its return code, bsx_last_error, the caller's device afterwards and the span [first, last)
of the HIP call log it produced."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from backscrub_amd import api  # noqa: E402  (module import only: api.lib() would pull torch in)

FLIP_H, FLIP_V, OFF = 2, 4, 32
YUYV, NO_MASK, YUYV_IN = 1, 8, 16


def blur(k):
    return (k & 255) << 8


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
    mask_cb = api.STAGE_FN(lambda c: None)

    def new(w, h, onmask=None):
        return L.bsx_new(model.encode(), 2, w, h, n, dev, dbg, api.STAGE_FN(), api.STAGE_FN(), onmask or api.STAGE_FN(), None)

    ctx = new(W, H)
    if not ctx:
        print(json.dumps({"error": "bsx_new failed: %s" % msgs}))
        return
    # "device" buffers are host memory under the stub
    frames = np.zeros((n, H, W, 3), np.uint8)
    frames2 = np.zeros((n, H, W, 2), np.uint8)
    gallery = np.zeros((3, H, W, 3), np.uint8)
    own = np.zeros((n, H, W, 3), np.uint8)
    out = np.zeros((n, H, W, 3), np.uint8)
    out2 = np.zeros((n, H, W, 2), np.uint8)
    odd = np.zeros(W * H * 3 + 8, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    calls = {}

    def run(key, fn, c=None):
        first = log_lines()
        rc = fn()
        err = (L.bsx_last_error(c or ctx) or b"").decode(errors="replace").strip()
        calls[key] = {"rc": rc, "error": err, "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()]}

    def settings(*entries):
        st = (api._StreamSetting * max(len(entries), 1))()
        for i, (bg, fl) in enumerate(entries):
            st[i].d_bg = bg if isinstance(bg, (int, type(None))) else bg.ctypes.data
            st[i].flags = fl
        return st

    def g(k):
        return gallery[k]

    def mixed(key, st, ids=None, flags=0, fr=frames, o=out, nn=None, c=None):
        a = (C.c_int * max(len(ids), 1))(*ids) if ids is not None else None
        k = (len(ids) if ids is not None else n) if nn is None else nn
        run(key, lambda: L.bsx_step_batch_mixed(c or ctx, a, p(fr) if fr is not None else None, st, p(o) if o is not None else None, k, None, flags), c)

    perm = list(range(n))[::-1]
    # a batch without blur streams, one with one blur size, one with two (a filter-off stream's blur size makes no launch)
    no_blur = settings((own[0], 0), (g(0), FLIP_H), (g(1), OFF), (g(0), FLIP_H | FLIP_V))
    one_blur = settings((own[0], 0), (None, blur(7) | FLIP_H), (g(1), OFF | blur(25)), (None, blur(7) | FLIP_V))
    two_blur = settings((None, blur(7)), (None, blur(25) | FLIP_H), (None, OFF | blur(3)), (g(2), FLIP_V))
    mixed("dense", no_blur)
    mixed("ids", no_blur, ids=perm)
    mixed("blur0", no_blur, ids=perm)
    mixed("blur1", one_blur, ids=perm)
    mixed("blur2", two_blur, ids=perm)
    mixed("yuyv", two_blur, flags=YUYV, o=out2)
    mixed("no_mask", one_blur, ids=perm, flags=NO_MASK)
    mixed("yuyv_in", no_blur, flags=YUYV_IN | YUYV, fr=frames2, o=out2)
    mixed("yuyv_in_blur", one_blur, ids=perm, flags=YUYV_IN | YUYV, fr=frames2, o=out2)
    for i in range(6):                                   # more calls than the ring has entries: entries are reused behind their events
        mixed("ring_%d" % i, no_blur)
    # n == 0: nothing happens, nothing is enqueued
    mixed("empty", None, nn=0, fr=None, o=None)
    mixed("empty_ids", None, ids=[], fr=None, o=None)
    # refusals: validated on the host before anything is enqueued
    mixed("dup", no_blur, ids=[0, 1, 0, 2])
    mixed("out_of_range", no_blur, ids=[0, n, 1, 2])
    mixed("negative_n", no_blur, nn=-1)
    mixed("too_many", no_blur, nn=n + 1)
    mixed("settings_null", None)
    mixed("batch_flip", no_blur, flags=FLIP_H)
    mixed("batch_bit5", no_blur, flags=OFF)
    mixed("batch_blur", no_blur, flags=blur(7))
    mixed("stream_yuyv_bit", settings((own[0], 0), (g(0), YUYV), (g(1), 0), (g(2), 0)))
    mixed("stream_bit6", settings((own[0], 0), (g(0), 0), (g(1), 64 | FLIP_H), (g(2), 0)))
    mixed("even_blur", settings((own[0], 0), (g(0), 0), (None, blur(8)), (g(2), 0)))
    mixed("big_blur", settings((None, blur(33)), (g(0), 0), (g(1), 0), (g(2), 0)))
    mixed("off_even_blur", settings((own[0], 0), (g(0), OFF | blur(4)), (g(1), 0), (g(2), 0)))
    mixed("null_bg", settings((own[0], 0), (g(0), 0), (g(1), 0), (None, FLIP_H)))
    mixed("unaligned_bg", settings((own[0], 0), (g(0), 0), (g(1), 0), (odd.ctypes.data + 1, 0)))
    mixed("out_is_frames", no_blur, o=frames)
    mixed("out_overlaps_bg", settings((own[0], 0), (out[2], FLIP_H), (g(1), 0), (g(2), 0)))
    mixed("unaligned_out", no_blur, o=np.frombuffer(odd.data, np.uint8, W * H * 3, 1).reshape(1, H, W, 3), nn=1)
    rc_pipe = L.bsx_step_batch_pipelined(ctx, p(frames), p(gallery), 0, p(out), n, None, 0)
    mixed("pending", no_blur)
    rc_flush = L.bsx_step_batch_pipelined(ctx, None, None, 0, None, 0, None, 0)
    mixed("after_flush", no_blur)
    # bit 5 stays refused by every other step entry point
    run("ex_bit5", lambda: L.bsx_step_batch_ex(ctx, p(frames), p(gallery), 0, p(out), n, None, OFF))
    ids4 = (C.c_int * n)(*perm)
    run("streams_bit5", lambda: L.bsx_step_batch_streams(ctx, ids4, p(frames), p(gallery), 0, p(out), n, None, OFF))
    # contexts whose geometry or callbacks the fused tile route does not take
    odd_ctx = new(W + 1, H)
    wide = np.zeros((n, H, W + 2, 3), np.uint8)
    wide_out = np.zeros((n, H, W + 2, 3), np.uint8)
    wide2 = np.zeros((n, H, W + 1, 2), np.uint8)
    mixed("odd_width_yuyv", no_blur, flags=YUYV, fr=wide, o=wide2, c=odd_ctx)
    mixed("odd_width_yuyv_in", no_blur, flags=YUYV_IN, fr=wide2, o=wide, c=odd_ctx)
    w2_ctx = new(W + 2, H)
    mixed("width_not_4", no_blur, fr=wide, o=wide_out, c=w2_ctx)
    cb_ctx = new(W, H, onmask=mask_cb)
    mixed("onmask", no_blur, c=cb_ctx)
    for c in (odd_ctx, w2_ctx, cb_ctx):
        L.bsx_delete(c)
    L.bsx_delete(ctx)
    print(json.dumps({"calls": calls, "pipelined": [rc_pipe, rc_flush], "messages": msgs}))


if __name__ == "__main__":
    main()
