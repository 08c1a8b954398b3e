"""Runs UNDER LD_PRELOAD=libhipstub.so (tests/test_vcam_mixed_host.py starts it): drives bsx_step_batch_vcam_mixed of libbsx.so for a context on device 1 while the
caller's current device is 0, through the library's real host code — the dense and the id form, every batch flag set, batches with 0, 1 and 2 distinct blur sizes, a
capture geometry and a background alignment the mixed step refuses, the capture size itself, the refusals and n == 0.  No torch, no GPU.  Prints one JSON line: per
call its return code, bsx_last_error, the caller's device afterwards and the span [first, last) of the HIP call log it produced."""
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
    OW, OH = 426, 240
    stub = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhipstub.so"))
    L = load()
    msgs = []
    dbg = api.DEBUG_FN(lambda c, m: msgs.append(m.decode(errors="replace")))

    def new(w, h):
        return L.bsx_new(model.encode(), 2, w, h, n, dev, dbg, api.STAGE_FN(), api.STAGE_FN(), api.STAGE_FN(), None)

    ctx = new(W, H)
    if not ctx:
        print(json.dumps({"error": "bsx_new failed: %s" % msgs}))
        return
    # "device" buffers are host memory under the stub
    frames = np.zeros((n, H, W, 3), np.uint8)
    frames2 = np.zeros((n, H, W, 2), np.uint8)
    gallery = np.zeros((3, H, W, 3), np.uint8)
    own = np.zeros((n, H, W, 3), np.uint8)
    out = np.zeros((n, OH, OW, 3), np.uint8)
    out2 = np.zeros((n, OH, OW, 2), np.uint8)
    full = np.zeros((n, H, W, 3), np.uint8)
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

    def vm(key, st, ids=None, flags=0, fr=frames, o=out, ow=OW, oh=OH, nn=None, c=None):
        a = (C.c_int * max(len(ids), 1))(*ids) if ids is not None else None
        k = (len(ids) if ids is not None else n) if nn is None else nn
        run(key, lambda: L.bsx_step_batch_vcam_mixed(c or ctx, a, p(fr) if fr is not None else None, st, p(o) if o is not None else None, ow, oh, k, None, flags), c)

    perm = list(range(n))[::-1]
    no_blur = settings((own[0], 0), (g(0), FLIP_H), (g(1), OFF), (g(0), FLIP_H | FLIP_V))
    one_blur = settings((own[0], 0), (None, blur(7) | FLIP_H), (g(1), OFF | blur(25)), (None, blur(7) | FLIP_V))
    two_blur = settings((None, blur(7)), (None, blur(25) | FLIP_H), (None, OFF | blur(3)), (g(2), FLIP_V))
    vm("dense", no_blur)
    vm("ids", no_blur, ids=perm)
    vm("blur0", no_blur, ids=perm)
    vm("blur1", one_blur, ids=perm)
    vm("blur2", two_blur, ids=perm)
    vm("yuyv", two_blur, flags=YUYV, o=out2)
    vm("yuyv_in", no_blur, flags=YUYV_IN | YUYV, fr=frames2, o=out2)
    vm("yuyv_in_blur", one_blur, ids=perm, flags=YUYV_IN | YUYV, fr=frames2, o=out2)
    vm("unaligned_bg", settings((own[0], 0), (g(0), 0), (g(1), 0), (odd.ctypes.data + 1, 0)))     # any alignment: the kernel's byte form for that stream
    vm("subset", settings((g(0), 0), (None, blur(7))), ids=[2, 0])
    for i in range(6):                                   # more calls than the ring has entries: entries are reused behind their events
        vm("ring_%d" % i, no_blur)
    vm("capture_size", no_blur, o=full, ow=W, oh=H)      # the capture size: bsx_step_batch_mixed
    # n == 0: nothing happens, nothing is enqueued
    vm("empty", None, nn=0, fr=None, o=None)
    vm("empty_ids", None, ids=[], fr=None, o=None)
    # refusals: validated on the host before anything is enqueued
    vm("dup", no_blur, ids=[0, 1, 0, 2])
    vm("out_of_range", no_blur, ids=[0, n, 1, 2])
    vm("negative_n", no_blur, nn=-1)
    vm("too_many", no_blur, nn=n + 1)
    vm("settings_null", None)
    vm("batch_flip", no_blur, flags=FLIP_H)
    vm("batch_bit5", no_blur, flags=OFF)
    vm("batch_blur", no_blur, flags=blur(7))
    vm("no_mask", no_blur, flags=NO_MASK)
    vm("no_mask_capture_size", no_blur, flags=NO_MASK, o=full, ow=W, oh=H)
    vm("stream_yuyv_bit", settings((own[0], 0), (g(0), YUYV), (g(1), 0), (g(2), 0)))
    vm("stream_bit6", settings((own[0], 0), (g(0), 0), (g(1), 64 | FLIP_H), (g(2), 0)))
    vm("even_blur", settings((own[0], 0), (g(0), 0), (None, blur(8)), (g(2), 0)))
    vm("big_blur", settings((None, blur(33)), (g(0), 0), (g(1), 0), (g(2), 0)))
    vm("off_even_blur", settings((own[0], 0), (g(0), OFF | blur(4)), (g(1), 0), (g(2), 0)))
    vm("null_bg", settings((own[0], 0), (g(0), 0), (g(1), 0), (None, FLIP_H)))
    vm("zero_width", no_blur, ow=0)
    vm("negative_height", no_blur, oh=-3)
    vm("odd_yuyv_out", no_blur, flags=YUYV, o=out2, ow=OW - 1)
    vm("out_is_frames", no_blur, o=frames)
    vm("out_inside_frames", no_blur, o=frames[1])
    vm("out_overlaps_bg", settings((own[0], 0), (out[2], FLIP_H), (g(1), 0), (g(2), 0)))
    vm("null_frames", no_blur, fr=None)
    rc_pipe = L.bsx_step_batch_pipelined(ctx, p(frames), p(gallery), 0, p(full), n, None, 0)
    vm("pending", no_blur)
    vm("pending_empty", None, nn=0, fr=None, o=None)
    rc_flush = L.bsx_step_batch_pipelined(ctx, None, None, 0, None, 0, None, 0)
    vm("after_flush", no_blur)
    # a capture width the mixed step refuses (not a multiple of 4), and an odd one with YUYV frames
    w2_ctx = new(W + 2, H)
    wide = np.zeros((n, H, W + 2, 3), np.uint8)
    wide_y = np.zeros((n, H, W + 2, 2), np.uint8)
    vm("width_not_4", no_blur, fr=wide, c=w2_ctx)
    vm("width_not_4_yuyv_in", one_blur, fr=wide_y, flags=YUYV_IN, c=w2_ctx)
    vm("width_not_4_capture_size", no_blur, fr=wide, o=np.zeros((n, H, W + 2, 3), np.uint8), ow=W + 2, oh=H, c=w2_ctx)
    odd_ctx = new(W + 1, H)
    vm("odd_width_yuyv_in", no_blur, flags=YUYV_IN, fr=wide_y, c=odd_ctx)
    for c in (odd_ctx, w2_ctx):
        L.bsx_delete(c)
    L.bsx_delete(ctx)
    print(json.dumps({"calls": calls, "pipelined": [rc_pipe, rc_flush], "messages": msgs}))


if __name__ == "__main__":
    main()
