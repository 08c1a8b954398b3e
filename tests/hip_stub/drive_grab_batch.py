"""Runs UNDER LD_PRELOAD=libhipstub.so (tests/test_grab_batch_host.py starts it): drives bsx_resize_bgr_batch and bsx_background_grab_batch of libbsx.so for a
context on device 1 while the caller's current device is 0, through the library's real host code — batches of 1, 3 and n_streams images with one, two and three
distinct source sizes, each a second time, more calls than the staging ring has entries, the picture choice for explicit times and for the clock, the refusals
and n == 0.  No torch, no GPU.  Prints one JSON line: per call its return code, bsx_last_error of the context and of the thread, the caller's device afterwards,
the frame numbers it wrote and the span [first, last) of the HIP call log it produced."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from backscrub_amd import api  # noqa: E402  (module import only: api.lib() would pull torch in)

SENTINEL = -77                      # what frame_nos holds before a call: a refused call must leave it


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

    def new():
        return L.bsx_new(model.encode(), 2, W, H, n, dev, dbg, api.STAGE_FN(), api.STAGE_FN(), api.STAGE_FN(), None)

    ctx, other = new(), new()
    if not ctx or not other:
        print(json.dumps({"error": "bsx_new failed: %s" % msgs}))
        return
    img = W * H * 3
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    calls = {}

    def run(key, fn, nos=None):
        first = log_lines()
        rc = fn()
        err = (L.bsx_last_error(ctx) or b"").decode(errors="replace").strip()
        err_thread = (L.bsx_last_error(None) or b"").decode(errors="replace").strip()
        calls[key] = {"rc": rc, "error": err, "error_thread": err_thread, "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()],
                      "frame_nos": list(nos) if nos is not None else None}

    # ---- bsx_resize_bgr_batch: "device" buffers are host memory under the stub -----------------------------------------------------------------------------
    out = np.zeros((n, H, W, 3), np.uint8)
    held = []

    def items(sizes, dsts=None, srcs=None):
        arr = (api._ResizeItem * max(len(sizes), 1))()
        for i, (sw, sh) in enumerate(sizes):
            src = np.zeros((max(sh, 1), max(sw, 1), 3), np.uint8)
            held.append(src)
            arr[i].d_src = src.ctypes.data if srcs is None else srcs[i]
            arr[i].sw, arr[i].sh = sw, sh
            arr[i].d_dst = out[i].ctypes.data if dsts is None else dsts[i]
        return arr

    def resize(key, sizes, nn=None, dw=W, dh=H, arr="make", **kw):
        a = items(sizes, **kw) if arr == "make" else arr
        run(key, lambda: L.bsx_resize_bgr_batch(ctx, a, len(sizes) if nn is None else nn, dw, dh, None))

    A, B, Cc, D, E, F = (32, 24), (50, 30), (17, 9), (64, 64), (100, 75), (31, 33)          # none the output size or its double: every one needs a table
    batches = {"rsz_1": [A], "rsz_3": [B, Cc, B], "rsz_n": ([D, E, F] * n)[:n]}
    for key, sizes in batches.items():
        resize(key, sizes)
    for key, sizes in batches.items():
        resize(key + "_again", sizes)
    resize("rsz_modes", [(W, H), (2 * W, 2 * H), A])            # the identity and the exact-2x mode have no table to upload
    for i in range(6):                                         # more calls than the ring has entries: entries are reused behind their events
        resize("rsz_ring_%d" % i, [A, B])
    resize("rsz_empty", [], arr=None)
    # refusals
    resize("rsz_negative_n", [A], nn=-1)
    resize("rsz_too_many", [A] * n, nn=n + 1)
    resize("rsz_items_null", [A], arr=None)
    resize("rsz_bad_out_size", [A], dw=0)
    big = np.zeros((H, W, 3), np.uint8)
    resize("rsz_null_src", [A, B, A], srcs=[big.ctypes.data, None, big.ctypes.data])
    resize("rsz_null_dst", [A, B, A], dsts=[out[0].ctypes.data, out[1].ctypes.data, None])
    resize("rsz_bad_src_size", [A, (0, 7), A])
    resize("rsz_dst_overlaps_dst", [A, B, A], dsts=[out[0].ctypes.data, out[1].ctypes.data, out[1].ctypes.data + 12])
    resize("rsz_dst_overlaps_src", [A, (W, H), A], srcs=[held[0].ctypes.data, big.ctypes.data, held[0].ctypes.data],
           dsts=[out[0].ctypes.data, out[1].ctypes.data, big.ctypes.data + img - 1])
    shared = np.zeros((24, 32, 3), np.uint8)                    # two entries, ONE source, two outputs: allowed
    resize("rsz_shared_src", [A, A], srcs=[shared.ctypes.data] * 2)

    # ---- bsx_background_grab_batch ---------------------------------------------------------------------------------------------------------------------------
    def background(w, h, frames, fps, c=None):
        px = np.zeros((frames, h, w, 3), np.uint8)
        b = L.bsx_background_from_frames(c or ctx, px.ctypes.data, w, h, frames, float(fps), 0)
        assert b
        return b

    still = background(40, 30, 1, 0.0)
    still2 = background(33, 21, 1, 0.0)
    anim = {"a": (background(32, 24, 5, 10.0), 5, 10.0), "b": (background(50, 30, 7, 24.0), 7, 24.0), "c": (background(17, 9, 3, 12.5), 3, 12.5)}
    foreign = background(40, 30, 1, 0.0, other)

    def grab(key, bgs, at, nn=None, w=W, h=H, o=out, stride=img, want_nos=True, arr="make"):
        a = (C.c_void_p * max(len(bgs), 1))(*bgs) if arr == "make" else arr
        nos = (C.c_int * max(len(bgs), 1))(*([SENTINEL] * max(len(bgs), 1))) if want_nos else None
        run(key, lambda: L.bsx_background_grab_batch(a, len(bgs) if nn is None else nn, w, h, p(o) if o is not None else None, stride, at, nos, None), nos)

    a_, b_, c_ = anim["a"][0], anim["b"][0], anim["c"][0]
    full = ([a_, still, b_, c_, still2, a_] * n)[:n]
    grab("grab_1", [a_], 0.0)
    grab("grab_3", [b_, still, b_], 0.0)
    grab("grab_n", full, 0.0)
    grab("grab_n_again", full, 0.25)
    grab("grab_no_nos", [a_, still], 0.0, want_nos=False)
    for i in range(6):
        grab("grab_ring_%d" % i, [a_, still], 0.1 * i)
    # picture choice: the middle of frame period k, k below, at and beyond one loop; the expectation is formed in the test
    picks = []
    for name, (b, frames, fps) in anim.items():
        for k in (0, 1, frames - 1, frames, frames + 2, 10 * frames + 1, 1000 * frames + frames - 1):
            key = "pick_%s_%d" % (name, k)
            grab(key, [b, still, b], (k + 0.5) / fps)
            picks.append({"key": key, "k": k, "frames": frames})
    grab("clock", [a_, still, b_, a_, b_], -1.0)
    grab("grab_empty", [], 0.0, o=None, arr=None)
    # refusals
    grab("grab_negative_n", [a_], 0.0, nn=-1)
    grab("grab_too_many", [a_] * (n + 1), 0.0)
    grab("grab_bgs_null", [a_], 0.0, arr=None)
    grab("grab_null_entry", [a_, still, None], 0.0)
    grab("grab_foreign", [a_, foreign, still], 0.0)
    grab("grab_bad_size", [a_, still], 0.0, h=0)
    grab("grab_null_out", [a_, still], 0.0, o=None)
    grab("grab_short_stride", [a_, still], 0.0, stride=img - 1)
    grab("grab_nan", [a_, still], float("nan"))
    grab("grab_inf", [a_, still], float("inf"))
    for b in [still, still2, foreign] + [v[0] for v in anim.values()]:
        L.bsx_background_free(b)
    L.bsx_delete(other)
    L.bsx_delete(ctx)
    print(json.dumps({"calls": calls, "picks": picks, "sentinel": SENTINEL, "n": n, "messages": msgs}))


if __name__ == "__main__":
    main()
