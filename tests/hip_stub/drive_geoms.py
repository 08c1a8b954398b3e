"""Runs UNDER LD_PRELOAD=libhipstub.so (tests/test_geoms_host.py starts it): drives bsx_new_geoms / bsx_step_batch_geoms of libbsx.so for contexts on device 1
while the caller's current device is 0, through the library's real host code — contexts of 1, 2 and 3 geometry classes stepping the same number of positions, the
mixed step of a one-geometry context next to them, every other entry point on a three-class context, the refusals and n == 0.  No torch, no GPU.  Prints one JSON
line: per call its return code, bsx_last_error, the caller's device afterwards and the span [first, last) of the HIP call log it produced."""
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
SIZES = [(640, 480), (1280, 720), (640, 360)]       # segm_lite: all on the fused tile route
N = 6                                               # positions of every traced step


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
    model, dev = sys.argv[1], int(sys.argv[2])
    stub = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhipstub.so"))
    L = load()
    msgs = []
    dbg = api.DEBUG_FN(lambda c, m: msgs.append(m.decode(errors="replace")))
    mask_cb = api.STAGE_FN(lambda c: None)
    none = api.STAGE_FN()
    calls = {}
    keep = []                                        # numpy buffers stay alive until the end

    def buf(*shape):
        a = np.zeros(shape, np.uint8)
        keep.append(a)
        return a

    def new_geoms(geoms, onmask=None, n_geoms=None, arr_null=False):
        arr = (api._Geometry * max(len(geoms), 1))(*[api._Geometry(*g) for g in geoms])
        return L.bsx_new_geoms(model.encode(), 2, None if arr_null else arr, len(geoms) if n_geoms is None else n_geoms, dev, dbg, none, none, onmask or none, None)

    def run(key, fn, c):
        first = log_lines()
        rc = fn()
        err = (L.bsx_last_error(c) or b"").decode(errors="replace").strip()
        calls[key] = {"rc": rc, "error": err, "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()]}

    def refused_new(key, *a, **k):
        first = log_lines()
        before = len(msgs)
        h = new_geoms(*a, **k)
        calls[key] = {"rc": 0 if h else -1, "error": "".join(msgs[before:]).strip() + " | " + (L.bsx_last_error(None) or b"").decode(errors="replace").strip(),
                      "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()], "null": not h}
        if h:
            L.bsx_delete(h)

    def geom_info(c):
        out = []
        for g in range(L.bsx_geom_count(c)):
            gi = api._GeomInfo()
            assert L.bsx_get_geom_info(c, g, C.byref(gi)) == 0
            out.append({k: (list(getattr(gi, k)) if k in ("roi", "in_roi") else getattr(gi, k)) for k, _ in api._GeomInfo._fields_})
        return out

    class Batch:
        """positions for the given stream ids of a context: its own frame, output and background per position"""
        def __init__(self, c, ids, yuyv=False, flags_of=lambda i: 0):
            info = geom_info(c)
            self.ids = (C.c_int * max(len(ids), 1))(*ids)
            self.n = len(ids)
            self.items = (api._GeomItem * max(len(ids), 1))()
            self.sizes = []
            for i, s in enumerate(ids):
                g = [q for q in info if q["first_stream"] <= s < q["first_stream"] + q["n_streams"]][0]
                W, H = g["width"], g["height"]
                self.sizes.append((W, H))
                fr, out, bg = buf(H, W, 3), buf(H, W, 2 if yuyv else 3), buf(H, W, 3)
                self.items[i].d_frame, self.items[i].d_out = fr.ctypes.data, out.ctypes.data
                self.items[i].setting.d_bg, self.items[i].setting.flags = bg.ctypes.data, flags_of(i)

    def step(key, c, b, flags=0, n=None, ids=True, items=True):
        run(key, lambda: L.bsx_step_batch_geoms(c, b.ids if ids else None, b.items if items else None, b.n if n is None else n, None, flags), c)

    cycle = [0, FLIP_H, FLIP_V, FLIP_H | FLIP_V, OFF, 0]

    # ---- the launch trace: N positions on contexts of 1, 2 and 3 classes, and the mixed step of a one-geometry context ---------------------------------------
    c1 = new_geoms([(640, 480, N)])
    c2 = new_geoms([(640, 480, 3), (1280, 720, 3)])
    c3 = new_geoms([(640, 480, 2), (1280, 720, 2), (640, 360, 2)])
    if not (c1 and c2 and c3):
        print(json.dumps({"error": "bsx_new_geoms failed: %s" % msgs}))
        return
    infos = {"c1": geom_info(c1), "c2": geom_info(c2), "c3": geom_info(c3)}
    inter = [4, 0, 2, 5, 1, 3]                       # interleaves the classes of c2 and c3
    b1, b2, b3 = Batch(c1, inter, flags_of=lambda i: cycle[i]), Batch(c2, inter, flags_of=lambda i: cycle[i]), Batch(c3, inter, flags_of=lambda i: cycle[i])
    step("trace_1", c1, b1)
    step("trace_2", c2, b2)
    step("trace_3", c3, b3)
    step("trace_3_again", c3, b3)
    step("yuyv", c3, Batch(c3, inter, yuyv=True, flags_of=lambda i: cycle[i]), flags=YUYV)
    step("no_mask", c3, b3, flags=NO_MASK)
    step("subset", c3, Batch(c3, [3, 0]))
    for i in range(6):                               # more calls than the ring has entries
        step("ring_%d" % i, c3, b3)
    # the mixed step of a one-geometry context with the same n: its network launches are the geoms step's
    cm = L.bsx_new(model.encode(), 2, 640, 480, N, dev, dbg, none, none, none, None)
    fr, out, bg = buf(N, 480, 640, 3), buf(N, 480, 640, 3), buf(480, 640, 3)
    st = (api._StreamSetting * N)()
    for i in range(N):
        st[i].d_bg, st[i].flags = bg.ctypes.data, cycle[i]
    ids6 = (C.c_int * N)(*inter)
    run("mixed_1", lambda: L.bsx_step_batch_mixed(cm, ids6, fr.ctypes.data, st, out.ctypes.data, N, None, 0), cm)
    # a context made by bsx_new takes the geoms step too
    step("on_bsx_new", cm, Batch(cm, inter, flags_of=lambda i: cycle[i]))

    # ---- n == 0 ----------------------------------------------------------------------------------------------------------------------------------------------
    step("empty", c3, Batch(c3, []), items=False)

    # ---- every other stepping entry point on the three-class context: refused, nothing enqueued ------------------------------------------------------------------
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    F, O, G = buf(N, 480, 640, 3), buf(N, 480, 640, 3), buf(480, 640, 3)
    idsN = (C.c_int * N)(*range(N))
    stN = (api._StreamSetting * N)()
    for i in range(N):
        stN[i].d_bg = G.ctypes.data
    stat = (api.LaunchStat * 64)()
    out4 = (C.c_long * 4)()
    refused = {
        "r_step": lambda: L.bsx_step_batch(c3, p(F), p(G), 0, p(O), N, None),
        "r_yuyv": lambda: L.bsx_step_batch_yuyv(c3, p(F), p(G), 0, p(O), N, None),
        "r_ex": lambda: L.bsx_step_batch_ex(c3, p(F), p(G), 0, p(O), N, None, 0),
        "r_streams": lambda: L.bsx_step_batch_streams(c3, idsN, p(F), p(G), 0, p(O), N, None, 0),
        "r_mixed": lambda: L.bsx_step_batch_mixed(c3, idsN, p(F), stN, p(O), N, None, 0),
        "r_vcam": lambda: L.bsx_step_batch_vcam(c3, p(F), p(G), 0, p(O), 320, 240, N, None, 0),
        "r_vcam_mixed": lambda: L.bsx_step_batch_vcam_mixed(c3, idsN, p(F), stN, p(O), 320, 240, N, None, 0),
        "r_pipelined": lambda: L.bsx_step_batch_pipelined(c3, p(F), p(G), 0, p(O), N, None, 0),
        "r_pipelined_flush": lambda: L.bsx_step_batch_pipelined(c3, None, None, 0, None, 0, None, 0),
        "r_process": lambda: L.bsx_process_batch(c3, p(F), N, None, None),
        "r_process_host": lambda: L.bsx_process_host(c3, 0, p(F), 640 * 3, p(O), 640),
        "r_composite": lambda: L.bsx_composite_batch(c3, p(G), 0, p(F), None, p(O), N, None),
        "r_profile": lambda: L.bsx_profile_batch(c3, p(F), p(G), 0, p(O), N, 1, stat, 64, None),
        "r_stage": lambda: L.bsx_debug_run_stage(c3, 0, p(F), N, None),
        "r_tile_stats": lambda: L.bsx_debug_mask_tile_stats(c3, N, out4),
    }
    for key, fn in refused.items():
        run(key, fn, c3)
    first = log_lines()
    live = L.bsx_live_new(c3)
    calls["r_live"] = {"rc": -1 if not live else 0, "error": (L.bsx_last_error(c3) or b"").decode(errors="replace").strip(),
                       "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()]}
    # ---- the allowed ones run ----------------------------------------------------------------------------------------------------------------------------------
    info = api._Info()
    run("a_info", lambda: L.bsx_get_info(c3, C.byref(info)), c3)
    info_d = {"width": info.width, "height": info.height, "n_streams": info.n_streams}
    run("a_reset", lambda: L.bsx_reset(c3, None), c3)
    three = (C.c_int * 3)(5, 0, 2)                   # one stream per class, classes out of order
    run("a_reset_streams", lambda: L.bsx_reset_streams(c3, three, 3, None), c3)
    small, big = buf(2, 90, 160, 3), buf(2, 480, 640, 3)
    run("a_resize", lambda: L.bsx_resize_bgr(c3, p(small), 160, 90, p(big), 640, 480, 2, None), c3)
    bgh = L.bsx_background_from_frames(c3, p(small), 160, 90, 2, 5.0, 0)
    grab_out = buf(2, 720, 1280, 3)
    bgs = (C.c_void_p * 2)(bgh, bgh)
    run("a_grab", lambda: L.bsx_background_grab_batch(bgs, 2, 1280, 720, p(grab_out), 1280 * 720 * 3, 0.3, None, None), c3)
    L.bsx_background_free(bgh)
    pbuf, pbytes = C.c_void_p(), C.c_size_t()
    run("a_debug_buffer", lambda: L.bsx_debug_buffer(c3, 3, C.byref(pbuf), C.byref(pbytes)), c3)
    mask_bytes = pbytes.value
    masks_dev = L.bsx_masks_device(c3)
    step("after_reset", c3, b3)

    # ---- refusals of the geoms step: validated on the host before anything is enqueued -----------------------------------------------------------------------
    def variant(key, change, flags=0, ids=inter, yuyv=False):
        b = Batch(c3, ids, yuyv=yuyv)
        change(b)
        step(key, c3, b, flags=flags)

    step("dup", c3, Batch(c3, [0, 1, 0, 2]))
    bad = Batch(c3, [0, 1, 2, 3])
    bad.ids[1] = N
    step("out_of_range", c3, bad)
    step("negative_n", c3, b3, n=-1)
    step("too_many", c3, b3, n=N + 1)
    step("ids_null", c3, b3, ids=False)
    step("items_null", c3, b3, items=False)
    step("batch_flip", c3, b3, flags=FLIP_H)
    step("batch_yuyv_in", c3, b3, flags=YUYV_IN)
    step("batch_blur", c3, b3, flags=blur(7))
    variant("setting_blur", lambda b: setattr(b.items[2].setting, "flags", blur(7)))
    variant("setting_bit0", lambda b: setattr(b.items[3].setting, "flags", YUYV | FLIP_H))
    variant("frame_null", lambda b: setattr(b.items[1], "d_frame", None))
    variant("frame_unaligned", lambda b: setattr(b.items[1], "d_frame", b.items[1].d_frame + 2))
    variant("out_null", lambda b: setattr(b.items[4], "d_out", None))
    variant("out_unaligned", lambda b: setattr(b.items[4], "d_out", b.items[4].d_out + 1))
    variant("bg_null", lambda b: setattr(b.items[5].setting, "d_bg", None))
    variant("bg_unaligned", lambda b: setattr(b.items[5].setting, "d_bg", b.items[5].setting.d_bg + 3))

    def bg_unread(b):                                # a filter-off position reads no background: NULL is fine there
        b.items[0].setting.d_bg, b.items[0].setting.flags = None, OFF
    variant("bg_null_filter_off", bg_unread)
    variant("out_is_frame", lambda b: setattr(b.items[2], "d_out", b.items[2].d_frame))
    variant("out_overlaps_other_frame", lambda b: setattr(b.items[2], "d_out", b.items[0].d_frame))
    variant("out_overlaps_bg", lambda b: setattr(b.items[3], "d_out", b.items[1].setting.d_bg))
    variant("out_overlaps_out", lambda b: setattr(b.items[3], "d_out", b.items[5].d_out + 4))
    # a pending pipelined composite (possible on a one-geometry context only)
    rc_pipe = L.bsx_step_batch_pipelined(cm, p(F), p(G), 0, p(O), N, None, 0)
    step("pending", cm, Batch(cm, inter))
    rc_flush = L.bsx_step_batch_pipelined(cm, None, None, 0, None, 0, None, 0)
    # one-geometry contexts the fused tile route does not take, or with an odd width and YUYV out, or with an onmask callback
    w2 = L.bsx_new(model.encode(), 2, 642, 480, 2, dev, dbg, none, none, none, None)
    step("class_off_route", w2, Batch(w2, [1, 0]))
    odd = L.bsx_new(model.encode(), 2, 641, 480, 2, dev, dbg, none, none, none, None)
    step("odd_width_yuyv", odd, Batch(odd, [1, 0], yuyv=True), flags=YUYV)
    cb = L.bsx_new(model.encode(), 2, 640, 480, 2, dev, dbg, none, none, mask_cb, None)
    step("onmask", cb, Batch(cb, [1, 0]))

    # ---- bsx_new_geoms refusals: NULL, the class named, nothing enqueued -----------------------------------------------------------------------------------------
    refused_new("new_zero", [], n_geoms=0)
    refused_new("new_nine", [(640 + 4 * i, 480, 1) for i in range(9)])
    refused_new("new_null", [(640, 480, 1)], arr_null=True)
    refused_new("new_bad_size", [(640, 480, 1), (0, 720, 1)])
    refused_new("new_bad_count", [(640, 480, 1), (1280, 720, 0)])
    refused_new("new_same_size", [(640, 480, 1), (1280, 720, 1), (640, 480, 2)])
    refused_new("new_too_many_streams", [(640, 480, 40000), (1280, 720, 30000)])
    refused_new("new_onmask", [(640, 480, 1), (1280, 720, 1)], onmask=mask_cb)
    refused_new("new_off_route", [(640, 480, 1), (1920, 1080, 1)])          # segm_lite: roi.w = 1799
    one_onmask = new_geoms([(640, 480, 2)], onmask=mask_cb)                  # one class IS bsx_new: an onmask callback and any size are fine
    one_odd = new_geoms([(1920, 1080, 1)])
    one_ok = [bool(one_onmask), bool(one_odd)]
    for c in (one_onmask, one_odd, w2, odd, cb, cm, c1, c2, c3):
        if c:
            L.bsx_delete(c)
    print(json.dumps({"calls": calls, "infos": infos, "info": info_d, "mask_bytes": mask_bytes, "masks_dev": bool(masks_dev), "pipelined": [rc_pipe, rc_flush],
                      "one_ok": one_ok, "sizes": {"b2": b2.sizes, "b3": b3.sizes}}))


if __name__ == "__main__":
    main()
