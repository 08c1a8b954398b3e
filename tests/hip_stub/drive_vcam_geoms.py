"""Runs UNDER LD_PRELOAD=libhipstub.so (tests/test_vcam_geoms_host.py starts it): drives bsx_step_batch_vcam_geoms of libbsx.so for contexts on device 1 while the
caller's current device is 0, through the library's real host code — contexts of 1, 2 and 3 geometry classes and one made by bsx_new stepping the same number of
positions at one output size, a second call at that size, other output sizes, the ring, the refusals and n == 0.  No torch, no GPU.  Prints one JSON line: per
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
N = 6                                               # positions of every traced step
OUT = (426, 240)


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

    def new_geoms(geoms):
        arr = (api._Geometry * len(geoms))(*[api._Geometry(*g) for g in geoms])
        return L.bsx_new_geoms(model.encode(), 2, arr, len(geoms), dev, dbg, none, none, none, None)

    def run(key, fn, c):
        first = log_lines()
        rc = fn()
        err = (L.bsx_last_error(c) or b"").decode(errors="replace").strip()
        calls[key] = {"rc": rc, "error": err, "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()]}

    def geom_info(c):
        out = []
        for g in range(L.bsx_geom_count(c)):
            gi = api._GeomInfo()
            assert L.bsx_get_geom_info(c, g, C.byref(gi)) == 0
            out.append({k: (list(getattr(gi, k)) if k in ("roi", "in_roi") else getattr(gi, k)) for k, _ in api._GeomInfo._fields_})
        return out

    class Batch:
        """positions for the given stream ids of a context: its own frame and background at the class's size, its own output at the output size"""
        def __init__(self, c, ids, out=OUT, yuyv=False, flags_of=lambda i: 0):
            info = geom_info(c)
            self.ids = (C.c_int * max(len(ids), 1))(*ids)
            self.n = len(ids)
            self.items = (api._GeomItem * max(len(ids), 1))()
            self.out = out
            for i, s in enumerate(ids):
                g = [q for q in info if q["first_stream"] <= s < q["first_stream"] + q["n_streams"]][0]
                W, H = g["width"], g["height"]
                fr, o, bg = buf(H, W, 3), buf(max(out[1], 1), max(out[0], 1), 2 if yuyv else 3), buf(H, W, 3)
                self.items[i].d_frame, self.items[i].d_out = fr.ctypes.data, o.ctypes.data
                self.items[i].setting.d_bg, self.items[i].setting.flags = bg.ctypes.data, flags_of(i)

    def step(key, c, b, flags=0, n=None, ids=True, items=True, out=None):
        ow, oh = out or b.out
        run(key, lambda: L.bsx_step_batch_vcam_geoms(c, b.ids if ids else None, b.items if items else None, b.n if n is None else n, ow, oh, None, flags), c)

    cycle = [0, FLIP_H, FLIP_V, FLIP_H | FLIP_V, OFF, 0]
    c1 = new_geoms([(640, 480, N)])
    c2 = new_geoms([(640, 480, 3), (1280, 720, 3)])
    c3 = new_geoms([(640, 480, 2), (1280, 720, 2), (640, 360, 2)])
    cn = L.bsx_new(model.encode(), 2, 640, 480, N, dev, dbg, none, none, none, None)
    if not (c1 and c2 and c3 and cn):
        print(json.dumps({"error": "context creation failed: %s" % msgs}))
        return
    infos = {"c1": geom_info(c1), "c2": geom_info(c2), "c3": geom_info(c3), "cn": geom_info(cn)}
    inter = [4, 0, 2, 5, 1, 3]                       # interleaves the classes of c2 and c3
    mk = lambda c, **k: Batch(c, inter, flags_of=lambda i: cycle[i], **k)  # noqa: E731
    b1, b2, b3, bn = mk(c1), mk(c2), mk(c3), mk(cn)
    step("trace_1", c1, b1)
    step("trace_2", c2, b2)
    step("trace_3", c3, b3)
    step("trace_new", cn, bn)
    step("trace_3_again", c3, b3)                    # the same output size: nothing allocated, nothing uploaded
    step("yuyv", c3, mk(c3, yuyv=True), flags=YUYV)
    step("odd_width", c3, mk(c3, out=(427, 240)))
    step("own_size", c3, mk(c3, out=(640, 360)))     # identity for class 2, exact 2x of class 1
    step("eighth", c3, mk(c3, out=(160, 90)))
    step("subset", c3, Batch(c3, [3, 0]))
    for i in range(6):                               # more calls than the ring has entries
        step("ring_%d" % i, c3, b3)
    # the geoms step after the vcam form on the same context: the shared front end serves both
    first = log_lines()
    g3 = Batch(c3, inter, out=(0, 0))
    info3 = geom_info(c3)
    for i, s in enumerate(inter):
        g = [q for q in info3 if q["first_stream"] <= s < q["first_stream"] + q["n_streams"]][0]
        g3.items[i].d_out = buf(g["height"], g["width"], 3).ctypes.data
    rc = L.bsx_step_batch_geoms(c3, g3.ids, g3.items, N, None, 0)
    calls["geoms_after"] = {"rc": rc, "error": "", "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()]}

    step("empty", c3, Batch(c3, []), items=False)

    # ---- refusals: validated on the host before anything is enqueued -----------------------------------------------------------------------------------------
    def variant(key, change, flags=0, ids=inter, yuyv=False, out=OUT):
        b = Batch(c3, ids, yuyv=yuyv, out=out)
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
    step("out_w_zero", c3, b3, out=(0, 240))
    step("out_h_negative", c3, b3, out=(426, -1))
    step("batch_no_mask", c3, b3, flags=NO_MASK)
    step("batch_yuyv_in", c3, b3, flags=YUYV_IN)
    step("batch_flip", c3, b3, flags=FLIP_H)
    step("batch_blur", c3, b3, flags=blur(7))
    step("odd_out_w_yuyv", c3, mk(c3, out=(427, 240), yuyv=True), flags=YUYV)
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
    # an output span has the OUTPUT size: an address one output image behind another output is free, one byte less is not
    ob = OUT[0] * OUT[1] * 3

    def packed(delta):
        big = buf(2 * ob + 8)

        def change(b):
            b.items[0].d_out, b.items[1].d_out = big.ctypes.data, big.ctypes.data + ob + delta
        return change
    variant("out_spans_touch", packed(0))
    variant("out_spans_overlap", packed(-4))
    # a pending pipelined composite (possible on a one-geometry context only)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    F, O, G = buf(N, 480, 640, 3), buf(N, 480, 640, 3), buf(480, 640, 3)
    rc_pipe = L.bsx_step_batch_pipelined(cn, p(F), p(G), 0, p(O), N, None, 0)
    step("pending", cn, Batch(cn, inter))
    rc_flush = L.bsx_step_batch_pipelined(cn, None, None, 0, None, 0, None, 0)
    # one-geometry contexts the fused tile route does not take, or with an onmask callback
    w2 = L.bsx_new(model.encode(), 2, 642, 480, 2, dev, dbg, none, none, none, None)
    step("class_off_route", w2, Batch(w2, [1, 0]))
    cb = L.bsx_new(model.encode(), 2, 640, 480, 2, dev, dbg, none, none, mask_cb, None)
    step("onmask", cb, Batch(cb, [1, 0]))
    # the dense and by-id vcam steps keep refusing a multi-geometry context
    idsN = (C.c_int * N)(*range(N))
    stN = (api._StreamSetting * N)()
    for i in range(N):
        stN[i].d_bg = G.ctypes.data
    run("r_vcam", lambda: L.bsx_step_batch_vcam(c3, p(F), p(G), 0, p(O), 320, 240, N, None, 0), c3)
    run("r_vcam_mixed", lambda: L.bsx_step_batch_vcam_mixed(c3, idsN, p(F), stN, p(O), 320, 240, N, None, 0), c3)

    first = log_lines()
    for c in (w2, cb, cn, c1, c2, c3):
        if c:
            L.bsx_delete(c)
    calls["delete"] = {"rc": 0, "error": "", "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()]}
    print(json.dumps({"calls": calls, "infos": infos, "pipelined": [rc_pipe, rc_flush]}))


if __name__ == "__main__":
    main()
