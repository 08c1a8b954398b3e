"""Runs UNDER LD_PRELOAD=libhipstub.so (tests/test_surfaces_host.py starts it): drives bsx_step_batch_surfaces and bsx_nv12_to_bgr of libbsx.so for contexts on
device 1 while the caller's current device is 0, through the library's real host code — contexts of 1 and 3 geometry classes stepping the same positions into the
same output records, a masks-only call, the ring, n == 0, every refusal, and next to them bsx_step_batch_vcam_geoms_outs_nv12 and bsx_step_batch_geoms on the same
context.  No torch, no GPU.  Prints one JSON line: per call its return code, bsx_last_error, the caller's device afterwards and the span [first, last) of the HIP
call log it produced."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from backscrub_amd import api  # noqa: E402  (module import only: api.lib() would pull torch in)

FLIP_H, FLIP_V, OFF, YUYV_IN = 2, 4, 32, 64
N = 6                                               # positions of every traced step
LAYERS = [(320, 180), (160, 90)]                    # every position at the first size, position 0 at the second too


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

    def buf(nbytes):
        a = np.zeros(nbytes + 8, np.uint8)
        keep.append(a)
        return a.ctypes.data + (-a.ctypes.data) % 4

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
        """positions for the given stream ids of a context: its own surface (pitches above the width, and different) and background at the class's size; the output
        records of LAYERS, each a surface of its own.  geom: the same positions as bsx_geom_item with BGR frames, for the two older entry points."""
        def __init__(self, c, ids, flags_of=lambda i: 0, pad=(64, 32)):
            info = geom_info(c)
            self.ids = (C.c_int * max(len(ids), 1))(*ids)
            self.n = len(ids)
            self.items = (api._SurfaceItem * max(len(ids), 1))()
            self.geom = (api._GeomItem * max(len(ids), 1))()
            self.sizes = []
            for i, s in enumerate(ids):
                g = [q for q in info if q["first_stream"] <= s < q["first_stream"] + q["n_streams"]][0]
                W, H = g["width"], g["height"]
                self.sizes.append((W, H))
                it = self.items[i]
                it.pitch_y, it.pitch_uv = (W + 3) // 4 * 4 + pad[0], (W + 3) // 4 * 4 + pad[1]
                it.d_y, it.d_uv = buf(it.pitch_y * H), buf(it.pitch_uv * (H // 2))
                it.setting.d_bg, it.setting.flags = buf(W * H * 3), flags_of(i)
                self.geom[i].d_frame, self.geom[i].d_out = buf(W * H * 3), buf(W * H * 3)
                self.geom[i].setting.d_bg, self.geom[i].setting.flags = it.setting.d_bg, flags_of(i)
            recs = [(i, LAYERS[0]) for i in range(self.n)] + ([(0, LAYERS[1])] if self.n else [])
            self.m = len(recs)
            self.outs = (api._VcamOutNv12 * max(self.m, 1))()
            for j, (i, (w, h)) in enumerate(recs):
                r = self.outs[j]
                r.item, r.out_w, r.out_h, r.pitch_y, r.pitch_uv = i, w, h, w + 96, w + 32
                r.d_y, r.d_uv = buf(r.pitch_y * h), buf(r.pitch_uv * (h // 2))

    def step(key, c, b, flags=0, n=None, ids=True, items=True, m=None):
        run(key, lambda: L.bsx_step_batch_surfaces(c, b.ids if ids else None, b.items if items else None, b.n if n is None else n, b.outs, b.m if m is None else m, None,
                                                   flags), c)

    cycle = [0, FLIP_H, FLIP_V, FLIP_H | FLIP_V, OFF, 0]
    c1 = new_geoms([(640, 480, N)])
    c3 = new_geoms([(640, 480, 2), (1280, 720, 2), (640, 360, 2)])
    cn = L.bsx_new(model.encode(), 2, 640, 480, N, dev, dbg, none, none, none, None)
    if not (c1 and c3 and cn):
        print(json.dumps({"error": "context creation failed: %s" % msgs}))
        return
    infos = {"c1": geom_info(c1), "c3": geom_info(c3)}
    inter = [4, 0, 2, 5, 1, 3]                       # interleaves the classes of c3
    mk = lambda c, **k: Batch(c, inter, flags_of=lambda i: cycle[i], **k)  # noqa: E731
    b1, b3 = mk(c1), mk(c3)
    step("surf_1", c1, b1)
    step("surf_3", c3, b3)
    step("surf_3_again", c3, b3)                     # the same sizes: nothing allocated, nothing uploaded
    step("tight", c3, mk(c3, pad=(0, 0)))            # pitch == W
    step("masks_only", c3, b3, m=0)
    for i in range(6):                               # more calls than the ring has entries
        step("ring_%d" % i, c3, b3)
    run("nv12_3", lambda: L.bsx_step_batch_vcam_geoms_outs_nv12(c3, b3.ids, b3.geom, N, b3.outs, b3.m, None, 0), c3)
    run("geoms_3", lambda: L.bsx_step_batch_geoms(c3, b3.ids, b3.geom, N, None, 0), c3)
    it0 = b3.items[1]                                # stream 0: 640 x 480
    run("conv", lambda: L.bsx_nv12_to_bgr(c3, it0.d_y, it0.pitch_y, it0.d_uv, it0.pitch_uv, 640, 480, 1, b3.geom[1].d_frame, None), c3)
    run("conv_tail", lambda: L.bsx_nv12_to_bgr(c3, it0.d_y, it0.pitch_y, it0.d_uv, it0.pitch_uv, 6, 4, 2, b3.geom[1].d_frame + 1, None), c3)
    step("empty", c3, Batch(c3, []), items=False)

    # ---- refusals: validated on the host before anything is enqueued -----------------------------------------------------------------------------------------
    def variant(key, change, flags=0, c=c3, ids=inter):
        b = Batch(c, ids)
        change(b)
        step(key, c, b, flags=flags)

    step("dup", c3, Batch(c3, [0, 1, 0, 2]))
    step("items_null", c3, b3, items=False)
    step("flags", c3, b3, flags=1)
    variant("setting_blur", lambda b: setattr(b.items[2].setting, "flags", blur(7)))
    variant("setting_yuyv_in", lambda b: setattr(b.items[3].setting, "flags", YUYV_IN | FLIP_H))
    variant("setting_bit0", lambda b: setattr(b.items[3].setting, "flags", 1 | FLIP_H))
    variant("y_null", lambda b: setattr(b.items[1], "d_y", None))
    variant("y_unaligned", lambda b: setattr(b.items[1], "d_y", b.items[1].d_y + 2))
    variant("uv_null", lambda b: setattr(b.items[4], "d_uv", None))
    variant("uv_unaligned", lambda b: setattr(b.items[4], "d_uv", b.items[4].d_uv + 1))
    variant("pitch_y_low", lambda b: setattr(b.items[0], "pitch_y", 636))
    variant("pitch_y_mod", lambda b: setattr(b.items[0], "pitch_y", 642))
    variant("pitch_uv_low", lambda b: setattr(b.items[3], "pitch_uv", 0))
    variant("pitch_uv_mod", lambda b: setattr(b.items[3], "pitch_uv", 1286))
    variant("bg_null", lambda b: setattr(b.items[5].setting, "d_bg", None))
    variant("bg_unaligned", lambda b: setattr(b.items[5].setting, "d_bg", b.items[5].setting.d_bg + 3))

    def bg_unread(b):                                # a filter-off position reads no background: NULL is fine there
        b.items[0].setting.d_bg, b.items[0].setting.flags = None, OFF
    variant("bg_null_filter_off", bg_unread)
    variant("out_y_is_in_y", lambda b: setattr(b.outs[2], "d_y", b.items[2].d_y))
    variant("out_uv_in_uv", lambda b: setattr(b.outs[1], "d_uv", b.items[0].d_uv + 4))
    variant("out_y_in_bg", lambda b: setattr(b.outs[3], "d_y", b.items[1].setting.d_bg))
    variant("out_y_in_out_uv", lambda b: setattr(b.outs[3], "d_y", b.outs[5].d_uv))

    # an input plane is judged on pitch * (rows - 1) + W: an output behind the last row's W bytes is free, one dword earlier is not
    def behind(delta):
        def change(b):
            it = b.items[1]                          # stream 0: 640 x 480, pitch_y 704
            it.d_y = buf(it.pitch_y * 480 + 320 * 180 + 512)
            b.outs[0].pitch_y = 320
            b.outs[0].d_y = it.d_y + it.pitch_y * 479 + 640 + delta
        return change
    variant("in_extent_touch", behind(0))
    variant("in_extent_overlap", behind(-4))
    variant("out_record", lambda b: setattr(b.outs[6], "pitch_uv", 158))           # a record refusal of vcam_nv12_plan.hpp arrives unchanged
    p = lambda a: C.c_void_p(a)  # noqa: E731
    F, O, G = buf(N * 480 * 640 * 3), buf(N * 480 * 640 * 3), buf(480 * 640 * 3)
    rc_pipe = L.bsx_step_batch_pipelined(cn, p(F), p(G), 0, p(O), N, None, 0)
    step("pending", cn, Batch(cn, inter))
    rc_flush = L.bsx_step_batch_pipelined(cn, None, None, 0, None, 0, None, 0)
    w2 = L.bsx_new(model.encode(), 2, 642, 480, 2, dev, dbg, none, none, none, None)
    step("class_off_route", w2, Batch(w2, [1, 0]))
    cb = L.bsx_new(model.encode(), 2, 640, 480, 2, dev, dbg, none, none, mask_cb, None)
    step("onmask", cb, Batch(cb, [1, 0]))
    # a class whose down-scale table is not the linear one: segm_lite's canvas is 160 x 96, so a 320 x 192 capture is the exact 2 x 2 mean
    ca = L.bsx_new(model.encode(), 2, 320, 192, 2, dev, dbg, none, none, none, None)
    if ca:
        infos["ca"] = geom_info(ca)
        step("class_area", ca, Batch(ca, [1, 0]))
    step("good_after", c3, b3)

    first = log_lines()
    for c in (ca, w2, cb, cn, c1, c3):
        if c:
            L.bsx_delete(c)
    calls["delete"] = {"rc": 0, "error": "", "caller_device": stub.bsx_stub_current_device(), "log": [first, log_lines()]}
    print(json.dumps({"calls": calls, "infos": infos, "pipelined": [rc_pipe, rc_flush]}))


if __name__ == "__main__":
    main()
