"""Runs UNDER LD_PRELOAD=libhipstub.so (tests/test_geoms_yuyv_in_host.py starts it): drives bsx_step_batch_geoms and bsx_step_batch_vcam_geoms of libbsx.so with
BSX_STREAM_YUYV_IN items through the library's real host code, the way tests/hip_stub/drive_geoms.py drives the BGR step.  No torch, no GPU.  Prints one JSON line:
per call its return code, bsx_last_error and the span [first, last) of the HIP call log it produced."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from backscrub_amd import api  # noqa: E402  (module import only: api.lib() would pull torch in)

FLIP_H, OFF, YIN = 2, 32, 64
YUYV, YUYV_IN = 1, 16
INTER = [4, 0, 2, 5, 1, 3]                          # interleaves the classes of the three-class context


def main():
    model, dev = sys.argv[1], int(sys.argv[2])
    L = C.CDLL(api.lib_path())
    for name, res, args in api.SYMBOLS:
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    msgs = []
    dbg = api.DEBUG_FN(lambda c, m: msgs.append(m.decode(errors="replace")))
    none = api.STAGE_FN()
    calls, keep = {}, []

    def log_lines():
        p = os.environ["BSX_STUB_LOG"]
        return len(open(p).read().splitlines()) if os.path.exists(p) else 0

    def buf(n):
        a = np.zeros(n + 64, np.uint8)
        keep.append(a)
        return a.ctypes.data + (-a.ctypes.data) % 16

    def new_geoms(geoms):
        arr = (api._Geometry * len(geoms))(*[api._Geometry(*g) for g in geoms])
        h = L.bsx_new_geoms(model.encode(), 2, arr, len(geoms), dev, dbg, none, none, none, None)
        if not h:
            print(json.dumps({"error": "bsx_new_geoms failed: %s" % msgs}))
            sys.exit(0)
        return h

    def geom_info(c):
        out = []
        for g in range(L.bsx_geom_count(c)):
            gi = api._GeomInfo()
            assert L.bsx_get_geom_info(c, g, C.byref(gi)) == 0
            out.append({k: (list(getattr(gi, k)) if k in ("roi", "in_roi") else getattr(gi, k)) for k, _ in api._GeomInfo._fields_})
        return out

    class Batch:
        """positions for the given stream ids: frame (2 or 3 bytes per pixel by the item's format bit), output and background of each; out_px: the vcam size"""
        def __init__(self, c, ids, flags_of, out_px=None, och=3):
            info = geom_info(c)
            self.n = len(ids)
            self.ids = (C.c_int * self.n)(*ids)
            self.items = (api._GeomItem * self.n)()
            for i, s in enumerate(ids):
                g = [q for q in info if q["first_stream"] <= s < q["first_stream"] + q["n_streams"]][0]
                px = g["width"] * g["height"]
                fl = flags_of(i)
                self.items[i].d_frame, self.items[i].d_out = buf(px * (2 if fl & YIN else 3)), buf((out_px or px) * och)
                self.items[i].setting.d_bg, self.items[i].setting.flags = buf(px * 3), fl

    def run(key, c, fn):
        first = log_lines()
        rc = fn()
        calls[key] = {"rc": rc, "error": (L.bsx_last_error(c) or b"").decode(errors="replace").strip(), "log": [first, log_lines()]}

    def geoms(key, c, b, flags=0):
        run(key, c, lambda: L.bsx_step_batch_geoms(c, b.ids, b.items, b.n, None, flags))

    def vcam(key, c, b, ow, oh, flags=0):
        run(key, c, lambda: L.bsx_step_batch_vcam_geoms(c, b.ids, b.items, b.n, ow, oh, None, flags))

    c3 = new_geoms([(640, 480, 2), (1280, 720, 2), (640, 360, 2)])
    cycle = [0, FLIP_H, OFF, 0, FLIP_H | OFF, 0]
    geoms("bgr", c3, Batch(c3, INTER, lambda i: cycle[i]))
    geoms("one_yuyv", c3, Batch(c3, INTER, lambda i: cycle[i] | (YIN if i == 3 else 0)))
    geoms("all_yuyv", c3, Batch(c3, INTER, lambda i: cycle[i] | YIN))
    geoms("all_yuyv_yuyv_out", c3, Batch(c3, INTER, lambda i: cycle[i] | YIN, och=2), flags=YUYV)
    geoms("bgr_again", c3, Batch(c3, INTER, lambda i: cycle[i]))
    vcam("v_bgr", c3, Batch(c3, INTER, lambda i: cycle[i], out_px=426 * 240), 426, 240)
    vcam("v_mixed", c3, Batch(c3, INTER, lambda i: cycle[i] | (YIN if i % 2 else 0), out_px=426 * 240), 426, 240)
    vcam("v_mixed_yuyv_out", c3, Batch(c3, INTER, lambda i: cycle[i] | (YIN if i % 2 else 0), out_px=426 * 240, och=2), 426, 240, flags=YUYV)

    # refusals: the batch flag; an output over the last bytes of a YUYV frame, and right behind it
    geoms("r_batch_flag", c3, Batch(c3, INTER, lambda i: 0), flags=YUYV_IN)
    vcam("r_v_batch_flag", c3, Batch(c3, INTER, lambda i: 0, out_px=426 * 240), 426, 240, flags=YUYV_IN)
    for key, fn, shift in (("r_overlap", geoms, -4), ("behind", geoms, 0), ("r_v_overlap", None, -4), ("v_behind", None, 0)):
        b = Batch(c3, [0, 3], lambda i: YIN, out_px=None if fn else 320 * 240)
        whole = buf(640 * 480 * 2 + 640 * 480 * 3)
        b.items[0].d_frame, b.items[0].d_out = whole, whole + 640 * 480 * 2 + shift
        if fn:
            geoms(key, c3, b)
        else:
            vcam(key, c3, b, 320, 240)
    # a BGR frame's extent is still W * H * 3: an output behind its first W * H * 2 bytes overlaps it
    b = Batch(c3, [0, 3], lambda i: 0)
    whole = buf(640 * 480 * 2 + 640 * 480 * 3)
    b.items[0].d_frame, b.items[0].d_out = whole, whole + 640 * 480 * 2
    geoms("r_bgr_extent", c3, b)

    # a class whose down-scale is the exact 2x2 area mean (256x192 -> segm_lite's 128x96)
    ca = new_geoms([(640, 480, 1), (256, 192, 1)])
    infos = {"c3": geom_info(c3), "ca": geom_info(ca)}
    geoms("r_area", ca, Batch(ca, [0, 1], lambda i: YIN))
    vcam("r_v_area", ca, Batch(ca, [0, 1], lambda i: YIN, out_px=320 * 240), 320, 240)
    geoms("area_as_bgr", ca, Batch(ca, [0, 1], lambda i: YIN if i == 0 else 0))
    # the mixed steps refuse the bit in a setting
    cm = L.bsx_new(model.encode(), 2, 640, 480, 2, dev, dbg, none, none, none, None)
    st = (api._StreamSetting * 1)()
    st[0].d_bg, st[0].flags = buf(640 * 480 * 3), YIN
    fr, out = buf(640 * 480 * 3), buf(640 * 480 * 3)
    run("r_mixed", cm, lambda: L.bsx_step_batch_mixed(cm, None, fr, st, out, 1, None, 0))
    run("r_vcam_mixed", cm, lambda: L.bsx_step_batch_vcam_mixed(cm, None, fr, st, out, 320, 240, 1, None, 0))
    for c in (c3, ca, cm):
        L.bsx_delete(c)
    print(json.dumps({"calls": calls, "infos": infos}))


if __name__ == "__main__":
    main()
