"""The ONE check of the five multi-geometry steps (csrc/geoms_request.hpp), driven by a stand-alone program built with the host sanitizers — no GPU, no library, no
frame memory: the pointers of a case are numbers the check only compares.  Per entry kind: every refusal it can give with its exact text (the literals are the format
strings of the five checks this header replaced), an accepted call and what it leaves behind, the precedence of the rules, and the overlap sweep at its boundaries.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")

MAIN = r"""
// One case per line on stdin:
//   kind n ids[n] flags pending onmask out_w out_h m items_null  then n items "a b pitch_y pitch_uv bg sflags" (a = d_frame | d_y, b = d_out | d_uv)  then m records
//   "item w h a b pitch_y pitch_uv" (a = d_out | d_y, b = d_uv).  Prints "0 c=<class of each item> s=<spans> o=<order of the records> f=<d_frame of the front
//   items>", "1 <text>" or "2" per case.
#include <cstdio>
#include "geoms_request.hpp"
using namespace bsx;
static const uint8_t* ptr(unsigned long long v) { return reinterpret_cast<const uint8_t*>((uintptr_t)v); }
int main() {
  // streams 0-1: 16 x 8; 2-3: 32 x 16; 4: 16 x 8 off the tile route; 5: 32 x 16 with the copy table; 6: 15 x 8 (linear, no YUYV prep); 7: 32 x 16 with the 2x2 table; 8: 3 x 1
  static const GeomsClass classes[7] = {{0, 16, 8, true, 0, 0, 16, 8, true}, {2, 32, 16, true, 0, 0, 32, 16, true}, {4, 16, 8, false, 0, 2, 12, 8, true},
                                        {5, 32, 16, true, 1, 0, 32, 16, false}, {6, 15, 8, true, 0, 1, 14, 8, false}, {7, 32, 16, true, 2, 0, 32, 16, false},
                                        {8, 3, 1, true, 0, 0, 3, 1, true}};
  int kind;
  GeomsChecked out;                                                   // kept between the cases, as a context keeps it
  while (scanf("%d", &kind) == 1) {
    GeomsRequest q{};
    q.kind = (GeomsKind)kind; q.classes = classes; q.n_classes = 7;
    int pending, onmask, null_items;
    if (scanf("%d", &q.n) != 1) return 2;
    int* ids = new int[(size_t)q.n];                                  // exactly n, on the heap: a read past them is the sanitizer's to report
    for (int i = 0; i < q.n; i++) if (scanf("%d", &ids[i]) != 1) return 2;
    if (scanf("%u %d %d %d %d %d %d", &q.flags, &pending, &onmask, &q.out_w, &q.out_h, &q.m, &null_items) != 7) return 2;
    q.ids = ids; q.pending = pending != 0; q.onmask = onmask != 0;
    const bool surface = q.kind == GeomsKind::Surfaces, nv12 = surface || q.kind == GeomsKind::VcamOutsNv12;
    bsx_geom_item* items = new bsx_geom_item[(size_t)q.n]();
    bsx_surface_item* surfaces = new bsx_surface_item[(size_t)q.n]();
    for (int i = 0; i < q.n; i++) {
      unsigned long long a, b, bg;
      int py, puv;
      unsigned f;
      if (scanf("%llu %llu %d %d %llu %u", &a, &b, &py, &puv, &bg, &f) != 6) return 2;
      items[i].d_frame = ptr(a); items[i].d_out = const_cast<uint8_t*>(ptr(b)); items[i].setting.d_bg = ptr(bg); items[i].setting.flags = f;
      surfaces[i].d_y = ptr(a); surfaces[i].d_uv = ptr(b); surfaces[i].pitch_y = py; surfaces[i].pitch_uv = puv; surfaces[i].setting = items[i].setting;
    }
    const int m = q.m > 0 ? q.m : 0;
    bsx_vcam_out* outs = new bsx_vcam_out[(size_t)m]();
    bsx_vcam_out_nv12* outs_nv12 = new bsx_vcam_out_nv12[(size_t)m]();
    for (int j = 0; j < m; j++) {
      unsigned long long a, b;
      bsx_vcam_out_nv12& o = outs_nv12[j];
      if (scanf("%d %d %d %llu %llu %d %d", &o.item, &o.out_w, &o.out_h, &a, &b, &o.pitch_y, &o.pitch_uv) != 7) return 2;
      o.d_y = const_cast<uint8_t*>(ptr(a)); o.d_uv = const_cast<uint8_t*>(ptr(b));
      outs[j] = bsx_vcam_out{o.item, o.out_w, o.out_h, o.d_y};
    }
    if (!null_items) { if (surface) q.surfaces = surfaces; else q.items = items; }
    if (nv12) q.outs_nv12 = outs_nv12; else if (q.kind == GeomsKind::VcamOuts) q.outs = outs;
    const int rc = geoms_check(q, &out);
    if (rc == GeomsChecked::kRefused) printf("1 %s\n", out.why.text);
    else if (rc == GeomsChecked::kTooLarge) printf("2\n");
    else {
      printf("0 c=");
      for (int i = 0; i < q.n; i++) printf("%d,", out.item_class[(size_t)i]);
      printf(" s=%zu o=", out.spans.size());
      if (geoms_kind(q.kind).records != GeomsRecords::None) for (int v : out.plan.order) printf("%d,", v);
      printf(" f=");
      if (surface) for (int i = 0; i < q.n; i++) printf("%llx,", (unsigned long long)(uintptr_t)out.front_items[(size_t)i].d_frame);
      printf("\n");
    }
    delete[] ids; delete[] items; delete[] surfaces; delete[] outs; delete[] outs_nv12;
  }
  return 0;
}
"""

GEOMS, VCAM, OUTS, NV12, SURF = range(5)
KINDS = [GEOMS, VCAM, OUTS, NV12, SURF]
FN = ["geoms", "vcam_geoms", "vcam_geoms_outs", "vcam_geoms_outs_nv12", "surfaces"]
# buffers 64 KiB apart: frames (for a surface: its Y plane), per-item outputs (for a surface: its UV plane), backgrounds, record outputs (Y, then UV)
F, O, B, R, RU = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
STEP = 0x10000
W_OF = {0: (16, 8), 1: (16, 8), 2: (32, 16), 3: (32, 16), 4: (16, 8), 5: (32, 16), 6: (15, 8), 7: (32, 16), 8: (3, 1)}
YUYV_IN_TEXT = ("flags 0x%x: YUYV input frames are not taken by the multi-geometry step as a batch flag (the format belongs to the item: the yuyv-in bit, 0x40, of "
                "items[i].setting.flags)")
PENDING = "a pipelined composite is pending (flush with bsx_step_batch_pipelined(ctx, NULL, ...) first)"
ONMASK = ["needs the fused mask + blend route (no onmask callback)"] + ["needs the fused mask route (no onmask callback)"] * 4
UNFUSABLE = "items[%d]: stream %d is of class %d (%d x %d), which is off the fused tile route (width, roi.x, roi.w multiples of 4, a tiled linear mask up-scale)"


class Call:
    """a call of `kind` for the given stream ids: well-formed unless a test changes it"""

    def __init__(self, kind, ids=(0, 2), m=None):
        self.kind, self.ids, self.flags, self.pending, self.onmask, self.null_items = kind, list(ids), 0, 0, 0, 0
        self.out_w, self.out_h = (24, 10) if kind == VCAM else (0, 0)
        self.items = []
        for i, s in enumerate(ids):
            w = W_OF[s][0]
            pitch = (w + 3) & ~3
            self.items.append(dict(a=F + i * STEP, b=O + i * STEP, py=pitch, puv=pitch, bg=B + i * STEP, f=0))
        self.outs = []
        if kind in (OUTS, NV12, SURF):
            for j in range(len(ids) if m is None else m):
                self.outs.append(dict(item=j % len(ids), w=8, h=4, a=R + j * STEP, b=RU + j * STEP, py=8, puv=8))
        self.m = None

    def line(self):
        v = [self.kind, len(self.ids)] + self.ids + [self.flags, self.pending, self.onmask, self.out_w, self.out_h, len(self.outs) if self.m is None else self.m,
                                                      self.null_items]
        for it in self.items:
            v += [it["a"], it["b"], it["py"], it["puv"], it["bg"], it["f"]]
        for o in self.outs if self.m is None else []:
            v += [o["item"], o["w"], o["h"], o["a"], o["b"], o["py"], o["puv"]]
        return " ".join(str(x) for x in v)


CASES = []          # (name, Call, expected line)


def case(name, call, want):
    CASES.append((name, call, want if want in ("2",) or want.startswith("0 ") else "1 " + want))


def bad_flags(c):
    c.flags = 4 if c.kind == GEOMS else 8 if c.kind in (VCAM, OUTS) else 1
    return {GEOMS: "flags 0x4 has bits outside yuyv / no-mask", VCAM: "unsupported flags 0x8 (the no-mask step has no vcam form)",
            OUTS: "unsupported flags 0x8 (the no-mask step has no vcam form)",
            NV12: "flags 0x1: this step takes no flags (an item's format and flips belong to items[i].setting.flags)",
            SURF: "flags 0x1: this step takes no flags (an item's flips belong to items[i].setting.flags)"}[c.kind]


def bad_item(c, i):
    c.items[i]["f"] = 0x700
    return "items[%d]: setting flags 0x700 asks for a background blur, which the multi-geometry step does not take" % i


def bad_plan(c):
    c.outs[1]["item"] = 9
    return "outs[1]: item 9 is outside [0, %d)" % len(c.ids)


def overlap(c):
    """an output on items[1]'s background; the text"""
    if c.kind in (GEOMS, VCAM):
        c.items[0]["b"] = c.items[1]["bg"]
        return "items[0]: d_out 0x%x overlaps a frame or background of items[1] (0x%x)" % (c.items[1]["bg"], c.items[1]["bg"])
    c.outs[0]["a"] = c.items[1]["bg"]
    if c.kind == OUTS:
        return "outs[0]: d_out 0x%x overlaps a frame or background of items[1] (0x%x)" % (c.items[1]["bg"], c.items[1]["bg"])
    return "outs[0]: d_y 0x%x overlaps %s of items[1] (0x%x)" % (c.items[1]["bg"], "setting.d_bg" if c.kind == SURF else "a frame or background", c.items[1]["bg"])


def accepted(c):
    spans = 0
    for it in c.items:
        spans += (2 if c.kind == SURF else 1) + (1 if c.kind in (GEOMS, VCAM) else 0) + (0 if it["f"] & 32 else 1)
    spans += len(c.outs) * (2 if c.kind in (NV12, SURF) else 1)
    cls = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 3, 6: 4, 7: 5, 8: 6}
    order = sorted(range(len(c.outs)), key=lambda j: (cls[c.ids[c.outs[j]["item"]]], (c.outs[j]["w"], c.outs[j]["h"]) != (c.outs[0]["w"], c.outs[0]["h"])))
    return "0 c=%s s=%d o=%s f=%s" % ("".join("%d," % cls[s] for s in c.ids), spans, "".join("%d," % j for j in order),
                                      "".join("%x," % it["a"] for it in c.items) if c.kind == SURF else "")


def build_cases():
    for k in KINDS:
        n = FN[k]
        # ---- accepted calls, and what they leave --------------------------------------------------------------------------------------------------------------
        case(n + ":accepted", Call(k), accepted(Call(k)))
        c = Call(k, ids=(3, 0, 1))                                    # the class of each item, the records ordered by the class of their item
        case(n + ":accepted_three", c, accepted(c))
        c = Call(k)                                                   # a filter_off item: its d_bg is neither looked at ...
        c.items[0]["f"], c.items[0]["bg"] = 32 | 2, 3
        case(n + ":filter_off_bg_ignored", c, accepted(c))
        c = Call(k)                                                   # ... nor part of the overlap sweep
        c.items[0]["f"] = 32
        overlap_target = c.items[0]["bg"]
        if k in (GEOMS, VCAM):
            c.items[1]["b"] = overlap_target
        else:
            c.outs[0]["a"] = overlap_target
        case(n + ":filter_off_bg_no_overlap", c, accepted(c))
        # ---- the call's own rules ------------------------------------------------------------------------------------------------------------------------------
        c = Call(k)
        c.null_items = 1
        case(n + ":items_null", c, "items is NULL")
        c = Call(k)
        case(n + ":flags", c, bad_flags(c))
        if k in (GEOMS, VCAM, OUTS):
            c = Call(k)
            c.flags = 16
            case(n + ":flag_yuyv_in", c, YUYV_IN_TEXT % 16)
        if k in (VCAM, OUTS):
            c = Call(k)
            c.flags = 2
            case(n + ":flag_outside", c, "flags 0x2 has bits outside yuyv")
        c = Call(k)
        c.pending = 1
        case(n + ":pending", c, PENDING)
        c = Call(k)
        c.onmask = 1
        case(n + ":onmask", c, ONMASK[k])
        # ---- the rules of an item ------------------------------------------------------------------------------------------------------------------------------
        c = Call(k)
        case(n + ":item_blur", c, bad_item(c, 1))
        c = Call(k)
        c.items[1]["f"] = 0x10000
        case(n + ":item_stray", c, "items[1]: setting flags 0x10000 has bits outside flip / filter-off" + ("" if k == SURF else " / yuyv-in"))
        a, b = ("d_y", "d_uv") if k == SURF else ("d_frame", "d_out")
        c = Call(k)
        c.items[1]["a"] = 0
        case(n + ":item_a_null", c, "items[1]: %s is NULL" % a)
        c = Call(k)
        c.items[1]["a"] += 2
        case(n + ":item_a_unaligned", c, "items[1]: %s 0x%x is not 4-byte aligned" % (a, c.items[1]["a"]))
        if k in (GEOMS, VCAM, SURF):
            c = Call(k)
            c.items[0]["b"] = 0
            case(n + ":item_b_null", c, "items[0]: %s is NULL" % b)
            c = Call(k)
            c.items[0]["b"] += 1
            case(n + ":item_b_unaligned", c, "items[0]: %s 0x%x is not 4-byte aligned" % (b, c.items[0]["b"]))
        else:                                                         # d_out is not read where the outputs are records
            c = Call(k)
            c.items[0]["b"] = 1
            case(n + ":item_d_out_not_read", c, accepted(c))
        c = Call(k, ids=(0, 4))
        case(n + ":item_unfusable", c, UNFUSABLE % (1, 4, 2, 16, 8) + ("; bsx_step_batch_vcam_mixed takes such a context" if k == VCAM else ""))
        c = Call(k)
        c.items[1]["bg"] = 0
        case(n + ":item_bg_null", c, "items[1]: setting.d_bg is NULL")
        c = Call(k)
        c.items[1]["bg"] += 3
        case(n + ":item_bg_unaligned", c, "items[1]: setting.d_bg 0x%x is not 4-byte aligned" % c.items[1]["bg"])
        if k == SURF:
            c = Call(k)
            c.items[0]["f"] = 0x42
            case(n + ":item_yuyv_bit", c, "items[0]: setting flags 0x42 has the yuyv-in bit: every frame of this call is an NV12 surface")
            for key, v, text in (("py", 12, "items[1]: pitch_y = 12 is below the width 32 of its class"), ("py", 34, "items[1]: pitch_y = 34 is not a multiple of 4"),
                                 ("puv", -32, "items[1]: pitch_uv = -32 is below the width 32 of its class"), ("puv", 38, "items[1]: pitch_uv = 38 is not a multiple of 4"),
                                 ("py", 1 << 28, "items[1]: pitch_y = 268435456, pitch_uv = 32 at 16 rows: a plane of 2 GiB or more")):
                c = Call(k)
                c.items[1][key] = v
                case(n + ":item_%s_%d" % (key, v), c, text)
            pre = "items[1]: stream %d is of class %d (%d x %d), which has no fused NV12 prep: "
            post = "; convert such surfaces with bsx_nv12_to_bgr"
            for s, text in ((5, pre % (5, 3, 32, 16) + "its down-scale table is a copy (capture ROI 32 x 16 = model ROI)" + post),
                            (7, pre % (7, 5, 32, 16) + "its down-scale table is the 2x2 area mean (capture ROI 32 x 16 = twice the model ROI)" + post),
                            (6, pre % (6, 4, 15, 8) + "NV12 needs an even width and height" + post)):
                c = Call(k, ids=(0, s))
                case(n + ":class_%d" % s, c, text)
        else:
            pre = "items[1]: stream %d is of class %d (%d x %d), which has no fused YUYV prep: "
            post = "; convert that stream's frames with bsx_yuyv_to_bgr and pass them as BGR"
            for s, text in ((5, pre % (5, 3, 32, 16) + "its down-scale table is a copy (capture ROI 32 x 16 = model ROI)" + post),
                            (7, pre % (7, 5, 32, 16) + "its down-scale table is the 2x2 area mean (capture ROI 32 x 16 = twice the model ROI)" + post),
                            (6, pre % (6, 4, 15, 8) + "its down-scale table is linear but width 15 and roi.x 1 must be even and the ROI row at least 4 pixels" + post)):
                c = Call(k, ids=(0, s))
                c.items[1]["f"] = 64
                case(n + ":yuyv_class_%d" % s, c, text)
                c = Call(k, ids=(0, s))                               # a BGR item of such a class is taken
                case(n + ":bgr_class_%d" % s, c, accepted(c))
            c = Call(k)                                               # a YUYV item: its frame is 2 bytes a pixel (the output of items[1] right behind it)
            c.items[0]["f"] = 64
            case(n + ":yuyv_item", c, accepted(c))
        # ---- precedence: of two broken rules the earlier one is reported --------------------------------------------------------------------------------------
        c = Call(k)
        c.null_items = 1
        if k == VCAM:
            c.out_w = 0
        else:
            bad_flags(c)
        case(n + ":null_before_next", c, "items is NULL")
        c = Call(k)
        want = bad_flags(c)
        c.pending = 1
        case(n + ":flags_before_pending", c, want)
        c = Call(k)
        c.pending = c.onmask = 1
        case(n + ":pending_before_onmask", c, PENDING)
        c = Call(k)
        c.onmask = 1
        bad_item(c, 0)
        if k == VCAM:
            c.flags, c.out_w = 1, 25
        case(n + ":onmask_before_next", c, ONMASK[k])
        c = Call(k)
        bad_item(c, 1)
        c.items[0]["a"] = 0
        case(n + ":items_in_index_order", c, "items[0]: %s is NULL" % a)
        c = Call(k)                                                   # within an item: the bits before the pointers, the frame before the background
        want = bad_item(c, 0)
        c.items[0]["a"] = c.items[0]["bg"] = 0
        case(n + ":item_rules_in_order", c, want)
        c = Call(k)
        want = bad_item(c, 1)
        if k in (OUTS, NV12, SURF):
            bad_plan(c)
            case(n + ":item_before_plan", c, want)
            c = Call(k)
            want = bad_plan(c)
            overlap(c)
            case(n + ":plan_before_overlap", c, want)
        else:
            overlap(c)
            case(n + ":item_before_overlap", c, want)
        # ---- overlaps ------------------------------------------------------------------------------------------------------------------------------------------
        c = Call(k)
        case(n + ":overlap_background", c, overlap(c))

    # ---- rules of one kind -------------------------------------------------------------------------------------------------------------------------------------
    c = Call(VCAM)
    c.out_w = 0
    case("vcam:out_size", c, "output size 0 x 10 must be positive")
    c = Call(VCAM)
    c.out_h, c.flags = -1, 8
    case("vcam:out_size_before_flags", c, "output size 24 x -1 must be positive")
    c = Call(VCAM)
    c.flags, c.out_w = 1, 25
    case("vcam:yuyv_odd", c, "YUYV output needs an even width (out_w = 25)")
    c = Call(VCAM)
    c.flags, c.out_w = 1, 25
    bad_item(c, 0)
    case("vcam:yuyv_odd_before_items", c, "YUYV output needs an even width (out_w = 25)")
    c = Call(GEOMS, ids=(0, 6))
    c.flags = 1
    case("geoms:yuyv_odd_class", c, "items[1]: YUYV output needs an even width (stream 6 is of class 4, 15 x 8)")
    c = Call(GEOMS, ids=(0, 6))                                       # (BGR out: an odd class is taken)
    case("geoms:bgr_odd_class", c, accepted(c))
    c = Call(GEOMS)
    c.flags = 1 | 8
    case("geoms:yuyv_no_mask", c, accepted(c))
    for k in (OUTS, NV12, SURF):                                      # the planners' refusals arrive unchanged; a grid of 2^31 workgroups is not a refusal
        c = Call(k)
        c.m = -1
        case(FN[k] + ":m_negative", c, "m = -1 is negative")
        c = Call(k)
        case(FN[k] + ":plan_item", c, bad_plan(c))
        c = Call(k, m=0)                                              # no record: every stream still advances
        case(FN[k] + ":no_record", c, accepted(c))
    c = Call(OUTS)
    c.flags, c.outs[0]["w"] = 1, 9
    case("vcam_geoms_outs:plan_yuyv_odd", c, "outs[0]: YUYV output needs an even width (out_w = 9)")
    c = Call(NV12)
    c.outs[1]["py"] = 6
    case("vcam_geoms_outs_nv12:plan_pitch", c, "outs[1]: pitch_y = 6 is below out_w = 8")
    c = Call(OUTS, m=4)                                               # 4 records of 2^14 x 2^15 tiles
    for o in c.outs:
        o["w"], o["h"] = 1 << 20, 1 << 20
    case("vcam_geoms_outs:too_large", c, "2")

    # ---- overlaps, at the boundaries: a destination may touch, not share a byte ---------------------------------------------------------------------------------
    for k in (GEOMS, VCAM):
        out_bytes = 24 * 10 * 3 if k == VCAM else None
        c = Call(k)                                                   # ... against another item's frame: items[1]'s output ends where items[0]'s frame begins
        ob = out_bytes or 32 * 16 * 3
        c.items[1]["b"] = c.items[0]["a"] - ob
        case(FN[k] + ":touch_frame", c, accepted(c))
        c = Call(k)
        c.items[1]["b"] = c.items[0]["a"] - ob + 4
        case(FN[k] + ":overlap_frame", c, "items[1]: d_out 0x%x overlaps a frame or background of items[0] (0x%x)" % (c.items[1]["b"], c.items[0]["a"]))
        c = Call(k)                                                   # ... against another output: the one that begins later is named
        ob0 = out_bytes or 16 * 8 * 3
        c.items[1]["b"] = c.items[0]["b"] + ob0
        case(FN[k] + ":touch_output", c, accepted(c))
        c = Call(k)
        c.items[1]["b"] = c.items[0]["b"] + ob0 - 4
        case(FN[k] + ":overlap_output", c, "items[1]: d_out 0x%x overlaps the output of items[0] (0x%x)" % (c.items[1]["b"], c.items[0]["b"]))
        c = Call(k, ids=(8, 0))                                       # a single byte: the 3 x 1 frame of stream 8 is 9 bytes
        c.items[1]["b"] = c.items[0]["a"] + 8
        case(FN[k] + ":overlap_one_byte", c, "items[1]: d_out 0x%x overlaps a frame or background of items[0] (0x%x)" % (c.items[1]["b"], c.items[0]["a"]))
        c = Call(k, ids=(8, 0))
        c.items[1]["b"] = c.items[0]["a"] + 12
        case(FN[k] + ":no_overlap_past_the_byte", c, accepted(c))
        c = Call(k, ids=(8, 0))                                       # the same for its background
        c.items[1]["b"] = c.items[0]["bg"] + 8
        case(FN[k] + ":overlap_one_byte_bg", c, "items[1]: d_out 0x%x overlaps a frame or background of items[0] (0x%x)" % (c.items[1]["b"], c.items[0]["bg"]))
        c = Call(k)                                                   # a YUYV frame is judged on 2 bytes a pixel
        c.items[0]["f"] = 64
        c.items[1]["b"] = c.items[0]["a"] + 16 * 8 * 2
        case(FN[k] + ":touch_yuyv_frame", c, accepted(c))
        c = Call(k)
        c.items[1]["b"] = c.items[0]["a"] + 16 * 8 * 2
        case(FN[k] + ":overlap_bgr_frame", c, "items[1]: d_out 0x%x overlaps a frame or background of items[0] (0x%x)" % (c.items[1]["b"], c.items[0]["a"]))
    c = Call(GEOMS)                                                   # YUYV out: an output is judged on 2 bytes a pixel
    c.flags = 1
    c.items[1]["b"] = c.items[0]["b"] + 16 * 8 * 2
    case("geoms:touch_yuyv_output", c, accepted(c))

    c = Call(OUTS)                                                    # records of 8 x 4 BGR: 96 bytes
    c.outs[1]["a"] = c.items[0]["a"] - 96
    case("vcam_geoms_outs:touch_frame", c, accepted(c))
    c = Call(OUTS)
    c.outs[1]["a"] = c.items[0]["a"] - 92
    case("vcam_geoms_outs:overlap_frame", c, "outs[1]: d_out 0x%x overlaps a frame or background of items[0] (0x%x)" % (c.outs[1]["a"], c.items[0]["a"]))
    c = Call(OUTS)
    c.outs[1]["a"] = c.outs[0]["a"] + 96
    case("vcam_geoms_outs:touch_output", c, accepted(c))
    c = Call(OUTS)
    c.outs[1]["a"] = c.outs[0]["a"] + 92
    case("vcam_geoms_outs:overlap_output", c, "outs[1]: d_out 0x%x overlaps the output of outs[0] (0x%x)" % (c.outs[1]["a"], c.outs[0]["a"]))
    c = Call(OUTS)                                                    # a single byte: a 3 x 1 BGR record is 9 bytes
    c.outs[0]["w"], c.outs[0]["h"] = 3, 1
    c.items[1]["a"] = c.outs[0]["a"] + 8
    case("vcam_geoms_outs:overlap_one_byte", c, "outs[0]: d_out 0x%x overlaps a frame or background of items[1] (0x%x)" % (c.outs[0]["a"], c.items[1]["a"]))
    c = Call(OUTS)
    c.outs[0]["w"], c.outs[0]["h"] = 3, 1
    c.items[1]["a"] = c.outs[0]["a"] + 12
    case("vcam_geoms_outs:no_overlap_past_the_byte", c, accepted(c))
    c = Call(OUTS)                                                    # YUYV records of 8 x 4: 64 bytes
    c.flags = 1
    c.outs[1]["a"] = c.outs[0]["a"] + 64
    case("vcam_geoms_outs:touch_yuyv_output", c, accepted(c))

    for k in (NV12, SURF):
        n = FN[k]
        c = Call(k)                                                   # a pitched plane: 4 rows of 8 bytes, 16 apart, end at 16 * 3 + 8 = 56, not at 16 * 4
        c.outs[0]["py"] = 16
        c.outs[1]["a"] = c.outs[0]["a"] + 56
        case(n + ":touch_pitched_y", c, accepted(c))
        c = Call(k)
        c.outs[0]["py"] = 16
        c.outs[1]["a"] = c.outs[0]["a"] + 52
        case(n + ":overlap_pitched_y", c, "outs[1]: d_y 0x%x overlaps d_y of outs[0] (0x%x)" % (c.outs[1]["a"], c.outs[0]["a"]))
        c = Call(k)                                                   # ... its chroma plane: 2 rows, end at 16 + 8
        c.outs[0]["puv"] = 16
        c.outs[1]["a"] = c.outs[0]["b"] + 24
        case(n + ":touch_pitched_uv", c, accepted(c))
        c = Call(k)                                                   # a d_uv plane against a d_y plane, both ways round
        c.outs[0]["puv"] = 16
        c.outs[1]["a"] = c.outs[0]["b"] + 20
        case(n + ":overlap_y_on_uv", c, "outs[1]: d_y 0x%x overlaps d_uv of outs[0] (0x%x)" % (c.outs[1]["a"], c.outs[0]["b"]))
        c = Call(k)
        c.outs[0]["b"] = c.outs[1]["a"] + 28                          # outs[1]'s Y plane: 8 * 3 + 8 = 32 bytes
        case(n + ":overlap_uv_on_y", c, "outs[0]: d_uv 0x%x overlaps d_y of outs[1] (0x%x)" % (c.outs[0]["b"], c.outs[1]["a"]))
        c = Call(k)
        c.outs[0]["b"] = c.outs[0]["a"] + 32                          # a surface in one allocation: the chroma plane right behind the luma plane
        case(n + ":uv_behind_y", c, accepted(c))
        c = Call(k)
        c.outs[0]["b"] = c.outs[0]["a"] + 28
        case(n + ":overlap_own_planes", c, "outs[0]: d_uv 0x%x overlaps d_y of outs[0] (0x%x)" % (c.outs[0]["b"], c.outs[0]["a"]))
        c = Call(k)                                                   # against an item's frame (for a surface: its Y plane, 8 rows of 16)
        c.outs[1]["b"] = c.items[0]["a"] - 16
        case(n + ":touch_frame", c, accepted(c))
        c = Call(k)
        c.outs[1]["b"] = c.items[0]["a"] - 12
        case(n + ":overlap_frame", c, "outs[1]: d_uv 0x%x overlaps %s of items[0] (0x%x)" % (c.outs[1]["b"], "d_y" if k == SURF else "a frame or background", c.items[0]["a"]))
    c = Call(SURF)                                                    # an input plane is judged on pitch * (rows - 1) + W: 32 * 7 + 16 = 240 for Y, 32 * 3 + 16 = 112 for UV
    c.items[0]["py"] = c.items[0]["puv"] = 32
    c.outs[0]["a"], c.outs[1]["a"] = c.items[0]["a"] + 240, c.items[0]["b"] + 112
    case("surfaces:touch_pitched_inputs", c, accepted(c))
    c = Call(SURF)
    c.items[0]["py"] = 32
    c.outs[0]["a"] = c.items[0]["a"] + 236
    case("surfaces:overlap_pitched_y_in", c, "outs[0]: d_y 0x%x overlaps d_y of items[0] (0x%x)" % (c.outs[0]["a"], c.items[0]["a"]))
    c = Call(SURF)
    c.items[1]["puv"] = 64
    c.outs[0]["a"] = c.items[1]["b"] + 64 * 7 + 28
    case("surfaces:overlap_pitched_uv_in", c, "outs[0]: d_y 0x%x overlaps d_uv of items[1] (0x%x)" % (c.outs[0]["a"], c.items[1]["b"]))
    c = Call(NV12)                                                    # a BGR frame of 16 x 8: 384 bytes
    c.outs[0]["a"] = c.items[0]["a"] + 384
    case("vcam_geoms_outs_nv12:touch_frame_end", c, accepted(c))
    c = Call(NV12)
    c.outs[0]["a"] = c.items[0]["a"] + 380
    case("vcam_geoms_outs_nv12:overlap_frame_end", c, "outs[0]: d_y 0x%x overlaps a frame or background of items[0] (0x%x)" % (c.outs[0]["a"], c.items[0]["a"]))


build_cases()


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("geoms_request")
    src, exe = tmp / "main.cpp", str(tmp / "request")
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-o", exe, str(src)])
    text = "\n".join(c.line() for _n, c, _w in CASES) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "the program failed (a sanitizer report?):\n" + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert len(lines) == len(CASES) + 1, r.stdout[-500:]
    return lines


def test_every_case_of_every_kind(answers):
    assert len({name for name, _c, _w in CASES}) == len(CASES)
    wrong = [(name, got, want) for (name, _c, want), got in zip(CASES, answers) if got != want]
    assert not wrong, "\n".join("%s:\n  got  %s\n  want %s" % w for w in wrong[:10])


@pytest.mark.parametrize("kind", KINDS, ids=FN)
def test_each_kind_refuses_accepts_and_orders_its_rules(answers, kind):
    """the sets of the module's cases that the issue asks for exist for every kind, and hold"""
    mine = {name.split(":", 1)[1]: (got, want) for (name, c, want), got in zip(CASES, answers) if c.kind == kind}
    for key in ("accepted", "items_null", "flags", "pending", "onmask", "item_blur", "item_bg_null", "null_before_next", "flags_before_pending", "pending_before_onmask",
                "onmask_before_next", "items_in_index_order", "overlap_background", "filter_off_bg_ignored", "filter_off_bg_no_overlap"):
        got, want = mine[key]
        assert got == want, (key, got, want)
    assert mine["accepted"][0].startswith("0 ")
    assert ("item_before_plan" in mine and "plan_before_overlap" in mine) or "item_before_overlap" in mine


def test_no_text_names_a_macro(answers):
    assert sum(1 for line in answers if line.startswith("1 ")) > 100
    for line in answers:
        assert "BSX_" not in line
