"""bsx_step_batch_surfaces and bsx_nv12_to_bgr on a box without a GPU:
  * header, both libraries, version script and binding agree on the two symbols; ctypes' bsx_surface_item has the size and offsets of the struct compiled from the
    header;
  * MaskGen.step_surfaces and MaskGen.nv12_to_bgr validate their arguments before the library is reached;
  * the item checks (csrc/vcam_surface_plan.hpp) driven by a stand-alone program built with the host sanitizers: every refusal text, the accepted cases;
  * the library's real host code against tests/hip_stub/libhipstub.so (tests/hip_stub/drive_surfaces.py): the launch list of one call on contexts of 1 and 3
    classes, one copy per ring, no host synchronisation, the refusals — and bsx_step_batch_vcam_geoms_outs_nv12 and bsx_step_batch_geoms still trace what they did;
  * the new kernels' resources (tools/kernel_regs.sh): no scratch, LDS not above vg_outs_nv12_fmt_k's and prep_geoms_fmt_k's of the same build."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, model_path

STEP, CONV = "bsx_step_batch_surfaces", "bsx_nv12_to_bgr"
CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
STUB_DIR = os.path.join(ROOT, "tests", "hip_stub")
STUB = os.path.join(STUB_DIR, "libhipstub.so")
BSX_EINVAL = -1
IDS = [4, 0, 2, 5, 1, 3]
LAYERS = [(320, 180), (160, 90)]


# ---- 1. the symbols and the item ---------------------------------------------------------------------------------------------------------------------------------
def test_header_libraries_and_binding_agree_on_the_symbols(tmp_path):
    from backscrub_amd import api, build
    build.build()
    C = ctypes
    want = {STEP: [C.c_void_p, C.POINTER(C.c_int), C.POINTER(api._SurfaceItem), C.c_int, C.POINTER(api._VcamOutNv12), C.c_int, C.c_void_p, C.c_uint],
            CONV: [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]}
    proto = {STEP: "bsx_ctx* ctx, const int* ids, const bsx_surface_item* items, int n, const bsx_vcam_out_nv12* outs, int m, void* stream, unsigned flags /* 0 */",
             CONV: "bsx_ctx* ctx, const uint8_t* d_y, int pitch_y, const uint8_t* d_uv, int pitch_uv, int w, int h, int n, uint8_t* d_bgr, void* stream"}
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    for sym in (STEP, CONV):
        entry = [s for s in api.SYMBOLS if s[0] == sym]
        assert len(entry) == 1 and entry[0][1] is C.c_int and entry[0][2] == want[sym], sym
        m = re.search(r"^BSX_API int %s\(([^)]*)\);" % sym, hdr, re.M)
        assert m, "the header does not declare %s" % sym
        assert re.sub(r"\s+", " ", m.group(1)) == proto[sym]
    # the version script exports the C ABI by its prefix: the symbols must be in the dynamic table of both builds
    assert re.search(r"global:\s*bsx_\*;", open(os.path.join(CSRC, "libbsx.map")).read())
    for lib in (build.LIB, build.LIB_DBG):
        names = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.split()
        assert STEP in names and CONV in names, lib
    assert hasattr(api.MaskGen, "step_surfaces") and hasattr(api.MaskGen, "nv12_to_bgr")
    # the header's contract: the definition, "believed, not checked", the out-of-scope list; the older list no longer names NV12 input as missing
    assert "Q[y][c] = ( Y[y][2c],  UV[y / 2][2c],  Y[y][2c + 1],  UV[y / 2][2c + 1] )" in hdr and "Believed, not checked" in hdr
    assert "P010 and I420" in hdr and "I420 / three-plane output, NV12 input" not in hdr
    # the item: a struct compiled from the header
    fields = ["d_y", "d_uv", "pitch_y", "pitch_uv", "setting"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bsx.h"\nint main(void) { printf("%zu", sizeof(bsx_surface_item));\n' +
                   "".join('  printf(" %%zu", offsetof(bsx_surface_item, %s));\n' % f for f in fields) +
                   '  printf(" %zu %zu", offsetof(bsx_surface_item, setting.d_bg), offsetof(bsx_surface_item, setting.flags));\n  printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    V = api._SurfaceItem
    assert [f for f, _t in V._fields_] == fields
    S = api._StreamSetting
    assert [C.sizeof(V)] + [getattr(V, f).offset for f in fields] + [V.setting.offset + S.d_bg.offset, V.setting.offset + S.flags.offset] == got == \
        [40, 0, 8, 16, 20, 24, 24, 32]


# ---- 2. the binding's validation ---------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_validates_before_the_library_is_reached():
    torch = pytest.importorskip("torch")
    from backscrub_amd import api

    host = []

    class Fake(api.MaskGen):
        """no context (h is None: a library call would fail loudly); two classes, 16 x 8 and 32 x 16, two streams each; host tensors count as on the device, but
        for the ones listed in `host`"""
        def __init__(self):
            self.h, self.device, self.n_streams = None, 0, 4
            self._geoms = [dict(width=16, height=8, n_streams=2, first_stream=0), dict(width=32, height=16, n_streams=2, first_stream=2)]

        def _on_device(self, t):
            return not any(t is h for h in host)

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8)

    def surface(w, h, pitch_y=None, pitch_uv=None, n=None):
        """(y, uv): views into one allocation laid out as a surface (n: as n surfaces, the planes of each kind one behind the other)"""
        py, puv = pitch_y or (w + 3) // 4 * 4, pitch_uv or (w + 3) // 4 * 4
        k = n or 1
        buf = u8(k * (py * h + puv * (h // 2)) + 64)
        off = (-buf.data_ptr()) % 4
        y = torch.as_strided(buf, (k, h, w), (py * h, py, 1), off)
        uv = torch.as_strided(buf, (k, h // 2, w), (puv * (h // 2), puv, 1), off + k * py * h)
        return (y, uv) if n else (y[0], uv[0])
    mg, S = Fake(), api.StreamSetting
    small, big, off = surface(16, 8, 32, 16), surface(32, 16, 32, 64), S(filter_off=True)
    out = (0,) + surface(12, 6, 16, 32)

    def call(outs=(), ids=(0, 2), surfaces=None, settings=None):
        return mg.step_surfaces(list(ids), surfaces or [small, big], settings or [off, off], list(outs))
    with pytest.raises(api.BsxError, match="2 ids for 1 surfaces and 2 settings"):
        call(surfaces=[small])
    with pytest.raises(api.BsxError, match=r"surfaces\[1\] must be a pair \(y, uv\)"):
        call(surfaces=[small, big[0]])
    with pytest.raises(api.BsxFrameFormatError, match=r"surfaces\[1\] is 16 x 8, stream 2 captures 32 x 16"):
        call(surfaces=[small, small])
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: the pitch of y, 8, is below out_w = 16"):
        call(surfaces=[(torch.as_strided(u8(256), (8, 16), (8, 1)), small[1]), big])
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: the pitch of uv, 18, is not a multiple of 4"):
        call(surfaces=[(small[0], u8(4, 18)[:, :16]), big])
    with pytest.raises(api.BsxError, match=r"surfaces\[1\]: uv must be \[8, 32\] for a y of \[16, 32\] \(it is \[16, 32\]\)"):
        call(surfaces=[small, (big[0], u8(16, 32))])
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: y has an inner stride of 2"):
        call(surfaces=[(u8(8, 32)[:, ::2], small[1]), big])
    base = u8(8 * 16 + 8)
    o = (-base.data_ptr()) % 4 + 2
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: y at 0x[0-9a-f]+ is not 4-byte aligned"):
        call(surfaces=[(torch.as_strided(base, (8, 16), (16, 1), o), small[1]), big])
    t = u8(8, 16)
    host.append(t)
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: y must be on cuda:0 \(it is on cpu\)"):
        call(surfaces=[(t, small[1]), big])
    with pytest.raises(api.BsxError, match=r"settings\[1\] is not a StreamSetting"):
        call(settings=[off, None])
    with pytest.raises(api.BsxError, match=r"settings\[0\]: bgblur is not taken by step_surfaces"):
        call(settings=[S(bgblur=5), off])
    with pytest.raises(api.BsxError, match=r"settings\[1\]: yuyv_in is not taken by step_surfaces"):
        call(settings=[off, S(filter_off=True, yuyv_in=True)])
    with pytest.raises(api.BsxError, match=r"settings\[1\]: bg is required"):
        call(settings=[off, S()])
    with pytest.raises(api.BsxError, match=r"settings\[1\].bg must be a contiguous cuda:0 uint8 tensor \[16,32,3\]"):
        call(settings=[off, S(bg=u8(8, 16, 3))])
    # the records: the messages of step_vcam_geoms_outs_nv12
    with pytest.raises(api.BsxError, match=r"outs\[0\] must be a triple"):
        call([out[:2]])
    with pytest.raises(api.BsxError, match=r"outs\[1\]: item 2 is not an index into the call's 2 positions"):
        call([out, (2,) + out[1:]])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: NV12 needs an even width and height \(y is 13 x 6\)"):
        call([(0,) + surface(13, 6, 16, 16)])
    with pytest.raises(api.BsxError, match=r"outs\[4\]: record 5 of position 1"):
        call([(1,) + surface(12, 6) for _ in range(5)])
    # nv12_to_bgr
    with pytest.raises(api.BsxFrameFormatError, match=r"y must be a non-empty uint8 tensor"):
        mg.nv12_to_bgr(u8(8, 16).float(), small[1])
    with pytest.raises(api.BsxFrameFormatError, match=r"y has 2 dimensions and uv 3"):
        mg.nv12_to_bgr(small[0], small[1][None])
    with pytest.raises(api.BsxFrameFormatError, match=r"y holds 3 images and uv 2"):
        mg.nv12_to_bgr(surface(16, 8, n=3)[0], surface(16, 8, n=2)[1])
    with pytest.raises(api.BsxFrameFormatError, match=r"the views are 16 x 8, not w = 16, h = 10"):
        mg.nv12_to_bgr(small[0], small[1], 16, 10)
    with pytest.raises(api.BsxError, match=r"nv12_to_bgr: NV12 needs an even width and height \(y is 15 x 8\)"):
        mg.nv12_to_bgr(u8(8, 16)[:, :15], u8(4, 16)[:, :15])
    with pytest.raises(api.BsxError, match=r"nv12_to_bgr: the pitch of uv, 18, is not a multiple of 4"):
        mg.nv12_to_bgr(small[0], u8(4, 18)[:, :16])
    y3, uv3 = surface(16, 8, 32, 16, n=3)
    with pytest.raises(api.BsxFrameFormatError, match=r"image i's planes must lie at i \* h \* pitch_y"):
        mg.nv12_to_bgr(y3[::2], uv3[::2])
    t = u8(4, 16)
    host.append(t)
    with pytest.raises(api.BsxError, match=r"nv12_to_bgr: uv must be on cuda:0"):
        mg.nv12_to_bgr(small[0], t)


# ---- 3. the item checks, stand-alone under the host sanitizers --------------------------------------------------------------------------------------------------
MAIN = r"""
// reads cases from stdin, one per line: "k ..." — k = 0: "i W H d_y d_uv pitch_y pitch_uv d_bg flags" -> vcam_surface_item; k = 1: "i id g W H mode roi_w roi_h" ->
// vcam_surface_class.  Prints "1" or "0 <text>" per case.
#include <cstdio>
#include "vcam_surface_plan.hpp"
int main() {
  int k;
  while (scanf("%d", &k) == 1) {
    bsx::SurfaceRefusal r;
    bool ok;
    if (k == 0) {
      int i, W, H;
      unsigned long long y, uv, bg;
      bsx_surface_item* it = new bsx_surface_item{};                 // exactly one item on the heap: a read past it is the sanitizer's to report
      if (scanf("%d %d %d %llu %llu %d %d %llu %u", &i, &W, &H, &y, &uv, &it->pitch_y, &it->pitch_uv, &bg, &it->setting.flags) != 9) return 2;
      it->d_y = reinterpret_cast<const uint8_t*>((uintptr_t)y);
      it->d_uv = reinterpret_cast<const uint8_t*>((uintptr_t)uv);
      it->setting.d_bg = reinterpret_cast<const uint8_t*>((uintptr_t)bg);
      ok = bsx::vcam_surface_item(*it, i, W, H, &r);
      delete it;
    } else {
      int i, id, g, W, H, mode, rw, rh;
      if (scanf("%d %d %d %d %d %d %d %d", &i, &id, &g, &W, &H, &mode, &rw, &rh) != 8) return 2;
      ok = bsx::vcam_surface_class(i, id, g, W, H, mode, rw, rh, &r);
    }
    if (ok) printf("1\n"); else printf("0 %s\n", r.text);
  }
  printf("%zu %zu\n", bsx::vcam_nv12_extent(768, 480, 640), bsx::vcam_nv12_extent(640, 240, 640));
  return 0;
}
"""
Y, UV, BG = 9 << 24, 10 << 24, 11 << 24
ITEM_CASES = [                    # (i, W, H, d_y, d_uv, pitch_y, pitch_uv, d_bg, flags) -> None (accepted) or the text
    ((0, 640, 480, Y, UV, 640, 640, BG, 0), None),                                   # pitch == W
    ((1, 640, 480, Y, UV, 768, 704, BG, 2 | 4), None),                               # pitch > W, the two different
    ((2, 1920, 1080, Y, UV, 2048, 1920, 0, 32), None),                               # filter off: no background is read
    ((3, 640, 480, Y, UV, 640, 640, BG + 2, 32 | 2), None),                          # ... nor is its alignment looked at
    ((4, 6, 4, Y, UV, 8, 8, BG, 0), None),
    ((5, 640, 480, Y, UV, 640, 640, BG, 0x700), "items[5]: setting flags 0x700 asks for a background blur, which the multi-geometry step does not take"),
    ((6, 640, 480, Y, UV, 640, 640, BG, 0x42), "items[6]: setting flags 0x42 has the yuyv-in bit: every frame of this call is an NV12 surface"),
    ((7, 640, 480, Y, UV, 640, 640, BG, 0x3), "items[7]: setting flags 0x3 has bits outside flip / filter-off"),
    ((8, 640, 480, Y, UV, 640, 640, BG, 0x10000), "items[8]: setting flags 0x10000 has bits outside flip / filter-off"),
    ((9, 640, 480, 0, UV, 640, 640, BG, 0), "items[9]: d_y is NULL"),
    ((10, 640, 480, 4098, UV, 640, 640, BG, 0), "items[10]: d_y 0x1002 is not 4-byte aligned"),
    ((11, 640, 480, Y, 0, 640, 640, BG, 0), "items[11]: d_uv is NULL"),
    ((12, 640, 480, Y, 4097, 640, 640, BG, 0), "items[12]: d_uv 0x1001 is not 4-byte aligned"),
    ((13, 640, 480, Y, UV, 636, 640, BG, 0), "items[13]: pitch_y = 636 is below the width 640 of its class"),
    ((14, 640, 480, Y, UV, 642, 640, BG, 0), "items[14]: pitch_y = 642 is not a multiple of 4"),
    ((15, 640, 480, Y, UV, 640, 0, BG, 0), "items[15]: pitch_uv = 0 is below the width 640 of its class"),
    ((16, 640, 480, Y, UV, 640, -704, BG, 0), "items[16]: pitch_uv = -704 is below the width 640 of its class"),
    ((17, 640, 480, Y, UV, 640, 646, BG, 0), "items[17]: pitch_uv = 646 is not a multiple of 4"),
    ((18, 640, 480, Y, UV, 1 << 23, 640, BG, 0), "items[18]: pitch_y = 8388608, pitch_uv = 640 at 480 rows: a plane of 2 GiB or more"),
    ((19, 640, 480, Y, UV, 640, 640, 0, 4), "items[19]: setting.d_bg is NULL"),
    ((20, 640, 480, Y, UV, 640, 640, BG + 3, 0), "items[20]: setting.d_bg 0xb000003 is not 4-byte aligned"),
]
CLASS_CASES = [                   # (i, id, g, W, H, mode, roi_w, roi_h)
    ((0, 3, 1, 1280, 720, 0, 1200, 720), None),
    ((1, 0, 0, 1920, 1080, 0, 1801, 1080), None),                                   # an odd ROI is no obstacle
    ((2, 5, 2, 4, 2, 0, 4, 2), None),
    ((3, 1, 0, 160, 96, 1, 160, 96), "items[3]: stream 1 is of class 0 (160 x 96), which has no fused NV12 prep: its down-scale table is a copy (capture ROI 160 x 96 = "
     "model ROI); convert such surfaces with bsx_nv12_to_bgr"),
    ((4, 1, 2, 320, 192, 2, 320, 192), "items[4]: stream 1 is of class 2 (320 x 192), which has no fused NV12 prep: its down-scale table is the 2x2 area mean (capture "
     "ROI 320 x 192 = twice the model ROI); convert such surfaces with bsx_nv12_to_bgr"),
    ((5, 7, 3, 641, 480, 0, 640, 480), "items[5]: stream 7 is of class 3 (641 x 480), which has no fused NV12 prep: NV12 needs an even width and height; convert such surfaces with bsx_nv12_to_bgr"),
    ((6, 7, 3, 640, 481, 0, 640, 480), "items[6]: stream 7 is of class 3 (640 x 481), which has no fused NV12 prep: NV12 needs an even width and height; convert such surfaces with bsx_nv12_to_bgr"),
    ((7, 0, 0, 2, 2, 0, 2, 2), "items[7]: stream 0 is of class 0 (2 x 2), which has no fused NV12 prep: the width 2 is below 4; convert such surfaces with bsx_nv12_to_bgr"),
]


def test_the_item_checks_stand_alone_under_the_host_sanitizers(tmp_path):
    src, exe = tmp_path / "main.cpp", str(tmp_path / "items")
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-o", exe, str(src)])
    cases = [(0, c, want) for c, want in ITEM_CASES] + [(1, c, want) for c, want in CLASS_CASES]
    text = "\n".join("%d %s" % (k, " ".join(str(v) for v in c)) for k, c, _w in cases) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "the program failed (a sanitizer report?):\n" + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert len(lines) == len(cases) + 2, r.stdout[-500:]
    for (k, c, want), got in zip(cases, lines):
        assert got == ("1" if want is None else "0 " + want), (k, c, got)
        assert "BSX_" not in got
    assert [int(v) for v in lines[-2].split()] == [768 * 479 + 640, 640 * 239 + 640]      # what an input plane is judged on


# ---- 4. the host code against the HIP interposer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from backscrub_amd import build
    build.build()
    src = os.path.join(STUB_DIR, "hip_stub.cpp")
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", STUB, src])
    log = str(tmp_path_factory.mktemp("surfaces") / "hip.log")
    env = dict(os.environ, LD_PRELOAD=STUB, BSX_STUB_LOG=log, BSX_STUB_NDEV="2")
    r = subprocess.run([sys.executable, os.path.join(STUB_DIR, "drive_surfaces.py"), model_path("lite"), "1"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "error" not in d, d
    lines = [l.split() for l in open(log).read().splitlines() if l.strip()]
    return d, lines


def _span(d, lines, key):
    a, b = d["calls"][key]["log"]
    return lines[a:b]


def _apis(d, lines, key):
    return [l[1] for l in _span(d, lines, key) if l[0] == "affine"]


def _kernels(d, lines, key):
    """(kernel name, grid x) of every launch of the call, in order"""
    return [(l[3], int(l[4][2:].split(",")[0])) for l in _span(d, lines, key) if l[0] == "affine" and l[1] in ("hipLaunchKernel", "hipModuleLaunchKernel")]


def _tiles(roi):
    return ((roi[2] + 127) // 128) * ((roi[3] + 31) // 32)


def _out_tiles(w, h):
    return ((w + 63) // 64) * ((h + 31) // 32)


OK_CALLS = ["surf_1", "surf_3", "surf_3_again", "tight", "bg_null_filter_off", "in_extent_touch", "good_after"] + ["ring_%d" % i for i in range(6)]
BACK_END = ("prep_", "tile_class", "mask_geoms_k", "mask_tile", "vg_outs", "outside_roi")
RECORDS = len(IDS) * _out_tiles(*LAYERS[0]) + _out_tiles(*LAYERS[1])


def test_a_call_runs_on_the_contexts_device_with_one_copy_per_ring_and_never_synchronises(run):
    d, lines = run
    for key in OK_CALLS + ["masks_only"]:
        c = d["calls"][key]
        assert c["rc"] == 0, (key, c)
        assert c["caller_device"] == 0, "%s: the caller's device was not restored" % key
        affine = [l for l in _span(d, lines, key) if l[0] == "affine"]
        assert affine and not [l for l in affine if int(l[2]) != 1], key
        assert not [l for l in _span(d, lines, key) if l[0] == "MISMATCH"], key
        apis = [l[1] for l in affine]
        # ids; descriptors with the surface records behind them; groups, output descriptors and plane records (none with m == 0)
        assert apis.count("hipMemcpyAsync") == (2 if key == "masks_only" else 3), (key, apis)
        assert "hipEventRecord" in apis
        assert "hipStreamSynchronize" not in apis and "hipDeviceSynchronize" not in apis and "hipEventSynchronize" not in apis, "%s synchronised the host" % key
    for key in ["surf_3_again", "good_after"] + ["ring_%d" % i for i in range(6)]:
        apis = _apis(d, lines, key)
        assert "hipHostMalloc" not in apis and "hipMalloc" not in apis and "hipMemcpy" not in apis, key
    assert "hipEventQuery" in [a for k in ("ring_%d" % i for i in range(6)) for a in _apis(d, lines, k)]
    assert d["pipelined"] == [0, 0]
    allocs = sum(1 for l in lines if l[0] == "affine" and l[1] == "hipMalloc")
    frees = sum(1 for l in lines if l[0] == "affine" and l[1] == "hipFree")
    assert allocs == frees, (allocs, frees)


def test_the_launch_list_of_a_call_and_of_the_older_entry_points(run):
    d, lines = run
    traces = {k: _kernels(d, lines, k) for k in ("surf_1", "surf_3", "surf_3_again", "tight", "masks_only", "nv12_3", "geoms_3")}

    def names(t):
        return [re.sub(r"\d+", "#", n) for n, _ in t]

    def network(t):
        return [x for x in t if not any(s in x[0] for s in BACK_END)]
    assert names(traces["surf_1"]) == names(traces["surf_3"]) == names(traces["surf_3_again"]) == names(traces["tight"])
    for key, classes in (("surf_1", "c1"), ("surf_3", "c3"), ("tight", "c3")):
        t = traces[key]
        order = [x[0] for x in t]
        one = {k: [x for x in t if k in x[0]] for k in ("prep_geoms_nv12_k", "tile_class_geoms_k", "mask_geoms_k", "vg_outs_nv12in_k")}
        for k, hit in one.items():
            assert len(hit) == 1, (key, k, order)
        # one prep launch, the network, tile classes, masks, one resize pass — and nothing else that reads a frame
        assert [n for n in order if any(s in n for s in BACK_END)] == [one[k][0][0] for k in ("prep_geoms_nv12_k", "tile_class_geoms_k", "mask_geoms_k", "vg_outs_nv12in_k")]
        assert order[0] == one["prep_geoms_nv12_k"][0][0] and order[-3:] == [one[k][0][0] for k in ("tile_class_geoms_k", "mask_geoms_k", "vg_outs_nv12in_k")]
        assert len(t) - 4 >= 5, "no network between prep and the back end: %s" % order
        assert not [n for n in order if any(e in n for e in ("nv12_to_bgr", "yuyv", "resize_bgr", "blend_k", "flip_bgr"))], order
        info = d["infos"][classes]
        of = [[q for q in info if q["first_stream"] <= s < q["first_stream"] + q["n_streams"]][0] for s in IDS]
        assert one["prep_geoms_nv12_k"][0][1] == len(IDS) * 5 * 3        # segm_lite's 160 x 96 canvas: 5 x 3 tiles of 32 x 32 per position
        assert one["tile_class_geoms_k"][0][1] == len(IDS)
        assert one["mask_geoms_k"][0][1] == sum(_tiles(q["roi"]) for q in of)
        assert one["vg_outs_nv12in_k"][0][1] == RECORDS
    # m == 0: the same front, masks only
    mo = [x[0] for x in traces["masks_only"]]
    assert [re.sub(r"\d+", "#", n) for n in mo] == names(traces["surf_3"])[:-1] and not [n for n in mo if "vg_outs" in n]
    # the two older entry points on the same context trace what they traced: their own prep and back end, the same network
    t = traces["nv12_3"]
    assert len([x for x in t if any(s in x[0] for s in BACK_END)]) == 4
    assert [k for k in ("prep_geoms_kI", "tile_class_geoms_k", "mask_geoms_kI", "vg_outs_nv12_kI") for x in t if k in x[0]] == \
        ["prep_geoms_kI", "tile_class_geoms_k", "mask_geoms_kI", "vg_outs_nv12_kI"]
    assert [x[1] for x in t if "vg_outs_nv12_kI" in x[0]] == [RECORDS] and [x[1] for x in t if "prep_geoms_kI" in x[0]] == [len(IDS) * 15]
    assert _apis(d, lines, "nv12_3").count("hipMemcpyAsync") == 3
    g = traces["geoms_3"]
    assert [k for x in g for k in ("prep_geoms_kI", "tile_class_geoms_k", "mask_tile_geoms_k") if k in x[0]] == ["prep_geoms_kI", "tile_class_geoms_k", "mask_tile_geoms_k"]
    assert not [x[0] for x in g if "nv12" in x[0] or "vg_" in x[0]]
    assert _apis(d, lines, "geoms_3").count("hipMemcpyAsync") == 2
    assert network(traces["surf_3"]) == network(t) == network(g) and network(traces["surf_1"]) == network(traces["surf_3"])
    # the stand-alone conversion: one launch, words or bytes
    assert d["calls"]["conv"]["rc"] == 0 and d["calls"]["conv_tail"]["rc"] == 0
    assert [(re.sub(r".*nv12_to_bgr_kILb(\d).*", r"\1", n), g_) for n, g_ in _kernels(d, lines, "conv")] == [("1", (160 * 240 + 255) // 256)]
    assert [(re.sub(r".*nv12_to_bgr_kILb(\d).*", r"\1", n), g_) for n, g_ in _kernels(d, lines, "conv_tail")] == [("0", 1)]


@pytest.mark.parametrize("key,words", [
    ("dup", ["ids[2] = 0", "repeats ids[0]"]),
    ("items_null", ["items is NULL"]),
    ("flags", ["flags 0x1", "takes no flags"]),
    ("setting_blur", ["items[2]", "flags 0x700", "background blur"]),
    ("setting_yuyv_in", ["items[3]", "flags 0x42", "yuyv-in"]),
    ("setting_bit0", ["items[3]", "flags 0x3", "outside flip / filter-off"]),
    ("y_null", ["items[1]", "d_y is NULL"]),
    ("y_unaligned", ["items[1]", "d_y", "not 4-byte aligned"]),
    ("uv_null", ["items[4]", "d_uv is NULL"]),
    ("uv_unaligned", ["items[4]", "d_uv", "not 4-byte aligned"]),
    ("pitch_y_low", ["items[0]", "pitch_y = 636", "below the width 640"]),
    ("pitch_y_mod", ["items[0]", "pitch_y = 642", "multiple of 4"]),
    ("pitch_uv_low", ["items[3]", "pitch_uv = 0", "below the width 640"]),
    ("pitch_uv_mod", ["items[3]", "pitch_uv = 1286", "multiple of 4"]),
    ("bg_null", ["items[5]", "d_bg is NULL"]),
    ("bg_unaligned", ["items[5]", "d_bg", "not 4-byte aligned"]),
    ("out_y_is_in_y", ["outs[2]", "d_y", "overlaps d_y of items[2]"]),
    ("out_uv_in_uv", ["outs[1]", "d_uv", "overlaps d_uv of items[0]"]),
    ("out_y_in_bg", ["outs[3]", "d_y", "overlaps setting.d_bg of items[1]"]),
    ("out_y_in_out_uv", ["d_y", "overlaps d_uv of outs["]),
    ("in_extent_overlap", ["outs[0]", "d_y", "overlaps d_y of items[1]"]),
    ("out_record", ["outs[6]", "pitch_uv = 158", "below out_w = 160"]),
    ("pending", ["pipelined composite is pending"]),
    ("class_off_route", ["items[0]", "stream 1", "642 x 480", "off the fused tile route"]),
    ("onmask", ["onmask"]),
    ("class_area", ["items[0]", "stream 1", "320 x 192", "no fused NV12 prep", "2x2 area mean", "bsx_nv12_to_bgr"]),
])
def test_refusals_name_the_position_and_value_and_enqueue_nothing(run, key, words):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL, (key, c)
    for w in words:
        assert w in c["error"], (key, w, c["error"])
    assert "bsx_step_batch_surfaces" in c["error"]
    assert not [l for l in _span(d, lines, key) if l[0] == "affine"], "%s made HIP calls" % key


def test_an_empty_batch_is_a_no_op(run):
    d, lines = run
    assert d["calls"]["empty"]["rc"] == 0
    assert not [l for l in _span(d, lines, "empty") if l[0] == "affine"]


# ---- 5. kernel resources ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_and_no_more_lds():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(CSRC, "kernels_img.hip"), "vg_outs|prep_geoms|nv12_to_bgr"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    row = re.compile(r"^(\S+)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)")
    rows = {m.group(1): dict(vgpr=int(m.group(2)), lds=int(m.group(4)), scratch=int(m.group(5))) for m in map(row.match, r.stdout.splitlines()) if m}

    def some(needle, count):
        hit = [v for k, v in rows.items() if needle in k]
        assert len(hit) == count, (needle, sorted(rows))
        return hit
    vg_limit = some("vg_outs_nv12_fmt_kI", 1)[0]["lds"]
    prep_limit = min(a["lds"] for a in some("prep_geoms_fmt_kI", 3))
    for new, count, limit in (("vg_outs_nv12in_kI", 1, vg_limit), ("prep_geoms_nv12_kI", 3, prep_limit), ("nv12_to_bgr_kI", 2, 0)):
        for a in some(new, count):
            print(new, a, "lds limit", limit)
            assert a["scratch"] == 0, "%s spills %d bytes" % (new, a["scratch"])
            assert a["lds"] <= limit, (new, a, limit)
