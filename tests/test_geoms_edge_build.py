"""bsx_new_geoms_ex / BSX_GEOMS_EDGE_ROI without a GPU: header, export map, library and binding agree on the new symbol; MaskGen.with_geometries(edge_roi=...)
validates its arguments before the library is reached; the creation-time refusals (they come before any device work) name the class and the value; and the three
kernels of the edge launcher keep to their bounds (tools/kernel_regs.sh, read as tests/test_geoms_host.py reads it): no scratch, LDS not above mask_tile_k's."""
import fnmatch
import os
import re

import pytest

from conftest import model_path
from test_geoms_host import _survey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")


def test_header_map_library_and_binding_agree_on_bsx_new_geoms_ex():
    import ctypes
    from backscrub_amd import api, build
    sym = "bsx_new_geoms_ex"
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    m = re.search(r"^BSX_API bsx_ctx\* %s\(([^;]*)\);" % sym, hdr, re.M)
    assert m, "include/bsx.h does not declare %s" % sym
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 11 and params[5] == "unsigned flags"
    assert re.search(r"^#define BSX_GEOMS_EDGE_ROI 1u$", hdr, re.M) and api.BSX_GEOMS_EDGE_ROI == 1
    entry = [s for s in api.SYMBOLS if s[0] == sym]
    assert len(entry) == 1 and entry[0][1] is ctypes.c_void_p and len(entry[0][2]) == 11 and entry[0][2][5] is ctypes.c_uint
    plain = [s for s in api.SYMBOLS if s[0] == "bsx_new_geoms"][0]
    assert entry[0][2][:5] == plain[2][:5] and entry[0][2][6:] == plain[2][5:]          # bsx_new_geoms's arguments with the flags word behind `device`
    exported = re.findall(r"global:\s*([^;]+);", open(os.path.join(CSRC, "libbsx.map")).read())
    assert any(fnmatch.fnmatch(sym, pat.strip()) for pats in exported for pat in pats.split()), "libbsx.map does not export %s" % sym
    for lib in (build.LIB, build.LIB_DBG):
        assert hasattr(ctypes.CDLL(lib), sym), (lib, sym)


def test_with_geometries_validates_edge_roi_before_reaching_c(monkeypatch):
    from backscrub_amd import api

    def no_c():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(api, "lib", no_c)
    with pytest.raises(api.BsxError, match="edge_roi must be True or False"):
        api.MaskGen.with_geometries("m.tflite", [(640, 480, 1)], edge_roi=1)
    with pytest.raises(api.BsxError, match="edge_roi must be True or False"):
        api.MaskGen.with_geometries("m.tflite", [(640, 480, 1)], edge_roi="yes")
    with pytest.raises(api.BsxError, match=r"geometries\[1\]: width 642 is not a multiple of 4"):
        api.MaskGen.with_geometries("m.tflite", [(640, 480, 1), (642, 480, 1)], edge_roi=True)
    with pytest.raises(api.BsxError, match="geometries must be"):
        api.MaskGen.with_geometries("m.tflite", [(640, 480)], edge_roi=True)
    with pytest.raises(AssertionError, match="the library was reached"):              # valid arguments go on to the library, with or without the flag
        api.MaskGen.with_geometries("m.tflite", [(640, 480, 1), (1920, 1080, 1)], edge_roi=True)
    with pytest.raises(AssertionError, match="the library was reached"):
        api.MaskGen.with_geometries("m.tflite", [(640, 480, 1), (642, 480, 1)])


def _new_ex(geoms, flags):
    """bsx_new_geoms_ex straight through the binding's table: (handle, message)"""
    from backscrub_amd import api
    L = api.lib()
    arr = (api._Geometry * len(geoms))(*[api._Geometry(*g) for g in geoms])
    quiet = api.DEBUG_FN(lambda _ctx, _msg: None)
    h = L.bsx_new_geoms_ex(os.fsencode(model_path("lite")), 2, arr, len(geoms), 0, flags, quiet, api.STAGE_FN(), api.STAGE_FN(), api.STAGE_FN(), None)
    return h, (L.bsx_last_error(None) or b"").decode()


@pytest.mark.parametrize("geoms,flags,words", [
    ([(640, 480, 1), (642, 480, 1)], 1, ["bsx_new_geoms_ex", "geoms[1]", "642 x 480", "width 642"]),
    ([(642, 480, 2)], 1, ["geoms[0]", "642 x 480", "width 642"]),                                          # one class: the rule holds from n_geoms = 1 up
    ([(640, 480, 1), (80, 48, 1)], 1, ["geoms[1]", "80 x 48", "off the fused tile route", "tiled linear"]),
    ([(640, 480, 1)], 4, ["flags 0x4", "unknown bit 0x4"]),
    ([(640, 480, 1)], 7, ["flags 0x7", "unknown bit 0x2"]),
    ([(640, 480, 1), (1920, 1080, 1)], 0, ["bsx_new_geoms:", "geoms[1]", "1920 x 1080", "roi.w 1799", "fused tile route"]),      # flags == 0 IS bsx_new_geoms
    ([(640, 480, 1), (640, 480, 1)], 1, ["bsx_new_geoms_ex:", "repeats the size of geoms[0]"]),
])
def test_creation_refusals_return_null_and_name_the_value(geoms, flags, words):
    h, text = _new_ex(geoms, flags)
    assert not h
    for w in words:
        assert w in text, (w, text)


def test_resources_of_the_edge_kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    rows = _survey()

    def pick(needle):
        hit = {k: v for k, v in rows.items() if needle in k}
        assert hit, needle
        return hit
    new = {}
    for needle in ("tile_class_geoms_edge_k", "mask_tile_geoms_edge_k", "outside_roi_geoms_edge_k"):
        new.update(pick(needle))
    assert len(new) == 3
    for name, r in new.items():
        assert r["scratch"] == 0, "%s spills %d bytes" % (name, r["scratch"])
    tile_lds = max(r["lds"] for r in pick("mask_tile_kI").values())
    for name, r in pick("mask_tile_geoms_edge_k").items():
        assert r["lds"] <= tile_lds, "%s: %d B of LDS, mask_tile_k has %d" % (name, r["lds"], tile_lds)
    cls_lds = max(r["lds"] for r in pick("tile_class_geoms_k").values())
    for name, r in pick("tile_class_geoms_edge_k").items():
        assert r["lds"] <= cls_lds, "%s: %d B of LDS, tile_class_geoms_k has %d" % (name, r["lds"], cls_lds)
    # the kernels the other launchers run keep their names and their number
    assert len(pick("mask_tile_geoms_k")) == 1 and len(pick("mask_tile_geoms_fmt_k")) == 1 and len(pick("tile_class_geoms_k")) == 1 and len(pick("mask_tile_kI")) == 9
