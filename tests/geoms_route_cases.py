"""The fleets of the multi-geometry audit (docs/design/02b-geometry-audit.md, "Multi-geometry steps"): plain data, shared by tests/test_geoms_route_cases.py (no
library: the classes' arithmetic and what each fleet is there for) and tests/test_gpu_geoms_routes.py (every fleet stepped on the GPU, bytes against the oracle).

bsx_step_batch_geoms / bsx_step_batch_vcam_geoms choose a body per WORKGROUP from a class record — prep_geoms_k between the table-driven and the general prep,
tile_class_geoms_k between the classifier and a zero-fill, mask_tile_geoms_k its place in a ragged grid of up to 8 classes — where the one-geometry kernels have the
launcher choose.  The fleets put the classes that take each branch into ONE context, next to ordinary camera sizes.

A class taken from the frame-geometry matrix is named by its row id and looked up in geometry_cases.ROWS, so the row's purpose and observed route travel with it;
the other classes are the camera sizes the existing geoms tests step.  Every class states the rectangles capture_rois gives it (written here, restated in float32
by the CPU test, compared with the library's and the oracle's on the GPU): roi, in_roi, the table mode of the down-scale (0 linear, 2 the exact 2x2 area mean) and
its 128 x 32 mask tiles (ntx, nty).
"""
import geometry_cases as gc

MODEL_INPUT = {"lite": (160, 96), "full": (256, 144), "mlkit": (256, 256)}      # (inW, inH) of the three models the fleets use
TILE_W, TILE_H = 128, 32                                                       # mask_tile_geoms_k's tile
CLS_MAX_TX = 16                                                                # kClsMaxTx: more tile columns than this and tile_class_geoms_k zero-fills


def K(W, H, n, roi, in_roi, down, tiles, row=None):
    return dict(size=(W, H), n=n, roi=roi, in_roi=in_roi, down=down, tiles=tiles, row=row)


def _whole(W, H):
    return (0, 0, W, H)


FLEETS = {
    # 8 classes (kMaxGeoms); general prep; both rows at the LDS fit boundary; portrait; pillarboxed frames (roi.x = 40, 20) beside whole-frame ones
    "lite8": dict(model="lite", classes=[
        K(320, 192, 2, _whole(320, 192), (0, 0, 160, 96), 2, (3, 6), row="lite-320x192"),
        K(132, 100, 2, _whole(132, 100), (16, 0, 126, 96), 0, (2, 4), row="lite-132x100"),
        K(108, 88, 2, _whole(108, 88), (21, 0, 117, 96), 0, (1, 3), row="lite-108x88"),
        K(360, 640, 2, _whole(360, 640), (53, 0, 54, 96), 0, (3, 20), row="lite-360x640"),
        K(640, 480, 2, _whole(640, 480), (16, 0, 128, 96), 0, (5, 15)),
        K(1280, 720, 2, (40, 0, 1200, 720), (0, 0, 160, 96), 0, (10, 23)),
        K(640, 360, 2, (20, 0, 600, 360), (0, 0, 160, 96), 0, (5, 12)),
        K(800, 600, 2, _whole(800, 600), (16, 0, 128, 96), 0, (7, 19)),
    ]),
    # general prep; a 5-tile portrait class beside classes of 576 / 592 / 629 tiles; ntx = 16 in range, ntx = 16 with a partial last tile row and ntx = 17 (out of
    # the classifier's range: the zero-fill) in one launch
    "full6": dict(model="full", classes=[
        K(512, 288, 2, _whole(512, 288), (0, 0, 256, 144), 2, (4, 9), row="full-512x288"),
        K(96, 160, 2, _whole(96, 160), (84, 0, 86, 144), 0, (1, 5), row="full-96x160"),
        K(2048, 1152, 2, _whole(2048, 1152), (0, 0, 256, 144), 0, (16, 36), row="full-2048x1152"),
        K(2048, 1160, 2, _whole(2048, 1160), (0, 0, 254, 144), 0, (16, 37), row="full-2048x1160"),
        K(2056, 1160, 2, _whole(2056, 1160), (0, 0, 255, 144), 0, (17, 37), row="full-2056x1160"),
        K(640, 480, 2, _whole(640, 480), (32, 0, 192, 144), 0, (5, 15)),
    ]),
    # general prep on a square model; two classes with strips outside the ROI (roi.x = 112, 80); the branch-B portrait
    "mlkit4": dict(model="mlkit", classes=[
        K(512, 512, 2, _whole(512, 512), (0, 0, 256, 256), 2, (4, 16), row="mlkit-512x512"),
        K(512, 288, 2, (112, 0, 288, 288), (0, 0, 256, 256), 0, (3, 9), row="mlkit-512x288"),
        K(240, 320, 2, _whole(240, 320), (32, 0, 192, 256), 0, (2, 10), row="mlkit-240x320"),
        K(640, 480, 2, (80, 0, 480, 480), (0, 0, 256, 256), 0, (4, 15)),
    ]),
    # a 3-workgroup class in front; 11 positions of a class whose rows share cache lines (8 tiles each): 8 in the one-XCD-per-frame order and 3 in the remainder
    "xcd_lite": dict(model="lite", classes=[
        K(108, 88, 1, _whole(108, 88), (21, 0, 117, 96), 0, (1, 3), row="lite-108x88"),
        K(132, 100, 11, _whole(132, 100), (16, 0, 126, 96), 0, (2, 4), row="lite-132x100"),
    ]),
    # the same with an outside-ROI launch and 27 tiles per position
    "xcd_mlkit": dict(model="mlkit", classes=[
        K(240, 320, 3, _whole(240, 320), (32, 0, 192, 256), 0, (2, 10), row="mlkit-240x320"),
        K(512, 288, 11, (112, 0, 288, 288), (0, 0, 256, 256), 0, (3, 9), row="mlkit-512x288"),
    ]),
}

STEP_FLEETS = ("lite8", "full6", "mlkit4")          # the fleets of the step schedule; the xcd_* fleets have a schedule of their own
XCD_FLEETS = ("xcd_lite", "xcd_mlkit")


def matrix_row(cls_or_id):
    """the row of the frame-geometry matrix a class names (None: an ordinary camera size)"""
    rid = cls_or_id["row"] if isinstance(cls_or_id, dict) else cls_or_id
    if rid is None:
        return None
    rows = [r for r in gc.ROWS if gc.row_id(r) == rid]
    assert len(rows) == 1, "%s names %d rows of the geometry matrix" % (rid, len(rows))
    return rows[0]


def geoms(name):
    """the fleet as MaskGen.with_geometries takes it"""
    return [c["size"] + (c["n"],) for c in FLEETS[name]["classes"]]


def first_streams(name):
    out, s = [], 0
    for c in FLEETS[name]["classes"]:
        out.append(s)
        s += c["n"]
    return out


def shares_lines(c):
    """mask_tile_grid's rule for the one-XCD-per-frame order: the ROI's rows do not start on a 128-byte line"""
    return ((c["roi"][0] * 3) & 127) != 0 or ((c["size"][0] * 3) & 127) != 0


def yuyv_in_admitted(c):
    """prep_yuyv_fusable: a linear down-scale, whole macropixels (even W and roi.x), an 8-byte window inside the row"""
    return c["down"] == 0 and c["size"][0] % 2 == 0 and c["roi"][0] % 2 == 0 and (c["size"][0] - c["roi"][0]) * 2 >= 8
