"""bsx_new_geoms_ex(BSX_GEOMS_EDGE_ROI) on the GPU: classes whose ROI is off the 4-pixel grid in the multi-geometry steps.  Per stream, composite, persistent mask and
temporal state (`ofinal`) are byte-identical to bsx_step_batch_streams of that one stream in a one-geometry context of its size — the route that takes any geometry
and is oracle-checked — called with the stream's background, stride 0 and the stream's flips OR'd with the batch's yuyv / no-mask flags.  A filter-off stream's
composite is its frame, then bsx_flip_bgr, then bsx_bgr_to_yuyv; a YUYV item equals the same call after bsx_yuyv_to_bgr.  Byte equality everywhere; the oracle
test asserts IoU 1.0 and a composite difference of 0.

Every d_out lies between two 64-byte bands of a sentinel that must survive every call, and after every call the persistent mask outside the ROI is 255.  Every
fleet first asserts, from bsx_get_geom_info, the ROIs its cases were chosen for, so no case can silently run on the word route."""
import numpy as np
import pytest

from conftest import model_path
from test_gpu_geoms import CYCLE, _frame, _image, bs          # noqa: F401 (bs: the library fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (capture size, ROI): what each class covers is in the comment; s = roi.x & 3
LITE = [((640, 480), [0, 0, 640, 480]),       # word route
        ((640, 360), [20, 0, 600, 360]),      # word route, strips outside the ROI
        ((512, 288), [16, 0, 479, 288]),      # ragged right edge only
        ((480, 270), [15, 0, 449, 270]),      # s = 3, aligned right edge, odd column
        ((320, 180), [10, 0, 300, 180]),      # both edges ragged, even column: YUYV items allowed
        ((264, 154), [3, 0, 256, 154]),       # s = 3 adds a third tile column; partial last tile row
        ((200, 112), [6, 0, 186, 112])]       # s = 2, right edge aligned
MLKIT = [((640, 480), [80, 0, 480, 480]),     # word route
         ((960, 540), [210, 0, 540, 540]),
         ((600, 338), [131, 0, 338, 338])]
FLEETS = {"lite": LITE, "mlkit": MLKIT}
BAND, SENTINEL = 64, 0xA5


def _on_grid(roi):
    return roi[0] % 4 == 0 and roi[2] % 4 == 0


def _guarded(shape):
    """a zeroed output of `shape` between two BAND-byte sentinel bands, in one allocation: (whole buffer, the output's view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[BAND:BAND + n].view(shape)
    out.zero_()
    assert out.data_ptr() % 4 == 0
    return buf, out


def _bands_intact(buf):
    return bool((buf[:BAND] == SENTINEL).all()) and bool((buf[-BAND:] == SENTINEL).all())


def _check_rois(mg, cases):
    for g, (size, roi) in zip(mg.geometries(), cases):
        assert (g["width"], g["height"]) == size
        assert g["roi"] == roi, "%s: ROI %s, the test was written for %s" % (size, g["roi"], roi)


_EDGE, _YUYV = {}, {}


def _edge_frame(W, H, roi, s, t):
    """the scene of tests/test_gpu_geoms.py rolled so that its centre — the person — lies ON a bound of the ROI: the left bound for an even stream, the right one
    for an odd stream.  The soft part of the mask then crosses the 4-pixel groups that straddle the bound (with the person in the middle those see uniform tiles
    only).  Computed once, never written."""
    key = (W, H, s, t)
    if key not in _EDGE:
        bound = roi[0] if s % 2 == 0 else roi[0] + roi[2]
        _EDGE[key] = torch.roll(_frame(W, H, s, t), bound - W // 2, dims=1).contiguous()
    return _EDGE[key]


def _yuyv_frame(mg, W, H, roi, s, t):
    """the frame as a camera delivers it, Y0 U Y1 V: the project's packer writes Y0 V Y1 U, so bytes 1 and 3 of every macropixel change places"""
    key = (W, H, s, t)
    if key not in _YUYV:
        packed = mg.bgr_to_yuyv(_edge_frame(W, H, roi, s, t)[None])[0]
        _YUYV[key] = packed.view(H, W // 2, 4)[:, :, [0, 3, 2, 1]].contiguous().view(H, W, 2)
    return _YUYV[key]


class EdgeFleet:
    """one edge context of all the classes of `cases` (2 streams each) and one one-geometry twin per class"""

    def __init__(self, bs, key, cases, per_class=2):
        self.bs, self.key, self.path, self.cases = bs, key, model_path(key), cases
        self.geoms = [(W, H, per_class) for (W, H), _roi in cases]
        self.n = per_class * len(cases)
        self.mg = bs.MaskGen.with_geometries(self.path, self.geoms, edge_roi=True)
        _check_rois(self.mg, cases)
        self.first = [g["first_stream"] for g in self.mg.geometries()]
        self.twins = [bs.MaskGen(self.path, W, H, n_streams=n) for W, H, n in self.geoms]
        for tw, (_size, roi) in zip(self.twins, cases):
            assert tw.info["roi"] == roi

    def reset(self):
        for c in [self.mg] + self.twins:
            c.reset()

    def cls(self, s):
        g = max(i for i, f in enumerate(self.first) if f <= s)
        return g, s - self.first[g]

    def streams_of(self, pred):
        """the streams of the classes whose ROI satisfies pred"""
        return [s for s in range(self.n) if pred(self.cases[self.cls(s)[0]][1])]

    def item(self, s, t, yuyv, yin):
        g, _ = self.cls(s)
        W, H, _n = self.geoms[g]
        bg, fl = CYCLE[(s + t) % len(CYCLE)]
        img = None if bg is None else _image(W, H, 100 + s if bg == "own" else 7 + g)
        roi = self.cases[g][1]
        frame = _yuyv_frame(self.mg, W, H, roi, s, t) if yin else _edge_frame(W, H, roi, s, t)
        buf, out = _guarded((H, W, 2 if yuyv else 3))
        return frame, buf, out, self.bs.StreamSetting(bg=img, yuyv_in=yin, **fl)

    def twin_composite(self, s, t, frame, sett, yuyv, no_mask, yin):
        """what the contract says stream s's composite is, from its twin (whose state advances by the same call)"""
        g, loc = self.cls(s)
        W, H, _n = self.geoms[g]
        tw = self.twins[g]
        bgr = tw.yuyv_to_bgr(frame[None]) if yin else frame[None]
        out = torch.zeros((1, H, W, 2 if yuyv else 3), dtype=torch.uint8, device="cuda")
        if sett.filter_off:
            tw.step_streams([loc], bgr, _image(W, H, 7 + g), out, yuyv=yuyv, no_mask=no_mask)      # state and mask advance; the composite is the frame's
            want = bgr
            if sett.flip_h or sett.flip_v:
                want = tw.flip_bgr(want, -1 if sett.flip_h and sett.flip_v else (1 if sett.flip_h else 0))
            return (tw.bgr_to_yuyv(want) if yuyv else want)[0]
        return tw.step_streams([loc], bgr, sett.bg, out, flip_h=sett.flip_h, flip_v=sett.flip_v, yuyv=yuyv, no_mask=no_mask)[0]

    def tick(self, t, ids, yuyv=False, no_mask=False, yin=(), tag=""):
        items = [self.item(s, t, yuyv, s in yin) for s in ids]
        self.mg.step_geoms(ids, [i[0] for i in items], [i[2] for i in items], [i[3] for i in items], yuyv=yuyv, no_mask=no_mask)
        for s, (frame, buf, out, sett) in zip(ids, items):
            size = self.cases[self.cls(s)[0]][0]
            assert _bands_intact(buf), "%st=%d stream %d %s: a guard band of d_out was written" % (tag, t, s, size)
            want = self.twin_composite(s, t, frame, sett, yuyv, no_mask, s in yin)
            bad = (out != want).any(-1)
            assert not bool(bad.any()), "%st=%d stream %d %s (%s): %d composite pixels differ, first at (y, x) = %s" % (
                tag, t, s, size, sett, int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]))
        self.compare_state(t, tag)

    def compare_state(self, t, tag=""):
        of = self.mg.ofinal()
        for s in range(self.n):
            g, loc = self.cls(s)
            size, roi = self.cases[g]
            assert torch.equal(of[s], self.twins[g].ofinal()[loc]), "%st=%d stream %d %s: temporal state differs" % (tag, t, s, size)
            m = self.mg.masks_of(s)
            assert torch.equal(m, self.twins[g].masks()[loc]), "%st=%d stream %d %s: persistent masks differ" % (tag, t, s, size)
            outside = torch.ones_like(m, dtype=torch.bool)
            outside[roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]] = False
            assert bool((m[outside] == 255).all()), "%st=%d stream %d %s: a mask byte outside the ROI is not 255" % (tag, t, s, size)

    def close(self):
        for c in [self.mg] + self.twins:
            c.close()


@pytest.fixture(scope="module")
def fleets(bs):
    made = {}

    def get(key):
        if key not in made:
            made[key] = EdgeFleet(bs, key, FLEETS[key])
        made[key].reset()
        return made[key]
    yield get
    for f in made.values():
        f.close()


def _orders(n, ticks, seed):
    rng = np.random.default_rng(seed)
    return [[int(i) for i in rng.permutation(n)] for _ in range(ticks)]


# ---- 1. byte identity (and 2., the guard bands and the mask outside the ROI, checked by every tick) -------------------------------------------------------------
@pytest.mark.parametrize("variant", ["bgr", "yuyv", "no_mask", "yuyv_items"])
@pytest.mark.parametrize("key", ["lite", "mlkit"])
def test_every_stream_equals_its_one_geometry_twin(fleets, key, variant):
    f = fleets(key)
    batch = {"yuyv": variant == "yuyv", "no_mask": variant == "no_mask"}
    yin = ()
    if variant == "yuyv_items":                       # the first stream of every class with an even ROI column brings the camera's YUYV
        yin = {s for s in f.streams_of(lambda roi: roi[0] % 2 == 0) if f.cls(s)[1] == 0}
        assert any(not _on_grid(f.cases[f.cls(s)[0]][1]) for s in yin)
    for t, ids in enumerate(_orders(f.n, 6, 11)):
        f.tick(t, ids, yin=yin, tag="%s %s " % (key, variant), **batch)
    if variant == "bgr":                              # the comparison was no formality: at both bounds of every ROI off the grid the mask is neither 0 nor 255 somewhere
        for g, (size, roi) in enumerate(f.cases):
            if not _on_grid(roi):
                m = torch.stack([f.mg.masks_of(f.first[g] + k)[:, roi[0]:roi[0] + roi[2]] for k in range(2)])
                for name, cols in (("left", m[:, :, :4]), ("right", m[:, :, -4:])):
                    assert bool(((cols > 0) & (cols < 255)).any()), "%s: no soft mask byte in the %s four columns of the ROI" % (size, name)


def test_subset_reset_and_a_call_of_word_route_classes_only(fleets):
    f = fleets("lite")
    orders = _orders(f.n, 6, 12)
    for t in range(3):
        f.tick(t, orders[t])
    f.tick(3, orders[3][:f.n // 2], tag="subset ")
    victim = f.first[3] + 1                                                 # a 480 x 270 stream
    f.mg.reset_streams([victim])
    f.twins[3].reset_streams([1])
    f.compare_state(3, "after reset_streams ")
    f.tick(4, orders[4], tag="after reset_streams ")
    word = f.streams_of(_on_grid)
    assert len(word) == 4
    f.tick(5, word[::-1], tag="word-route classes only ")
    f.tick(6, f.streams_of(lambda roi: not _on_grid(roi)), tag="edge classes only ")


def test_guard_bands_and_the_mask_outside_the_roi(fleets):
    """flips and YUYV out together on the fleet whose ROIs start far inside the frame (MLKit): EdgeFleet.tick asserts the bands and the outside bytes after every call"""
    f = fleets("mlkit")
    for t, ids in enumerate(_orders(f.n, 3, 13)):
        f.tick(t + 2, ids, yuyv=t == 1, tag="guard ")


# ---- 3. the CPU oracle ------------------------------------------------------------------------------------------------------------------------------------------
def test_an_edge_class_against_the_oracle(bs, oracle):
    """two 480 x 270 streams of a ONE-class edge context against the CPU oracle over the same frames from a reset state.  The figures are printed before they are
    asserted."""
    from backscrub_amd import synth
    W, H = 480, 270
    path = model_path("lite")
    mg = bs.MaskGen.with_geometries(path, [(W, H, 2)], edge_roi=True)
    _check_rois(mg, [((W, H), [15, 0, 449, 270])])
    ids = [1, 0]
    bgs = {s: synth.background(W, H, seed=3 + s) for s in ids}
    ocs = {s: oracle.Ctx(path, W, H) for s in ids}
    figures = []
    for t in range(4):
        host = {s: synth.frame(W, H, s, t) for s in ids}
        items = [_guarded((H, W, 3)) for _ in ids]
        mg.step_geoms(ids, [torch.from_numpy(host[s]).cuda() for s in ids], [o for _b, o in items], [bs.StreamSetting(bg=torch.from_numpy(bgs[s]).cuda()) for s in ids])
        torch.cuda.synchronize()
        for (buf, out), s in zip(items, ids):
            assert _bands_intact(buf)
            want = ocs[s].process(host[s])
            got = mg.masks_of(s).cpu().numpy()
            fa, fb = got < 128, want < 128
            union = np.logical_or(fa, fb).sum()
            iou = 1.0 if union == 0 else float(np.logical_and(fa, fb).sum()) / float(union)
            comp = oracle.alpha_blend(bgs[s], host[s], want)
            diff = int(np.abs(out.cpu().numpy().astype(np.int16) - comp.astype(np.int16)).max())
            figures.append((t, s, iou, diff, int((got != want).sum())))
    for fgr in figures:
        print("t=%d stream %d: IoU %.6f, composite max |difference| %d, mask bytes that differ %d" % fgr)
    for oc in ocs.values():
        oc.close()
    mg.close()
    for t, s, iou, diff, _ in figures:
        assert iou == 1.0, "t=%d stream %d: mask IoU %.6f" % (t, s, iou)
        assert diff == 0, "t=%d stream %d: composite differs by %d" % (t, s, diff)


# ---- 4. 1920 x 1080 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_full_hd_lite_joins_a_fleet(bs):
    from backscrub_amd import api, synth
    path = model_path("lite")
    geoms = [(640, 480, 1), (1920, 1080, 1)]
    with pytest.raises(api.BsxError, match=r"geoms\[1\] \(1920 x 1080\) is off the fused tile route: width 1920, roi\.x 60 and roi\.w 1799 must be multiples of 4"):
        bs.MaskGen.with_geometries(path, geoms)
    mg = bs.MaskGen.with_geometries(path, geoms, edge_roi=True)
    _check_rois(mg, [((640, 480), [0, 0, 640, 480]), ((1920, 1080), [60, 0, 1799, 1080])])
    twins = [bs.MaskGen(path, W, H, n_streams=1) for W, H, _n in geoms]
    for t in range(2):
        small = synth.frame(480, 270, 1, t)                                # the big frame: rendered at a quarter of the size and repeated
        frames = [_frame(640, 480, 0, t), torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(small, 4, 0), 4, 1))).cuda()]
        bgs = [_image(W, H, 21 + g) for g, (W, H, _n) in enumerate(geoms)]
        items = [_guarded((H, W, 3)) for W, H, _n in geoms]
        flip = t == 1
        mg.step_geoms([1, 0], frames[::-1], [o for _b, o in items][::-1], [bs.StreamSetting(bg=b, flip_h=flip) for b in bgs][::-1])
        for g, (W, H, _n) in enumerate(geoms):
            want = twins[g].step_streams([0], frames[g][None], bgs[g], torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda"), flip_h=flip)
            assert _bands_intact(items[g][0])
            assert torch.equal(items[g][1], want[0]), "t=%d %d x %d: composites differ" % (t, W, H)
            assert torch.equal(mg.masks_of(g), twins[g].masks()[0]) and torch.equal(mg.ofinal()[g], twins[g].ofinal()[0]), "t=%d %d x %d: state differs" % (t, W, H)
    for c in [mg] + twins:
        c.close()


# ---- 5. the vcam step --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_w,out_h,yuyv", [(320, 240, False), (320, 240, True), (480, 270, False)])
def test_vcam_geoms_is_the_resized_composite_of_the_geoms_step(bs, fleets, out_w, out_h, yuyv):
    f = fleets("lite")
    other = bs.MaskGen.with_geometries(f.path, f.geoms, edge_roi=True)     # steps bsx_step_batch_vcam_geoms; the fleet's context steps geoms + resize
    for t, ids in enumerate(_orders(f.n, 3, 14)):
        items = [f.item(s, t, False, False) for s in ids]
        frames, sett = [i[0] for i in items], [i[3] for i in items]
        f.mg.step_geoms(ids, frames, [i[2] for i in items], sett)
        got = [_guarded((out_h, out_w, 2 if yuyv else 3)) for _ in ids]
        other.step_vcam_geoms(ids, frames, [o for _b, o in got], sett, yuyv=yuyv)
        for s, item, (buf, out) in zip(ids, items, got):
            want = f.mg.resize_bgr(item[2][None], out_w, out_h)
            want = (f.mg.bgr_to_yuyv(want) if yuyv else want)[0]
            assert _bands_intact(buf)
            assert torch.equal(out, want), "t=%d stream %d %s -> %d x %d: outputs differ" % (t, s, f.cases[f.cls(s)[0]][0], out_w, out_h)
        for s in range(f.n):
            assert torch.equal(other.masks_of(s), f.mg.masks_of(s)), "t=%d stream %d: persistent masks differ" % (t, s)
        assert torch.equal(other.ofinal(), f.mg.ofinal()), "t=%d: temporal state differs" % t
    other.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_class_and_write_nothing(bs):
    from backscrub_amd import api
    path = model_path("lite")
    L = api.lib()
    # creation: the width (checked by the library too: the binding's own check is bypassed here), a class without the tiled up-scale, an unknown flag bit
    for geoms, flags, words in (([(640, 480, 1), (642, 480, 1)], 1, ["geoms[1]", "642 x 480", "width 642"]),
                                ([(640, 480, 1), (80, 48, 1)], 1, ["geoms[1]", "80 x 48", "fused tile route", "tiled linear"]),
                                ([(640, 480, 1)], 5, ["unknown bit 0x4"])):
        arr = (api._Geometry * len(geoms))(*[api._Geometry(*g) for g in geoms])
        h = L.bsx_new_geoms_ex(path.encode(), 2, arr, len(geoms), 0, flags, api.DEBUG_FN(lambda _c, _m: None), api.STAGE_FN(), api.STAGE_FN(), api.STAGE_FN(), None)
        text = (L.bsx_last_error(None) or b"").decode()
        assert not h, geoms
        for w in words:
            assert w in text, (w, text)
    with pytest.raises(api.BsxError, match="width 642"):
        bs.MaskGen.with_geometries(path, [(642, 480, 1)], edge_roi=True)
    # per item: a YUYV frame for a class with an odd ROI column; the mixed step on a one-class edge context
    W, H = 480, 270
    mg = bs.MaskGen.with_geometries(path, [(W, H, 2)], edge_roi=True)
    _check_rois(mg, [((W, H), [15, 0, 449, 270])])
    buf, out = _guarded((H, W, 3))
    out.fill_(SENTINEL)
    masks, of = mg.masks().clone(), mg.ofinal().clone()
    with pytest.raises(api.BsxError, match=r"items\[0\]: stream 1 is of class 0 \(480 x 270\), which has no fused YUYV prep.*roi\.x 15"):
        mg.step_geoms([1], [_yuyv_frame(mg, W, H, [15, 0, 449, 270], 1, 0)], [out], [bs.StreamSetting(bg=_image(W, H, 5), yuyv_in=True)])
    with pytest.raises(api.BsxError, match=r"needs the fused mask \+ blend geometry"):
        mg.step_mixed(_frame(W, H, 0, 0)[None], out[None], [bs.StreamSetting(bg=_image(W, H, 5))])
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and torch.equal(mg.masks(), masks) and torch.equal(mg.ofinal(), of)
    mg.close()
