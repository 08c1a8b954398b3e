"""BSX_STREAM_YUYV_IN on the GPU: bsx_step_batch_geoms and bsx_step_batch_vcam_geoms with a pixel format per item.  A camera's raw YUYV 4:2:2 frame, read by
the per-position kernels, gives per stream the bytes of (a) bsx_step_batch_mixed(.., BSX_STEP_YUYV_IN) of that stream on a one-geometry context of its size (existing,
oracle-checked code), (b) the same multi-geometry call with that frame first converted by bsx_yuyv_to_bgr, and (c) the CPU oracle run on its own YUYV -> BGR of the
frame: composites, persistent masks and temporal state (`ofinal`), every tick.  Byte equality everywhere; the oracle test asserts IoU 1.0 and a difference of 0.

Fleets are three classes x 2 streams of segm_lite (the smallest network): 320x240 (ROI = frame, bars in the canvas, a partial last tile column and row), 640x360
(ROI (20,0,600,360): strips outside the ROI) and 640x480; each ROI is confirmed from bsx_get_geom_info.  Every run is 4 ticks, which flushes the temporal filter.
YUYV frames are the synthetic BGR frames through the project's own packer, bytes 1 and 3 of each word exchanged (the packer writes Y0 V Y1 U, a camera Y0 U Y1 V)."""
import ctypes

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

QVGA, NHD, VGA = (320, 240), (640, 360), (640, 480)
SIZES = [QVGA, NHD, VGA]
ROIS = {QVGA: [0, 0, 320, 240], NHD: [20, 0, 600, 360], VGA: [0, 0, 640, 480]}
# settings a stream cycles through: (background: "own" / "shared" / None, StreamSetting flags) — the cycle of tests/test_gpu_geoms.py
CYCLE = [("own", {}), ("shared", {}), ("own", {"flip_h": True}), ("shared", {"flip_v": True}), ("own", {"flip_h": True, "flip_v": True}), (None, {"filter_off": True})]
# the positions of the four ticks: classes interleaved, two ticks in which streams sit out
TICKS = [[4, 1, 2, 5, 0, 3], [3, 0, 4], [5, 2, 1, 0], [5, 4, 3, 2, 1, 0]]
BSX_EINVAL = -1


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


_CACHE = {}


def _bgr(W, H, s, t):
    """stream s at tick t as BGR: the photo fixture on streams 4-5 (VGA), else the moving synthetic scene.  Computed once, never written."""
    key = ("bgr", W, H, s, t)
    if key not in _CACHE:
        from backscrub_amd import synth
        if (W, H) == VGA and s >= 4:
            from tools import make_photo_fixture
            _CACHE[key] = torch.from_numpy(np.ascontiguousarray(make_photo_fixture.load_frames()[s - 4])).cuda()
        else:
            _CACHE[key] = torch.from_numpy(synth.frame(W, H, s, t)).cuda()
    return _CACHE[key]


def _yuyv(mg, W, H, s, t):
    """the same frame as a camera delivers it: Y0 U Y1 V.  bsx_bgr_to_yuyv packs Y0 V Y1 U, so bytes 1 and 3 of every macropixel change places."""
    key = ("yuyv", W, H, s, t)
    if key not in _CACHE:
        packed = mg.bgr_to_yuyv(_bgr(W, H, s, t)[None])[0]
        _CACHE[key] = packed.view(H, W // 2, 4)[:, :, [0, 3, 2, 1]].contiguous().view(H, W, 2)
    return _CACHE[key]


def _image(W, H, seed):
    key = ("bg", W, H, seed)
    if key not in _CACHE:
        from backscrub_amd import synth
        _CACHE[key] = torch.from_numpy(synth.background(W, H, seed=seed)).cuda()
    return _CACHE[key]


def _out(W, H, ch, n=None):
    shape = (H, W, ch)
    return torch.zeros(shape if n is None else (n,) + shape, dtype=torch.uint8, device="cuda")


def _check_rois(mg, sizes, rois=ROIS):
    """the ROIs the cases were chosen for (segm_lite's unless given), from bsx_get_geom_info"""
    for g, size in zip(mg.geometries(), sizes):
        assert (g["width"], g["height"]) == size
        assert g["roi"] == rois[size], "%s: ROI %s, the test was written for %s" % (size, g["roi"], rois[size])


class Fleet:
    """one multi-geometry context and one one-geometry twin per class; stream s delivers YUYV where yin(s) (default: the even streams, so the formats alternate
    and every class has one stream of each)."""

    def __init__(self, bs, key="lite", sizes=SIZES, per_class=2, yin=lambda s: s % 2 == 0, rois=ROIS):
        self.bs, self.path, self.yin = bs, model_path(key), yin
        self.geoms = [(W, H, per_class) for W, H in sizes]
        self.n = per_class * len(sizes)
        self.mg = bs.MaskGen.with_geometries(self.path, self.geoms)
        _check_rois(self.mg, sizes, rois)
        self.twins = [bs.MaskGen(self.path, W, H, n_streams=n) for W, H, n in self.geoms]
        self.first = [g["first_stream"] for g in self.mg.geometries()]

    def cls(self, s):
        g = max(i for i, f in enumerate(self.first) if f <= s)
        return g, s - self.first[g]

    def size(self, s):
        return self.geoms[self.cls(s)[0]][:2]

    def frame(self, s, t, fmt=None):
        W, H = self.size(s)
        return _yuyv(self.mg, W, H, s, t) if (self.yin(s) if fmt is None else fmt) else _bgr(W, H, s, t)

    def setting(self, s, t, item=True):
        """the stream's setting at tick t; item: with its format bit (the twins' mixed step takes the format batch-wide and refuses the bit)"""
        g, _ = self.cls(s)
        W, H = self.size(s)
        bg, fl = CYCLE[(s + t) % len(CYCLE)]
        img = None if bg is None else _image(W, H, 100 + s if bg == "own" else 7 + g)
        return self.bs.StreamSetting(bg=img, yuyv_in=item and self.yin(s), **fl)

    def items(self, ids, t, yuyv, behind=()):
        """frames, outputs and settings of one call.  behind: streams whose output lies directly behind the last byte of their frame, in one allocation."""
        frames, outs, sett = [], [], []
        for s in ids:
            W, H = self.size(s)
            fr, och = self.frame(s, t), 2 if yuyv else 3
            if s in behind:
                buf = torch.zeros(fr.numel() + W * H * och, dtype=torch.uint8, device="cuda")
                buf[:fr.numel()] = fr.reshape(-1)
                fr, out = buf[:fr.numel()].view(fr.shape), buf[fr.numel():].view(H, W, och)
                assert out.data_ptr() == fr.data_ptr() + W * H * fr.shape[2] and out.data_ptr() % 4 == 0
            else:
                out = _out(W, H, och)
            frames.append(fr)
            outs.append(out)
            sett.append(self.setting(s, t))
        return frames, outs, sett

    def tick(self, t, ids, yuyv=False, no_mask=False, behind=(), tag=""):
        """one geoms call for the streams `ids` against the twins — per class one mixed call for its YUYV streams (yuyv_in) and one for its BGR streams — then EVERY
        stream's mask and ofinal against its twin's (a stream that sits out keeps its state).  Returns the composites by stream."""
        frames, outs, sett = self.items(ids, t, yuyv, behind)
        self.mg.step_geoms(ids, frames, outs, sett, yuyv=yuyv, no_mask=no_mask)
        for g, (W, H, _n) in enumerate(self.geoms):
            for fmt in (True, False):
                pos = [i for i, s in enumerate(ids) if self.cls(s)[0] == g and self.yin(s) == fmt]
                if not pos:
                    continue
                want = _out(W, H, 2 if yuyv else 3, len(pos))
                self.twins[g].step_mixed(torch.stack([frames[i] for i in pos]), want, [self.setting(ids[i], t, item=False) for i in pos],
                                         ids=[self.cls(ids[i])[1] for i in pos], yuyv=yuyv, no_mask=no_mask, yuyv_in=fmt)
                for k, i in enumerate(pos):
                    assert torch.equal(outs[i], want[k]), "%st=%d stream %d (%dx%d, %s): composites differ" % (tag, t, ids[i], W, H, "YUYV" if fmt else "BGR")
        self.compare_state(t, masks=not no_mask, tag=tag)
        return dict(zip(ids, outs))

    def compare_state(self, t, masks=True, tag=""):
        of = self.mg.ofinal()
        for s in range(self.n):
            g, k = self.cls(s)
            assert torch.equal(of[s], self.twins[g].ofinal()[k]), "%st=%d stream %d: temporal state differs" % (tag, t, s)
            if masks:
                assert torch.equal(self.mg.masks_of(s), self.twins[g].masks()[k]), "%st=%d stream %d: persistent masks differ" % (tag, t, s)

    def run(self, tag="", **batch):
        return [{s: o.cpu() for s, o in self.tick(t, ids, tag=tag, **batch).items()} for t, ids in enumerate(TICKS)]

    def close(self):
        for c in [self.mg] + self.twins:
            c.close()


# ---- 1. mixed formats in one call, against the twins ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [{}, {"yuyv": True}, {"no_mask": True}], ids=["bgr", "yuyv", "no_mask"])
def test_mixed_formats_in_one_call_equal_the_twins(bs, batch):
    f = Fleet(bs)
    assert [f.yin(s) for s in range(f.n)] == [True, False] * 3
    f.run(**batch)
    f.close()


# ---- 2. against convert-then-step ---------------------------------------------------------------------------------------------------------------------------
def test_equals_the_bgr_call_on_converted_frames(bs):
    """a second multi-geometry context takes the same items with every YUYV frame first converted by bsx_yuyv_to_bgr: every byte is equal"""
    f = Fleet(bs)
    other = bs.MaskGen.with_geometries(f.path, f.geoms)
    for t, ids in enumerate(TICKS):
        frames, outs, sett = f.items(ids, t, False)
        f.mg.step_geoms(ids, frames, outs, sett)
        conv = [other.yuyv_to_bgr(fr[None])[0] if f.yin(s) else fr for s, fr in zip(ids, frames)]
        want = [torch.zeros_like(o) for o in outs]
        other.step_geoms(ids, conv, want, [f.setting(s, t, item=False) for s in ids])
        for s, a, b in zip(ids, outs, want):
            assert torch.equal(a, b), "t=%d stream %d: composites differ" % (t, s)
        assert torch.equal(f.mg.ofinal(), other.ofinal()), "t=%d: temporal state differs" % t
        for s in range(f.n):
            assert torch.equal(f.mg.masks_of(s), other.masks_of(s)), "t=%d stream %d: persistent masks differ" % (t, s)
    other.close()
    f.close()


# ---- 3. against the CPU oracle ----------------------------------------------------------------------------------------------------------------------------------
def test_one_yuyv_stream_per_class_against_the_oracle(bs, oracle):
    """one stream per class, all YUYV, against the CPU oracle run on the oracle's own YUYV -> BGR of the same frames, from a reset state: the bar of
    test_one_stream_per_class_against_the_oracle (mask IoU 1.0, composite difference 0).  The figures are printed before they are asserted."""
    from backscrub_amd import synth
    path = model_path("lite")
    mg = bs.MaskGen.with_geometries(path, [(W, H, 2) for W, H in SIZES])
    _check_rois(mg, SIZES)
    ids = [2 * g + 1 for g in range(len(SIZES))][::-1]
    size = {s: SIZES[s // 2] for s in ids}
    bgs = {s: synth.background(size[s][0], size[s][1], seed=3 + s) for s in ids}
    ocs = {s: oracle.Ctx(path, size[s][0], size[s][1]) for s in ids}
    figures = []
    for t in range(4):
        raw = {s: _yuyv(mg, size[s][0], size[s][1], s, t) for s in ids}
        outs = [_out(size[s][0], size[s][1], 3) for s in ids]
        mg.step_geoms(ids, [raw[s] for s in ids], outs, [bs.StreamSetting(bg=torch.from_numpy(bgs[s]).cuda(), yuyv_in=True) for s in ids])
        torch.cuda.synchronize()
        for i, s in enumerate(ids):
            host = oracle.yuyv_to_bgr(raw[s].cpu().numpy())
            want = ocs[s].process(host)
            got = mg.masks_of(s).cpu().numpy()
            fa, fb = got < 128, want < 128
            union = np.logical_or(fa, fb).sum()
            iou = 1.0 if union == 0 else float(np.logical_and(fa, fb).sum()) / float(union)
            comp = oracle.alpha_blend(bgs[s], host, want)
            diff = int(np.abs(outs[i].cpu().numpy().astype(np.int16) - comp.astype(np.int16)).max())
            figures.append((t, s, size[s], iou, diff, int((got != want).sum()), float(fb.mean())))
    for fgr in figures:
        print("t=%d stream %d %s: IoU %.6f, composite max |difference| %d, mask bytes that differ %d, oracle foreground share %.3f" % fgr)
    for oc in ocs.values():
        oc.close()
    mg.close()
    for t, s, sz, iou, diff, _, _ in figures:
        assert iou == 1.0, "t=%d stream %d %s: mask IoU %.6f" % (t, s, sz, iou)
        assert diff == 0, "t=%d stream %d %s: composite differs by %d" % (t, s, sz, diff)


# ---- 4. the uniform-tile shortcut off: every tile takes the general body ------------------------------------------------------------------------------------
def test_without_the_uniform_tile_shortcut(bs, monkeypatch):
    f = Fleet(bs)
    default = f.run()
    f.close()
    monkeypatch.setenv("BSX_NO_UNIFORM_TILES", "1")
    f = Fleet(bs)
    general = f.run(tag="general path: ")
    f.close()
    assert len(default) == len(general) == len(TICKS)
    for t, (a, b) in enumerate(zip(default, general)):
        assert a.keys() == b.keys()
        for s in a:
            assert torch.equal(a[s], b[s]), "t=%d stream %d: the general path differs from the default run" % (t, s)


# ---- 5. MLKit: a ROI with strips on both sides, filtered and filter-off YUYV streams --------------------------------------------------------------------------
@pytest.mark.parametrize("yuyv", [False, True], ids=["bgr_out", "yuyv_out"])
def test_mlkit_yuyv_items_and_the_strips_outside_the_roi(bs, yuyv):
    f = Fleet(bs, "mlkit", [VGA], per_class=3, yin=lambda s: True, rois={VGA: [80, 0, 480, 480]})
    S = bs.StreamSetting
    bg = _image(640, 480, 11)
    settings = [S(bg=bg, yuyv_in=True), S(filter_off=True, yuyv_in=True), S(bg=bg, flip_h=True, yuyv_in=True), S(filter_off=True, flip_v=True, yuyv_in=True)]
    och = 2 if yuyv else 3
    for t in range(4):
        ids = [2, 0, 1]
        sett = [settings[(s + t) % 4] for s in ids]                       # every stream is filtered in some ticks and filter-off in others
        frames = [f.frame(s, t) for s in ids]
        outs = [_out(640, 480, och) for _ in ids]
        f.mg.step_geoms(ids, frames, outs, sett, yuyv=yuyv)
        want = _out(640, 480, och, 3)
        f.twins[0].step_mixed(torch.stack(frames), want, [S(bg=q.bg, flip_h=q.flip_h, flip_v=q.flip_v, filter_off=q.filter_off) for q in sett], ids=ids, yuyv=yuyv,
                              yuyv_in=True)
        for k, s in enumerate(ids):
            for name, cols in (("left strip", slice(0, 80)), ("right strip", slice(560, 640)), ("ROI", slice(80, 560))):
                assert torch.equal(outs[k][:, cols], want[k][:, cols]), "t=%d stream %d (%s): %s differs" % (t, s, sett[k], name)
        f.compare_state(t)
    f.close()


# ---- 6. the step at the virtual camera's geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yuyv", [False, True], ids=["bgr_out", "yuyv_out"])
@pytest.mark.parametrize("ow,oh", [(426, 240), (320, 240), (640, 360)], ids=["426x240", "320x240", "640x360"])
def test_vcam_geoms_with_mixed_formats(bs, ow, oh, yuyv):
    """426x240: no class has an integer ratio; 320x240: exactly 2x for VGA (the area mean) and QVGA's own size; 640x360: one class's own size.  Against step_geoms
    with the same items on a second context, then bsx_resize_bgr [+ bsx_bgr_to_yuyv] of each composite; masks and ofinal of every stream equal that call's."""
    f = Fleet(bs)
    other = bs.MaskGen.with_geometries(f.path, f.geoms)
    for t, ids in enumerate(TICKS):
        frames, _, sett = f.items(ids, t, False)
        outs = [_out(ow, oh, 2 if yuyv else 3) for _ in ids]
        f.mg.step_vcam_geoms(ids, frames, outs, sett, yuyv=yuyv)
        comps = [_out(*f.size(s), 3) for s in ids]
        other.step_geoms(ids, frames, comps, sett)
        for s, got, comp in zip(ids, outs, comps):
            r = other.resize_bgr(comp[None], ow, oh)
            want = (other.bgr_to_yuyv(r) if yuyv else r)[0]
            assert torch.equal(got, want), "t=%d stream %d %s (%s): outputs differ" % (t, s, f.size(s), "YUYV" if f.yin(s) else "BGR")
        assert torch.equal(f.mg.ofinal(), other.ofinal()), "t=%d: temporal state differs" % t
        for s in range(f.n):
            assert torch.equal(f.mg.masks_of(s), other.masks_of(s)), "t=%d stream %d: persistent masks differ" % (t, s)
    other.close()
    f.close()


# ---- 7. refusals change nothing; an output directly behind a YUYV frame is taken --------------------------------------------------------------------------------
def _raw_call(api, mg, entry, ids, frames, outs, sett, flags, out_size=None):
    """the C entry point itself, for arguments MaskGen does not let through: (return code, error text)"""
    n = len(ids)
    arr = (ctypes.c_int * n)(*ids)
    items = (api._GeomItem * n)()
    for i in range(n):
        items[i].d_frame, items[i].d_out = frames[i].data_ptr(), outs[i].data_ptr()
        items[i].setting.d_bg = sett[i].bg.data_ptr() if sett[i].bg is not None else None
        items[i].setting.flags = sett[i].flags()
    fn = getattr(api.lib(), entry)
    rc = fn(mg.h, arr, items, n, None, flags) if out_size is None else fn(mg.h, arr, items, n, out_size[0], out_size[1], None, flags)
    return rc, (api.lib().bsx_last_error(mg.h) or b"").decode(errors="replace")


def test_refusals_leave_every_stream_unchanged(bs):
    from backscrub_amd import api
    S = bs.StreamSetting
    f = Fleet(bs)
    for t in range(3):
        f.tick(t, TICKS[0])
    total = sum(W * H * n for W, H, n in f.geoms)
    masks, of = f.mg._view(3, "uint8", (total,)).clone(), f.mg.ofinal().clone()

    # a YUYV item in a class whose down-scale is the exact 2x2 area mean: 256x192 -> segm_lite's 128x96
    area = bs.MaskGen.with_geometries(f.path, [(256, 192, 1), (640, 480, 1)])
    g0 = area.geometries()[0]
    assert g0["roi"] == [0, 0, 256, 192] and g0["in_roi"][2:] == [128, 96], g0
    a_masks, a_of = area._view(3, "uint8", (256 * 192 + 640 * 480,)).clone(), area.ofinal().clone()
    a_frames = [_yuyv(area, 640, 480, 1, 0), _yuyv(area, 256, 192, 0, 0)]
    a_sett = [S(bg=_image(640, 480, 50), yuyv_in=True), S(bg=_image(256, 192, 50), yuyv_in=True)]
    for step, outs in ((area.step_geoms, [_out(640, 480, 3), _out(256, 192, 3)]), (area.step_vcam_geoms, [_out(320, 240, 3), _out(320, 240, 3)])):
        with pytest.raises(api.BsxError) as e:
            step([1, 0], a_frames, outs, a_sett)
        for word in ("items[1]", "stream 0", "256 x 192", "2x2 area", "bsx_yuyv_to_bgr"):
            assert word in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(area._view(3, "uint8", (256 * 192 + 640 * 480,)), a_masks) and torch.equal(area.ofinal(), a_of)
    area.close()

    # an output that overlaps the last byte of a YUYV frame (stream 4: VGA, YUYV)
    W, H = f.size(4)
    raw = f.frame(4, 9)
    last = W * H * 2 - 4                                                    # the 4-byte aligned offset whose word holds the frame's last byte
    buf = torch.zeros(last + W * H * 3, dtype=torch.uint8, device="cuda")
    buf[:W * H * 2] = raw.reshape(-1)
    fr = buf[:W * H * 2].view(H, W, 2)
    for step, o in ((f.mg.step_geoms, buf[last:].view(H, W, 3)), (f.mg.step_vcam_geoms, buf[last:last + 320 * 240 * 3].view(240, 320, 3))):
        with pytest.raises(api.BsxError, match=r"items\[0\]: d_out .* overlaps a frame or background of items\[0\]"):
            step([4], [fr], [o], [S(bg=_image(W, H, 50), yuyv_in=True)])

    # the batch-wide flag stays refused on both entry points
    ids = [4, 1]
    frames, outs, sett = f.items(ids, 9, False)
    for entry, size in (("bsx_step_batch_geoms", None), ("bsx_step_batch_vcam_geoms", (320, 240))):
        o = outs if size is None else [_out(320, 240, 3) for _ in ids]
        rc, text = _raw_call(api, f.mg, entry, ids, frames, o, sett, 0x10, size)
        assert rc == BSX_EINVAL and "flags 0x10" in text and "YUYV input" in text, (entry, rc, text)

    # the mixed steps take one packed array with one layout: bit 64 in a setting is refused there, with the text they had
    twin = f.twins[2]
    for step, o in ((twin.step_mixed, _out(640, 480, 3, 1)), (twin.step_vcam_mixed, _out(320, 240, 3, 1))):
        with pytest.raises(api.BsxError, match=r"settings\[0\]: flags 0x40 has bits outside flip / blur / filter-off"):
            step(_bgr(640, 480, 4, 9)[None], o, [S(bg=_image(640, 480, 50), yuyv_in=True)], ids=[0])

    # a BGR tensor where the item announces YUYV never reaches the library
    for step, o in ((f.mg.step_geoms, _out(W, H, 3)), (f.mg.step_vcam_geoms, _out(320, 240, 3))):
        with pytest.raises(ValueError, match=r"frames\[0\].*\[480,640,2\].*YUYV item"):
            step([4], [_bgr(W, H, 4, 9)], [o], [S(bg=_image(W, H, 50), yuyv_in=True)])
    with pytest.raises(ValueError, match=r"frames\[0\].*\[480,640,3\]"):
        f.mg.step_geoms([4], [raw], [_out(W, H, 3)], [S(bg=_image(W, H, 50))])

    torch.cuda.synchronize()
    assert torch.equal(f.mg._view(3, "uint8", (total,)), masks) and torch.equal(f.mg.ofinal(), of)
    f.compare_state(3)
    # ... and an output placed directly behind the W * H * 2 bytes of a YUYV frame is accepted and correct: the context goes on, against its twins
    f.tick(3, TICKS[3], behind={4, 0, 2})
    f.tick(4, TICKS[0], yuyv=True, behind={4, 2})
    f.close()
