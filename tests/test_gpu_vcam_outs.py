"""bsx_step_batch_vcam_geoms_outs on the GPU: one step, several outputs per stream, each of its own size.  The yardstick is the sequence the call replaces, as in
tests/test_gpu_vcam_geoms.py: a twin context of the same classes runs step_geoms into capture-size composites, then resize_bgr [+ bgr_to_yuyv] per output record.
Byte equality throughout; after every tick the persistent mask and the temporal state (`ofinal`) of ALL streams are compared with the twin's.

The fleet is segm_lite with VGA, 1280x720 and 640x360, two streams each (the smallest classes the suite knows to be on the fused route), settings cycling as
tests/test_gpu_vcam_geoms.py's CYCLE.  Every output lies between two sentinel bands that must survive the call."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD, FHD, NHD = (640, 480), (1280, 720), (1920, 1080), (640, 360)
LITE = [VGA, HD, NHD]
SIM = [(640, 360), (320, 180), (160, 90)]
CYCLE = [("own", {}), ("shared", {}), ("own", {"flip_h": True}), ("shared", {"flip_v": True}), ("own", {"flip_h": True, "flip_v": True}), (None, {"filter_off": True})]
BAND, SENTINEL = 64, 0xA5
BSX_EINVAL = -1


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


@functools.lru_cache(maxsize=None)
def _frame(W, H, s, t):
    """stream s at tick t: the moving synthetic scene.  Computed once, never written."""
    from backscrub_amd import synth
    return torch.from_numpy(synth.frame(W, H, s, t)).cuda()


@functools.lru_cache(maxsize=None)
def _image(W, H, seed):
    from backscrub_amd import synth
    return torch.from_numpy(synth.background(W, H, seed=seed)).cuda()


def _guarded(W, H, ch):
    """an output of 0x5a between two BAND-byte sentinel bands, in one allocation: (whole buffer, the output's view)"""
    n = W * H * ch
    buf = torch.full((n + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[BAND:BAND + n].view(H, W, ch)
    out.fill_(0x5a)
    assert out.data_ptr() % 4 == 0
    return buf, out


def _bands_intact(buf):
    return bool((buf[:BAND] == SENTINEL).all()) and bool((buf[-BAND:] == SENTINEL).all())


class Fleet:
    """two contexts of the same classes: `mg` takes the new call, `twin` the sequence it replaces"""

    def __init__(self, bs, key, sizes, per_class=2):
        self.bs, self.path = bs, model_path(key)
        self.geoms = [(W, H, per_class) for W, H in sizes]
        self.n = per_class * len(sizes)
        self.mg = bs.MaskGen.with_geometries(self.path, self.geoms)
        self.twin = bs.MaskGen.with_geometries(self.path, self.geoms)
        self.first = [g["first_stream"] for g in self.mg.geometries()]
        self.t = 0
        self.yin = set()                 # streams that deliver YUYV frames

    def size(self, s):
        g = max(i for i, f in enumerate(self.first) if f <= s)
        return self.geoms[g][0], self.geoms[g][1], g

    def frame(self, s, t):
        W, H, _g = self.size(s)
        f = _frame(W, H, s, t)
        if s in self.yin:                # as a camera delivers it, Y0 U Y1 V: the project's packer writes Y0 V Y1 U
            return self.twin.bgr_to_yuyv(f[None])[0].view(H, W // 2, 4)[:, :, [0, 3, 2, 1]].contiguous().view(H, W, 2)
        return f

    def setting(self, s, t):
        W, H, g = self.size(s)
        bg, fl = CYCLE[(s + t) % len(CYCLE)]
        img = None if bg is None else _image(W, H, 100 + s if bg == "own" else 7 + g)
        return self.bs.StreamSetting(bg=img, yuyv_in=s in self.yin, **fl)

    def tick(self, ids, records, yuyv=False, tag=""):
        """one call: positions `ids`, records (stream, (out_w, out_h)) in the caller's order.  Returns the outputs in record order."""
        t = self.t
        self.t += 1
        ch = 2 if yuyv else 3
        frames = [self.frame(s, t) for s in ids]
        sett = [self.setting(s, t) for s in ids]
        bufs = [_guarded(ow, oh, ch) for _s, (ow, oh) in records]
        self.mg.step_vcam_geoms_outs(ids, frames, sett, [(ids.index(s), o) for (s, _z), (_b, o) in zip(records, bufs)], yuyv=yuyv)
        comps = {s: torch.full((self.size(s)[1], self.size(s)[0], 3), 0x5a, dtype=torch.uint8, device="cuda") for s in ids}
        self.twin.step_geoms(ids, frames, [comps[s] for s in ids], sett)
        want = {}
        for (s, (ow, oh)), (buf, out) in zip(records, bufs):
            if (s, ow, oh) not in want:
                r = self.twin.resize_bgr(comps[s][None], ow, oh)
                want[(s, ow, oh)] = (self.twin.bgr_to_yuyv(r) if yuyv else r)[0]
            W, H, _g = self.size(s)
            what = "%st=%d stream %d (%dx%d -> %dx%d%s, %s)" % (tag, t, s, W, H, ow, oh, " yuyv" if yuyv else "", CYCLE[(s + t) % len(CYCLE)])
            assert _bands_intact(buf), what + ": a guard band of d_out was written"
            bad = (out != want[(s, ow, oh)]).any(-1)
            assert not bool(bad.any()), "%s: %d output pixels differ, first at (y, x) = %s" % (what, int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]))
        self.compare_state(t, tag)
        return [o for _b, o in bufs]

    def compare_state(self, t, tag=""):
        of, of_twin = self.mg.ofinal(), self.twin.ofinal()
        for s in range(self.n):
            assert torch.equal(of[s], of_twin[s]), "%st=%d stream %d: temporal state differs" % (tag, t, s)
            assert torch.equal(self.mg.masks_of(s), self.twin.masks_of(s)), "%st=%d stream %d: persistent masks differ" % (tag, t, s)

    def subsets(self, ticks, seed):
        """everyone first, then a different subset each tick, in a seeded order that interleaves the classes"""
        rng = np.random.default_rng(7000 + seed)
        for k in range(ticks):
            ids = [int(i) for i in rng.permutation(self.n)]
            yield ids if k == 0 else ids[:int(rng.integers(self.n // 2, self.n))]

    def close(self):
        for c in (self.mg, self.twin):
            c.close()


@pytest.fixture(scope="module")
def lite(bs):
    f = Fleet(bs, "lite", LITE)
    yield f
    f.close()


# ---- 1. simulcast ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yuyv", [False, True], ids=["bgr", "yuyv"])
def test_simulcast_three_layers_per_stream(lite, yuyv):
    """640x360 is identity for one class, the exact 2x area mean for another (1280x720) and an aspect change for the third (VGA)"""
    for ids in lite.subsets(4, int(yuyv)):
        lite.tick(ids, [(s, z) for s in ids for z in SIM], yuyv=yuyv)


# ---- 2. speaker and thumbnails --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speaker", [0, 3, 4])
def test_speaker_and_thumbnails(lite, speaker):
    """one stream at 1280x720 (an up-scale for VGA and 640x360), the rest at 320x180, two items without a record; the records in a seeded shuffle"""
    ids = [4, 1, 2, 5, 0, 3]
    silent = [s for s in ids if s != speaker][:2]
    recs = [(s, HD if s == speaker else (320, 180)) for s in ids if s not in silent]
    rng = np.random.default_rng(speaker)
    lite.tick(ids, [recs[j] for j in rng.permutation(len(recs))], yuyv=bool(speaker % 2))


# ---- 3. twelve groups, ragged tiles and stores ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,yuyv", [([(427, 240), (426, 240), (66, 34), (64, 32)], False), ([(426, 240), (66, 34), (64, 32), (160, 90)], True)], ids=["bgr", "yuyv"])
def test_twelve_groups_with_ragged_tiles_and_stores(lite, sizes, yuyv):
    """427: odd width, byte-wise stores; 426: w % 4 == 2; 66x34: one pixel group past one 64x32 tile in both directions; 64x32: exactly one tile"""
    for ids in lite.subsets(2, 10 + int(yuyv)):
        rng = np.random.default_rng(len(ids))
        recs = [(s, z) for z in sizes for s in ids]
        lite.tick(ids, [recs[j] for j in rng.permutation(len(recs))], yuyv=yuyv)


# ---- 4. one item named four times -----------------------------------------------------------------------------------------------------------------------------------
def test_one_item_named_four_times(lite):
    ids = [3, 0, 5]
    outs = lite.tick(ids, [(0, (640, 360)), (3, (320, 180)), (0, (160, 90)), (0, (640, 360)), (0, (320, 180))])
    assert outs[0].data_ptr() != outs[3].data_ptr() and torch.equal(outs[0], outs[3])


# ---- 5. YUYV and BGR items in one call ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yuyv", [False, True], ids=["bgr_out", "yuyv_out"])
def test_yuyv_and_bgr_items_in_one_call(bs, yuyv):
    """the _fmt kernel: 320x240, 640x360 and VGA (the classes tests/test_gpu_geoms_yuyv_in.py knows to have the fused YUYV prep), the even streams YUYV"""
    f = Fleet(bs, "lite", [(320, 240), NHD, VGA])
    f.yin = {0, 2, 4}
    try:
        for ids in f.subsets(3, 20 + int(yuyv)):
            f.tick(ids, [(s, z) for z in [(426, 240), (160, 90)] for s in ids], yuyv=yuyv)
    finally:
        f.close()


# ---- 6. an edge context ---------------------------------------------------------------------------------------------------------------------------------------------
def test_edge_context_against_one_geometry_contexts(bs):
    """edge_roi=True with VGA + 1920x1080 (segm_lite's ROI there is off the 4-pixel grid), against step_streams + resize on one-geometry contexts, as
    tests/test_gpu_geoms_edge.py does"""
    path = model_path("lite")
    geoms = [(VGA[0], VGA[1], 2), (FHD[0], FHD[1], 2)]
    mg = bs.MaskGen.with_geometries(path, geoms, edge_roi=True)
    twins = [bs.MaskGen(path, W, H, n_streams=n) for W, H, n in geoms]
    try:
        roi = mg.geometries()[1]["roi"]
        assert roi[0] % 4 or roi[2] % 4, "1920x1080: ROI %s is on the 4-pixel grid, the test was written for one that is not" % (roi,)
        for t, ids in enumerate([[2, 0, 3, 1], [1, 3], [3, 2, 0]]):
            sett, frames = [], []
            for s in ids:
                W, H, _n = geoms[s // 2]
                bg, fl = CYCLE[(s + t) % len(CYCLE)]
                sett.append(bs.StreamSetting(bg=None if bg is None else _image(W, H, 100 + s if bg == "own" else 7 + s // 2), **fl))
                frames.append(_frame(W, H, s, t))
            recs = [(i, z) for z in [(640, 360), (426, 240)] for i in range(len(ids))]
            bufs = [_guarded(ow, oh, 3) for _i, (ow, oh) in recs]
            mg.step_vcam_geoms_outs(ids, frames, sett, [(i, o) for (i, _z), (_b, o) in zip(recs, bufs)])
            comp = {}
            for i, s in enumerate(ids):
                g, loc = s // 2, s % 2
                W, H, _n = geoms[g]
                tw, st = twins[g], sett[i]
                out = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
                if st.filter_off:
                    tw.step_streams([loc], frames[i][None], _image(W, H, 7 + g), out)             # state and mask advance; the composite is the frame's
                    c = frames[i][None]
                    if st.flip_h or st.flip_v:
                        c = tw.flip_bgr(c, -1 if st.flip_h and st.flip_v else (1 if st.flip_h else 0))
                    comp[i] = c
                else:
                    comp[i] = tw.step_streams([loc], frames[i][None], st.bg, out, flip_h=st.flip_h, flip_v=st.flip_v)
            for (i, (ow, oh)), (buf, out) in zip(recs, bufs):
                assert _bands_intact(buf)
                assert torch.equal(out, twins[ids[i] // 2].resize_bgr(comp[i], ow, oh)[0]), "t=%d stream %d -> %dx%d: outputs differ" % (t, ids[i], ow, oh)
            of = mg.ofinal()
            for s in range(4):
                assert torch.equal(of[s], twins[s // 2].ofinal()[s % 2]), "t=%d stream %d: temporal state differs" % (t, s)
                assert torch.equal(mg.masks_of(s), twins[s // 2].masks()[s % 2]), "t=%d stream %d: persistent masks differ" % (t, s)
    finally:
        for c in [mg] + twins:
            c.close()


# ---- 7. one record per item, one size: step_vcam_geoms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yuyv", [False, True], ids=["bgr", "yuyv"])
def test_one_record_per_item_is_step_vcam_geoms(lite, yuyv):
    ow, oh, ch = 426, 240, 2 if yuyv else 3
    for ids in lite.subsets(2, 30 + int(yuyv)):
        t = lite.t
        lite.t += 1
        frames, sett = [lite.frame(s, t) for s in ids], [lite.setting(s, t) for s in ids]
        bufs = [_guarded(ow, oh, ch) for _ in ids]
        lite.mg.step_vcam_geoms_outs(ids, frames, sett, [(i, o) for i, (_b, o) in enumerate(bufs)], yuyv=yuyv)
        wants = [torch.full((oh, ow, ch), 0x5a, dtype=torch.uint8, device="cuda") for _ in ids]
        lite.twin.step_vcam_geoms(ids, frames, wants, sett, yuyv=yuyv)
        for s, (buf, out), want in zip(ids, bufs, wants):
            assert _bands_intact(buf) and torch.equal(out, want), "t=%d stream %d: differs from step_vcam_geoms" % (t, s)
        lite.compare_state(t)


def test_on_a_context_made_by_bsx_new(bs):
    W, H = VGA
    path = model_path("lite")
    mg, twin = bs.MaskGen(path, W, H, n_streams=4), bs.MaskGen(path, W, H, n_streams=4)
    try:
        for t, ids in enumerate([[2, 0, 3, 1], [3, 1], [1, 3, 0, 2]]):
            frames = [_frame(W, H, s, t) for s in ids]
            sett = []
            for s in ids:
                bg, fl = CYCLE[(s + t) % len(CYCLE)]
                sett.append(bs.StreamSetting(bg=None if bg is None else _image(W, H, 100 + s if bg == "own" else 7), **fl))
            bufs = [_guarded(426, 240, 3) for _ in ids]
            mg.step_vcam_geoms_outs(ids, frames, sett, [(i, o) for i, (_b, o) in enumerate(bufs)])
            want = [torch.full((240, 426, 3), 0x5a, dtype=torch.uint8, device="cuda") for _ in ids]
            twin.step_vcam_geoms(ids, frames, want, sett)
            for s, (buf, out), w in zip(ids, bufs, want):
                assert _bands_intact(buf) and torch.equal(out, w), "t=%d stream %d: differs from step_vcam_geoms" % (t, s)
            assert torch.equal(mg.masks(), twin.masks()) and torch.equal(mg.ofinal(), twin.ofinal()), "t=%d: state differs" % t
    finally:
        mg.close()
        twin.close()


# ---- 8. the per-tap form forced -------------------------------------------------------------------------------------------------------------------------------------
def test_forced_per_tap_form_gives_the_same_bytes(debug_switches, monkeypatch):
    """BSX_VCAM_DIRECT (debug library) forces the per-tap form on every class: the same bytes as the staged form, and both equal the separate calls"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    res = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("BSX_VCAM_DIRECT", env)
        f = Fleet(debug_switches, "lite", LITE)
        try:
            got = []
            for ids in f.subsets(2, 40):
                got += [o.cpu() for o in f.tick(ids, [(s, z) for z in [(426, 240), (160, 90)] for s in ids], tag="direct=%s " % env)]
            torch.cuda.synchronize()
            res.append(got)
        finally:
            f.close()
    assert len(res[0]) == len(res[1]) > 0
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), "record %d: the per-tap form differs from the staged one" % k


# ---- 9. no record at all --------------------------------------------------------------------------------------------------------------------------------------------
def test_no_records_is_a_masks_only_step(lite):
    for ids in ([5, 0, 2], [1, 4, 3, 0]):
        lite.tick(ids, [])


# ---- 10. MLKit ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_mlkit_two_sizes(bs):
    f = Fleet(bs, "mlkit", [VGA, FHD])
    try:
        for ids in f.subsets(2, 50):
            f.tick(ids, [(s, z) for s in ids for z in [(854, 480), (320, 180)]])
    finally:
        f.close()


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(lite):
    from backscrub_amd import api
    f = lite
    f.tick([5, 0, 3, 1, 4, 2], [(s, (320, 180)) for s in range(6)])
    total = sum(W * H * n for W, H, n in f.geoms)
    masks, of = f.mg._view(3, "uint8", (total,)).clone(), f.mg.ofinal().clone()
    ids = [4, 0, 2]
    frames = [_frame(*f.size(s)[:2], s, 9) for s in ids]
    bgs = [_image(*f.size(s)[:2], 50) for s in ids]
    pool = [torch.full((360 * 640 * 3 + 8,), 0x5a, dtype=torch.uint8, device="cuda") for _ in range(6)]

    def raw(recs, n=3, m=None, flags=0, null_outs=False, item_flags=(0, 0, 0), frame_ptrs=None):
        """the C entry point itself: records (item, out_w, out_h, address); (return code, error text)"""
        arr = (ctypes.c_int * 3)(*ids)
        items = (api._GeomItem * 3)()
        for i in range(3):
            items[i].d_frame = frame_ptrs[i] if frame_ptrs else frames[i].data_ptr()
            items[i].d_out = None
            items[i].setting.d_bg, items[i].setting.flags = bgs[i].data_ptr(), item_flags[i]
        out = (api._VcamOut * max(len(recs), 1))()
        for j, (item, w, h, p) in enumerate(recs):
            out[j].item, out[j].out_w, out[j].out_h, out[j].d_out = item, w, h, p
        rc = api.lib().bsx_step_batch_vcam_geoms_outs(f.mg.h, arr, items, n, None if null_outs else out, len(recs) if m is None else m, None, flags)
        return rc, (api.lib().bsx_last_error(f.mg.h) or b"").decode(errors="replace")
    P = [p.data_ptr() for p in pool]
    assert all(p % 4 == 0 for p in P)
    ok = [(0, 320, 180, P[0]), (1, 160, 90, P[1]), (2, 320, 180, P[2])]
    cases = [
        (dict(recs=ok, null_outs=True), "outs is NULL with m = 3"),
        (dict(recs=ok, m=-1), "m = -1 is negative"),
        (dict(recs=ok + [(3, 64, 32, P[3])]), "outs[3]: item 3 is outside [0, 3)"),
        (dict(recs=ok + [(-1, 64, 32, P[3])]), "outs[3]: item -1 is outside [0, 3)"),
        (dict(recs=ok + [(0, 64, 32, P[3]), (0, 64, 32, P[4]), (0, 64, 32, P[5]), (0, 64, 32, P[5] + 64 * 32 * 3 + 4)]), "outs[6]: record 5 of items[0]"),
        (dict(recs=ok + [(0, 64, 32, P[3]), (1, 66, 34, P[4]), (2, 68, 36, P[5])]), "outs[5]: 68 x 36 is distinct output size 5"),
        (dict(recs=ok + [(1, 0, 32, P[3])]), "outs[3]: output size 0 x 32 must be positive"),
        (dict(recs=ok + [(1, 64, -1, P[3])]), "outs[3]: output size 64 x -1 must be positive"),
        (dict(recs=[(0, 321, 180, P[0])], flags=1), "outs[0]: YUYV output needs an even width (out_w = 321)"),
        (dict(recs=ok + [(1, 64, 32, 0)]), "outs[3]: d_out is NULL"),
        (dict(recs=ok + [(1, 64, 32, P[3] + 2)]), "outs[3]: d_out 0x%x is not 4-byte aligned" % (P[3] + 2)),
        (dict(recs=ok + [(1, 64, 32, P[0] + 320 * 180 * 3 - 4)]), "outs[3]: d_out 0x%x overlaps the output of outs[0]" % (P[0] + 320 * 180 * 3 - 4)),
        (dict(recs=ok + [(1, 64, 32, frames[2].data_ptr() + 1280 * 720 * 3 - 4)]), "overlaps a frame or background of items[2]"),
        (dict(recs=ok + [(1, 64, 32, bgs[0].data_ptr())]), "overlaps a frame or background of items[0]"),
        # a YUYV item's frame is W * H * 2 bytes: an output across its last bytes overlaps it
        (dict(recs=ok + [(1, 64, 32, frames[1].data_ptr() + 640 * 480 * 2 - 4)], item_flags=(0, 64, 0)), "overlaps a frame or background of items[1]"),
        (dict(recs=ok, flags=8), "no vcam form"),
        (dict(recs=ok, flags=16), "YUYV input"),
        (dict(recs=ok, flags=2), "outside yuyv"),
        (dict(recs=ok, item_flags=(0, 0x700, 0)), "items[1]: setting flags 0x700 asks for a background blur"),
        (dict(recs=ok, item_flags=(0, 0, 128)), "items[2]: setting flags 0x80 has bits outside"),
        (dict(recs=ok, frame_ptrs=[frames[0].data_ptr(), 0, frames[2].data_ptr()]), "items[1]: d_frame is NULL"),
        (dict(recs=ok, frame_ptrs=[frames[0].data_ptr() + 2, frames[1].data_ptr(), frames[2].data_ptr()]), "is not 4-byte aligned"),
    ]
    for kw, words in cases:
        rc, text = raw(**kw)
        assert rc == BSX_EINVAL and words in text, (kw, rc, text)
        assert "BSX_" not in text, text
    saved = ids
    ids = [4, 0, 4]
    rc, text = raw(ok)
    assert rc == BSX_EINVAL and "repeats" in text, text
    ids = [4, 0, 6]
    rc, text = raw(ok)
    assert rc == BSX_EINVAL and "out of range" in text, text
    ids = saved
    assert raw(ok, n=0)[0] == 0                                                       # n == 0: nothing to do
    # the binding's own refusal
    with pytest.raises(api.BsxError, match=r"outs\[0\]: item 3"):
        f.mg.step_vcam_geoms_outs(ids, frames, [f.bs.StreamSetting(bg=b) for b in bgs], [(3, pool[0][:180 * 320 * 3].view(180, 320, 3))])
    torch.cuda.synchronize()
    assert torch.equal(f.mg._view(3, "uint8", (total,)), masks) and torch.equal(f.mg.ofinal(), of), "a refused call changed the state"
    for p in pool:
        assert bool((p == 0x5a).all()), "a refused call wrote an output"
    f.compare_state(f.t)
    # and the context goes on as if nothing had been asked
    f.tick([2, 4, 0], [(s, z) for s in (0, 4) for z in SIM[1:]])
