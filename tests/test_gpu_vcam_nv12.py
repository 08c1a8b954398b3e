"""bsx_step_batch_vcam_geoms_outs_nv12 and bsx_bgr_to_nv12 on the GPU: every output record an NV12 surface with row pitches.

The yardstick is the definition in include/bsx.h: an NV12 output is a pure function of the YUYV output the library already produces.  A twin context of the same
classes runs step_vcam_geoms_outs(.., yuyv=True) — existing code, pinned through bsx_bgr_to_yuyv to the reference's packer — and the expected planes are computed
from its output with torch integer ops, exactly as the definition reads.  Byte equality throughout; after every tick the persistent mask and the temporal state
(`ofinal`) of ALL streams are compared with the twin's.

The fleet is tests/test_gpu_vcam_outs.py's: segm_lite with VGA, 1280x720 and 640x360, two streams each, the same CYCLE of settings.  Every surface is ONE
allocation — a band, the Y plane, the UV plane, a band — pre-filled with a sentinel: the bands and everything outside [0, out_w) of each row must survive."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD, FHD, NHD = (640, 480), (1280, 720), (1920, 1080), (640, 360)
LITE = [VGA, HD, NHD]
# (out_w, out_h): pitch.  640x360, 320x180, 160x90: the simulcast — 1280x720 -> 160x90 is the per-tap form, 1280x720 -> 640x360 the staged form at its LDS limit,
# 640x360 a class's own size and an exact 2x; 160 in rows of 256 bytes.  318x178: the 2-pixel group that ends a row of out_w % 4 == 2 and a last tile row of 18, in
# rows of 320.  64x2: one row pair.
PITCH = {(640, 360): 640, (320, 180): 320, (160, 90): 256, (318, 178): 320, (64, 2): 64}
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


class Surface:
    """one allocation laid out as a surface: BAND bytes, [h] rows of pitch_y, [h / 2] rows of pitch_uv, BAND bytes — all of it the sentinel"""

    def __init__(self, w, h, pitch_y=None, pitch_uv=None, n=1):
        self.w, self.h, self.n = w, h, n
        self.pitch_y, self.pitch_uv = pitch_y or w, pitch_uv or pitch_y or w
        ybytes, uvbytes = self.pitch_y * h * n, self.pitch_uv * (h // 2) * n
        self.buf = torch.full((2 * BAND + ybytes + uvbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.y = torch.as_strided(self.buf, (n, h, w), (self.pitch_y * h, self.pitch_y, 1), BAND)
        self.uv = torch.as_strided(self.buf, (n, h // 2, w), (self.pitch_uv * (h // 2), self.pitch_uv, 1), BAND + ybytes)
        assert self.y.data_ptr() % 4 == 0 and self.uv.data_ptr() % 4 == 0

    def planes(self):
        return self.y[0], self.uv[0]

    def untouched_outside(self):
        """the bands and bytes [w, pitch) of every row still hold the sentinel"""
        rest = self.buf.clone()
        torch.as_strided(rest, self.y.shape, self.y.stride(), BAND).fill_(SENTINEL)
        torch.as_strided(rest, self.uv.shape, self.uv.stride(), BAND + self.pitch_y * self.h * self.n).fill_(SENTINEL)
        return bool((rest == SENTINEL).all())


def nv12_of_yuyv(q):
    """the definition: q = [.., h, w, 2] YUYV bytes, i.e. [.., h, w / 2] words (Y0, Ca, Y1, Cb) -> (Y [.., h, w], UV [.., h / 2, w])"""
    h, w = int(q.shape[-3]), int(q.shape[-2])
    lead = tuple(q.shape[:-3])
    words = q.reshape(lead + (h, w // 2, 4))
    y = words[..., [0, 2]].reshape(lead + (h, w))
    c = words[..., [1, 3]].to(torch.int32).reshape(lead + (h // 2, 2, w // 2, 2))      # [.., r, row of the pair, c, (Ca, Cb)]
    uv = torch.div(c[..., 0, :, :] + c[..., 1, :, :], 2, rounding_mode="floor").to(torch.uint8).reshape(lead + (h // 2, w))
    return y, uv


class Fleet:
    """two contexts of the same classes: `mg` takes the new call, `twin` step_vcam_geoms_outs with YUYV out"""

    def __init__(self, bs, key, sizes, per_class=2, **kw):
        self.bs, self.path = bs, model_path(key)
        self.geoms = [(W, H, per_class) for W, H in sizes]
        self.n = per_class * len(sizes)
        self.mg = bs.MaskGen.with_geometries(self.path, self.geoms, **kw)
        self.twin = bs.MaskGen.with_geometries(self.path, self.geoms, **kw)
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

    def tick(self, ids, records, tag=""):
        """one call: positions `ids`, records (stream, (out_w, out_h)) in the caller's order.  Returns the surfaces in record order."""
        t = self.t
        self.t += 1
        frames = [self.frame(s, t) for s in ids]
        sett = [self.setting(s, t) for s in ids]
        surf = [Surface(ow, oh, PITCH[(ow, oh)]) for _s, (ow, oh) in records]
        self.mg.step_vcam_geoms_outs_nv12(ids, frames, sett, [(ids.index(s),) + sf.planes() for (s, _z), sf in zip(records, surf)])
        keys = sorted({(s, z) for s, z in records})
        tight = [torch.full((oh, ow, 2), 0x5a, dtype=torch.uint8, device="cuda") for _s, (ow, oh) in keys]
        self.twin.step_vcam_geoms_outs(ids, frames, sett, [(ids.index(s), o) for (s, _z), o in zip(keys, tight)], yuyv=True)
        want = {k: nv12_of_yuyv(o) for k, o in zip(keys, tight)}
        for (s, (ow, oh)), sf in zip(records, surf):
            W, H, _g = self.size(s)
            what = "%st=%d stream %d (%dx%d -> %dx%d, pitch %d, %s)" % (tag, t, s, W, H, ow, oh, sf.pitch_y, CYCLE[(s + t) % len(CYCLE)])
            assert sf.untouched_outside(), what + ": a byte outside [0, out_w) of the rows of the surface was written"
            for name, got, exp in zip(("Y", "UV"), sf.planes(), want[(s, (ow, oh))]):
                bad = got != exp
                assert not bool(bad.any()), "%s: %d %s bytes differ, first at (row, byte) = %s" % (what, int(bad.sum()), name, tuple(int(v) for v in bad.nonzero()[0]))
        self.compare_state(t, tag)
        return surf

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


# ---- 1. three ticks over changing subsets --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [SIM + [(64, 2)], [(318, 178), (160, 90), (64, 2)]], ids=["simulcast", "tail"])
def test_layers_for_an_encoder(lite, sizes):
    for k, ids in enumerate(lite.subsets(3, len(sizes))):
        rng = np.random.default_rng(k)
        recs = [(s, z) for s in ids for z in sizes]
        lite.tick(ids, [recs[j] for j in rng.permutation(len(recs))])


# ---- 2. YUYV and BGR items in one call: vg_outs_nv12_fmt_k ------------------------------------------------------------------------------------------------------------
def test_two_streams_deliver_yuyv_frames(bs):
    """320x240, 640x360 and VGA (the classes tests/test_gpu_geoms_yuyv_in.py knows to have the fused YUYV prep), two streams YUYV"""
    f = Fleet(bs, "lite", [(320, 240), NHD, VGA])
    f.yin = {1, 4}
    try:
        ids = [4, 0, 3, 1, 5, 2]
        f.tick(ids, [(s, z) for z in [(318, 178), (160, 90), (640, 360)] for s in ids])
    finally:
        f.close()


# ---- 3. an edge context -----------------------------------------------------------------------------------------------------------------------------------------------
def test_edge_context_with_a_1920x1080_class(bs):
    f = Fleet(bs, "lite", [VGA, FHD], edge_roi=True)
    try:
        roi = f.mg.geometries()[1]["roi"]
        assert roi[0] % 4 or roi[2] % 4, "1920x1080: ROI %s is on the 4-pixel grid, the test was written for one that is not" % (roi,)
        ids = [2, 0, 3, 1]
        f.tick(ids, [(s, z) for z in [(640, 360), (318, 178)] for s in ids])
    finally:
        f.close()


# ---- 4. multiplicity --------------------------------------------------------------------------------------------------------------------------------------------------
def test_an_item_without_a_record_advances_and_two_records_of_one_size_are_equal(lite):
    ids = [3, 0, 5, 1]
    surf = lite.tick(ids, [(0, (640, 360)), (3, (320, 180)), (0, (160, 90)), (0, (640, 360)), (0, (320, 180))])      # 5 and 1: no record (compare_state covers them)
    a, b = surf[0], surf[3]
    assert a.y.data_ptr() != b.y.data_ptr() and torch.equal(a.y, b.y) and torch.equal(a.uv, b.uv)
    lite.tick([2, 4], [])                                                                                           # m == 0: a masks-only step


# ---- 5. the stand-alone conversion --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,pitch_y,pitch_uv", [(64, 2, 64, 64), (64, 2, 128, 68), (318, 178, 320, 320), (318, 178, 384, 512), (640, 360, 640, 640),
                                                  (640, 360, 1024, 768)])
def test_bgr_to_nv12_is_the_definition_applied_to_bgr_to_yuyv(lite, w, h, pitch_y, pitch_uv):
    from backscrub_amd import api
    n = 3
    bgr = torch.stack([_frame(1280, 720, s, 1)[40:40 + h, 100 * s:100 * s + w] for s in range(n)]).contiguous()
    sf = Surface(w, h, pitch_y, pitch_uv, n=n)
    P = ctypes.c_void_p
    rc = api.lib().bsx_bgr_to_nv12(lite.mg.h, P(bgr.data_ptr()), w, h, n, P(sf.y.data_ptr()), pitch_y, P(sf.uv.data_ptr()), pitch_uv, None)
    assert rc == 0, api.lib().bsx_last_error(lite.mg.h)
    y, uv = nv12_of_yuyv(lite.twin.bgr_to_yuyv(bgr))
    assert torch.equal(sf.y, y) and torch.equal(sf.uv, uv)
    assert sf.untouched_outside(), "bsx_bgr_to_nv12 wrote outside [0, w) of a row"
    # the binding: planes of its own, the same bytes; a source that is not 4-byte aligned takes the byte form
    by, buv = lite.mg.bgr_to_nv12(bgr, pitch_y, pitch_uv)
    assert by.stride() == (pitch_y * h, pitch_y, 1) and buv.stride() == (pitch_uv * (h // 2), pitch_uv, 1) and torch.equal(by, y) and torch.equal(buv, uv)
    odd = torch.empty((bgr.numel() + 8,), dtype=torch.uint8, device="cuda")
    shifted = odd[(-odd.data_ptr()) % 4 + 1:][:bgr.numel()].view(bgr.shape)
    shifted.copy_(bgr)
    sy, suv = lite.mg.bgr_to_nv12(shifted)
    assert torch.equal(sy, y) and torch.equal(suv, uv)


def test_bgr_to_nv12_refusals(lite):
    from backscrub_amd import api
    L, P, h = api.lib(), ctypes.c_void_p, lite.mg.h
    bgr = torch.zeros((2, 4, 8, 3), dtype=torch.uint8, device="cuda")
    sf = Surface(8, 4, 8, 8, n=2)
    b, y, uv = bgr.data_ptr(), sf.y.data_ptr(), sf.uv.data_ptr()
    for args, words in [((None, 8, 4, 2, P(y), 8, P(uv), 8), "is NULL"), ((P(b), 8, 4, 2, None, 8, P(uv), 8), "is NULL"), ((P(b), 8, 4, 2, P(y), 8, None, 8), "is NULL"),
                        ((P(b), 0, 4, 2, P(y), 8, P(uv), 8), "w = 0"), ((P(b), 8, 4, 0, P(y), 8, P(uv), 8), "n = 0"),
                        ((P(b), 7, 4, 2, P(y), 8, P(uv), 8), "even width and height (7 x 4)"), ((P(b), 8, 3, 2, P(y), 8, P(uv), 8), "even width and height (8 x 3)"),
                        ((P(b), 8, 4, 2, P(y), 4, P(uv), 8), "pitch_y = 4"), ((P(b), 8, 4, 2, P(y), 10, P(uv), 8), "pitch_y = 10"),
                        ((P(b), 8, 4, 2, P(y), 8, P(uv), 6), "pitch_uv = 6"), ((P(b), 8, 4, 2, P(y + 2), 8, P(uv), 8), "d_y 0x%x is not 4-byte aligned" % (y + 2)),
                        ((P(b), 8, 4, 2, P(y), 8, P(uv + 1), 8), "d_uv 0x%x is not 4-byte aligned" % (uv + 1))]:
        rc = L.bsx_bgr_to_nv12(h, *args, None)
        text = (L.bsx_last_error(h) or b"").decode(errors="replace")
        assert rc == BSX_EINVAL and words in text, (args, rc, text)
    torch.cuda.synchronize()
    assert bool((sf.buf == SENTINEL).all()), "a refused call wrote a plane"


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(lite):
    from backscrub_amd import api
    f = lite
    f.tick([5, 0, 3, 1, 4, 2], [(s, (320, 180)) for s in range(6)])
    total = sum(W * H * n for W, H, n in f.geoms)
    masks, of = f.mg._view(3, "uint8", (total,)).clone(), f.mg.ofinal().clone()
    ids = [4, 0, 2]
    frames = [_frame(*f.size(s)[:2], s, 9) for s in ids]
    bgs = [_image(*f.size(s)[:2], 50) for s in ids]
    pool = [torch.full((360 * 640 * 2,), 0x5a, dtype=torch.uint8, device="cuda") for _ in range(7)]

    def raw(recs, n=3, m=None, flags=0, null_outs=False, item_flags=(0, 0, 0), frame_ptrs=None):
        """the C entry point itself: records (item, out_w, out_h, pitch_y, pitch_uv, d_y, d_uv); (return code, error text)"""
        arr = (ctypes.c_int * 3)(*ids)
        items = (api._GeomItem * 3)()
        for i in range(3):
            items[i].d_frame = frame_ptrs[i] if frame_ptrs else frames[i].data_ptr()
            items[i].d_out = None
            items[i].setting.d_bg, items[i].setting.flags = bgs[i].data_ptr(), item_flags[i]
        out = (api._VcamOutNv12 * max(len(recs), 1))()
        for j, (item, w, h, py, puv, y, uv) in enumerate(recs):
            r = out[j]
            r.item, r.out_w, r.out_h, r.pitch_y, r.pitch_uv, r.d_y, r.d_uv = item, w, h, py, puv, y, uv
        rc = api.lib().bsx_step_batch_vcam_geoms_outs_nv12(f.mg.h, arr, items, n, None if null_outs else out, len(recs) if m is None else m, None, flags)
        return rc, (api.lib().bsx_last_error(f.mg.h) or b"").decode(errors="replace")
    P = [p.data_ptr() for p in pool]
    assert all(p % 4 == 0 for p in P)

    def rec(item, w, h, k, py=None, puv=None, y=None, uv=None):
        """a surface in pool[k]: Y at its start, UV right behind"""
        py, puv = py or w, puv or w
        return (item, w, h, py, puv, P[k] if y is None else y, P[k] + py * h if uv is None else uv)
    ok = [rec(0, 320, 180, 0), rec(1, 160, 90, 1, 256, 256), rec(2, 320, 180, 2)]
    end0 = P[0] + 320 * 180 + 320 * 90                                                # one past the last byte of outs[0]'s UV plane
    cases = [
        (dict(recs=ok, null_outs=True), "outs is NULL with m = 3"),
        (dict(recs=ok, m=-1), "m = -1 is negative"),
        (dict(recs=ok + [rec(3, 64, 32, 3)]), "outs[3]: item 3 is outside [0, 3)"),
        (dict(recs=ok + [rec(-1, 64, 32, 3)]), "outs[3]: item -1 is outside [0, 3)"),
        (dict(recs=ok + [rec(0, 64, 32, 3), rec(0, 64, 32, 4), rec(0, 64, 32, 5), rec(0, 64, 32, 6)]), "outs[6]: record 5 of items[0]"),
        (dict(recs=ok + [rec(0, 64, 32, 3), rec(1, 66, 34, 4, 68, 68), rec(2, 68, 36, 5)]), "outs[5]: 68 x 36 is distinct output size 5"),
        (dict(recs=ok + [rec(1, 0, 32, 3, 64, 64)]), "outs[3]: output size 0 x 32 must be positive"),
        (dict(recs=ok + [rec(1, 64, -2, 3)]), "outs[3]: output size 64 x -2 must be positive"),
        (dict(recs=[rec(0, 321, 180, 0, 324, 324)]), "outs[0]: NV12 output needs an even width and height (321 x 180)"),
        (dict(recs=ok + [rec(1, 64, 31, 3)]), "outs[3]: NV12 output needs an even width and height (64 x 31)"),
        (dict(recs=ok + [rec(1, 64, 32, 3, 60, 64)]), "outs[3]: pitch_y = 60 is below out_w = 64"),
        (dict(recs=ok + [rec(1, 64, 32, 3, 64, 32)]), "outs[3]: pitch_uv = 32 is below out_w = 64"),
        (dict(recs=ok + [rec(1, 6, 4, 3, 6, 8)]), "outs[3]: pitch_y = 6 is not a multiple of 4"),
        (dict(recs=ok + [rec(1, 64, 32, 3, 64, 70)]), "outs[3]: pitch_uv = 70 is not a multiple of 4"),
        (dict(recs=ok + [rec(1, 64, 32, 3, y=0)]), "outs[3]: d_y is NULL"),
        (dict(recs=ok + [rec(1, 64, 32, 3, uv=0)]), "outs[3]: d_uv is NULL"),
        (dict(recs=ok + [rec(1, 64, 32, 3, y=P[3] + 2)]), "outs[3]: d_y 0x%x is not 4-byte aligned" % (P[3] + 2)),
        (dict(recs=ok + [rec(1, 64, 32, 3, uv=P[3] + 64 * 32 + 1)]), "outs[3]: d_uv 0x%x is not 4-byte aligned" % (P[3] + 64 * 32 + 1)),
        # overlaps: another record's plane, the record's own second plane, a frame, a background; two records that interleave their rows inside one canvas
        (dict(recs=ok + [rec(1, 64, 32, 3, y=end0 - 4)]), "outs[3]: d_y 0x%x overlaps d_uv of outs[0]" % (end0 - 4)),
        (dict(recs=ok + [rec(1, 64, 32, 3, uv=P[0] + 320 * 180 - 4)]), "outs[3]: d_uv 0x%x overlaps d_y of outs[0]" % (P[0] + 320 * 180 - 4)),
        (dict(recs=ok + [rec(1, 64, 32, 3, uv=P[3] + 64 * 32 - 4)]), "outs[3]: d_uv 0x%x overlaps d_y of outs[3]" % (P[3] + 64 * 32 - 4)),
        (dict(recs=ok + [rec(1, 64, 32, 3, y=frames[2].data_ptr() + 1280 * 720 * 3 - 4)]), "overlaps a frame or background of items[2]"),
        (dict(recs=ok + [rec(1, 64, 32, 3, uv=bgs[0].data_ptr())]), "overlaps a frame or background of items[0]"),
        (dict(recs=ok + [rec(1, 64, 32, 3, 128, 128, P[3], P[4]), rec(2, 64, 32, 5, 128, 128, P[3] + 64, P[5])]), "outs[4]: d_y 0x%x overlaps d_y of outs[3]" % (P[3] + 64)),
        # a YUYV item's frame is W * H * 2 bytes: a plane across its last bytes overlaps it
        (dict(recs=ok + [rec(1, 64, 32, 3, y=frames[1].data_ptr() + 640 * 480 * 2 - 4)], item_flags=(0, 64, 0)), "overlaps a frame or background of items[1]"),
        (dict(recs=ok, flags=1), "flags 0x1: this step takes no flags"),
        (dict(recs=ok, flags=8), "flags 0x8"),
        (dict(recs=ok, flags=1 << 20), "flags 0x100000"),
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
        f.mg.step_vcam_geoms_outs_nv12(ids, frames, [f.bs.StreamSetting(bg=b) for b in bgs], [(3, pool[0][:180 * 320].view(180, 320), pool[1][:90 * 320].view(90, 320))])
    torch.cuda.synchronize()
    assert torch.equal(f.mg._view(3, "uint8", (total,)), masks) and torch.equal(f.mg.ofinal(), of), "a refused call changed the state"
    for p in pool:
        assert bool((p == 0x5a).all()), "a refused call wrote a plane"
    f.compare_state(f.t)
    # and the context goes on as if nothing had been asked: the results of a fleet (the twin) that never saw a refused call
    f.tick([2, 4, 0], [(s, z) for s in (0, 4) for z in SIM[1:]])
