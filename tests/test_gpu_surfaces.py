"""bsx_step_batch_surfaces and bsx_nv12_to_bgr on the GPU: NV12 decoder surfaces in, NV12 encoder surfaces out.

The yardsticks are the definition in include/bsx.h and the call's twin.  bsx_nv12_to_bgr is compared with the oracle's YUYV -> BGR of the 4:2:2 image Q built on the
host from the two planes.  The step is compared with a second context of the same classes that is fed bsx_nv12_to_bgr of the same surfaces through
step_vcam_geoms_outs_nv12 — existing code: planes, every stream's persistent mask and `ofinal` must be equal, byte for byte, after every tick.

The fleet is tests/test_gpu_vcam_nv12.py's: segm_lite with VGA, 1280x720 and 640x360, two streams each, the same CYCLE of settings.  Input surfaces are made of the
synthetic frames by bgr_to_nv12 and laid out with pitch_y != pitch_uv, both above the width (tight for 640x360); every surface, in or out, is ONE allocation — a band,
the Y plane, the UV plane, a band — whose padding holds a sentinel."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD, FHD, NHD = (640, 480), (1280, 720), (1920, 1080), (640, 360)
LITE = [VGA, HD, NHD]
IN_PITCH = {VGA: (768, 704), HD: (1408, 1344), NHD: (640, 640), FHD: (1920, 2048)}      # (pitch_y, pitch_uv) of a class's input surfaces
# output records as in tests/test_gpu_vcam_nv12.py: 1280x720 -> 160x90 is the per-tap form, 1280x720 -> 640x360 the staged form at its LDS limit, 640x360 a class's
# own size and an exact 2x of 1280x720; 318x178 ends its rows with a 2-pixel group; 64x2 is one row pair; 1280x720 is an up-scale of 640x360 (taps clamped at W - 1,
# the last chroma row)
PITCH = {(640, 360): 640, (320, 180): 320, (160, 90): 256, (318, 178): 320, (64, 2): 64, (1280, 720): 1280}
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
    """one allocation laid out as a surface: BAND bytes, [h] rows of pitch_y, [h / 2] rows of pitch_uv, BAND bytes — all of it `fill`"""

    def __init__(self, w, h, pitch_y=None, pitch_uv=None, n=1, fill=SENTINEL):
        self.w, self.h, self.n, self.fill = w, h, n, fill
        self.pitch_y, self.pitch_uv = pitch_y or w, pitch_uv or pitch_y or w
        ybytes, uvbytes = self.pitch_y * h * n, self.pitch_uv * (h // 2) * n
        self.buf = torch.full((2 * BAND + ybytes + uvbytes,), fill, dtype=torch.uint8, device="cuda")
        self.y = torch.as_strided(self.buf, (n, h, w), (self.pitch_y * h, self.pitch_y, 1), BAND)
        self.uv = torch.as_strided(self.buf, (n, h // 2, w), (self.pitch_uv * (h // 2), self.pitch_uv, 1), BAND + ybytes)
        assert self.y.data_ptr() % 4 == 0 and self.uv.data_ptr() % 4 == 0

    def planes(self):
        return self.y[0], self.uv[0]

    def untouched_outside(self):
        """the bands and bytes [w, pitch) of every row still hold the fill"""
        rest = self.buf.clone()
        torch.as_strided(rest, self.y.shape, self.y.stride(), BAND).fill_(self.fill)
        torch.as_strided(rest, self.uv.shape, self.uv.stride(), BAND + self.pitch_y * self.h * self.n).fill_(self.fill)
        return bool((rest == self.fill).all())


class Fleet:
    """two contexts of the same classes: `mg` takes the new call, `twin` step_vcam_geoms_outs_nv12 with the BGR frames nv12_to_bgr makes of the same surfaces"""

    def __init__(self, bs, key, sizes, per_class=2, **kw):
        self.bs, self.path = bs, model_path(key)
        self.geoms = [(W, H, per_class) for W, H in sizes]
        self.n = per_class * len(sizes)
        self.mg = bs.MaskGen.with_geometries(self.path, self.geoms, **kw)
        self.twin = bs.MaskGen.with_geometries(self.path, self.geoms, **kw)
        self.first = [g["first_stream"] for g in self.mg.geometries()]
        self.t = 0
        self.seen = set()                # the settings of every position that had a record

    def size(self, s):
        g = max(i for i, f in enumerate(self.first) if f <= s)
        return self.geoms[g][0], self.geoms[g][1], g

    def surface(self, s, t, garbage=SENTINEL):
        """stream s at tick t as a decoder leaves it: bgr_to_nv12 of the synthetic frame in rows of the class's pitches, `garbage` in the padding and the bands"""
        W, H, _g = self.size(s)
        y, uv = self.twin.bgr_to_nv12(_frame(W, H, s, t)[None])
        sf = Surface(W, H, *IN_PITCH[(W, H)], fill=garbage)
        sf.y.copy_(y)
        sf.uv.copy_(uv)
        return sf

    def setting(self, s, t):
        W, H, g = self.size(s)
        bg, fl = CYCLE[(s + t) % len(CYCLE)]
        img = None if bg is None else _image(W, H, 100 + s if bg == "own" else 7 + g)
        return self.bs.StreamSetting(bg=img, **fl)

    def outs(self, ids, records):
        surf = [Surface(ow, oh, PITCH[(ow, oh)]) for _s, (ow, oh) in records]
        return surf, [(ids.index(s),) + sf.planes() for (s, _z), sf in zip(records, surf)]

    def tick(self, ids, records, tag="", garbage=(SENTINEL, SENTINEL), both_surfaces=False):
        """one call: positions `ids`, records (stream, (out_w, out_h)) in the caller's order.  both_surfaces: the twin takes the new call as well (with its own
        garbage in the padding).  Returns the surfaces the new call wrote, in record order."""
        t = self.t
        self.t += 1
        sett = [self.setting(s, t) for s in ids]
        ins = [self.surface(s, t, garbage[0]) for s in ids]
        surf, recs = self.outs(ids, records)
        self.mg.step_surfaces(ids, [sf.planes() for sf in ins], sett, recs)
        want, wrecs = self.outs(ids, records)
        if both_surfaces:
            ins2 = [self.surface(s, t, garbage[1]) for s in ids]
            self.twin.step_surfaces(ids, [sf.planes() for sf in ins2], sett, wrecs)
        else:
            frames = [self.twin.nv12_to_bgr(sf.y, sf.uv)[0] for sf in ins]
            self.twin.step_vcam_geoms_outs_nv12(ids, frames, sett, wrecs)
        for (s, (ow, oh)), sf, exp in zip(records, surf, want):
            W, H, _g = self.size(s)
            self.seen.add(CYCLE[(s + t) % len(CYCLE)][0:1] + tuple(sorted(CYCLE[(s + t) % len(CYCLE)][1])))
            what = "%st=%d stream %d (%dx%d -> %dx%d, pitch %d, %s)" % (tag, t, s, W, H, ow, oh, sf.pitch_y, CYCLE[(s + t) % len(CYCLE)])
            assert sf.untouched_outside(), what + ": a byte outside [0, out_w) of the rows of the surface was written"
            for name, got, e in zip(("Y", "UV"), sf.planes(), exp.planes()):
                bad = got != e
                assert not bool(bad.any()), "%s: %d %s bytes differ, first at (row, byte) = %s" % (what, int(bad.sum()), name, tuple(int(v) for v in bad.nonzero()[0]))
        for sf in ins:
            assert sf.untouched_outside(), "an input surface was written"
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


# ---- 1. the stand-alone conversion against the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,pitch_y,pitch_uv,n", [(8, 2, 8, 8, 1), (6, 4, 8, 12, 2), (640, 480, 768, 704, 3)], ids=["one_block_row", "tail_bytes", "vga_padded"])
def test_nv12_to_bgr_is_yuyv_to_bgr_of_the_422_image(lite, w, h, pitch_y, pitch_uv, n):
    from backscrub_amd import api
    from oracle import oracle_py
    rng = np.random.default_rng(w * 1000 + h)
    hy, huv = rng.integers(0, 256, (n, h, w), dtype=np.uint8), rng.integers(0, 256, (n, h // 2, w), dtype=np.uint8)
    hy[0, 0, :4], huv[0, 0, :4] = [0, 15, 16, 255], [0, 255, 255, 0]                      # the clamps of both ends
    # Q[y][c] = (Y[y][2c], UV[y / 2][2c], Y[y][2c + 1], UV[y / 2][2c + 1])
    q = np.empty((n, h, w // 2, 4), np.uint8)
    rep = np.repeat(huv, 2, axis=1)
    q[..., 0], q[..., 1], q[..., 2], q[..., 3] = hy[..., 0::2], rep[..., 0::2], hy[..., 1::2], rep[..., 1::2]
    q = q.reshape(n, h, w, 2)
    want = torch.from_numpy(np.stack([oracle_py.yuyv_to_bgr(q[i]) for i in range(n)])).cuda()
    sf = Surface(w, h, pitch_y, pitch_uv, n=n, fill=0x3c)
    sf.y.copy_(torch.from_numpy(hy).cuda())
    sf.uv.copy_(torch.from_numpy(huv).cuda())
    got = lite.mg.nv12_to_bgr(sf.y, sf.uv, w, h)
    assert got.shape == (n, h, w, 3) and torch.equal(got, want)
    assert torch.equal(lite.mg.nv12_to_bgr(sf.y[0], sf.uv[0]), want[0])                     # one surface, two-dimensional views
    assert torch.equal(lite.mg.yuyv_to_bgr(torch.from_numpy(q).cuda()), want)               # ... and the device's own YUYV route gives the same bytes
    assert sf.untouched_outside()
    # a destination that is not 4-byte aligned takes the byte route; what lies around it stays
    raw = torch.full((want.numel() + 16,), 0x77, dtype=torch.uint8, device="cuda")
    o = (-raw.data_ptr()) % 4 + 5
    P = ctypes.c_void_p
    rc = api.lib().bsx_nv12_to_bgr(lite.mg.h, P(sf.y.data_ptr()), pitch_y, P(sf.uv.data_ptr()), pitch_uv, w, h, n, P(raw.data_ptr() + o), None)
    assert rc == 0, api.lib().bsx_last_error(lite.mg.h)
    torch.cuda.synchronize()
    assert torch.equal(raw[o:o + want.numel()].view(want.shape), want)
    assert bool((raw[:o] == 0x77).all()) and bool((raw[o + want.numel():] == 0x77).all())
    # the padding means nothing
    sf2 = Surface(w, h, pitch_y, pitch_uv, n=n, fill=0xC3)
    sf2.y.copy_(sf.y)
    sf2.uv.copy_(sf.uv)
    assert torch.equal(lite.mg.nv12_to_bgr(sf2.y, sf2.uv), want)


def test_nv12_to_bgr_refusals(lite):
    from backscrub_amd import api
    L, P, h = api.lib(), ctypes.c_void_p, lite.mg.h
    out = torch.full((2, 4, 8, 3), 0x11, dtype=torch.uint8, device="cuda")
    sf = Surface(8, 4, 8, 8, n=2)
    b, y, uv = out.data_ptr(), sf.y.data_ptr(), sf.uv.data_ptr()
    for args, words in [((None, 8, P(uv), 8, 8, 4, 2, P(b)), "is NULL"), ((P(y), 8, None, 8, 8, 4, 2, P(b)), "is NULL"), ((P(y), 8, P(uv), 8, 8, 4, 2, None), "is NULL"),
                        ((P(y), 8, P(uv), 8, 0, 4, 2, P(b)), "w = 0"), ((P(y), 8, P(uv), 8, 8, -2, 2, P(b)), "h = -2"), ((P(y), 8, P(uv), 8, 8, 4, 0, P(b)), "n = 0"),
                        ((P(y), 8, P(uv), 8, 7, 4, 2, P(b)), "even width and height (7 x 4)"), ((P(y), 8, P(uv), 8, 8, 3, 2, P(b)), "even width and height (8 x 3)"),
                        ((P(y), 4, P(uv), 8, 8, 4, 2, P(b)), "pitch_y = 4"), ((P(y), 10, P(uv), 8, 8, 4, 2, P(b)), "pitch_y = 10"),
                        ((P(y), 8, P(uv), 6, 8, 4, 2, P(b)), "pitch_uv = 6"), ((P(y + 2), 8, P(uv), 8, 8, 4, 2, P(b)), "d_y 0x%x is not 4-byte aligned" % (y + 2)),
                        ((P(y), 8, P(uv + 1), 8, 8, 4, 2, P(b)), "d_uv 0x%x is not 4-byte aligned" % (uv + 1))]:
        rc = L.bsx_nv12_to_bgr(h, *args, None)
        text = (L.bsx_last_error(h) or b"").decode(errors="replace")
        assert rc == BSX_EINVAL and words in text and "bsx_nv12_to_bgr" in text, (args, rc, text)
    torch.cuda.synchronize()
    assert bool((out == 0x11).all()), "a refused call wrote the image"


# ---- 2. the step against its twin, three ticks over changing subsets; 6. every setting of the CYCLE is reached ------------------------------------------------------
@pytest.mark.parametrize("sizes", [SIM + [(64, 2)], [(318, 178), (160, 90), (64, 2)]], ids=["simulcast", "tail"])
def test_surfaces_in_surfaces_out(lite, sizes):
    lite.seen.clear()
    for k, ids in enumerate(lite.subsets(3, len(sizes))):
        rng = np.random.default_rng(k)
        recs = [(s, z) for s in ids for z in sizes]
        nhd = [s for s in ids if lite.size(s)[:2] == NHD]
        assert k > 0 or nhd
        if len(sizes) == 3 and nhd:                # the fourth size of the call: one 640x360 stream up-scaled to 1280x720 (the first tick has every stream)
            recs.append((nhd[0], (1280, 720)))
        lite.tick(ids, [recs[j] for j in rng.permutation(len(recs))])
    assert lite.seen == {(bg,) + tuple(sorted(fl)) for bg, fl in CYCLE}, "the three ticks did not reach every setting of the CYCLE: %s" % sorted(lite.seen, key=str)
    assert ("own", "flip_h") in lite.seen and ("shared", "flip_v") in lite.seen and ("own", "flip_h", "flip_v") in lite.seen and (None, "filter_off") in lite.seen


# ---- 3. prep alone -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_masks_only_step_leaves_the_twins_network_input(lite):
    ids = [3, 0, 5, 1, 4, 2]
    lite.tick(ids, [])                                                 # m == 0: prep, the network, the masks
    torch.cuda.synchronize()
    a, b = lite.mg.input_u8()[:len(ids)], lite.twin.input_u8()[:len(ids)]
    bad = (a != b).any(dim=-1)
    assert not bool(bad.any()), "the network input of prep_geoms_nv12_k differs from prep_geoms_k's on the converted frames: %d pixels, first at (position, y, x) = %s" % (
        int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]))
    assert bool((a[..., :3] != 0).any())


# ---- 4. the padding means nothing ------------------------------------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_the_padding(lite):
    ids = [4, 1, 2, 5, 0, 3]
    lite.tick(ids, [(s, z) for s in ids for z in [(320, 180), (160, 90), (318, 178)]], garbage=(0x00, 0xFF), both_surfaces=True)


# ---- 5. an edge context ------------------------------------------------------------------------------------------------------------------------------------------------
def test_edge_context_with_a_1920x1080_class(bs):
    f = Fleet(bs, "lite", [VGA, FHD], edge_roi=True)
    try:
        roi = f.mg.geometries()[1]["roi"]
        assert roi[0] % 4 or roi[2] % 4, "1920x1080: ROI %s is on the 4-pixel grid, the test was written for one that is not" % (roi,)
        ids = [2, 0, 3, 1]
        f.tick(ids, [(s, z) for z in [(640, 360), (318, 178)] for s in ids])
        torch.cuda.synchronize()
        assert torch.equal(f.mg.input_u8()[:4], f.twin.input_u8()[:4])
    finally:
        f.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(lite):
    from backscrub_amd import api
    f = lite
    f.tick([5, 0, 3, 1, 4, 2], [(s, (320, 180)) for s in range(6)])
    total = sum(W * H * n for W, H, n in f.geoms)
    masks, of = f.mg._view(3, "uint8", (total,)).clone(), f.mg.ofinal().clone()
    ids = [4, 0, 2]                                                                   # 640x360, 640x480, 1280x720
    ins = [f.surface(s, 9) for s in ids]
    bgs = [_image(*f.size(s)[:2], 50) for s in ids]
    pool = [torch.full((360 * 640 * 2,), 0x5a, dtype=torch.uint8, device="cuda") for _ in range(4)]
    P = [p.data_ptr() for p in pool]
    assert all(p % 4 == 0 for p in P)

    def raw(recs, n=3, flags=0, null_items=False, item=None, use_ids=None):
        """the C entry point itself.  item: (position, {field: value}) changes one item; (return code, error text)"""
        arr = (ctypes.c_int * 3)(*(use_ids or ids))
        items = (api._SurfaceItem * 3)()
        for i in range(3):
            it = items[i]
            it.d_y, it.d_uv, it.pitch_y, it.pitch_uv = ins[i].y.data_ptr(), ins[i].uv.data_ptr(), ins[i].pitch_y, ins[i].pitch_uv
            it.setting.d_bg, it.setting.flags = bgs[i].data_ptr(), 0
        if item:
            for k, v in item[1].items():
                if k in ("d_bg", "flags"):
                    setattr(items[item[0]].setting, k, v)
                else:
                    setattr(items[item[0]], k, v)
        out = (api._VcamOutNv12 * max(len(recs), 1))()
        for j, (it_, w, h, py, puv, y, uv) in enumerate(recs):
            r = out[j]
            r.item, r.out_w, r.out_h, r.pitch_y, r.pitch_uv, r.d_y, r.d_uv = it_, w, h, py, puv, y, uv
        rc = api.lib().bsx_step_batch_surfaces(f.mg.h, arr, None if null_items else items, n, out, len(recs), None, flags)
        return rc, (api.lib().bsx_last_error(f.mg.h) or b"").decode(errors="replace")

    def rec(item, w, h, k, y=None, uv=None):
        """a surface in pool[k]: Y at its start, UV right behind"""
        return (item, w, h, w, w, P[k] if y is None else y, P[k] + w * h if uv is None else uv)
    ok = [rec(0, 320, 180, 0), rec(1, 160, 90, 1), rec(2, 320, 180, 2)]
    y1, uv1, bg2 = ins[1].y.data_ptr(), ins[1].uv.data_ptr(), bgs[2].data_ptr()
    end_y1 = y1 + 768 * 479 + 640                                                     # one past the last byte of items[1]'s Y plane that means anything
    cases = [
        (dict(null_items=True), "items is NULL"),
        (dict(item=(1, dict(d_y=None))), "items[1]: d_y is NULL"),
        (dict(item=(1, dict(d_y=y1 + 2))), "items[1]: d_y 0x%x is not 4-byte aligned" % (y1 + 2)),
        (dict(item=(2, dict(d_uv=None))), "items[2]: d_uv is NULL"),
        (dict(item=(1, dict(d_uv=uv1 + 1))), "items[1]: d_uv 0x%x is not 4-byte aligned" % (uv1 + 1)),
        (dict(item=(1, dict(pitch_y=636))), "items[1]: pitch_y = 636 is below the width 640"),
        (dict(item=(1, dict(pitch_y=770))), "items[1]: pitch_y = 770 is not a multiple of 4"),
        (dict(item=(2, dict(pitch_uv=1276))), "items[2]: pitch_uv = 1276 is below the width 1280"),
        (dict(item=(0, dict(pitch_uv=642))), "items[0]: pitch_uv = 642 is not a multiple of 4"),
        (dict(item=(0, dict(flags=64))), "items[0]: setting flags 0x40 has the yuyv-in bit"),
        (dict(item=(2, dict(flags=0x700))), "items[2]: setting flags 0x700 asks for a background blur"),
        (dict(item=(2, dict(flags=128))), "items[2]: setting flags 0x80 has bits outside flip / filter-off"),
        (dict(flags=1), "flags 0x1: this step takes no flags"),
        (dict(flags=1 << 20), "flags 0x100000"),
        (dict(item=(2, dict(d_bg=None))), "items[2]: setting.d_bg is NULL"),
        (dict(item=(2, dict(d_bg=bg2 + 1))), "items[2]: setting.d_bg 0x%x is not 4-byte aligned" % (bg2 + 1)),
        # an output plane across an input plane, a background, another output plane; an input plane ends at pitch * (rows - 1) + W
        (dict(recs=ok + [rec(1, 64, 32, 3, y=end_y1 - 4)]), "outs[3]: d_y 0x%x overlaps d_y of items[1]" % (end_y1 - 4)),
        (dict(recs=ok + [rec(1, 64, 32, 3, uv=uv1)]), "outs[3]: d_uv 0x%x overlaps d_uv of items[1]" % uv1),
        (dict(recs=ok + [rec(1, 64, 32, 3, uv=bg2 + 1280 * 720 * 3 - 4)]), "overlaps setting.d_bg of items[2]"),
        (dict(recs=ok + [rec(1, 64, 32, 3, y=P[0] + 320 * 180 - 4)]), "outs[3]: d_y 0x%x overlaps d_y of outs[0]" % (P[0] + 320 * 180 - 4)),
        # the record refusals of the NV12 output form arrive unchanged
        (dict(recs=ok + [rec(3, 64, 32, 3)]), "outs[3]: item 3 is outside [0, 3)"),
        (dict(recs=ok + [(1, 64, 32, 60, 64, P[3], P[3] + 4096)]), "outs[3]: pitch_y = 60 is below out_w = 64"),
        (dict(recs=[rec(0, 321, 180, 0)]), "outs[0]: NV12 output needs an even width and height (321 x 180)"),
        (dict(use_ids=[4, 0, 4]), "repeats"),
        (dict(use_ids=[4, 0, 6]), "out of range"),
    ]
    for kw, words in cases:
        kw = dict(kw)
        rc, text = raw(kw.pop("recs", ok), **kw)
        assert rc == BSX_EINVAL and words in text and "bsx_step_batch_surfaces" in text, (kw, rc, text)
        assert "BSX_" not in text, text
    assert raw(ok, n=0)[0] == 0                                                       # n == 0: nothing to do
    # a refused call must leave everything as it was
    torch.cuda.synchronize()
    assert torch.equal(f.mg._view(3, "uint8", (total,)), masks) and torch.equal(f.mg.ofinal(), of), "a refused call changed the state"
    for p in pool:
        assert bool((p == 0x5a).all()), "a refused call wrote a plane"
    for sf in ins:
        assert sf.untouched_outside()
    f.compare_state(f.t)
    # and the context goes on as if nothing had been asked: the results of a twin that never saw a refused call
    f.tick([2, 4, 0], [(s, z) for s in (0, 4) for z in SIM[1:]])
