"""bsx_gaussian_blur_surfaces_batch on the GPU: n NV12 decoder surfaces, each of its own size, pitches and blur size, blurred into BGR images in one launch.
Byte equality everywhere.  Expected values come from the CPU oracle alone: the 4:2:2 image Q[y][c] = (Y[y][2c], UV[y / 2][2c], Y[y][2c + 1], UV[y / 2][2c + 1]) is
built in numpy, converted with cv::COLOR_YUV2BGR_YUYV's integers and blurred with cv::GaussianBlur's.  The call is also compared with bsx_nv12_to_bgr followed by
bsx_gaussian_blur_bgr of each surface alone, and — as the background of bsx_step_batch_surfaces — with a twin context that converts, blurs with
bsx_gaussian_blur_bgr_batch and steps the BGR frames through bsx_step_batch_vcam_geoms_outs_nv12.

Every surface, and every destination, lies in a larger buffer filled with a pattern; what surrounds the pixels is checked after the calls."""
import ctypes

import numpy as np
import pytest

from conftest import model_path, synthetic_model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KID_RING = 4                    # bsx_ctx::kIdRing (csrc/bsx_api.hip): entries of the descriptor staging ring
PAD, FILL = 64, 0xA5            # bytes around every destination and every plane, and what they (and a destination before the call) hold
# (w, h, ksize, pitch_y, pitch_uv, surface key, destination offset in its buffer): interleaved in the caller's order — not by size.  8 distinct sizes.
ITEMS = [
    (640, 480, 25, 768, 704, "vga", PAD),      # word staging, interior and border tiles, two different pitches
    (66, 18, 5, 68, 72, "s66", PAD),           # w % 4 == 2: byte stores, a partial second tile
    (64, 16, 5, 64, 64, "t1", PAD),            # exactly one tile, pitch == w
    (20, 12, 25, 32, 20, "small", PAD),        # smaller than the radius: multiple reflections, the chroma row of the reflected row
    (2, 2, 3, 4, 4, "s2", PAD),                # the smallest surface
    (40, 30, 1, 64, 40, "s40", PAD),           # the conversion alone
    (130, 70, 31, 256, 132, "k31", PAD),       # the largest tap count
    (322, 242, 3, 324, 384, "odd", PAD),       # w % 4 == 2 at size
    (640, 480, 9, 768, 704, "vga", PAD + 1),   # the first item's surface again, another blur size, the same size class; a destination at an odd byte offset
]


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


@pytest.fixture(scope="module")
def mg(bs):
    m = bs.MaskGen(synthetic_model_path("lite"), 640, 480, n_streams=16)
    yield m
    m.close()


class Surface:
    """one allocation laid out as a surface: PAD bytes, [h] rows of pitch_y, [h / 2] rows of pitch_uv, PAD bytes — all of it `fill`, then the planes' pixels"""

    def __init__(self, w, h, pitch_y, pitch_uv, hy=None, huv=None, fill=FILL):
        self.w, self.h, self.pitch_y, self.pitch_uv = w, h, pitch_y, pitch_uv
        ybytes, uvbytes = pitch_y * h, pitch_uv * (h // 2)
        self.buf = torch.full((2 * PAD + ybytes + uvbytes,), fill, dtype=torch.uint8, device="cuda")
        self.y = torch.as_strided(self.buf, (h, w), (pitch_y, 1), PAD)
        self.uv = torch.as_strided(self.buf, (h // 2, w), (pitch_uv, 1), PAD + ybytes)
        assert self.y.data_ptr() % 4 == 0 and self.uv.data_ptr() % 4 == 0
        if hy is not None:
            self.y.copy_(torch.from_numpy(hy).cuda())
            self.uv.copy_(torch.from_numpy(huv).cuda())
        self.before = self.buf.clone()

    def planes(self):
        return self.y, self.uv

    def unchanged(self):
        return torch.equal(self.buf, self.before)


def _planes(key, w, h):
    """host planes of a surface: seeded noise (any bytes are a valid surface); the first surface has its top third white and both clamps of the conversion"""
    from backscrub_amd import synth
    seed = 700 + sum(map(ord, key))
    hy, huv = synth.random_u8((h, w), seed), synth.random_u8((h // 2, w), seed + 1)
    if key == "vga":
        hy[: h // 3] = 235
        huv[: h // 6] = 128
        hy[h - 1, :4], huv[h // 2 - 1, :4] = [0, 15, 16, 255], [0, 255, 255, 0]
    return hy, huv


def _bgr_of(oracle, hy, huv):
    """the surface's BGR frame by the definition: the oracle's YUYV -> BGR of Q"""
    h, w = hy.shape
    rep = np.repeat(huv, 2, axis=0)
    q = np.empty((h, w // 2, 4), np.uint8)
    q[..., 0], q[..., 1], q[..., 2], q[..., 3] = hy[:, 0::2], rep[:, 0::2], hy[:, 1::2], rep[:, 1::2]
    return oracle.yuyv_to_bgr(q.reshape(h, w, 2))


@pytest.fixture(scope="module")
def case(oracle):
    """the item list: host planes, device surfaces, and the oracle's outputs — computed once, never written"""
    host, dev, want = {}, {}, []
    for w, h, k, py, puv, key, _off in ITEMS:
        if key not in host:
            host[key] = _planes(key, w, h)
            dev[key] = Surface(w, h, py, puv, *host[key])
        want.append(oracle.gaussian_blur(_bgr_of(oracle, *host[key]), k))
    return host, dev, want


def _dst(w, h, off=PAD):
    """a destination inside a larger pattern-filled buffer: (buffer, the [h,w,3] view at byte `off`)"""
    buf = torch.full((off + w * h * 3 + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[off:off + w * h * 3].view(h, w, 3)


def _untouched_around(buf, w, h, off=PAD):
    return bool((buf[:off] == FILL).all()) and bool((buf[off + w * h * 3:] == FILL).all())


def _call(mg, surfaces, items=ITEMS):
    bufs = [_dst(w, h, off) for w, h, *_r, off in items]
    out = mg.gaussian_blur_surfaces([surfaces[key].planes() for *_r, key, _off in items], [k for _w, _h, k, *_r in items], out=[d for _b, d in bufs])
    return bufs, out


def test_against_the_oracle(mg, case):
    assert len({(w, h) for w, h, *_r in ITEMS}) == 8                        # as many distinct sizes as one call takes
    _host, dev, want = case
    bufs, out = _call(mg, dev)
    torch.cuda.synchronize()
    for i, ((w, h, k, py, puv, key, off), (buf, dst), exp) in enumerate(zip(ITEMS, bufs, want)):
        got = out[i].cpu().numpy()
        assert out[i].data_ptr() == dst.data_ptr()
        bad = (got != exp).any(axis=2)
        assert not bad.any(), "items[%d] %dx%d ksize %d pitches %d / %d: %d pixels differ, first at (y, x) = %s" % (
            i, w, h, k, py, puv, bad.sum(), tuple(int(v) for v in np.argwhere(bad)[0]))
        assert _untouched_around(buf, w, h, off), "items[%d] %dx%d: bytes around the destination were written" % (i, w, h)
    assert all(sf.unchanged() for sf in dev.values()), "a surface, its padding or its guard bytes were written"


def test_same_as_the_two_single_calls(mg, case):
    _host, dev, _want = case
    _bufs, out = _call(mg, dev)
    for i, (w, h, k, _py, _puv, key, _off) in enumerate(ITEMS):
        bgr = mg.nv12_to_bgr(*dev[key].planes())
        single = mg.gaussian_blur(bgr[None], k)[0]
        assert torch.equal(out[i], single), "items[%d] %dx%d ksize %d" % (i, w, h, k)


def test_new_outputs_and_one_ksize_for_all(mg, case, oracle):
    host, dev, _want = case
    out = mg.gaussian_blur_surfaces([dev["odd"].planes(), dev["s66"].planes()], 7)
    assert [tuple(o.shape) for o in out] == [(242, 322, 3), (18, 66, 3)]
    for o, key in zip(out, ("odd", "s66")):
        assert np.array_equal(o.cpu().numpy(), oracle.gaussian_blur(_bgr_of(oracle, *host[key]), 7)), key


def test_the_result_does_not_depend_on_the_padding(mg, case):
    host, _dev, want = case
    outs = []
    for fill in (0x00, 0xFF):
        surfaces = {}
        for w, h, _k, py, puv, key, _off in ITEMS:
            if key not in surfaces:
                surfaces[key] = Surface(w, h, py, puv, *host[key], fill=fill)
        _bufs, out = _call(mg, surfaces)
        outs.append([o.clone() for o in out])
    for i, (a, b, exp) in enumerate(zip(outs[0], outs[1], want)):
        assert torch.equal(a, b), "items[%d]: the output depends on bytes [w, pitch) of a row" % i
        assert np.array_equal(a.cpu().numpy(), exp), "items[%d]" % i


# ---- the two-call tick: blur every decoder surface, then the surfaces step ---------------------------------------------------------------------------------------
VGA, HD = (640, 480), (1280, 720)
IN_PITCH = {VGA: (768, 704), HD: (1408, 1344)}                              # tests/test_gpu_surfaces.py's
OUT_PITCH = {(640, 360): 640, (320, 180): 320, (160, 90): 256}


def test_two_call_tick_equals_the_twin_on_bgr_frames(bs):
    from backscrub_amd import synth
    S = bs.StreamSetting
    path = model_path("lite")
    geoms = [VGA + (2,), HD + (2,)]
    fleet, twin = bs.MaskGen.with_geometries(path, geoms), bs.MaskGen.with_geometries(path, geoms)
    sizes = [VGA, VGA, HD, HD]
    conf = [dict(k=25), dict(k=7, flip_h=True), dict(k=25), dict(off=True)]      # stream: blur size, flip, filter off (which gets no blur item)
    ids = [2, 0, 3, 1]                                                      # classes interleaved
    records = [(s, z) for z in OUT_PITCH for s in ids]
    try:
        for t in range(2):
            surf, frames = {}, {}
            for s, (W, H) in enumerate(sizes):
                y, uv = twin.bgr_to_nv12(torch.from_numpy(synth.frame(W, H, s, t)).cuda()[None])
                surf[s] = Surface(W, H, *IN_PITCH[(W, H)], y[0].cpu().numpy(), uv[0].cpu().numpy())
                frames[s] = twin.nv12_to_bgr(*surf[s].planes())
            blurred = [s for s in ids if not conf[s].get("off")]
            ks = [conf[s]["k"] for s in blurred]
            planes = {}
            for ctx, name in ((fleet, "new"), (twin, "twin")):
                if ctx is fleet:
                    bgs = dict(zip(blurred, ctx.gaussian_blur_surfaces([surf[s].planes() for s in blurred], ks)))
                else:
                    bgs = dict(zip(blurred, ctx.gaussian_blur_batch([frames[s] for s in blurred], ks)))
                sett = [S(bg=bgs.get(s), flip_h=conf[s].get("flip_h", False), filter_off=conf[s].get("off", False)) for s in ids]
                outs = [Surface(ow, oh, OUT_PITCH[(ow, oh)], OUT_PITCH[(ow, oh)]) for _s, (ow, oh) in records]
                recs = [(ids.index(s),) + o.planes() for (s, _z), o in zip(records, outs)]
                if ctx is fleet:
                    ctx.step_surfaces(ids, [surf[s].planes() for s in ids], sett, recs)
                else:
                    ctx.step_vcam_geoms_outs_nv12(ids, [frames[s] for s in ids], sett, recs)
                planes[name] = outs
            for (s, (ow, oh)), a, b in zip(records, planes["new"], planes["twin"]):
                assert torch.equal(a.buf, b.buf), "t=%d stream %d -> %dx%d: the output surfaces differ (planes or what surrounds them)" % (t, s, ow, oh)
                assert not torch.equal(a.buf, a.before)
            for s in range(4):
                assert torch.equal(fleet.masks_of(s), twin.masks_of(s)), "t=%d stream %d: persistent masks differ" % (t, s)
            assert torch.equal(fleet.ofinal(), twin.ofinal()), "t=%d: temporal state differs" % t
            assert all(sf.unchanged() for sf in surf.values()), "an input surface was written"
    finally:
        fleet.close()
        twin.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(mg, items, n=None, null_items=False):
    """the C entry point with hand-made items (d_y, d_uv, d_dst, pitch_y, pitch_uv, w, h, ksize, flags): (return code, error text)"""
    from backscrub_amd import api
    arr = (api._BlurSurfaceItem * max(len(items), 1))()
    for i, f in enumerate(items):
        it = arr[i]
        it.d_y, it.d_uv, it.d_dst, it.pitch_y, it.pitch_uv, it.w, it.h, it.ksize, it.flags = f
    rc = api.lib().bsx_gaussian_blur_surfaces_batch(mg.h, None if null_items else arr, len(items) if n is None else n, api._stream_ptr())
    return rc, (api.lib().bsx_last_error(mg.h) or b"").decode(errors="replace")


def test_refusals_change_nothing(mg, case, oracle):
    import re
    host, dev, _want = case
    a, b = dev["t1"], dev["s66"]                                            # 64 x 16 at 64 / 64, 66 x 18 at 68 / 72
    buf0, d0 = _dst(64, 16)
    buf1, d1 = _dst(66, 18)
    P = lambda t: t.data_ptr()
    good = [(P(a.y), P(a.uv), P(d0), 64, 64, 64, 16, 5, 0), (P(b.y), P(b.uv), P(d1), 68, 72, 66, 18, 5, 0)]
    names = ("y", "uv", "dst", "pitch_y", "pitch_uv", "w", "h", "k", "flags")

    def second(**kw):
        """the good call with fields of items[1] replaced"""
        f = dict(zip(names, good[1]))
        f.update(kw)
        return [good[0], tuple(f[k] for k in names)]
    big = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    B = P(big)
    assert B % 4 == 0
    eight = [(B + 49152, B + 57344, B + 4096 * s, 64, 64, 8 + 4 * s, 6 + 2 * s, 3, 0) for s in range(8)]      # (planes inside `big` at every size)
    cases = [
        (second(w=0), r"items\[1\]: size 0 x 18 is not positive"),
        (second(h=-4), r"items\[1\]: size 66 x -4 is not positive"),
        (second(w=67), r"items\[1\]: NV12 needs an even width and height \(67 x 18\)"),
        (second(h=17), r"items\[1\]: NV12 needs an even width and height \(66 x 17\)"),
        (second(k=4), r"items\[1\]: ksize 4 "),
        (second(k=0), r"items\[1\]: ksize 0 "),
        (second(k=-1), r"items\[1\]: ksize -1 "),
        (second(k=33), r"items\[1\]: ksize 33 "),
        (second(y=None), r"items\[1\]: d_y is NULL"),
        (second(uv=None), r"items\[1\]: d_uv is NULL"),
        (second(dst=None), r"items\[1\]: d_dst is NULL"),
        (second(y=P(b.y) + 2), r"items\[1\]: d_y 0x%x is not 4-byte aligned" % (P(b.y) + 2)),
        (second(uv=P(b.uv) + 1), r"items\[1\]: d_uv 0x%x is not 4-byte aligned" % (P(b.uv) + 1)),
        (second(pitch_y=64), r"items\[1\]: pitch_y = 64 is below w = 66"),
        (second(pitch_y=70), r"items\[1\]: pitch_y = 70 is not a multiple of 4"),
        (second(pitch_uv=0), r"items\[1\]: pitch_uv = 0 is below w = 66"),
        (second(pitch_uv=74), r"items\[1\]: pitch_uv = 74 is not a multiple of 4"),
        (second(flags=64), r"items\[1\]: flags 0x40"),
        (second(flags=1), r"items\[1\]: flags 0x1"),
        (second(w=32768, h=21846, pitch_y=32768, pitch_uv=32768), r"items\[1\]: size 32768 x 21846 is beyond the kernel's 32-bit offsets"),
        (second(w=64, h=32770, pitch_y=65536, pitch_uv=64), r"items\[1\]: the Y plane \(32770 rows of pitch_y = 65536\) extends over 2 GiB or more"),
        (second(w=64, h=32772, pitch_y=64, pitch_uv=131072), r"items\[1\]: the UV plane \(16386 rows of pitch_uv = 131072\) extends over 2 GiB or more"),
        (eight + [(B + 49152, B + 57344, B + 4096 * 8, 64, 64, 40, 22, 3, 0)], r"items\[8\]: 40 x 22 is distinct size 9 of the call \(at most 8\)"),
        # a destination over its own Y plane (by its last four bytes), over another item's UV plane (64 x 7 + 64 bytes: by its last four), over another
        # destination (by one byte)
        ([(B + 3068, B + 8192, B, 64, 64, 64, 16, 5, 0)], r"items\[0\]: d_dst 0x%x overlaps the Y plane of items\[0\]" % B),
        ([good[0], (B, B + 8, P(a.uv) + 64 * 7 + 60, 4, 4, 2, 2, 3, 0)], r"items\[1\]: d_dst 0x%x overlaps the UV plane of items\[0\]" % (P(a.uv) + 64 * 7 + 60)),
        ([good[0], (B, B + 8, P(d0) + 64 * 16 * 3 - 1, 4, 4, 2, 2, 3, 0)], r"items\[1\]: d_dst 0x%x overlaps the destination of items\[0\]" % (P(d0) + 64 * 16 * 3 - 1)),
    ]
    for items, pattern in cases:
        rc, text = _raw(mg, items)
        assert rc == -1 and re.search(pattern, text) and "bsx_gaussian_blur_surfaces_batch" in text, (pattern, rc, text)
    # a plane ends at byte w of its last row, not at its pitch: 64 x 16 at pitches of 128 — Y [0, 1984), UV [2048, 3008) — and a destination right behind the UV plane
    rc, text = _raw(mg, [(B, B + 2048, B + 3008, 128, 128, 64, 16, 5, 0)])
    assert rc == 0, text
    rc, text = _raw(mg, [(B, B + 2048, B + 3004, 128, 128, 64, 16, 5, 0)])
    assert rc == -1 and "overlaps the UV plane of items[0]" in text, text
    for items, n, null, pattern in [([], -1, True, "n = -1 is negative"), ([good[0]] * 17, None, False, "n = 17 exceeds the context's 16 streams"), ([], 2, True, "items is NULL")]:
        rc, text = _raw(mg, items, n, null)
        assert rc == -1 and pattern in text, (pattern, rc, text)
    assert _raw(mg, [], 0, True)[0] == 0                                     # n == 0: nothing is read, nothing written
    torch.cuda.synchronize()
    for buf in (buf0, buf1):
        assert bool((buf == FILL).all()), "a refused call wrote a destination"
    assert a.unchanged() and b.unchanged()
    # a good call right afterwards is correct
    rc, text = _raw(mg, good)
    assert rc == 0, text
    torch.cuda.synchronize()
    assert np.array_equal(d0.cpu().numpy(), oracle.gaussian_blur(_bgr_of(oracle, *host["t1"]), 5))
    assert np.array_equal(d1.cpu().numpy(), oracle.gaussian_blur(_bgr_of(oracle, *host["s66"]), 5))
    assert _untouched_around(buf0, 64, 16) and _untouched_around(buf1, 66, 18)


def test_eight_sizes_pass_in_one_call(mg, oracle):
    from backscrub_amd import synth
    sizes = [(8 + 4 * i, 6 + 2 * i) for i in range(8)]
    host = [(synth.random_u8((h, w), 40 + i), synth.random_u8((h // 2, w), 80 + i)) for i, (w, h) in enumerate(sizes)]
    surf = [Surface(w, h, (w + 3) // 4 * 4 + 4 * (i % 3), (w + 3) // 4 * 4, *p) for i, ((w, h), p) in enumerate(zip(sizes, host))]
    out = mg.gaussian_blur_surfaces([s.planes() for s in surf] + [surf[0].planes()], 5)      # eight sizes, two surfaces of the first: 9 items
    for p, o in zip(host + [host[0]], out):
        assert np.array_equal(o.cpu().numpy(), oracle.gaussian_blur(_bgr_of(oracle, *p), 5))


def test_more_calls_than_ring_entries_without_a_synchronise(mg, case, oracle):
    host, dev, _want = case
    keys = ["t1", "s66"]
    ks = [(3 + 2 * (c % 14), 31 - 2 * (c % 14)) for c in range(KID_RING + 3)]
    outs = [mg.gaussian_blur_surfaces([dev[k].planes() for k in keys], list(kk)) for kk in ks]       # back to back: no synchronise in between
    torch.cuda.synchronize()
    bgr = {k: _bgr_of(oracle, *host[k]) for k in keys}
    for kk, out in zip(ks, outs):
        for key, k, o in zip(keys, kk, out):
            assert np.array_equal(o.cpu().numpy(), oracle.gaussian_blur(bgr[key], k)), "%s ksize %d" % (key, k)


def test_a_multi_class_context_gives_the_same_bytes(bs, mg, case):
    _host, dev, _want = case
    fleet = bs.MaskGen.with_geometries(synthetic_model_path("lite"), [VGA + (8,), HD + (8,)])
    try:
        _bufs, want = _call(mg, dev)
        _bufs2, got = _call(fleet, dev)
        for i, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(x, y), "items[%d]" % i
    finally:
        fleet.close()
