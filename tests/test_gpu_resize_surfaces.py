"""bsx_resize_surfaces_batch on the GPU: n NV12 decoder surfaces, each of its own size and pitches, resized into BGR images of their own sizes in one launch.
Byte equality everywhere.  Expected values come from the CPU oracle alone: the 4:2:2 image Q[y][c] = (Y[y][2c], UV[y / 2][2c], Y[y][2c + 1], UV[y / 2][2c + 1]) is
built in numpy, converted with cv::COLOR_YUV2BGR_YUYV's integers and resized with cv::resize's.  The call is also compared with bsx_nv12_to_bgr followed by
bsx_resize_bgr of each surface alone, and — as the background of bsx_step_batch_surfaces — with a twin context that converts, resizes with bsx_resize_bgr and steps
the BGR frames through bsx_step_batch_vcam_geoms_outs_nv12.

Every surface, and every destination, lies in a larger buffer filled with a pattern; what surrounds the pixels is checked after the calls.  The planes are seeded
noise over the whole byte range, so both clamps of the conversion are hit on most taps."""
import numpy as np
import pytest

from conftest import model_path, synthetic_model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KID_RING = 4                    # bsx_ctx::kIdRing (csrc/bsx_api.hip): entries of the descriptor staging ring
PAD, FILL = 64, 0xA5            # bytes around every destination and every plane, and what they (and a destination before the call) hold
# (sw, sh, pitch_y, pitch_uv, dw, dh, surface key, destination offset in its buffer): interleaved in the caller's order, no class's items adjacent.  7 output sizes.
ITEMS = [
    (2, 2, 4, 4, 5, 3, "s2", PAD + 1),           # every tap clamps; byte stores; a tail group of one pixel
    (322, 182, 384, 328, 160, 96, "a", PAD),     # 15 workgroups per image; scale 2.0125 is not the area mode
    (6, 4, 8, 8, 6, 4, "s6", PAD),               # copy mode: equals bsx_nv12_to_bgr; sw % 4 == 2
    (66, 34, 128, 72, 20, 12, "s66", PAD),       # linear down by 3.3 x 2.83: odd and even left columns, odd and even upper rows; dword stores
    (24, 12, 24, 24, 12, 6, "s24", PAD),         # the 2x2 area mode; dword stores; pitch == sw
    (322, 182, 384, 328, 160, 96, "b", PAD),     # the second position of that class
    (18, 10, 20, 20, 20, 12, "s18", PAD),        # a second source size and table in the class of 20 x 12
    (66, 34, 128, 72, 21, 11, "s66", PAD + 1),   # a shared source; byte stores
    (16, 8, 16, 16, 36, 20, "s16", PAD),         # linear up: the right edge's clamped second tap, rows above the first at the top
    (66, 34, 128, 72, 160, 96, "s66", PAD),      # the third position of 160 x 96: up-scale and down-scale tables in one class
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
    """host planes of a surface: seeded noise over 0..255 (any bytes are a valid surface)"""
    from backscrub_amd import synth
    seed = 900 + sum(map(ord, key))
    return synth.random_u8((h, w), seed), synth.random_u8((h // 2, w), seed + 1)


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
    for sw, sh, py, puv, dw, dh, key, _off in ITEMS:
        if key not in host:
            host[key] = _planes(key, sw, sh)
            dev[key] = Surface(sw, sh, py, puv, *host[key])
        want.append(oracle.resize_linear(_bgr_of(oracle, *host[key]), dw, dh))
    assert all(int(p.min()) == 0 and int(p.max()) == 255 for k in ("a", "b", "s66") for p in host[k])      # the whole range
    return host, dev, want


def _dst(w, h, off=PAD):
    """a destination inside a larger pattern-filled buffer: (buffer, the [h,w,3] view at byte `off`)"""
    buf = torch.full((off + w * h * 3 + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[off:off + w * h * 3].view(h, w, 3)


def _untouched_around(buf, w, h, off=PAD):
    return bool((buf[:off] == FILL).all()) and bool((buf[off + w * h * 3:] == FILL).all())


def _call(mg, surfaces, items=ITEMS):
    bufs = [_dst(dw, dh, off) for _sw, _sh, _py, _puv, dw, dh, _key, off in items]
    out = mg.resize_surfaces([surfaces[it[6]].planes() for it in items], [(it[4], it[5]) for it in items], out=[d for _b, d in bufs])
    return bufs, out


def test_against_the_oracle(mg, case):
    assert len({(it[4], it[5]) for it in ITEMS}) == 7 and all(ITEMS[i][4:6] != ITEMS[i + 1][4:6] for i in range(len(ITEMS) - 1))
    _host, dev, want = case
    bufs, out = _call(mg, dev)
    torch.cuda.synchronize()
    for i, ((sw, sh, py, puv, dw, dh, key, off), (buf, dst), exp) in enumerate(zip(ITEMS, bufs, want)):
        got = out[i].cpu().numpy()
        assert out[i].data_ptr() == dst.data_ptr() and (dst.data_ptr() % 4 != 0) == (off != PAD)
        bad = (got != exp).any(axis=2)
        assert not bad.any(), "items[%d] %dx%d (pitches %d / %d) -> %dx%d: %d pixels differ, first at (y, x) = %s" % (
            i, sw, sh, py, puv, dw, dh, bad.sum(), tuple(int(v) for v in np.argwhere(bad)[0]))
        assert _untouched_around(buf, dw, dh, off), "items[%d] -> %dx%d: bytes around the destination were written" % (i, dw, dh)
    assert all(sf.unchanged() for sf in dev.values()), "a surface, its padding or its guard bytes were written"


def test_same_as_the_two_single_calls(mg, case):
    _host, dev, _want = case
    _bufs, out = _call(mg, dev)
    for i, (sw, sh, _py, _puv, dw, dh, key, _off) in enumerate(ITEMS):
        bgr = mg.nv12_to_bgr(*dev[key].planes())
        single = mg.resize_bgr(bgr[None], dw, dh)[0]
        assert torch.equal(out[i], single), "items[%d] %dx%d -> %dx%d" % (i, sw, sh, dw, dh)
        if (sw, sh) == (dw, dh):
            assert torch.equal(out[i], bgr), "items[%d]: the copy mode is the conversion" % i


def test_new_outputs_and_one_size_for_all(mg, case, oracle):
    host, dev, _want = case
    out = mg.resize_surfaces([dev["a"].planes(), dev["s66"].planes(), dev["s2"].planes()], (33, 17))
    assert [tuple(o.shape) for o in out] == [(17, 33, 3)] * 3
    for o, key in zip(out, ("a", "s66", "s2")):
        assert np.array_equal(o.cpu().numpy(), oracle.resize_linear(_bgr_of(oracle, *host[key]), 33, 17)), key
    assert mg.resize_surfaces([], (33, 17)) == []


def test_the_result_does_not_depend_on_the_padding(mg, case):
    host, _dev, want = case
    outs = []
    for fill in (0x00, 0xFF):
        surfaces = {}
        for sw, sh, py, puv, _dw, _dh, key, _off in ITEMS:
            if key not in surfaces:
                surfaces[key] = Surface(sw, sh, py, puv, *host[key], fill=fill)
        _bufs, out = _call(mg, surfaces)
        outs.append([o.clone() for o in out])
    for i, (a, b, exp) in enumerate(zip(outs[0], outs[1], want)):
        assert torch.equal(a, b), "items[%d]: the output depends on bytes [sw, pitch) of a row or on bytes around the planes" % i
        assert np.array_equal(a.cpu().numpy(), exp), "items[%d]" % i


# ---- the two-call tick: resize every background video's surface, then the surfaces step --------------------------------------------------------------------------
VGA, NHD = (640, 480), (640, 360)                                           # the two smallest classes tests/test_gpu_surfaces.py steps
IN_PITCH = {VGA: (768, 704), NHD: (640, 640)}
OUT_PITCH = {(320, 180): 320, (160, 90): 256}
# per stream: its background video's (sw, sh, pitch_y, pitch_uv) — a linear down-scale, the copy (a 640 x 480 video for a 640 x 480 camera), the 2x2 area mean
# (1280 x 720 for 640 x 360), a linear up-scale
VIDEO = {0: (802, 602, 896, 804), 1: (640, 480, 640, 704), 2: (1280, 720, 1408, 1280), 3: (162, 90, 192, 164)}


def test_two_call_tick_equals_the_twin_on_bgr_frames(bs):
    from backscrub_amd import synth
    S = bs.StreamSetting
    path = model_path("lite")
    geoms = [VGA + (2,), NHD + (2,)]
    fleet, twin = bs.MaskGen.with_geometries(path, geoms), bs.MaskGen.with_geometries(path, geoms)
    sizes = [VGA, VGA, NHD, NHD]
    ids = [2, 0, 3, 1]                                                      # classes interleaved
    records = [(s, z) for z in OUT_PITCH for s in ids]
    try:
        for t in range(3):
            surf, frames, video = {}, {}, {}
            for s, (W, H) in enumerate(sizes):
                y, uv = twin.bgr_to_nv12(torch.from_numpy(synth.frame(W, H, s, t)).cuda()[None])
                surf[s] = Surface(W, H, *IN_PITCH[(W, H)], y[0].cpu().numpy(), uv[0].cpu().numpy())
                frames[s] = twin.nv12_to_bgr(*surf[s].planes())
                vw, vh, vpy, vpuv = VIDEO[s]
                video[s] = Surface(vw, vh, vpy, vpuv, synth.random_u8((vh, vw), 50 + 10 * t + s), synth.random_u8((vh // 2, vw), 90 + 10 * t + s))
            planes = {}
            for ctx, name in ((fleet, "new"), (twin, "twin")):
                if ctx is fleet:
                    bgs = dict(zip(ids, ctx.resize_surfaces([video[s].planes() for s in ids], [sizes[s] for s in ids])))
                else:
                    bgs = {s: ctx.resize_bgr(ctx.nv12_to_bgr(*video[s].planes())[None], *sizes[s])[0] for s in ids}
                sett = [S(bg=bgs[s], flip_h=(s == 0)) for s in ids]
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
            assert all(sf.unchanged() for sf in list(surf.values()) + list(video.values())), "an input surface was written"
    finally:
        fleet.close()
        twin.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
NAMES = ("y", "uv", "dst", "pitch_y", "pitch_uv", "sw", "sh", "dw", "dh", "flags", "reserved")


def _raw(mg, items, n=None, null_items=False):
    """the C entry point with hand-made items (NAMES): (return code, error text)"""
    from backscrub_amd import api
    arr = (api._ResizeSurfaceItem * max(len(items), 1))()
    for i, f in enumerate(items):
        it = arr[i]
        it.d_y, it.d_uv, it.d_dst, it.pitch_y, it.pitch_uv, it.sw, it.sh, it.dw, it.dh, it.flags, it.reserved = f
    rc = api.lib().bsx_resize_surfaces_batch(mg.h, None if null_items else arr, len(items) if n is None else n, api._stream_ptr())
    return rc, (api.lib().bsx_last_error(mg.h) or b"").decode(errors="replace")


def test_refusals_change_nothing(mg, case, oracle):
    import re
    host, dev, _want = case
    a, b = dev["s24"], dev["s66"]                                           # 24 x 12 at 24 / 24, 66 x 34 at 128 / 72
    buf0, d0 = _dst(12, 6)
    buf1, d1 = _dst(20, 12)
    P = lambda t: t.data_ptr()
    good = [(P(a.y), P(a.uv), P(d0), 24, 24, 24, 12, 12, 6, 0, 0), (P(b.y), P(b.uv), P(d1), 128, 72, 66, 34, 20, 12, 0, 0)]

    def second(**kw):
        """the good call with fields of items[1] replaced"""
        f = dict(zip(NAMES, good[1]))
        f.update(kw)
        return [good[0], tuple(f[k] for k in NAMES)]
    big = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    B = P(big)
    assert B % 4 == 0
    eight = [(B + 49152, B + 57344, B + 4096 * s, 64, 64, 64, 16, 8 + 3 * s, 5 + 2 * s, 0, 0) for s in range(8)]      # (one surface inside `big`, eight output sizes)
    cases = [
        (second(y=None), r"items\[1\]: d_y is NULL"),
        (second(uv=None), r"items\[1\]: d_uv is NULL"),
        (second(dst=None), r"items\[1\]: d_dst is NULL"),
        (second(y=P(b.y) + 2), r"items\[1\]: d_y 0x%x is not 4-byte aligned" % (P(b.y) + 2)),
        (second(uv=P(b.uv) + 1), r"items\[1\]: d_uv 0x%x is not 4-byte aligned" % (P(b.uv) + 1)),
        (second(sw=0), r"items\[1\]: source size 0 x 34 is not positive"),
        (second(sh=-4), r"items\[1\]: source size 66 x -4 is not positive"),
        (second(sw=65), r"items\[1\]: NV12 needs an even width and height \(65 x 34\)"),
        (second(sh=33), r"items\[1\]: NV12 needs an even width and height \(66 x 33\)"),
        (second(pitch_y=64), r"items\[1\]: pitch_y = 64 is below sw = 66"),
        (second(pitch_y=70), r"items\[1\]: pitch_y = 70 is not a multiple of 4"),
        (second(pitch_uv=0), r"items\[1\]: pitch_uv = 0 is below sw = 66"),
        (second(pitch_uv=74), r"items\[1\]: pitch_uv = 74 is not a multiple of 4"),
        (second(dw=0), r"items\[1\]: output size 0 x 12 is not positive"),
        (second(dh=-3), r"items\[1\]: output size 20 x -3 is not positive"),
        (second(flags=64), r"items\[1\]: flags 0x40"),
        (second(flags=1), r"items\[1\]: flags 0x1"),
        (second(reserved=5), r"items\[1\]: reserved = 5 is not 0"),
        (second(dw=32768, dh=21846), r"items\[1\]: output size 32768 x 21846 is beyond the kernel's 32-bit offsets"),
        (second(sw=64, sh=32770, pitch_y=65536, pitch_uv=64), r"items\[1\]: the Y plane \(32770 rows of pitch_y = 65536\) extends over 2 GiB or more"),
        (second(sw=64, sh=32772, pitch_y=64, pitch_uv=131072), r"items\[1\]: the UV plane \(16386 rows of pitch_uv = 131072\) extends over 2 GiB or more"),
        (eight + [(B + 49152, B + 57344, B + 4096 * 8, 64, 64, 64, 16, 32, 21, 0, 0)], r"items\[8\]: 32 x 21 is distinct output size 9 of the call \(at most 8\)"),
        # a destination (12 x 6 x 3 = 216 bytes) over its own Y plane (by its last four bytes), over another item's UV plane (24 x 5 + 24 bytes: by its last four),
        # over another destination (by one byte)
        ([(B + 212, B + 8192, B, 64, 64, 64, 16, 12, 6, 0, 0)], r"items\[0\]: d_dst 0x%x overlaps the Y plane of items\[0\]" % B),
        ([good[0], (B, B + 8, P(a.uv) + 24 * 5 + 20, 4, 4, 2, 2, 5, 3, 0, 0)], r"items\[1\]: d_dst 0x%x overlaps the UV plane of items\[0\]" % (P(a.uv) + 24 * 5 + 20)),
        ([good[0], (B, B + 8, P(d0) + 12 * 6 * 3 - 1, 4, 4, 2, 2, 5, 3, 0, 0)], r"items\[1\]: d_dst 0x%x overlaps the destination of items\[0\]" % (P(d0) + 12 * 6 * 3 - 1)),
    ]
    for items, pattern in cases:
        rc, text = _raw(mg, items)
        assert rc == -1 and re.search(pattern, text) and "bsx_resize_surfaces_batch" in text, (pattern, rc, text)
    # a plane ends at byte sw of its last row, not at its pitch: 64 x 16 at pitches of 128 — Y [0, 1984), UV [2048, 3008) — and a destination right behind the UV plane
    rc, text = _raw(mg, [(B, B + 2048, B + 3008, 128, 128, 64, 16, 12, 6, 0, 0)])
    assert rc == 0, text
    rc, text = _raw(mg, [(B, B + 2048, B + 3004, 128, 128, 64, 16, 12, 6, 0, 0)])
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
    assert np.array_equal(d0.cpu().numpy(), oracle.resize_linear(_bgr_of(oracle, *host["s24"]), 12, 6))
    assert np.array_equal(d1.cpu().numpy(), oracle.resize_linear(_bgr_of(oracle, *host["s66"]), 20, 12))
    assert _untouched_around(buf0, 12, 6) and _untouched_around(buf1, 20, 12)


def test_eight_sizes_pass_in_one_call(mg, case, oracle):
    host, dev, _want = case
    sizes = [(8 + 3 * i, 5 + 2 * i) for i in range(8)]
    keys = ["s66", "a", "s16", "s66", "s24", "b", "s18", "s6", "s2"]
    out = mg.resize_surfaces([dev[k].planes() for k in keys], sizes + [sizes[0]])      # eight output sizes, the first twice: 9 items
    for k, (dw, dh), o in zip(keys, sizes + [sizes[0]], out):
        assert np.array_equal(o.cpu().numpy(), oracle.resize_linear(_bgr_of(oracle, *host[k]), dw, dh)), (k, dw, dh)


def test_more_calls_than_ring_entries_without_a_synchronise(mg, case, oracle):
    host, dev, _want = case
    keys = ["s24", "s66"]
    szs = [((7 + c, 5 + c), (40 - 3 * c, 9 + 2 * c)) for c in range(KID_RING + 3)]
    outs = [mg.resize_surfaces([dev[k].planes() for k in keys], list(zz)) for zz in szs]       # back to back: no synchronise in between
    torch.cuda.synchronize()
    bgr = {k: _bgr_of(oracle, *host[k]) for k in keys}
    for zz, out in zip(szs, outs):
        for key, (dw, dh), o in zip(keys, zz, out):
            assert np.array_equal(o.cpu().numpy(), oracle.resize_linear(bgr[key], dw, dh)), "%s -> %dx%d" % (key, dw, dh)


def test_a_multi_class_context_gives_the_same_bytes(bs, mg, case):
    _host, dev, _want = case
    fleet = bs.MaskGen.with_geometries(synthetic_model_path("lite"), [(640, 480, 8), (1280, 720, 8)])
    try:
        _bufs, want = _call(mg, dev)
        _bufs2, got = _call(fleet, dev)
        for i, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(x, y), "items[%d]" % i
    finally:
        fleet.close()
