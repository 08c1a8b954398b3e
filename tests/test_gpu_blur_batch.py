"""bsx_gaussian_blur_bgr_batch on the GPU: n images, each of its own size, blur size and pixel format (BGR or a camera's raw YUYV 4:2:2), blurred in one launch.
Byte equality everywhere: against the CPU oracle (cv::GaussianBlur's integers, after cv::COLOR_YUV2BGR_YUYV's for a YUYV item), against bsx_gaussian_blur_bgr of each
image alone, and — as the background of the multi-geometry steps — against the mixed steps' own blur mode (`-p bgblur` without `-b`) on one-geometry contexts."""
import numpy as np
import pytest

from conftest import model_path, synthetic_model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KID_RING = 4                    # bsx_ctx::kIdRing (csrc/bsx_api.hip): entries of the descriptor staging ring
PAD, FILL = 64, 0xA5            # bytes around every destination, and what they (and a destination before the call) hold
# (w, h, ksize, yuyv, source key, destination offset in its buffer): interleaved in the caller's order — not by size, not by format.  8 distinct sizes.
ITEMS = [
    (640, 480, 25, False, "vga", PAD),         # word staging, interior and border tiles
    (66, 18, 5, True, "y66", PAD),             # YUYV, an even width that is no multiple of 4
    (64, 16, 5, False, "t1", PAD),             # exactly one tile
    (640, 480, 25, True, "yvga", PAD),         # YUYV, word staging
    (20, 12, 25, False, "small", PAD),         # smaller than the radius: multiple reflections
    (65, 17, 7, False, "t1+", PAD),            # one column and one row more than a tile
    (40, 30, 1, True, "y40", PAD),             # the conversion alone
    (322, 242, 3, False, "odd", PAD),          # w % 4 != 0: byte staging, byte stores
    (640, 480, 9, False, "vga", PAD + 1),      # the first item's source again, another blur size, the same size class; a destination that is not 4-byte aligned
    (130, 70, 31, False, "k31", PAD),          # the largest tap count
    (40, 30, 1, False, "c40", PAD),            # the copy
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


def _source(key, w, h, yuyv):
    """host image of an item: seeded noise ([h,w,2] for YUYV: any bytes are a valid frame); the first image has its top third at 255"""
    from backscrub_amd import synth
    img = synth.random_u8((h, w, 2 if yuyv else 3), 900 + sum(map(ord, key)))
    if key == "vga":
        img[: h // 3] = 255
    return img


@pytest.fixture(scope="module")
def case(oracle):
    """the item list: host sources, device sources, and the oracle's outputs — computed once, never written"""
    host, dev, want = {}, {}, []
    for w, h, k, yuyv, key, _off in ITEMS:
        if key not in host:
            host[key] = _source(key, w, h, yuyv)
            dev[key] = torch.from_numpy(host[key]).cuda()
        bgr = oracle.yuyv_to_bgr(host[key]) if yuyv else host[key]
        want.append(oracle.gaussian_blur(bgr, k))
    return host, dev, want


def _dst(w, h, off=PAD):
    """a destination inside a larger pattern-filled buffer: (buffer, the [h,w,3] view at byte `off`)"""
    buf = torch.full((off + w * h * 3 + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[off:off + w * h * 3].view(h, w, 3)


def _untouched_around(buf, w, h, off=PAD):
    return bool((buf[:off] == FILL).all()) and bool((buf[off + w * h * 3:] == FILL).all())


def _call(mg, case, items=ITEMS):
    _host, dev, _want = case
    bufs = [_dst(w, h, off) for w, h, _k, _y, _key, off in items]
    out = mg.gaussian_blur_batch([dev[key] for *_r, key, _off in items], [k for _w, _h, k, *_r in items], out=[d for _b, d in bufs])
    return bufs, out


def test_against_the_oracle(mg, case):
    assert len({(w, h) for w, h, *_r in ITEMS}) == 8                        # as many distinct sizes as one call takes
    bufs, out = _call(mg, case)
    torch.cuda.synchronize()
    for i, ((w, h, k, yuyv, key, off), (buf, dst), want) in enumerate(zip(ITEMS, bufs, case[2])):
        got = out[i].cpu().numpy()
        assert out[i].data_ptr() == dst.data_ptr()
        assert np.array_equal(got, want), "items[%d] %dx%d ksize %d %s: %d bytes differ" % (i, w, h, k, "yuyv" if yuyv else "bgr", (got != want).sum())
        assert _untouched_around(buf, w, h, off), "items[%d] %dx%d: bytes around the destination were written" % (i, w, h)


def test_same_as_the_single_call(mg, case):
    _bufs, out = _call(mg, case)
    for i, (w, h, k, yuyv, key, _off) in enumerate(ITEMS):
        src = case[1][key]
        single = mg.gaussian_blur(mg.yuyv_to_bgr(src[None]) if yuyv else src[None], k)[0]
        assert torch.equal(out[i], single), "items[%d] %dx%d ksize %d" % (i, w, h, k)


def test_new_outputs_and_one_ksize_for_all(mg, case, oracle):
    host, dev, _want = case
    out = mg.gaussian_blur_batch([dev["odd"], dev["y66"]], 7)
    assert [tuple(o.shape) for o in out] == [(242, 322, 3), (18, 66, 3)]
    assert np.array_equal(out[0].cpu().numpy(), oracle.gaussian_blur(host["odd"], 7))
    assert np.array_equal(out[1].cpu().numpy(), oracle.gaussian_blur(oracle.yuyv_to_bgr(host["y66"]), 7))


# ---- the two-call tick: blur every camera's own frame, then the multi-geometry step ----------------------------------------------------------------------------
VGA, HD = (640, 480), (1280, 720)


def _yuyv_frame(mg, bgr):
    """the frame as a camera delivers it (Y0 U Y1 V): bsx_bgr_to_yuyv packs Y0 V Y1 U, so bytes 1 and 3 of every macropixel change places"""
    h, w, _ = bgr.shape
    return mg.bgr_to_yuyv(bgr[None])[0].view(h, w // 2, 4)[:, :, [0, 3, 2, 1]].contiguous().view(h, w, 2)


@pytest.mark.parametrize("vcam", [None, (426, 240)], ids=["geoms", "vcam_geoms"])
def test_two_call_tick_equals_the_mixed_steps_blur_mode(bs, vcam):
    from backscrub_amd import synth
    S = bs.StreamSetting
    path = model_path("lite")
    fleet = bs.MaskGen.with_geometries(path, [VGA + (2,), HD + (2,)])
    sizes = [VGA, VGA, HD, HD]
    # stream: blur size, YUYV frame, flips, filter off
    conf = [dict(k=25, yin=True), dict(k=7, flip_h=True), dict(k=25), dict(k=7, off=True)]
    twins = [bs.MaskGen(path, W, H, n_streams=1) for W, H in sizes]
    ow, oh = vcam if vcam else (0, 0)
    for t in range(2):
        frames, sett, blur_src, blur_k, blur_pos = [], [], [], [], []
        for s, ((W, H), c) in enumerate(zip(sizes, conf)):
            fr = torch.from_numpy(synth.frame(W, H, s, t)).cuda()
            if c.get("yin"):
                fr = _yuyv_frame(fleet, fr)
            frames.append(fr)
            if not c.get("off"):                                            # a filter-off stream needs no blur item
                blur_src.append(fr); blur_k.append(c["k"]); blur_pos.append(s)
        bgs = dict(zip(blur_pos, fleet.gaussian_blur_batch(blur_src, blur_k)))
        for s, c in enumerate(conf):
            sett.append(S(bg=bgs.get(s), flip_h=c.get("flip_h", False), filter_off=c.get("off", False), yuyv_in=c.get("yin", False)))
        outs = [torch.zeros((oh, ow, 3) if vcam else (H, W, 3), dtype=torch.uint8, device="cuda") for W, H in sizes]
        ids = [2, 0, 3, 1]                                                  # classes interleaved
        step = fleet.step_vcam_geoms if vcam else fleet.step_geoms
        step(ids, [frames[s] for s in ids], [outs[s] for s in ids], [sett[s] for s in ids])
        for s, ((W, H), c, tw) in enumerate(zip(sizes, conf, twins)):
            one = S(bgblur=0 if c.get("off") else c["k"], flip_h=c.get("flip_h", False), filter_off=c.get("off", False))
            want = torch.zeros((1,) + tuple(outs[s].shape), dtype=torch.uint8, device="cuda")
            if vcam:
                tw.step_vcam_mixed(frames[s][None], want, [one], yuyv_in=c.get("yin", False))
            else:
                tw.step_mixed(frames[s][None], want, [one], yuyv_in=c.get("yin", False))
            assert torch.equal(outs[s], want[0]), "t=%d stream %d: composites differ" % (t, s)
            assert torch.equal(fleet.masks_of(s), tw.masks()[0]), "t=%d stream %d: persistent masks differ" % (t, s)
            assert torch.equal(fleet.ofinal()[s], tw.ofinal()[0]), "t=%d stream %d: temporal state differs" % (t, s)
    for c in [fleet] + twins:
        c.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(bs, mg, items):
    """the C entry point with hand-made items: (d_src, d_dst, w, h, ksize, flags)"""
    from backscrub_amd import api
    arr = (api._BlurItem * max(len(items), 1))()
    for i, (src, dst, w, h, k, fl) in enumerate(items):
        arr[i].d_src, arr[i].d_dst, arr[i].w, arr[i].h, arr[i].ksize, arr[i].flags = src, dst, w, h, k, fl
    api._check(api.lib().bsx_gaussian_blur_bgr_batch(mg.h, arr, len(items), api._stream_ptr()), mg.h, "bsx_gaussian_blur_bgr_batch")


def test_refusals_change_nothing(bs, mg, case, oracle):
    from backscrub_amd import api
    host, dev, _want = case
    YIN = api.BSX_STREAM_YUYV_IN
    src, ysrc = dev["t1"], dev["y66"]                                       # 64 x 16 BGR, 66 x 18 YUYV
    buf0, d0 = _dst(64, 16)
    buf1, d1 = _dst(66, 18)
    good = [(src.data_ptr(), d0.data_ptr(), 64, 16, 5, 0), (ysrc.data_ptr(), d1.data_ptr(), 66, 18, 5, YIN)]

    def second(**kw):
        """the good call with fields of items[1] replaced"""
        f = dict(zip(("src", "dst", "w", "h", "k", "fl"), good[1]))
        f.update(kw)
        return [good[0], (f["src"], f["dst"], f["w"], f["h"], f["k"], f["fl"])]
    big = torch.zeros(64 * 16 * 3 * 2, dtype=torch.uint8, device="cuda")
    cases = [
        (second(w=0), r"items\[1\].*0 x 18"),
        (second(h=-3), r"items\[1\].*66 x -3"),
        (second(k=4), r"items\[1\].*ksize 4"),
        (second(k=0), r"items\[1\].*ksize 0"),
        (second(k=-1), r"items\[1\].*ksize -1"),
        (second(k=33), r"items\[1\].*ksize 33"),
        (second(src=None), r"items\[1\].*d_src is NULL"),
        (second(dst=None), r"items\[1\].*d_dst is NULL"),
        (second(fl=YIN | 2), r"items\[1\].*0x42"),
        (second(fl=0x1900), r"items\[1\].*0x1900"),
        (second(w=65), r"items\[1\].*even width.*65"),
        (second(src=ysrc.data_ptr() + 2), r"items\[1\].*%x.*4-byte aligned" % (ysrc.data_ptr() + 2)),
        # a destination over its own source, over another item's source, over another destination (by one byte); a YUYV source's extent is w * h * 2
        ([(big.data_ptr(), big.data_ptr() + 64 * 16 * 3 - 1, 64, 16, 5, 0)], r"items\[0\].*overlaps the source of items\[0\]"),
        ([good[0], (ysrc.data_ptr(), src.data_ptr() + 5, 2, 2, 3, YIN)], r"items\[1\].*overlaps the source of items\[0\]"),
        ([good[0], (src.data_ptr(), d0.data_ptr() + 64 * 16 * 3 - 1, 2, 2, 3, 0)], r"items\[1\].*overlaps the destination of items\[0\]"),
        ([(big.data_ptr(), big.data_ptr() + 64 * 16 * 2 - 1, 64, 16, 5, YIN)], r"items\[0\].*overlaps the source of items\[0\]"),
    ]
    for items, pattern in cases:
        with pytest.raises(bs.BsxError, match=pattern):
            _raw(bs, mg, items)
    # a YUYV source ends after w * h * 2 bytes: a destination right behind it is fine
    _raw(bs, mg, [(big.data_ptr(), big.data_ptr() + 64 * 16 * 2, 64, 16, 5, YIN)])
    with pytest.raises(bs.BsxError, match="n = -1"):
        api._check(api.lib().bsx_gaussian_blur_bgr_batch(mg.h, None, -1, api._stream_ptr()), mg.h, "blur")
    with pytest.raises(bs.BsxError, match="n = 17.*16"):
        api._check(api.lib().bsx_gaussian_blur_bgr_batch(mg.h, (api._BlurItem * 17)(), 17, api._stream_ptr()), mg.h, "blur")
    with pytest.raises(bs.BsxError, match="items is NULL"):
        api._check(api.lib().bsx_gaussian_blur_bgr_batch(mg.h, None, 2, api._stream_ptr()), mg.h, "blur")
    assert api.lib().bsx_gaussian_blur_bgr_batch(mg.h, None, 0, api._stream_ptr()) == 0      # n == 0: nothing is read, nothing written
    torch.cuda.synchronize()
    for buf in (buf0, buf1):
        assert bool((buf == FILL).all()), "a refused call wrote a destination"
    # a good call right afterwards is correct
    _raw(bs, mg, good)
    torch.cuda.synchronize()
    assert np.array_equal(d0.cpu().numpy(), oracle.gaussian_blur(host["t1"], 5))
    assert np.array_equal(d1.cpu().numpy(), oracle.gaussian_blur(oracle.yuyv_to_bgr(host["y66"]), 5))
    assert _untouched_around(buf0, 64, 16) and _untouched_around(buf1, 66, 18)


def test_a_ninth_distinct_size_is_refused_and_eight_pass(bs, mg, oracle):
    from backscrub_amd import synth
    sizes = [(8 + 4 * i, 6 + i) for i in range(9)]
    host = [synth.random_u8((h, w, 3), 40 + i) for i, (w, h) in enumerate(sizes)]
    srcs = [torch.from_numpy(a).cuda() for a in host]
    # eight sizes, two images of the first: 9 items
    out = mg.gaussian_blur_batch(srcs[:8] + [srcs[0]], 5)
    for a, o in zip(host[:8] + [host[0]], out):
        assert np.array_equal(o.cpu().numpy(), oracle.gaussian_blur(a, 5))
    dst = [_dst(w, h) for w, h in sizes]
    with pytest.raises(bs.BsxError, match=r"items\[8\].*40 x 14"):
        mg.gaussian_blur_batch(srcs, 5, out=[d for _b, d in dst])
    torch.cuda.synchronize()
    assert all(bool((b == FILL).all()) for b, _d in dst)


def test_more_calls_than_ring_entries_without_a_synchronise(mg, case, oracle):
    host, dev, _want = case
    keys = [("t1", 64, 16, False), ("y66", 66, 18, True)]
    ks = [(3 + 2 * (c % 14), 31 - 2 * (c % 14)) for c in range(KID_RING + 3)]
    outs = [mg.gaussian_blur_batch([dev[k] for k, *_r in keys], list(kk)) for kk in ks]       # back to back: no synchronise in between
    torch.cuda.synchronize()
    for kk, out in zip(ks, outs):
        for (key, _w, _h, yuyv), k, o in zip(keys, kk, out):
            bgr = oracle.yuyv_to_bgr(host[key]) if yuyv else host[key]
            assert np.array_equal(o.cpu().numpy(), oracle.gaussian_blur(bgr, k)), "%s ksize %d" % (key, k)


def test_a_multi_class_context_takes_the_call(bs, mg, case):
    fleet = bs.MaskGen.with_geometries(synthetic_model_path("lite"), [VGA + (8,), HD + (8,)])
    _bufs, want = _call(mg, case)
    _bufs2, got = _call(fleet, case)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), "items[%d]" % i
    fleet.close()
