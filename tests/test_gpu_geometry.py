"""The image kernels around the network — prep, mask, tile classes, the outside-ROI strips and the composite — on every frame-geometry route, against the CPU oracle
(docs/design/02b-geometry-audit.md).  One case per row of tests/geometry_cases.py; tests/test_geometry_host.py proves from launch traces which route each row takes.

Every comparison is byte equality and none depends on the network's float result: prep is compared on identical frames, the mask kernels on injected model-resolution
states, and the whole step is judged from the DEVICE'S OWN temporal state — after each call the state the device holds is read back, the oracle's resize and blur make
the mask it implies, and the oracle's blend (flip, YUYV pack) makes the composite that mask implies."""
import numpy as np
import pytest

from conftest import model_path
import geometry_cases as gc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IN_PLACE = ("lite-132x100", "lite-512x288")          # one fused row and one unfused row also step in place (out is frames)


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_mask_of = gc.mask_of_state


def _states(oh, ow, seed):
    """the injected model-resolution states: pure noise; half 255 / half 0 with a horizontal edge; all 255 but one 254 byte and one 0 corner; 0 / 255 noise on one
    half and uniform on the other (both ways)"""
    rng = np.random.default_rng(seed)
    s = np.zeros((5, oh, ow), np.uint8)
    s[0] = rng.integers(0, 256, (oh, ow), dtype=np.uint8)
    s[1, : oh // 2] = 255
    s[2] = 255; s[2, oh // 3, ow // 2] = 254; s[2, -1, -1] = 0
    s[3] = rng.integers(0, 2, (oh, ow)).astype(np.uint8) * 255; s[3, :, : ow // 2] = 0
    s[4] = rng.integers(0, 2, (oh, ow)).astype(np.uint8) * 255; s[4, :, ow // 2:] = 255
    return s


def _flip(oracle, img, fh, fv):
    if fh and fv:
        return oracle.flip_bgr(img, -1)
    return oracle.flip_bgr(img, 1) if fh else (oracle.flip_bgr(img, 0) if fv else img)


@pytest.mark.parametrize("row", gc.ROWS, ids=gc.row_id)
def test_row_is_bit_exact(bs, oracle, row):
    from backscrub_amd import synth
    from backscrub_amd.api import BsxError, StreamSetting
    key, W, H, n, _, route = row
    path = model_path(key)
    mg = bs.MaskGen(path, W, H, n_streams=n)
    oc = oracle.Ctx(path, W, H)
    info = mg.info
    assert tuple(info["roi"]) == oc.roidim and tuple(info["in_roi"]) == oc.in_roidim
    oh, ow = info["out_h"], info["out_w"]
    if W * H > 1 << 20:                                             # a large frame: the scene rendered at a quarter of the size and repeated (rendering costs seconds there)
        base = np.stack([np.repeat(np.repeat(synth.frame((W + 3) // 4, (H + 3) // 4, s), 4, 0), 4, 1)[:H, :W] for s in range(n)])
    else:
        base = np.stack([synth.frame(W, H, s) for s in range(n)])
    base[n - 1] = synth.random_u8((H, W, 3), 7)                     # the last stream is pure noise: it stresses the integer paths
    even = W % 2 == 0

    # ---- prep: resize + BGR2RGB + bilateral + normalise, from BGR frames and (where prep reads them) from the packed YUYV form --------------------------------------
    mg.run_stage(0, _dev(base))
    got = mg.input_tensor().cpu().numpy()
    for i in range(n):
        want = oc.prep(base[i])
        assert np.array_equal(got[i], want), "prep, stream %d: %d values differ" % (i, (got[i] != want).sum())
    if even:
        packed = np.stack([oracle.bgr_to_yuyv(f) for f in base])
        unpacked = np.stack([oracle.yuyv_to_bgr(p) for p in packed])
    if route["stage4"]:
        mg.input_tensor().zero_()
        mg.run_stage(4, _dev(packed))
        got = mg.input_tensor().cpu().numpy()
        for i in range(n):
            want = oc.prep(unpacked[i])
            assert np.array_equal(got[i], want), "prep from YUYV, stream %d: %d values differ" % (i, (got[i] != want).sum())
    else:
        with pytest.raises(BsxError):
            mg.run_stage(4, _dev(np.zeros((n, H, W, 2), np.uint8)))

    # ---- mask from injected states (stand-alone mask kernel) ---------------------------------------------------------------------------------------------------
    states = list(_states(oh, ow, 5))
    # one state and its mask from the oracle's own post-processing: logits and a previous state of our choice, the oracle's decode + IIR makes the state
    rng = np.random.default_rng(11)
    oc.set_output((rng.standard_normal((oh, ow, info["out_c"])) * 3).astype(np.float32))
    oc.set_ofinal(rng.integers(0, 256, (oh, ow), dtype=np.uint8))
    oracle_mask = oc.post()
    states.append(oc.ofinal())
    assert np.array_equal(_mask_of(oracle, states[-1], info, W, H), oracle_mask)      # the helper IS the oracle's mask stage
    wants = [_mask_of(oracle, s, info, W, H) for s in states]
    for k0 in range(0, len(states), n):
        batch = states[k0:k0 + n]
        mg.ofinal()[:len(batch)].copy_(_dev(np.stack(batch)))
        mg.run_stage(3, n=len(batch))
        got = mg.masks().cpu().numpy()
        for j in range(len(batch)):
            assert np.array_equal(got[j], wants[k0 + j]), "state %d: %d mask bytes differ" % (k0 + j, (got[j] != wants[k0 + j]).sum())
    if route["cls"] != "none":
        rw, rh = info["roi"][2], info["roi"][3]
        tiles = ((rw + 127) // 128) * ((rh + 31) // 32) * n
        mg.ofinal().fill_(255)
        st = mg.mask_tile_stats()
        assert st["tiles"] == tiles
        if route["cls"] == "memset":                                # out of the classifier's range: every tile is general
            assert st["general"] == tiles and st["uniform_255"] == 0 and st["uniform_0"] == 0, st
        else:
            assert st["uniform_255"] == tiles and st["general"] == 0, st
        mg.ofinal()[0, info["in_roi"][1], info["in_roi"][0]] = 254  # one byte off in the first tile's source block
        st = mg.mask_tile_stats()
        assert st["general"] == (tiles if route["cls"] == "memset" else 1), st

    # ---- the whole step, judged from the device's own state --------------------------------------------------------------------------------------------------
    mg.reset()
    bg = synth.random_u8((n, H, W, 3), 81)
    d_bg = _dev(bg)
    out3 = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    out2 = torch.empty((n, H, W, 2), dtype=torch.uint8, device="cuda")
    lively = False
    t = 0

    def fresh():
        nonlocal t
        t += 1
        return np.ascontiguousarray(np.roll(base, (3 * t, 5 * t), axis=(1, 2)))      # fresh frames every call: the scene shifted, the noise with it

    def check(what, seen, got, m, flips, yuyv=False, no_mask=False, masks_before=None, bgs=None):
        """streams [0, m): the mask the device's state implies, the composite that mask implies; streams [m, n): untouched"""
        nonlocal lively
        of, masks = mg.ofinal().cpu().numpy(), mg.masks().cpu().numpy()
        lively = lively or bool(((of < 128).any() and (of >= 128).any()) or ((of != 0) & (of != 255)).any())
        for i in range(m):
            want_m = _mask_of(oracle, of[i], info, W, H)
            if no_mask:
                assert np.array_equal(masks[i], masks_before[i]), "%s: stream %d: the mask changed under no_mask" % (what, i)
            else:
                assert np.array_equal(masks[i], want_m), "%s: stream %d: %d mask bytes differ" % (what, i, (masks[i] != want_m).sum())
            want = _flip(oracle, oracle.alpha_blend(bg[i] if bgs is None else bgs[i], seen[i], want_m), *flips[i])
            if yuyv:
                want = oracle.bgr_to_yuyv(want)
            assert np.array_equal(got[i], want), "%s: stream %d: %d composite bytes differ" % (what, i, (got[i] != want).sum())
        return of, masks

    variants = [("plain", dict()), ("flip_h+yuyv", dict(flip_h=True, yuyv=True) if even else dict(flip_h=True)), ("yuyv_in", dict(yuyv_in=True)),
                ("flip_v+no_mask", dict(flip_v=True, no_mask=True))]
    for name, kw in variants:
        if kw.get("yuyv_in") and not even:
            with pytest.raises(BsxError):                            # odd width: refused, nothing advances
                mg.step_ex(_dev(np.zeros((n, H, W, 2), np.uint8)), d_bg, out3, yuyv_in=True)
            continue
        if kw.get("no_mask"):
            mg.masks().fill_(0x5A)                                   # any byte the library stores into the persistent masks shows
        for _ in range(3):
            frames = fresh()
            seen = frames
            if kw.get("yuyv_in"):
                pk = np.stack([oracle.bgr_to_yuyv(f) for f in frames])
                seen = np.stack([oracle.yuyv_to_bgr(p) for p in pk])
            before = mg.masks().cpu().numpy()
            out = out2 if kw.get("yuyv") else out3
            out.zero_()
            mg.step_ex(_dev(pk if kw.get("yuyv_in") else frames), d_bg, out, **kw)
            check(name, seen, out.cpu().numpy(), n, [(kw.get("flip_h", False), kw.get("flip_v", False))] * n, kw.get("yuyv", False), kw.get("no_mask", False), before)
        if kw.get("no_mask"):
            mg.masks().fill_(255)                                    # as bsx_new left them: the ROI is rewritten by the next storing call, outside it 255 stays
    if route["fused"]:                                               # every stream its own background and flip, one tile launch
        frames = fresh()
        flips = [(True, False), (False, True), (False, False)][:n]
        own = synth.random_u8((n, H, W, 3), 82)
        d_own = _dev(own)
        out3.zero_()
        mg.step_mixed(_dev(frames), out3, [StreamSetting(bg=d_own[i], flip_h=flips[i][0], flip_v=flips[i][1]) for i in range(n)])
        check("mixed", frames, out3.cpu().numpy(), n, flips, bgs=own)
    else:
        with pytest.raises(BsxError):
            mg.step_mixed(_dev(base), out3, [StreamSetting(bg=d_bg[i]) for i in range(n)])
    if gc.row_id(row) in IN_PLACE:
        frames = fresh()
        d_frames = _dev(frames)
        mg.step_ex(d_frames, d_bg, d_frames)
        check("in place", frames, d_frames.cpu().numpy(), n, [(False, False)] * n)
    # a partial batch: the streams beyond it keep their state and mask bytes
    of0, masks0 = mg.ofinal().cpu().numpy(), mg.masks().cpu().numpy()
    frames = fresh()
    out3.zero_()
    mg.step_ex(_dev(frames[:n - 1]), d_bg, out3[:n - 1])
    of1, masks1 = check("partial batch", frames, out3.cpu().numpy(), n - 1, [(False, False)] * n)
    assert np.array_equal(of1[n - 1], of0[n - 1]) and np.array_equal(masks1[n - 1], masks0[n - 1])
    assert not out3[n - 1].any()
    # the composite checks above are not trivial: some state the device held had both sides of the threshold, or a byte that is neither 0 nor 255
    assert lively
    oc.close()
    mg.close()
