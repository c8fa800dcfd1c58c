"""The six kernels of yomitoku_amd/csrc/ymk_image.hip alone, on seeded uint8 noise, against the plain definitions of
tests/image_ref.py (which tests/test_image_ref_host.py holds against oracle/cvlike.py on the same cases):

  k_det_preprocess      float64 box integral / cv2's linear rule; the bound is max(4 x e32, 2^-22 max|ref|), e32 = the error of the
                        fp32 restatement (oracle.cvlike.resize_area + the reference's normalisation) measured here on the CPU
  k_pil_resize_*        Pillow's own BILINEAR, exactly
  k_warp_quads          the caller's scratch bytes against warp_ref, exactly - and every byte no crop owns left alone
  k_crop_resize_norm    crop_resize_ref of those bytes, exactly: {copy, 2 x 2, 3 x 3, general} x {upright, turned} x {flip 0, 1}
  k_halve_u8c3          halve_ref, exactly

Outputs start as a NaN pattern (0xA5 bytes for uint8) with a guard tail behind them; every launch is repeated for equal bits."""
import numpy as np
import pytest
import torch

from tests import hipops
from tests import image_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ detector
@pytest.mark.parametrize("hw,ohw", R.DET_CASES)
def test_det_preprocess_against_float64(dev, hw, ohw):
    from oracle import cvlike

    (h, w), (oh, ow) = hw, ohw
    sy, sx = R.det_scales(h, w, oh, ow)
    area = sx >= 1 and sy >= 1
    if area:
        assert R.box_overlaps_are_clean(h, oh) and R.box_overlaps_are_clean(w, ow)
    if (hw, ohw) in R.DET_MIXED:
        assert (sx < 1 < sy) or (sy < 1 < sx)  # the linear rule on an axis that shrinks
    img = R.det_page(h, w)
    ref = R.det_ref64(img, oh, ow)
    e32 = float(np.abs(R.det_normalise32(cvlike.resize_area(img.astype(np.float32), (ow, oh))).astype(np.float64) - ref).max())
    page = _dev(img, dev)
    y = hipops.det_preprocess(page, oh, ow)
    again = hipops.det_preprocess(page, oh, ow)
    got = y.cpu().numpy()
    assert not np.isnan(got).any()
    assert hipops.untouched(hipops.guard_tail(y))
    assert torch.equal(y.view(torch.int32), again.view(torch.int32))
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bound = R.det_bound(e32, ref)
    print(f"det {hw} -> {ohw} ({'area' if area else 'linear'}): e32 = {e32:.3e}, gpu = {err:.3e}, bound = {bound:.3e}")
    assert err <= bound
    if hw == ohw:  # one tap of weight 1: the normalised pixel, to the rounding of the fp32 division and the final cast
        assert np.array_equal(got, R.det_normalise32(np.ascontiguousarray(img.astype(np.float32))))


def test_det_preprocess_refuses_a_scale_of_21(dev):
    (h, w), (oh, ow) = R.DET_REFUSED
    assert h / oh == 21.0
    err, y = hipops.det_preprocess(_dev(R.det_page(h, w), dev), oh, ow, unchecked=True)
    assert err is not None and "down-scale factor too large" in err
    assert hipops.untouched(y) and hipops.untouched(hipops.guard_tail(y))


# ------------------------------------------------------------------ Pillow resamplers
PIL_BOXES = [None, (0, 0, 1, 1), (130, 96, 131, 97), (5, 3, 8, 96), (0, 40, 131, 43)]


@pytest.mark.parametrize("out_hw", [(24, 40), (300, 7), (33, 257)])
def test_pil_resize_is_pillow_exact(dev, out_hw):
    from PIL import Image

    from yomitoku_amd import imaging

    img = R.noise_page(5, 97, 131)
    page = _dev(img, dev)
    rgb = img[:, :, ::-1]
    singles = []
    for box in PIL_BOXES:
        crop = rgb if box is None else rgb[box[1]: box[3], box[0]: box[2]]
        want = np.asarray(Image.fromarray(np.ascontiguousarray(crop)).resize((out_hw[1], out_hw[0]), Image.BILINEAR))
        want = torch.from_numpy(want.copy()).permute(2, 0, 1).to(torch.float32).div(255)
        out, size, off = imaging.rtdetr_tensor(page, box, out_hw)
        assert size == crop.shape[:2] and off == ((0, 0) if box is None else box[:2])
        assert out.shape == (3,) + out_hw and torch.equal(out.cpu(), want), box
        singles.append(out)
    batch, metas = imaging.rtdetr_batch_tensor([page], [(0, box) for box in PIL_BOXES], out_hw)
    assert batch.shape == (len(PIL_BOXES), 3) + out_hw
    for k, one in enumerate(singles):
        assert torch.equal(batch[k].view(torch.int32), one.view(torch.int32)), PIL_BOXES[k]


# ------------------------------------------------------------------ text-line crops
def _plan(table, shape_hw, pyramid=False):
    """-> (descriptor records, canvas widths) of the quads of `table`, planned by the product's own planner."""
    from yomitoku_amd import imaging

    quads = [v[0] for v in table.values()]
    if pyramid:
        plans, levels = imaging.plan_crops_pyramid(shape_hw, quads, R.CROP_CANVAS, True, source_downscale=True)
        assert levels.tolist() == [1] * len(quads)
    else:
        plans = imaging.plan_crops(shape_hw, quads, R.CROP_CANVAS, True)
    assert all(p is not None for p in plans)
    descs = np.stack([p.table[p.row] for p in plans])
    assert descs["level"].tolist() == [1 if pyramid else 0] * len(quads)
    return descs, [p.canvas_width for p in plans]


def _owned(descs, offs, nbytes):
    own = np.zeros(nbytes, dtype=bool)
    for d, off in zip(descs, offs.tolist()):
        own[off: off + int(d["ww"]) * int(d["wh"]) * 3] = True
    return own


def _check_crop_launch(levels_np, levels_dev, descs, out_h, batch_w, slots, flip):
    """One launch of both stages: the scratch bytes against warp_ref (bytes no crop owns untouched), the batch tensor against
    crop_resize_ref of the GPU's bytes and of warp_ref's, every word written, -1 outside nw x nh, guard intact, bits repeat."""
    out, scratch, offs = hipops.crop_batch(levels_dev, descs, out_h, batch_w, slots=slots, flip=flip)
    out2, scratch2, _ = hipops.crop_batch(levels_dev, descs, out_h, batch_w, slots=slots, flip=flip)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(scratch, scratch2)
    assert hipops.untouched(hipops.guard_tail(out))
    got, raw = out.cpu().numpy(), scratch.cpu().numpy()
    assert not np.isnan(got).any()
    assert (offs % 16 == 0).all() and len(set(offs.tolist())) == len(descs)
    own = _owned(descs, offs, raw.size)
    assert (~own).sum() >= hipops.IMAGE_GUARD and (raw[~own] == hipops.SCRATCH_FILL).all()
    flips = np.broadcast_to(np.asarray(flip, dtype=np.int64), (len(descs),))
    fractional = []
    for k, d in enumerate(descs):
        ww, wh = int(d["ww"]), int(d["wh"])
        rgb = levels_np[int(d["level"])][:, :, ::-1]
        roi = rgb[d["by"]: d["by"] + d["bh"], d["bx"]: d["bx"] + d["bw"]]
        want = R.warp_ref(roi, d["minv"], ww, wh)
        mine = raw[offs[k]: offs[k] + ww * wh * 3].reshape(wh, ww, 3)
        assert np.array_equal(mine, want), f"crop {k}: warped bytes differ"
        xi, yi = R.warp_coords(d["minv"], ww, wh)
        fractional.append(float((((xi & 31) != 0) & ((yi & 31) != 0)).mean()))
        rec = {f: int(d[f]) for f in ("rot", "rw", "rh", "nw", "nh")}
        rec["flip"] = int(flips[k])
        slot = k if slots is None else int(slots[k])
        for src in (mine, want):
            assert np.array_equal(got[slot], R.crop_resize_ref(src, rec, out_h, batch_w)), f"crop {k}: tensor differs"
        assert (got[slot][:, :, rec["nw"]:] == -1).all() and (got[slot][:, rec["nh"]:, :] == -1).all()
    return fractional


@pytest.mark.parametrize("level", [0, 1])
def test_warp_stage_alone(dev, level):
    """The warped uint8 pixels in the caller's scratch: a translation (all 1/32 fractions zero), the whole page (the taps at
    sx + 1 == bw, sy + 1 == bh are masked), a quad reaching every page corner (taps outside the box on all four edges), slanted
    quads with fractions on both axes, a turned one - in ONE launch, so ww and wh differ per crop.  level 1: the same from the
    halved page of a source_downscale plan."""
    img = R.crop_page()
    page = _dev(img, dev)
    table = R.WARP_QUADS if level == 0 else R.WARP_QUADS_LEVEL1
    if level == 0:
        levels_np, levels_dev, shape = [img], [page], img.shape[:2]
    else:
        half = hipops.halve(page)
        assert np.array_equal(half.cpu().numpy(), R.halve_ref(img))
        levels_np, levels_dev, shape = [img, R.halve_ref(img)], [page, half], img.shape[:2]
    descs, canvases = _plan(table, shape, pyramid=level == 1)
    assert len({(int(d["ww"]), int(d["wh"])) for d in descs}) == len(descs)
    batch_w = max(canvases) + 8
    frac = _check_crop_launch(levels_np, levels_dev, descs, 32, batch_w, None, False)
    for (name, (_, translation, turned)), d, f in zip(table.items(), descs, frac):
        assert bool(d["rot"]) == turned, name
        if translation:
            xi, yi = R.warp_coords(d["minv"], int(d["ww"]), int(d["wh"]))
            assert ((xi & 31) == 0).all() and ((yi & 31) == 0).all(), name
        else:
            assert f > 0.5, (name, f)  # most pixels blend four source pixels
    if level == 0:
        d = descs[list(table).index("page")]
        assert (d["bw"], d["bh"], d["ww"], d["wh"]) == (136, 200, 136, 200)
        d = descs[list(table).index("corners")]
        assert (d["bx"], d["by"], d["bw"], d["bh"]) == (0, 0, 136, 200)


def test_resize_stage_every_route_turn_and_flip(dev):
    """All sixteen of {copy, fast 2 x 2, fast 3 x 3, general} x {upright, turned} x {flip 0, 1} - and fast 4 x 4, the only
    factor here whose sums have rounding ties - in one launch of eighteen crops, slots permuted, batch_w beyond every canvas
    and no multiple of the 64-thread block.  The route of each crop is read from its descriptor and has to be the intended one."""
    img = R.crop_page()
    page = _dev(img, dev)
    base, canvases = _plan(R.STAGE2_QUADS, img.shape[:2])
    descs = np.concatenate([base, base])
    flip = [0] * len(base) + [1] * len(base)
    names = list(R.STAGE2_QUADS) * 2
    ran = set()
    for name, d, f in zip(names, descs, flip):  # read from the very records and flips that are launched below
        _, route, turned = R.STAGE2_QUADS[name]
        branch = R.area_branch(int(d["rw"]), int(d["rh"]), int(d["nw"]), int(d["nh"]))
        taken = "copy" if (d["nw"], d["nh"]) == (d["rw"], d["rh"]) else "general" if not (d["fast_x"] > 0 and d["fast_y"] > 0) else \
            "fast2" if (d["fast_x"], d["fast_y"]) == (2, 2) else "fast"
        assert branch == route == taken and bool(d["rot"]) == turned, (name, branch, taken)
        if taken == "fast":
            taken += str(int(d["fast_x"]))
            assert d["fast_x"] == d["fast_y"] == int(name[4])
        ran.add((taken, bool(d["rot"]), int(f)))
    assert ran >= {(r, t, f) for r in ("copy", "fast2", "fast3", "general") for t in (False, True) for f in (0, 1)}
    slots = np.random.default_rng(3).permutation(len(descs))
    batch_w = 203
    assert batch_w > max(canvases) and batch_w % 64 != 0
    _check_crop_launch([img], [page], descs, 32, batch_w, slots, flip)


# ------------------------------------------------------------------ pyramid step
@pytest.mark.parametrize("hw", R.HALVE_CASES)
def test_halve_against_reference(dev, hw):
    img = R.noise_page(hw[0] * 31 + hw[1], *hw)
    page = _dev(img, dev)
    y, again = hipops.halve(page), hipops.halve(page)
    assert y.shape == (R.half_size(hw[0]), R.half_size(hw[1]), 3)
    assert np.array_equal(y.cpu().numpy(), R.halve_ref(img))
    assert hipops.untouched(hipops.guard_tail(y)) and torch.equal(y, again)


def test_halve_refuses_an_empty_destination(dev):
    h, w = R.HALVE_REFUSED
    assert R.half_size(h) == 0
    err, y = hipops.halve(_dev(R.noise_page(1, h, w), dev), unchecked=True)
    assert err is not None and "bad argument" in err
    assert hipops.untouched(hipops.guard_tail(y))
