"""CPU checks of tests/image_ref.py against oracle/cvlike.py and the oracle chains of oracle/preprocess.py, on every case
tests/test_image_ops_gpu.py uses, so that the GPU module does not rest on an untested reference.  The two sides state the
operations differently (box integrals / tap tables, integer / float warp weights, array sums / cell loops); the uint8 ones
have to agree exactly, the float64 detector reference within the rounding of the fp32 restatement."""
import math

import numpy as np
import pytest

from oracle import cvlike
from oracle import preprocess as opre
from tests import image_ref as R

ALL_DET = R.DET_CASES + [R.DET_REFUSED]


@pytest.mark.parametrize("hw,ohw", ALL_DET)
def test_detector_reference_against_the_fp32_restatement(hw, ohw):
    """e32 = max |cvlike.resize_area + the reference's normalisation - det_ref64|.  A bound for it from the formats alone: the
    restatement is a convex combination of nx * ny values <= 255 with float32 weights, summed in float32 - at most
    (nx + ny + 6) roundings of 2^-24 relative to a partial sum <= 255 -, divided by 255 and by std >= 0.224, and cast once
    more.  Area cases must have clean overlaps (then the box integral and cv2's table are the same numbers)."""
    (h, w), (oh, ow) = hw, ohw
    img = R.det_page(h, w)
    ref = R.det_ref64(img, oh, ow)
    assert ref.shape == (3, oh, ow) and ref.dtype == np.float64 and np.isfinite(ref).all()
    sy, sx = R.det_scales(h, w, oh, ow)
    if sx >= 1 and sy >= 1:
        assert R.box_overlaps_are_clean(h, oh) and R.box_overlaps_are_clean(w, ow)
        nx, ny = math.ceil(sx) + 2, math.ceil(sy) + 2
    else:
        nx = ny = 2
    f32 = R.det_normalise32(cvlike.resize_area(img.astype(np.float32), (ow, oh)))
    e32 = float(np.abs(f32.astype(np.float64) - ref).max())
    print(f"det {hw} -> {ohw}: e32 = {e32:.3e}, max|ref| = {np.abs(ref).max():.3f}")
    assert e32 <= (nx + ny + 6) * 2.0 ** -24 / 0.224 + 2.0 ** -24 * np.abs(ref).max()


def test_detector_reference_edges():
    """Scale 1 returns the normalised pixels; integer scales are plain block means; a 1 x 1 page is constant; box weights sum
    to one per cell, and the length a cell is divided by, min(scale, ssize - d * scale), is `scale` to a few ulp of the double
    (scale = ssize / dsize, so only the last cell can be cut, by a rounding error).  The linear rule's fraction is below 1 in exact
    arithmetic before cv2 takes its fractional part; in double it reaches exactly 1.0f where d * scale falls one ulp short of an
    integer - at DET_FRACTION_ONE, which two detector cases contain, and at no other case's sizes - and there
    `fx - floor(fx)` makes it 0."""
    img = R.det_page(32, 32)
    assert np.array_equal(R.det_resize64(img, 32, 32), img.astype(np.float64))
    img = R.det_page(64, 96)
    blocks = img.astype(np.float64).reshape(32, 2, 32, 3, 3).mean(axis=(1, 3))
    assert np.abs(R.det_resize64(img, 32, 32) - blocks).max() < 1e-12
    one = R.det_page(1, 1)
    assert np.array_equal(R.det_resize64(one, 32, 32), np.broadcast_to(one.astype(np.float64), (32, 32, 3)))
    ones = {(s, d): at for s, d, at in R.DET_FRACTION_ONE}
    met = set()
    for (h, w), (oh, ow) in ALL_DET + [((1279, 1320), (1280, 1312))]:
        for s, d in ((h, oh), (w, ow)):
            scale = s / d
            k = np.arange(d, dtype=np.float64)
            if s >= d:
                assert np.abs(R.box_weights(s, d).sum(1) - 1.0).max() < 1e-12
                cell = np.minimum(scale, s - k * scale)
                assert (np.abs(cell - scale) <= 2 * np.spacing(float(s))).all(), (s, d)  # the rounding of d * scale, near ssize
                assert ((1.0 / cell).astype(np.float32) == np.float32(1.0 / scale)).all(), (s, d)  # gone in the weight's cast
            raw = ((k + 1.0) - (np.floor(k * scale) + 1.0) * (1.0 / scale)).astype(np.float32)
            at = np.flatnonzero(raw >= 1.0).tolist()
            i0, i1, f = R.linear_area_axis(s, d)
            if (s, d) in ones:
                n = ones[(s, d)]
                assert at == [n] and raw[n] == 1.0 and n * s % d == 0 and k[n] * scale < n * s // d, (s, d, at)
                assert i0[n] == n * s // d - 1 and i0[n] < s - 1 and f[n] == 0.0
                met.add((s, d))
            else:
                assert at == [], (s, d, at)
            assert i0.min() >= 0 and i1.max() <= s - 1 and (f >= 0).all() and (f < 1).all()
    assert met == set(ones)
    # an axis that shrinks by less than 2 under the linear rule: the two taps are the box integral; by 3 they are not
    for s, d, same in ((40, 32, True), (1320, 1312, True), (96, 32, False)):
        i0, i1, f = R.linear_area_axis(s, d)
        lin = np.zeros((d, s))
        np.add.at(lin, (np.arange(d), i0), 1.0 - f)
        np.add.at(lin, (np.arange(d), i1), f)
        gap = np.abs(lin - R.box_weights(s, d)).max()
        assert (gap < 1e-6) if same else (gap > 0.3), (s, d, gap)
    assert not R.box_overlaps_are_clean(1000, 999) and R.box_overlaps_are_clean(669, 32) and R.box_overlaps_are_clean(7, 7)


def test_warp_weights_integer_and_float_forms_agree():
    """All 32 x 32 fractions: cv2's float table (rint of products of n / 32, the fourth weight as what is left of 32768) is
    the integer table, and the fourth weight is also the rint of its own product - the products are exact in float32."""
    a = np.arange(32)
    ax, ay = (a[None, :] / np.float32(32)).astype(np.float32), (a[:, None] / np.float32(32)).astype(np.float32)
    one, k = np.float32(1), np.float32(32768)
    w00, w01, w10 = np.rint((one - ax) * (one - ay) * k), np.rint(ax * (one - ay) * k), np.rint((one - ax) * ay * k)
    w11 = 32768 - w00 - w01 - w10
    ix, iy = a[None, :], a[:, None]
    assert np.array_equal(w00, (32 - ix) * (32 - iy) * 32) and np.array_equal(w01, ix * (32 - iy) * 32)
    assert np.array_equal(w10, (32 - ix) * iy * 32) and np.array_equal(w11, ix * iy * 32)
    assert np.array_equal(w11, np.rint(ax * ay * k))


def _plans(table, pyramid=False):
    from yomitoku_amd import imaging

    quads = [v[0] for v in table.values()]
    if pyramid:
        plans, levels = imaging.plan_crops_pyramid(R.CROP_PAGE_HW, quads, R.CROP_CANVAS, True, source_downscale=True)
        assert levels.tolist() == [1] * len(quads)
    else:
        plans = imaging.plan_crops(R.CROP_PAGE_HW, quads, R.CROP_CANVAS, True)
    assert all(p is not None for p in plans)
    return quads, plans


def _record(plan):
    return plan.table[plan.row]


@pytest.mark.parametrize("which", ["level0", "level1", "stage2"])
def test_crop_references_match_the_oracle_chain(which):
    """warp_ref == cvlike.warp_perspective and crop_resize_ref == oracle.preprocess.parseq_crop / canvas_tensor (the turned
    form through a 180 degree turn of the oracle's ROI), for every quad of the GPU module, exactly."""
    table = {"level0": R.WARP_QUADS, "level1": R.WARP_QUADS_LEVEL1, "stage2": R.STAGE2_QUADS}[which]
    quads, plans = _plans(table, which == "level1")
    page = R.crop_page()
    if which == "level1":
        page = R.halve_ref(page)
        assert np.array_equal(page, cvlike.resize_half(R.crop_page()))
        quads = [(np.asarray(q, dtype=np.float32) / 2.0).tolist() for q in quads]
    rgb = page[:, :, ::-1]
    for name, quad, plan in zip(table, quads, plans):
        d = _record(plan)
        roi = rgb[d["by"]: d["by"] + d["bh"], d["bx"]: d["bx"] + d["bw"]]
        warped = R.warp_ref(roi, d["minv"], int(d["ww"]), int(d["wh"]))
        want = opre.extract_roi_with_perspective(rgb, quad)
        assert np.array_equal(warped, want), name
        t, cw, turned = opre.parseq_crop(rgb, quad, R.CROP_CANVAS, False, with_roi=True)
        assert cw == d["nw"]
        for flip in (0, 1):
            rec = {k: int(d[k]) for k in ("rot", "rw", "rh", "nw", "nh")}
            rec["flip"] = flip
            got = R.crop_resize_ref(warped, rec, 32, 800)
            if flip:
                t, _ = opre.canvas_tensor(np.ascontiguousarray(np.rot90(turned, 2)), R.CROP_CANVAS)
            assert np.array_equal(got, t.numpy()), (name, flip)


def test_stage2_quads_take_the_routes_they_are_named_for():
    """Every resize route upright and turned, from the planner itself; the route cv2's rule gives is the one the descriptor's
    fast_x / fast_y select."""
    _, plans = _plans(R.STAGE2_QUADS)
    seen = set()
    for (name, (_, route, rot)), plan in zip(R.STAGE2_QUADS.items(), plans):
        d = _record(plan)
        branch = R.area_branch(int(d["rw"]), int(d["rh"]), int(d["nw"]), int(d["nh"]))
        assert branch == route and bool(d["rot"]) == rot, name
        assert (d["fast_x"] > 0 and d["fast_y"] > 0) == (branch != "general"), name
        seen.add((name.replace("_rot", ""), rot))
    assert seen >= {(r, t) for r in ("copy", "fast2", "fast3", "general") for t in (False, True)}


@pytest.mark.parametrize("rw,rh,nw,nh", [(97, 53, 31, 17), (136, 200, 21, 32), (96, 40, 76, 32), (64, 64, 32, 32), (63, 45, 21, 15),
                                          (64, 32, 16, 8), (50, 30, 50, 30), (2000, 40, 800, 16)])
def test_area_resize_u8_against_cvlike(rw, rh, nw, nh):
    img = R.noise_page(rw * 3 + nh, rh, rw)
    assert np.array_equal(R.area_resize_u8(img, nw, nh), cvlike.resize_area(img, (nw, nh)))


@pytest.mark.parametrize("hw", R.HALVE_CASES + [(200, 136), (7, 3)])
def test_halve_reference_against_cvlike(hw):
    img = R.noise_page(hw[0] * 31 + hw[1], *hw)
    got = R.halve_ref(img)
    assert got.shape == (R.half_size(hw[0]), R.half_size(hw[1]), 3) and got.dtype == np.uint8
    assert np.array_equal(got, cvlike.resize_half(img))


def test_halve_reference_cells():
    """(5, 7) -> (2, 4): the fifth row is dropped, the last column is a one-pixel-wide cell; (3, 3) -> (2, 2): three cut cells;
    a 4 x 4 sum of 8 mod 16 is where round-half-even and round-half-up part (the 4 x 4 route of the crops)."""
    assert R.half_size(1) == 0 and R.half_size(3) == 2 and R.half_size(5) == 2 and R.half_size(7) == 4 and R.half_size(513) == 256
    img = R.noise_page(3, 5, 7).astype(np.int64)
    got = R.halve_ref(img.astype(np.uint8)).astype(np.int64)
    assert np.array_equal(got[1, 1], (img[2:4, 2:4].sum((0, 1)) + 2) >> 2)
    assert np.array_equal(got[1, 3], np.rint((img[2:4, 6].sum(0)).astype(np.float32) / np.float32(2)))
    img = np.zeros((3, 3, 3), dtype=np.uint8)
    img[2, 2] = (255, 1, 128)
    img[0:2, 2] = [[1, 2, 3], [2, 3, 3]]
    got = R.halve_ref(img)
    assert got[1, 1].tolist() == [255, 1, 128] and got[0, 1].tolist() == [2, 2, 3]  # 1.5 -> 2, 2.5 -> 2: half to even
    flat = np.zeros((4, 4, 3), dtype=np.uint8)
    flat[0, 0] = 8
    assert R.area_resize_u8(np.tile(flat, (2, 2, 1)), 2, 2)[0, 0, 0] == 0  # 8 / 16 = 0.5 -> 0


def test_pillow_cases_are_what_they_are_meant_to_be():
    """The resampler cases of the GPU module: kernel widths from 3 (an enlarged axis) to 39, an output wider than one
    256-thread block."""
    from yomitoku_amd import imaging

    ks = []
    for size in (131, 97, 1, 3):
        for out in (24, 40, 300, 7, 33, 257):
            b, c, k = imaging.pil_bilinear_coeffs(size, out)
            assert c.shape == (out, k) and (c.sum(1) > 0).all()
            ks.append(k)
    assert min(ks) == 3 and max(ks) == 39  # 131 -> 7: support 18.7, 2 * 19 + 1 taps
