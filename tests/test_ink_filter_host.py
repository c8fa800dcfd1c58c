"""CPU checks of the ink filter of layered pages: the definition (tests/ink_filter_ref.py) against scipy.ndimage, what it does
on the golden page, and the host side of the two keys (yomitoku_amd/despeckle.py: check_blobs; yomitoku_amd/mrc.py: check_mrc)."""
import functools
import os

import numpy as np
import pytest

from tests import deskew_ref, despeckle_ref, mrc_ref
from tests import ink_filter_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_page.jpg")


# ---------------------------------------------------------------------------------------------------------------- the definition
def _scipy_blobs(mask, side, fill):
    """Step 3 by scipy: label under the 3 x 3 structure, find_objects for the boxes."""
    ndimage = pytest.importorskip("scipy.ndimage")
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    out, gone, pixels = mask.copy(), 0, 0
    for k, (ys, xs) in enumerate(ndimage.find_objects(lab), start=1):
        bh, bw, a = ys.stop - ys.start, xs.stop - xs.start, int((lab[ys, xs] == k).sum())
        if bh >= side and bw >= side and 256 * a >= fill * bh * bw:
            out[lab == k] = False
            gone, pixels = gone + 1, pixels + a
    return out, gone, pixels


@pytest.mark.parametrize("side, fill", [(2, 64), (3, 128), (4, 100), (2, 256), (5, 1)])
def test_the_blob_step_equals_scipy_on_random_masks(side, fill):
    rng = np.random.default_rng(100 * side + fill)
    for shape, d in (((33, 70), 0.3), ((17, 97), 0.45), ((40, 40), 0.6), ((1, 50), 0.5), ((50, 1), 0.5), ((64, 64), 0.35)):
        mask = rng.random(shape) < d
        clean, gone, pixels, found = R.remove_blobs(mask, side, fill)
        want, want_gone, want_pixels = _scipy_blobs(mask, side, fill)
        assert (clean == want).all() and (gone, pixels) == (want_gone, want_pixels), (shape, d)
        assert len(found) == gone and sum(f[4] for f in found) == pixels


def test_filter_ink_is_despeckle_then_the_blob_step_and_zero_skips_a_step():
    rng = np.random.default_rng(7)
    mask = rng.random((40, 90)) < 0.4
    mask[5:25, 10:40] = True
    mask[8, 12] = mask[20, 30] = False  # pinholes: step 2 fills them before step 3 measures the block
    step2, four = despeckle_ref.despeckle(mask, 4, 4)
    step3, gone, pixels, _ = R.remove_blobs(step2, 8, 64)
    clean, six = R.filter_ink(mask, 4, 4, 8, 64)
    assert (clean == step3).all() and six == tuple(four) + (gone, pixels) and gone >= 1
    clean0, six0 = R.filter_ink(mask, 4, 4, 0, 64)
    assert (clean0 == step2).all() and six0 == tuple(four) + (0, 0)
    only, six_only = R.filter_ink(mask, 0, 0, 8, 64)
    assert six_only[:4] == (0, 0, 0, 0) and (only == R.remove_blobs(mask, 8, 64)[0]).all()


def test_both_equalities_of_the_rule():
    """256 a == fill bh bw goes and one pixel fewer stays; a box of exactly `side` goes and of side - 1 stays"""
    block = np.zeros((12, 12), bool)
    block[2:6, 3:11] = True  # 4 x 8, full: 256 * 32 == 256 * 32
    assert R.remove_blobs(block, 4, 256)[1:3] == (1, 32)
    block[3, 5] = False  # 31 pixels in the same box
    assert R.remove_blobs(block, 4, 256)[1:3] == (0, 0)
    assert R.remove_blobs(block, 4, 248)[1:3] == (1, 31)  # 256 * 31 == 248 * 32
    assert R.remove_blobs(block, 5, 1)[1:3] == (0, 0)  # bh = 4 = side - 1
    assert R.is_blob(1 << 27, 16383, 16383, 2, 128) and not R.is_blob(1 << 27, 16383, 16383, 2, 129)  # products above 2^32


# ---------------------------------------------------------------------------------------------------------------- the golden page
@functools.lru_cache(maxsize=None)
def _golden_ink():
    from PIL import Image

    bgr = np.ascontiguousarray(np.asarray(Image.open(GOLDEN).convert("RGB"))[..., ::-1])
    assert bgr.shape == (842, 596, 3)
    ink = deskew_ref.ink(bgr)
    return ink, despeckle_ref.despeckle(ink, 4, 4)[0]


def test_the_golden_pages_mask_file_shrinks_by_the_two_steps():
    ink, specks = _golden_ink()
    assert len(mrc_ref.mask_file(ink)) == 732
    assert len(mrc_ref.mask_file(specks)) == 670
    clean, six = R.filter_ink(ink, 4, 4, 48, 64)
    assert len(mrc_ref.mask_file(clean)) == 528 and six[4:] == (1, 2323)


def test_the_golden_pages_one_blob_is_the_clip_art_and_the_grid_stays():
    _, specks = _golden_ink()
    assert R.remove_blobs(specks, 48, 64)[3] == [(211, 289, 80, 154, 2323)]  # 79 x 75 pixels, fill 0.39
    assert R.remove_blobs(specks, 128, 64)[1:] == (0, 0, [])  # the default side: nothing on this small page
    grid = (130, 177, 72, 522, 1488)  # the table: 48 x 451, fill 0.069
    assert R.remove_blobs(specks, 48, 16)[3] == [grid, (211, 289, 80, 154, 2323)]  # without `fill` in the rule the grid would go


# ---------------------------------------------------------------------------------------------------------------- the switches
def test_check_blobs_accepts_and_refuses():
    from yomitoku_amd.despeckle import check_blobs

    assert check_blobs() is None and check_blobs(False) is None
    assert check_blobs(True) == {"side": 128, "fill": 64}
    assert check_blobs({}) == {"side": 128, "fill": 64}
    assert check_blobs({"side": 48}) == {"side": 48, "fill": 64}
    assert check_blobs({"fill": 256, "side": 2}) == {"side": 2, "fill": 256}
    assert check_blobs({"side": 16383, "fill": 1}) == {"side": 16383, "fill": 1}
    for bad in (None, 1, 48, "on", [48, 64], {"side": 1}, {"side": 0}, {"side": 16384}, {"side": 48.0}, {"side": True}, {"fill": 0},
                {"fill": 257}, {"fill": 0.25}, {"fill": False}, {"area": 4}, {"side": 48, "black": 4}):
        with pytest.raises(ValueError):
            check_blobs(bad)


def test_check_mrc_takes_the_two_keys_and_is_what_it_was_without_them():
    from yomitoku_amd.mrc import check_mrc

    cells = {"bg_cell": 2, "fg_cell": 8}
    assert check_mrc(True) == cells and check_mrc({}) == cells and check_mrc(False) is None
    assert check_mrc({"despeckle": False, "blobs": False}) == cells
    assert check_mrc({"despeckle": True}) == dict(cells, despeckle={"black": 4, "white": 4})
    assert check_mrc({"blobs": True, "bg_cell": 4}) == {"bg_cell": 4, "fg_cell": 8, "blobs": {"side": 128, "fill": 64}}
    assert check_mrc({"despeckle": {"black": 6}, "blobs": {"side": 48}}) == dict(cells, despeckle={"black": 6, "white": 0},
                                                                                  blobs={"side": 48, "fill": 64})
    assert check_mrc({"despeckle": 3}) == dict(cells, despeckle={"black": 3, "white": 3})
    for bad in ({"despeckle": 0}, {"despeckle": {"grey": 1}}, {"despeckle": "yes"}, {"blobs": 48}, {"blobs": {"side": 1}}, {"speckle": True},
                {"blobs": True, "bg_cell": 3}):
        with pytest.raises(ValueError):
            check_mrc(bad)


def test_the_switches_reach_the_page_files_through_the_dict_alone():
    from yomitoku_amd.jpeg import check_jpeg_preset, page_files

    files = check_jpeg_preset("high", jpeg_mrc={"despeckle": True, "blobs": {"side": 48}})
    assert files.mrc == {"bg_cell": 2, "fg_cell": 8, "despeckle": {"black": 4, "white": 4}, "blobs": {"side": 48, "fill": 64}}
    assert files.despeckle is None  # jpeg_despeckle keeps meaning the Group 4 pages
    assert page_files("high", mrc=True).mrc == {"bg_cell": 2, "fg_cell": 8}
    with pytest.raises(ValueError):
        check_jpeg_preset("high", jpeg_mrc={"blobs": {"fill": 300}})
    with pytest.raises(ValueError):
        check_jpeg_preset(None, jpeg_mrc={"despeckle": True})


def test_filter_params_and_the_record():
    from yomitoku_amd.despeckle import InkFiltered, filter_params, filter_result

    assert filter_params(None, {"side": 48, "fill": 64}) == {"black": 0, "white": 0, "side": 48, "fill": 64}
    assert filter_params({"black": 4, "white": 2}, None) == {"black": 4, "white": 2, "side": 0, "fill": 0}
    rec = filter_result(filter_params({"black": 4, "white": 4}, {"side": 48, "fill": 64}), [1, 2, 3, 4, 5, 6])
    assert rec == InkFiltered(4, 4, 48, 64, 1, 2, 3, 4, 5, 6)
    with pytest.raises(Exception):
        rec.side = 2  # frozen
