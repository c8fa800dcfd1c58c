"""CPU checks of the despeckling definition (tests/despeckle_ref.py) against scipy's labelling and against cases spelled out by
hand, of what it is for - the Group 4 file of a noisy page - on the golden page, and of the host side of the switch
(yomitoku_amd/despeckle.py: check_despeckle; check_jpeg_preset; the serve entries).  The device is held to the definition in
tests/test_despeckle_gpu.py."""
import functools
import os

import numpy as np
import pytest

from tests import binarize_ref, ccitt_ref
from tests import despeckle_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_page.jpg")


# ---------------------------------------------------------------------------------------------------------------- scipy
def _by_scipy(black, n_black, n_white):
    ndimage = pytest.importorskip("scipy.ndimage")

    def remove(mask, n, structure):
        if n == 0:
            return mask, 0, 0
        labels, count = ndimage.label(mask, structure=structure)
        areas = np.bincount(labels.ravel(), minlength=count + 1)
        small = areas < n
        small[0] = False
        return mask & ~small[labels], int(small.sum()), int(areas[small].sum())

    step1, bc, bp = remove(np.asarray(black, bool), n_black, np.ones((3, 3), int))
    white, wc, wp = remove(~step1, n_white, ndimage.generate_binary_structure(2, 1))
    return ~white, (bc, bp, wc, wp)


@pytest.mark.parametrize("shape", [(1, 1), (1, 33), (33, 1), (17, 70), (64, 129)])
@pytest.mark.parametrize("density", [0.02, 0.2, 0.5, 0.8])
def test_the_definition_is_scipys_labelling(shape, density):
    pytest.importorskip("scipy")
    mask = np.random.default_rng(int(1000 * density) + shape[0] * shape[1]).random(shape) < density
    for n_black in (0, 1, 2, 4, 9):
        for n_white in (0, 1, 2, 4, 9):
            got, counts = R.despeckle(mask, n_black, n_white)
            exp, exp_counts = _by_scipy(mask, n_black, n_white)
            assert (got == exp).all() and counts == exp_counts, (shape, density, n_black, n_white)


# ---------------------------------------------------------------------------------------------------------------- by hand
def test_a_diagonal_line_is_one_black_component():
    line = np.eye(9, dtype=bool)
    assert len(R.components(line, R.NEIGHBOURS_8)) == 1 and len(R.components(line, R.NEIGHBOURS_4)) == 9
    clean, counts = R.despeckle(line, 9, 0)
    assert (clean == line).all() and counts == (0, 0, 0, 0)
    clean, counts = R.despeckle(line, 10, 0)
    assert not clean.any() and counts == (1, 9, 0, 0)
    # and the two sides of it are separate holes: 36 pixels each
    assert sorted(len(c) for c in R.components(~line, R.NEIGHBOURS_4)) == [36, 36]


def test_a_checkerboard_is_one_black_component_and_every_white_pixel_its_own():
    y, x = np.mgrid[0:6, 0:7]
    board = (y + x) % 2 == 0
    whites = int((~board).sum())
    assert len(R.components(board, R.NEIGHBOURS_8)) == 1 and len(R.components(~board, R.NEIGHBOURS_4)) == whites
    clean, counts = R.despeckle(board, 4, 2)
    assert clean.all() and counts == (0, 0, whites, whites)
    clean, counts = R.despeckle(board, 4, 1)
    assert (clean == board).all() and counts == (0, 0, 0, 0)


@pytest.mark.parametrize("n", [1, 2, 4, 9])
def test_a_component_of_exactly_n_pixels_stays_and_one_of_n_minus_1_goes(n):
    mask = np.zeros((5, 30), bool)
    mask[1, 1 : 1 + n] = True  # n pixels
    mask[3, 15 : 15 + n - 1] = True  # n - 1
    clean, counts = R.despeckle(mask, n, 0)
    assert clean[1, 1 : 1 + n].all() and not clean[3].any() and counts == ((1, n - 1, 0, 0) if n > 1 else (0, 0, 0, 0))
    clean, counts = R.despeckle(~mask, 0, n)  # the same for white
    assert not clean[1, 1 : 1 + n].any() and clean[3].all() and counts == ((0, 0, 1, n - 1) if n > 1 else (0, 0, 0, 0))


def test_a_speck_inside_a_pinhole_inside_a_blob():
    mask = np.zeros((11, 11), bool)
    mask[1:10, 1:10] = True  # the blob
    mask[4:7, 4:7] = False  # the pinhole: 9 pixels, 8 once the speck is in it
    mask[5, 5] = True  # the speck
    clean, counts = R.despeckle(mask, 2, 9)  # the speck goes, and the pinhole - 9 pixels now - stays
    assert not clean[5, 5] and not clean[4:7, 4:7].any() and counts == (1, 1, 0, 0)
    clean, counts = R.despeckle(mask, 2, 10)  # the second pass sees the first's result: the hole it fills has 9 pixels
    assert clean[1:10, 1:10].all() and counts == (1, 1, 1, 9)
    clean, counts = R.despeckle(mask, 0, 9)  # the speck stays: the ring round it has 8 pixels and is filled
    assert clean[1:10, 1:10].all() and counts == (0, 0, 1, 8)


def test_the_one_pixel_pages_have_no_exception_for_the_border():
    white, black = np.zeros((1, 1), bool), np.ones((1, 1), bool)
    assert R.despeckle(white, 4, 4) == (black, (0, 0, 1, 1))  # the rule taken literally: the white page becomes black
    clean, counts = R.despeckle(black, 4, 4)  # the speck goes - and the hole it leaves is filled again
    assert clean.all() and counts == (1, 1, 1, 1)
    clean, counts = R.despeckle(black, 4, 0)
    assert not clean.any() and counts == (1, 1, 0, 0)
    assert R.despeckle(black, 1, 1) == (black, (0, 0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------- the options
def test_check_despeckle_takes_and_refuses():
    from yomitoku_amd.despeckle import Despeckled, check_despeckle

    assert check_despeckle(False) is None and check_despeckle() is None
    assert check_despeckle(True) == {"black": 4, "white": 4}
    assert check_despeckle(7) == {"black": 7, "white": 7} and check_despeckle(65535) == {"black": 65535, "white": 65535}
    assert check_despeckle({"black": 3}) == {"black": 3, "white": 0} and check_despeckle({"white": 9}) == {"black": 0, "white": 9}
    assert check_despeckle({"black": 2, "white": 5}) == {"black": 2, "white": 5} and check_despeckle({"black": 0, "white": 1}) == {"black": 0, "white": 1}
    bad = [None, 0, -1, 65536, 4.0, "4", "auto", [4, 4], {}, {"black": 0}, {"black": 0, "white": 0}, {"ink": 4}, {"black": 4, "grey": 1},
           {"black": True}, {"white": 2.0}, {"black": "4"}, {"white": -1}, {"black": 65536}, {"black": None}]
    for value in bad:
        with pytest.raises(ValueError, match="despeckle"):
            check_despeckle(value)
    d = Despeckled(4, 4, 1, 2, 3, 4)
    assert (d.black, d.white, d.black_components, d.black_pixels, d.white_components, d.white_pixels) == (4, 4, 1, 2, 3, 4)
    with pytest.raises(Exception):
        d.black = 5  # frozen


def test_check_jpeg_preset_takes_the_switch_and_refuses_it_three_ways():
    from yomitoku_amd.jpeg import check_jpeg_preset, page_files

    assert check_jpeg_preset("high", jpeg_bilevel="otsu", jpeg_despeckle=True).despeckle == {"black": 4, "white": 4}
    assert check_jpeg_preset("low", jpeg_bilevel="auto", jpeg_despeckle={"white": 6}).despeckle == {"black": 0, "white": 6}
    assert check_jpeg_preset("high", False, None, False, "adaptive", False, 3).despeckle == {"black": 3, "white": 3}  # the last parameter
    assert check_jpeg_preset("high", jpeg_bilevel="otsu").despeckle is None and check_jpeg_preset("high").despeckle is None
    assert page_files("high", bilevel="otsu", despeckle=True).despeckle == {"black": 4, "white": 4}
    with pytest.raises(ValueError, match="despeckle"):  # a value check_despeckle refuses
        check_jpeg_preset("high", jpeg_bilevel="otsu", jpeg_despeckle={"black": 0})
    with pytest.raises(ValueError, match="jpeg_despeckle.*needs jpeg="):  # the switch without `jpeg`
        check_jpeg_preset(None, jpeg_despeckle=True)
    with pytest.raises(ValueError, match="there is no Group 4 file to clean"):  # the switch with jpeg_bilevel=False
        check_jpeg_preset("high", jpeg_despeckle=True)
    with pytest.raises(ValueError, match="there is no Group 4 file to clean"):
        check_jpeg_preset("high", jpeg_mrc=True, jpeg_despeckle=4)
    check_jpeg_preset(None, jpeg_despeckle=False)


def test_the_entry_points_refuse_before_a_source_is_read_or_a_device_asked_for():
    from yomitoku_amd.ccitt import EncodedBilevel, encode_g4_pages
    from yomitoku_amd.document_analyzer import OCR, DocumentAnalyzer
    from yomitoku_amd.jpeg import encode_jpeg_pages

    def sources():
        raise AssertionError("a source was read")
        yield

    for cls in (DocumentAnalyzer, OCR):
        an = object.__new__(cls)  # the checks stand in front of everything an analyzer owns
        an.visualize = False
        with pytest.raises(ValueError, match="jpeg_despeckle"):
            cls.serve(an, sources(), jpeg_despeckle=True)
        with pytest.raises(ValueError, match="no Group 4 file to clean"):
            cls.serve(an, sources(), jpeg="high", jpeg_despeckle=True)
        with pytest.raises(ValueError, match="despeckle"):
            cls.serve(an, sources(), jpeg="high", jpeg_bilevel="otsu", jpeg_despeckle={"dust": 4})
    page = np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError, match="despeckle"):
        encode_g4_pages([page], despeckle=0)
    with pytest.raises(ValueError, match="despeckle"):
        encode_jpeg_pages([page], "high", bilevel="otsu", despeckle="yes")
    with pytest.raises(ValueError, match="no Group 4 file to clean"):
        encode_jpeg_pages([page], "high", despeckle=True)
    # the entry's new field is its last, and None unless the switch ran: positional constructions and equality as before
    assert EncodedBilevel(b"x", 3, 2) == EncodedBilevel(b"x", 3, 2, 1.0, "auto", None, None) and EncodedBilevel(b"x", 3, 2).despeckled is None


# ---------------------------------------------------------------------------------------------------------------- the golden page
@functools.lru_cache(maxsize=None)
def _measured(noisy, method):
    """(bytes of the Group 4 file as is, bytes after despeckle(4, 4), pixels changed) of the golden page."""
    page = R.noisy_page(R.golden_page(GOLDEN)) if noisy else R.golden_page(GOLDEN)
    black = binarize_ref.black_mask(page, method)
    clean, _ = R.despeckle(black, 4, 4)
    return len(ccitt_ref.encode_g4(black)), len(ccitt_ref.encode_g4(clean)), int((clean != black).sum())


@pytest.mark.parametrize("method", ["otsu", "adaptive"])
def test_the_noisy_golden_pages_file_is_under_half_and_the_clean_page_is_almost_untouched(method):
    pytest.importorskip("PIL")
    before, after, _ = _measured(True, method)
    print(f"noisy, {method}: {before} -> {after} bytes ({after / before:.3f})")
    assert 2 * after < before  # the definition alone gives 0.21 and 0.22
    before, after, changed = _measured(False, method)
    print(f"clean, {method}: {before} -> {after} bytes, {changed} px")
    assert 0 < changed < 100 and after <= before  # the definition alone gives 35 and 41 px
