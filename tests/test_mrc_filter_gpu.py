"""Layered pages with a filtered ink mask - `mrc={"despeckle": ..., "blobs": ...}` on separate_pages, encode_jpeg_pages and
OCR.serve: the mask rows, both layers and the three files are those of the definitions (tests/mrc_ref.py on the ink that
tests/ink_filter_ref.py leaves) and of the project's unchanged encoders, byte for byte; `mask.despeckled` says what went; a page
whose ink is all blobs stays the plain file; and without the two keys nothing differs from the call without them."""
import functools
import os

import numpy as np
import pytest

from tests import deskew_ref, mrc_ref
from tests import ink_filter_ref as R
from tests.test_mrc_serve_gpu import _check_layered

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_page.jpg")
MRC = {"despeckle": True, "blobs": {"side": 48}}
PARAMS = (4, 4, 48, 64)


def _patch_page(text=True):
    """96 x 160, B G R: tinted paper, a dark blue patch of 52 x 56 pixels - whose rim the adaptive rule marks as ink: one component
    with a box of at least 48 a side -, and, `text`, strokes and dust beside it."""
    rng = np.random.default_rng(17)
    page = np.empty((96, 160, 3), np.uint8)
    page[:] = (225, 238, 242)
    page[20:72, 60:116] = (120, 50, 30)
    if text:
        for y in range(8, 90, 9):
            page[y : y + 2, 6:52] = (40, 30, 35)
        page[10:88:6, 124:156] = (30, 30, 120)
        for y, x in zip(rng.integers(0, 96, 12), rng.integers(118, 160, 12)):
            page[y, x] = (20, 20, 20)
    return page


@functools.lru_cache(maxsize=None)
def cases():
    """(page, the definition's separation of it on the filtered ink, the six counts) of the golden page and of the patch page"""
    from PIL import Image

    golden = np.ascontiguousarray(np.asarray(Image.open(GOLDEN).convert("RGB"))[..., ::-1])
    out = []
    for page in (golden, _patch_page()):
        clean, six = R.filter_ink(deskew_ref.ink(page), *PARAMS)
        want = mrc_ref.separate(page, mask=clean)
        assert want[0] == 1 and (want[1] == clean).all() and six[4] >= 1  # a blob goes on either page
        out.append((page, want, six))
    assert out[0][2][4:] == (1, 2323)  # the golden page's clip art
    return out


def _record(six):
    from yomitoku_amd.despeckle import InkFiltered

    return InkFiltered(*PARAMS, *six)


def test_separate_pages_equals_the_definitions_on_the_filtered_ink(dev):
    from yomitoku_amd.despeckle import unpack_rows
    from yomitoku_amd.mrc import separate_pages

    got = separate_pages([c[0] for c in cases()], mrc=MRC)
    for (page, want, _), (flag, rows, fg, bg) in zip(cases(), got):
        assert flag == 1
        assert (unpack_rows(rows, page.shape[1]).cpu().numpy() == want[1]).all()
        assert np.array_equal(fg.cpu().numpy(), want[2]) and np.array_equal(bg.cpu().numpy(), want[3])
    # a caller's ink goes through the same filter
    inks = [deskew_ref.ink(c[0]) for c in cases()]
    again = separate_pages([c[0] for c in cases()], mrc=MRC, masks=inks)
    for a, b in zip(again, got):
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_encode_jpeg_pages_writes_the_three_files_of_the_filtered_page(dev):
    from yomitoku_amd.jpeg import encode_jpeg_pages
    from yomitoku_amd.mrc import encode_mrc_pages

    pages = [c[0] for c in cases()]
    got = encode_jpeg_pages(pages, "high", mrc=MRC)
    plain = encode_jpeg_pages(pages, "high", mrc=True)
    for (page, want, six), entry, before in zip(cases(), got, plain):
        _check_layered(entry, page, want, mrc_ref.mask_file(want[1]))
        assert entry.mask.despeckled == _record(six)
        assert before.mask.despeckled is None and len(entry.mask.data) < len(before.mask.data)  # what it is for
    assert len(got[0].mask.data) == 528 and len(plain[0].mask.data) == 732  # the golden page
    alone = encode_mrc_pages(pages, "high", MRC)
    assert alone == got and [e.mask.despeckled for e in alone] == [e.mask.despeckled for e in got]
    # either key alone: the other step is off, and says so
    for mrc, p in (({"despeckle": True}, (4, 4, 0, 0)), ({"blobs": {"side": 48}}, (0, 0, 48, 64))):
        entry = encode_jpeg_pages(pages[1:], "high", mrc=mrc)[0]
        clean, six = R.filter_ink(deskew_ref.ink(pages[1]), p[0], p[1], p[2], p[3] or 64)
        assert entry.mask.data == mrc_ref.mask_file(clean)
        d = entry.mask.despeckled
        assert (d.black, d.white, d.side, d.fill) == p and (d.black_components, d.black_pixels, d.white_components, d.white_pixels,
                                                            d.blob_components, d.blob_pixels) == six


def test_a_page_whose_ink_is_all_blobs_stays_the_plain_file(dev):
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg_pages
    from yomitoku_amd.mrc import separate_pages

    page = _patch_page(text=False)
    ink = deskew_ref.ink(page)
    clean, six = R.filter_ink(ink, *PARAMS)
    assert ink.any() and not clean.any() and six[4] == 1
    got = encode_jpeg_pages([page, cases()[1][0]], "high", mrc=MRC)
    plain = encode_jpeg_pages([page], "high")[0]
    assert isinstance(got[0], EncodedJpeg) and got[0] == plain and got[0].data == plain.data
    assert got[1].mask.despeckled == _record(cases()[1][2])  # beside a page that is layered as ever
    flag, rows, fg, bg = separate_pages([page], mrc=MRC)[0]
    assert flag == 0 and not rows.any() and fg is None and bg is None
    assert getattr(encode_jpeg_pages([page], "high", mrc=True)[0], "mrc", False) is True  # unfiltered, its rim is ink


def test_without_the_keys_the_files_are_those_of_the_call_without_them(dev):
    from yomitoku_amd.jpeg import encode_jpeg_pages

    pages = [c[0] for c in cases()]
    a = encode_jpeg_pages(pages, "high", mrc=True)
    b = encode_jpeg_pages(pages, "high", mrc={"bg_cell": 2, "fg_cell": 8})
    c = encode_jpeg_pages(pages, "high", mrc={"bg_cell": 2, "fg_cell": 8, "despeckle": False, "blobs": False})
    for x, y, z in zip(a, b, c):
        assert x == y == z
        assert x.mask.data == y.mask.data == z.mask.data and x.foreground.data == y.foreground.data == z.foreground.data
        assert x.background.data == y.background.data == z.background.data
        assert x.mask.despeckled is None and y.mask.despeckled is None and z.mask.despeckled is None


def test_an_ocr_serve_job_with_the_switches(dev):
    from tests.test_ocr_serve_gpu import _ocr
    from yomitoku_amd.jpeg import encode_jpeg_pages

    pages = [c[0] for c in cases()]
    an = _ocr()
    try:
        base = an.serve(pages, wave=2, jpeg="high", jpeg_mrc=True)
        got = an.serve(pages, wave=2, jpeg="high", jpeg_mrc=MRC)
    finally:
        an.close()
    want = encode_jpeg_pages(pages, "high", mrc=MRC)
    for entry, plain, w, (_, _, six) in zip(got, base, want, cases()):
        assert len(entry) == 2 and entry[0].model_dump() == plain[0].model_dump()  # the networks see the page as it arrived
        assert entry[1] == w and entry[1].mask.data == w.mask.data and entry[1].foreground.data == w.foreground.data
        assert entry[1].background.data == w.background.data and entry[1].mask.despeckled == _record(six)
        assert plain[1].mask.despeckled is None
