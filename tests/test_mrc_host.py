"""Layered pages on the host: the definition (tests/mrc_ref.py) against its literal loop, exact separation of a flat page, the
values `check_mrc` and `check_jpeg_preset` take and refuse, and the PDF writer's handling of an EncodedMrc - on plain objects of
its shape, without torch or the library.  No GPU."""
import re
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from tests import mrc_ref as R


def _flat_page(h=45, w=70, seed=0):
    """paper (200, 220, 240), ink (90, 30, 20) in two-pixel rules with random gaps -> (page, its ink)"""
    rng = np.random.default_rng(seed)
    ink = np.zeros((h, w), bool)
    for y0 in range(4, h - 3, 7):
        ink[y0 : y0 + 2, 5 : w - 5] = rng.random(w - 10) < 0.7
    page = np.empty((h, w, 3), np.uint8)
    page[:] = (200, 220, 240)
    page[ink] = (90, 30, 20)
    return page, ink


def _noisy(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ink = ((yy % 7 < 2) & (xx % 11 < 7)) ^ (rng.random((h, w)) < 0.03)
    shape = (h, w) if ch == 1 else (h, w, 3)
    base = np.where(ink if ch == 1 else ink[..., None], 50, 210)
    return np.clip(base + rng.integers(-25, 26, shape), 0, 255).astype(np.uint8)


def _same(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert (x is None and y is None) or (x.dtype == y.dtype == np.uint8 and x.shape == y.shape and np.array_equal(x, y))


@pytest.mark.parametrize("shape,cells", [((13, 21, 3), (2, 8)), ((17, 33), (1, 2)), ((3, 5, 3), (16, 16)), ((20, 19, 3), (4, 4)), ((9, 40), (2, 16))])
def test_the_definition_equals_the_literal_loop(shape, cells):
    page = _noisy(shape[0], shape[1], 1 if len(shape) == 2 else 3, sum(shape))
    got = R.separate(page, *cells)
    _same(got, R.separate_loop(page, *cells))
    rng = np.random.default_rng(5)
    for density in (0.5, 0.05, 0.999):
        mask = rng.random(shape[:2]) < density
        _same(R.separate(page, *cells, mask=mask), R.separate_loop(page, *cells, mask=mask))


def test_masks_without_ink_or_without_paper_have_flag_0():
    page = _noisy(12, 18, 3, 1)
    for mask in (np.zeros((12, 18), bool), np.ones((12, 18), bool)):
        assert R.separate(page, mask=mask)[0] == 0 and R.separate_loop(page, mask=mask)[0] == 0
    lone = np.zeros((12, 18), bool)
    lone[0, 0] = True
    flag, _, fg, bg = R.separate(page, 2, 8, mask=lone)
    assert flag == 1 and (fg == page[0, 0]).all()  # everything is pushed from the top
    _same(R.separate(page, 2, 8, mask=lone), R.separate_loop(page, 2, 8, mask=lone))
    edge = np.ones((3, 3), bool)
    edge[1, 1] = False  # paper, but none outside the dilated ink
    assert R.separate(page[:3, :3], mask=edge)[0] == 0


def test_dilation_is_the_3_x_3_square_clipped_at_the_edge():
    m = np.zeros((5, 6), bool)
    m[0, 0] = m[3, 4] = True
    want = np.zeros((5, 6), bool)
    want[0:2, 0:2] = want[2:5, 3:6] = True
    assert np.array_equal(R.dilate(m), want)


def test_a_flat_page_separates_exactly():
    page, ink = _flat_page()
    flag, M, fg, bg = R.separate(page)
    assert flag == 1 and np.array_equal(M, ink)
    assert fg.shape == (6, 9, 3) and bg.shape == (23, 35, 3)
    assert (fg == (90, 30, 20)).all() and (bg == (200, 220, 240)).all()
    assert np.array_equal(R.compose(M, fg, bg), page)
    for cells in ((1, 1), (4, 16), (16, 2)):
        _, M2, fg2, bg2 = R.separate(page, *cells)
        assert np.array_equal(R.compose(M2, fg2, bg2, *cells), page)


def test_check_mrc_takes_and_refuses():
    from yomitoku_amd.mrc import CELLS, DEFAULTS, check_mrc
    from yomitoku_amd.serving import check_jpeg_preset

    assert DEFAULTS == {"bg_cell": 2, "fg_cell": 8} and CELLS == (1, 2, 4, 8, 16)
    assert check_mrc(False) is None and check_mrc(True) == DEFAULTS and check_mrc({}) == DEFAULTS
    assert check_mrc({"bg_cell": 1}) == {"bg_cell": 1, "fg_cell": 8} and check_mrc({"bg_cell": 16, "fg_cell": 4}) == {"bg_cell": 16, "fg_cell": 4}
    bad = [None, 1, "auto", "True", [2, 8], {"cell": 2}, {"bg_cell": 3}, {"fg_cell": 32}, {"bg_cell": 0}, {"bg_cell": 2.0}, {"fg_cell": True},
           {"bg_cell": "2"}]
    for value in bad:
        with pytest.raises(ValueError, match="mrc"):
            check_mrc(value)
        with pytest.raises(ValueError, match="mrc"):
            check_jpeg_preset("high", jpeg_mrc=value)
    for good in (True, {"bg_cell": 4}, {"bg_cell": 1, "fg_cell": 16}):
        check_jpeg_preset("low", jpeg_mrc=good)
        check_jpeg_preset("high", True, "4:4:4", "auto", "adaptive", good)
        with pytest.raises(ValueError, match="jpeg_mrc"):
            check_jpeg_preset(None, jpeg_mrc=good)
    check_jpeg_preset(None, jpeg_mrc=False)
    check_jpeg_preset(None)


def test_the_public_entry_points_refuse_before_a_source_is_read():
    from yomitoku_amd.document_analyzer import OCR, DocumentAnalyzer

    def sources():
        raise AssertionError("a source was read")
        yield

    for cls in (DocumentAnalyzer, OCR):
        an = object.__new__(cls)  # the checks stand in front of everything an analyzer owns
        an.visualize = False
        with pytest.raises(ValueError, match="jpeg_mrc"):
            cls.serve(an, sources(), jpeg_mrc=True)
        with pytest.raises(ValueError, match="mrc"):
            cls.serve(an, sources(), jpeg="high", jpeg_mrc={"bg_cell": 3})


def test_the_encoder_entry_refuses_before_any_device_work():
    from yomitoku_amd.jpeg import encode_jpeg_pages
    from yomitoku_amd.mrc import encode_mrc_pages, separate_pages

    for bad in ("yes", {"bg_cell": 5}, None):
        with pytest.raises(ValueError, match="mrc"):
            encode_jpeg_pages([np.zeros((4, 4), np.uint8)], "high", mrc=bad)
    with pytest.raises(ValueError, match="mrc"):
        encode_mrc_pages([], "high", mrc=False)
    with pytest.raises(ValueError, match="mrc"):
        separate_pages([], mrc=False)
    assert separate_pages([]) == [] and encode_jpeg_pages([], "high", mrc=True) == []


# ------------------------------------------------------------------------------------------------ the PDF
def _jpeg(w, h, grey, tag):
    return SimpleNamespace(data=b"\xff\xd8" + tag + b"\xff\xd9", width=w, height=h, grey=grey, scale=1.0)


def _mrc(w=70, h=45, bg_cell=2, fg_cell=8, grey=False):
    mask = SimpleNamespace(data=b"MASK-BYTES\x00\x10\x01", width=w, height=h, scale=1.0, bilevel=True)
    return SimpleNamespace(mask=mask, background=_jpeg(-(-w // bg_cell), -(-h // bg_cell), grey, b"BACKGROUND"),
                           foreground=_jpeg(-(-w // fg_cell), -(-h // fg_cell), grey, b"FOREGROUND"), width=w, height=h, scale=1.0,
                           bg_cell=bg_cell, fg_cell=fg_cell, mrc=True)


def _doc():
    return SimpleNamespace(words=[SimpleNamespace(points=[[5, 5], [40, 5], [40, 15], [5, 15]], content="abc", direction="horizontal")])


def _objects(pdf):
    return {int(m.group(1)): m.group(2) for m in re.finditer(rb"(\d+) 0 obj\n(.*?)\nendobj\n", pdf, flags=re.S)}


def _stream(body):
    return body.split(b"stream\n", 1)[1].rsplit(b"\nendstream", 1)[0]


def test_a_layered_page_becomes_three_images_and_two_placements():
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    entry = _mrc()
    objs = _objects(searchable_pdf_bytes([entry], [_doc()]))
    images = {k: v for k, v in objs.items() if b"/Subtype /Image" in v}
    assert len(images) == 3
    (n_mask, mask), = [(k, v) for k, v in images.items() if b"/CCITTFaxDecode" in v]
    (n_fore, fore), = [(k, v) for k, v in images.items() if b"/Mask" in v and b"/ImageMask" not in v]
    (n_back, back), = [(k, v) for k, v in images.items() if k not in (n_mask, n_fore)]
    assert _stream(mask) == entry.mask.data and _stream(fore) == entry.foreground.data and _stream(back) == entry.background.data
    assert b"/ImageMask true" in mask and b"/BitsPerComponent 1" in mask and b"/ColorSpace" not in mask
    assert b"/DecodeParms << /K -1 /Columns 70 /Rows 45 >>" in mask and b"/Width 70 /Height 45" in mask
    assert f"/Mask {n_mask} 0 R".encode() in fore and b"/Filter /DCTDecode" in fore and b"/Width 9 /Height 6" in fore and b"/DeviceRGB" in fore
    assert b"/Filter /DCTDecode" in back and b"/Mask" not in back and b"/Width 35 /Height 23" in back
    (page,) = [v for v in objs.values() if b"/Type /Page " in v]
    assert b"/MediaBox [0 0 70 45]" in page
    names = dict(re.findall(rb"/(Im\d) (\d+) 0 R", page))
    assert {names[b"Im0"], names[b"Im1"]} == {str(n_fore).encode(), str(n_back).encode()}
    content = zlib.decompress(_stream(objs[int(re.search(rb"/Contents (\d+) 0 R", page).group(1))])).decode()
    lines = content.split("\n")
    back_name, fore_name = ("Im1", "Im0") if names[b"Im1"] == str(n_back).encode() else ("Im0", "Im1")
    # the background in its box of whole cells, 35 x 2 by 23 x 2, anchored at the top-left: 46 - 45 = 1 point below the page
    assert lines[0] == f"q 70 0 0 46 0 -1 cm /{back_name} Do Q"
    assert lines[1] == f"q 70 0 0 45 0 0 cm /{fore_name} Do Q"
    assert lines[2] == "BT" and "Tj" in content  # the text layer behind them, at scale 1.0


def test_a_grey_layered_page_and_cells_that_divide_the_page():
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    pdf = searchable_pdf_bytes([_mrc(64, 32, 4, 16, grey=True)], [_doc()])
    assert pdf.count(b"/DeviceGray") == 2 and pdf.count(b"/DeviceRGB") == 0
    content = [zlib.decompress(_stream(v)) for v in _objects(pdf).values() if b"/FlateDecode" in v and b"/Length" in v]
    assert any(c.startswith(b"q 64 0 0 32 0 0 cm /Im1 Do Q\nq 64 0 0 32 0 0 cm /Im0 Do Q\n") for c in content)


def test_a_document_that_mixes_the_entry_kinds():
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    plain = _jpeg(30, 20, False, b"PLAIN")
    bilevel = SimpleNamespace(data=b"G4", width=30, height=20, scale=1.0, bilevel=True)
    array = np.full((20, 30, 3), 200, np.uint8)
    pdf = searchable_pdf_bytes([plain, bilevel, _mrc(), array, _mrc(33, 65)], [_doc()] * 5)
    assert pdf.count(b"/Filter /DCTDecode") == 1 + 2 + 1 + 2
    assert pdf.count(b"/Filter /CCITTFaxDecode") == 1 + 1 + 1
    assert pdf.count(b"/ImageMask true") == 2 and len(re.findall(rb"/Mask \d+ 0 R", pdf)) == 2
    assert pdf.count(b"/Type /Page ") == 5
    # an object that only says `mrc` is not taken for one
    with pytest.raises(Exception):
        searchable_pdf_bytes([SimpleNamespace(mrc=True)], [_doc()])


def test_encoded_mrc_is_what_the_writer_recognises():
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import EncodedJpeg
    from yomitoku_amd.mrc import EncodedMrc
    from yomitoku_amd.utils.searchable_pdf import _is_bilevel, _is_encoded, _is_mrc

    entry = EncodedMrc(EncodedBilevel(b"abc", 70, 45, 1.0, "adaptive"), EncodedJpeg(b"12345", 35, 23, False), EncodedJpeg(b"67", 9, 6, False), 70, 45)
    assert _is_mrc(entry) and not _is_bilevel(entry) and not _is_encoded(entry)
    assert (entry.mrc, entry.scale, entry.bg_cell, entry.fg_cell, entry.nbytes) == (True, 1.0, 2, 8, 10)
    assert not _is_mrc(entry.mask) and not _is_mrc(entry.background)
