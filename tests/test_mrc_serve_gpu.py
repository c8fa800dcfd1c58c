"""DocumentAnalyzer.serve / OCR.serve(jpeg=..., jpeg_mrc=True): a page with ink and paper ends with its EncodedMrc - the Group 4
file of its ink mask and the JPEG files of its two layers, each byte for byte what the definition (tests/mrc_ref.py) and the
unchanged encoders give -, a blank page with the JPEG file it gets without the switch, and the schemas and overlays are those of
the job without it: the networks see the page as it arrived.  The analyzers and their seeded weights are those of
tests/test_serving_gpu.py and tests/test_ocr_serve_gpu.py."""
import numpy as np
import pytest

from tests import ccitt_ref, deskew_ref
from tests import mrc_ref as R
from tests.test_serving_gpu import _analyzer

pytestmark = pytest.mark.gpu

COLOUR, GREY, TWO_VALUED, BLANK = 0, 1, 2, 3


@pytest.fixture(scope="module")
def analyzer(dev):
    an = _analyzer()
    yield an
    an.close()


@pytest.fixture(scope="module")
def ocr(dev):
    from tests.test_ocr_serve_gpu import _ocr

    an = _ocr()
    yield an
    an.close()


@pytest.fixture(scope="module")
def pages():
    """Four small pages as load_image hands them over, B G R: a colour page, a grey-valued scan, a 1-bit scan, a blank page."""
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    out = [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate([(600, 640), (640, 600), (500, 700)])]
    g = out[GREY][..., 1]
    out[GREY] = np.ascontiguousarray(np.stack([g] * 3, -1))
    v = np.where(out[TWO_VALUED][..., 1] < 128, 0, 255).astype(np.uint8)
    out[TWO_VALUED] = np.ascontiguousarray(np.stack([v] * 3, -1))
    out.append(np.full((300, 333, 3), 255, np.uint8))
    assert [ccitt_ref.is_bilevel(p) for p in out] == [False, False, True, True]
    return out


@pytest.fixture(scope="module")
def separated(pages):
    """per page (flag, M, foreground, background) by the definition, and the mask's Group 4 file - computed once"""
    out = [R.separate(p) for p in pages]
    assert [s[0] for s in out] == [1, 1, 1, 0]
    return out, [R.mask_file(s[1]) if s[0] else None for s in out]


def _layer_files(layers, quality="high", **how):
    """the files `encode_jpeg_pages` writes for layers handed in as pages, at the capacity a layer gets"""
    from yomitoku_amd.jpeg import encode_jpeg_pages

    return encode_jpeg_pages(list(layers), quality, capacities=[a.size + 2048 for a in layers], **how)


def _check_layered(entry, page, want, mask_file, cells=(2, 8), quality="high", **how):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import EncodedJpeg
    from yomitoku_amd.mrc import EncodedMrc

    _, M, fg, bg = want
    assert isinstance(entry, EncodedMrc) and entry.mrc is True
    assert (entry.width, entry.height, entry.scale, entry.bg_cell, entry.fg_cell) == (page.shape[1], page.shape[0], 1.0, *cells)
    assert isinstance(entry.mask, EncodedBilevel) and entry.mask.data == mask_file
    assert (entry.mask.width, entry.mask.height, entry.mask.scale, entry.mask.method, entry.mask.threshold) == (page.shape[1], page.shape[0], 1.0, "adaptive", None)
    fore, back = _layer_files([fg, bg], quality, **how)
    assert isinstance(entry.foreground, EncodedJpeg) and entry.foreground == fore and entry.foreground.data == fore.data
    assert isinstance(entry.background, EncodedJpeg) and entry.background == back and entry.background.data == back.data
    assert (entry.foreground.width, entry.foreground.height) == (fg.shape[1], fg.shape[0]) and entry.foreground.grey == (fg.ndim == 2)
    assert entry.nbytes == len(mask_file) + len(fore.data) + len(back.data)


@pytest.mark.parametrize("which", ["analyzer", "ocr"])
def test_serve_gives_layered_pages_next_to_the_plain_files(which, pages, separated, request):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import EncodedJpeg
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    an = request.getfixturevalue(which)
    want, mask_files = separated
    base = an.serve(pages, wave=2, jpeg="high")
    got = an.serve(pages, wave=2, jpeg="high", jpeg_mrc=True)
    assert len(got) == len(base) == 4
    for k, (entry, plain) in enumerate(zip(got, base)):
        assert isinstance(entry, tuple) and len(entry) == 2
        assert entry[0].model_dump() == plain[0].model_dump()
        if k == BLANK:  # no ink: the file of the job without the switch
            assert isinstance(entry[1], EncodedJpeg) and entry[1] == plain[1] and entry[1].data == plain[1].data
        else:
            _check_layered(entry[1], pages[k], want[k], mask_files[k])
    assert sum(e[1].nbytes for e in got[:BLANK]) < sum(len(e[1].data) for e in base[:BLANK])  # what it is for
    pdf = searchable_pdf_bytes([e[1] for e in got], [e[0] for e in got])
    assert pdf.count(b"/Filter /CCITTFaxDecode") == 3 and pdf.count(b"/ImageMask true") == 3 and pdf.count(b"/Filter /DCTDecode") == 7
    # `jpeg_bilevel` decides first: the 1-bit scan - and the blank page - get their Group 4 files, the others are layered as before
    both = an.serve(pages, wave=2, jpeg="high", jpeg_bilevel="auto", jpeg_mrc=True)
    two = an.serve(pages[TWO_VALUED:], wave=2, jpeg="high", jpeg_bilevel="auto")
    for k in (TWO_VALUED, BLANK):
        assert isinstance(both[k][1], EncodedBilevel) and both[k][1] == two[k - TWO_VALUED][1] and both[k][1].method == "auto"
    for k in (COLOUR, GREY):
        assert both[k][1] == got[k][1] and both[k][0].model_dump() == base[k][0].model_dump()
    pdf = searchable_pdf_bytes([e[1] for e in both], [e[0] for e in both])
    assert pdf.count(b"/Filter /CCITTFaxDecode") == 4 and pdf.count(b"/ImageMask true") == 2 and pdf.count(b"/Filter /DCTDecode") == 4
    # the switch belongs to the job: the next one is plain again, byte for byte
    after = an.serve(pages, wave=2, jpeg="high")
    assert [e[1] for e in after] == [e[1] for e in base] and [e[1].data for e in after] == [e[1].data for e in base]


@pytest.mark.parametrize("which", ["analyzer", "ocr"])
def test_overlays_are_those_of_the_job_without_the_switch(which, pages, request):
    an = request.getfixturevalue(which)
    base = an.serve(pages, wave=2, overlays=True, jpeg="high")
    got = an.serve(pages, wave=2, overlays=True, jpeg="high", jpeg_mrc={"bg_cell": 4, "fg_cell": 16})
    for entry, plain in zip(got, base):
        assert len(entry) == len(plain) >= 3
        assert entry[0].model_dump() == plain[0].model_dump()
        assert all(np.array_equal(a, b) for a, b in zip(entry[1:-1], plain[1:-1]))
    assert [getattr(e[-1], "mrc", False) for e in got] == [True, True, True, False]
    assert [(e[-1].bg_cell, e[-1].fg_cell) for e in got[:BLANK]] == [(4, 16)] * 3


def test_other_cells_and_the_encoders_options_apply_to_the_layers(dev, pages, separated):
    """the stand-alone entry: cells of a call's own; `optimize` and `subsampling` reach the two layer files, `grey` does not - the
    grey-valued page's layers keep three channels -, and a preset that would shrink the page leaves a layered page at full size"""
    from yomitoku_amd.jpeg import encode_jpeg_pages
    from yomitoku_amd.mrc import encode_mrc_pages

    want, mask_files = separated
    job = [pages[COLOUR], pages[GREY][..., 0].copy(), pages[BLANK]]
    got = encode_mrc_pages(job, "high", {"bg_cell": 1, "fg_cell": 4}, optimize=True, subsampling="4:4:4")
    plain = encode_jpeg_pages(job, "high", optimize=True, subsampling="4:4:4")
    for k in range(2):  # the masks do not depend on the cells, and the one-channel page is its own luminance
        _check_layered(got[k], job[k], R.separate(job[k], 1, 4), mask_files[k], (1, 4), optimize=True, subsampling="4:4:4")
    assert got[0].foreground.subsampling == "4:4:4" and got[0].foreground.optimized
    assert got[1].foreground.grey and got[1].background.grey  # a one-channel page: one-channel layers
    assert got[2] == plain[2]
    greyed = encode_jpeg_pages([pages[GREY], pages[BLANK]], "high", grey="auto", mrc=True)
    _check_layered(greyed[0], pages[GREY], want[GREY], mask_files[GREY])
    assert greyed[1] == encode_jpeg_pages([pages[BLANK]], "high", grey="auto")[0] and greyed[1].grey
    strip = np.ascontiguousarray(np.tile(pages[COLOUR][200:248], (1, 3, 1)))  # 48 x 1920: "low" shrinks a page beyond 1500
    small = encode_jpeg_pages([strip, np.full((8, 1600, 3), 255, np.uint8)], "low", mrc=True)
    sep = R.separate(strip)
    assert sep[0] == 1 and small[0].scale == 1.0 and small[1].scale == 1500 / 1600 and small[1].width == 1500
    _check_layered(small[0], strip, sep, R.mask_file(sep[1]), quality="low")


def test_with_deskew_the_layers_are_those_of_the_corrected_page(ocr, pages):
    from PIL import Image

    from yomitoku_amd.deskew import PageSkew

    turned = np.ascontiguousarray(np.asarray(Image.fromarray(pages[COLOUR]).rotate(-2, Image.BICUBIC, fillcolor=(255, 255, 255))))
    fixed, k = deskew_ref.deskew(turned)[:2]
    assert k != 0
    got = ocr.serve([turned], wave=2, jpeg="high", jpeg_mrc=True, deskew=True)
    assert len(got[0]) == 3 and isinstance(got[0][2], PageSkew) and got[0][2].index == k
    want = R.separate(fixed)
    assert want[0] == 1
    _check_layered(got[0][1], fixed, want, R.mask_file(want[1]))


def test_the_switch_is_refused_without_jpeg_before_a_source_is_read(analyzer, ocr):
    def sources():
        raise AssertionError("a source was read")
        yield

    for an in (analyzer, ocr):
        with pytest.raises(ValueError, match="jpeg_mrc"):
            an.serve(sources(), wave=2, jpeg_mrc=True)
        for bad in ("auto", 1, {"bg_cell": 3}, {"cells": 2}):
            with pytest.raises(ValueError, match="mrc"):
                an.serve(sources(), wave=2, jpeg="high", jpeg_mrc=bad)
