"""Host checks of the JPEG encoder's per-page modes (no GPU): the definition tests/jpeg_modes_ref.py against Pillow, the
library's mode-taking host entries against the definition, the PDF writer's handling of such files, and the validation of the
new arguments.

The device encoder (tests/test_jpeg_modes_gpu.py) must equal the definition byte for byte, so what is shown here of the
definition's files holds for the device's."""
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image, JpegImagePlugin

from tests import jpeg_modes_ref, jpeg_opt_ref, jpeg_ref
from tests.test_jpeg_host import _doc, _image_streams, decoded, pillow_jpeg, synthetic_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 8), (8, 16), (16, 16), (16, 32), (32, 48), (24, 40), (37, 53), (37, 48), (5, 16), (13, 64), (37, 56), (9, 8)]  # (h, w)
PILLOW_ID = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


@pytest.fixture(scope="module")
def golden():
    page = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_page.jpg")).convert("RGB"))[:, :, ::-1]
    return np.ascontiguousarray(page)


def _pages(golden, h, w):
    """Noise, and a crop of the golden page from a place with print on it."""
    y0, x0 = min(200, golden.shape[0] - h), min(120, golden.shape[1] - w)
    return [np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8), np.ascontiguousarray(golden[y0 : y0 + h, x0 : x0 + w])]


def _equals_pillow(subsampling, w):
    """Where the definition's file IS Pillow's: 4:4:4 everywhere, 4:2:2 where the luminance has an even number of block columns."""
    return subsampling == "4:4:4" or (subsampling == "4:2:2" and (-(-w // 8)) % 2 == 0)


@pytest.mark.parametrize("subsampling", ["4:4:4", "4:2:2"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_definition_against_pillow(golden, size, subsampling):
    h, w = size
    for quality in (85, 50):
        for page in _pages(golden, h, w):
            mine = jpeg_modes_ref.encode(page, quality, subsampling)
            if _equals_pillow(subsampling, w):
                assert mine == pillow_jpeg(page, quality, subsampling=subsampling, restart_marker_rows=1), (size, quality)
            image, _ = decoded(mine)
            assert image.size == (w, h) and image.mode == "RGB" and image.format == "JPEG"
            assert JpegImagePlugin.get_sampling(image) == PILLOW_ID[subsampling]


@pytest.mark.parametrize("size", SIZES + [(40, 200), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_420_of_the_generalised_definition_is_jpeg_refs(golden, size):
    for page in _pages(golden, *size):
        assert np.array_equal(jpeg_modes_ref.coefficients(page, 85, "4:2:0"), jpeg_ref.coefficients(page, 85))
        assert jpeg_modes_ref.encode(page, 85, "4:2:0") == jpeg_ref.encode(page, 85)
        assert jpeg_modes_ref.encode(page, 50, "4:2:0", optimize=True) == jpeg_opt_ref.encode(page, 50)
    image, _ = decoded(jpeg_modes_ref.encode(page, 85, "4:2:0"))
    assert JpegImagePlugin.get_sampling(image) == 2


@pytest.mark.parametrize("size", [(8, 8), (37, 53), (24, 40), (13, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_grey_file_of_a_grey_valued_colour_page(golden, size):
    """B == G == R everywhere: the file is jpeg_ref's of the plane, which is Pillow's save of convert("L") - its L weights sum to
    65536, so L of a grey pixel is the pixel."""
    for src in _pages(golden, *size):
        plane = np.ascontiguousarray(src[..., 1])
        page = np.stack([plane, plane, plane], -1)
        assert jpeg_modes_ref.is_grey(page) and not jpeg_modes_ref.is_grey(src)
        for quality in (85, 50):
            mine = jpeg_modes_ref.encode(page, quality, "4:4:4", grey="auto")
            assert mine == jpeg_ref.encode(plane, quality)
            lum = Image.fromarray(np.ascontiguousarray(page[:, :, ::-1])).convert("L")
            assert np.array_equal(np.asarray(lum), plane)
            out = io.BytesIO()
            lum.save(out, "JPEG", quality=quality, restart_marker_rows=1)
            assert mine == out.getvalue()
            assert jpeg_modes_ref.encode(page, quality, "4:4:4", grey="auto", optimize=True) == jpeg_opt_ref.encode(plane, quality)
        # without grey="auto" the page stays a colour file, and a colour page is never a grey one
        assert decoded(jpeg_modes_ref.encode(page, 85, "4:4:4"))[0].mode == "RGB"
        assert jpeg_modes_ref.encode(src, 85, "4:2:2", grey="auto") == jpeg_modes_ref.encode(src, 85, "4:2:2")


@pytest.mark.parametrize("subsampling", ["4:4:4", "4:2:2"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_optimised_tables_against_pillows_optimize(golden, size, subsampling):
    """jpeg_opt_ref's rule on this mode's blocks: Pillow's `optimize=True` file wherever the plain file is Pillow's; everywhere the
    same pixels as the plain file, and no more bytes."""
    h, w = size
    for quality in (85, 50):
        for page in _pages(golden, h, w):
            mine = jpeg_modes_ref.encode(page, quality, subsampling, optimize=True)
            plain = jpeg_modes_ref.encode(page, quality, subsampling)
            if _equals_pillow(subsampling, w):
                assert mine == pillow_jpeg(page, quality, subsampling=subsampling, restart_marker_rows=1, optimize=True), (size, quality)
            assert np.array_equal(decoded(mine)[1], decoded(plain)[1]) and len(mine) <= len(plain)


# ------------------------------------------------------------------------------------------------ the library's host entries
MODES = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2}


@pytest.mark.parametrize("subsampling", ["4:2:0", "4:2:2", "4:4:4"])
def test_the_librarys_headers_and_sizes_are_the_definitions(subsampling):
    from yomitoku_amd import _lib
    from yomitoku_amd.jpeg import MODE_GREY, SUBSAMPLINGS, _geometry, _header, _header_opt, scratch_sizes

    assert SUBSAMPLINGS == MODES
    mode = MODES[subsampling]
    hs, vs = jpeg_modes_ref.SAMPLING[subsampling]
    shapes = [(1, 1, 3), (8, 8, 3), (9, 23, 3), (37, 53, 3), (40, 200, 3), (16383, 16383, 3)]
    for h, w, _ in shapes:
        want = jpeg_modes_ref.header(h, w, 85, subsampling)
        assert _header(h, w, 3, 85, mode) == want
        stripped, split = _header_opt(h, w, 3, 85, mode)
        first = want.index(b"\xff\xc4")
        assert stripped == want[:first] + want[want.index(b"\xff\xdd\x00\x04") :] and split == first
        assert _header(h, w, 3, 85, MODE_GREY) == jpeg_ref.header(h, w, True, 85)
    assert _header(40, 200, 3, 85, 0) == _header(40, 200, 3, 85) == jpeg_ref.header(40, 200, False, 85)
    sized = scratch_sizes(shapes, modes=[mode] * len(shapes))
    mcus = [(-(-w // (8 * hs))) * (-(-h // (8 * vs))) for h, w, _ in shapes]
    assert sized[1] == sum(m * (hs * vs + 2) for m in mcus) and sized[2] == sum(-(-h // (8 * vs)) for h, _, _ in shapes)
    assert sized[0] == sum((-(-w // 16)) * (-(-h // 16)) for h, w, _ in shapes)  # 16 x 16 tiles in every colour mode
    assert sized[:3] == tuple(sum(v) for v in zip(*[_geometry(h, w, 3, mode) for h, w, _ in shapes]))
    assert sized[3:] == (sized[1] * 128, sized[1] * 208, sized[2] * 8)
    # the grey file of a three-channel page: a one-channel page's blocks and intervals, a colour page's tiles
    assert scratch_sizes(shapes, modes=[MODE_GREY] * len(shapes)) == sized[:1] + scratch_sizes([(h, w, 1) for h, w, _ in shapes])[1:]
    assert scratch_sizes(shapes, modes=[0] * len(shapes)) == scratch_sizes(shapes)
    assert scratch_sizes(shapes, True, [mode] * len(shapes))[:4] == sized[:4]
    # an unknown mode, a mode on a one-channel page: refused
    lib = _lib.load()
    buf = (__import__("ctypes").c_ubyte * 1024)()
    for channels, bad in ((3, 3), (3, 5), (3, -1), (1, 1), (1, 4)):
        assert lib.ymk_jpeg_header_mode(16, 16, channels, bad, 85, buf, 1024) == -1 and lib.ymk_last_error()
        with pytest.raises(_lib.YmkError):
            scratch_sizes([(16, 16, channels)], modes=[bad])


# ------------------------------------------------------------------------------------------------ the arguments
def _no_sources():
    raise AssertionError("a source was read")
    yield


BAD = [dict(jpeg="high", jpeg_subsampling="4:1:1"), dict(jpeg="high", jpeg_subsampling=0), dict(jpeg="high", jpeg_grey=True),
       dict(jpeg="high", jpeg_grey="always"), dict(jpeg_subsampling="4:4:4"), dict(jpeg_grey="auto"), dict(jpeg_subsampling="4:2:0")]


@pytest.mark.parametrize("kwargs", BAD, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_bad_values_are_refused_before_a_source_is_read(kwargs):
    from tests.test_serving import StubAnalyzer
    from yomitoku_amd.document_analyzer import OCR, DocumentAnalyzer
    from yomitoku_amd.serving import PagePipeline, check_jpeg_preset

    for cls in (DocumentAnalyzer, OCR):
        with pytest.raises(ValueError, match="jpeg"):
            cls.serve(SimpleNamespace(visualize=False), _no_sources(), **kwargs)
    pipe = PagePipeline(StubAnalyzer(), wave=2, in_flight=1)
    try:
        with pytest.raises(ValueError, match="jpeg"):
            pipe.serve(_no_sources(), files=check_jpeg_preset(**{"jpeg": None, **kwargs}))
    finally:
        pipe.close()


def test_encode_jpeg_pages_refuses_bad_values_before_any_device_work(monkeypatch):
    import torch

    from yomitoku_amd import jpeg

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    page = np.zeros((8, 8, 3), np.uint8)
    for kwargs in (dict(subsampling="4:1:1"), dict(subsampling=None), dict(subsampling=2), dict(grey=True), dict(grey="yes")):
        with pytest.raises(ValueError, match="jpeg"):
            jpeg.encode_jpeg_pages([page], "high", **kwargs)
        with pytest.raises(ValueError, match="jpeg"):
            jpeg.encode_jpeg(page, "high", **kwargs)
    assert jpeg.check_modes() == 0 and jpeg.check_modes("4:4:4", "auto") == 2


def test_the_options_travel_on_the_job_to_the_jpeg_stage():
    from tests.test_serving import StubAnalyzer, page
    from yomitoku_amd.serving import PagePipeline, check_jpeg_preset

    seen = []

    class Stub(StubAnalyzer):
        def _stage_jpeg(self, wave, results):
            seen.append((wave.job.files.preset, wave.job.files.optimize, wave.job.files.subsampling, wave.job.files.grey))
            return [(("file", wave.ids[k]),) for k in range(len(results))]

    pipe = PagePipeline(Stub(), wave=4, in_flight=2)
    try:
        out = pipe.serve([page(i) for i in range(3)], files=check_jpeg_preset("low", jpeg_subsampling="4:4:4", jpeg_grey="auto"))
        assert [o[1] for o in out] == [("file", i) for i in range(3)]
        pipe.serve([page(0)], files=check_jpeg_preset("low"))
    finally:
        pipe.close()
    assert seen == [("low", False, "4:4:4", "auto"), ("low", False, "4:2:0", False)]


def test_encoded_jpeg_says_its_subsampling():
    from yomitoku_amd.jpeg import EncodedJpeg

    assert EncodedJpeg(b"x", 1, 1, False).subsampling == "4:2:0"
    assert EncodedJpeg(b"x", 1, 1, True, 1.0, False, None).subsampling is None


# ------------------------------------------------------------------------------------------------ the PDF writer
def test_pdf_embeds_a_444_file_and_an_auto_grey_file():
    """The writer takes the colour space from EncodedJpeg.grey: a 4:4:4 file is /DeviceRGB, the grey file of a grey-valued colour
    page /DeviceGray, both embedded as they are."""
    from yomitoku_amd.jpeg import EncodedJpeg
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    colour = synthetic_page(120, 400, seed=2)
    plane = synthetic_page(120, 400, seed=3, grey=True)
    flat = np.stack([plane, plane, plane], -1)
    a = EncodedJpeg(jpeg_modes_ref.encode(colour, 85, "4:4:4", grey="auto"), 400, 120, False, 1.0, False, "4:4:4")
    b = EncodedJpeg(jpeg_modes_ref.encode(flat, 85, "4:4:4", grey="auto"), 400, 120, True, 1.0, False, None)
    pdf = searchable_pdf_bytes([a, b], [_doc(), _doc()], image_quality="high")
    streams = _image_streams(pdf)
    assert [(s[0], s[1], s[2]) for s in streams] == [(400, 120, "DeviceRGB"), (400, 120, "DeviceGray")]
    assert streams[0][3] == a.data and streams[1][3] == b.data
    assert [decoded(s[3])[0].mode for s in streams] == ["RGB", "L"]
