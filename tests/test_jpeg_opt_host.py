"""Host checks of the optimised Huffman tables (no GPU): the definition tests/jpeg_opt_ref.py against Pillow's `optimize=True`,
its table rule on crafted histograms, and the PDF writer's handling of such a file.

The device (tests/test_jpeg_opt_gpu.py) must equal the definition byte for byte, so what holds for the definition's files here
holds for the device's."""
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_opt_ref, jpeg_ref
from tests.test_jpeg_host import _doc, _image_streams, decoded, pillow_jpeg, synthetic_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_crop(h, w):
    page = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_page.jpg")).convert("RGB"))[:, :, ::-1]
    return np.ascontiguousarray(page[200 : 200 + h, 100 : 100 + w])


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


PAGES = {
    "flat_16x16": lambda: np.full((16, 16, 3), 128, np.uint8),
    "noise_32x48": lambda: noise((32, 48, 3), 1),
    "page_48x208": lambda: synthetic_page(48, 208, seed=2),
    "golden_160x256": lambda: golden_crop(160, 256),
    "grey_flat_8x8": lambda: np.full((8, 8), 77, np.uint8),
    "grey_64x128": lambda: synthetic_page(64, 128, seed=3, grey=True),
}


@pytest.mark.parametrize("quality", [85, 80, 60])
@pytest.mark.parametrize("name", list(PAGES))
def test_the_definition_equals_pillows_optimised_save(name, quality):
    """Required wherever the plain definition equals Pillow's plain save of the same page; where that does not hold (another
    libjpeg build) the case is skipped with that reason.  With Pillow 12.2 (libjpeg-turbo) no case is skipped."""
    page = PAGES[name]()
    if jpeg_ref.encode(page, quality) != pillow_jpeg(page, quality, restart_marker_rows=1):
        pytest.skip("this Pillow's plain save differs from tests/jpeg_ref.py for this page: nothing to compare the tables on")
    mine = jpeg_opt_ref.encode(page, quality)
    assert mine == pillow_jpeg(page, quality, optimize=True, restart_marker_rows=1)
    assert len(mine) < len(jpeg_ref.encode(page, quality))


@pytest.mark.parametrize("shape", [(16, 16, 3), (32, 48, 3), (33, 17, 3), (40, 200, 3), (9, 23), (64, 128)], ids=str)
def test_the_optimised_file_decodes_to_the_plain_files_pixels(shape):
    for quality, page in ((85, synthetic_page(shape[0], shape[1], seed=4, grey=len(shape) == 2)), (60, noise(shape, 5))):
        a, b = decoded(jpeg_opt_ref.encode(page, quality)), decoded(jpeg_ref.encode(page, quality))
        assert a[0].size == b[0].size == (shape[1], shape[0]) and a[0].mode == b[0].mode
        assert np.array_equal(a[1], b[1])


def crafted_histograms():
    """name -> frequencies: what the table rule must get right besides real pages."""
    deep = np.zeros(256, np.int64)
    deep[np.arange(18) * 7 + 3] = 3 ** np.arange(18)  # 18 symbols, each three times the one before: a chain 18 deep
    one = np.zeros(256, np.int64)
    one[0x21] = 12345
    two = np.zeros(256, np.int64)
    two[[0x00, 0xF0]] = (5, 5)
    return {"powers_of_three": deep, "all_256_once": np.ones(256, np.int64), "one_symbol": one, "two_symbols": two}


def check_table(freq, bits, vals):
    """The code is complete but for ONE code of the longest length in use - the reserved all-ones code: in units of 2^-16 the
    Kraft sum is 2^16 - 2^(16 - longest), which is 2^16 - 1 where the longest code has 16 bits.  Nothing is over 16 bits."""
    present = [s for s in range(len(freq)) if freq[s]]
    assert len(bits) == 16 and sum(bits) == len(vals) and sorted(vals) == present
    longest = max(length for length, n in enumerate(bits, 1) if n)
    assert sum(n << (16 - length) for length, n in enumerate(bits, 1)) == (1 << 16) - (1 << (16 - longest))
    codes = jpeg_ref.huffman_codes((bits, vals))
    assert max(length for _, length in codes.values()) <= 16
    return codes


@pytest.mark.parametrize("name", list(crafted_histograms()))
def test_the_table_rule_on_crafted_histograms(name):
    freq = crafted_histograms()[name]
    bits, vals = jpeg_opt_ref.optimal_table(freq)
    codes = check_table(freq, bits, vals)
    size = jpeg_opt_ref.code_sizes(freq)
    lengths = [codes[s][1] for s in vals]
    # by (length, value): libjpeg sorts by the length BEFORE limiting, which is the code's length wherever nothing was limited
    assert lengths == sorted(lengths) and vals == sorted(vals, key=lambda s: (size[s], s))
    if name == "powers_of_three":
        assert max(size) > 16 and vals[0] == 17 * 7 + 3  # Figure K.3's loop really runs
        assert bits[15] > 0 and sum(n << (16 - length) for length, n in enumerate(bits, 1)) == (1 << 16) - 1
    else:
        assert max(size) <= 16 and vals == sorted(vals, key=lambda s: (codes[s][1], s))
    if name == "all_256_once":
        assert bits[7] == 255 and bits[8] == 1 and sum(bits) == 256
    if name == "one_symbol":
        assert codes == {0x21: (0, 1)}
    if name == "two_symbols":
        assert sorted(length for _, length in codes.values()) == [1, 2]
    assert jpeg_opt_ref.optimal_table(np.zeros(256, np.int64)) == ([0] * 16, [])


def test_histograms_count_what_the_interval_coder_emits():
    """The bits of the scan are the histograms' counts times the code lengths plus the magnitude bits: checked through the
    file's length with Annex K's tables, whose lengths are known."""
    page = synthetic_page(40, 200, seed=6)
    coefs = jpeg_ref.coefficients(page, 85)
    dc, ac = jpeg_opt_ref.histograms(coefs, 40, 200, False)
    assert dc.sum() == len(coefs) and dc[0].sum() == 4 * 13 * 3 and ac[:, 0].sum() <= len(coefs)
    tables = [(0x00, jpeg_ref.DC_LUMA), (0x10, jpeg_ref.AC_LUMA), (0x01, jpeg_ref.DC_CHROMA), (0x11, jpeg_ref.AC_CHROMA)]
    assert jpeg_opt_ref.assemble(coefs, 40, 200, False, 85, tables) == jpeg_ref.assemble(coefs, 40, 200, False, 85)


def test_pdf_embeds_an_optimised_jpeg_as_it_is():
    from yomitoku_amd.jpeg import EncodedJpeg
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    page = synthetic_page(120, 400, seed=2)
    data = jpeg_opt_ref.encode(page, 85)
    entry = EncodedJpeg(data, 400, 120, False, 1.0, True)
    assert entry.optimized and not EncodedJpeg(data, 400, 120, False).optimized
    pdf = searchable_pdf_bytes([entry, SimpleNamespace(data=data, width=400, height=120, grey=False, scale=1.0)], [_doc(), _doc()], "high")
    streams = _image_streams(pdf)
    assert [(s[0], s[1], s[2]) for s in streams] == [(400, 120, "DeviceRGB")] * 2 and streams[0][3] == data == streams[1][3]
    image = Image.open(io.BytesIO(streams[0][3]))
    image.load()
    assert image.size == (400, 120)


def test_the_host_entries_of_the_optimised_path():
    """No device needed: the header without DHT segments is the definition's two parts, and the scratch sizes are the plain
    ones but for the stream's reservation and the three new buffers."""
    from yomitoku_amd.jpeg import _header, _header_opt, scratch_sizes

    for h, w, ch in ((33, 17, 3), (9, 23, 1), (16383, 1, 3)):
        part, split = _header_opt(h, w, ch, 85)
        plain = jpeg_ref.header(h, w, ch == 1, 85)
        assert plain == _header(h, w, ch, 85)
        tables = [(0x00, jpeg_ref.DC_LUMA), (0x10, jpeg_ref.AC_LUMA)] + ([] if ch == 1 else [(0x01, jpeg_ref.DC_CHROMA), (0x11, jpeg_ref.AC_CHROMA)])
        assert part[:split] + jpeg_opt_ref.dht_segments(tables) + part[split:] == plain
        assert jpeg_opt_ref.header(h, w, ch == 1, 85, []) == part
    shapes = [(1, 1, 3), (40, 200, 3), (9, 23, 1)]
    plain, opt = scratch_sizes(shapes), scratch_sizes(shapes, optimize=True)
    assert len(plain) == 6 and len(opt) == 9 and opt[:4] == plain[:4] and opt[5] == plain[5]
    assert plain[4] == 208 * plain[1] and opt[4] == 212 * opt[1] and 212 * 8 >= 16 + 11 + 63 * 26 > 208 * 8
    assert opt[6:] == (3 * 544 * 4, 3 * 544 * 4, 3 * 656)


def test_jpeg_optimize_without_jpeg_is_refused_before_a_page_is_read():
    from tests.test_serving import StubAnalyzer
    from yomitoku_amd.document_analyzer import DocumentAnalyzer
    from yomitoku_amd.serving import PagePipeline, check_jpeg_preset

    def sources():
        raise AssertionError("a source was read")
        yield

    with pytest.raises(ValueError, match="jpeg_optimize"):
        DocumentAnalyzer.serve(SimpleNamespace(visualize=False), sources(), jpeg_optimize=True)
    pipe = PagePipeline(StubAnalyzer(), wave=2, in_flight=1)
    try:
        with pytest.raises(ValueError, match="jpeg_optimize"):
            pipe.serve(sources(), files=check_jpeg_preset(None, jpeg_optimize=True))
    finally:
        pipe.close()
