"""The Group 4 definition (tests/ccitt_ref.py) against libtiff's strips - recorded (tests/golden/ccitt_g4_cases.npz, written by
tools/record_ccitt_cases.py through Pillow) and, where Pillow has libtiff, live -, the row-slot bound of the device encoder,
the PDF writer's handling of an EncodedBilevel, and the refusals of serve(jpeg_bilevel=...).  No GPU."""
import io
import itertools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image, features

from tests import ccitt_ref
from tests.test_jpeg_host import _doc, _image_streams, _objects, _text_matrices, synthetic_page
from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ccitt_g4_cases.npz")


def golden_cases():
    """name -> (the page as H x W bool, True = black; libtiff's strip)."""
    z = np.load(GOLDEN)
    out = {}
    for key in z.files:
        if key.endswith(".shape"):
            name = key[: -len(".shape")]
            h, w = (int(v) for v in z[key])
            out[name] = (np.unpackbits(z[name + ".bits"], axis=1)[:, :w].astype(bool).reshape(h, w), z[name + ".strip"].tobytes())
    return out


CASES = golden_cases()
FAMILIES = ["noise_1x1", "noise_1x7", "noise_2x31", "noise_3x32", "noise_3x33", "noise_2x63", "noise_5x64", "noise_4x65", "noise_9x100",
            "noise_40x300_05", "noise_40x300_50", "noise_40x300_95", "white_70x33", "black_70x33", "drift", "long_3x2700", "long_2x5300",
            "golden_crop", "terminating", "white_run_0", "black_run_0"]


def test_the_fixture_holds_the_case_families():
    assert set(FAMILIES) <= set(CASES) and sum(name.startswith("makeup_") for name in CASES) >= 14
    assert CASES["golden_crop"][0].shape == (300, 400) and CASES["long_2x5300"][0].shape == (2, 5300)


@pytest.mark.parametrize("name", sorted(CASES))
def test_definition_equals_the_recorded_libtiff_strip(name):
    black, strip = CASES[name]
    assert ccitt_ref.encode_g4(black) == strip


def test_the_two_row_cases_use_every_code_of_both_colours():
    """The horizontal-mode runs of the recorded cases, which the definition reproduces byte for byte: every terminating code and
    every make-up code - 64 ... 1728 of each colour, 1792 ... 2560 of both - is among their codes."""
    used = {False: set(), True: set()}
    for black, _ in CASES.values():
        above = np.zeros(black.shape[1], bool)
        for row in black:
            for step in ccitt_ref.row_steps(row, above):
                if step[0] == "horizontal":
                    used[step[3]] |= set(ccitt_ref.run_codes(step[1], step[3]))
                    used[not step[3]] |= set(ccitt_ref.run_codes(step[2], not step[3]))
            above = row
    assert set(ccitt_ref.WHITE_TERM + ccitt_ref.WHITE_MAKEUP + ccitt_ref.EXTENDED_MAKEUP) <= used[False]
    assert set(ccitt_ref.BLACK_TERM + ccitt_ref.BLACK_MAKEUP + ccitt_ref.EXTENDED_MAKEUP) <= used[True]


def test_the_drift_case_uses_every_mode():
    black, _ = CASES["drift"]
    seen, above = set(), np.zeros(black.shape[1], bool)
    for row in black:
        seen |= set(ccitt_ref.row_codes(row, above))
        above = row
    assert set(ccitt_ref.VERTICAL.values()) | {ccitt_ref.PASS, ccitt_ref.HORIZONTAL} <= seen


def _libtiff_strip(black):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(black, dtype=bool)).save(buf, "TIFF", compression="group4", tiffinfo={278: black.shape[0]})
    buf.seek(0)
    tags = Image.open(buf).tag_v2
    (at,), (n,) = tags[273], tags[279]
    return buf.getvalue()[at : at + n]


@pytest.mark.skipif(not features.check("libtiff"), reason="Pillow without libtiff: nothing to compare against live")
def test_definition_equals_libtiff_live_and_the_tiff_wrapper_opens():
    rng = np.random.default_rng()
    for _ in range(12):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 400))
        black = rng.random((h, w)) < rng.random()
        if rng.random() < 0.5:  # runs, not noise: vertical and pass modes
            black = np.repeat(np.repeat(black[: -(-h // 3), : -(-w // 5)], 3, axis=0), 5, axis=1)[:h, :w]
        data = ccitt_ref.encode_g4(black)
        assert data == _libtiff_strip(black), (h, w)
        image = Image.open(io.BytesIO(ccitt_ref.to_tiff(data, w, h)))
        image.load()
        assert image.size == (w, h) and np.array_equal(np.asarray(image.convert("L")) == 0, black)


def test_is_bilevel_and_the_packed_rows():
    page = np.where(np.random.default_rng(1).random((5, 70)) < 0.3, 0, 255).astype(np.uint8)
    colour = np.stack([page] * 3, -1)
    assert ccitt_ref.is_bilevel(page) and ccitt_ref.is_bilevel(colour)
    off = page.copy()
    off[2, 3] = 254
    tinted = colour.copy()
    tinted[4, 69, 1] ^= 255
    assert not ccitt_ref.is_bilevel(off) and not ccitt_ref.is_bilevel(tinted) and not ccitt_ref.is_bilevel(page.astype(np.int16))
    packed = ccitt_ref.pack_rows(ccitt_ref.black_mask(colour))
    assert packed.shape == (5, 3) and packed.dtype == np.uint32
    assert bool(packed[0, 0] >> 31) == (page[0, 0] == 0) and bool((packed[3, 2] >> (31 - 5)) & 1) == (page[3, 69] == 0)
    assert not (packed[:, 2] & ((1 << 26) - 1)).any()  # nothing behind column 70


def _row_bits(cur, ref):
    return sum(n for n, _ in ccitt_ref.row_codes(np.array(cur, bool), np.array(ref, bool)))


def test_no_row_exceeds_the_slot_bound():
    """7 w + 21 bits (the proof is in yomitoku_amd/csrc/ymk_ccitt.hip): every pair of rows up to 6 wide, and the patterns with the
    most changes a pixel at widths round the word size."""
    for w in range(1, 7):
        rows = list(itertools.product((False, True), repeat=w))
        assert max(_row_bits(cur, ref) for cur in rows for ref in rows) <= 7 * w + 21
    worst = 0.0
    for w in (31, 32, 33, 64, 65, 200):
        x = np.arange(w)
        patterns = [x % 2 == 0, x % 2 == 1, x % 3 == 0, x % 4 < 2, (x // 2) % 2 == 1, np.zeros(w, bool), np.ones(w, bool),
                    np.random.default_rng(w).random(w) < 0.5]
        for cur in patterns:
            for ref in patterns:
                bits = _row_bits(cur, ref)
                assert bits <= 7 * w + 21
                worst = max(worst, bits / w)
    assert 3.0 < worst < 7.0  # the bound is not vacuous on these patterns


# ------------------------------------------------------------------------------------------------ the PDF writer
def _bilevel(page, scale=1.0):
    from yomitoku_amd.ccitt import EncodedBilevel

    return EncodedBilevel(ccitt_ref.encode_g4(ccitt_ref.black_mask(page)), page.shape[1], page.shape[0], scale)


def _text_page(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    black = (yy % 24 < 7) & (xx % 97 < 60) & (rng.random((h, w)) < 0.8)
    return np.where(black, 0, 255).astype(np.uint8)


def test_encoded_bilevel_has_the_fields_and_a_tiff_pillow_opens():
    page = _text_page(120, 400, 3)
    entry = _bilevel(page)
    assert entry.bilevel is True and (entry.width, entry.height, entry.scale) == (400, 120, 1.0) and not hasattr(entry, "grey")
    assert entry.to_tiff() == ccitt_ref.to_tiff(entry.data, 400, 120)
    image = Image.open(io.BytesIO(entry.to_tiff()))
    image.load()
    tags = image.tag_v2
    assert (tags[256], tags[257], tags[258], tags[259], tags[262], tags[277], tags[278], tags[293]) == (400, 120, (1,), 4, 0, 1, 120, 0)
    assert np.array_equal(np.where(np.asarray(image.convert("L")) == 0, 0, 255), page)


def test_pdf_embeds_an_encoded_bilevel_as_a_ccitt_image():
    from yomitoku_amd.utils.searchable_pdf import _is_bilevel, _is_encoded

    doc = _doc()
    page = _text_page(120, 400, 4)
    entry = _bilevel(page)
    assert _is_bilevel(entry) and not _is_encoded(entry)
    pdf = searchable_pdf_bytes([entry], [doc], image_quality="low")
    (body,) = [b for b in _objects(pdf) if b.startswith(b"<< /Type /XObject")]
    head, _, rest = body.partition(b"\nstream\n")
    assert head == (b"<< /Type /XObject /Subtype /Image /Width 400 /Height 120 /ColorSpace /DeviceGray /BitsPerComponent 1 "
                    b"/Filter /CCITTFaxDecode /DecodeParms << /K -1 /Columns 400 /Rows 120 >> /Length %d >>" % len(entry.data))
    stream = rest[: len(entry.data)]
    assert stream == entry.data and rest[len(entry.data) :] == b"\nendstream"
    image = Image.open(io.BytesIO(ccitt_ref.to_tiff(stream, 400, 120)))
    image.load()
    assert np.array_equal(np.where(np.asarray(image.convert("L")) == 0, 0, 255), page)
    # the text layer and the MediaBox are those of an EncodedJpeg of the same size and scale
    for scale in (1.0, 0.375):
        jpeg = SimpleNamespace(data=b"\xff\xd8\xff\xd9", width=400, height=120, grey=True, scale=scale)
        ours = searchable_pdf_bytes([_bilevel(page, scale)], [doc], "high")
        theirs = searchable_pdf_bytes([jpeg], [doc], "high")
        assert _text_matrices(ours) == _text_matrices(theirs) and len(_text_matrices(ours)) == 1
        assert re.findall(rb"/MediaBox \[.*?\]", ours) == re.findall(rb"/MediaBox \[.*?\]", theirs) == [b"/MediaBox [0 0 400 120]"]


def test_a_mixed_document_keeps_its_order():
    doc = _doc()
    first, third = _text_page(60, 100, 5), _text_page(33, 70, 6)
    jpeg = SimpleNamespace(data=b"\xff\xd8 second \xff\xd9", width=150, height=45, grey=False, scale=0.375)
    array = synthetic_page(40, 56, seed=2)
    pdf = searchable_pdf_bytes([_bilevel(first), jpeg, _bilevel(third), array], [doc] * 4, "high")
    filters = re.findall(rb"/Width (\d+) /Height (\d+) /ColorSpace /Device\w+ /BitsPerComponent (\d) /Filter /(\w+)", pdf)
    assert filters == [(b"100", b"60", b"1", b"CCITTFaxDecode"), (b"150", b"45", b"8", b"DCTDecode"), (b"70", b"33", b"1", b"CCITTFaxDecode"),
                       (b"56", b"40", b"8", b"DCTDecode")]
    assert [m for m in re.findall(rb"/MediaBox \[0 0 (\d+) (\d+)\]", pdf)] == [(b"100", b"60"), (b"150", b"45"), (b"70", b"33"), (b"56", b"40")]
    streams = _image_streams(pdf)
    assert streams[1][3] == jpeg.data and len(streams) == 4
    assert streams[0][3] == ccitt_ref.encode_g4(first == 0) and streams[2][3] == ccitt_ref.encode_g4(third == 0)


# ------------------------------------------------------------------------------------------------ refusals
BAD = [dict(jpeg="high", jpeg_bilevel=True), dict(jpeg="high", jpeg_bilevel="always"), dict(jpeg="high", jpeg_bilevel=1),
       dict(jpeg="high", jpeg_bilevel=None), dict(jpeg=None, jpeg_bilevel="auto"), dict(jpeg=None, jpeg_bilevel="always")]


@pytest.mark.parametrize("kwargs", BAD, ids=str)
def test_check_jpeg_preset_refuses(kwargs):
    from yomitoku_amd.serving import check_jpeg_preset

    with pytest.raises(ValueError, match="bilevel"):
        check_jpeg_preset(**kwargs)


def test_check_jpeg_preset_accepts_the_switch_and_its_default():
    from yomitoku_amd.serving import check_jpeg_preset

    for kwargs in (dict(jpeg="high", jpeg_bilevel="auto"), dict(jpeg="low", jpeg_bilevel=False), dict(jpeg=None), dict(jpeg=None, jpeg_bilevel=False),
                   dict(jpeg="middle", jpeg_bilevel="auto", jpeg_optimize=True, jpeg_subsampling="4:4:4", jpeg_grey="auto")):
        check_jpeg_preset(**kwargs)


def test_the_encoders_refuse_a_bad_switch_before_any_device_work():
    from yomitoku_amd.jpeg import encode_jpeg, encode_jpeg_pages

    page = _text_page(8, 8, 1)
    for bad in (True, "yes", 0, None):
        with pytest.raises(ValueError, match="bilevel"):
            encode_jpeg_pages([page], "high", bilevel=bad)
        with pytest.raises(ValueError, match="bilevel"):
            encode_jpeg(page, "high", bilevel=bad)


def test_serve_sharded_keeps_refusing_jpeg():
    from yomitoku_amd import distributed

    src = open(distributed.__file__).read()
    assert 'serve_kwargs.get("jpeg") is not None' in src and "NotImplementedError" in src


def test_host_abi_sizes():
    from yomitoku_amd import _lib

    lib = _lib.load()
    assert lib.ymk_g4_page_words() == 16
    for w in (1, 31, 32, 33, 1600, 16383):
        assert lib.ymk_g4_slot_words(w) * 32 >= 7 * w + 21 and lib.ymk_g4_slot_words(w) == -(-(7 * w + 32) // 32)
    assert lib.ymk_g4_slot_words(0) == -1 and lib.ymk_g4_slot_words(16384) == -1
    assert lib.ymk_g4_file_capacity(1200, 1600) == -(-(1200 * (7 * 1600 + 21) + 24) // 8)
    assert lib.ymk_g4_file_capacity(0, 5) == -1 and lib.ymk_g4_file_capacity(5, 16384) == -1
    from yomitoku_amd.ccitt import scratch_sizes

    rows, packed, slots, bits, offs = scratch_sizes([(3, 33), (70, 1)])
    assert rows == 73 and packed == (3 * 2 + 70) * 4 and slots == -(-(3 * lib.ymk_g4_slot_words(33) + 70 * 2) // 2) * 8
    assert bits == 74 * 4 and offs == 75 * 8


def test_load_image_hands_a_one_bit_file_over_as_a_two_valued_page(tmp_path):
    """What the switch is for: a 1-bit TIFF or PNG comes out of load_image as B G R with every sample 0 or 255."""
    from yomitoku_amd.data.functions import load_image

    black = np.random.default_rng(7).random((50, 70)) < 0.2
    for name, kwargs in (("scan.tif", {"compression": "group4"} if features.check("libtiff") else {}), ("scan.png", {})):
        Image.fromarray(~black).save(str(tmp_path / name), **kwargs)
        (page,) = load_image(str(tmp_path / name))
        assert page.shape == (50, 70, 3) and ccitt_ref.is_bilevel(page) and np.array_equal(ccitt_ref.black_mask(page), black)
