"""The device binariser (yomitoku_amd/csrc/ymk_binarize.hip, yomitoku_amd/ccitt.py) against its definition,
tests/binarize_ref.py - which tests/test_binarize_host.py holds to exact arithmetic.  Every comparison is exact: the flags,
Otsu's thresholds, the packed rows against ccitt_ref.pack_rows(mask), the files against ccitt_ref.encode_g4(mask)."""
import functools

import numpy as np
import pytest

from tests import binarize_ref, ccitt_ref
from tests.test_jpeg_gpu import _guard_ok, _guarded
from tests.test_jpeg_host import synthetic_page

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 64), (3, 65), (17, 31), (33, 130), (64, 257), (40, 2100), (2100, 40), (96, 160)]
CONTENTS = ["noise", "bimodal", "two_valued", "uniform"]


@functools.lru_cache(maxsize=None)
def grey_pages(h, w, content):
    """The single-channel pages of a case, seeded by its shape.  The 96 x 160 noise page is the gradient page."""
    rng = np.random.default_rng(1000 * h + w)
    if content == "noise":
        return (binarize_ref.gradient_page()[0],) if (h, w) == (96, 160) else (rng.integers(0, 256, (h, w), dtype=np.uint8),)
    if content == "uniform":
        return tuple(np.full((h, w), v, np.uint8) for v in (0, 128, 255))
    yy, xx = np.mgrid[0:h, 0:w]
    ink = ((yy % 11 < 4) & (xx % 37 < 21)) ^ (rng.random((h, w)) < 0.02)  # strokes of a few pixels, some specks
    if content == "two_valued":
        return (np.where(ink, 0, 255).astype(np.uint8),)
    return (np.clip(np.where(ink, 50, 200) + rng.integers(-30, 31, (h, w)), 0, 255).astype(np.uint8),)


@functools.lru_cache(maxsize=None)
def expected(h, w, content, method):
    """Per page of the case (threshold, mask, packed rows, file) by the definition - computed once, for both channel counts."""
    out = []
    for page in grey_pages(h, w, content):
        mask = binarize_ref.black_mask(page, method)
        out.append((binarize_ref.otsu_threshold(page) if method == "otsu" else None, mask, ccitt_ref.pack_rows(mask), ccitt_ref.encode_g4(mask)))
    return out


def _bgr(page):
    return np.ascontiguousarray(np.stack([page] * 3, -1))


def _binarize(pages, method, scratch=None):
    """start_binarize on host pages -> (flags, thresholds, the packed rows per page)"""
    from yomitoku_amd.ccitt import start_binarize

    tensors = [torch.from_numpy(np.ascontiguousarray(p)).to("cuda:0") for p in pages]
    run = start_binarize(tensors, {} if scratch is None else scratch, method)
    torch.cuda.synchronize()
    words = run.packed.cpu().numpy().view(np.uint32)
    packed = []
    for p, at in zip(pages, run.packed_at):
        h, rw = p.shape[0], -(-p.shape[1] // 32)
        packed.append(words[at : at + h * rw].reshape(h, rw))
    assert run.answers() == [f == 0 for f in run.flags()]
    return run.flags(), run.thresholds(), packed


@pytest.mark.parametrize("method", binarize_ref.METHODS)
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_flags_thresholds_rows_and_files_equal_the_definition(dev, shape, content, method):
    """one wave per case: its pages with one channel, then the same with three"""
    from yomitoku_amd.ccitt import EncodedBilevel, encode_g4_pages

    grey = list(grey_pages(*shape, content))
    want = expected(*shape, content, method) * 2
    pages = grey + [_bgr(p) for p in grey]
    flags, thresholds, packed = _binarize(pages, method)
    assert flags == [0] * len(pages)
    assert thresholds == [t for t, _, _, _ in want]
    for k, (rows, (_, _, ref_rows, _)) in enumerate(zip(packed, want)):
        assert np.array_equal(rows, ref_rows), k
    files = encode_g4_pages(pages, binarize=method)
    for k, (page, entry, (t, _, _, data)) in enumerate(zip(pages, files, want)):
        assert isinstance(entry, EncodedBilevel), (k, entry)
        assert entry.data == data, k
        assert (entry.width, entry.height, entry.scale, entry.method, entry.threshold) == (page.shape[1], page.shape[0], 1.0, method, t)
    if content == "two_valued":  # the file of "auto"
        auto = encode_g4_pages(pages)
        assert [e.data for e in auto] == [e.data for e in files] and all(e.method == "auto" and e.threshold is None for e in auto)


def test_the_gradient_page_on_the_device_tells_the_methods_apart(dev):
    page, ink = binarize_ref.gradient_page()
    _, _, (adaptive,) = _binarize([page], "adaptive")
    _, _, (otsu,) = _binarize([page], "otsu")
    assert np.array_equal(adaptive, ccitt_ref.pack_rows(ink)) and not np.array_equal(otsu, ccitt_ref.pack_rows(ink))


@pytest.mark.parametrize("method", binarize_ref.METHODS)
def test_a_wave_of_mixed_sizes_with_a_colour_page_and_a_float_page(dev, method):
    from yomitoku_amd.ccitt import EncodedBilevel, encode_g4_pages

    colour = synthetic_page(45, 70, seed=4)
    assert colour.ndim == 3 and not binarize_ref.is_grey_valued(colour)
    nearly = _bgr(grey_pages(33, 130, "bimodal")[0])
    nearly[32, 129, 2] ^= 1  # one sample of the last pixel
    cases = [((17, 31), "noise"), ((64, 257), "bimodal"), None, ((3, 65), "two_valued"), ((33, 130), "noise")]
    pages = [colour if c is None else (_bgr(grey_pages(*c[0], c[1])[0]) if k % 2 else grey_pages(*c[0], c[1])[0]) for k, c in enumerate(cases)]
    pages.append(nearly)
    flags, thresholds, packed = _binarize(pages, method)
    assert flags == [0, 0, 1, 0, 0, 1]
    for k, c in enumerate(cases):
        if c is not None:
            t, _, rows, _ = expected(*c[0], c[1], method)[0]
            assert thresholds[k] == t and np.array_equal(packed[k], rows), k
    sources = pages[:4] + [pages[4].astype(np.float32)] + pages[4:]
    out = encode_g4_pages(sources, binarize=method)
    assert isinstance(out[4], ValueError) and "uint8" in str(out[4])
    out = out[:4] + out[5:]
    for k, c in enumerate(cases):
        if c is None:
            assert isinstance(out[k], ValueError) and "grey-valued" in str(out[k])
        else:
            assert isinstance(out[k], EncodedBilevel) and out[k].data == expected(*c[0], c[1], method)[0][3], k
    assert isinstance(out[5], ValueError) and "grey-valued" in str(out[5])
    with pytest.raises(ValueError, match="bilevel"):
        encode_g4_pages(pages, binarize="auto")


def test_a_page_whose_summed_area_table_passes_2_to_32(dev):
    """4120 x 4112 of 255 with about 1 % of samples in 200..220: the table's last entry is 4.31e9 > 2^32, so a 32-bit table
    that did not wrap exactly - or a 32-bit intermediate that is not a difference - shows in the rows.  (At 4100 rows, the height
    first planned, the page sums to 4 291 517 487, which is 3.4 M short of 2^32 and would exercise nothing; twenty more rows pass
    it.)  r = 257.  The NumPy side sums in int64.  The file of this page is not compared: the coder behind the rows is the one
    every other case runs, and the definition in Python would take a minute on it."""
    h, w = 4120, 4112
    rng = np.random.default_rng(41)
    page = np.full((h, w), 255, np.uint8)
    at = rng.random((h, w)) < 0.01
    page[at] = rng.integers(200, 221, int(at.sum()), dtype=np.uint8)
    assert int(page.astype(np.int64).sum()) > 1 << 32
    mask = binarize_ref.black_mask(page, "adaptive")
    assert 0.005 < mask.mean() < 0.01 and np.array_equal(mask, page <= 216)  # 17 / 20 of a mean just below 255
    flags, _, (rows,) = _binarize([page], "adaptive")
    assert flags == [0] and np.array_equal(rows, ccitt_ref.pack_rows(mask))
    flags, thresholds, (rows,) = _binarize([page], "otsu")
    t = binarize_ref.otsu_threshold(page)
    assert flags == [0] and thresholds == [t] and np.array_equal(rows, ccitt_ref.pack_rows(page <= t))


@pytest.mark.parametrize("method", binarize_ref.METHODS)
def test_the_calls_stay_inside_the_buffers_they_are_given_and_take_a_bad_record_as_absent(dev, method):
    """through the C ABI with guarded scratch: three pages, the middle one's record says its table (its packed rows, for "otsu")
    lies beyond the buffer - its flag is the grey test's, none of its rows is written, the neighbours' are, and no guard changes"""
    from yomitoku_amd import _lib
    from yomitoku_amd.ccitt import binarize_scratch_sizes, page_table, scratch_sizes

    lib, device = _lib.load(), torch.device("cuda:0")
    cases = [((33, 130), "noise"), ((64, 257), "bimodal"), ((17, 31), "bimodal")]
    pages = [grey_pages(*s, c)[0] for s, c in cases]
    tensors = [torch.from_numpy(p).to(device) for p in pages]
    blob, packed_at, _, _ = page_table(tensors, capacities=[0] * 3, tables=True)
    rec = blob.reshape(-1, 16)
    assert rec[1, 14] == 33 * 130 and rec[2, 14] == 33 * 130 + 64 * 257 and not rec[:, 13].any() and not rec[:, 15].any()
    packed_b = scratch_sizes([p.shape for p in pages])[1]
    hist_b, sat_b = binarize_scratch_sizes([p.shape for p in pages])
    assert hist_b == 3 * 256 * 4 and sat_b >= 4 * sum(p.size for p in pages)
    if method == "adaptive":
        rec[1, 14] = sat_b // 4 - 64 * 257 + 1  # one word too far
    else:
        rec[1, 6] = packed_b // 4 - 64 * 9 + 1
    sizes = {"answer": 24, "hist": hist_b, "sat": sat_b, "packed": packed_b}
    buf = {k: _guarded(v, device) for k, v in sizes.items()}
    blob_dev = torch.from_numpy(rec.reshape(-1)).to(device)
    stream = torch.cuda.current_stream().cuda_stream
    common = (blob_dev.data_ptr(), blob_dev.numel(), 3)
    most = max(p.size for p in pages)
    if method == "otsu":
        _lib.check(lib.ymk_bin_test_hist(*common, most, buf["answer"].data_ptr(), buf["hist"].data_ptr(), stream), "ymk_bin_test_hist")
        _lib.check(lib.ymk_bin_otsu(3, buf["hist"].data_ptr(), buf["answer"].data_ptr() + 12, stream), "ymk_bin_otsu")
        _lib.check(lib.ymk_bin_otsu_pack(*common, most, buf["answer"].data_ptr() + 12, buf["packed"].data_ptr(), packed_b, stream), "ymk_bin_otsu_pack")
    else:
        _lib.check(lib.ymk_bin_test_hist(*common, most, buf["answer"].data_ptr(), None, stream), "ymk_bin_test_hist")
        _lib.check(lib.ymk_bin_adaptive_pack(*common, 64, 257, buf["sat"].data_ptr(), sat_b, buf["packed"].data_ptr(), packed_b, stream),
                   "ymk_bin_adaptive_pack")
    torch.cuda.synchronize()
    assert all(_guard_ok(buf[k], n) for k, n in sizes.items())
    answer = buf["answer"][:24].cpu().numpy().view(np.int32).tolist()
    assert answer[:3] == [0, 0, 0]
    words = buf["packed"][:packed_b].cpu().numpy().view(np.uint32)
    if method == "otsu":
        assert answer[3:] == [expected(*s, c, "otsu")[0][0] for s, c in cases]
        hist = buf["hist"][:hist_b].cpu().numpy().view(np.uint32).reshape(3, 256)
        assert all(np.array_equal(hist[k], binarize_ref.histogram(p)) for k, p in enumerate(pages))
    for k in (0, 2):
        rows = expected(*cases[k][0], cases[k][1], method)[0][2]
        assert np.array_equal(words[packed_at[k] : packed_at[k] + rows.size].reshape(rows.shape), rows), k
    assert (words[packed_at[1] : packed_at[2]] == 0xA5A5A5A5).all()  # the absent page's rows: as the buffer was
    # a record of zeros is no page
    zero = torch.zeros(16, dtype=torch.int32, device=device)
    _lib.check(lib.ymk_bin_test_hist(zero.data_ptr(), 16, 1, 0, buf["answer"].data_ptr(), None, stream), "ymk_bin_test_hist")
    torch.cuda.synchronize()
    assert buf["answer"][:4].cpu().numpy().view(np.int32).tolist() == [-1]


@pytest.mark.parametrize("method", binarize_ref.METHODS)
def test_encode_jpeg_pages_gives_grey_valued_pages_group4_files_and_colour_pages_their_jpegs(dev, method):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg, encode_jpeg_pages

    cases = {0: ((40, 2100), "bimodal"), 2: ((96, 160), "noise"), 4: ((33, 130), "two_valued")}
    pages = [grey_pages(*cases[0][0], cases[0][1])[0], synthetic_page(40, 1700, seed=1), _bgr(grey_pages(*cases[2][0], cases[2][1])[0]),
             synthetic_page(60, 80, seed=2), _bgr(grey_pages(*cases[4][0], cases[4][1])[0])]
    plain = encode_jpeg_pages(pages, "low")
    assert all(isinstance(e, EncodedJpeg) for e in plain) and plain[0].scale < 1.0 and plain[1].scale < 1.0  # "low" resizes what is longer than 1500
    scratch = {}
    for _ in range(2):  # the second call reuses the scratch
        got = encode_jpeg_pages(pages, "low", bilevel=method, scratch=scratch, optimize=False, grey=False)
        for k, (page, entry) in enumerate(zip(pages, got)):
            if k in cases:
                t, _, _, data = expected(*cases[k][0], cases[k][1], method)[0]
                assert isinstance(entry, EncodedBilevel) and entry.data == data, k
                assert (entry.width, entry.height, entry.scale, entry.method, entry.threshold) == (page.shape[1], page.shape[0], 1.0, method, t)
            else:
                assert entry == plain[k], k
    # untouched by the other options; the colour pages take them as they do without the switch
    more = encode_jpeg_pages(pages, "low", bilevel=method, optimize=True, subsampling="4:4:4", grey="auto")
    assert [more[k] for k in cases] == [got[k] for k in cases]
    assert [more[k] for k in (1, 3)] == [encode_jpeg_pages(pages, "low", optimize=True, subsampling="4:4:4", grey="auto")[k] for k in (1, 3)]
    assert encode_jpeg(pages[2], "low", bilevel=method) == got[2]
    assert encode_jpeg_pages(pages, "low", bilevel="auto")[4].data == got[4].data
