"""The device encoder's optimised Huffman tables (ymk_jpeg_histogram, ymk_jpeg_optimal_tables, the *_opt entropy and compaction
stages; `encode_jpeg_pages(..., optimize=True)`) against their definition, tests/jpeg_opt_ref.py.  Everything is integer
arithmetic: every comparison is exact."""
import numpy as np
import pytest

from tests import jpeg_opt_ref, jpeg_ref
from tests.test_jpeg_host import synthetic_page
from tests.test_jpeg_opt_host import crafted_histograms, golden_crop, noise

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64  # bytes of 0xA5 behind every buffer the library writes
LUT = 2 * (256 + 16)  # YMK_JPEG_TABLE_WORDS
DHT = 656  # YMK_JPEG_DHT_BYTES


class OptWave:
    """Pages on the device, their page table (the *_opt form) and guarded scratch, driven stage by stage through the C ABI."""

    def __init__(self, pages, quality, capacities=None):
        from yomitoku_amd import _lib
        from yomitoku_amd.jpeg import page_table, scratch_sizes

        self.lib, self.check = _lib.load(), _lib.check
        self.dev = torch.device("cuda:0")
        self.pages = [np.ascontiguousarray(p) for p in pages]
        self.n = len(pages)
        self.tensors = [torch.from_numpy(p).to(self.dev) for p in self.pages]
        self.quality = quality
        if capacities is None:
            capacities = [4 * p.size + 2048 for p in self.pages]
        blob, self.offsets, self.out_bytes = page_table(self.tensors, quality, capacities, optimize=True)
        self.blob = torch.from_numpy(blob).to(self.dev)
        self.shapes = [(p.shape[0], p.shape[1], 1 if p.ndim == 2 else 3) for p in self.pages]
        sized = scratch_sizes(self.shapes, optimize=True)
        self.mcus, self.blocks, self.intervals = sized[:3]
        assert sized[4] == 212 * self.blocks and sized[6] == sized[7] == 4 * LUT * self.n and sized[8] == DHT * self.n
        assert scratch_sizes(self.shapes)[4] == 208 * self.blocks  # the plain path keeps its reservation
        self.sizes = dict(zip(("coef", "stream", "iv", "hist", "tables", "dht"), sized[3:]), out=self.out_bytes, len=4 * self.n)
        self.buf = {k: torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=self.dev) for k, n in self.sizes.items()}
        self.stream = torch.cuda.current_stream().cuda_stream
        self.table = (self.blob.data_ptr(), self.blob.numel(), self.n)

    def ptr(self, key):
        return self.buf[key].data_ptr()

    def words(self, key, dtype=np.int32):
        torch.cuda.synchronize()
        return self.buf[key][: self.sizes[key]].cpu().numpy().view(dtype)

    def put(self, key, array):
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        assert raw.size == self.sizes[key], (key, raw.size, self.sizes[key])
        self.buf[key][: raw.size] = torch.from_numpy(raw.copy()).to(self.dev)

    def reference_coefficients(self):
        return [jpeg_ref.coefficients(p, self.quality) for p in self.pages]

    def histogram(self):
        self.check(self.lib.ymk_jpeg_histogram(*self.table, self.ptr("coef"), self.blocks, self.intervals, self.ptr("hist"), self.stream),
                   "ymk_jpeg_histogram")
        return self.words("hist").reshape(self.n, 2, 272)

    def optimal_tables(self):
        self.check(self.lib.ymk_jpeg_optimal_tables(*self.table, self.ptr("hist"), self.ptr("tables"), self.ptr("dht"), self.stream),
                   "ymk_jpeg_optimal_tables")
        dht = self.words("dht", np.uint8).reshape(self.n, DHT)
        lengths = dht[:, :4].copy().view(np.int32).reshape(-1)
        return self.words("tables", np.uint32).reshape(self.n, 2, 272), [bytes(d[4 : 4 + n]) for d, n in zip(dht, lengths)]

    def entropy_and_compact(self):
        self.check(self.lib.ymk_jpeg_entropy_opt(*self.table, self.ptr("coef"), self.blocks, self.ptr("tables"), self.ptr("stream"),
                                                 self.sizes["stream"], self.ptr("iv"), self.intervals, self.stream), "ymk_jpeg_entropy_opt")
        self.check(self.lib.ymk_jpeg_compact_opt(*self.table, self.ptr("stream"), self.sizes["stream"], self.blocks, self.ptr("iv"),
                                                 self.intervals, self.ptr("dht"), self.ptr("out"), self.out_bytes, self.ptr("len"),
                                                 self.stream), "ymk_jpeg_compact_opt")
        return self.files()

    def encode(self):
        self.check(self.lib.ymk_jpeg_encode_pages_opt(*self.table, self.mcus, self.blocks, self.intervals, self.ptr("coef"), self.ptr("hist"),
                                                      self.ptr("tables"), self.ptr("dht"), self.ptr("stream"), self.sizes["stream"],
                                                      self.ptr("iv"), self.ptr("out"), self.out_bytes, self.ptr("len"), self.stream),
                   "ymk_jpeg_encode_pages_opt")
        return self.files()

    def files(self):
        lengths = self.words("len").tolist()
        out = self.buf["out"].cpu().numpy()
        return [None if n < 0 else out[o : o + n].tobytes() for o, n in zip(self.offsets, lengths)], out

    def guards_ok(self):
        torch.cuda.synchronize()
        return all(bool((self.buf[k][n:] == 0xA5).all().item()) for k, n in self.sizes.items())


def _want_hist(coefs, shape):
    dc, ac = jpeg_opt_ref.histograms(coefs, shape[0], shape[1], shape[2] == 1)
    return np.concatenate([ac, dc], axis=1)  # [2][256 + 16]: the device's layout


def _page(shape, seed):
    return synthetic_page(shape[0], shape[1], seed=seed, grey=len(shape) == 2)


SHAPES = [(1, 1, 3), (16, 16, 3), (33, 17, 3), (40, 200, 3), (9, 23)]
MIXED = [(48, 64, 3), (17, 33, 3), (23, 9), (40, 200, 3), (1, 1, 3)]


def _mixed_pages(seed):
    return [noise(s, seed + k) if k % 2 else _page(s, seed + k) for k, s in enumerate(MIXED)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_histograms_equal_the_definition(shape):
    """(40, 200, 3): 78 blocks per interval - more than one chunk of 64 - and three intervals adding into one page's counts.
    The second run on the same scratch, with other coefficients, must not see the first one's counts."""
    wave = OptWave([_page(shape, 1)], 85)
    for page, quality in ((_page(shape, 1), 85), (noise(shape, 2), 100)):
        coefs = jpeg_ref.coefficients(page, quality)
        wave.put("coef", coefs)
        got = wave.histogram()
        assert np.array_equal(got[0], _want_hist(coefs, wave.shapes[0])), (shape, quality)
    assert wave.guards_ok()


def test_histograms_of_a_wave_of_five_pages_twice_on_the_same_scratch():
    wave = OptWave(_mixed_pages(10), 85)
    for seed in (10, 20):
        pages = _mixed_pages(seed)
        coefs = [jpeg_ref.coefficients(p, 85) for p in pages]
        wave.put("coef", np.concatenate(coefs))
        got = wave.histogram()
        for k, c in enumerate(coefs):
            assert np.array_equal(got[k], _want_hist(c, wave.shapes[k])), (seed, k)
    assert wave.guards_ok()


def _table_cases():
    """Per page the uploaded counts [2][272] (AC bins, then DC bins): crafted ones, every symbol present with counts up to the
    blocks of a 16383 x 16383 page, and those of a real crop."""
    rng = np.random.default_rng(7)
    crafted = crafted_histograms()
    a = np.zeros((2, 272), np.int64)
    a[0, :256], a[1, :256] = crafted["powers_of_three"], crafted["all_256_once"]
    a[0, 256 + 3], a[1, 256 + 0], a[1, 256 + 5] = 9, 4, 4  # one DC symbol; two of the same count
    b = np.zeros((2, 272), np.int64)
    b[0, :256] = rng.integers(1, 6 * 1024 * 1024 + 1, 256)
    b[0, 256:] = rng.integers(1, 6 * 1024 * 1024 + 1, 16)
    b[1, :256], b[1, 256:] = crafted["one_symbol"], 3 ** np.arange(16)[::-1]  # a DC chain as deep as 16 symbols can make it
    c = np.zeros((2, 272), np.int64)
    c[0, :256], c[1, :256] = crafted["two_symbols"], rng.integers(0, 3, 256) * rng.integers(1, 1000, 256)
    c[:, 256:] = 1
    crop = golden_crop(64, 96)
    real = _want_hist(jpeg_ref.coefficients(crop, 85), (64, 96, 3))
    grey = np.zeros((2, 272), np.int64)
    grey[0] = _want_hist(jpeg_ref.coefficients(crop[:, :, 1], 85), (64, 96, 1))[0]
    grey[1] = 5  # a grey page has no chrominance tables, whatever stands in their counts
    return [(a, False), (b, False), (c, False), (real, False), (grey, True)]


def _want_tables(hist, grey):
    out = [(0x00, jpeg_opt_ref.optimal_table(hist[0, 256:])), (0x10, jpeg_opt_ref.optimal_table(hist[0, :256]))]
    if not grey:
        out += [(0x01, jpeg_opt_ref.optimal_table(hist[1, 256:])), (0x11, jpeg_opt_ref.optimal_table(hist[1, :256]))]
    return out


def test_tables_equal_the_definition_on_uploaded_histograms():
    cases = _table_cases()
    wave = OptWave([np.zeros((8, 8) if grey else (8, 8, 3), np.uint8) for _, grey in cases], 85)
    wave.put("hist", np.stack([h for h, _ in cases]).astype(np.int32))
    words, dht = wave.optimal_tables()
    for k, (hist, grey) in enumerate(cases):
        want = _want_tables(hist, grey)
        assert dht[k] == jpeg_opt_ref.dht_segments(want), k
        assert np.array_equal(words[k], jpeg_opt_ref.lut_words(want)), k
    assert max(jpeg_opt_ref.code_sizes(cases[0][0][0, :256])) > 16  # the first case went through Figure K.3's loop
    assert wave.guards_ok()


def test_a_block_of_the_worst_case_stays_inside_its_reservation():
    """One interval of 66 blocks, every DC difference of category 11 and every AC coefficient +-1023, with tables in which those
    two symbols have 16-bit codes: 1665 bits per block - more than the plain path's 208 bytes, inside this path's 212."""
    h, w = 16, 176
    coefs = np.zeros((11, 6, 64), np.int16)
    coefs[:, :, 1:] = np.where(np.arange(63) % 2, -1023, 1023)
    y = np.where(np.arange(44) % 2, 1023, -1024).reshape(11, 4)
    coefs[:, :4, 0] = y
    coefs[:, 4, 0] = coefs[:, 5, 0] = np.where(np.arange(11) % 2, 1023, -1024)
    coefs = coefs.reshape(66, 64)
    hist = np.zeros((2, 272), np.int64)
    hist[:, 256 + np.array([11] + [c for c in range(16) if c != 11])] = 3 ** np.arange(16)  # category 11 the rarest of sixteen
    rare = [0x0A] + [s for s in range(1, 40) if s != 0x0A][:17]
    hist[:, rare] = 3 ** np.arange(18)  # 0x0A the rarest of eighteen
    tables = _want_tables(hist, False)
    for ident, spec in tables:
        codes = jpeg_ref.huffman_codes(spec)
        assert codes[0x0A if ident >> 4 else 11][1] == 16, ident
    want = jpeg_opt_ref.assemble(coefs, h, w, False, 85, tables)
    head = len(jpeg_opt_ref.header(h, w, False, 85, tables))
    scan = len(want) - head - 2 - want[head:].count(b"\xff\x00")
    assert scan == -(-66 * 1665 // 8) and 66 * 208 < scan <= 66 * 212
    wave = OptWave([np.zeros((h, w, 3), np.uint8)], 85)
    wave.put("coef", coefs)
    wave.put("hist", hist.astype(np.int32)[None])
    wave.optimal_tables()
    (got,), _ = wave.entropy_and_compact()
    assert got == want
    assert wave.guards_ok()  # the stream's guard stands right behind the interval's 66 * 212 bytes


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_five_stages_equal_the_definitions_file(shape):
    for quality, page in ((85, _page(shape, 3)), (100, noise(shape, 4))):
        wave = OptWave([page], quality)
        (got,), _ = wave.encode()
        assert got == jpeg_opt_ref.encode(page, quality), (shape, quality)
        assert wave.guards_ok()


def test_encode_jpeg_pages_optimize_equals_the_definition_and_the_default_is_unchanged():
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg_pages

    pages = [_page(s, 5) for s in SHAPES] + _mixed_pages(30)
    room = [4 * p.size + 2048 for p in pages]
    scratch = {}
    got = encode_jpeg_pages(pages, "high", scratch=scratch, capacities=room, optimize=True)
    plain = encode_jpeg_pages(pages, "high", scratch=scratch, capacities=room)
    again = encode_jpeg_pages(pages[::-1], "high", scratch=scratch, capacities=room[::-1], optimize=True)  # the scratch's old counts
    for page, g, p, a in zip(pages, got, plain, again[::-1]):
        assert isinstance(g, EncodedJpeg) and g.optimized and isinstance(p, EncodedJpeg) and not p.optimized
        assert g.data == a.data == jpeg_opt_ref.encode(page, 85)
        assert p.data == jpeg_ref.encode(page, 85)
        assert (g.width, g.height, g.grey, g.scale) == (page.shape[1], page.shape[0], page.ndim == 2, 1.0)


def test_a_page_over_its_capacity_fails_alone():
    from yomitoku_amd.jpeg import encode_jpeg_pages

    pages = [_page((48, 64, 3), 1), noise((32, 48, 3), 2), _page((24, 40), 3)]
    want = [jpeg_opt_ref.encode(p, 85) for p in pages]
    out = encode_jpeg_pages(pages, "high", capacities=[len(want[0]), len(want[1]) - 1, len(want[2])], optimize=True)
    assert isinstance(out[1], Exception) and "capacity" in str(out[1])
    assert out[0].data == want[0] and out[2].data == want[2]
    wave = OptWave(pages, 85, capacities=[len(want[0]), 64, len(want[2])])
    got, raw = wave.encode()
    assert got == [want[0], None, want[2]]
    assert (raw[wave.offsets[1] : wave.offsets[2]] == 0xA5).all()  # not a byte of the page that did not fit was written
    assert wave.guards_ok()


def test_the_low_preset_shrinks_then_optimises():
    from PIL import Image

    from yomitoku_amd.jpeg import encode_jpeg

    page = synthetic_page(64, 1600, seed=9)
    got = encode_jpeg(page, "low", optimize=True)
    small = np.asarray(Image.fromarray(page).resize((1500, 60), Image.LANCZOS))
    assert (got.width, got.height, got.scale, got.optimized) == (1500, 60, 1500 / 1600, True)
    assert got.data == jpeg_opt_ref.encode(small, 60)
