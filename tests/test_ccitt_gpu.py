"""The device Group 4 encoder (yomitoku_amd/csrc/ymk_ccitt.hip, yomitoku_amd/ccitt.py) against its definition, tests/ccitt_ref.py
- which tests/test_ccitt_host.py holds to libtiff.  Every comparison is exact."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import ccitt_ref
from tests.test_ccitt_host import CASES
from tests.test_jpeg_gpu import _guard_ok, _guarded
from tests.test_jpeg_host import synthetic_page

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _page(black, channels):
    """The uint8 page of a mask: 0 where black, 255 elsewhere, H x W or H x W x 3."""
    v = np.where(black, 0, 255).astype(np.uint8)
    return v if channels == 1 else np.ascontiguousarray(np.stack([v] * 3, -1))


class G4Wave:
    """Pages on the device, their page table and guarded scratch, driven stage by stage through the C ABI."""

    def __init__(self, pages):
        from yomitoku_amd import _lib
        from yomitoku_amd.ccitt import page_table, scratch_sizes

        self.lib, self.check = _lib.load(), _lib.check
        self.dev = torch.device("cuda:0")
        self.pages = [np.ascontiguousarray(p) for p in pages]
        self.tensors = [torch.from_numpy(p).to(self.dev) for p in self.pages]
        blob, self.packed_at, self.offsets, self.out_bytes = page_table(self.tensors)
        self.rec = blob.reshape(-1, 16)
        self.blob = torch.from_numpy(blob).to(self.dev)
        self.rows, packed_b, slot_b, bits_b, off_b = scratch_sizes([p.shape for p in self.pages])
        n = len(pages)
        self.sizes = {"flags": 4 * n, "packed": packed_b, "slots": slot_b, "bits": bits_b, "off": off_b, "out": self.out_bytes, "len": 4 * n}
        self.buf = {k: _guarded(v, self.dev) for k, v in self.sizes.items()}
        self.stream = torch.cuda.current_stream().cuda_stream
        self.max_cap, self.max_rows = int(self.rec[:, 10].max()), max(p.shape[0] for p in self.pages)

    def ptr(self, key):
        return self.buf[key].data_ptr()

    def host(self, key, dtype):
        torch.cuda.synchronize()
        return self.buf[key][: self.sizes[key]].cpu().numpy().view(dtype)

    def put(self, key, array):
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        assert raw.size <= self.sizes[key]
        self.buf[key][: raw.size] = torch.from_numpy(raw.copy()).to(self.dev)

    def common(self):
        return self.blob.data_ptr(), self.blob.numel(), len(self.pages)

    def test_pack(self):
        self.check(self.lib.ymk_g4_test_pack(*self.common(), max(p.shape[0] * p.shape[1] for p in self.pages), self.ptr("flags"), self.ptr("packed"),
                                             self.sizes["packed"], self.stream), "ymk_g4_test_pack")
        flags, words = self.host("flags", np.int32).tolist(), self.host("packed", np.uint32)
        packed = []
        for p, at in zip(self.pages, self.packed_at):
            h, rw = p.shape[0], -(-p.shape[1] // 32)
            packed.append(words[at : at + h * rw].reshape(h, rw))
        return flags, packed

    def code_rows(self):
        self.check(self.lib.ymk_g4_code_rows(*self.common(), self.rows, self.max_rows, self.ptr("packed"), self.sizes["packed"], self.ptr("slots"),
                                             self.sizes["slots"], self.out_bytes, self.ptr("bits"), self.stream), "ymk_g4_code_rows")
        bits, slots = self.host("bits", np.uint32), self.host("slots", np.uint32)
        out = []
        for k, p in enumerate(self.pages):
            first, sw = int(self.rec[k, 5]), self.lib.ymk_g4_slot_words(p.shape[1])
            at = int(self.rec[k, 11])  # below 2^31 in these tests
            rows = []
            for y in range(p.shape[0]):
                n = int(bits[first + y])
                rows.append((slots[at + y * sw : at + (y + 1) * sw].astype(">u4").tobytes()[: -(-n // 8)], n))
            out.append(rows)
        return out

    def scan(self):
        self.check(self.lib.ymk_g4_scan(*self.common(), self.rows, self.sizes["packed"], self.sizes["slots"], self.out_bytes, self.ptr("bits"),
                                        self.ptr("off"), self.ptr("len"), self.stream), "ymk_g4_scan")
        off = self.host("off", np.uint64)
        return [off[int(self.rec[k, 5]) + k :][: p.shape[0] + 1].tolist() for k, p in enumerate(self.pages)], self.host("len", np.int32).tolist()

    def concat(self):
        self.check(self.lib.ymk_g4_concat(*self.common(), self.rows, self.sizes["packed"], self.ptr("slots"), self.sizes["slots"], self.ptr("off"),
                                          self.ptr("len"), self.ptr("out"), self.out_bytes, self.max_cap, self.stream), "ymk_g4_concat")
        return self.files()

    def encode(self):
        self.check(self.lib.ymk_g4_encode_pages(*self.common(), self.rows, self.max_rows, self.ptr("packed"), self.sizes["packed"], self.ptr("slots"),
                                                self.sizes["slots"], self.ptr("bits"), self.ptr("off"), self.ptr("out"), self.out_bytes, self.max_cap,
                                                self.ptr("len"), self.stream), "ymk_g4_encode_pages")
        return self.files()

    def files(self):
        lengths, out = self.host("len", np.int32).tolist(), self.host("out", np.uint8)
        return [None if n < 0 else out[o : o + n].tobytes() for o, n in zip(self.offsets, lengths)]

    def guards_ok(self):
        return all(_guard_ok(self.buf[k], n) for k, n in self.sizes.items())


@pytest.fixture(scope="module")
def definition():
    """name -> (per row (bytes, bits), the file) of every recorded case, computed once."""
    return {name: (ccitt_ref.encode_rows(black), strip) for name, (black, strip) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_stage_equals_the_definition(name, definition, dev):
    """Every stage on its own, fed with the definition's output of the stage before: flags and packed rows, per-row bits and bit
    counts, offsets and length, the file.  Three-channel and one-channel pages in turn."""
    black, strip = CASES[name]
    rows, want = definition[name]
    assert want == strip
    channels = 3 if sorted(CASES).index(name) % 2 == 0 else 1
    wave = G4Wave([_page(black, channels)])
    flags, (packed,) = wave.test_pack()
    assert flags == [0] and np.array_equal(packed, ccitt_ref.pack_rows(black))
    wave.put("packed", ccitt_ref.pack_rows(black))
    (got_rows,) = wave.code_rows()
    assert [n for _, n in got_rows] == [n for _, n in rows]
    assert got_rows == rows
    wave.put("bits", np.array([n for _, n in rows], np.uint32))
    (offsets,), lengths = wave.scan()
    assert offsets == np.concatenate([[0], np.cumsum([n for _, n in rows])]).tolist() and lengths == [len(strip)]
    assert wave.concat() == [strip]
    assert wave.guards_ok()


def test_flags_tell_the_pages_that_are_not_two_valued(dev):
    rng = np.random.default_rng(3)
    base = rng.random((37, 150)) < 0.4
    good3, good1 = _page(base, 3), _page(base, 1)
    grey_254 = good3.copy()
    grey_254[36, 149] = 254  # the last pixel of the page, in all three channels
    one_1 = good1.copy()
    one_1[0, 0] = 1
    tinted = good3.copy()
    tinted[20, 64, 1] ^= 255  # B != G in one pixel, every sample still 0 or 255
    red = good3.copy()
    red[5, 31, 2] ^= 255  # G != R
    pages = [good3, grey_254, good1, one_1, tinted, red, synthetic_page(23, 40, seed=1)]
    wave = G4Wave(pages)
    flags, packed = wave.test_pack()
    assert flags == [0, 1, 0, 1, 1, 1, 1] == [0 if ccitt_ref.is_bilevel(p) else 1 for p in pages]
    assert np.array_equal(packed[0], ccitt_ref.pack_rows(base)) and np.array_equal(packed[2], ccitt_ref.pack_rows(base))
    assert wave.guards_ok()


def test_all_recorded_cases_as_one_wave_through_encode_g4_pages(definition, dev):
    from yomitoku_amd.ccitt import EncodedBilevel, encode_g4_pages

    names = sorted(CASES)
    pages = [_page(CASES[name][0], 1 + 2 * (k % 2)) for k, name in enumerate(names)]
    wave = G4Wave(pages)  # the whole wave through the C ABI: pages of every size in one table
    flags, _ = wave.test_pack()
    assert flags == [0] * len(pages) and wave.encode() == [CASES[name][1] for name in names] and wave.guards_ok()
    # the public entry point: host arrays and device tensors, a page that is not two-valued and one that is no page, in their places
    off = pages[3].copy()
    off.flat[7] = 128
    mixed = pages[:5] + [off, np.zeros((4, 4, 2), np.uint8)] + [torch.from_numpy(p).to("cuda:0") for p in pages[5:]]
    scratch = {}
    out = encode_g4_pages(mixed, scratch=scratch)
    assert isinstance(out[5], ValueError) and "two-valued" in str(out[5]) and isinstance(out[6], ValueError)
    for name, page, entry in zip(names, pages, out[:5] + out[7:]):
        assert isinstance(entry, EncodedBilevel) and entry.bilevel is True
        assert (entry.data, entry.width, entry.height, entry.scale) == (CASES[name][1], page.shape[1], page.shape[0], 1.0)
    crop = names.index("golden_crop")
    image = Image.open(io.BytesIO(out[crop if crop < 5 else crop + 2].to_tiff()))
    image.load()
    assert np.array_equal(np.asarray(image.convert("L")) == 0, CASES["golden_crop"][0])
    # the same scratch again with other sizes: no stale bits
    again = encode_g4_pages(list(reversed(pages[:9])), scratch=scratch)
    assert [e.data for e in again] == [CASES[name][1] for name in reversed(names[:9])]
    assert all(isinstance(e, ValueError) for e in encode_g4_pages([off]))


def _wave_pages(seed, sizes):
    rng = np.random.default_rng(seed)
    (h0, w0), (h1, w1), (h2, w2), (h3, w3), (h4, w4) = sizes
    yy, xx = np.mgrid[0:h0, 0:w0]
    text = ((yy % 12 < 5) & ((xx + 3 * (yy // 12)) % 31 < 20) & (rng.random((h0, w0)) < 0.9))
    three = _page(text, 3)
    one = _page(rng.random((h1, w1)) < 0.3, 1)
    colour = synthetic_page(h2, w2, seed=seed)
    grey_254 = _page(rng.random((h3, w3)) < 0.1, 3)
    grey_254[h3 // 2, w3 // 3] = 254
    tinted = _page(rng.random((h4, w4)) < 0.2, 3)
    tinted[h4 - 1, w4 - 1, 0] ^= 255
    return [three, one, colour, grey_254, tinted]


def test_a_wave_of_five_pages_two_of_them_two_valued(dev):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg_pages

    scratch = {}
    for seed, sizes in ((1, [(75, 130), (33, 70), (48, 64), (40, 56), (17, 33)]), (2, [(20, 45), (90, 200), (23, 9), (64, 80), (50, 31)])):
        pages = _wave_pages(seed, sizes)
        got = encode_jpeg_pages(pages, "high", scratch=scratch, optimize=True, grey="auto", bilevel="auto")
        for page, entry in zip(pages[:2], got[:2]):
            assert isinstance(entry, EncodedBilevel) and entry.data == ccitt_ref.encode_g4(ccitt_ref.black_mask(page))
            assert (entry.width, entry.height, entry.scale) == (page.shape[1], page.shape[0], 1.0)
        want = encode_jpeg_pages(pages[2:], "high", optimize=True, grey="auto")
        assert all(isinstance(e, EncodedJpeg) for e in want) and got[2:] == want
        assert [e.grey for e in want] == [False, True, False]
        # the switch off: the files of today, also for the two-valued pages
        plain = encode_jpeg_pages(pages, "high", scratch=scratch, optimize=True, grey="auto")
        assert all(isinstance(e, EncodedJpeg) for e in plain) and plain[2:] == want and plain[0].grey and plain[1].grey
    # nothing qualifies / everything does
    assert encode_jpeg_pages(pages[2:], "high", scratch=scratch, optimize=True, bilevel="auto") == encode_jpeg_pages(pages[2:], "high", optimize=True)
    both = encode_jpeg_pages(pages[:2], "high", scratch=scratch, bilevel="auto", grey="auto")
    assert [type(e) for e in both] == [EncodedBilevel] * 2 and both == got[:2]


def test_a_two_valued_page_is_not_resized_by_the_preset(dev):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import encode_jpeg, encode_jpeg_pages

    rng = np.random.default_rng(5)
    xx = np.arange(1600)[None, :].repeat(20, 0)
    two = _page((xx % 40 < 7) & (rng.random((20, 1600)) < 0.9), 3)
    colour = synthetic_page(20, 1600, seed=6)
    grey_valued = np.ascontiguousarray(np.stack([synthetic_page(20, 1600, seed=7, grey=True)] * 3, -1))
    got = encode_jpeg_pages([colour, two, grey_valued], "low", bilevel="auto", grey="auto")
    assert isinstance(got[1], EncodedBilevel) and (got[1].width, got[1].height, got[1].scale) == (1600, 20, 1.0)
    assert got[1].data == ccitt_ref.encode_g4(ccitt_ref.black_mask(two))
    assert got[0] == encode_jpeg(colour, "low", grey="auto") and (got[0].width, got[0].scale) == (1500, 1500 / 1600)
    assert got[2] == encode_jpeg(grey_valued, "low", grey="auto") and got[2].grey and got[2].width == 1500
    assert encode_jpeg(two, "low", bilevel="auto") == got[1]
