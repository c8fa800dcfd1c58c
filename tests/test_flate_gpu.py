"""The lossless page coder on the device (yomitoku_amd/csrc/ymk_flate.hip; yomitoku_amd/flate.py) against its definition,
tests/flate_ref.py: every phase entry held to the reference's intermediate - filtered bytes and filter types, tokens, histograms,
code lengths, codes and header bits, bit counts, file bytes - on the shapes at which the code takes another path (one pixel, one
row, one column, a flat page, noise without a match, a one-channel page, a row of exactly one segment, a row of two), the tables
entry on crafted histograms fed directly, and the combined entry on a wave of 16 mixed pages with guard bytes behind every file."""

import functools
import os
import zlib

import numpy as np
import pytest
import torch

from tests import flate_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def golden_page() -> np.ndarray:
    from PIL import Image

    return np.ascontiguousarray(np.array(Image.open(os.path.join(ROOT, "tests", "golden", "test_page.jpg")).convert("RGB"))[:, :, ::-1])


@functools.lru_cache(maxsize=None)
def pages() -> tuple:
    rng = np.random.default_rng(11)
    striped = np.zeros((3, 2731, 3), np.uint8)
    striped[:, ::7] = (200, 90, 10)
    striped[1, 5::11, 1] = 77
    crop = golden_page()[100:196, 100:260]
    return (("1x1", rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)),
            ("1x3", rng.integers(0, 256, (1, 3, 3), dtype=np.uint8)),
            ("3x1", rng.integers(0, 256, (3, 1, 3), dtype=np.uint8)),
            ("flat", np.full((33, 67, 3), 77, np.uint8)),
            ("noise", rng.integers(0, 256, (40, 70, 3), dtype=np.uint8)),
            ("crop", np.ascontiguousarray(crop)),
            ("grey", np.ascontiguousarray(crop[:, :, 1])),
            ("one_segment", np.ascontiguousarray(striped[:, :2730])),
            ("two_segments", striped))


NAMES = tuple(name for name, _ in pages())


@functools.lru_cache(maxsize=None)
def reference(name: str) -> R.Encoded:
    return R.Encoded(dict(pages())[name])


class Phases:
    """The five phase entries, one after the other, over all pages in one call; every buffer read back."""

    def __init__(self):
        from yomitoku_amd import flate

        self.flate = flate
        self.devs = [torch.from_numpy(p).cuda() for _, p in pages()]
        c = self.coding = flate._Coding(self.devs, {})
        c.start()  # ymk_flate_rows, ymk_flate_tables
        torch.cuda.synchronize()
        self.sizes_after_tables = c.answers()
        c.finish(list(range(len(self.devs))))  # ymk_flate_code, ymk_flate_scan, ymk_flate_gather
        torch.cuda.synchronize()
        self.rec = c.blob.reshape(-1, flate.PAGE_WORDS)
        host = lambda t: t.cpu().numpy()  # noqa: E731
        self.filt, self.tokens = host(c.filt), host(c.tokens).view(np.uint16)
        self.segtok, self.segbits = host(c.segtok).view(np.uint32), host(c.segbits).view(np.uint32)
        self.hist, self.tables, self.head = host(c.hist), host(c.tables).view(np.uint32), host(c.head).view(np.uint32)
        self.out, self.sizes = host(c.out), c.answers()

    def place(self, k: int):
        r = self.rec[k].view(np.uint32).astype(np.int64)
        return int(r[6] | r[7] << 32), int(r[8] | r[9] << 32), int(r[12] | r[13] << 32)  # filtered bytes, segments, file


@functools.lru_cache(maxsize=None)
def phases() -> Phases:
    return Phases()


def _reversed(code: int, bits: int) -> int:
    return int(format(code, f"0{bits}b")[::-1], 2) if bits else 0


def _expected_tables(t: R.Tables) -> np.ndarray:
    lens = np.concatenate([t.lit_len, t.dist_len])
    codes = np.concatenate([t.lit_code, t.dist_code])
    return np.array([int(n) << 16 | _reversed(int(c), int(n)) if n else 0 for n, c in zip(lens, codes)], np.uint32)


def _expected_head(t: R.Tables):
    w = R.BitWriter()
    w.put(0x9C78, 16)
    t.header(w)
    return w.n, w.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_filtered_bytes_and_filter_types(name):
    ph, k, ref = phases(), NAMES.index(name), reference(name)
    at, _, _ = ph.place(k)
    got = ph.filt[at : at + ref.filtered.size].reshape(ref.filtered.shape)
    assert np.array_equal(got[:, 0], ref.types)
    assert np.array_equal(got, ref.filtered)


@pytest.mark.parametrize("name", NAMES)
def test_tokens(name):
    ph, k, ref = phases(), NAMES.index(name), reference(name)
    at, seg, _ = ph.place(k)
    row, per_row = ref.filtered.shape[1], -(-ref.filtered.shape[1] // R.SEGMENT)
    assert len(ref.tokens) == ref.height * per_row
    for s, want in enumerate(ref.tokens):
        y, sg = divmod(s, per_row)
        first = at + y * row + sg * R.SEGMENT
        assert int(ph.segtok[seg + s]) == len(want), (y, sg)
        assert np.array_equal(ph.tokens[first : first + len(want)], want), (y, sg)


@pytest.mark.parametrize("name", NAMES)
def test_histograms(name):
    ph, k, ref = phases(), NAMES.index(name), reference(name)
    mine = ph.hist[k * ph.flate.HIST_WORDS :]
    assert np.array_equal(mine[: R.N_LIT], ref.lit_hist)
    assert np.array_equal(mine[R.N_LIT : R.N_LIT + R.N_DIST], ref.dist_hist)


@pytest.mark.parametrize("name", NAMES)
def test_code_lengths_codes_header_bits_and_the_exact_size(name):
    ph, k, ref = phases(), NAMES.index(name), reference(name)
    assert np.array_equal(ph.tables[k * ph.flate.HIST_WORDS :][: R.N_LIT + R.N_DIST], _expected_tables(ref.tables))
    head = ph.head[k * ph.flate.HEAD_WORDS :][: ph.flate.HEAD_WORDS]
    bits, data = _expected_head(ref.tables)
    assert int(head[2]) == bits
    assert head[10:].tobytes()[: len(data)] == data
    assert int(head[4]) == ref.adler == zlib.adler32(ref.filtered.tobytes())
    assert ph.sizes_after_tables[k] == (len(ref.data), ref.channels)  # exact before a bit is coded


@pytest.mark.parametrize("name", NAMES)
def test_bit_counts(name):
    ph, k, ref = phases(), NAMES.index(name), reference(name)
    _, seg, _ = ph.place(k)
    assert ph.segbits[seg : seg + len(ref.tokens)].tolist() == ref.segment_bits


@pytest.mark.parametrize("name", NAMES)
def test_file_bytes(name):
    ph, k, ref = phases(), NAMES.index(name), reference(name)
    _, _, at = ph.place(k)
    assert ph.sizes[k] == (len(ref.data), ref.channels)
    assert ph.out[at : at + len(ref.data)].tobytes() == ref.data
    assert np.array_equal(R.decode(ref.data, ref.height, ref.width, ref.channels), dict(pages())[name])


def _fibonacci(n: int) -> list:
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _crafted() -> list:
    fib = np.zeros(R.N_LIT, np.int64)
    fib[100:135] = _fibonacci(35)  # 35 symbols: the merges alone give 34 bits - the 15-bit limit binds
    fib[256] = 1
    dist_fib = np.zeros(R.N_DIST, np.int64)
    dist_fib[:25] = _fibonacci(25)
    one = np.zeros(R.N_LIT, np.int64)
    one[256] = 1  # one used symbol; no distance
    two = np.zeros(R.N_LIT, np.int64)
    two[[65, 256]] = (7, 1)
    d1 = np.zeros(R.N_DIST, np.int64)
    d1[3] = 9  # one used distance symbol
    spread = np.arange(1, R.N_LIT + 1, dtype=np.int64) % 17 + 1
    return [("fibonacci", fib, dist_fib), ("one", one, np.zeros(R.N_DIST, np.int64)), ("two", two, d1), ("all_used", spread, np.arange(R.N_DIST) + 1)]


def test_tables_entry_on_crafted_histograms_fed_directly():
    from yomitoku_amd import _lib, flate

    cases = _crafted()
    devs = [torch.zeros((1, 1), dtype=torch.uint8, device="cuda") for _ in cases]
    c = flate._Coding(devs, {})
    c.start()  # sizes every buffer and fills the segments' checksum parts; the histograms are then replaced
    hist = np.zeros((len(cases), flate.HIST_WORDS), np.int32)
    for k, (_, lit, dist) in enumerate(cases):
        hist[k, : R.N_LIT], hist[k, R.N_LIT : R.N_LIT + R.N_DIST] = lit, dist
    c.hist[: hist.size].copy_(torch.from_numpy(hist.reshape(-1)))
    _lib.check(_lib.load().ymk_flate_tables(*c._common(c.blob_dev, c.blob.size, c.n), None, c.hist.data_ptr(), c.segadler.data_ptr(), c.tables.data_ptr(),
                                            c.head.data_ptr(), c.sizes.data_ptr(), _lib.current_stream_ptr()), "ymk_flate_tables")
    torch.cuda.synchronize()
    tables, head = c.tables.cpu().numpy().view(np.uint32), c.head.cpu().numpy().view(np.uint32)
    for k, (name, lit, dist) in enumerate(cases):
        want = R.Tables(lit, dist)
        got = tables[k * flate.HIST_WORDS :][: R.N_LIT + R.N_DIST]
        assert np.array_equal(got >> 16, np.concatenate([want.lit_len, want.dist_len])), name
        assert np.array_equal(got, _expected_tables(want)), name
        bits, data = _expected_head(want)
        mine = head[k * flate.HEAD_WORDS :][: flate.HEAD_WORDS]
        assert int(mine[2]) == bits and mine[10:].tobytes()[: len(data)] == data, name
    assert int(R.Tables(cases[0][1], cases[0][2]).lit_len.max()) == 15  # the limit was reached


def _wave() -> list:
    rng = np.random.default_rng(5)
    g = golden_page()
    fixed = dict(pages())
    out = [fixed["1x1"], fixed["two_segments"], fixed["flat"], fixed["grey"], fixed["noise"]]
    for k, (h, w) in enumerate(((64, 96), (17, 130), (96, 160), (5, 1), (41, 3), (1, 200), (30, 31), (50, 64), (8, 8), (23, 77), (12, 300))):
        page = np.ascontiguousarray(g[40 * k : 40 * k + h, 30 * k : 30 * k + w])
        if k % 3 == 1:
            page = np.ascontiguousarray(page[:, :, 0])
        if k % 4 == 2:
            page = (page // 64 * 64).astype(np.uint8)  # flat colour: long matches
        if k == 9:
            page = rng.integers(0, 2, page.shape, dtype=np.uint8) * 255
        out.append(page)
    assert len(out) == 16
    return out


def test_combined_entry_on_a_wave_of_sixteen_mixed_pages_with_guard_bytes():
    from yomitoku_amd import flate

    batch = _wave()
    devs = [torch.from_numpy(p).cuda() for p in batch]
    c = flate._Coding(devs, {})
    c.out.fill_(0xA5)
    c.run()  # ymk_flate_encode_pages
    torch.cuda.synchronize()
    out, sizes = c.out.cpu().numpy(), c.answers()
    ends = c.offsets[1:] + [c.out.numel()]
    for k, page in enumerate(batch):
        want = R.encode(page)
        assert sizes[k] == (len(want), 1 if page.ndim == 2 else 3), k
        assert out[c.offsets[k] : c.offsets[k] + len(want)].tobytes() == want, k
        assert (out[c.offsets[k] + len(want) : ends[k]] == 0xA5).all(), k  # no byte behind the file's end is touched
    # the public entry: the same bytes, and a budget that only the compressible pages meet
    got = flate.encode_lossless_pages(batch[:6])
    assert [e.data for e in got] == [R.encode(p) for p in batch[:6]]
    assert [(e.width, e.height, e.channels, e.scale, e.nbytes) for e in got] == [(p.shape[1], p.shape[0], 1 if p.ndim == 2 else 3, 1.0, len(e.data))
                                                                                   for p, e in zip(batch[:6], got)]
    tight = flate.encode_lossless_pages([batch[2], batch[4]], budget=0.5)  # the flat page; noise
    assert tight[0].data == R.encode(batch[2]) and isinstance(tight[1], ValueError)


def test_a_file_that_does_not_fit_its_capacity_is_reported_and_nothing_of_it_written():
    from yomitoku_amd import flate

    batch = [dict(pages())["noise"], dict(pages())["flat"]]
    devs = [torch.from_numpy(p).cuda() for p in batch]
    c = flate._Coding(devs, {}, capacities=[100, 4096])
    c.out.fill_(0xA5)
    c.run()
    torch.cuda.synchronize()
    out, sizes = c.out.cpu().numpy(), c.answers()
    assert sizes[0][0] == -1 and (out[: c.offsets[1]] == 0xA5).all()
    want = R.encode(batch[1])
    assert sizes[1][0] == len(want) and out[c.offsets[1] : c.offsets[1] + len(want)].tobytes() == want
