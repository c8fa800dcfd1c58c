"""The device's page-skew step (yomitoku_amd/csrc/ymk_deskew.hip, yomitoku_amd/deskew.py) against its definition,
tests/deskew_ref.py - which tests/test_deskew_host.py holds to a literal loop and exact arithmetic.  Every comparison is exact:
the luminance plane, the ink, the whole score array, the choice words, the rotated bytes.  One wave mixes the shapes at which
the kernels can go wrong - a packed word plus a tail, widths of exactly one and two words, three channels, a page without
ink, noise, a real page, a record that is no page - and is driven twice: stage by stage through the C ABI into guarded buffers
of exactly the stated sizes, and as the one composite call `launch` makes."""
import functools
import os

import numpy as np
import pytest

from tests import ccitt_ref
from tests import deskew_ref as R
from tests.test_jpeg_gpu import _guard_ok, _guarded

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_page.jpg")
MALFORMED = 6  # the wave's record that is edited into no page


def _strokes(h, w, seed):
    """a grey page with dark strokes of a few pixels on noisy paper"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ink = ((yy % 9 < 3) & (xx % 23 < 15)) ^ (rng.random((h, w)) < 0.02)
    return np.clip(np.where(ink, 40, 215) + rng.integers(-20, 21, (h, w)), 0, 255).astype(np.uint8)


def _bars(a):
    from PIL import Image

    page = np.full((64, 96), 255, np.uint8)
    for y0 in range(8, 56, 12):
        page[y0 : y0 + 4, 10:86] = 0
    return page if a == 0 else np.asarray(Image.fromarray(page).rotate(a, Image.BICUBIC, fillcolor=255))


@functools.lru_cache(maxsize=None)
def wave_pages():
    from PIL import Image

    rng = np.random.default_rng(42)
    golden = np.asarray(Image.open(GOLDEN).convert("L").rotate(3, Image.BICUBIC, fillcolor=255))
    colour = np.stack([_strokes(40, 100, 5), _strokes(40, 100, 6), _strokes(40, 100, 7)], -1)
    pages = [_strokes(33, 37, 1), _bars(0), _bars(2), _bars(-4), _strokes(40, 32, 2), _strokes(50, 64, 3),
             _strokes(20, 20, 4),  # MALFORMED: its record is edited
             colour, np.full((30, 45), 255, np.uint8), rng.integers(0, 256, (70, 90), dtype=np.uint8),
             np.ascontiguousarray(golden[50:350, 50:300])]
    return tuple(np.array(p, order="C") for p in pages)  # writable copies: Pillow hands out read-only views


@functools.lru_cache(maxsize=None)
def expected(index, step=0.1, max_angle=5.0, min_angle=0.3):
    """(ink mask, [S_k], (k, S_k, S_0), the corrected page) of page `index` of the wave by the definition - computed once."""
    from yomitoku_amd.deskew import angle_table, dead_band

    page = wave_pages()[index]
    table = angle_table(step, max_angle)
    mask = R.ink(page)
    S = R.scores(mask, table)
    choice = R.choose(S, dead_band(step, min_angle))
    s, c = table[choice[0] + len(table) // 2].tolist()
    return mask, S, choice, R.rotate(page, s, c)


def _malform(rec):
    rec[MALFORMED, 2] = 0  # h = 0: no page


class Staged:
    """Pages on the device, the page table and guarded buffers of exactly the stated sizes, driven stage by stage through the
    C ABI."""

    def __init__(self, pages, params, edit=None):
        from yomitoku_amd import _lib
        from yomitoku_amd.deskew import _checked_table, page_table, scratch_sizes

        self.lib, self.check, self.dev = _lib.load(), _lib.check, torch.device("cuda:0")
        self.pages = list(pages)
        self.tensors = [torch.from_numpy(p).to(self.dev) for p in self.pages]
        self.n = len(pages)
        self.table, self.s_max, self.dead = _checked_table(params)
        self.sizes, self.fits = scratch_sizes([p.shape for p in pages], len(self.table), self.s_max)
        self.dst_bytes = [p.size for p in self.pages]
        self.dsts = [_guarded(b, self.dev) for b in self.dst_bytes]
        rec = page_table(self.tensors, self.dsts)
        if edit is not None:
            edit(rec)
        self.rec = rec
        self.blob = torch.from_numpy(rec.reshape(-1).copy()).to(self.dev)
        self.table_dev = torch.from_numpy(self.table.reshape(-1).copy()).to(self.dev)
        self.luma, self.sat, self.packed, self.scores, self.choice = (_guarded(b, self.dev) for b in self.sizes)
        self.planes = _guarded(self.n * 16 * 4, self.dev)
        self.stream = _lib.current_stream_ptr()
        self.most = max(p.shape[0] * p.shape[1] for p in pages)
        self.max_h, self.max_w = max(p.shape[0] for p in pages), max(p.shape[1] for p in pages)

    def run(self, rotate=True):
        luma_b, sat_b, packed_b, _, _ = self.sizes
        b, bw, n = self.blob.data_ptr(), self.blob.numel(), self.n
        self.check(self.lib.ymk_dsk_luma(b, bw, n, self.most, self.luma.data_ptr(), luma_b, packed_b, sat_b, self.planes.data_ptr(), self.stream),
                   "ymk_dsk_luma")
        self.check(self.lib.ymk_bin_adaptive_pack(self.planes.data_ptr(), n * 16, n, self.max_h, self.max_w, self.sat.data_ptr(), sat_b,
                                                  self.packed.data_ptr(), packed_b, self.stream), "ymk_bin_adaptive_pack")
        self.check(self.lib.ymk_dsk_scores(b, bw, n, self.packed.data_ptr(), packed_b, sat_b, luma_b, self.table_dev.data_ptr(), len(self.table),
                                           self.s_max, self.scores.data_ptr(), self.stream), "ymk_dsk_scores")
        self.check(self.lib.ymk_dsk_choose(b, bw, n, packed_b, sat_b, luma_b, self.scores.data_ptr(), len(self.table), self.s_max, self.dead,
                                           self.choice.data_ptr(), self.stream), "ymk_dsk_choose")
        if rotate:
            self.check(self.lib.ymk_dsk_rotate(b, bw, n, 3 * self.most, self.table_dev.data_ptr(), len(self.table), self.choice.data_ptr(),
                                               self.stream), "ymk_dsk_rotate")
        torch.cuda.synchronize()
        for buf, size in zip((self.luma, self.sat, self.packed, self.scores, self.choice), self.sizes):
            assert _guard_ok(buf, size)
        assert _guard_ok(self.planes, self.n * 64)
        for buf, size in zip(self.dsts, self.dst_bytes):
            assert _guard_ok(buf, size)
        return self

    def luma_of(self, k):
        at = int(self.rec[k, 8])
        h, w = self.pages[k].shape[:2]
        return self.luma[at : at + h * w].cpu().numpy().reshape(h, w)

    def ink_of(self, k):
        at = int(self.rec[k, 6])
        h, rw = self.pages[k].shape[0], -(-self.pages[k].shape[1] // 32)
        return self.packed[: self.sizes[2]].cpu().numpy().view(np.uint32)[at : at + h * rw].reshape(h, rw)

    def scores_of(self, k):
        n = len(self.table)
        return self.scores[: self.sizes[3]].cpu().numpy().view(np.uint64).reshape(self.n, n)[k].tolist()

    def choice_of(self, k):
        words = self.choice[: self.sizes[4]].cpu().numpy().view(np.int32).reshape(self.n, 8)[k]
        big = words[2:6].copy().view(np.uint64)
        assert words[6] == 0 and words[7] == 0
        return int(words[0]), int(words[1]), int(big[0]), int(big[1])

    def dst_of(self, k):
        return self.dsts[k][: self.dst_bytes[k]].cpu().numpy().reshape(self.pages[k].shape)


def _check_wave(run, indices, params=(), rotate=True):
    """every stage of a staged run of the wave's pages `indices` against the definition"""
    for j, index in enumerate(indices):
        page = run.pages[j]
        if index == MALFORMED and run.n > 1:  # absent: nothing written, flag -1
            assert run.scores_of(j) == [0] * len(run.table)
            assert run.choice_of(j) == (0, -1, 0, 0)
            assert bool((run.dsts[j] == 0xA5).all().item())
            continue
        mask, S, choice, fixed = expected(index, *params)
        if page.ndim == 3:
            assert (run.luma_of(j) == R.luminance(page)).all(), index
        assert (run.ink_of(j) == ccitt_ref.pack_rows(mask)).all(), index
        assert run.scores_of(j) == S, index
        assert run.choice_of(j) == (choice[0], 1, choice[1], choice[2]), index
        if rotate:
            assert run.dst_of(j).tobytes() == fixed.tobytes(), index
            if choice[0] == 0:
                assert run.dst_of(j).tobytes() == page.tobytes(), index


def test_the_definition_turns_some_pages_of_the_wave_and_leaves_others(dev):
    """what the wave is for: the kernels' rotation and copy paths are both taken, and by a real page"""
    ks = [expected(i)[2][0] for i in range(len(wave_pages())) if i != MALFORMED]
    assert any(k > 0 for k in ks) and any(k < 0 for k in ks) and any(k == 0 for k in ks)
    assert abs(expected(10)[2][0] * 0.1 - 3.0) <= 0.1 + 1e-9  # the golden crop, turned by 3 degrees
    assert expected(8)[1] == [0] * 101 and expected(8)[2] == (0, 0, 0)  # the blank page
    assert expected(9)[2][0] == 0  # noise


def test_every_stage_of_the_wave_equals_the_definition(dev):
    from yomitoku_amd.deskew import DEFAULTS

    run = Staged(wave_pages(), dict(DEFAULTS), edit=_malform).run()
    _check_wave(run, range(len(wave_pages())))


def test_another_table_of_angles(dev):
    run = Staged(wave_pages(), {"step": 0.25, "max_angle": 2.0, "min_angle": 0.3}, edit=_malform).run()
    assert len(run.table) == 17
    _check_wave(run, range(len(wave_pages())), params=(0.25, 2.0, 0.3))


@pytest.mark.parametrize("index", [7, 10, 0])
def test_a_call_with_one_page(dev, index):
    """block counts that differ from the wave's must not hide an indexing error: the colour page, the golden crop, 33 x 37"""
    from yomitoku_amd.deskew import DEFAULTS

    run = Staged([wave_pages()[index]], dict(DEFAULTS)).run()
    _check_wave(run, [index])


def test_a_page_too_large_for_the_profile_is_copied_and_not_estimated(dev):
    """16200 x 8: more row bins than the LDS profile holds.  Scores 0, k 0, flag 0, the bytes as they were - beside a page that is
    estimated as ever"""
    from yomitoku_amd.deskew import DEFAULTS, deskew_pages

    tall = _strokes(16200, 8, 9)
    run = Staged([tall, wave_pages()[3]], dict(DEFAULTS)).run()
    assert run.fits == [False, True]
    assert run.scores_of(0) == [0] * 101 and run.choice_of(0) == (0, 0, 0, 0)
    assert run.dst_of(0).tobytes() == tall.tobytes()
    _check_wave(Staged([wave_pages()[3]], dict(DEFAULTS)).run(), [3])
    assert run.scores_of(1) == expected(3)[1] and run.dst_of(1).tobytes() == expected(3)[3].tobytes()
    fixed, skews = deskew_pages([tall])
    assert not skews[0].estimated and skews[0].angle == 0.0 and fixed[0].cpu().numpy().tobytes() == tall.tobytes()


def test_the_composite_call_with_a_malformed_record(dev):
    from yomitoku_amd.deskew import DEFAULTS, launch

    pages = wave_pages()
    tensors = [torch.from_numpy(p).to(dev) for p in pages]
    done = launch(tensors, dict(DEFAULTS), {}, edit_table=_malform)
    torch.cuda.synchronize()
    skews = done.skews()
    n_scores = done.buffers["scores"][: len(pages) * 101].cpu().numpy().view(np.uint64).reshape(len(pages), 101)
    for k, page in enumerate(pages):
        if k == MALFORMED:
            assert skews[k].index == 0 and not skews[k].estimated and not n_scores[k].any()
            continue
        mask, S, choice, fixed = expected(k)
        assert n_scores[k].tolist() == S
        assert (skews[k].index, skews[k].score, skews[k].score_upright, skews[k].estimated) == (choice[0], choice[1], choice[2], True)
        assert skews[k].angle == pytest.approx(choice[0] * 0.1)
        assert done.corrected[k].cpu().numpy().tobytes() == fixed.tobytes()


def test_deskew_pages_on_host_arrays_and_device_tensors(dev):
    from yomitoku_amd.deskew import PageSkew, deskew_pages, estimate_skew_pages

    pages = [p for k, p in enumerate(wave_pages()) if k != MALFORMED]
    wanted = [expected(k) for k in range(len(wave_pages())) if k != MALFORMED]
    scratch = {}
    from_host, skews_host = deskew_pages(list(pages) + [np.zeros((4, 4), np.float32)], scratch=scratch)
    assert isinstance(from_host[-1], ValueError) and isinstance(skews_host[-1], ValueError)
    tensors = [torch.from_numpy(p).to(dev) for p in pages]
    from_dev, skews_dev = deskew_pages(tensors, scratch=scratch)  # the scratch of the first call again
    only = estimate_skew_pages(tensors, True)
    for j, (_, _, choice, fixed) in enumerate(wanted):
        for got, skew in ((from_host[j], skews_host[j]), (from_dev[j], skews_dev[j])):
            assert isinstance(skew, PageSkew) and got.device.type == "cuda" and got.dtype == torch.uint8
            assert got.cpu().numpy().tobytes() == fixed.tobytes()
            assert (skew.index, skew.score, skew.score_upright) == choice
        assert only[j].index == choice[0] and np.array_equal(only[j].matrix, skews_dev[j].matrix)
        assert tensors[j].cpu().numpy().tobytes() == pages[j].tobytes()  # the input is left alone
    turned = skews_dev[-1]  # the golden crop: the matrix maps the corrected centre to the centre
    h, w = pages[-1].shape
    assert turned.index != 0 and np.allclose(turned.to_original([(w - 1) / 2, (h - 1) / 2]), [(w - 1) / 2, (h - 1) / 2])
    assert deskew_pages([]) == ([], []) and estimate_skew_pages([]) == []
    with pytest.raises(ValueError):
        deskew_pages(tensors[:1], deskew="yes")


def test_the_library_refuses_bad_arguments(dev):
    from yomitoku_amd.deskew import DEFAULTS

    run = Staged([wave_pages()[0]], dict(DEFAULTS))
    lib, b = run.lib, run.blob.data_ptr()
    assert lib.ymk_dsk_scores(b, 15, 1, run.packed.data_ptr(), run.sizes[2], run.sizes[1], 0, run.table_dev.data_ptr(), 101, 1428,
                              run.scores.data_ptr(), run.stream) != 0  # a table of fewer words than a record
    assert lib.ymk_dsk_scores(b, 16, 1, run.packed.data_ptr(), run.sizes[2], run.sizes[1], 0, run.table_dev.data_ptr(), 100, 1428,
                              run.scores.data_ptr(), run.stream) != 0  # an even number of angles
    assert lib.ymk_dsk_choose(b, 16, 1, run.sizes[2], run.sizes[1], 0, run.scores.data_ptr(), 403, 1428, 3, run.choice.data_ptr(), run.stream) != 0
    assert lib.ymk_dsk_rotate(b, 16, 1, 64, None, 101, run.choice.data_ptr(), run.stream) != 0
    assert lib.ymk_last_error()
    assert lib.ymk_dsk_pages(b, 16, 0, 1, 1, None, 0, None, 0, None, 0, None, None, 101, 1428, 3, None, None, 1, run.stream) == 0  # no pages
    torch.cuda.synchronize()
