"""The device's despeckling (yomitoku_amd/csrc/ymk_cc.hip, yomitoku_amd/despeckle.py: despeckle_masks) against its definition,
tests/despeckle_ref.py - which tests/test_despeckle_host.py holds to scipy.  Every comparison is exact: the clean mask bit for bit
and the four counts.  The shapes are those at which the kernels can go wrong: widths round a packed word, heights round a tile,
components on and across every seam of the tiles, one component that winds through every tile, the same inverted for the white
pass, pages of several sizes in one call, a record that is none, the pad bits."""
import functools

import numpy as np
import pytest

from tests import despeckle_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A


def _run(masks, n, **kw):
    from yomitoku_amd.despeckle import despeckle_masks

    return despeckle_masks(masks, black=n[0], white=n[1], **kw)


def _same(got, mask, n):
    from yomitoku_amd.despeckle import Despeckled

    clean, counts = R.despeckle(mask, *n)
    assert not isinstance(got, BaseException), got
    assert got[0].dtype == torch.bool and tuple(got[0].shape) == mask.shape
    assert (got[0].cpu().numpy() == clean).all(), (mask.shape, n, int((got[0].cpu().numpy() != clean).sum()))
    assert got[1] == Despeckled(n[0], n[1], *counts), (mask.shape, n)


def _tile():
    from yomitoku_amd.despeckle import tile

    return tile()


# ------------------------------------------------------------------------------------------------------- word and row edges
WIDTHS, HEIGHTS, DENSITIES = (1, 31, 32, 33, 63, 64, 65, 97), (1, 2, 15, 16, 17, 33), (0.1, 0.5)


@functools.lru_cache(maxsize=None)
def edge_masks():
    rng = np.random.default_rng(11)
    return [rng.random((h, w)) < d for w in WIDTHS for h in HEIGHTS for d in DENSITIES]


@pytest.mark.parametrize("n", [(1, 1), (4, 4), (0, 3), (5, 0)])
def test_word_and_row_edges(n):
    masks = edge_masks()
    for got, mask in zip(_run(masks, n), masks):
        _same(got, mask, n)


# ------------------------------------------------------------------------------------------------------- tile seams
def _seam_masks():
    tw, th = _tile()
    h, w = 2 * th + 1, 2 * tw + 1
    blocks = np.zeros((h, w), bool)  # a 2 x 2 block on every seam and on the four-tile corner
    for y, x in ((th - 1, 10), (th - 1, tw - 1), (5, tw - 1), (2 * th - 1, tw + 30), (th + 4, 2 * tw - 1), (2 * th - 1, 2 * tw - 1), (th - 1, tw + 20),
                 (th + 8, tw - 1)):
        blocks[y : y + 2, x : x + 2] = True
    pairs = np.zeros((h, w), bool)  # a diagonal pair, either way, across every seam
    for (y, x), (yy, xx) in (((th - 1, 20), (th, 21)), ((th - 1, 31), (th, 30)), ((3, tw - 1), (4, tw)), ((8, tw), (9, tw - 1)),
                             ((2 * th - 1, tw + 5), (2 * th, tw + 6)), ((2 * th - 1, tw + 15), (2 * th, tw + 14)),
                             ((th + 3, 2 * tw - 1), (th + 4, 2 * tw)), ((th + 9, 2 * tw), (th + 10, 2 * tw - 1)),
                             ((2 * th - 1, 2 * tw - 1), (2 * th, 2 * tw))):
        pairs[y, x] = pairs[yy, xx] = True
    down = np.zeros((h, w), bool)  # the corner's two diagonals, each on a page of its own
    down[th - 1, tw - 1] = down[th, tw] = True
    up = np.zeros((h, w), bool)
    up[th - 1, tw] = up[th, tw - 1] = True
    rng = np.random.default_rng(5)
    return [blocks, pairs, down, up, rng.random((h, w)) < 0.45, ~blocks, ~pairs, ~down, ~up]


@pytest.mark.parametrize("n", [(2, 2), (3, 3), (4, 4), (5, 5)])
def test_blocks_and_diagonal_pairs_on_every_seam(n):
    masks = _seam_masks()
    got = _run(masks, n)
    for g, mask in zip(got, masks):
        _same(g, mask, n)
    if n[0] == 2:  # a diagonal pair is one component of two pixels: it stays
        assert got[2][1].black_components == 0 and got[3][1].black_components == 0
    if n[0] == 3:
        assert (got[2][1].black_components, got[2][1].black_pixels) == (1, 2) and (got[3][1].black_components, got[3][1].black_pixels) == (1, 2)


@functools.lru_cache(maxsize=None)
def serpentines():
    """One-pixel-wide paths through a 5 x 5-tile page: rows joined at alternate ends (crosses every upright seam in every tile
    row), and columns joined at alternate ends (crosses every level seam in every tile column)."""
    tw, th = _tile()
    h, w = 5 * th, 5 * tw
    rows = np.zeros((h, w), bool)
    rows[0::2, :] = True
    for y in range(1, h - 1, 2):
        rows[y, w - 1 if (y // 2) % 2 == 0 else 0] = True
    cols = np.zeros((h, w), bool)
    cols[:, 0::2] = True
    for x in range(1, w - 1, 2):
        cols[h - 1 if (x // 2) % 2 == 0 else 0, x] = True
    return rows, cols


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("white", [False, True])
def test_a_serpentine_through_every_tile_is_kept_whole_and_removed_whole(which, white):
    path = serpentines()[which]
    area = int(path.sum())
    assert len(R.components(path, R.NEIGHBOURS_4)) == 1 and area + 1 <= 65535
    mask = ~path if white else path
    for n, gone in ((area - 1, False), (area + 1, True)):
        pair = (0, n) if white else (n, 0)
        got = _run([mask], pair)[0]
        _same(got, mask, pair)
        d = got[1]
        went = (d.white_components, d.white_pixels) if white else (d.black_components, d.black_pixels)
        assert went == ((1, area) if gone else (0, 0))
        assert bool(got[0].all() if white else not got[0].any()) == gone


# ------------------------------------------------------------------------------------------------------- mixed pages
@functools.lru_cache(maxsize=None)
def mixed_masks():
    rng = np.random.default_rng(23)
    return [rng.random(s) < d for s, d in (((257, 515), 0.3), ((1, 1), 0.5), ((40, 70), 0.6), ((17, 300), 0.1), ((130, 33), 0.5), ((1, 1), 0.0))]


@functools.lru_cache(maxsize=None)
def mixed_expected():
    return [R.despeckle(m, 4, 4) for m in mixed_masks()]


def _equal_to_expected(got, order):
    exp = mixed_expected()
    for g, k in zip(got, order):
        assert (g[0].cpu().numpy() == exp[k][0]).all(), k
        assert (g[1].black_components, g[1].black_pixels, g[1].white_components, g[1].white_pixels) == exp[k][1], k


def test_pages_of_several_sizes_in_one_call_and_refused_masks():
    masks = mixed_masks()
    got = _run(masks + [np.zeros((3, 3), np.uint8), np.zeros((2, 2, 2), bool), torch.zeros((0, 4), dtype=torch.bool)], (4, 4), scratch={})
    _equal_to_expected(got[: len(masks)], range(len(masks)))
    assert all(isinstance(e, ValueError) for e in got[len(masks):])
    assert got[5][0].cpu().numpy().all()  # the 1 x 1 white page: the rule taken literally


def test_the_result_depends_on_the_masks_alone():
    masks = mixed_masks()
    scratch = {}
    first = _run(masks, (4, 4), scratch=scratch)
    again = _run([torch.from_numpy(m).cuda() for m in masks], (4, 4), scratch=scratch)
    order = list(range(len(masks)))[::-1]
    turned = _run([masks[k] for k in order], (4, 4), scratch=scratch)
    _equal_to_expected(first, range(len(masks)))
    _equal_to_expected(again, range(len(masks)))
    _equal_to_expected(turned, order)


# ------------------------------------------------------------------------------------------------------- a record that is none
def _launched(masks, n, edit_table=None, buffers=None):
    """`despeckle.launch` on the packed masks, as despeckle_masks calls it -> per mask (clean, its four counts, its packed rows)."""
    from yomitoku_amd import despeckle

    test = despeckle._Masks(masks, torch.device("cuda"))
    counts = despeckle.launch(test, list(range(len(masks))), {"black": n[0], "white": n[1]}, {}, edit_table, buffers)
    torch.cuda.synchronize()
    four = counts[: 4 * len(masks)].view(-1, 4).tolist()
    return [(despeckle.unpack_rows(test.rows(j), masks[j].shape[1]), tuple(four[j]), test.rows(j)) for j in range(len(masks))]


def _poisoned(masks, guard=256):
    from yomitoku_amd.despeckle import scratch_sizes

    label_b, area_b = scratch_sizes([m.shape for m in masks])
    assert label_b == area_b and label_b <= 4 * sum(m.size for m in masks) + 4
    return tuple(torch.full((b // 4 + guard,), POISON, dtype=torch.int32, device="cuda") for b in (label_b, area_b)), label_b // 4


@pytest.mark.parametrize("word, value", [(2, 0), (2, 34), (3, 130), (3, 20000), (6, 1 << 20), (14, 1 << 20)])
def test_a_malformed_record_is_taken_as_absent_and_the_scratch_is_not_overrun(word, value):
    """h = 0; h and w one above the call's largest, which the grids would cover in part only; a side above 16383; packed rows
    and labels that would lie behind their buffers"""
    from yomitoku_amd.mrc import pack_mask

    rng = np.random.default_rng(3)
    masks = [rng.random(s) < 0.4 for s in ((33, 70), (20, 45), (18, 129))]
    buffers, named = _poisoned(masks)

    def no_page(rec):
        assert rec.shape == (3, 16) and rec[1, 2:4].tolist() == [20, 45]
        rec[1, word] = value

    got = _launched(masks, (4, 4), no_page, buffers)
    for k in (0, 2):
        clean, counts = R.despeckle(masks[k], 4, 4)
        assert (got[k][0].cpu().numpy() == clean).all() and got[k][1] == counts
    assert (got[1][0].cpu().numpy() == masks[1]).all() and got[1][1] == (0, 0, 0, 0)
    assert (got[1][2] == pack_mask(masks[1], "cuda")).all()
    at = masks[0].size  # the absent page's labels and areas: not written either
    for buf in buffers:
        assert (buf[named:] == POISON).all()
        assert (buf[at : at + masks[1].size] == POISON).all()


# ------------------------------------------------------------------------------------------------------- pad bits
@pytest.mark.parametrize("w", [1, 33, 70, 97])
def test_pad_bits_stay_zero_after_a_white_pass(w):
    h = 19
    rng = np.random.default_rng(w)
    masks = [np.zeros((h, w), bool), rng.random((h, w)) < 0.7]
    n = (0, 65535)  # every white component is filled: the pages end all black, the pad bits do not
    for got, mask in zip(_launched(masks, n), masks):
        clean, counts = R.despeckle(mask, *n)
        assert (got[0].cpu().numpy() == clean).all() and got[1] == counts
        assert got[0].all() and got[1][3] == int((~mask).sum())
        rows = got[2].cpu().numpy().view(np.uint32)
        pad = 32 * rows.shape[1] - w
        assert (rows[:, -1] & np.uint32((1 << pad) - 1) == 0).all()
        assert (rows[:, -1] >> np.uint32(pad) == (1 << (32 - pad)) - 1).all()
