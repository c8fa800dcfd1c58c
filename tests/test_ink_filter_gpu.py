"""The device's ink filter (yomitoku_amd/csrc/ymk_cc.hip: ymk_cc_filter_pages; yomitoku_amd/despeckle.py: filter_masks) against its
definition, tests/ink_filter_ref.py - which tests/test_ink_filter_host.py holds to scipy.  Every comparison is exact: the clean mask
bit for bit and the six counts.  The shapes are those at which the blob pass can go wrong: widths with odd and even word counts a
row, so that a wave's two words lie on one row or on two; heights round a tile; components whose box is the page and whose area is
not; both equalities of the rule; several pages in one call; scratch that is not zero; a record that is none."""
import functools

import numpy as np
import pytest

from tests import despeckle_ref
from tests import ink_filter_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A


def _run(masks, p, **kw):
    from yomitoku_amd.despeckle import filter_masks

    return filter_masks(masks, black=p[0], white=p[1], side=p[2], fill=p[3], **kw)


def _record(p, six):
    from yomitoku_amd.despeckle import InkFiltered

    return InkFiltered(p[0], p[1], p[2], p[3] if p[2] else 0, *six)


def _same(got, mask, p):
    clean, six = R.filter_ink(mask, *p)
    assert not isinstance(got, BaseException), got
    assert got[0].dtype == torch.bool and tuple(got[0].shape) == mask.shape
    assert (got[0].cpu().numpy() == clean).all(), (mask.shape, p, int((got[0].cpu().numpy() != clean).sum()))
    assert got[1] == _record(p, six), (mask.shape, p, got[1], six)
    return six


# ------------------------------------------------------------------------------------------------------- word and row edges
WIDTHS, HEIGHTS, DENSITIES = (1, 31, 32, 33, 64, 65, 97), (1, 16, 17, 33), (0.3, 0.45, 0.6)


@functools.lru_cache(maxsize=None)
def edge_masks():
    rng = np.random.default_rng(29)
    return [rng.random((h, w)) < d for w in WIDTHS for h in HEIGHTS for d in DENSITIES]


@pytest.mark.parametrize("p", [(0, 0, 2, 64), (0, 0, 3, 100), (4, 4, 4, 96), (2, 3, 2, 160), (0, 0, 2, 1)])
def test_word_and_row_edges(p):
    masks = edge_masks()
    went = 0
    for got, mask in zip(_run(masks, p), masks):
        went += _same(got, mask, p)[4]
    assert went >= 20  # many components qualify: the rule is exercised, not skipped


# ------------------------------------------------------------------------------------------------------- the rule's equalities
def _block(h, w, y, x, bh, bw):
    m = np.zeros((h, w), bool)
    m[y : y + bh, x : x + bw] = True
    return m


@pytest.mark.parametrize("x", [3, 28, 60])  # inside a word, across two words, across the tiles' seam
def test_both_equalities_of_the_rule(x):
    full = _block(24, 97, 14, x, 4, 8)  # 256 * 32 == 256 * 4 * 8
    less = full.copy()
    less[15, x + 2] = False  # 31 pixels in the same box
    for mask, p, gone in ((full, (0, 0, 4, 256), (1, 32)), (less, (0, 0, 4, 256), (0, 0)), (less, (0, 0, 4, 248), (1, 31)),
                          (less, (0, 0, 4, 249), (0, 0)), (full, (0, 0, 5, 1), (0, 0)), (full.T.copy(), (0, 0, 5, 1), (0, 0)),
                          (full.T.copy(), (0, 0, 4, 256), (1, 32))):
        assert _same(_run([mask], p)[0], mask, p)[4:] == gone, (x, p)


# ------------------------------------------------------------------------------------------------------- page-sized components
@functools.lru_cache(maxsize=None)
def wound():
    """On a 33 x 130 page, 3 x 3 tiles: its one-pixel frame; a one-pixel path along every fourth row, joined at alternate ends,
    which passes through every tile; the page all black.  Each is one component whose box is the page."""
    h, w = 33, 130
    ring = np.zeros((h, w), bool)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
    path = np.zeros((h, w), bool)
    path[0::4, :] = True
    for k, y in enumerate(range(0, h - 4, 4)):
        path[y : y + 4, w - 1 if k % 2 == 0 else 0] = True
    return ring, path, np.ones((h, w), bool)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_component_as_large_as_the_page_has_its_true_area_and_box(which):
    mask = wound()[which]
    h, w = mask.shape
    area = int(mask.sum())
    assert len(despeckle_ref.components(mask, despeckle_ref.NEIGHBOURS_8)) == 1
    fill = 256 * area // (h * w)  # the largest fill at which it still goes
    cases = [((0, 0, 33, fill), True), ((0, 0, 34, 1), False)]  # the box is exactly 33 high
    if fill < 256:
        cases.append(((0, 0, 33, fill + 1), False))
    for p, gone in cases:
        got = _run([mask], p)[0]
        assert _same(got, mask, p)[4:] == ((1, area) if gone else (0, 0)), (which, p)
        assert bool(not got[0].any()) == gone


def test_a_solid_block_across_the_four_tile_corner():
    mask = _block(40, 140, 10, 58, 12, 12)  # rows 10..21 across y = 16, columns 58..69 across x = 64
    mask[3, 3] = mask[30, 100] = True
    for p, gone in (((0, 0, 12, 256), (1, 144)), ((0, 0, 13, 1), (0, 0)), ((2, 0, 12, 256), (1, 144))):
        assert _same(_run([mask], p)[0], mask, p)[4:] == gone


def test_pinholes_are_filled_before_the_blob_is_measured():
    mask = _block(30, 80, 6, 20, 16, 50)
    mask[8, 25] = mask[15, 64] = mask[16, 64] = False  # pinholes of 1 and 2 pixels, one across the tiles' seam
    filled = _same(_run([mask], (0, 4, 16, 256))[0], mask, (0, 4, 16, 256))
    assert filled == (0, 0, 2, 3, 1, 800)
    assert _same(_run([mask], (0, 0, 16, 256))[0], mask, (0, 0, 16, 256))[4:] == (0, 0)  # with its holes it does not fill its box


# ------------------------------------------------------------------------------------------------------- mixed pages
PARAMS = (4, 4, 3, 90)


@functools.lru_cache(maxsize=None)
def mixed_masks():
    rng = np.random.default_rng(31)
    return [rng.random(s) < d for s, d in (((65, 259), 0.35), ((1, 1), 1.0), ((40, 70), 0.6), ((17, 300), 0.3), ((130, 33), 0.5), ((3, 3), 1.0))]


@functools.lru_cache(maxsize=None)
def mixed_expected():
    return [R.filter_ink(m, *PARAMS) for m in mixed_masks()]


def _equal_to_expected(got, order):
    exp = mixed_expected()
    for g, k in zip(got, order):
        assert (g[0].cpu().numpy() == exp[k][0]).all(), k
        assert g[1] == _record(PARAMS, exp[k][1]), k


def test_pages_of_several_sizes_in_one_call_and_refused_masks():
    masks = mixed_masks()
    got = _run(masks + [np.zeros((3, 3), np.uint8), np.zeros((2, 2, 2), bool)], PARAMS, scratch={})
    _equal_to_expected(got[: len(masks)], range(len(masks)))
    assert all(isinstance(e, ValueError) for e in got[len(masks):])
    assert got[5][1].blob_components == 1 and not got[5][0].any()  # the 3 x 3 black page is a blob of side 3
    assert sum(e[1][4] for e in mixed_expected()) >= 5
    with pytest.raises(ValueError):
        _run(masks[:1], (0, 0, 0, 64))
    with pytest.raises(ValueError):
        _run(masks[:1], (4, 4, 1, 64))


def test_the_result_depends_on_the_masks_alone():
    masks = mixed_masks()
    scratch = {}
    first = _run(masks, PARAMS, scratch=scratch)
    order = list(range(len(masks)))[::-1]
    turned = _run([torch.from_numpy(masks[k]).cuda() for k in order], PARAMS, scratch=scratch)
    _equal_to_expected(first, range(len(masks)))
    _equal_to_expected(turned, order)


def test_side_zero_is_despeckle_masks_bit_for_bit():
    from yomitoku_amd.despeckle import despeckle_masks

    masks = mixed_masks()
    plain = despeckle_masks(masks, black=4, white=4)
    for got, want, mask in zip(_run(masks, (4, 4, 0, 64)), plain, masks):
        assert torch.equal(got[0], want[0])
        d, f = want[1], got[1]
        assert (f.black, f.white, f.side, f.fill) == (4, 4, 0, 0)
        assert (f.black_components, f.black_pixels, f.white_components, f.white_pixels) == (d.black_components, d.black_pixels,
                                                                                            d.white_components, d.white_pixels)
        assert (f.blob_components, f.blob_pixels) == (0, 0)


# ------------------------------------------------------------------------------------------------------- scratch and records
def _launched(masks, p, edit_table=None, buffers=None):
    """`despeckle.launch_filter` on the packed masks, as filter_masks calls it -> per mask (clean, its six counts, its rows)."""
    from yomitoku_amd import despeckle

    test = despeckle._Masks(masks, torch.device("cuda"))
    params = {"black": p[0], "white": p[1], "side": p[2], "fill": p[3]}
    counts = despeckle.launch_filter(test, list(range(len(masks))), params, {}, edit_table, buffers)
    torch.cuda.synchronize()
    six = counts[: 6 * len(masks)].view(-1, 6).tolist()
    return [(despeckle.unpack_rows(test.rows(j), masks[j].shape[1]), tuple(six[j]), test.rows(j)) for j in range(len(masks))]


def _poisoned(masks, guard=256):
    from yomitoku_amd.despeckle import filter_scratch_sizes

    sizes = filter_scratch_sizes([m.shape for m in masks])
    pixels = sum(m.size for m in masks)
    assert sizes[0] == sizes[1] and sizes[2] == 3 * sizes[0] and 4 * pixels <= sizes[0] <= 4 * pixels + 4  # 20 bytes a pixel
    return tuple(torch.full((b // 4 + guard,), POISON, dtype=torch.int32, device="cuda") for b in sizes), [b // 4 for b in sizes]


def test_scratch_that_is_not_zero_changes_nothing_and_is_not_overrun():
    masks = mixed_masks()
    buffers, named = _poisoned(masks)
    exp = mixed_expected()
    for k, got in enumerate(_launched(masks, PARAMS, None, buffers)):
        assert (got[0].cpu().numpy() == exp[k][0]).all() and got[1] == exp[k][1], k
    for buf, words in zip(buffers, named):
        assert (buf[words:] == POISON).all()


@pytest.mark.parametrize("word, value", [(2, 0), (2, 34), (3, 130), (3, 20000), (6, 1 << 20), (14, 1 << 20)])
def test_a_malformed_record_is_taken_as_absent_and_the_scratch_is_not_overrun(word, value):
    """h = 0; h and w one above the call's largest, which the grids would cover in part only; a side above 16383; packed rows
    and labels that would lie behind their buffers"""
    from yomitoku_amd.mrc import pack_mask

    rng = np.random.default_rng(3)
    masks = [rng.random(s) < 0.4 for s in ((33, 70), (20, 45), (18, 129))]
    buffers, named = _poisoned(masks)
    p = (4, 4, 3, 90)

    def no_page(rec):
        assert rec.shape == (3, 16) and rec[1, 2:4].tolist() == [20, 45]
        rec[1, word] = value

    got = _launched(masks, p, no_page, buffers)
    for k in (0, 2):
        clean, six = R.filter_ink(masks[k], *p)
        assert (got[k][0].cpu().numpy() == clean).all() and got[k][1] == six
        assert six[4] >= 1
    assert (got[1][0].cpu().numpy() == masks[1]).all() and got[1][1] == (0, 0, 0, 0, 0, 0)
    assert (got[1][2] == pack_mask(masks[1], "cuda")).all()
    at, size = masks[0].size, masks[1].size  # the absent page's labels, areas and boxes: not written either
    for buf, words in zip(buffers[:2], named):
        assert (buf[words:] == POISON).all()
        assert (buf[at : at + size] == POISON).all()
    assert (buffers[2][named[2]:] == POISON).all()
    assert (buffers[2][3 * at : 3 * (at + size)] == POISON).all()


def test_boxes_that_are_too_small_for_a_page_make_it_absent():
    """the third buffer bounds a page's place like the first two: stated one word short, the last page is none"""
    from yomitoku_amd import _lib, despeckle, imaging

    rng = np.random.default_rng(9)
    masks = [rng.random((20, 40)) < 0.5, rng.random((10, 64)) < 0.5]
    buffers, named = _poisoned(masks)
    test = despeckle._Masks(masks, torch.device("cuda"))
    blob = despeckle.page_table([m.shape for m in masks], test.packed_at)
    blob_dev = imaging._stage_blob(blob.reshape(-1), test.packed.device)
    counts = torch.zeros(12, dtype=torch.int32, device="cuda")
    pixels = sum(m.size for m in masks)
    _lib.check(_lib.load().ymk_cc_filter_pages(blob_dev.data_ptr(), blob.size, 2, 20, 64, test.packed.data_ptr(), test.packed_bytes,
                                               buffers[0].data_ptr(), 4 * pixels, buffers[1].data_ptr(), 4 * pixels, buffers[2].data_ptr(),
                                               12 * pixels - 4, 0, 0, 2, 64, counts.data_ptr(), _lib.current_stream_ptr()), "ymk_cc_filter_pages")
    torch.cuda.synchronize()
    clean, six = R.filter_ink(masks[0], 0, 0, 2, 64)
    assert (despeckle.unpack_rows(test.rows(0), 40).cpu().numpy() == clean).all() and tuple(counts[:6].tolist()) == six
    assert (despeckle.unpack_rows(test.rows(1), 64).cpu().numpy() == masks[1]).all() and counts[6:].tolist() == [0] * 6
    assert (buffers[2][3 * masks[0].size :] == POISON).all()
