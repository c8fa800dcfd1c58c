"""The device's separation of a page into an ink mask and two layers (yomitoku_amd/csrc/ymk_mrc.hip, yomitoku_amd/mrc.py) against
its definition, tests/mrc_ref.py - which tests/test_mrc_host.py holds to a literal loop.  Every comparison is exact: the flags, the
packed mask, every byte of the buffer the layers are written to - poisoned beforehand, so that what must not be written is seen
not to be - and the guard behind it.  The shapes are those at which the kernels can go wrong: a packed word plus a tail with the
dilation across the word boundary, clipped cells, a page smaller than a cell, one channel, several tiles each way; each alone and
all in one call, at three pairs of cells."""
import functools

import numpy as np
import pytest

from tests import ccitt_ref
from tests import mrc_ref as R
from tests.test_jpeg_gpu import _guard_ok, _guarded

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(45, 70, 3), (33, 65, 3), (3, 5, 3), (64, 96), (97, 130, 3)]
CELLS = [(1, 2), (2, 8), (16, 16)]
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def page(index):
    """strokes of a few pixels on noisy paper, each channel its own noise"""
    shape = SHAPES[index]
    rng = np.random.default_rng(100 + index)
    yy, xx = np.mgrid[0 : shape[0], 0 : shape[1]]
    ink = ((yy % 9 < 3) & (xx % 23 < 15)) ^ (rng.random(shape[:2]) < 0.02)
    base = np.where(ink, 45, 210) if len(shape) == 2 else np.where(ink[..., None], (60, 40, 150), (215, 225, 200))
    out = np.clip(base + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mask(index, kind):
    h, w = SHAPES[index][:2]
    rng = np.random.default_rng(7 * index + len(kind))
    m = np.zeros((h, w), bool)
    if kind in ("0.5", "0.999"):
        m = rng.random((h, w)) < float(kind)
    elif kind == "corner":
        m[h - 1, w - 1] = True
    elif kind == "borders":
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    elif kind == "block":
        m[20:60, 30:70] = True
    elif kind == "ink":
        m[:] = True
    else:
        assert kind == "white"
    return m


@functools.lru_cache(maxsize=None)
def expected(index, cells, kind=None):
    """(flag, M, foreground, background) by the definition - computed once"""
    return R.separate(page(index), cells[0], cells[1], None if kind is None else mask(index, kind))


def _run(dev, indices, cells, kinds=None, edit=None, absent=()):
    """separate the pages `indices` in one call into a poisoned buffer and hold everything it wrote to the definition"""
    from yomitoku_amd.mrc import launch, scratch_sizes

    pages = [page(i) for i in indices]
    sizes, places = scratch_sizes([p.shape for p in pages], *cells)
    layers = _guarded(sizes[4], dev)
    tensors = [torch.from_numpy(np.array(p)).to(dev) for p in pages]
    masks = None if kinds is None else [mask(i, k) for i, k in zip(indices, kinds)]
    done = launch(tensors, {"bg_cell": cells[0], "fg_cell": cells[1]}, {}, masks=masks, layers=layers, edit_table=edit)
    torch.cuda.synchronize()
    assert _guard_ok(layers, sizes[4])
    want = np.full(sizes[4], POISON, np.uint8)
    flags = done.flags()
    for j, i in enumerate(indices):
        if j in absent:
            assert flags[j] == -1, (i, cells)
            continue
        flag, M, fg, bg = expected(i, cells, None if kinds is None else kinds[j])
        assert flags[j] == flag, (i, cells, kinds)
        assert (done.mask_rows(j).cpu().numpy().view(np.uint32) == ccitt_ref.pack_rows(M)).all(), (i, cells, kinds)
        if flag == 1:
            want[places[j][1] : places[j][1] + fg.size] = fg.reshape(-1)
            want[places[j][2] : places[j][2] + bg.size] = bg.reshape(-1)
            assert done.foreground(j).shape == fg.shape and done.background(j).shape == bg.shape
            assert done.foreground(j).cpu().numpy().tobytes() == fg.tobytes(), (i, cells, kinds)
            assert done.background(j).cpu().numpy().tobytes() == bg.tobytes(), (i, cells, kinds)
    # every byte: the layers where the flag is 1; the poison in the gaps between them and where no layer is written
    assert layers[: sizes[4]].cpu().numpy().tobytes() == want.tobytes(), (indices, cells, kinds)
    return flags


@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("indices", [(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)])
def test_the_separation_equals_the_definition(dev, indices, cells):
    flags = _run(dev, indices, cells)
    if 4 in indices:
        assert flags[-1] == 1  # the pages are not all trivially unlayered


@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("kind", ["0.5", "0.999", "corner", "borders"])
def test_masks_handed_in(dev, kind, cells):
    """random masks at two densities (0.999: almost nothing is paper, and the dilation leaves less), one ink pixel in a corner -
    the whole foreground is pushed from the top -, ink on all four borders"""
    _run(dev, (0, 1, 2, 3, 4), cells, kinds=[kind] * 5)


@pytest.mark.parametrize("cells", CELLS)
def test_a_solid_block_is_pushed_over_several_levels(dev, cells):
    flag, _, fg, bg = expected(4, cells, "block")
    assert flag == 1
    _run(dev, (4,), cells, kinds=["block"])


@pytest.mark.parametrize("cells", CELLS)
def test_pages_without_ink_or_without_paper_get_no_layers(dev, cells):
    """flag 0, and not a byte of the poisoned buffer is written - beside a page that is layered as ever"""
    flags = _run(dev, (0, 1, 4, 3), cells, kinds=["white", "ink", "block", "ink"])
    assert flags == [0, 0, 1, 0]


@pytest.mark.parametrize("kinds", [None, ["0.5", "block", "borders"]])
def test_a_malformed_record_is_absent_and_the_others_are_right(dev, kinds):
    def edit(rec):
        rec[1, 2] = 0  # h = 0: no page

    assert _run(dev, (0, 4, 1), (2, 8), kinds=kinds, edit=edit, absent=(1,))[1] == -1

    def far(rec):
        rec[1, 5] = 1 << 30  # pyramids outside the stated buffer

    assert _run(dev, (0, 4, 1), (2, 8), kinds=kinds, edit=far, absent=(1,))[1] == -1


def test_separate_pages_on_host_arrays_and_device_tensors(dev):
    from yomitoku_amd.mrc import separate_pages

    pages = [np.array(page(i)) for i in range(5)]
    scratch = {}
    got = separate_pages(pages + [np.zeros((4, 4), np.float32)], scratch=scratch)
    assert isinstance(got[-1], ValueError)
    again = separate_pages([torch.from_numpy(p).to(dev) for p in pages], {"bg_cell": 1, "fg_cell": 2}, scratch=scratch)
    handed = separate_pages(pages, True, masks=[mask(i, "borders") for i in range(5)])
    for i in range(5):
        for entry, cells, kind in ((got[i], (2, 8), None), (again[i], (1, 2), None), (handed[i], (2, 8), "borders")):
            flag, M, fg, bg = expected(i, cells, kind)
            assert entry[0] == flag and entry[1].dtype == torch.int32 and entry[1].device.type == "cuda"
            assert (entry[1].cpu().numpy().view(np.uint32) == ccitt_ref.pack_rows(M)).all()
            if flag == 1:
                assert entry[2].cpu().numpy().tobytes() == fg.tobytes() and entry[3].cpu().numpy().tobytes() == bg.tobytes()
                assert tuple(entry[2].shape) == fg.shape and tuple(entry[3].shape) == bg.shape
            else:
                assert entry[2] is None and entry[3] is None
    with pytest.raises(ValueError):
        separate_pages(pages[:1], mrc="yes")
    assert isinstance(separate_pages(pages[:1], masks=[np.zeros((2, 2), bool)])[0], ValueError)


def test_the_library_refuses_bad_arguments(dev):
    from yomitoku_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream_ptr()
    buf = torch.zeros(4096, dtype=torch.int32, device=dev)
    b = buf.data_ptr()
    assert lib.ymk_mrc_cells(b, 15, 1, 8, 8, 2, 8, b, 64, b, 64, 64, stream) != 0  # a table of fewer words than a record
    assert lib.ymk_mrc_cells(b, 16, 1, 8, 8, 3, 8, b, 64, b, 64, 64, stream) != 0  # a cell that is no power of two
    assert lib.ymk_mrc_pull(b, 16, 1, 8, 8, 2, 32, 64, b, 64, 64, stream) != 0
    assert lib.ymk_mrc_push(b, 16, 1, 8, 8, 2, 8, 64, b, 64, b, 64, None, stream) != 0  # no flags
    assert lib.ymk_mrc_cells(b, 16, 1, 0, 8, 2, 8, b, 64, b, 64, 64, stream) != 0
    assert lib.ymk_last_error()
    assert lib.ymk_mrc_pages(b, 16, 0, 1, 1, 2, 8, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, stream) == 0  # no pages
    torch.cuda.synchronize()
