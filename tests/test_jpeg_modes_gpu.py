"""The device JPEG encoder's per-page modes - 4:2:2 and 4:4:4 chroma, the grey file of a grey-valued colour page, the grey test
(yomitoku_amd/csrc/ymk_jpeg.hip, yomitoku_amd/jpeg.py) - against their definition, tests/jpeg_modes_ref.py.  Everything is
integer arithmetic: every comparison is exact."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_modes_ref, jpeg_ref
from tests.test_jpeg_gpu import _guard_ok, _guarded, _noise
from tests.test_jpeg_host import synthetic_page

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODES = ["4:2:2", "4:4:4"]


class ModeWave:
    """Colour pages on the device in one mode, their page table and guarded scratch, driven through the C ABI."""

    def __init__(self, pages, quality, subsampling):
        from yomitoku_amd import _lib
        from yomitoku_amd.jpeg import SUBSAMPLINGS, page_table, scratch_sizes

        self.lib, self.check = _lib.load(), _lib.check
        self.dev = torch.device("cuda:0")
        self.pages = [np.ascontiguousarray(p) for p in pages]
        self.tensors = [torch.from_numpy(p).to(self.dev) for p in self.pages]
        modes = [SUBSAMPLINGS[subsampling]] * len(pages)
        blob, self.offsets, self.out_bytes = page_table(self.tensors, quality, [4 * p.size + 2048 for p in self.pages], modes=modes)
        self.blob = torch.from_numpy(blob).to(self.dev)
        self.tiles, self.blocks, self.intervals, self.coef_b, self.stream_b, self.iv_b = scratch_sizes([p.shape for p in self.pages], modes=modes)
        self.sizes = {"coef": self.coef_b, "stream": self.stream_b, "iv": self.iv_b, "out": self.out_bytes, "len": 4 * len(pages)}
        self.buf = {k: _guarded(n, self.dev) for k, n in self.sizes.items()}
        self.stream = torch.cuda.current_stream().cuda_stream

    def ptr(self, key):
        return self.buf[key].data_ptr()

    def coefficients(self):
        self.check(self.lib.ymk_jpeg_coefficients(self.blob.data_ptr(), self.blob.numel(), len(self.pages), self.tiles, self.ptr("coef"),
                                                  self.blocks, self.stream), "ymk_jpeg_coefficients")
        torch.cuda.synchronize()
        return self.buf["coef"][: self.coef_b].cpu().numpy().view(np.int16).reshape(-1, 64)

    def encode(self):
        self.check(self.lib.ymk_jpeg_encode_pages(self.blob.data_ptr(), self.blob.numel(), len(self.pages), self.tiles, self.blocks,
                                                  self.intervals, self.ptr("coef"), self.ptr("stream"), self.stream_b, self.ptr("iv"),
                                                  self.ptr("out"), self.out_bytes, self.ptr("len"), self.stream), "ymk_jpeg_encode_pages")
        torch.cuda.synchronize()
        lengths = self.buf["len"][: 4 * len(self.pages)].cpu().numpy().view(np.int32).tolist()
        out = self.buf["out"].cpu().numpy()
        return [None if n < 0 else out[o : o + n].tobytes() for o, n in zip(self.offsets, lengths)]

    def guards_ok(self):
        return all(_guard_ok(self.buf[k], n) for k, n in self.sizes.items())


@pytest.mark.parametrize("subsampling", MODES)
@pytest.mark.parametrize("shape", [(1, 1, 3), (8, 8, 3), (9, 23, 3), (16, 16, 3), (33, 17, 3), (40, 200, 3)], ids=str)
def test_coefficients_equal_the_definition(shape, subsampling):
    """One pixel; one 4:4:4 MCU, half a 4:2:2 one; a row pitch that is no multiple of 16 with both edges ragged; one 16 x 16 tile
    of two or four MCUs; tiles whose second MCU row or column is not the page's; 13 tiles across, 52 or 75 blocks per MCU row."""
    for quality, page in ((85, synthetic_page(shape[0], shape[1], seed=1)), (100, _noise(shape, 2))):
        wave = ModeWave([page], quality, subsampling)
        got = wave.coefficients()
        assert np.array_equal(got, jpeg_modes_ref.coefficients(page, quality, subsampling)), (shape, quality)
        assert wave.guards_ok()


FILES = {
    "444_ten_intervals": ((80, 8, 3), "4:4:4"),     # RSTm wraps
    "444_66_blocks": ((8, 176, 3), "4:4:4"),        # one interval of 66 blocks: DC prediction crosses the 64-block chunk inside an MCU
    "422_68_blocks": ((8, 272, 3), "4:2:2"),        # one interval of 68 blocks
    "444_ragged": ((37, 53, 3), "4:4:4"),
    "422_ragged": ((37, 53, 3), "4:2:2"),
}


@pytest.mark.parametrize("optimize", [False, True], ids=["plain", "optimize"])
@pytest.mark.parametrize("name", list(FILES))
def test_whole_files_equal_the_definition(name, optimize):
    from yomitoku_amd.jpeg import encode_jpeg_pages

    shape, subsampling = FILES[name]
    for page in (synthetic_page(shape[0], shape[1], seed=4), _noise(shape, 6)):
        want = jpeg_modes_ref.encode(page, 85, subsampling, optimize=optimize)
        if name == "444_ten_intervals":
            assert want.count(b"\xff\xd0") >= 2 and b"\xff\xd7" in want
        (got,) = encode_jpeg_pages([page], "high", capacities=[4 * page.size + 2048], optimize=optimize, subsampling=subsampling)
        assert got.data == want and got.optimized == optimize and got.subsampling == subsampling and not got.grey
        if not optimize:  # the same through the C ABI, every buffer guarded
            wave = ModeWave([page], 85, subsampling)
            assert wave.encode() == [want] and wave.guards_ok()
        image = Image.open(io.BytesIO(got.data))
        image.load()
        assert image.size == (shape[1], shape[0]) and image.mode == "RGB"


def _flat(plane):
    return np.ascontiguousarray(np.stack([plane, plane, plane], -1))


@pytest.mark.parametrize("optimize", [False, True], ids=["plain", "optimize"])
def test_one_call_over_five_pages_444_and_auto_grey(optimize):
    from yomitoku_amd.jpeg import encode_jpeg_pages

    pages = [synthetic_page(48, 64, seed=1), _flat(synthetic_page(40, 56, seed=2, grey=True)), synthetic_page(23, 9, seed=3, grey=True),
             _noise((1, 1, 3), 5), synthetic_page(33, 23, seed=6)]
    pages[3][0, 0, 1] = pages[3][0, 0, 0] ^ 1  # one pixel, and it is coloured
    got = encode_jpeg_pages(pages, "high", capacities=[4 * p.size + 2048 for p in pages], optimize=optimize, subsampling="4:4:4", grey="auto")
    assert [(g.grey, g.subsampling) for g in got] == [(False, "4:4:4"), (True, None), (True, None), (False, "4:4:4"), (False, "4:4:4")]
    for page, g in zip(pages, got):
        assert g.data == jpeg_modes_ref.encode(page, 85, "4:4:4", grey="auto", optimize=optimize)
        assert (g.width, g.height, g.optimized, g.scale) == (page.shape[1], page.shape[0], optimize, 1.0)
        image = Image.open(io.BytesIO(g.data))
        image.load()
        assert image.size == (page.shape[1], page.shape[0]) and image.mode == ("L" if g.grey else "RGB")
    if not optimize:
        assert got[1].data == jpeg_ref.encode(pages[1][..., 0], 85)
    # the same pages without grey="auto": the grey-valued one is a colour file
    again = encode_jpeg_pages(pages, "high", capacities=[4 * p.size + 2048 for p in pages], optimize=optimize, subsampling="4:2:2")
    assert [(g.grey, g.subsampling) for g in again] == [(False, "4:2:2"), (False, "4:2:2"), (True, None), (False, "4:2:2"), (False, "4:2:2")]
    for page, g in zip(pages, again):
        assert g.data == jpeg_modes_ref.encode(page, 85, "4:2:2", optimize=optimize)


@pytest.mark.parametrize("w", [23, 64])
def test_the_grey_test_alone(w):
    """h = 9: 207 pixels are twelve groups of sixteen and a tail of fifteen, 576 are thirty-six groups and no tail - the last
    pixel is looked at by the tail's loop or by the wide loads' last byte."""
    from yomitoku_amd.jpeg import grey_pages

    dev = torch.device("cuda:0")
    grey = _flat(synthetic_page(9, w, seed=7, grey=True))
    last = grey.copy()
    last[-1, -1, 2] = np.uint8((int(last[-1, -1, 2]) + 1) & 255)
    first_row = grey.copy()
    first_row[0, w // 2, 0] ^= 0x80
    big = _flat(synthetic_page(300, 400, seed=8, grey=True))  # eight workgroups
    big_green = big.copy()
    big_green[171, 333, 1] ^= 1
    pages = [grey, last, first_row, big, big_green, grey[..., 0].copy()]
    tensors = [torch.from_numpy(p).to(dev) for p in pages]
    assert grey_pages(tensors) == [True, False, False, True, False, False]
    # the same pixels at an address that is not 16-byte aligned: every pixel goes through the tail's loop
    shifted = []
    for p in pages[:5]:
        buf = torch.zeros(p.size + 16, dtype=torch.uint8, device=dev)
        buf[1 : 1 + p.size] = torch.from_numpy(p.reshape(-1)).to(dev)
        shifted.append(buf[1 : 1 + p.size].view(p.shape))
        assert shifted[-1].data_ptr() % 16 == 1 and shifted[-1].is_contiguous()
    assert grey_pages(shifted) == [True, False, False, True, False]
    assert grey_pages([tensors[5]]) == [False] and grey_pages([]) == []


def test_the_defaults_still_give_jpeg_refs_bytes():
    from yomitoku_amd.jpeg import encode_jpeg, encode_jpeg_pages

    pages = [synthetic_page(48, 64, seed=1), _flat(synthetic_page(40, 56, seed=2, grey=True)), synthetic_page(23, 9, seed=3, grey=True),
             synthetic_page(33, 23, seed=6)]
    caps = [4 * p.size + 2048 for p in pages]
    for got in (encode_jpeg_pages(pages, "high", capacities=caps), encode_jpeg_pages(pages, "high", capacities=caps, subsampling="4:2:0", grey=False)):
        for page, g in zip(pages, got):
            assert g.data == jpeg_ref.encode(page, 85) and g.grey == (page.ndim == 2) and g.subsampling == (None if page.ndim == 2 else "4:2:0")
    # 4:2:0 with grey="auto": only the grey-valued page's file changes
    auto = encode_jpeg_pages(pages, "high", capacities=caps, grey="auto")
    assert [g.data for g in auto] == [jpeg_ref.encode(pages[0], 85), jpeg_ref.encode(pages[1][..., 0], 85), jpeg_ref.encode(pages[2], 85),
                                      jpeg_ref.encode(pages[3], 85)]
    one = synthetic_page(120, 160, seed=9)
    assert encode_jpeg(one, "high", subsampling="4:2:2").data == jpeg_modes_ref.encode(one, 85, "4:2:2")


def test_a_444_noise_page_over_its_capacity_fails_alone():
    """The default capacity is the page's raw byte count, 768 bytes at 16 x 16: the header's ~620 and three blocks of noise per
    MCU at quality 85 are more than that (the definition says by how much)."""
    from yomitoku_amd import _lib
    from yomitoku_amd.jpeg import encode_jpeg_pages

    pages = [synthetic_page(48, 64, seed=1), _noise((16, 16, 3), 2), _flat(synthetic_page(40, 56, seed=3, grey=True))]
    want = [jpeg_modes_ref.encode(p, 85, "4:4:4", grey="auto") for p in pages]
    assert len(want[1]) > pages[1].size and len(want[0]) <= pages[0].size and len(want[2]) <= pages[2].size
    got = encode_jpeg_pages(pages, "high", subsampling="4:4:4", grey="auto")
    assert isinstance(got[1], _lib.YmkError) and "capacity" in str(got[1])
    assert got[0].data == want[0] and got[2].data == want[2] and got[2].grey
    roomy = encode_jpeg_pages(pages, "high", subsampling="4:4:4", grey="auto", capacities=[p.size for p in pages[:1]] + [len(want[1])] + [pages[2].size])
    assert [g.data for g in roomy] == want
