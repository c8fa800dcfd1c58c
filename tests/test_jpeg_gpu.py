"""The device JPEG encoder (yomitoku_amd/csrc/ymk_jpeg.hip, yomitoku_amd/jpeg.py) against its definition, tests/jpeg_ref.py.
Everything is integer arithmetic: every comparison is exact."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_ref
from tests.test_jpeg_host import synthetic_page

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64  # bytes of 0xA5 behind every buffer the library writes


def _guarded(nbytes, dev):
    buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    return buf


def _guard_ok(buf, nbytes):
    return bool((buf[nbytes:] == 0xA5).all().item())


class Wave:
    """Pages on the device, their page table and guarded scratch, driven stage by stage through the C ABI."""

    def __init__(self, pages, quality, capacities=None):
        from yomitoku_amd import _lib
        from yomitoku_amd.jpeg import page_table, scratch_sizes

        self.lib, self.check = _lib.load(), _lib.check
        self.dev = torch.device("cuda:0")
        self.pages = [np.ascontiguousarray(p) for p in pages]
        self.tensors = [torch.from_numpy(p).to(self.dev) for p in self.pages]
        self.quality = quality
        if capacities is None:  # room for any file: noise at quality 100 outgrows the default, the page's raw byte count
            capacities = [4 * p.size + 2048 for p in self.pages]
        blob, self.offsets, self.out_bytes = page_table(self.tensors, quality, capacities)
        self.caps = [int(blob[k * 16 + 10]) for k in range(len(pages))]
        self.blob = torch.from_numpy(blob).to(self.dev)
        shapes = [(p.shape[0], p.shape[1], 1 if p.ndim == 2 else 3) for p in self.pages]
        self.mcus, self.blocks, self.intervals, self.coef_b, self.stream_b, self.iv_b = scratch_sizes(shapes)
        self.sizes = {"coef": self.coef_b, "stream": self.stream_b, "iv": self.iv_b, "out": self.out_bytes, "len": 4 * len(pages)}
        self.buf = {k: _guarded(n, self.dev) for k, n in self.sizes.items()}
        self.stream = torch.cuda.current_stream().cuda_stream

    def ptr(self, key):
        return self.buf[key].data_ptr()

    def coefficients(self):
        self.check(self.lib.ymk_jpeg_coefficients(self.blob.data_ptr(), self.blob.numel(), len(self.pages), self.mcus, self.ptr("coef"),
                                                  self.blocks, self.stream), "ymk_jpeg_coefficients")
        torch.cuda.synchronize()
        return self.buf["coef"][: self.coef_b].cpu().numpy().view(np.int16).reshape(-1, 64)

    def set_coefficients(self, coefs):
        raw = np.ascontiguousarray(coefs, dtype=np.int16).reshape(-1).view(np.uint8)
        assert raw.size == self.coef_b
        self.buf["coef"][: self.coef_b] = torch.from_numpy(raw.copy()).to(self.dev)

    def entropy_and_compact(self):
        n = len(self.pages)
        self.check(self.lib.ymk_jpeg_entropy(self.blob.data_ptr(), self.blob.numel(), n, self.ptr("coef"), self.blocks, self.ptr("stream"),
                                             self.stream_b, self.ptr("iv"), self.intervals, self.stream), "ymk_jpeg_entropy")
        self.check(self.lib.ymk_jpeg_compact(self.blob.data_ptr(), self.blob.numel(), n, self.ptr("stream"), self.stream_b, self.blocks,
                                             self.ptr("iv"), self.intervals, self.ptr("out"), self.out_bytes, self.ptr("len"),
                                             self.stream), "ymk_jpeg_compact")
        return self.files()

    def encode(self):
        self.check(self.lib.ymk_jpeg_encode_pages(self.blob.data_ptr(), self.blob.numel(), len(self.pages), self.mcus, self.blocks,
                                                  self.intervals, self.ptr("coef"), self.ptr("stream"), self.stream_b, self.ptr("iv"),
                                                  self.ptr("out"), self.out_bytes, self.ptr("len"), self.stream), "ymk_jpeg_encode_pages")
        return self.files()

    def files(self):
        torch.cuda.synchronize()
        lengths = self.buf["len"][: 4 * len(self.pages)].cpu().numpy().view(np.int32).tolist()
        out = self.buf["out"].cpu().numpy()
        return [None if n < 0 else out[o : o + n].tobytes() for o, n in zip(self.offsets, lengths)], out

    def guards_ok(self):
        return all(_guard_ok(self.buf[k], n) for k, n in self.sizes.items())


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("shape", [(1, 1, 3), (8, 8, 3), (16, 16, 3), (33, 17, 3), (40, 200, 3), (9, 23)], ids=str)
def test_coefficients_equal_the_definition(shape):
    """Shapes are (h, w[, 3]): one pixel, less than an MCU, one MCU, edge replication both ways, 13 MCUs = 78 blocks per MCU
    row (more than a wave of lanes), and a grey page with both edges ragged."""
    for quality, page in ((85, synthetic_page(shape[0], shape[1], seed=1, grey=len(shape) == 2)), (100, _noise(shape, 2))):
        wave = Wave([page], quality)
        got = wave.coefficients()
        assert np.array_equal(got, jpeg_ref.coefficients(page, quality)), (shape, quality)
        assert wave.guards_ok()


def _checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    v = ((((yy // 8) + (xx // 8)) & 1) * 255).astype(np.uint8)
    return np.stack([v, v, v], -1)


def _gradient(h, w):
    """A ramp with a faint one-pixel checker on it: a few low frequencies, then nothing until the highest ones."""
    yy, xx = np.mgrid[0:h, 0:w]
    v = 20 + (xx * 200) // max(w - 1, 1) + 12 * ((xx + yy) & 1)
    return np.stack([v, v, v], -1).astype(np.uint8)


def _has_zero_run_of_16(coefs):
    """A non-zero AC coefficient with sixteen or more zeros before it in some block: the coder must emit ZRL."""
    for row in coefs:
        at = np.flatnonzero(row[1:])
        if at.size and np.diff(np.r_[-1, at]).max() > 16:
            return True
    return False


ENTROPY_CASES = {
    "noise_q100": (lambda: _noise((32, 48, 3), 3), 100),        # last coefficient non-zero: no EOB; FF bytes to stuff
    "flat": (lambda: np.full((32, 160, 3), 128, np.uint8), 85),  # 6 bits and less per block: many blocks per word
    "gradient": (lambda: _gradient(64, 96), 85),                 # zero runs of 16 and more: ZRL
    "checker_q100": (lambda: _checkerboard(32, 64), 100),        # DC differences of category 11
    "ten_intervals": (lambda: synthetic_page(160, 48, seed=4), 85),  # 48 wide, 160 high: RSTm wraps
    "grey_noise": (lambda: _noise((24, 40), 5), 100),
}


@pytest.mark.parametrize("name", list(ENTROPY_CASES))
def test_entropy_and_compaction_equal_the_definitions_file(name):
    make, quality = ENTROPY_CASES[name]
    page = make()
    coefs = jpeg_ref.coefficients(page, quality)
    if name == "noise_q100":
        assert (coefs[:, 63] != 0).any()
    if name == "gradient":
        assert _has_zero_run_of_16(coefs)
    if name == "checker_q100":
        assert np.abs(np.diff(coefs[:4, 0].astype(int))).max() >= 1024
    wave = Wave([page], quality)
    wave.set_coefficients(coefs)
    (got,), _ = wave.entropy_and_compact()
    want = jpeg_ref.assemble(coefs, page.shape[0], page.shape[1], page.ndim == 2, quality)
    if name == "noise_q100":
        assert want.count(b"\xff\x00") > 3
    if name == "ten_intervals":
        assert b"\xff\xd7" in want and want.count(b"\xff\xd0") >= 2
    assert got == want
    assert wave.guards_ok()


def test_a_wave_of_five_pages_of_different_sizes():
    pages = [synthetic_page(48, 64, seed=1), _noise((17, 33, 3), 2), synthetic_page(23, 9, seed=3, grey=True), synthetic_page(40, 200, seed=4),
             _noise((1, 1, 3), 5)]
    wave = Wave(pages, 85)
    files, _ = wave.encode()
    for page, data in zip(pages, files):
        assert data == jpeg_ref.encode(page, 85)
        image = Image.open(io.BytesIO(data))
        image.load()
        assert image.size == (page.shape[1], page.shape[0]) and image.mode == ("L" if page.ndim == 2 else "RGB")
    assert wave.guards_ok()


def test_a_page_over_its_capacity_gets_minus_one_and_nothing_else_changes():
    pages = [synthetic_page(48, 64, seed=1), _noise((32, 48, 3), 2), synthetic_page(24, 40, seed=3, grey=True)]
    whole = Wave(pages, 85)
    files, _ = whole.encode()
    assert all(f is not None for f in files)
    caps = [whole.caps[0], 64, whole.caps[2]]
    tight = Wave(pages, 85, capacities=caps)
    got, raw = tight.encode()
    assert got[1] is None and got[0] == files[0] and got[2] == files[2]
    assert (raw[tight.offsets[1] : tight.offsets[2]] == 0xA5).all()  # not a byte of the page that did not fit was written
    assert tight.guards_ok() and whole.guards_ok()
    # a capacity of exactly the file's length fits, one byte less does not
    exact = Wave(pages, 85, capacities=[len(files[0]), len(files[1]) - 1, len(files[2])])
    got, _ = exact.encode()
    assert got[0] == files[0] and got[1] is None and got[2] == files[2] and exact.guards_ok()


@pytest.mark.parametrize("grey", [False, True])
def test_pil_resize_u8_equals_pillows_lanczos(grey):
    from yomitoku_amd.jpeg import resize_pages

    img = _noise((208, 160) if grey else (208, 160, 3), 7)
    other = _noise((100, 77) if grey else (100, 77, 3), 8)  # a second page of another size in the same launch, enlarged
    dev = torch.device("cuda:0")
    outs = resize_pages([torch.from_numpy(img).to(dev), torch.from_numpy(other).to(dev)], [(195, 150), (130, 100)])
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), np.asarray(Image.fromarray(img).resize((150, 195), Image.LANCZOS)))
    assert np.array_equal(outs[1].cpu().numpy(), np.asarray(Image.fromarray(other).resize((100, 130), Image.LANCZOS)))


def test_encode_jpeg_low_shrinks_like_pillow_then_equals_the_definition():
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg, encode_jpeg_pages

    page = synthetic_page(1200, 1600, seed=9)
    got = encode_jpeg(page, "low")
    small = np.asarray(Image.fromarray(page).resize((1500, 1125), Image.LANCZOS))  # per channel: the channel order does not matter
    assert isinstance(got, EncodedJpeg) and (got.width, got.height, got.grey) == (1500, 1125, False) and got.scale == 1500 / 1600
    assert got.data == jpeg_ref.encode(small, 60)
    # "high" leaves the size alone; host arrays, device tensors and a page that is not one, in one call
    dev_page = torch.from_numpy(synthetic_page(40, 56, seed=2)).to("cuda:0")
    grey = synthetic_page(31, 20, seed=3, grey=True)
    out = encode_jpeg_pages([dev_page, np.zeros((4, 4, 2), np.uint8), grey], "high")
    assert isinstance(out[1], ValueError)
    assert out[0].data == jpeg_ref.encode(dev_page.cpu().numpy(), 85) and out[0].scale == 1.0
    assert out[2].data == jpeg_ref.encode(grey, 85) and out[2].grey and (out[2].width, out[2].height) == (20, 31)
