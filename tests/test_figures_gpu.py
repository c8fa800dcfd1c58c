"""Figure crops on the device: ymk_crop_u8 (yomitoku_amd/csrc/ymk_crop.hip) byte for byte against NumPy slices, and
`crop_figure_files` (yomitoku_amd/figures.py) byte for byte against the encoder's definitions (tests/jpeg_ref.py, jpeg_opt_ref.py,
jpeg_modes_ref.py) of the crops of tests/figures_ref.py."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import figures_ref as R
from tests import jpeg_modes_ref, jpeg_opt_ref, jpeg_ref

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _view_at(page, offset, dev):
    """`page` on the device as a view that begins `offset` bytes into its allocation and ends where the allocation ends."""
    whole = torch.empty(offset + page.size, dtype=torch.uint8, device=dev)
    whole[:offset] = 0x5A
    view = whole[offset:].view(page.shape)
    view.copy_(torch.from_numpy(page))
    assert view.data_ptr() == whole.data_ptr() + offset and view.is_contiguous()
    return view


def test_crop_kernel_equals_numpy_slices_and_writes_nothing_else(dev):
    from yomitoku_amd import _lib, imaging
    from yomitoku_amd.devpages import addr_words

    lib = _lib.load()
    words = lib.ymk_crop_u8_record_words()
    assert words == 16
    colour, grey = _noise((53, 70, 3), 1), _noise((40, 37), 2)
    # both pages are views at an odd offset into a larger tensor, and end where it ends: an aligned dword that reaches over
    # either end of a page is outside the allocation's contents
    pages = [(colour, _view_at(colour, 1, dev)), (grey, _view_at(grey, 3, dev))]
    assert pages[0][1].data_ptr() % 4 == 1 and pages[1][1].data_ptr() % 4 == 3

    rects = []  # (page, x0, y0, cw, ch)
    rects += [(0, 0, 0, 70, 53), (1, 0, 0, 37, 40)]  # the whole page
    rects += [(0, 69, 52, 1, 1), (1, 36, 39, 1, 1)]  # 1 x 1 at the last pixel
    rects += [(0, x0, 3 + x0, 17, 6) for x0 in range(16)]  # every x0 % 16 for a 17-pixel-wide crop
    rects += [(1, x0, 2 + x0, 17, 5) for x0 in range(16)]
    rects += [(p, 7, 11, cw, 9) for p in (0, 1) for cw in (1, 2, 5)]  # cw * C < 16: a chunk straddles several rows
    rects += [(0, 41, 20, 29, 33), (1, 20, 31, 17, 9), (0, 0, 45, 70, 8), (1, 30, 0, 7, 40)]  # touching the right and bottom edges
    rects += [(0, 10, 10, 30, 20), (0, 25, 18, 30, 20)]  # two that overlap
    rects += [(0, 0, 0, 1, 1), (0, 1, 0, 5, 1), (0, 0, 0, 6, 1)]  # at the page's first bytes: the covering dwords start before it
    rects += [(0, 64, 52, 6, 1), (1, 20, 39, 17, 1)]  # ... and at its last bytes: they end behind it
    # four records that do not fit: an origin beyond the page, x0 + cw > W, C = 2, a misaligned destination
    bad = {3: ("origin", (0, 72, 5, 4, 4)), 9: ("wide", (0, 60, 5, 11, 4)), 20: ("channels", (0, 0, 0, 8, 8)), 41: ("misaligned", (1, 2, 2, 8, 8))}

    recs, want_parts, at, chunk = [], [], 32, 0  # 32 untouched bytes in front of the first crop
    order = list(rects)
    for pos in sorted(bad):
        order.insert(pos, bad[pos])
    for k, item in enumerate(order):
        kind, (p, x0, y0, cw, ch) = item if isinstance(item[0], str) else (None, item)
        host, page = pages[p]
        c = 1 if host.ndim == 2 else 3
        rec = np.zeros(words, np.int32)
        rec[0:2] = addr_words(page.data_ptr())
        rec[2:9] = (host.shape[0], host.shape[1], 2 if kind == "channels" else c, x0, y0, cw, ch)
        nbytes = ch * cw * (2 if kind == "channels" else c)
        chunks = -(-nbytes // 16)
        rec[11] = chunk
        recs.append((rec, at + (4 if kind == "misaligned" else 0)))
        if kind is None:
            want_parts.append((at, host[y0 : y0 + ch, x0 : x0 + cw].reshape(-1)))
        at += 16 * chunks + (16 * (k % 3))  # padding between the crops: none, one chunk, two
        chunk += chunks
    total = at + 48  # and untouched bytes behind the last crop
    out = torch.full((total,), FILL, dtype=torch.uint8, device=dev)
    assert out.data_ptr() % 16 == 0
    for rec, off in recs:
        rec[9:11] = addr_words(out.data_ptr() + off)
    blob = np.concatenate([rec for rec, _ in recs])
    blob_dev = imaging._stage_blob(blob, dev)
    _lib.check(lib.ymk_crop_u8(blob_dev.data_ptr(), blob.size, len(recs), chunk, _lib.current_stream_ptr()), "ymk_crop_u8")
    torch.cuda.synchronize()
    want = np.full(total, FILL, np.uint8)
    for off, data in want_parts:
        want[off : off + data.size] = data
    got = out.cpu().numpy()
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, f"{wrong.size} bytes differ, the first at {wrong[:8]}"
    assert len(want_parts) == len(rects) and int((want != FILL).sum()) > 0

    # n == 0 queues nothing and looks at nothing
    _lib.check(lib.ymk_crop_u8(None, 0, 0, 0, _lib.current_stream_ptr()), "ymk_crop_u8")


PAGE = None


def _page():
    global PAGE
    if PAGE is None:
        from tests.test_jpeg_host import synthetic_page

        PAGE = np.array(synthetic_page(160, 200, seed=5))  # 160 x 200 x 3
        PAGE[40:80, 100:160] = _noise((40, 60, 3), 7)  # a "photograph"
    return PAGE


BOXES = [[10.7, 20.2, 58.9, 52.99], [100, 40, 160, 80], [150.5, 100.5, 250.0, 170.0], [30, 30, 30, 60], [199, 159, 200, 160], [0, 0, 33, 50]]


def test_default_files_equal_the_definition_of_the_crops(dev):
    from yomitoku_amd.figures import PageFigures, crop_figure_files
    from yomitoku_amd.jpeg import EncodedJpeg

    page = _page()
    grey = np.ascontiguousarray(page[:, :, 1])
    scratch = {}
    made = crop_figure_files([page, np.zeros((16, 16, 3), np.uint8), grey, np.zeros((4, 4), np.float32)], [BOXES, [], BOXES[:3], BOXES[:1]], scratch=scratch)
    assert isinstance(made[0], PageFigures) and len(made[0]) == len(BOXES) and len(made[1]) == 0 and made[1].rects == ()
    assert isinstance(made[3], ValueError)  # a page that is no page
    assert made[0].rects == tuple(R.rect(b, 160, 200) for b in BOXES) and made[0].rects[3] is None and made[0].files[3] is None
    assert made[0].rects[2] == (150, 100, 200, 160) and made[0].rects[4] == (199, 159, 200, 160)  # clamped; 1 x 1: the capacity rule
    for box, file in zip(BOXES, made[0]):
        crop = R.crop(page, box)
        if crop is None:
            continue
        assert isinstance(file, EncodedJpeg) and (file.height, file.width) == crop.shape[:2]
        assert (file.grey, file.scale, file.optimized, file.subsampling) == (False, 1.0, False, "4:2:0")
        assert file.data == jpeg_ref.encode(crop, 95)
    for box, file in zip(BOXES[:3], made[2]):  # a one-channel page gives grey files
        crop = R.crop(grey, box)
        assert (file.grey, file.subsampling, file.height, file.width) == (True, None) + crop.shape and file.data == jpeg_ref.encode(crop, 95)
        assert Image.open(io.BytesIO(file.data)).mode == "L"
    # device pages give what host pages give, with the scratch of the first call
    again = crop_figure_files([torch.from_numpy(page).to(dev), torch.from_numpy(grey).to(dev)], [BOXES, BOXES[:3]], scratch=scratch)
    assert again[0] == made[0] and again[1] == made[2]
    # an int is the quality
    q60 = crop_figure_files([page], [BOXES[:1]], figures=60)[0]
    assert q60.files[0].data == jpeg_ref.encode(R.crop(page, BOXES[0]), 60)


def test_optimize_subsampling_and_max_side_equal_their_definitions(dev):
    from yomitoku_amd.figures import crop_figure_files

    page = _page()
    boxes = [BOXES[1], BOXES[5]]
    opt = crop_figure_files([page], [boxes], figures={"optimize": True})[0]
    full = crop_figure_files([page], [boxes], figures={"subsampling": "4:4:4", "quality": 100})[0]
    for box, a, b in zip(boxes, opt, full):
        crop = R.crop(page, box)
        assert a.optimized and a.data == jpeg_opt_ref.encode(crop, 95)
        assert b.subsampling == "4:4:4" and b.data == jpeg_modes_ref.encode(crop, 100, "4:4:4")  # noise at 100 / 4:4:4 fits its capacity
    # max_side: a 100 x 60 crop is shrunk with Pillow's Lanczos resample to 32 x 19, a 30 x 20 one is left alone
    small = crop_figure_files([page], [[[20, 30, 80, 130], [5, 5, 35, 25]]], figures={"max_side": 32})[0]
    crop = R.crop(page, [20, 30, 80, 130])
    assert crop.shape == (100, 60, 3)
    scale = 32 / 100
    oh, ow = max(int(100 * scale), 1), max(int(60 * scale), 1)
    shrunk = np.asarray(Image.fromarray(crop).resize((ow, oh), Image.LANCZOS))  # per channel: the channel order does not matter
    assert (small.files[0].height, small.files[0].width, small.files[0].scale) == (oh, ow, scale)
    assert small.files[0].data == jpeg_ref.encode(shrunk, 95)
    assert small.files[1].scale == 1.0 and small.files[1].data == jpeg_ref.encode(R.crop(page, [5, 5, 35, 25]), 95)
    assert small.rects == ((20, 30, 80, 130), (5, 5, 35, 25))  # the rectangles stay those of the page
