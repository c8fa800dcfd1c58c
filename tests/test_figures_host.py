"""Figure crops, the host side (yomitoku_amd/figures.py, yomitoku_amd/export.py): the rectangle rule against plain slices, the
checked options, the exporters' `figures=` keyword, and the definition of a figure file against the file the exporters write
today.  No device."""
import io
import json
import os

import numpy as np
import pytest

from tests import figures_ref as R
from tests import jpeg_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ------------------------------------------------------------------------------------------------ the rule
def test_the_rect_rule_is_the_exporters_slice_of_the_clamped_box():
    from yomitoku_amd.figures import figure_rects

    rng = np.random.default_rng(11)
    h, w = 37, 53
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    boxes = [[float(v) for v in row] for row in rng.uniform(-8, 62, size=(200, 4))]
    # degenerate and edge-touching ones
    boxes += [[0, 0, w, h], [0, 0, 0, 0], [w, h, w, h], [w - 1, h - 1, w, h], [5, 5, 5, 9], [5, 9, 8, 9], [9, 5, 3, 8], [-0.9, -0.9, 0.9, 0.9],
              [-0.9, -0.9, 1.0, 1.0], [w - 0.5, 0, w + 3, h], [0, h - 0.2, w, h + 1], [3.99, 2.01, 7.99, 6.5], [-5, -5, w + 5, h + 5]]
    got = figure_rects(boxes, h, w)
    assert len(got) == len(boxes)
    live = 0
    for box, r in zip(boxes, got):
        assert r == R.rect(box, h, w)
        x1, y1, x2, y2 = (min(max(int(v), 0), lim) for v, lim in zip(box, (w, h, w, h)))  # the clamped box, int() toward zero
        want = img[y1:y2, x1:x2]
        if r is None:
            assert want.size == 0 and R.crop(img, box) is None
        else:
            live += 1
            assert r == (x1, y1, x2, y2) and np.array_equal(R.crop(img, box), want) and np.array_equal(R.crop_rect(img, r), want)
    assert 20 < live < len(boxes)  # about a quarter of the random boxes have x2 > x1 and y2 > y1: both kinds are there
    # a box inside the page: exactly what _save_figures cuts
    for box in ([3.7, 2.2, 20.9, 30.99], [0, 0, w, h]):
        x1, y1, x2, y2 = map(int, box)
        assert np.array_equal(R.crop(img, box), img[y1:y2, x1:x2, :])
    assert figure_rects([[-0.9, -0.9, 0.9, 0.9]], h, w) == [None]  # toward zero, not floor
    assert figure_rects([], h, w) == []


# ------------------------------------------------------------------------------------------------ the options
def test_check_figures_accepts_and_refuses():
    from yomitoku_amd.figures import FigureOptions, check_figures
    from yomitoku_amd.jpeg import SUBSAMPLINGS

    assert check_figures(None) is None and check_figures(False) is None
    default = check_figures(True)
    assert default == FigureOptions(95, "4:2:0", False, None)
    assert check_figures(1) == FigureOptions(1, "4:2:0", False, None) != default  # True is a bool: the defaults, not quality 1
    assert check_figures(100).quality == 100 and check_figures(np.int64(80)).quality == 80
    assert check_figures({}) == default and check_figures(default) == default
    for sub in SUBSAMPLINGS:
        assert check_figures({"subsampling": sub}).subsampling == sub
    full = check_figures({"quality": 70, "subsampling": "4:4:4", "optimize": True, "max_side": 512})
    assert full == FigureOptions(70, "4:4:4", True, 512)
    assert check_figures({"max_side": None}).max_side is None and check_figures({"max_side": 16}).max_side == 16
    assert check_figures({"max_side": 16383}).max_side == 16383
    with pytest.raises(Exception):
        full.quality = 3  # frozen
    bad = ["x", 0, 101, -1, 95.0, [95], (95,), {"quality": 0}, {"quality": 101}, {"quality": True}, {"quality": "95"}, {"quality": 95.0},
           {"subsampling": "4:1:1"}, {"subsampling": None}, {"subsampling": 0}, {"optimize": 1}, {"optimize": None}, {"max_side": 15},
           {"max_side": 16384}, {"max_side": True}, {"max_side": 64.0}, {"size": 3}, {"quality": 95, "grey": "auto"}, {1: 2}]
    for value in bad:
        with pytest.raises(ValueError):
            check_figures(value)


def test_page_figures_is_a_sized_iterable_of_its_files():
    from yomitoku_amd.figures import PageFigures

    assert len(PageFigures()) == 0 and list(PageFigures()) == []
    made = PageFigures(files=("a", None), rects=((0, 0, 1, 1), None))
    assert len(made) == 2 and list(made) == ["a", None]


def test_crop_figure_files_without_a_crop_needs_no_device():
    from yomitoku_amd.figures import PageFigures, crop_figure_files

    page = np.zeros((20, 30, 3), np.uint8)
    out = crop_figure_files([page, page[:, :, 0], np.zeros((4, 4), np.float32)], [[], [[5, 5, 5, 9], [40, 3, 50, 9]], []])
    assert out[0] == PageFigures((), ()) and out[1] == PageFigures((None, None), (None, None)) and isinstance(out[2], ValueError)
    assert crop_figure_files([], []) == []
    with pytest.raises(ValueError):
        crop_figure_files([page], [[]], figures=0)
    with pytest.raises(ValueError):
        crop_figure_files([page], [[]], figures=None)
    with pytest.raises(ValueError):
        crop_figure_files([page], [])


# ------------------------------------------------------------------------------------------------ the exporters
def _doc():
    from yomitoku_amd.schemas import DocumentAnalyzerSchema

    with open(os.path.join(GOLD, "export.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    return DocumentAnalyzerSchema(**next(c["doc"] for c in cases if c["doc"]["figures"] and c["doc"]["tables"]))


def _figure_files(root):
    found = {}
    for base, _, names in os.walk(root):
        for name in names:
            if "_figure_" in name:
                with open(os.path.join(base, name), "rb") as f:
                    found[os.path.relpath(os.path.join(base, name), root)] = f.read()
    return found


def test_exporters_write_the_given_files_under_todays_names(tmp_path):
    from yomitoku_amd import export as ex
    from yomitoku_amd.figures import PageFigures
    from yomitoku_amd.jpeg import EncodedJpeg

    doc = _doc()
    n = len(doc.figures)
    assert n >= 1
    img = np.random.default_rng(0).integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    payload = [b"\xff\xd8figure-%d\xff\xd9" % i for i in range(n)]
    forms = {"bytes": list(payload),
             "jpegs": tuple(EncodedJpeg(p, 3, 2, False) for p in payload),
             "page": PageFigures(tuple(EncodedJpeg(p, 3, 2, False) for p in payload), tuple((0, 0, 3, 2) for _ in payload))}
    calls = {
        "json": lambda d, root, **kw: ex.export_json(d, os.path.join(root, "page.json"), export_figure=True, **kw),
        "csv": lambda d, root, **kw: ex.export_csv(d, os.path.join(root, "page.csv"), **kw),
        "md": lambda d, root, **kw: ex.export_markdown(d, os.path.join(root, "page.md"), export_figure_letter=True, **kw),
        "html": lambda d, root, **kw: ex.export_html(d, os.path.join(root, "page.html"), **kw),
    }
    for fmt, call in calls.items():
        old_root = str(tmp_path / f"{fmt}_img")
        os.makedirs(old_root)
        old_doc = doc.model_copy(deep=True)
        old = call(old_doc, old_root, img=img)
        names = sorted(_figure_files(old_root))
        assert len(names) == n
        for form, files in forms.items():
            root = str(tmp_path / f"{fmt}_{form}")
            os.makedirs(root)
            new_doc = doc.model_copy(deep=True)
            new = call(new_doc, root, figures=files)  # img=None: neither needed nor looked at
            written = _figure_files(root)
            assert sorted(written) == names and [written[k] for k in names] == payload
            if fmt == "json":
                assert new.model_dump() == old.model_dump() and [f.figure_path for f in new.figures] == [f.figure_path for f in old.figures]
                assert new.figures[0].figure_path == os.path.join("figures", "page_figure_0.png")
            else:
                assert new == old
            main = "page." + fmt
            assert open(os.path.join(root, main), "rb").read() == open(os.path.join(old_root, main), "rb").read()
    # the schema's own methods forward the keyword
    os.makedirs(tmp_path / "m")
    md = doc.model_copy(deep=True).to_markdown(str(tmp_path / "m" / "page.md"), figures=forms["page"])
    assert "figures/page_figure_0.png" in md and _figure_files(str(tmp_path / "m"))[os.path.join("figures", "page_figure_0.png")] == payload[0]
    # the convert_* and figure_to_* layers take it too
    text, _ = ex.convert_markdown(doc.model_copy(deep=True), str(tmp_path / "c" / "page.md"), figures=payload)
    assert text == ex.convert_markdown(doc.model_copy(deep=True), str(tmp_path / "c2" / "page.md"), img=img)[0]
    html, _ = ex.convert_html(doc.model_copy(deep=True), str(tmp_path / "h" / "page.html"), False, True, False, figures=payload)
    assert "page_figure_0.png" in html
    ex.convert_csv(doc.model_copy(deep=True), str(tmp_path / "v" / "page.csv"), False, figures=payload)
    ex.convert_json(doc.model_copy(deep=True), str(tmp_path / "j" / "page.json"), False, None, True, "figures", figures=payload)
    for sub in ("c", "h", "v", "j"):
        written = _figure_files(str(tmp_path / sub))
        assert [written[k] for k in sorted(written)] == payload
    assert ex.figure_to_md(doc.figures, None, str(tmp_path / "f" / "page.md"), files=payload)[0]["md"].startswith('<img src="figures/page_figure_0.png"')
    assert ex.figure_to_html(doc.figures, None, str(tmp_path / "g" / "page.html"), files=payload)[0]["html"].startswith('<img src="figures/page_figure_0.png"')


def test_exporters_refuse_a_wrong_count_and_an_empty_slot(tmp_path):
    from yomitoku_amd import _lib
    from yomitoku_amd import export as ex
    from yomitoku_amd.figures import PageFigures

    doc = _doc()
    n = len(doc.figures)
    good = [b"x"] * n
    for fn, path in ((ex.export_markdown, "page.md"), (ex.export_html, "page.html"), (ex.export_csv, "page.csv")):
        for files in (good + [b"y"], good[:-1], PageFigures((), ())):
            with pytest.raises(ValueError, match="figures"):
                fn(doc.model_copy(deep=True), str(tmp_path / path), figures=files)
        with pytest.raises(ValueError, match="Failed to encode image") as none_slot:
            fn(doc.model_copy(deep=True), str(tmp_path / path), figures=[None] + good[1:])
        assert none_slot.value.__cause__ is None
        cause = _lib.YmkError("figure 0 of page 0: the JPEG file does not fit")
        with pytest.raises(ValueError, match="Failed to encode image") as failed_slot:
            fn(doc.model_copy(deep=True), str(tmp_path / path), figures=PageFigures((cause,) + tuple(good[1:]), (None,) * n))
        assert failed_slot.value.__cause__ is cause
    with pytest.raises(ValueError, match="figures"):
        ex.export_json(doc.model_copy(deep=True), str(tmp_path / "page.json"), export_figure=True, figures=[])
    with pytest.raises(AssertionError):  # without the keyword: what it always was
        ex.export_markdown(doc.model_copy(deep=True), str(tmp_path / "page.md"))


# ------------------------------------------------------------------------------------------------ the definition of a file
@pytest.mark.parametrize("shape", [(32, 48), (16, 16), (33, 50), (1, 1), (7, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_defaults_decode_to_the_pixels_of_todays_file(shape, tmp_path):
    """jpeg_ref.encode(crop, 95) - what the device writes byte for byte (tests/test_figures_gpu.py) - and the file save_image
    writes for the same crop decode, with Pillow, to exactly the same pixels: quality 95, 4:2:0, the same tables and DCT."""
    from PIL import Image

    from yomitoku_amd.export import save_image

    crop = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 256, shape + (3,), dtype=np.uint8)
    path = str(tmp_path / "crop.png")
    save_image(crop, path)
    today = np.asarray(Image.open(path).convert("RGB"))
    ours = np.asarray(Image.open(io.BytesIO(jpeg_ref.encode(crop, 95))).convert("RGB"))
    assert today.shape == ours.shape == shape + (3,)
    assert np.array_equal(today, ours)
