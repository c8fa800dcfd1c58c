"""CPU checks of the page-skew definition (tests/deskew_ref.py) against independent restatements - a literal per-pixel loop,
exact rational interpolation -, of the estimator on the golden page turned by Pillow, and of the host side of the switch
(yomitoku_amd/deskew.py: check_deskew, PageSkew; serve(deskew=...) on the stub pipeline).  The device is held to the definition
in tests/test_deskew_gpu.py."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import deskew_ref as R
from yomitoku_amd import deskew as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_page.jpg")
STEP = D.DEFAULTS["step"]


def _golden(quarter=False):
    from PIL import Image

    img = Image.open(GOLDEN).convert("L")
    return img.rotate(90, expand=True) if quarter else img


def _turned(img, a):
    from PIL import Image

    return np.asarray(img.rotate(a, Image.BICUBIC, fillcolor=255))


_CACHE = {}


def _estimate(quarter, a):
    """(k, angle, S, S_0, the turned page) of the golden page turned by a degrees - the estimate itself, min_angle 0 -,
    computed once per session."""
    key = (quarter, a)
    if key not in _CACHE:
        page = _turned(_golden(quarter), a)
        _CACHE[key] = R.estimate(page, min_angle=0.0) + (page,)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------- the table
def test_angle_table_is_symmetric_integer_and_the_library_accepts_it():
    table = D.angle_table()
    assert table.shape == (101, 2) and table.dtype == np.int32
    assert table[50].tolist() == [0, 1 << 14]
    assert (table[::-1, 0] == -table[:, 0]).all() and (table[::-1, 1] == table[:, 1]).all()
    assert table[60].tolist() == [286, 16382] and table[100].tolist() == [1428, 16322]  # round(2^14 sin / cos) of 1 and 5 degrees
    got, s_max, dead = D._checked_table(dict(D.DEFAULTS))
    assert (got == table).all() and s_max == 1428 and dead == 3
    assert D.angle_table(0.25, 2.0).shape == (17, 2)
    assert D.dead_band(0.1, 0.3) == 3 and D.dead_band(0.25, 0.3) == 2 and D.dead_band(0.1, 0.0) == 0


def test_the_library_refuses_a_table_that_is_none():
    import ctypes

    from yomitoku_amd import _lib

    lib = _lib.load()

    def check(table):
        arr = np.ascontiguousarray(table, np.int32)
        s_max = ctypes.c_int()
        return lib.ymk_dsk_check_angles(arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(arr), ctypes.byref(s_max))

    good = D.angle_table()
    assert check(good) == 0
    assert check(good[:100]) != 0  # even
    bad = good.copy()
    bad[3, 0] += 40  # not symmetric, not on the circle
    assert check(bad) != 0
    bad = good.copy()
    bad[50] = (1, 1 << 14)  # the middle is not 0
    assert check(bad) != 0 and lib.ymk_last_error()
    sizes, fits = D.scratch_sizes([(8192, 8192, 3), (16383, 16383), (40, 100, 3)], 101, 1428)
    assert fits == [True, False, True]  # the stated limit: 8192 a side is estimated, the largest page is not
    assert sizes[0] == 8192 * 8192 + 4000 and sizes[3] == 3 * 101 * 8 and sizes[4] == 3 * 8 * 4


# ---------------------------------------------------------------------------------------------------------------- scores
def test_scores_equal_a_literal_per_pixel_loop():
    rng = np.random.default_rng(7)
    mask = rng.random((24, 40)) < 0.2
    mask[5, :] = True  # a ruling
    table = D.angle_table()
    h, w = mask.shape
    want = []
    for s, c in table.tolist():
        rows, cols = {}, {}
        for y in range(h):
            for x in range(w):
                if mask[y, x]:
                    r = (y * c + x * s + (w << 14)) >> 14
                    q = (x * c - y * s + (h << 14)) >> 14
                    rows[r] = rows.get(r, 0) + 1
                    cols[q] = cols.get(q, 0) + 1
        total = 0
        for prof in (rows, cols):
            for b in range(min(prof) - 1, max(prof) + 1):
                total += (prof.get(b + 1, 0) - prof.get(b, 0)) ** 2
        want.append(total)
    assert R.scores(mask, table) == want
    assert R.scores(np.zeros((24, 40), bool), table) == [0] * 101


def test_luminance_is_the_stated_integer_form():
    rng = np.random.default_rng(3)
    page = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    want = [[(29 * int(b) + 150 * int(g) + 77 * int(r) + 128) >> 8 for b, g, r in row] for row in page]
    assert R.luminance(page).tolist() == want
    assert R.luminance(page[..., 0]) is not None and (R.luminance(page[..., 0]) == page[..., 0]).all()
    assert R.luminance(np.full((2, 2, 3), 255, np.uint8)).tolist() == [[255, 255], [255, 255]]


# ---------------------------------------------------------------------------------------------------------------- rotation
@pytest.mark.parametrize("shape,k", [((13, 17), 30), ((13, 17), -46), ((11, 8, 3), 50), ((5, 1), -7)])
def test_rotation_equals_exact_bilinear_interpolation_at_the_truncated_fractions(shape, k):
    rng = np.random.default_rng(11)
    page = rng.integers(0, 256, shape, dtype=np.uint8)
    s, c = D.angle_table()[k + 50].tolist()
    h, w = shape[:2]
    src = page.reshape(h, w, -1)

    def tap(yy, xx, ch):
        return int(src[yy, xx, ch]) if 0 <= yy < h and 0 <= xx < w else 255

    want = np.zeros_like(src)
    for Y in range(h):
        for X in range(w):
            u, v = 2 * X - (w - 1), 2 * Y - (h - 1)
            sx, sy = c * u + s * v + ((w - 1) << 14), -s * u + c * v + ((h - 1) << 14)
            x0, y0 = sx >> 15, sy >> 15
            fx, fy = Fraction((sx >> 7) & 255, 256), Fraction((sy >> 7) & 255, 256)
            for ch in range(src.shape[2]):
                exact = ((1 - fx) * (1 - fy) * tap(y0, x0, ch) + fx * (1 - fy) * tap(y0, x0 + 1, ch) + (1 - fx) * fy * tap(y0 + 1, x0, ch)
                         + fx * fy * tap(y0 + 1, x0 + 1, ch))
                want[Y, X, ch] = int((exact + Fraction(1, 2)).__floor__())
    assert (R.rotate(page, s, c) == want.reshape(shape)).all()


def test_rotation_by_index_zero_leaves_the_bytes():
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    s, c = D.angle_table()[50].tolist()
    assert R.rotate(page, s, c).tobytes() == page.tobytes()
    fixed, k, _, _ = R.deskew(np.full((20, 30), 255, np.uint8))
    assert k == 0 and fixed.tobytes() == bytes([255]) * 600


# ---------------------------------------------------------------------------------------------------------------- choice
def test_the_tie_rule_and_the_margin():
    assert R.choose([0] * 101, 3) == (0, 0, 0)  # a blank page ties everywhere
    assert R.estimate(np.full((50, 70), 255, np.uint8))[:2] == (0, 0.0)
    S = [10] * 7
    S[1] = S[5] = 40  # k = -2 and k = 2: the negative one
    assert R.choose(S, 0) == (-2, 40, 10)
    S[2] = 40  # k = -1: the smaller |k|
    assert R.choose(S, 0) == (-1, 40, 10)
    assert R.choose(S, 2) == (0, 40, 10)  # inside the dead band
    assert R.choose([8, 8, 8, 8, 8, 8, 8], 0) == (0, 8, 8)
    assert R.choose([8, 8, 8, 80, 8, 8, 89], 0) == (0, 89, 80)  # 8 * 89 < 9 * 80: not 12.5 % above upright
    assert R.choose([8, 8, 8, 80, 8, 8, 90], 0) == (3, 90, 80)


def _bars(h=64, w=96):
    page = np.full((h, w), 255, np.uint8)
    for y0 in range(8, h - 8, 12):
        page[y0 : y0 + 4, 10 : w - 10] = 0
    return page


def test_horizontal_bars_on_a_narrow_page_are_upright():
    """96 pixels wide: the row profile does not change over a plateau of angles around 0, and the tie rule takes its middle"""
    k, angle, s_best, s_zero = R.estimate(_bars())
    assert (k, angle) == (0, 0.0) and s_best == s_zero > 0


# ---------------------------------------------------------------------------------------------------------------- the estimator
@pytest.mark.parametrize("quarter,a", [(False, 0.3), (False, 1.0), (False, 3.0), (False, -4.6), (True, 1.5), (True, -3.2)])
def test_the_golden_page_turned_by_pillow_estimates_its_angle(quarter, a):
    """The estimate - the angle of the largest score with the 9 / 8 margin, before the dead band - is within one step of the
    turn.  The page turned by 0.3 estimates 0.2 (one step off, as the feasibility check of the feature measured), which the
    default dead band of 0.3 then leaves alone: that case is why the estimate is taken with min_angle 0 here, and the dead
    band has its own test below."""
    k, angle, s_best, s_zero, _ = _estimate(quarter, a)
    print(f"turned {a}: k {k} angle {angle:.2f} S {s_best} S_0 {s_zero} ratio {s_best / max(s_zero, 1):.2f}")
    assert abs(angle - a) <= STEP + 1e-9


@pytest.mark.parametrize("quarter,a", [(False, 0.3), (False, 1.0), (False, 3.0), (False, -4.6), (True, 1.5), (True, -3.2)])
def test_the_default_dead_band_on_the_golden_page(quarter, a):
    """min_angle 0.3: an estimate of 0.2 is left alone, every estimate from 0.3 on is kept as it is"""
    k, _, s_best, s_zero, page = _estimate(quarter, a)
    assert R.estimate(page) == ((0 if abs(k) < 3 else k), (0 if abs(k) < 3 else k) * STEP, s_best, s_zero)


def test_the_upright_golden_page_estimates_zero():
    for quarter in (False, True):
        assert R.estimate(np.asarray(_golden(quarter)))[:2] == (0, 0.0)


@pytest.mark.parametrize("a", [1.0, 3.0, -4.6])
def test_the_corrected_golden_page_estimates_zero(a):
    k, _, _, _, page = _estimate(False, a)
    s, c = D.angle_table()[k + 50].tolist()
    again = R.estimate(R.rotate(page, s, c))
    print(f"turned {a}, corrected by k {k}: re-estimate {again[1]:.2f}")
    assert abs(again[1]) <= STEP + 1e-9


def test_uniform_noise_estimates_zero():
    page = np.random.default_rng(1).integers(0, 256, (300, 260), dtype=np.uint8)
    k, angle, s_best, s_zero = R.estimate(page)
    print(f"noise: S {s_best} S_0 {s_zero}")
    assert (k, angle) == (0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_check_deskew_accepts_and_refuses():
    assert D.check_deskew(False) is None
    assert D.check_deskew(True) == {"max_angle": 5.0, "step": 0.1, "min_angle": 0.3}
    assert D.check_deskew({"step": 0.25, "max_angle": 2}) == {"max_angle": 2.0, "step": 0.25, "min_angle": 0.3}
    assert D.check_deskew({}) == D.DEFAULTS
    assert D.check_deskew({"max_angle": 20.0}) is not None  # 401 angles
    for bad in ("yes", None, 1, 0, 1.0, ["step"], {"steps": 0.1}, {"step": 0}, {"step": -0.1}, {"step": "0.1"}, {"step": True},
                {"max_angle": 20.1}, {"max_angle": 50, "step": 1.0}, {"max_angle": -1}, {"min_angle": -0.1}, {"step": float("nan")}):
        with pytest.raises(ValueError):
            D.check_deskew(bad)


def test_serve_refuses_a_bad_deskew_before_a_source_is_pulled():
    from tests.test_serving import StubAnalyzer, page
    from yomitoku_amd.serving import PagePipeline

    pulled = []

    def feed():
        for i in range(3):
            pulled.append(i)
            yield page(i)

    pipe = PagePipeline(StubAnalyzer(), wave=2, in_flight=2)
    try:
        for bad in ("yes", {"angle": 1}, {"step": 0}):
            with pytest.raises(ValueError):
                pipe.serve(feed(), deskew=bad)
        with pytest.raises(ValueError, match="HIP device"):  # a pipeline without a device refuses the switch
            pipe.serve(feed(), deskew=True)
        assert pulled == []
        out = pipe.serve(feed(), deskew=False)  # and the entries of a job without it are today's
        assert [o[0] for o in out] == [0, 1, 2] and pulled == [0, 1, 2]
    finally:
        pipe.close()


def test_the_public_serves_take_the_switch():
    import inspect

    from yomitoku_amd.document_analyzer import OCR, DocumentAnalyzer
    from yomitoku_amd.table_semantic_parser import TableSemanticParser

    for cls in (OCR, DocumentAnalyzer, TableSemanticParser, __import__("yomitoku_amd.serving", fromlist=["PagePipeline"]).PagePipeline):
        assert inspect.signature(cls.serve).parameters["deskew"].default is False, cls


# ---------------------------------------------------------------------------------------------------------------- PageSkew
@pytest.mark.parametrize("h,w,k", [(842, 596, 30), (37, 33, -46), (100, 40, 1)])
def test_the_matrix_is_the_rotations_own_source_coordinates(h, w, k):
    s, c = D.angle_table()[k + 50].tolist()
    skew = D.PageSkew(k * STEP, k, 2, 1, True, D.rotation_matrix(h, w, s, c))
    centre = np.array([(w - 1) / 2, (h - 1) / 2])
    assert np.allclose(skew.to_original(centre), centre, atol=1e-9)
    sx, sy = R.source_coordinates(h, w, s, c)
    corners = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    got = skew.to_original(np.array(corners, np.float64))
    want = np.array([(sx[y, x] / 32768.0, sy[y, x] / 32768.0) for x, y in corners])
    assert np.allclose(got, want, atol=1e-9)
    flat = D.PageSkew()
    assert flat.angle == 0.0 and flat.index == 0 and flat.estimated and np.array_equal(flat.to_original([[3, 4]]), [[3.0, 4.0]])
