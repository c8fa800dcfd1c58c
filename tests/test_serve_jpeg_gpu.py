"""DocumentAnalyzer.serve(jpeg=...): the page's JPEG file next to its schema, made in the render stage.  The analyzer and its
seeded weights are those of tests/test_serving_gpu.py."""
import io
import re
import threading

import numpy as np
import pytest
from PIL import Image

from tests.test_serving_gpu import _analyzer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def analyzer(dev):
    an = _analyzer()
    yield an
    an.close()


@pytest.fixture(scope="module")
def pages():
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    return [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate([(640, 600), (600, 640), (640, 600), (500, 700), (640, 600)])]


def test_serve_jpeg_gives_schema_and_file_and_isolates_failures(analyzer, pages, tmp_path):
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg

    plain = analyzer.serve(pages, wave=2)
    assert not [t for t in threading.enumerate() if t.name == "ymk-render"]
    # a page the detector cannot take (a 2-D array) and a file that does not exist, as in tests/test_serving_gpu.py
    sources = [pages[0], pages[1], np.zeros((50, 60), dtype=np.uint8), pages[2], str(tmp_path / "nope.png"), pages[3], pages[4]]
    keep = [0, 1, 3, 5, 6]
    before = [p.copy() for p in pages]
    got = analyzer.serve(sources, wave=2, jpeg="high")
    assert len(got) == len(sources) and isinstance(got[2], Exception) and isinstance(got[4], Exception)
    for k, page, want in zip(keep, pages, plain):
        entry = got[k]
        assert isinstance(entry, tuple) and len(entry) == 2 and isinstance(entry[1], EncodedJpeg)
        assert entry[0].model_dump() == want.model_dump()
        assert entry[1] == encode_jpeg(page, "high")
        assert (entry[1].width, entry[1].height, entry[1].grey, entry[1].scale) == (page.shape[1], page.shape[0], False, 1.0)
        image = Image.open(io.BytesIO(entry[1].data))
        image.load()
        assert image.size == (page.shape[1], page.shape[0]) and image.mode == "RGB"
    assert all(np.array_equal(a, b) for a, b in zip(pages, before))
    # the next job on the same analyzer, without jpeg: plain schemas, no render visit
    analyzer._pipeline.trace = []
    after = analyzer.serve(pages, wave=2)
    assert all(not isinstance(e, tuple) for e in after) and [e.model_dump() for e in after] == [e.model_dump() for e in plain]
    assert "render" not in {t[0] for t in analyzer._pipeline.trace}
    analyzer._pipeline.trace = None
    # a preset that shrinks: the file is that of the shrunk page and says by how much
    low = analyzer.serve(pages[:1], wave=2, jpeg="low", with_source=True)
    assert low[0][:2] == (0, 0) and low[0][2][1] == encode_jpeg(pages[0], "low") and low[0][2][1].scale == 1.0  # 640 x 600: below 1500
    with pytest.raises(ValueError, match="nope"):
        analyzer.serve(pages[:1], jpeg="nope")


def test_serve_jpeg_with_overlays_has_four_members(analyzer, pages):
    from yomitoku_amd.jpeg import encode_jpeg

    three = analyzer.serve(pages[:3], wave=2, overlays=True)
    four = analyzer.serve(pages[:3], wave=2, overlays=True, jpeg="middle")
    assert all(isinstance(e, tuple) and len(e) == 4 for e in four)
    for page, (schema, ocr, lay), entry in zip(pages, three, four):
        assert entry[0].model_dump() == schema.model_dump()
        assert np.array_equal(entry[1], ocr) and np.array_equal(entry[2], lay) and not np.array_equal(ocr, page)
        assert entry[3] == encode_jpeg(page, "middle")  # from the clean page, not from a canvas


def test_searchable_pdf_from_the_jobs_output(analyzer, pages):
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    out = analyzer.serve(pages[:3], wave=2, jpeg="high")
    pdf = searchable_pdf_bytes([e[1] for e in out], [e[0] for e in out])
    sizes = []
    for m in re.finditer(rb"/Subtype /Image /Width (\d+) /Height (\d+) /ColorSpace /DeviceRGB .*? /Length (\d+) >>\nstream\n", pdf, re.S):
        data = pdf[m.end() : m.end() + int(m.group(3))]
        image = Image.open(io.BytesIO(data))
        image.load()
        assert image.size == (int(m.group(1)), int(m.group(2)))
        sizes.append(image.size)
    assert sizes == [(p.shape[1], p.shape[0]) for p in pages[:3]]
    assert [e[1].data in pdf for e in out] == [True] * 3


def test_serve_sharded_refuses_jpeg(pages):
    from yomitoku_amd.distributed import ShardedServer

    server = ShardedServer.__new__(ShardedServer)  # no process group: the refusal comes before anything is served
    with pytest.raises(NotImplementedError, match="jpeg"):
        server.serve_local(pages[:1], jpeg="high")
