"""The host parts of the text-only job (OCR.serve): the render stage draws as many pictures per page as the analyzer records
(StageAnalyzer._stage_render, with the wave renderer replaced by a recorder), and the searchable PDF takes a document that is
words alone (an OCRSchema) as one container - the page."""
import re
from types import SimpleNamespace

import numpy as np
import pytest

from yomitoku_amd.schemas import DocumentAnalyzerSchema, OCRSchema
from yomitoku_amd.serving import StageAnalyzer
from yomitoku_amd.utils import searchable_pdf as sp
from yomitoku_amd.utils import visualizer


class Draws(StageAnalyzer):
    def __init__(self, per_page):
        self.per_page = per_page
        self._render_pinned = {}

    def _page_drawings(self, wave, k, results):
        if results == "cannot":
            raise ValueError("cannot draw this page")
        return tuple(f"drawing {wave.ids[k]}.{j}" for j in range(self.per_page[k]))


class _Wave(SimpleNamespace):
    def __len__(self):
        return len(self.ids)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_the_render_stage_draws_what_the_analyzer_records(monkeypatch, n):
    calls = []

    def render_wave(pages, drawings, pinned=None, store=None):
        calls.append((list(pages), list(drawings), pinned))
        return [f"{d} on {p}" for p, d in zip(pages, drawings)]

    monkeypatch.setattr(visualizer, "render_wave", render_wave)
    wave = _Wave(ids=[10, 11, 12, 13], pages=["page 10", "page 11", "page 12", "page 13"], ring=1, dags="kept")
    an = Draws([n] * 4)
    out = an._stage_render(wave, ["schema", RuntimeError("failed before"), "cannot", "schema"])
    assert out[1] is None and isinstance(out[2], ValueError) and wave.dags is None
    assert out[0] == tuple(f"drawing 10.{j} on page 10" for j in range(n)) and out[3] == tuple(f"drawing 13.{j} on page 13" for j in range(n))
    (pages, drawings, pinned), = calls  # one call for the wave: every live page n times, its drawings next to it
    assert pages == ["page 10"] * n + ["page 13"] * n and len(drawings) == 2 * n
    assert pinned is an._render_pinned[1]


def test_pages_with_differing_picture_counts_are_a_bug(monkeypatch):
    monkeypatch.setattr(visualizer, "render_wave", lambda *a, **k: pytest.fail("nothing may be drawn"))
    wave = _Wave(ids=[0, 1], pages=["a", "b"], ring=0, dags=None)
    with pytest.raises(AssertionError, match="same number of pictures"):
        Draws([1, 2])._stage_render(wave, ["schema", "schema"])


def _word(x, y, w, h, text, direction="horizontal"):
    return {"points": [[x, y], [x + w, y], [x + w, y + h], [x, y + h]], "content": text, "direction": direction, "rec_score": 0.9, "det_score": 0.9}


def test_a_document_of_words_alone_is_one_container():
    words = [_word(300, 200, 120, 30, "third"), _word(40, 40, 200, 30, "first"), _word(40, 200, 120, 30, "second")]
    doc = OCRSchema(words=words)
    assert [w.content for w in sp.words_in_reading_order(doc)] == ["first", "second", "third"]
    vertical = OCRSchema(words=[_word(40, 40, 30, 200, "left", "vertical"), _word(300, 40, 30, 200, "right", "vertical"), _word(100, 400, 90, 30, "foot")])
    assert [w.content for w in sp.words_in_reading_order(vertical)] == ["right", "foot", "left"]  # right to left, as in a vertical container
    # a DocumentAnalyzerSchema keeps the rule it had: words outside every container are not written
    full = DocumentAnalyzerSchema(paragraphs=[], tables=[], figures=[], words=words)
    assert sp.words_in_reading_order(full) == []
    ops = sp.text_layer(doc, 400)
    assert [op[-1] for op in ops if op[0] == "text"] == ["first", "second", "third"]
    # a scaled page (a preset that shrinks): the view carries the words alone
    assert [w.content for w in sp.words_in_reading_order(sp._scaled_document(doc, 0.5))] == ["first", "second", "third"]
    assert sp._scaled_document(doc, 0.5).words[1].points[2] == [120.0, 35.0]


def test_searchable_pdf_of_ocr_schemas():
    page = np.full((400, 500, 3), 255, dtype=np.uint8)
    docs = [OCRSchema(words=[_word(40, 40, 200, 30, "first")]), OCRSchema(words=[])]
    pdf = sp.searchable_pdf_bytes([page, page], docs)
    assert pdf.startswith(b"%PDF") and len(re.findall(rb"/Type /Page\b", pdf)) == 2
