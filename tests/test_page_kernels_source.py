"""Host check over the kernel sources: what the page-file kernels share has ONE definition, in ymk_pages.h, and the guard of the
extern "C" entries one, in ymk_common.h.  The JPEG encoder's optimised tables and the Deflate coder's equal their references byte
for byte only while both run the same merge (libjpeg's tie rule) and the same limiter (Figure K.3); a private copy in either file
would let the two drift apart without any diagnostic."""
import glob
import os

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yomitoku_amd", "csrc")
PAGES_H = "ymk_pages.h"
COMMON_H = "ymk_common.h"


def _sources(*patterns):
    paths = sorted(p for pat in patterns for p in glob.glob(os.path.join(CSRC, pat)))
    assert paths
    return {os.path.basename(p): open(p).read() for p in paths}


def _files_with(every, text):
    return [n for n, s in every.items() if text in s]


def test_huffman_construction_is_defined_once():
    every = _sources("*.h", "*.hip", "*.cpp")
    # the merge's tie key: among equal frequencies the largest symbol
    assert _files_with(every, "0xffff - (k * 64 + lane)") == [PAGES_H], "the pattern is found where it is known to be, and only there"
    # the update of Figure K.3
    assert _files_with(every, "bits[i] -= 2") == [PAGES_H]
    # both coders call it
    for name in ("ymk_jpeg.hip", "ymk_flate.hip"):
        for call in ("huff_merge_lengths(", "huff_limit_counts("):
            assert call in every[name], f"{name}: no call of {call[:-1]}"


def test_page_record_reader_is_defined_once():
    every = _sources("*.h", "*.hip", "*.cpp")
    assert _files_with(every, "<< 32) | (unsigned long long)(unsigned)r[k]") == [PAGES_H]
    users = _files_with(every, "page_word64(r, ")
    assert {"ymk_jpeg.hip", "ymk_flate.hip", "ymk_ccitt.hip", "ymk_binarize.hip", "ymk_cc.hip", "ymk_mrc.hip", "ymk_deskew.hip"} <= set(users)


def test_entry_guard_is_defined_once():
    every = _sources("*.h", "*.hip", "*.cpp")
    assert _files_with(every, "catch (const std::exception") == [COMMON_H]
    assert "catch (...)" in every[COMMON_H]
    assert _files_with(every, "catch (...)") == [COMMON_H]
    # no private guard macro beside the shared one
    assert _files_with(every, "#define YMK_API_BEGIN") == [COMMON_H]
    assert [n for n, s in every.items() if n != COMMON_H and " try {" in s] == []
