"""CPU checks of the C-ABI boundary: the library loads without a GPU and exports every symbol
include/ymk.h declares; the ctypes table in yomitoku_amd/_lib.py covers the same set."""
import os
import re

from yomitoku_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "ymk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ymk_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    syms = _header_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in ymk.h but not exported"


def test_ctypes_table_matches_header():
    assert sorted(_lib.SIGNATURES) == _header_symbols()


def test_view_entries_of_the_sequence_kernels_have_as_many_ctypes_arguments_as_the_header():
    """ymk_op_attention_view / ymk_op_layernorm_view: one ctypes argument per declared parameter, the batch strides as int64;
    the same for the glue kernels' entries (the pooling / resize views, the layout change, the broadcast add, the max|x| passes)"""
    import ctypes

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ymk.h")).read(), flags=re.S)
    for name, count in (("ymk_op_attention_view", 31), ("ymk_op_layernorm_view", 11), ("ymk_op_maxpool3x3s2_view", 9),
                        ("ymk_op_avgpool2x2_ceil_view", 9), ("ymk_op_upsample_nearest2x_view", 9),
                        ("ymk_op_upsample_bilinear_view", 13), ("ymk_op_nchw3_to_nhwc4", 6), ("ymk_op_add_bcast", 7),
                        ("ymk_op_absmax", 7), ("ymk_op_amax_merge", 3)):
        params = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)", src, flags=re.S).group(1).split(",")
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params) == count, name
        for p, a in zip(params, args):
            assert ("int64_t" in p) == (a is ctypes.c_int64), (name, p)
            assert ("*" in p) == (a is ctypes.c_void_p), (name, p)
            assert ("float " in p and "*" not in p) == (a is ctypes.c_float), (name, p)


def test_version_and_error_slot():
    lib = _lib.load()
    assert lib.ymk_version() >= 100
    # an unknown model kind fails cleanly (no GPU needed: hipSetDevice fails first or kind check)
    h = lib.ymk_model_create(b"no-such-model", 0)
    assert not h
    assert lib.ymk_last_error()


def test_debug_options_exist_and_their_documented_defaults_agree():
    """ymk_debug_option keys the tools and tests use are known to the library (no GPU needed: they only set process-wide
    switches), an unknown key is refused, and the default of "conv_fast" is the same number in the kernel source, the
    header comment and the Python constant the tests reset it to."""
    lib = _lib.load()
    assert lib.ymk_debug_option(b"no_such_option", 1) != 0
    for key, default in (("conv_fast", _lib.CONV_FAST_DEFAULT), ("conv_variant", 0), ("no_splitk", 0), ("splitk_force", -1),
                         ("conv_split", -1), ("conv_split_tile", 0), ("prof_dump", 0), ("dec_rows", 0), ("parseq_no_rowmax", 0), ("amax_check", 0), ("rowmax_tile", 0), ("astat", 1), ("act_planes", 1), ("ar_publish", 1)):
        assert lib.ymk_debug_option(key.encode(), default) == 0, key
    # "conv_split_tile" takes the selectors the routing code knows and nothing else: a retired or mistyped one is an error,
    # never a run of the default tile under another label
    try:
        for tile in (0, 1, 3, 21, 30):
            assert lib.ymk_debug_option(b"conv_split_tile", tile) == 0, tile
        for tile in (2, 4, 11, 20, 5, 10, 12, 14, 99, -1):
            assert lib.ymk_debug_option(b"conv_split_tile", tile) != 0, tile
            assert lib.ymk_last_error(), tile
        for variant in (0, 1, 2, 3, 4, 7, 8):
            assert lib.ymk_debug_option(b"conv_variant", variant) == 0, variant
        for variant in (5, 6, 9, -1):  # 5 / 6: the two-tiles-ahead loads, retired
            assert lib.ymk_debug_option(b"conv_variant", variant) != 0, variant
            assert lib.ymk_last_error(), variant
        for tile in (0, 6):
            assert lib.ymk_debug_option(b"rowmax_tile", tile) == 0, tile
        for tile in (1, 2, 3, 4, 5, 7, -1):
            assert lib.ymk_debug_option(b"rowmax_tile", tile) != 0, tile
            assert lib.ymk_last_error(), tile
    finally:
        assert lib.ymk_debug_option(b"conv_split_tile", 0) == 0
        assert lib.ymk_debug_option(b"rowmax_tile", 0) == 0
        assert lib.ymk_debug_option(b"conv_variant", 0) == 0
    src = open(os.path.join(ROOT, "yomitoku_amd", "csrc", "ymk_conv.hip")).read()
    assert int(re.search(r"g_conv_fast\{(\d+)\}", src).group(1)) == _lib.CONV_FAST_DEFAULT
    header = open(os.path.join(ROOT, "include", "ymk.h")).read()
    assert int(re.search(r'"conv_fast" \((\d+)\)', header).group(1)) == _lib.CONV_FAST_DEFAULT


def test_library_loads_with_roctx_ranges_asked_for():
    """YMK_ROCTX=1: the marker library is looked up at run time (dlopen) at the first range - asking for ranges must never be
    the reason the library does not load or a host-only entry point fails, with or without a marker library on the box."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from yomitoku_amd import _lib; l = _lib.load(); assert l.ymk_version() >= 100; print(l.ymk_device_count() >= -1)"
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, YMK_ROCTX="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("True"), r.stderr[-500:]
