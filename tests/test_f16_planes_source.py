"""Host check over the kernel sources: the fp16-plane arithmetic and the by-value kernel argument of the fused ViT MLP each
have ONE definition.  The convolution tests hold the fp16-split kernels to bit identity with each other; that only stays
true while every kernel cuts its operands with the primitives of ymk_f16_planes.h, and a second `struct MlpK` would
corrupt kernel arguments without any diagnostic."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yomitoku_amd", "csrc")
PLANES_H = "ymk_f16_planes.h"


def _sources(*patterns):
    paths = sorted(p for pat in patterns for p in glob.glob(os.path.join(CSRC, pat)))
    assert paths
    return {os.path.basename(p): open(p).read() for p in paths}


def test_fp16_plane_arithmetic_and_mlpk_are_defined_once():
    every = _sources("*.h", "*.hip", "*.cpp")
    assert [n for n, s in every.items() if re.search(r"\bstruct\s+MlpK\s*\{", s)] == ["ymk_vit_mlp.h"]
    # the exponent clamp of the plane scale
    assert [n for n, s in every.items() if "268 - e" in s] == [PLANES_H]

    # the _Float16 vector types, whatever they are called and wherever they are declared
    f16_vectors = set()
    for s in every.values():
        f16_vectors.update(re.findall(r"typedef\s+_Float16\s+(\w+)\s+__attribute__\(\(ext_vector_type", s))
    assert {"f16x2", "f16x8"} <= f16_vectors
    to_f16 = re.compile(r"__builtin_convertvector\s*\((?:[^()]|\([^()]*\))*,\s*(?:%s)\s*\)" % "|".join(sorted(f16_vectors)))
    assert to_f16.search(every[PLANES_H]), "the pattern no longer finds the cut where it is known to be"
    for name, s in _sources("*.hip", "*.cpp").items():
        assert not re.search(r"typedef\s+_Float16\s+\w+\s+__attribute__\(\(ext_vector_type", s), f"{name}: a private fp16 vector type"
        assert not to_f16.search(s), f"{name}: cuts fp16 planes itself instead of through {PLANES_H}"
