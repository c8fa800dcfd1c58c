"""Pin the non-autoregressive PARSeq mode (decode_ar = 0) against the REFERENCE's own class, on the CPU:

    python -m tools.pin_parseq_nar

writes tests/golden/parseq_ref_nar.npz.  The reference module is imported the way oracle/pin_against_reference.py does
(same helpers, the seeded checkpoints and the input generator of the parseq_ref_* goldens); it only runs where the reference's
sources are available.  Per case the file keeps the checkpoint kwargs, the config scalars, the arg-max tokens, the max
logit per row, a strided sample of the logits, and the smallest top-1 / top-2 margin over the rows up to each sample's
first <eos>.  The script refuses seeds whose margin is below MIN_MARGIN: a token comparison on the device (logit
tolerance 1e-3) is then a statement about the kernels, not a coin toss - at every pass, since the tokens of one pass are
the context of the next (the refine_iters = 0 / 1 outputs are the intermediate stages of the refine_iters = 2 case).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MIN_MARGIN = 1e-2  # ten times the project's logit tolerance (tests/test_parseq_gpu.py: LOGIT_TOL)
STRIDE = 293       # class stride of the kept logit sample

LITE = dict(patch=[4, 8], dim=192, heads=6, num_tokens=7121)
WIDE = dict(patch=[8, 8], dim=512, heads=8, num_tokens=7312)
# (tag, geometry, synth.parseq_state_dict kwargs, refine_iters).  Seeds: the first of 1235.. (lite) / 77.. (wide) at the
# <eos> bias of parseq_ref_eos whose margin passes at every pass AND whose samples are not all empty strings (with random
# weights a 101-row sequence has a ~1e-3 margin somewhere: the <eos> bias keeps the decisive prefix short)
CASES = [
    ("lite_r1", LITE, dict(seed=1239, eos_bias=4.5, enc_depth=2), 1),
    ("lite_r0", LITE, dict(seed=1239, eos_bias=4.5, enc_depth=2), 0),
    ("lite_r2", LITE, dict(seed=1239, eos_bias=4.5, enc_depth=2), 2),
    ("wide_r1", WIDE, dict(seed=79, eos_bias=4.5, patch=(8, 8), enc_dim=512, dec_dim=512, num_tokens=7312, enc_depth=2), 1),
]
INPUT = dict(seed=11, batch=2, width=96)  # synthetic_line_batch arguments (seed and width of the parseq_ref_* goldens)


def _margin(logits: torch.Tensor) -> float:
    """Smallest top-1 - top-2 over the rows up to and including each sample's first <eos> (class 0)."""
    worst = float("inf")
    ids = logits.argmax(-1)
    for b in range(logits.shape[0]):
        eos = (ids[b] == 0).nonzero()
        last = int(eos[0]) if len(eos) else logits.shape[1] - 1
        top2 = logits[b, : last + 1].topk(2, dim=-1).values
        worst = min(worst, float((top2[:, 0] - top2[:, 1]).min()))
    return worst


def _run(mod, geo, kw, refine, x):
    from types import SimpleNamespace

    from oracle.pin_against_reference import AttrDict
    from yomitoku_amd.utils.synth import parseq_state_dict

    depth = kw["enc_depth"]
    rcfg = AttrDict(
        max_label_length=100, decode_ar=0, refine_iters=refine, num_tokens=geo["num_tokens"], data={"img_size": [32, 800]},
        encoder={"patch_size": geo["patch"], "num_heads": geo["heads"], "embed_dim": geo["dim"], "mlp_ratio": 4, "depth": depth},
        decoder={"embed_dim": geo["dim"], "num_heads": geo["heads"], "mlp_ratio": 4, "depth": 1},
    )
    model = mod.PARSeq(rcfg)
    model.load_state_dict(parseq_state_dict(**kw), strict=True)
    model.eval()
    model.tokenizer = SimpleNamespace(eos_id=0, bos_id=geo["num_tokens"] - 2, pad_id=geo["num_tokens"] - 1)
    with torch.inference_mode():
        return model(x)


def main():
    from oracle.pin_against_reference import GOLDEN, ref_import
    from yomitoku_amd.utils.synth import synthetic_line_batch

    mod = ref_import("yomitoku.models.parseq")
    x = synthetic_line_batch(INPUT["seed"], INPUT["batch"], INPUT["width"])
    out = {"x": x.numpy(), "input": np.array(repr(INPUT)), "tags": np.array([c[0] for c in CASES]), "stride": STRIDE}
    for tag, geo, kw, refine in CASES:
        ref = _run(mod, geo, kw, refine, x)
        assert ref.shape == (INPUT["batch"], 101, geo["num_tokens"] - 2), ref.shape
        margin = _margin(ref)
        # the passes before the last one feed it their tokens: their margins count too
        stages = [_margin(_run(mod, geo, kw, r, x)) for r in range(refine)]
        ids = ref.argmax(-1)
        lens = [int((row == 0).nonzero()[0]) if (row == 0).any() else len(row) for row in ids]
        print(f"[parseq-nar/{tag}] refine {refine}: lengths {lens}, margin {margin:.4f}, earlier passes {[round(m, 4) for m in stages]}")
        assert min([margin] + stages) >= MIN_MARGIN, f"{tag}: top-1/top-2 margin below {MIN_MARGIN}: pick another seed"
        out[f"{tag}_ckpt"] = np.array(repr(kw))
        out[f"{tag}_cfg"] = np.array(repr(dict(geo, refine_iters=refine, decode_ar=0, max_label_length=100, enc_depth=kw["enc_depth"])))
        out[f"{tag}_ids"] = ids.numpy().astype(np.int16)
        out[f"{tag}_top"] = ref.max(-1).values.numpy()
        out[f"{tag}_sample"] = ref[:, :, ::STRIDE].numpy()
        out[f"{tag}_margin"] = np.float32(margin)
    path = os.path.join(GOLDEN, "parseq_ref_nar.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
