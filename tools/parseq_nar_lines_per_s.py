"""Recogniser lines/s in either decoding mode, one fresh process per measurement:

    python tools/parseq_nar_lines_per_s.py --decode-ar {0,1} [--repeats 3] [--tree DIR] [--out FILE]

The leg is the one bench.py reports as `lines_per_s_parseq-tiny-dynw-v4` (secondary_metrics): one TextRecognizer call
(dynamic_width, batch_bucketing) over the 2048-line synthetic sheet, 2 warm-up calls, then 3 timed calls per repeat.
`--tree DIR` measures another checkout of the project (the parent commit, built in DIR) with the same script;
`decode_ar` reaches the recogniser the way a user sets it: a YAML file given as `path_cfg`.  Prints one JSON line.
tools/parseq_nar_measure.sh chains the runs; profiles/parseq_nar_lines_per_s.json holds what they gave on the MI355X."""
import argparse
import json
import os
import sys
import tempfile
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode-ar", type=int, default=1, choices=[0, 1])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lines", type=int, default=2048)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    from yomitoku_amd import imaging
    from yomitoku_amd.text_recognizer import TextRecognizer
    from yomitoku_amd.utils.synth import parseq_state_dict, synthetic_line_sheet

    import bench  # REC_PRESETS: the checkpoint kwargs of the bench leg

    model = "parseq-tiny-dynw-v4"
    ckpt_kw, _, _ = bench.REC_PRESETS[model]
    device = torch.device("cuda:0")
    sheet, quads = synthetic_line_sheet(seed=1, n_lines=args.lines)
    page = imaging.page_to_device(sheet, device)
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "rec.yaml")
        with open(cfg, "w") as f:
            f.write(f"decode_ar: {args.decode_ar}\n")
        rec = TextRecognizer(model_name=model, path_cfg=cfg, from_pretrained=False, device=str(device), dynamic_width=True,
                             batch_bucketing=True)
    rec.model.load_state_dict(parseq_state_dict(**ckpt_kw))
    for _ in range(2):
        rec(page, quads)
    torch.cuda.synchronize()
    values = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(3):
            res = rec(page, quads)[0]
        torch.cuda.synchronize()
        values.append(round(3 * args.lines / (time.perf_counter() - t0), 1))
    out = {"decode_ar": args.decode_ar, "tree": os.path.abspath(args.tree), "lines_per_s": values, "lines_per_step": args.lines,
           "steps_per_repeat": 3, "last_forward_ar_steps": int(rec.model.last_ar_steps), "distinct_strings": len(set(res.contents))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    rec.model.close()


if __name__ == "__main__":
    main()
