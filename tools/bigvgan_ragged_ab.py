"""A/B in one process: BigVGAN.decode_ragged_buffer (one set of launches for all utterances) against the per-utterance `forward` loop that
`decode_utterances` ran before it (one generator pass per utterance, then torch.cat), on the generator at the published size
(bigvgan_v2_24khz_100band_256x shape, 112.4 M parameters, random initial weights: bench.py's recipe, no checkpoint offline).

Shapes: 8 x 683 frames (an 8-chunk generate() call), 4 x 300, and 32 lengths drawn from 50 .. 900 (an infer_prompts() bucket).  Timing by HIP
events on the current stream: warm-up of both sides, then REPS alternated repetitions per side; reported are the median and the spread
(max - min) of each side.  Prints a markdown table and one JSON line; --out writes the same to a file.

--group-frames sets the tuning key "bigvgan_group_frames" (the frame budget of one launch set; default: the library's) for the ragged side,
--extra adds two shapes between the small and the large ones (8 x 300, 4 x 683).

    python tools/bigvgan_ragged_ab.py [--reps 7] [--warmup 2] [--group-frames N] [--extra] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.bigvgan import BigVGAN  # noqa: E402
from oracle import cpu_ref  # noqa: E402  (only its seeded weight generator)

SHAPES = {"8 x 683": [683] * 8, "4 x 300": [300] * 4, "32 x (50 .. 900)": [int(x) for x in np.random.default_rng(5).integers(50, 901, 32)]}


def per_utterance_loop(voc, rows, row_start, frames):
    """decode_utterances(kind="bigvgan") as it was: the generator once per utterance, then one concatenation"""
    waves = [voc(rows[r: r + t].unsqueeze(0).permute(0, 2, 1)).reshape(-1) for r, t in zip(row_start, frames)]
    return torch.cat(waves), [int(w.numel()) for w in waves]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--group-frames", type=int, default=None)
    ap.add_argument("--extra", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5
    shapes = dict(SHAPES)
    if args.extra:
        shapes.update({"8 x 300": [300] * 8, "4 x 683": [683] * 4})
    if args.group_frames is not None:
        _lib.check(_lib.load().f5_tuning_set(b"bigvgan_group_frames", args.group_frames))
    W = cpu_ref.random_bigvgan_weights(cpu_ref.BIGVGAN_V2_24K_100BAND_256X, seed=1)
    W["conv_post.weight"] = W["conv_post.weight"] * 0.0015
    voc = BigVGAN()
    voc.load_state_dict(W)
    voc = voc.eval().cuda()
    results = {}
    for name, frames in shapes.items():
        g = torch.Generator().manual_seed(len(frames))
        rows = (torch.randn(sum(frames), 100, generator=g) * 2 - 3).clamp(math.log(1e-5), 3.0).cuda()
        starts = [int(x) for x in np.cumsum([0] + frames[:-1])]
        sides = {"ragged": lambda: voc.decode_ragged_buffer(rows, starts, frames), "loop": lambda: per_utterance_loop(voc, rows, starts, frames)}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        last = {}
        for _ in range(args.reps):
            for k, fn in sides.items():  # alternated: ragged, loop, ragged, loop, ...
                t, out = timed(fn)
                ms[k].append(t)
                last[k] = out[0]
        equal = bool(torch.equal(last["ragged"], last["loop"]))
        r = {k: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}
        slack = max(r["ragged"]["spread_ms"], r["loop"]["spread_ms"])
        results[name] = {"utterances": len(frames), "frames": sum(frames), **r, "bit_identical": equal,
                         "speedup": r["loop"]["median_ms"] / r["ragged"]["median_ms"],
                         "ragged_not_slower": r["ragged"]["median_ms"] <= r["loop"]["median_ms"] + slack}
        del rows, last
        torch.cuda.empty_cache()
    lines = ["| shape | frames | ragged median ms | ragged spread ms | loop median ms | loop spread ms | loop / ragged | bit-identical | not slower |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, r in results.items():
        lines.append(f"| {name} | {r['frames']} | {r['ragged']['median_ms']:.2f} | {r['ragged']['spread_ms']:.2f} | {r['loop']['median_ms']:.2f} | "
                     f"{r['loop']['spread_ms']:.2f} | {r['speedup']:.3f} | {r['bit_identical']} | {r['ragged_not_slower']} |")
    text = "\n".join(lines) + "\n\n" + json.dumps({"reps": args.reps, "warmup": args.warmup, "bigvgan_group_frames": args.group_frames or "default", "device": torch.cuda.get_device_name(0), "shapes": results})
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
