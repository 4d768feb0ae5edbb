"""Silence removal, host route against device route, in one process: one constructed 30 s, 24 kHz wave with five pauses, at the reference's values
(min_silence_len 1000, silence_thresh -50, keep_silence 500, seek_step 10).

Both sides start from what the wave tail leaves on the device (the float wave and its truncating PCM) and end with the kept float wave as a numpy
array on the host:
  host    copy the whole wave to the host, then `utils_infer.remove_silence` on the array (`audio.split_sample_ranges`: the Python loop over windows)
  device  `utils_infer.remove_silence` on the device tensors (csrc/silence.hip), then copy the kept samples
Timed with a host clock around work that ends in a device synchronise; warm-up of both sides, then the sides alternate.  The results of the two
sides are compared byte for byte before anything is timed.  No pass mark: the numbers are a record.

    python tools/silence_ab.py [--reps 7] [--warmup 2] [--out profiles/silence_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.infer import utils_infer as U  # noqa: E402

SR = 24000
# (seconds, peak amplitude in int16 units): 30 s, pauses of 1.2, 1.5, 1.1, 2.0 and 1.3 s, one short pause that stays
LAYOUT = [(3.1, 9000), (1.2, 20), (4.4, 8000), (1.5, 0), (3.3, 9000), (0.6, 25), (2.9, 7000), (1.1, 30), (4.2, 9000), (2.0, 10), (3.0, 8000),
          (1.3, 0), (1.4, 6000)]


def make_wave(dtype):
    g = np.random.default_rng(0)
    parts = []
    for secs, amp in LAYOUT:
        n = int(round(secs * SR))
        t = np.arange(n) / SR
        parts.append(amp / 32767.0 * (0.8 * np.sin(2 * np.pi * 180 * t + g.uniform(0, 6)) + 0.2 * np.sin(2 * np.pi * 1900 * t)))
    return np.concatenate(parts).astype(dtype)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = _lib.require_gpu()
    lines = [f"Silence removal: host route against device route ({name}; one process, the sides alternate)",
             f"wave: {sum(s for s, _ in LAYOUT):.1f} s at {SR} Hz, five pauses of 1.1 .. 2.0 s, rule {U.SILENCE_DEFAULTS}",
             f"{args.warmup} warm-up calls, then {args.reps} timed calls per side; median (min .. max) in ms, device -> host copy included", ""]
    for dtype in (np.float32, np.float64):
        x = make_wave(dtype)
        dev = torch.from_numpy(x).cuda()
        pcm = torch.from_numpy(np.clip(np.trunc(x.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)).cuda()

        def host():
            return U.remove_silence(dev.cpu().numpy(), SR, pcm16=pcm.cpu().numpy())

        def device():
            kept, kept_pcm = U.remove_silence(dev, SR, pcm16=pcm)
            return kept.cpu().numpy(), kept_pcm.cpu().numpy()

        (hw, hp), (dw, dp) = host(), device()
        assert hw.tobytes() == dw.tobytes() and hp.tobytes() == dp.tobytes(), "the two routes disagree"
        for _ in range(args.warmup):
            host()
            device()
        th, td = [], []
        for _ in range(args.reps):
            th.append(timed(host)[0])
            td.append(timed(device)[0])
        mh, md = statistics.median(th), statistics.median(td)
        lines += [f"{np.dtype(dtype).name}: {len(x)} samples in, {len(dw)} kept (identical bytes from both routes)",
                  f"    host    {mh:9.3f} ({min(th):.3f} .. {max(th):.3f})",
                  f"    device  {md:9.3f} ({min(td):.3f} .. {max(td):.3f})",
                  f"    host / device = {mh / md:.1f}", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
