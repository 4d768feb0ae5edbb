"""Output formats: the device conversion against the nearest route the library offered before it, in one process: one 30 s, 24 kHz wave, delivered
as 8 kHz mu-law (a telephony leg) and as 48 kHz PCM16 (a player).

Both sides start from the finished float wave on the device and end with the codes as a numpy array on the host:
  before  `frontend.resample` (f5_frontend_resample: the fp32 FIR of the reference-voice input side), a copy of the float result to the host, and
          numpy there: `(x * 32767).astype(int16)` with clipping, then `infer.deliver.g711_encode` for mu-law
  device  `infer.deliver.convert_wave` (csrc/deliver.hip: ordered fp64 sums, PCM and G.711 in the same kernel), then a copy of the codes
Each side copies into a pinned host buffer of its own, allocated once, as a server would: a `.cpu()` into fresh pageable memory was measured at up
to 27 ms for the 2.9 MB of the 48 kHz result (the runtime pins the pages first), whichever side makes it, and would bury both sides' work.
The two resamplers do not promise each other's bits (fp32 against fp64 sums), so the sides are compared by the share of codes that differ, not byte
for byte; the device side's own contract is tests/test_gpu_output_format.py.  Timed with a host clock around work that ends in a device
synchronise; warm-up of both sides, then the sides alternate.  No pass mark: the numbers are a record.

    python tools/deliver_ab.py [--reps 9] [--warmup 3] [--out profiles/deliver_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eraxvif5tts_amd import _lib, frontend  # noqa: E402
from eraxvif5tts_amd.infer import deliver as D  # noqa: E402

SR, SECONDS = 24000, 30.0
CASES = [(8000, "mulaw"), (48000, "pcm16")]


def make_wave(dtype):
    g = np.random.default_rng(0)
    t = np.arange(int(SECONDS * SR)) / SR
    x = 0.25 * np.sin(2 * np.pi * 180 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.1 * np.sin(2 * np.pi * 2300 * t) + 0.02 * g.standard_normal(len(t))
    return x.astype(dtype)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = _lib.require_gpu()
    lines = [f"Output formats: the route before (fp32 resampler, float copy, numpy encoding) against the device conversion ({name}; one process, the "
             "sides alternate)",
             f"wave: {SECONDS:.0f} s at {SR} Hz ({int(SECONDS * SR)} samples) on the device; result: the codes on the host",
             f"{args.warmup} warm-up calls, then {args.reps} timed calls per side; median (min .. max) in ms, device -> host copy included", ""]
    for dtype in (np.float32, np.float64):
        dev = torch.from_numpy(make_wave(dtype)).cuda()
        for rate, enc in CASES:
            count = D.converted_length(len(dev), SR, rate)
            pin_f = torch.empty(count, dtype=torch.float32, pin_memory=True)
            pin_c = torch.empty(count, dtype=torch.int16 if enc == "pcm16" else torch.uint8, pin_memory=True)

            def landed(pin, t):  # device tensor -> the side's pinned buffer, as an array
                pin.copy_(t, non_blocking=True)
                torch.cuda.synchronize()
                return pin.numpy()

            def before():
                x = landed(pin_f, frontend.resample(dev.to(torch.float32), SR, rate))
                pcm = np.clip(np.trunc(x * np.float32(32767.0)), -32768, 32767).astype(np.int16)
                return D.g711_encode(pcm, enc) if enc != "pcm16" else pcm

            def device():
                return landed(pin_c, D.convert_wave(dev, SR, rate, enc, want_float=False, want_codes=True)[1])

            b, d = before().copy(), device().copy()
            assert b.shape == d.shape and b.dtype == d.dtype
            differ = float((b != d).mean())
            for _ in range(args.warmup):
                before()
                device()
            tb, td = [], []
            for _ in range(args.reps):
                tb.append(timed(before)[0])
                td.append(timed(device)[0])
            # where each side's time goes: the conversion alone (synchronised, nothing copied) and the copy of its result alone
            held_b, held_d = frontend.resample(dev.to(torch.float32), SR, rate), D.convert_wave(dev, SR, rate, enc, want_float=False, want_codes=True)[1]
            parts = {}
            for key, fn in (("before: resample", lambda: frontend.resample(dev.to(torch.float32), SR, rate)), ("before: copy", lambda: landed(pin_f, held_b)),
                            ("device: convert", lambda: D.convert_wave(dev, SR, rate, enc, want_float=False, want_codes=True)), ("device: copy", lambda: landed(pin_c, held_d))):
                parts[key] = statistics.median(timed(fn)[0] for _ in range(args.reps))
            mb, md = statistics.median(tb), statistics.median(td)
            lines += [f"{np.dtype(dtype).name} wave -> {rate} Hz {enc}: {len(d)} codes; {100 * differ:.3f} % differ between the sides (fp32 against fp64 sums)",
                      f"    before  {mb:9.3f} ({min(tb):.3f} .. {max(tb):.3f})",
                      f"    device  {md:9.3f} ({min(td):.3f} .. {max(td):.3f})",
                      f"    before / device = {mb / md:.1f}",
                      "    of which " + ", ".join(f"{k} {v:.3f}" for k, v in parts.items()), ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
