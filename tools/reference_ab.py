"""The reference-voice front-end, host route against device route, in one process: five constructed clips (16-bit PCM) at the reference's values.

Both sides start from the decoded `audio.Segment` and end with what `F5TTSWrapper._preprocess_voice` returns: the fp32 wave on the device at
24 kHz, upload and resampler included.
  host    `audio.clip_reference`, `audio.remove_silence_edges`, the 50 ms pad, `segment_to_float`, the mono mean, torch's rms and boost on the
          CPU, one copy of the float wave to the device, the device resampler
  device  `infer.reference.prepare_reference_device` (one copy of the int16 PCM to the device, csrc/reference.hip, two small reads), the device
          resampler
Timed with a host clock around work that ends in a device synchronise; warm-up of both sides, then the sides alternate.  Before anything is timed
the two results are compared: equal length, and equal within rtol 1e-5 (the device route divides by the exact rms, the host by torch's fp32 one;
the line says whether the two rms values had the same bits).  No pass mark: the numbers are a record.

    python tools/reference_ab.py [--reps 7] [--warmup 2] [--out profiles/reference_ab.txt]
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
from eraxvif5tts_amd.infer import audio  # noqa: E402
from eraxvif5tts_amd.infer.reference import prepare_reference_device  # noqa: E402

TARGET_SR, TARGET_RMS = 24000, 0.1


def pattern(piece, total):
    out, t = [], 0.0
    while t < total - 1e-9:
        for kind, secs in piece:
            out.append((kind, min(secs, total - t)))
            t += out[-1][1]
            if t >= total - 1e-9:
                break
    return out


# (label, rate, channels, layout of (kind, seconds), the message the host route shows)
CLIPS = [
    ("6 s at 24 kHz, nothing to clip", 24000, 1, [("speech", 6.0)], None),
    ("20 s at 24 kHz, long pauses", 24000, 1, pattern([("speech", 3.6), ("pause", 1.4)], 20.0), 1),
    ("20 s at 24 kHz, short pauses", 24000, 1, pattern([("speech", 1.2), ("pause", 0.28)], 20.0), 2),
    ("15 s at 44.1 kHz stereo, no pause", 44100, 2, [("speech", 15.0)], 3),
    ("30 s at 48 kHz, long pauses", 48000, 1, pattern([("speech", 3.6), ("pause", 1.4)], 30.0), 1),
]


def make_clip(rate, channels, layout):
    g = np.random.default_rng(0)
    cols = []
    for _ in range(channels):
        parts = []
        for kind, secs in layout:
            n = int(round(secs * rate))
            t = np.arange(n) / rate
            amp = 2600.0 if kind == "speech" else 15.0
            parts.append(amp * (0.8 * np.sin(2 * np.pi * 180 * t + g.uniform(0, 6)) + 0.2 * np.sin(2 * np.pi * 1900 * t)) + g.normal(0, amp / 8, n))
        cols.append(np.concatenate(parts))
    return audio.Segment(np.clip(np.round(np.stack(cols, axis=1)), -32768, 32767).astype(np.int32), rate, 2)


def host_route(seg, said):
    aseg = audio.clip_reference(seg, said.append)
    aseg = audio.remove_silence_edges(aseg)
    aseg = aseg + aseg.silent_like(50)
    x = audio.segment_to_float(aseg)
    if x.shape[0] > 1:
        x = torch.mean(x, dim=0, keepdim=True)
    rms = torch.sqrt(torch.mean(torch.square(x)))
    if rms < TARGET_RMS:
        x = x * TARGET_RMS / rms
    x = x.cuda()
    return (audio.resample(x, seg.frame_rate, TARGET_SR) if seg.frame_rate != TARGET_SR else x), rms


def device_route(seg, said):
    x, sr, rec = prepare_reference_device(seg, True, TARGET_RMS, said.append)
    return (audio.resample(x, sr, TARGET_SR) if sr != TARGET_SR else x), rec


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
    lines = [f"Reference-voice front-end: host route against device route ({name}; one process, the sides alternate)",
             "from the decoded 16-bit Segment to the fp32 wave on the device at 24 kHz (what _preprocess_voice returns): upload and resampler included",
             f"{args.warmup} warm-up calls, then {args.reps} timed calls per side; median (min .. max) in ms", ""]
    for label, rate, channels, layout, number in CLIPS:
        seg = make_clip(rate, channels, layout)
        said_h, said_d = [], []
        (hw, hrms), (dw, rec) = host_route(seg, said_h), device_route(seg, said_d)
        assert said_h == said_d == ([f"Audio is over 12s, clipping short. ({number})"] if number else []), (label, said_h, said_d)
        assert hw.shape == dw.shape, "the two routes disagree in length"
        if rate == TARGET_SR:  # (behind the resampler a sample near zero has no relative bound)
            torch.testing.assert_close(dw, hw, rtol=1e-5, atol=0)
        same_rms = np.float32(hrms.item()).view(np.uint32) == rec["rms32"].view(np.uint32)
        for _ in range(args.warmup):
            host_route(seg, [])
            device_route(seg, [])
        th, td = [], []
        for _ in range(args.reps):
            th.append(timed(lambda: host_route(seg, []))[0])
            td.append(timed(lambda: device_route(seg, []))[0])
        mh, md = statistics.median(th), statistics.median(td)
        verdict = "the device route is faster" if md < mh else "the device route is NOT faster"
        lines += [f"{label}: {seg.samples.shape[0]} frames in, {rec['kept']} kept + {rec['out_frames'] - rec['kept']} pad, "
                  f"message {'(%d)' % number if number else 'none'}, rms32 {float(rec['rms32']):.6f} "
                  f"({'the same bits as' if same_rms else 'other bits than'} the host's fp32 rms), boost {rec['boost']}",
                  f"    host    {mh:9.3f} ({min(th):.3f} .. {max(th):.3f})",
                  f"    device  {md:9.3f} ({min(td):.3f} .. {max(td):.3f})",
                  f"    host / device = {mh / md:.1f}: {verdict}", ""]
    lines += ["What is timed: host = audio.clip_reference + audio.remove_silence_edges (Python loops over windows and milliseconds), pad, float",
              "conversion, mean, rms and boost on the CPU, the copy of the float wave, the device resampler; device = the copy of the int16 PCM,",
              "f5_op_reference_plan (five launches), one read of the counts and the part table, f5_reference_prepare (three launches), a second",
              "small read for the record, the device resampler.  Host clock around work that ends in a device synchronise",
              "(python tools/reference_ab.py).  No pass mark is attached; the default route stays the host's."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
