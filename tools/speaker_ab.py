#!/usr/bin/env python
"""The speaker-similarity head on the device beside tests/speaker_ref.py: error figures and times.  Numbers only, no threshold.

    python tools/speaker_ab.py [--utterances 64] [--min-seconds 3] [--max-seconds 12] [--repeats 7] [--skip-errors]

Errors: every (width, T, op) case of tests/test_gpu_speaker.py -- rel-L2 and max-abs of the device and of the fp32 restatement, both against the
fp64 restatement on the same fp32 inputs.
Times: `--utterances` utterances of 3 .. 12 s (50 frames per second) at the production width (L 25, F 1024, C 512) through ONE ragged
SpeakerEncoder.embed call, against tests/speaker_ref.py's torch graph on the same GPU one utterance at a time -- the reference's route, since
run_sim is batch 1.  Both after warm-up calls, HIP events around each repeat, the median of the repeats; kernel launches per call counted by
torch.profiler.  Needs an MI355X."""
import argparse
import functools
import os
import statistics
import sys

import numpy as np
import torch

print = functools.partial(print, flush=True)  # the figures appear as they are measured
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speaker_ref as R  # noqa: E402
from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.eval import SpeakerEncoder  # noqa: E402


def errors():
    import test_gpu_speaker as G
    print("case                              rel-L2 gpu   rel-L2 ref32   ratio   max-abs gpu   max-abs ref32   max|ref64|")
    for name, T in G.SHAPES:
        for op in G.OPS:
            f = G.measure(name, T, op)
            print(f"{name:10s} T={T:<4d} {op:12s}   {f['rel_gpu']:.3e}    {f['rel_ref']:.3e}   {f['rel_gpu'] / f['rel_ref']:5.2f}    {f['max_gpu']:.3e}     "
                  f"{f['max_ref']:.3e}    {f['scale']:.3e}")


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        ms.append(start.elapsed_time(end))
    return statistics.median(ms), min(ms), max(ms)


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--min-seconds", type=float, default=3.0)
    ap.add_argument("--max-seconds", type=float, default=12.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-errors", action="store_true")
    a = ap.parse_args()
    print(_lib.require_gpu())
    if not a.skip_errors:
        errors()
    cfg = R.PRODUCTION_CONFIG
    P32 = R.filled_state(cfg)
    enc = SpeakerEncoder().load_state_dict(P32)
    rs = np.random.RandomState(0)
    frames = [int(round(50 * s)) for s in rs.uniform(a.min_seconds, a.max_seconds, a.utterances)]
    g = torch.Generator(device="cuda").manual_seed(0)
    utts = [torch.randn(cfg["layers"], t, cfg["feat_dim"], device="cuda", generator=g) for t in frames]
    Pd = {k: v.cuda() for k, v in P32.items()}
    packed = torch.cat(utts, dim=1).contiguous()  # what embed() builds from the list; timed without that copy below as well

    def ragged():
        return enc.embed(utts)

    def torch_route():
        with torch.no_grad():
            return torch.cat([R.forward(Pd, u, cfg) for u in utts])

    dev, ref = ragged(), torch_route()
    rel = float((dev.double() - ref.double()).norm() / ref.double().norm())
    print(f"\n{a.utterances} utterances, {min(frames)} .. {max(frames)} frames ({sum(frames)} in all, {packed.numel() * 4 / 2 ** 30:.2f} GiB of hidden states); "
          f"device vs torch-on-GPU embeddings rel-L2 {rel:.3e}")
    for label, fn in (("one ragged embed call (list in, concatenation included)", ragged),
                      ("torch restatement on the same GPU, one utterance at a time", torch_route)):
        med, lo, hi = timed(fn, 2, a.repeats)
        try:
            n = kernel_launches(fn)
        except Exception as e:  # noqa: BLE001
            n = f"not counted ({type(e).__name__})"
        print(f"{label:62s} median {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, {a.repeats} repeats)   device activities per call: {n}")


if __name__ == "__main__":
    main()
