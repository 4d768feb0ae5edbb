#!/usr/bin/env python
"""Device alignment search against the host restatement at a production size (default B = 8, nt = 200, T = 1500).

    python tools/align_ab.py [--batch 8] [--nt 200] [--frames 1500] [--seconds 1.0]

Device time per call from HIP events around a run of calls on one stream (after warm-up calls of the same shape, enough calls to fill
--seconds); host time of tests/alignment_ref.py (numpy, one run, wall clock) beside it, and the device results checked against it element
for element.  The host figure is the restatement's, not the reference's own Python double loop, which is slower still.  Needs an MI355X."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alignment_ref as R  # noqa: E402
from eraxvif5tts_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nt", type=int, default=200)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--seconds", type=float, default=1.0)
    a = ap.parse_args()
    name = _lib.require_gpu()
    lib = _lib.load()
    B, nt, T = a.batch, a.nt, a.frames
    rng = np.random.default_rng(0)
    sim_np = rng.standard_normal((B, nt, T)).astype(np.float32)
    band = np.abs(np.arange(nt)[:, None] * T // nt - np.arange(T)[None, :]) < max(3, T // 10)
    sim_np += 3.0 * band.astype(np.float32)  # the diagonal bias of the trainer's similarity
    sim = torch.from_numpy(sim_np).cuda()
    work = torch.empty(lib.f5_align_workspace(B, nt, T) // 4, dtype=torch.int32, device="cuda")
    dur = torch.empty(B, nt, device="cuda")
    ali = torch.empty(B, nt, T, device="cuda")
    print(f"{name}: B = {B}, nt = {nt}, T = {T}")
    for alg, fn in (("viterbi", lib.f5_align_viterbi), ("window", lib.f5_align_window)):
        t0 = time.perf_counter()
        want = R.SEARCH[alg](sim_np)
        host_s = time.perf_counter() - t0
        for label, out in (("alignment + durations", ali), ("durations only", None)):
            call = lambda: _lib.check(fn(B, nt, T, _lib.ptr(sim), _lib.ptr(dur), _lib.ptr(out), _lib.ptr(work), _lib.stream_ptr()), alg)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            calls, ms = 4, 0.0
            while True:  # grow the timed run until it fills the window
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(calls):
                    call()
                end.record()
                end.synchronize()
                ms = start.elapsed_time(end)
                if ms >= a.seconds * 1e3 or calls >= 1 << 16:
                    break
                calls *= 4
            same = np.array_equal(dur.cpu().numpy(), want.sum(axis=2)) and (out is None or np.array_equal(ali.cpu().numpy(), want))
            print(f"{alg:8s} {label:22s} device {ms / calls:9.4f} ms / call ({calls} calls in {ms:.0f} ms)   host restatement {host_s * 1e3:9.1f} ms"
                  f"   x{host_s * 1e3 / (ms / calls):8.1f}   equal: {same}")
            if not same:
                raise SystemExit("device and host disagree")


if __name__ == "__main__":
    main()
