"""A script in several voices: F5TTSWrapper.generate_multi() against the serial route it replaces -- one generate() per tagged piece with
that voice's fields installed, the results joined with np.concatenate (the right-hand side of generate_multi's contract).  F5TTS_Base and
Vocos at the published size with random weights (built as bench.py builds them), three voices with synthetic prompts of 4 to 7 s, a 12-line
dialogue of 8 to 15 s per line, NFE 32, CFG 2, bf16.

    python tools/multi_voice_ab.py [--repeats 5] [--out FILE] [--json FILE]

Both routes run in the same process, alternating, after one warm-up of each (plans, workspaces and hipGraphs exist from then on); wall clock
from the call to the array in the caller's hands, device synchronised before the start.  Reported: median and spread (min .. max) of each
route over the repeats, and whether the two arrays are byte-equal after the same seed."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None, help="write the figures as text to this file")
ap.add_argument("--json", default=None, help="also write the result record to this file")
ap.add_argument("--nfe", type=int, default=32)
ap.add_argument("--cfg", type=float, default=2.0)
ap.add_argument("--precision", default="bf16")
args = ap.parse_args()
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (synth_weights: the random initialisation of the benchmark)
from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.infer import audio  # noqa: E402
from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper  # noqa: E402
from eraxvif5tts_amd.infer.utils_infer import split_voice_script  # noqa: E402
from eraxvif5tts_amd.vocos import Vocos  # noqa: E402
from oracle import cpu_ref  # noqa: E402  (only its seeded weight generator)

SR = 24000
# (name, seconds, amplitude, Hz, reference text)
PROMPTS = [("main", 4.0, 0.08, 190, "a steady tone, held for four seconds."),
           ("anna", 5.5, 0.05, 260, "a second and somewhat higher tone, held a little longer."),
           ("bert", 7.0, 0.30, 120, "a third tone, low and loud, which is held for all of seven seconds.")]
LINES = ["the quick brown fox jumps over the lazy dog and then runs all the way back home again",
         "nobody had expected the rain to start so early in the afternoon, and nobody had an umbrella",
         "if you take the second road on the left you will reach the harbour before it gets dark tonight",
         "she counted the boxes twice and wrote the number down in the little book she always carried"]
ORDER = ["main", "anna", "bert", "anna", "main", "bert", "main", "anna", "bert", "main", "bert", "anna"]
SCRIPT = " ".join(f"[{v}] {LINES[i % len(LINES)]}." for i, v in enumerate(ORDER))


class RandomInitWrapper(F5TTSWrapper):
    """no checkpoint exists offline: the weights bench.py measures with"""

    def _load_checkpoint(self, model, ckpt_path, dtype=None, use_ema=True):
        bench.synth_weights(model.transformer)
        return model.to(self.device)


@contextlib.contextmanager
def installed(tts, voice):
    kept = tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len
    tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len = voice["audio"], voice["ref_text"], voice["ref_audio_len"]
    try:
        yield
    finally:
        tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len = kept


def main():
    _lib.require_gpu()
    torch.manual_seed(0)  # DiT() draws its non-zero initial weights from the global generator
    voc = Vocos()
    V = cpu_ref.random_vocos_weights(seed=3)
    voc.load_state_dict({k: t for k, t in V.items() if k in voc.state_dict()}, strict=False)
    with contextlib.redirect_stdout(io.StringIO()), tempfile.TemporaryDirectory() as tmp:
        tts = RandomInitWrapper(model_name="F5TTS_Base", ckpt_path="random-init", vocoder=voc.cuda(), precision=args.precision)
        for name, secs, amp, hz, text in PROMPTS:
            t = np.arange(int(secs * SR)) / SR
            path = os.path.join(tmp, name + ".wav")
            audio.write_wav(path, amp * np.sin(2 * np.pi * hz * t + 0.7) * (1 + 0.3 * np.sin(2 * np.pi * 5 * t)), SR)
            if name == "main":
                tts.preprocess_reference(path, text)
            else:
                tts.add_voice(name, path, text)
        voices = dict(tts.voices)
        pieces = split_voice_script(SCRIPT, voices)
        _, jobs, job_voices, seg_sizes = tts._plan_jobs(SCRIPT, tagged=True)
    assert len(pieces) == 12 and seg_sizes == [1] * 12, f"{len(pieces)} pieces, jobs per piece {seg_sizes}: a line is meant to be one chunk"
    line_secs = [(d - v["ref_audio_len"]) * 256 / SR for (_, d), v in zip(jobs, job_voices)]
    assert 8.0 <= min(line_secs) and max(line_secs) <= 15.0, line_secs
    kw = dict(nfe_step=args.nfe, cfg_strength=args.cfg, return_numpy=True)

    def serial():
        outs = []
        for name, piece in pieces:
            with installed(tts, voices[name]):
                outs.append(tts.generate(piece, **kw)[0])
        return np.concatenate(outs)

    def multi():
        return tts.generate_multi(SCRIPT, **kw)[0]

    def timed(fn, seed):
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    rows = {"serial_ms": [], "generate_multi_ms": []}
    equal = True
    for rep in range(-1, args.repeats):  # (-1: the warm-up of each route, not recorded)
        s_ms, a = timed(serial, 100 + rep)
        m_ms, b = timed(multi, 100 + rep)
        equal = equal and a.dtype == b.dtype and np.array_equal(a, b)
        if rep >= 0:
            rows["serial_ms"].append(s_ms)
            rows["generate_multi_ms"].append(m_ms)
    med = {k: round(statistics.median(v), 2) for k, v in rows.items()}
    spread = {k: [round(min(v), 2), round(max(v), 2)] for k, v in rows.items()}
    rec = {"voices": {n: round(v["audio"].shape[-1] / SR, 2) for n, v in voices.items()}, "lines": 12,
           "line_seconds": [round(x, 2) for x in line_secs], "frames": [d for _, d in jobs], "samples": int(len(b)), "nfe": args.nfe,
           "cfg": args.cfg, "precision": args.precision, "repeats": args.repeats, "median_ms": med, "min_max_ms": spread,
           "all_ms": {k: [round(x, 2) for x in v] for k, v in rows.items()}, "byte_equal": bool(equal),
           "serial_over_multi": round(med["serial_ms"] / med["generate_multi_ms"], 3), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rec, fh, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("tools/multi_voice_ab.py: generate_multi() against one generate() per piece, same process, alternating, one warm-up each\n")
            fh.write(f"device {rec['device']}; F5TTS_Base + Vocos, random weights, {args.precision}, NFE {args.nfe}, CFG {args.cfg}\n")
            fh.write(f"voices (prompt seconds): {rec['voices']}\n")
            fh.write(f"12 lines, one chunk each; seconds per line: {rec['line_seconds']}\n")
            fh.write(f"frames per utterance (prompt included): {rec['frames']}; {rec['samples']} output samples\n")
            for k in rows:
                fh.write(f"{k:18s} median {med[k]:9.2f}   min {spread[k][0]:9.2f}   max {spread[k][1]:9.2f}   all {rec['all_ms'][k]}\n")
            fh.write(f"serial / generate_multi (medians): {rec['serial_over_multi']}\n")
            fh.write(f"the two arrays are byte-equal after the same seed, in every repeat: {rec['byte_equal']}\n")


if __name__ == "__main__":
    main()
