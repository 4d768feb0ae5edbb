"""Several independent requests: F5TTSWrapper.generate_batch() against the serial route a server has today -- one generate() per request
with that request's voice installed and its settings (the right-hand side of generate_batch's contract).  F5TTS_Base and Vocos at the
published size with random weights (built as bench.py builds them), three voices with synthetic prompts of 4 to 7 s, one-chunk requests of
6 to 10 s, NFE 32, bf16.  Four request mixes:

    a   8 requests, one voice, equal settings
    b   the same 8 texts over three voices and three guidance strengths
    c   2 requests
    d   8 requests with 8 different nfe_step values: every sampler group has one job, which prices the planner's overhead

    python tools/generate_batch_ab.py [--repeats 5] [--out FILE.md] [--json FILE]

Both routes run in the same process, alternating, after one warm-up of each per mix; wall clock from the call to the arrays in the caller's
hands, device synchronised before the start.  Reported per mix and route: median and range (min .. max) over the repeats, whether every
request's array was byte-equal after the same seed in every repeat, and the verdict by the rule the table states."""
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
ap.add_argument("--out", default=None, help="write the table (markdown) to this file")
ap.add_argument("--json", default=None, help="also write the result record to this file")
ap.add_argument("--nfe", type=int, default=32)
ap.add_argument("--precision", default="bf16")
args = ap.parse_args()
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (synth_weights: the random initialisation of the benchmark)
from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.infer import audio  # noqa: E402
from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper, TTSJob  # noqa: E402
from eraxvif5tts_amd.vocos import Vocos  # noqa: E402
from oracle import cpu_ref  # noqa: E402  (only its seeded weight generator)

SR = 24000
# (name, seconds, amplitude, Hz, reference text)
PROMPTS = [("main", 4.0, 0.08, 190, "a steady tone, held for four seconds."),
           ("anna", 5.5, 0.05, 260, "a second and somewhat higher tone, held a little longer."),
           ("bert", 7.0, 0.30, 120, "a third tone, low and loud, which is held for all of seven seconds.")]
LINES = ["the quick brown fox jumps over the lazy dog and then runs all the way back",
         "nobody had expected the rain to start so early in the afternoon, and nobody had an umbrella",
         "if you take the second road on the left you will reach the harbour before dark",
         "she counted the boxes twice and wrote the number down in the little book she carried"]
TEXTS = [LINES[i % len(LINES)] + "." for i in range(8)]
VOICES = ["main", "anna", "bert", "anna", "main", "bert", "main", "anna"]
GUIDANCE = [2.0, 1.5, 3.0, 2.0, 3.0, 1.5, 2.0, 1.5]


def mixes(nfe):
    return {"a: 8 requests, one voice, equal settings": [TTSJob(t, nfe_step=nfe) for t in TEXTS],
            "b: 8 requests, three voices, three guidance strengths": [TTSJob(t, voice=v, cfg_strength=c, nfe_step=nfe)
                                                                      for t, v, c in zip(TEXTS, VOICES, GUIDANCE)],
            "c: 2 requests": [TTSJob(t, voice=v, nfe_step=nfe) for t, v in zip(TEXTS[:2], VOICES[:2])],
            "d: 8 requests, 8 different nfe_step": [TTSJob(t, voice=v, nfe_step=nfe - 7 + i) for i, (t, v) in enumerate(zip(TEXTS, VOICES))]}


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

    def serial(reqs):
        outs = []
        for q in reqs:
            with installed(tts, voices[q.voice]):
                outs.append(tts.generate(q.text, nfe_step=q.nfe_step, cfg_strength=q.cfg_strength, return_numpy=True)[0])
        return outs

    def batch(reqs):
        return [r[0] for r in tts.generate_batch(reqs)]

    def timed(fn, reqs, seed):
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            out = fn(reqs)
        return (time.perf_counter() - t0) * 1e3, out

    rec = {"nfe": args.nfe, "precision": args.precision, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "voices": {n: round(v["audio"].shape[-1] / SR, 2) for n, v in voices.items()}, "mixes": {}}
    for name, reqs in mixes(args.nfe).items():
        rows = {"serial_ms": [], "generate_batch_ms": []}
        equal, secs = [], []
        for rep in range(-1, args.repeats):  # (-1: the warm-up of each route, not recorded)
            s_ms, a = timed(serial, reqs, 100 + rep)
            b_ms, b = timed(batch, reqs, 100 + rep)
            same = len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
            if rep >= 0:
                rows["serial_ms"].append(s_ms)
                rows["generate_batch_ms"].append(b_ms)
                equal.append(bool(same))
            secs = [round(len(x) / SR, 2) for x in a]
        med = {k: statistics.median(v) for k, v in rows.items()}
        rng = {k: [min(v), max(v)] for k, v in rows.items()}
        spread = rng["serial_ms"][1] - rng["serial_ms"][0]
        lost = med["generate_batch_ms"] > med["serial_ms"] + spread
        rec["mixes"][name] = {"requests": len(reqs), "seconds": secs, "median_ms": {k: round(v, 2) for k, v in med.items()},
                              "min_max_ms": {k: [round(x, 2) for x in v] for k, v in rng.items()},
                              "all_ms": {k: [round(x, 2) for x in v] for k, v in rows.items()}, "byte_equal": equal,
                              "serial_spread_ms": round(spread, 2), "serial_over_batch": round(med["serial_ms"] / med["generate_batch_ms"], 3),
                              "lost": bool(lost)}
    print(json.dumps(rec), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rec, fh, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("# generate_batch() against one generate() per request\n\n")
            fh.write("`tools/generate_batch_ab.py`: both routes in one process, alternating, one warm-up each per mix, "
                     f"{args.repeats} repeats; wall clock in ms from the call to the arrays on the host.\n")
            fh.write(f"Device {rec['device']}; F5TTS_Base + Vocos, random weights, {args.precision}, NFE {args.nfe}; "
                     f"voices (prompt seconds): {rec['voices']}.\n\n")
            fh.write("A mix counts as lost when the batch route's median is slower than the serial median by more than the serial route's own "
                     "range (max - min) over its repeats.\n\n")
            fh.write("| mix | serial median (min .. max) | generate_batch median (min .. max) | serial / batch | serial range | byte-equal per repeat | verdict |\n")
            fh.write("|---|---|---|---|---|---|---|\n")
            for name, m in rec["mixes"].items():
                s, b = m["min_max_ms"]["serial_ms"], m["min_max_ms"]["generate_batch_ms"]
                fh.write(f"| {name} | {m['median_ms']['serial_ms']:.2f} ({s[0]:.2f} .. {s[1]:.2f}) | "
                         f"{m['median_ms']['generate_batch_ms']:.2f} ({b[0]:.2f} .. {b[1]:.2f}) | {m['serial_over_batch']:.3f} | "
                         f"{m['serial_spread_ms']:.2f} | {m['byte_equal']} | {'lost' if m['lost'] else 'kept'} |\n")
            fh.write("\nSeconds of audio per request:\n\n")
            for name, m in rec["mixes"].items():
                fh.write(f"- {name}: {m['seconds']}\n")


if __name__ == "__main__":
    main()
