"""Time to first audio of F5TTSWrapper.generate_stream() against generate(): F5TTS_Base and Vocos at the published size with random weights
(built as bench.py builds them), one synthetic 4 s prompt, a text that cuts into 8 chunks, NFE 32, CFG 2, bf16.

    python tools/stream_ttfa.py [--repeats 5] [--tree DIR] [--json OUT]

Per repeat, after one warm-up of every measured call (plans, workspaces and hipGraphs exist from then on), wall-clock with a device
synchronisation before the start:
  (a) first_piece_ms   generate_stream(return_pcm16=True): the call to the first piece in the caller's hands
  (c) stream_total_ms  the same stream, to exhaustion
  (b) generate_ms      generate(return_pcm16=True) over the same text
  (d) one_chunk_ms     generate(return_pcm16=True) of chunk 0 alone
Medians over the repeats.  ``--tree DIR`` imports the package from another checkout (a build of the parent commit: (b) and (d) there are the
figures the stream is compared with; a tree without generate_stream reports those two only).  The clocks `rocm-smi` shows are recorded before
and after (read only)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tree", default=None, help="import eraxvif5tts_amd (and bench.py's builders) from this checkout instead of this one")
ap.add_argument("--json", default=None, help="also write the result record to this file")
ap.add_argument("--nfe", type=int, default=32)
ap.add_argument("--cfg", type=float, default=2.0)
ap.add_argument("--precision", default="bf16")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (synth_weights: the random initialisation of the benchmark)
from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.infer import audio  # noqa: E402
from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper  # noqa: E402
from eraxvif5tts_amd.infer.utils_infer import chunk_text  # noqa: E402
from eraxvif5tts_amd.vocos import Vocos  # noqa: E402
from oracle import cpu_ref  # noqa: E402  (only its seeded weight generator)

SR = 24000
SENTENCE = "the quick brown fox jumps over the lazy dog and then runs back home again. "
TEXT = SENTENCE * 16  # two sentences per chunk at this prompt's byte budget: 8 chunks


class RandomInitWrapper(F5TTSWrapper):
    """no checkpoint exists offline: the weights bench.py measures with"""

    def _load_checkpoint(self, model, ckpt_path, dtype=None, use_ema=True):
        bench.synth_weights(model.transformer)
        return model.to(self.device)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:16]
    except Exception as e:  # noqa: BLE001
        return [f"rocm-smi unavailable: {e}"]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(t0)
    torch.cuda.synchronize()
    return out


def main():
    _lib.require_gpu()
    torch.manual_seed(0)  # DiT() draws its non-zero initial weights from the global generator
    voc = Vocos()
    V = cpu_ref.random_vocos_weights(seed=3)
    voc.load_state_dict({k: t for k, t in V.items() if k in voc.state_dict()}, strict=False)
    with contextlib.redirect_stdout(io.StringIO()):
        tts = RandomInitWrapper(model_name="F5TTS_Base", ckpt_path="random-init", vocoder=voc.cuda(), precision=args.precision)
        t = np.arange(int(4.0 * SR)) / SR
        wav = 0.08 * np.sin(2 * np.pi * 190 * t + 0.7) * (1 + 0.3 * np.sin(2 * np.pi * 5 * t)) + 0.02 * np.sin(2 * np.pi * 1370 * t)
        with tempfile.TemporaryDirectory() as tmp:
            audio.write_wav(os.path.join(tmp, "ref.wav"), wav, SR)
            tts.preprocess_reference(os.path.join(tmp, "ref.wav"), "a steady tone, held for four seconds.")
    secs = tts.ref_audio_processed.shape[-1] / SR
    chunks = chunk_text(TEXT, max_chars=int(len(tts.ref_text.encode("utf-8")) / secs * (22 - secs)))
    assert len(chunks) == 8, f"the text cuts into {len(chunks)} chunks, not 8"
    kw = dict(nfe_step=args.nfe, cfg_strength=args.cfg, return_pcm16=True)
    has_stream = hasattr(tts, "generate_stream")

    def whole(text):
        def run(t0):
            with contextlib.redirect_stdout(io.StringIO()):
                pcm, _ = tts.generate(text, return_numpy=True, **kw)
            return (time.perf_counter() - t0) * 1e3, len(pcm)
        return run

    def stream(t0):
        first, n = None, 0
        with contextlib.redirect_stdout(io.StringIO()):
            for pcm, _ in tts.generate_stream(TEXT, **kw):
                if first is None:
                    first = (time.perf_counter() - t0) * 1e3
                n += len(pcm)
        return first, (time.perf_counter() - t0) * 1e3, n

    before = clocks()
    rows = {"generate_ms": [], "one_chunk_ms": [], "first_piece_ms": [], "stream_total_ms": []}
    samples = {}
    for rep in range(-1, args.repeats):  # (-1: the warm-up, not recorded)
        torch.manual_seed(100 + rep)
        g_ms, samples["generate"] = timed(whole(TEXT))
        o_ms, samples["one_chunk"] = timed(whole(chunks[0]))
        if has_stream:
            f_ms, s_ms, samples["stream"] = timed(stream)
        if rep >= 0:
            rows["generate_ms"].append(g_ms)
            rows["one_chunk_ms"].append(o_ms)
            if has_stream:
                rows["first_piece_ms"].append(f_ms)
                rows["stream_total_ms"].append(s_ms)
    after = clocks()
    if has_stream:
        assert samples["stream"] == samples["generate"]
    med = {k: round(statistics.median(v), 2) for k, v in rows.items() if v}
    rec = {"tree": ROOT if args.tree else "this checkout", "has_generate_stream": has_stream, "chunks": len(chunks), "nfe": args.nfe, "cfg": args.cfg,
           "precision": args.precision, "repeats": args.repeats, "prompt_frames": tts.ref_audio_len, "samples": samples, "median_ms": med,
           "all_ms": {k: [round(x, 2) for x in v] for k, v in rows.items() if v}, "clocks_before": before, "clocks_after": after,
           "device": torch.cuda.get_device_name(0)}
    if has_stream:
        rec["first_piece_over_generate"] = round(med["first_piece_ms"] / med["generate_ms"], 4)
        rec["first_piece_over_one_chunk"] = round(med["first_piece_ms"] / med["one_chunk_ms"], 4)
        rec["stream_minus_generate_ms"] = round(med["stream_total_ms"] - med["generate_ms"], 2)
    print(json.dumps(rec), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
