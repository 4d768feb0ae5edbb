"""Same-process A/B of the fp16 precision mode against the bf16 production mode (the same-box A/B form).

One process holds F5TTS_Base twice -- precision "bf16" and "fp16" -- with the same synthetic weights (bench.synth_weights behind the same
torch seed) and times alternating sample() calls with HIP events at 1 x 1024, 4 x 1024 and 32 x 1024 frames, NFE 8, CFG 2 (hipGraph
replay, as bench.py times it).  The bf16 mode pre-scales q and the fp16 mode cannot, so the bf16 model is also timed
with the plan option attn_prescale = 0: the column that compares like with like.  Where the fp16 mode is slower than the bf16 mode as it
ships by more than 3 %, an eager sample() of each model with the in-situ event pairs (f5_plan_timing_site) names the call site.

    python tools/precision_ab.py [--out profiles/fp16_mode_ab.md] [--shapes 1x1024,4x1024,32x1024] [--reps 7]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.model import CFM, DiT  # noqa: E402

NFE, CFG = 8, 2.0


def make(prec):
    torch.manual_seed(1234)  # DiT's default init draws from the global RNG: the same weights for every precision
    model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision=prec), seed=0)
    return CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()


def set_plan_option(cfm, key, value):
    for _, h in cfm.transformer._plans:
        _lib.check(_lib.load().f5_plan_set_option(h, key, value))


def timed(cfm, kw):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    cfm.sample(**kw)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def site_table(cfm, B, N, kw):
    lib = _lib.load()
    plan = cfm.transformer.plan(B, N, NFE)
    ms, cnt = C.c_float(0.0), C.c_int(0)
    _lib.check(lib.f5_plan_timing_begin(plan, (7 * bench.BASE_ARCH["depth"] + 4) * NFE), "timing_begin")
    cfm.sample(**{**kw, "use_graph": False})
    _lib.check(lib.f5_plan_timing_end(plan, C.byref(ms), C.byref(cnt), _lib.stream_ptr()), "timing_end")
    out = {}
    for i, name in enumerate(_lib.SITES):
        a, n = C.c_float(0.0), C.c_int(0)
        _lib.check(lib.f5_plan_timing_site(plan, i, C.byref(a), C.byref(n)), "timing_site")
        out[name] = (a.value * 1e3, n.value)  # us per launch, launches
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp16_mode_ab.md"))
    ap.add_argument("--shapes", default="1x1024,4x1024,32x1024")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    _lib.require_gpu()
    models = {"bf16": make("bf16"), "fp16": make("fp16")}
    lines = ["# fp16 precision mode against the bf16 production mode, same process", "",
             f"F5TTS_Base, synthetic weights, NFE {NFE}, CFG {CFG:g}, hipGraph replay; alternating `sample()` calls timed with HIP events, median of "
             f"{args.reps} (min - max).  `bf16, q as projected` is the bf16 model with the plan option `attn_prescale = 0`: the fp16 mode never "
             "pre-scales q, so this is the like-for-like column.  Written by `tools/precision_ab.py`.", "",
             "| shape | bf16 (ms) | bf16, q as projected (ms) | fp16 (ms) | fp16 / bf16 | fp16 / bf16 q as projected |", "|---|---|---|---|---|---|"]
    slow = []
    for shape in args.shapes.split(","):
        B, N = (int(v) for v in shape.split("x"))
        cond, text, lens, dur = bench.synth_batch(B, N, "cuda", seed=3)
        kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=NFE, cfg_strength=CFG, sway_sampling_coef=-1.0, seed=0, return_trajectory=False,
                  use_graph=True)
        legs = [("bf16", "bf16", -1), ("bf16_plain", "bf16", 0), ("fp16", "fp16", -1)]
        t = {k: [] for k, _, _ in legs}
        for rep in range(args.reps + 2):  # two warm-up rounds: capture + first replay
            for key, which, prescale in legs:
                cfm = models[which]
                cfm.transformer.plan(B, N, NFE)
                set_plan_option(cfm, b"attn_prescale", prescale)  # (drops the graphs captured under the other value: re-captured below)
                if which == "bf16":
                    cfm.sample(**kw)  # re-capture outside the timed call
                ms = timed(cfm, kw)
                if rep >= 2:
                    t[key].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        fmt = lambda k: f"{med[k]:.2f} ({min(t[k]):.2f} - {max(t[k]):.2f})"
        lines.append(f"| {B} x {N} | {fmt('bf16')} | {fmt('bf16_plain')} | {fmt('fp16')} | {med['fp16'] / med['bf16']:.3f} | {med['fp16'] / med['bf16_plain']:.3f} |")
        print(lines[-1], flush=True)
        if med["fp16"] > 1.03 * med["bf16"]:
            slow.append((B, N, kw))
    for B, N, kw in slow:
        set_plan_option(models["bf16"], b"attn_prescale", -1)
        sb, sh = site_table(models["bf16"], B, N, kw), site_table(models["fp16"], B, N, kw)
        lines += ["", f"## {B} x {N}: the fp16 mode is more than 3 % slower than the bf16 mode -- per call site (eager, in-situ event pairs; bf16 as it ships)", "",
                  "| site | launches | bf16 (us) | fp16 (us) | fp16 / bf16 |", "|---|---|---|---|---|"]
        for name in _lib.SITES:
            (ub, n), (uh, _) = sb[name], sh[name]
            if n:
                lines.append(f"| {name} | {n} | {ub:.1f} | {uh:.1f} | {uh / ub:.3f} |")
    if not slow:
        lines += ["", "No shape has the fp16 mode more than 3 % slower than the bf16 mode: no per-site table."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
