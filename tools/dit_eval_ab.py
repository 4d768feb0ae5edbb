"""Bit identity of the network evaluation (csrc/dit_eval.hip, mmdit_eval.hip, unett_eval.hip) between two builds of the library.

  python tools/dit_eval_ab.py --parent-lib eraxvif5tts_amd/lib/libf5hip_parent.so [--report FILE]

runs the case list below once with the parent's build and once with this tree's (F5HIP_LIB selects the library; the Python side is the same), each
in a fresh child process under its own time limit -- the second child starts only if the first one exited 0 -- and compares every case's output
byte for byte.  No tolerance: the evaluation's host code may be rearranged, its launches may not change.

  python tools/dit_eval_ab.py --child DIR     one library: every case's output as DIR/<index>.bin
  python tools/dit_eval_ab.py --trace B N     one library: one eager B x N sample() and nothing else (run it under rocprofv3 --kernel-trace --stats)
  python tools/dit_eval_ab.py --time          one library: median wall time of an eager 1 x 256 sample() at NFE 32, F5TTS_Base

Model of the cases: a DiT of dim 1024, 16 heads, ff_mult 2, depth 3 (a fold needs block 1 for a folded QKV projection and block 2 for the
producer chain), seeded weights, 2 Euler steps, CFG 2."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARCH = dict(dim=1024, depth=3, heads=16, ff_mult=2, text_dim=512, text_mask_padding=False, conv_layers=4, pe_attn_head=1)
RAGGED = [300, 517, 411]  # per CFG half 320 + 544 + 432 = 1296 rows: 2592 token rows, no multiple of 256
KNOBS = ["ln_fold", "resid_rmw", "ln_defer", "residual_f16", "gemm_pad_rows", "ln_fold_inkernel", "gemm_w4", "w_prefetch"]
CHILD_TIMEOUT_S = 420


def _load_lib():
    from eraxvif5tts_amd import _lib
    return _lib.load()  # (the library F5HIP_LIB names, or this tree's)


def _dit(prec="bf16", **kw):
    import torch
    import bench
    from eraxvif5tts_amd.model import CFM, DiT
    torch.manual_seed(1234)
    model = bench.synth_weights(DiT(**ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision=prec, **kw), seed=0)
    return model, CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()


def _problem(B, N, seed):
    import torch
    import bench
    cond, text, lens, dur = bench.synth_batch(B, N, "cuda", seed=seed)
    y0 = torch.randn(B, N, 100, generator=torch.Generator().manual_seed(seed + 1))
    return dict(cond=cond, text=text, duration=dur, lens=lens, steps=2, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, return_trajectory=False,
                use_graph=False)


def _sample(cfm, B, N):
    return cfm.sample(**_problem(B, N, seed=B * 10000 + N))[0]


def _forward(model, B, N, seed, text_len=None):
    """one evaluation with per-sample times (f5_dit_forward / f5_mmdit_forward)"""
    import torch
    import bench
    g = torch.Generator().manual_seed(seed)
    x, cond = torch.randn(B, N, 100, generator=g), torch.randn(B, N, 100, generator=g) * 2 - 3
    text = torch.randint(0, bench.VOCAB, (B, text_len or N // 6), generator=g)
    t = torch.rand(B, generator=g)
    return model(x=x.cuda(), cond=cond.cuda(), text=text.cuda(), time=t.cuda(), drop_audio_cond=False, drop_text=False)


def cases(lib):
    """yields (name, output tensor); one model per precision / config, dropped before the next"""
    import torch
    import bench
    from eraxvif5tts_amd.model import MMDiT, UNetT

    def knob(key, value):
        import ctypes as C
        old = C.c_int(0)
        assert lib.f5_tuning_get(key.encode(), C.byref(old)) == 0 and lib.f5_tuning_set(key.encode(), value) == 0, key
        return old.value

    model, cfm = _dit("bf16")
    yield "bf16 1x256 (512 rows: smallest launch of the tuned kernels)", _sample(cfm, 1, 256)
    yield "bf16 2x900 (3600 rows: padded-rows window)", _sample(cfm, 2, 900)
    yield "bf16 3x1024 (6144 rows: split-v window at 256 CUs)", _sample(cfm, 3, 1024)
    g = torch.Generator().manual_seed(61)
    cond = (torch.randn(1, 100, 100, generator=g) * 2 - 3).clamp(-11.5, 3.0).cuda()
    texts = [torch.randint(0, bench.VOCAB, (1, d // 7), generator=g).cuda() for d in RAGGED]
    y0s = [torch.randn(1, d, 100, generator=g).cuda() for d in RAGGED]
    outs = cfm.sample_ragged(cond, texts, RAGGED, y0s=y0s, use_graph=False, steps=2, cfg_strength=2.0, sway_sampling_coef=-1.0)
    yield f"bf16 ragged {RAGGED} (2592 rows)", torch.cat([o.reshape(-1, 100) for o in outs])
    yield "bf16 forward 2x512, per-sample times", _forward(model, 2, 512, seed=5)
    model.set_active_blocks((0, 2))
    yield "bf16 2x900, block subset (0, 2)", _sample(cfm, 2, 900)
    model.set_active_blocks(None)
    plan = model.plan(1, 256, 2)
    tap = torch.zeros(2 * 256, ARCH["dim"], device="cuda")
    model.set_tap(plan, "blk1.n1", tap)
    out = _sample(cfm, 1, 256)
    model.set_tap(plan, None, None)
    yield "bf16 1x256, stage tap blk1.n1 (output | tap)", torch.cat([out.reshape(-1), tap.reshape(-1)])
    model.set_attn_dropout(0.1, seed=20240)
    yield "bf16 1x256, attention dropout p = 0.1, seed 20240", _sample(cfm, 1, 256)
    model.set_attn_dropout(None)
    for key in KNOBS:
        value = 1 if key == "ln_fold_inkernel" else 0
        for B, N in ((1, 256), (2, 900), (3, 1024)):
            old = knob(key, value)
            try:
                out = _sample(cfm, B, N)
            finally:
                knob(key, old)
            yield f"bf16 {B}x{N}, {key}={value}", out
    assert model.residual_fallbacks() == 0
    del cfm, model
    model, cfm = _dit("fp16")
    yield "fp16 2x900", _sample(cfm, 2, 900)
    assert model.residual_fallbacks() == 0
    del cfm, model
    model, cfm = _dit("fp32")
    yield "fp32 1x200", _sample(cfm, 1, 200)
    del cfm, model
    for tag, kw in (("long_skip_connection=True", dict(long_skip_connection=True)), ("qk_norm=rms_norm", dict(qk_norm="rms_norm"))):
        model, cfm = _dit("bf16", **kw)
        yield f"bf16 2x900, {tag}", _sample(cfm, 2, 900)
        yield f"bf16 3x1024, {tag}", _sample(cfm, 3, 1024)
        del cfm, model
    small = dict(dim=512, depth=4, heads=8, ff_mult=2)
    for cls in (MMDiT, UNetT):
        torch.manual_seed(77)
        model = bench.synth_weights(cls(**small, text_num_embeds=bench.VOCAB, mel_dim=100, precision="bf16"), seed=0).cuda()
        yield f"{cls.__name__} bf16 forward 2x512 (dim 512, depth 4)", _forward(model, 2, 512, seed=9, text_len=80)
        del model
    torch.cuda.empty_cache()


def trace(B, N):
    """what a kernel trace of one library should see: one eager B x N sample() of the bf16 model (behind its weight upload), nothing else"""
    import torch
    _load_lib()
    model, cfm = _dit("bf16")
    _sample(cfm, B, N)
    torch.cuda.synchronize()
    assert model.residual_fallbacks() == 0


def child(out_dir):
    import torch
    lib = _load_lib()
    os.makedirs(out_dir, exist_ok=True)
    names = []
    for i, (name, out) in enumerate(cases(lib)):
        torch.cuda.synchronize()
        host = out.detach().float().cpu().contiguous()
        assert torch.isfinite(host).all(), name
        with open(os.path.join(out_dir, f"{i:03d}.bin"), "wb") as f:
            f.write(host.numpy().tobytes())
        names.append((f"{i:03d}", name))
    with open(os.path.join(out_dir, "cases.json"), "w") as f:
        json.dump(names, f)
    print(f"{len(names)} cases -> {out_dir}")


def time_eager():
    """median wall time (ms) of an eager 1 x 256 sample() at NFE 32 on F5TTS_Base: the call where host launch code is the largest share"""
    import torch
    import bench
    from eraxvif5tts_amd.model import CFM, DiT
    _load_lib()
    torch.manual_seed(1234)
    model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision="bf16"), seed=0)
    cfm = CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()
    kw = dict(_problem(1, 256, seed=3), steps=32)
    for _ in range(5):
        cfm.sample(**kw)
    torch.cuda.synchronize()
    ms = []
    for _ in range(30):
        t0 = time.perf_counter()
        cfm.sample(**kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    print(json.dumps({"eager_1x256_nfe32_ms_median": round(ms[len(ms) // 2], 3), "min": round(ms[0], 3)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib")
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "dit_eval_ab"), help="where the children write their outputs (git-ignored)")
    ap.add_argument("--report")
    ap.add_argument("--child", metavar="DIR")
    ap.add_argument("--trace", nargs=2, type=int, metavar=("B", "N"))
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if a.time:
        return time_eager()
    if a.trace:
        return trace(*a.trace)
    if a.child:
        return child(a.child)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's build of the library (python -m eraxvif5tts_amd.build in a checkout of it)")
    dirs = {}
    for side, lib in (("parent", os.path.abspath(a.parent_lib)), ("new", None)):
        env = dict(os.environ)
        env.pop("F5HIP_LIB", None)
        if lib:
            env["F5HIP_LIB"] = lib
        dirs[side] = os.path.join(a.work, side)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dirs[side]], env=env, timeout=CHILD_TIMEOUT_S).returncode
        if rc != 0:  # nothing more is started on the GPU after a child that failed
            sys.exit(f"{side} child exited {rc}")
    names = {s: json.load(open(os.path.join(d, "cases.json"))) for s, d in dirs.items()}
    assert names["parent"] == names["new"], "the two children ran different case lists"
    lines, same = [], True
    for key, name in names["new"]:
        blob = {s: open(os.path.join(d, key + ".bin"), "rb").read() for s, d in dirs.items()}
        eq = blob["parent"] == blob["new"]
        same &= eq
        sha = {s: hashlib.sha256(b).hexdigest()[:16] for s, b in blob.items()}
        lines.append(f"  {'identical' if eq else 'DIFFERENT'}  parent {sha['parent']}  new {sha['new']}  {len(blob['new']):>9d} B  {name}")
    lines.append(f"verdict: {'every case byte-identical' if same else 'OUTPUTS DIFFER'} ({len(lines)} cases)")
    text = "\n".join(lines)
    print(text)
    if a.report:
        with open(a.report, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
