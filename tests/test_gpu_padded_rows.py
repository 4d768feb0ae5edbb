"""The block GEMMs' padding rows (csrc/dit_eval.hip, rows_g): with the in-place fp16 residual stream on and a token count of at least 3584 that is
not a multiple of 256, the four block GEMMs of an evaluation run over the rows rounded up to 256.  The padding rows of the fp16 stream are never
reset -- every out-projection and FF2 epilogue keeps adding gate * (A W + b) to them, call after call -- and a folded consumer that finishes
the row statistics inside the kernel (by default: FF1 on the one-wave-per-SIMD kernel's 128-row tiles) computes them for those rows too.  None of
that may reach a real row or the fp16 range guard: outputs must equal the unpadded launches bit for bit, on every call of a plan's life, with no
fallback to fp32 storage.

F5TTS_Base width and depth, synthetic weights and batches as the neighbouring full-size tests; CFG 2 throughout (token rows = 2 B N)."""
import ctypes as C

import pytest
import torch

from conftest import rel_l2
from gpu_helpers import knobs

pytestmark = pytest.mark.gpu

DEPTH = 22

# (B, N) -> (in-kernel statistics on the QKV launch, on the FF1 launch), as measured on the MI355X (256-CU persistent grid) and pinned here through
# the timing sites.  A folded consumer finishes the statistics itself on the one-wave-per-SIMD kernel's 128-row tiles only where the 8-wave kernel
# would not take the 256-wide tile (gemm_fast_tile: FF1 up to 16 token tiles of 256 rows, QKV up to 13): inside the padding window (rows >= 3584)
# that is FF1 at 3840 and 4096 padded rows -- QKV never.
CASES = {
    (1, 1790): (False, False),  # 3580 rows: below the padding threshold (control)
    (2, 896): (False, True),  # 3584 rows: a multiple of 256, no padding, same kernels (control)
    (2, 900): (False, True),  # 3600 -> 3840 rows: FF1 finishes the padding rows' statistics
    (1, 2000): (False, True),  # 4000 -> 4096: FF1
    (2, 1020): (False, True),  # 4080 -> 4096: FF1, 16 padding rows (upper edge of the window)
    (3, 700): (False, False),  # 4200 -> 4352: padding, statistics launches in front of both consumers (control)
    (2, 1470): (False, False),  # 5880 -> 5888: the same (control)
    (2, 1500): (False, False),  # 6000 -> 6144: the same (control)
}
# two chunks as one ragged batch: per CFG half round_up(round_up(900 + 16, 16) + 1000 + 16, 16) = 1952 rows (csrc/sampler.hip, RAGGED_GAP), so
# 3904 token rows -> 4096
RAGGED = [900, 1000]


def _ragged_rows(frames, gap=16):
    t = 0
    for f in frames:
        t = -(-(t + f + gap) // 16) * 16
    return 2 * t


def _rows_g(rows):
    return -(-rows // 256) * 256 if rows >= 3584 and rows % 256 else rows


def _make(prec, scale=None, seed=1234):
    """F5TTS_Base on the GPU; `scale` multiplies the biases of every block's attention out-projection and second FF linear (the constant part of
    what the in-place residual epilogues add to the fp16 stream)"""
    import bench
    from eraxvif5tts_amd.model import CFM, DiT
    torch.manual_seed(seed)  # DiT's default init draws from the global RNG: same weights for both precisions
    model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision=prec), seed=0)
    if scale is not None:
        with torch.no_grad():
            for name, p in model.named_parameters():
                if name.startswith("transformer_blocks.") and name.endswith(("attn.to_out.0.bias", "ff.ff.2.bias")):
                    p.mul_(scale)
    return model, CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()


def _problem(B, N, seed):
    import bench
    cond, text, lens, dur = bench.synth_batch(B, N, "cuda", seed=seed)
    y0 = torch.randn(B, N, 100, generator=torch.Generator().manual_seed(seed + 1))
    return dict(cond=cond, text=text, duration=dur, lens=lens, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, return_trajectory=False)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus & ~7 == 256, f"CASES are worked out for a 256-CU persistent grid, this device has {cus} CUs"


@pytest.fixture(scope="module")
def models():
    made = {prec: _make(prec) for prec in ("bf16", "fp32")}
    yield made
    made.clear()
    torch.cuda.empty_cache()


def _site_launches(model, cfm, B, N, kw):
    """one eager sample() with the in-situ timing on: launches counted under the LayerNorm sites (LN1: block 0's pass plus a statistics launch in
    front of every folded QKV projection that does not finish them itself; LN2: a statistics launch in front of every FF1 that does not)"""
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    plan = model.plan(B, N, kw["steps"])
    _lib.check(lib.f5_plan_timing_begin(plan, (7 * DEPTH + 4) * kw["steps"]))
    out = cfm.sample(use_graph=False, **kw)[0]
    ms, cnt = C.c_float(0.0), C.c_int(0)
    _lib.check(lib.f5_plan_timing_end(plan, C.byref(ms), C.byref(cnt), _lib.stream_ptr()))
    n = {}
    for site, idx in (("qkv", 0), ("ff1", 3), ("ln1", 5), ("ln2", 6)):
        a, k = C.c_float(0.0), C.c_int(0)
        _lib.check(lib.f5_plan_timing_site(plan, idx, C.byref(a), C.byref(k)))
        n[site] = k.value
    return out.cpu(), n


@pytest.mark.parametrize("B,N", list(CASES))
def test_padded_launches_equal_every_equivalent_path(models, B, N):
    """3 Euler steps: the default path against no padding (gemm_pad_rows = 0), statistics launches (gemm_w4_ink = 0), the 8-wave kernel
    (gemm_w4 = 0) and graph replay -- all bit-identical -- and against fp32 mode (rel-L2 <= 2e-2); no fp16 range-guard fallback anywhere.  The
    timing sites pin each case to the statistics path CASES claims, so that a tuning change cannot move it out of the window unnoticed."""
    model, cfm = models["bf16"]
    kw = dict(_problem(B, N, seed=B * 10000 + N), steps=3)
    rows = 2 * B * N
    ink_qkv, ink_ff1 = CASES[(B, N)]
    assert (_rows_g(rows) != rows) == (rows in (3600, 4000, 4080, 4200, 5880, 6000))
    ref = cfm.sample(use_graph=False, **kw)[0].cpu()
    assert torch.isfinite(ref).all()
    for _ in range(2):  # capture, replay
        assert torch.equal(cfm.sample(use_graph=True, **kw)[0].cpu(), ref)
    timed, n = _site_launches(model, cfm, B, N, kw)
    assert torch.equal(timed, ref)
    evals = kw["steps"]
    assert n["qkv"] == n["ff1"] == evals * DEPTH, n
    assert n["ln1"] == evals * (1 if ink_qkv else DEPTH), (n, "QKV in-kernel statistics" if ink_qkv else "QKV statistics launches")
    assert n["ln2"] == evals * (0 if ink_ff1 else DEPTH), (n, "FF1 in-kernel statistics" if ink_ff1 else "FF1 statistics launches")
    for tag, kv in (("unpadded", {"gemm_pad_rows": 0}), ("launches", {"gemm_w4_ink": 0}), ("8wave", {"gemm_w4": 0})):
        with knobs(**kv):
            out = cfm.sample(use_graph=False, **kw)[0].cpu()
            if tag == "launches":  # (the control leg really takes the other path)
                _, nl = _site_launches(model, cfm, B, N, kw)
                assert nl["ln1"] == nl["ln2"] == evals * DEPTH, nl
        assert torch.equal(out, ref), (tag, float((out - ref).abs().max()))
    assert model.residual_fallbacks() == 0
    want = models["fp32"][1].sample(**kw)[0].cpu()
    n_ref = kw["cond"].shape[1]
    err = rel_l2(ref[:, n_ref:], want[:, n_ref:])
    print(f"{B} x {N} ({rows} -> {_rows_g(rows)} rows): bf16 vs fp32 mode rel-L2 {err:.3e}; launches at LN1 / LN2 {n['ln1']} / {n['ln2']}")
    assert err < 2e-2


@pytest.mark.parametrize("knob,value", [("gemm_reverse_sites", 0), ("gemm_reverse_sites", 15), ("gemm_group", 1), ("gemm_group", 3), ("gemm_persist_grid", 8),
                                        ("gemm_persist_grid", 24)])
def test_tile_walk_knobs_change_no_bit(models, knob, value):
    """2 x 900 (3600 -> 3840 rows), 3 Euler steps: the order in which a block GEMM walks its tiles -- backwards at no call site or at all four
    (gemm_reverse_sites; op launches carry no call site, so the reversed walk runs here only), L2 patches of 1 and 3 token tiles (gemm_group),
    persistent grids of 8 and 24 workgroups (gemm_persist_grid, which also moves the tile rule) -- gives the default path's bits: "same values
    either way" is what the knobs' comments promise."""
    model, cfm = models["bf16"]
    kw = dict(_problem(2, 900, seed=20900), steps=3)
    ref = cfm.sample(use_graph=False, **kw)[0].cpu()
    assert torch.isfinite(ref).all()
    with knobs(**{knob: value}):
        out = cfm.sample(use_graph=False, **kw)[0].cpu()
    assert torch.equal(out, ref), (knob, value, float((out - ref).abs().max()))
    assert model.residual_fallbacks() == 0


def test_padded_launches_with_the_other_statistics_forms(models):
    """2 x 900 (3600 -> 3840 rows) with the statistics form that is off by default, the 8-wave kernel's in-kernel statistics
    (ln_fold_inkernel = 1), beside the one-wave-per-SIMD kernel and without it -- same bits as the default path, no fallback."""
    model, cfm = models["bf16"]
    kw = dict(_problem(2, 900, seed=29), steps=3)
    ref = cfm.sample(use_graph=False, **kw)[0].cpu()
    for kv in ({"ln_fold_inkernel": 1}, {"ln_fold_inkernel": 1, "gemm_w4": 0}):
        with knobs(**kv):
            out = cfm.sample(use_graph=False, **kw)[0].cpu()
            assert torch.equal(out, ref), kv
            for _ in range(2):
                assert torch.equal(cfm.sample(use_graph=True, **kw)[0].cpu(), ref), (kv, "graph")
    assert model.residual_fallbacks() == 0


def test_padded_ragged_batch_equals_every_equivalent_path(models):
    """Two chunks as one ragged batch (f5_sample_ragged) whose token rows (3904) pad to 4096: default, unpadded, statistics launches, 8-wave
    kernel and graph replay bit-identical; every utterance within 2e-2 of its own fp32-mode sample()."""
    import bench
    model, cfm = models["bf16"]
    rows = _ragged_rows(RAGGED)
    assert rows == 3904 and _rows_g(rows) == 4096
    g = torch.Generator().manual_seed(61)
    cond = (torch.randn(1, 300, 100, generator=g) * 2 - 3).clamp(-11.5, 3.0).cuda()
    texts = [torch.randint(0, bench.VOCAB, (1, d // 7), generator=g).cuda() for d in RAGGED]
    y0s = [torch.randn(1, d, 100, generator=g).cuda() for d in RAGGED]
    kw = dict(steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0)
    ref = [o.cpu() for o in cfm.sample_ragged(cond, texts, RAGGED, y0s=y0s, use_graph=False, **kw)]
    for _ in range(2):
        for a, b in zip(cfm.sample_ragged(cond, texts, RAGGED, y0s=y0s, use_graph=True, **kw), ref):
            assert torch.equal(a.cpu(), b), "graph"
    for kv in ({"gemm_pad_rows": 0}, {"gemm_w4_ink": 0}, {"gemm_w4": 0}):
        with knobs(**kv):
            for a, b in zip(cfm.sample_ragged(cond, texts, RAGGED, y0s=y0s, use_graph=False, **kw), ref):
                assert torch.equal(a.cpu(), b), kv
    assert model.residual_fallbacks() == 0
    cfm32 = models["fp32"][1]
    for t, d, y, got in zip(texts, RAGGED, y0s, ref):
        want = cfm32.sample(cond=cond, text=t, duration=d, y0=y, return_trajectory=False, **kw)[0].cpu()
        err = rel_l2(got[:, 300:], want[:, 300:])
        print(f"ragged chunk of {d} frames: bf16 vs fp32 mode rel-L2 {err:.3e}")
        assert torch.isfinite(got).all() and err < 2e-2


@pytest.mark.parametrize("method,edit", [("euler", False), ("rk4", False), ("euler", True)])
def test_plan_lifetime_at_a_padded_shape(method, edit):
    """One plan serving 2 x 900 (3600 -> 3840 rows) for 40 NFE-32 calls with graph replay, after a 2 x 1024 call left its activations in the
    padding rows: every output equals a fresh plan's first 2 x 900 output bit for bit and the fp16 range guard never fires -- the padding rows
    drift for the whole life of the plan, but they are no token's and must not send the plan to fp32 storage.  Euler, rk4 (four evaluations
    per step: four times the drift per call) and a speech-edit mask."""
    from eraxvif5tts_amd.model import CFM
    model, _ = _make("bf16")
    cfm = CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}, odeint_kwargs={"method": method}).cuda()
    kw = dict(_problem(2, 900, seed=71), steps=32)
    if edit:  # (over the prompt frames, as cfm.py builds lens_to_mask(lens) & edit_mask)
        m = torch.ones(2, kw["cond"].shape[1], dtype=torch.bool)
        m[0, 40:120] = False
        m[1, 150:260] = False
        kw["edit_mask"] = m.cuda()
    first = cfm.sample(use_graph=True, **kw)[0].cpu()  # a fresh plan sized for 2 x 900
    assert torch.isfinite(first).all() and model.residual_fallbacks() == 0
    model.refresh_native()  # new plans: the next one is sized for 2 x 1024, and 2 x 900 reuses it
    big = _problem(2, 1024, seed=73)
    if edit:
        big["edit_mask"] = torch.ones(2, big["cond"].shape[1], dtype=torch.bool, device="cuda")
    cfm.sample(use_graph=False, steps=32, **big)
    for i in range(40):
        out = cfm.sample(use_graph=True, **kw)[0].cpu()
        assert model.residual_fallbacks() == 0, f"fp16 range guard fired on call {i + 1} after the 2 x 1024 call"
        assert torch.equal(out, first), i
    del cfm, model
    torch.cuda.empty_cache()


# bias scale of the witness below, calibrated on the MI355X against the build before GemmParams::lnf_rows (whose FF1 launches carried the padding
# rows into the range guard): powers of two up to 4096 never fell back within four NFE-32 calls, 8192 fell back on the third call, 16384 on the
# second (the smallest within two), 32768 on the first -- every time at row 3600, the first padding row.  Doubled: 32768.  The unpadded control
# stays clean at that scale (rel-L2 7e-4 against fp32 mode).
WITNESS_SCALE = 32768.0


def test_padding_rows_never_trip_the_fp16_range_guard():
    """A deterministic witness: out-projection and FF2 biases scaled by WITNESS_SCALE, so that the constant gate * b term dominates what the
    in-place epilogues add.  A real row receives 2 x 22 such adds per evaluation and starts afresh every evaluation; a padding row receives them
    on every evaluation of every call.  Control (gemm_pad_rows = 0): no fallback and within 2e-2 of fp32 mode on the same weights -- the real
    rows are well inside fp16's range.  With the padding: the same bits on every call and still no fallback."""
    kw = dict(_problem(2, 900, seed=81), steps=32)
    n_ref = kw["cond"].shape[1]
    model32, cfm32 = _make("fp32", scale=WITNESS_SCALE)
    want = cfm32.sample(**kw)[0].cpu()
    del cfm32, model32
    model, cfm = _make("bf16", scale=WITNESS_SCALE)
    with knobs(gemm_pad_rows=0):
        ctrl = cfm.sample(use_graph=False, **kw)[0].cpu()
    assert model.residual_fallbacks() == 0
    err = rel_l2(ctrl[:, n_ref:], want[:, n_ref:])
    print(f"bias scale {WITNESS_SCALE:g}: unpadded bf16 vs fp32 mode rel-L2 {err:.3e}")
    assert torch.isfinite(ctrl).all() and err < 2e-2
    model.refresh_native()  # a fresh plan whose padding rows start from zero
    for i in range(3):
        out = cfm.sample(use_graph=i > 0, **kw)[0].cpu()
        assert model.residual_fallbacks() == 0, f"fp16 range guard fired on padded call {i + 1}"
        assert torch.equal(out, ctrl), i
    del cfm, model
    torch.cuda.empty_cache()
