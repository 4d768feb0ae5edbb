"""f5_debug_eval_modes (csrc/dit_eval.hip: dit_eval_modes): the launch forms of a DiT evaluation, read back from the function the evaluation itself
decides with.  Two kinds of checks: the fields against values worked out from the conditions as the parent commit wrote them inline (not from the
getter's code), and the fields against what an evaluation then really launches, counted by the in-situ timing sites.

Model: dim 1024, 16 heads, ff_mult 2, depth 3 (a fold needs block 1 for a folded QKV projection and block 2 for the producer chain), 2 Euler
steps, CFG 2: one evaluation runs nb = 2 B batch rows.  The getter reads the plan's present state -- the fold table and the evaluation index the
last call left -- so every reading follows an eager sample() in the state it asks about.

The split of the QKV projection (q|k and v apart) cannot be seen from outside at its launch: one timed() wraps both launches of a split, and
f5_debug_last_gemm holds the LAST launch of the process, which after any evaluation -- a one-block model's included -- is proj_out.  What is checked
here is the getter's split_v field (the tile arithmetic) against the parent's formula at three shapes; that the launches of the 2 x 900 and 3 x 1024
evaluations are the parent's, kernel by kernel, is recorded in profiles/dit_eval_sites_ab.txt."""
import ctypes as C

import pytest
import torch

import gpu_helpers as G

pytestmark = pytest.mark.gpu

ARCH = dict(dim=1024, depth=3, heads=16, ff_mult=2, text_dim=512, text_mask_padding=False, conv_layers=4, pe_attn_head=1)
DEPTH, STEPS = ARCH["depth"], 2
SITE_QKV, SITE_FF1, SITE_LN1, SITE_LN2 = 0, 3, 5, 6  # include/f5hip.h: F5_SITE_*


def _make(prec, **kw):
    import bench
    from eraxvif5tts_amd.model import CFM, DiT
    torch.manual_seed(1234)
    model = bench.synth_weights(DiT(**ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision=prec, **kw), seed=0)
    return model, CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()


def _sample(cfm, B, N):
    import bench
    cond, text, lens, dur = bench.synth_batch(B, N, "cuda", seed=B * 10000 + N)
    y0 = torch.randn(B, N, 100, generator=torch.Generator().manual_seed(B + N))
    out = cfm.sample(cond=cond, text=text, duration=dur, lens=lens, steps=STEPS, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0,
                     return_trajectory=False, use_graph=False)[0]
    assert torch.isfinite(out).all()


def _modes(model, cfm, B, N, **kw):
    """the modes of the evaluations of an eager B x N sample(), read after it"""
    _sample(cfm, B, N)
    return G.eval_modes(model.plan(B, N, STEPS), 2 * B, N, **kw)


@pytest.fixture(scope="module")
def bf16():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus & ~7 == 256, f"the shapes are worked out for a 256-CU device, this one has {cus} CUs"
    made = _make("bf16")
    yield made
    del made
    torch.cuda.empty_cache()


def test_fields_in_the_bf16_production_mode(bf16):
    """Default knobs.  rows_g: 3 600 rows are past the padding threshold (3 584) and no multiple of 256 -> 3 840; 6 144 is a multiple, 512 is below
    it.  The fold runs (in-place fp16 stream, a staged table, the tuned kernels from 512 rows on) with pre-scaled q.  split_v, with t = ceil(rows /
    256) token tiles and 8 / 12 feature tiles of q|k / q|k|v: 160 <= 8 t <= 256 < 12 t holds for t = 24 (6 144 rows), not for t = 15 or 2."""
    model, cfm = bf16
    for (B, N), rows_g, split in (((1, 256), 512, 0), ((2, 900), 3840, 0), ((3, 1024), 6144, 1)):
        md = _modes(model, cfm, B, N)
        assert md["rows"] == 2 * B * N and md["rows_g"] == rows_g, md
        assert (md["defer"], md["r16"], md["rmw"], md["lnf"], md["qs"], md["wpf"]) == (1, 1, 1, 1, 1, 1), md
        assert md["split_v"] == split, md
        assert md["frow0"] == (STEPS - 1) * DEPTH * (3 * 1024 + 2048), md  # the last evaluation's rows of the table: [evals][depth][3 inner + ff]
    assert model.residual_fallbacks() == 0


def test_fields_under_every_switch_that_turns_a_mode_off(bf16):
    model, cfm = bf16
    with G.knobs(gemm_pad_rows=0):
        md = _modes(model, cfm, 2, 900)
        assert md["rows_g"] == md["rows"] == 3600 and md["lnf"] == 1, md
    with G.knobs(ln_fold=0):
        md = _modes(model, cfm, 2, 900)
        assert (md["lnf"], md["qs"], md["rmw"], md["rows_g"]) == (0, 0, 1, 3840), md
    for value in (0, 1):  # rmw follows the knob; without the in-place stream nothing pads and nothing folds
        with G.knobs(resid_rmw=value):
            md = _modes(model, cfm, 2, 900)
            assert md["rmw"] == value and md["lnf"] == value and md["rows_g"] == (3840 if value else 3600) and md["r16"] == 1, md
    with G.knobs(ln_defer=0):  # fp32 stream, written after every pass
        md = _modes(model, cfm, 2, 900)
        assert (md["defer"], md["r16"], md["rmw"], md["lnf"], md["wpf"]) == (0, 0, 0, 0, 0), md
    with G.knobs(residual_f16=0):
        md = _modes(model, cfm, 2, 900)
        assert (md["defer"], md["r16"], md["rmw"], md["lnf"]) == (1, 0, 0, 0), md
    with G.knobs(w_prefetch=0):
        assert _modes(model, cfm, 2, 900)["wpf"] == 0
    # per-sample times (f5_dit_forward): one AdaLN row per batch row -> no in-place stream, no fold; the stream stays fp16
    md = _modes(model, cfm, 2, 900, per_batch_rows=True)
    assert (md["r16"], md["rmw"], md["lnf"], md["rows_g"]) == (1, 0, 0, 3600), md
    model.set_active_blocks((0, 2))
    try:
        md = _modes(model, cfm, 2, 900)
        assert (md["rmw"], md["lnf"], md["qs"], md["rows_g"]) == (1, 0, 0, 3840), md
    finally:
        model.set_active_blocks(None)
    plan = model.plan(2, 900, STEPS)
    tap = torch.zeros(2 * 2 * 900, ARCH["dim"], device="cuda")
    model.set_tap(plan, "blk1.n1", tap)
    try:
        md = _modes(model, cfm, 2, 900)
        assert (md["defer"], md["r16"], md["rmw"], md["lnf"], md["qs"]) == (0, 0, 0, 0, 0), md
    finally:
        model.set_tap(plan, None, None)
    model.set_attn_dropout(0.1, seed=7)
    try:
        md = _modes(model, cfm, 2, 900)
        assert (md["lnf"], md["qs"]) == (1, 0), md  # the dropout kernels take q as projected: the fold stays, its table unscaled
    finally:
        model.set_attn_dropout(None)
    md = _modes(model, cfm, 2, 900)
    assert (md["lnf"], md["qs"], md["rows_g"]) == (1, 1, 3840), md  # and everything is back
    assert model.residual_fallbacks() == 0


def test_fields_in_the_other_precision_modes():
    for prec, want in (("fp16", dict(r16=1, rmw=1, lnf=1, qs=0, rows_g=3840)), ("fp32", dict(r16=0, rmw=0, lnf=0, qs=0, rows_g=3600, wpf=0))):
        model, cfm = _make(prec)
        md = _modes(model, cfm, 2, 900)
        assert {k: md[k] for k in want} == want, (prec, md)
        assert model.residual_fallbacks() == 0
        del cfm, model
        torch.cuda.empty_cache()


def _site_launches(model, cfm, B, N):
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    plan = model.plan(B, N, STEPS)
    _lib.check(lib.f5_plan_timing_begin(plan, (7 * DEPTH + 4) * STEPS))
    _sample(cfm, B, N)
    ms, cnt = C.c_float(0.0), C.c_int(0)
    _lib.check(lib.f5_plan_timing_end(plan, C.byref(ms), C.byref(cnt), _lib.stream_ptr()))
    n = {}
    for site, idx in (("qkv", SITE_QKV), ("ff1", SITE_FF1), ("ln1", SITE_LN1), ("ln2", SITE_LN2)):
        a, k = C.c_float(0.0), C.c_int(0)
        _lib.check(lib.f5_plan_timing_site(plan, idx, C.byref(a), C.byref(k)))
        n[site] = k.value
    return n, G.eval_modes(plan, 2 * B, N)


@pytest.mark.parametrize("B,N,kv", [(1, 256, {}), (2, 900, {}), (3, 1024, {}), (1, 256, {"ln_fold": 0}), (1, 256, {"ln_fold_inkernel": 1}),
                                    (2, 900, {"gemm_w4_ink": 0}), (1, 256, {"resid_rmw": 0})])
def test_modes_predict_the_launches_at_the_layernorm_sites(bf16, B, N, kv):
    """One eager sample() with the in-situ timing on.  Launches under F5_SITE_LN1 per evaluation: a LayerNorm pass for every block whose first
    LayerNorm is not folded (all of them without the fold, block 0 with it), and one statistics launch for every folded one (lnf1: blocks 1 ..)
    unless its QKV projection finishes the statistics in its own kernel; under F5_SITE_LN2 the same with lnf and FF1 for every block.  One
    timed() wraps both launches of a split QKV projection, so F5_SITE_QKV and F5_SITE_FF1 count one per block either way."""
    model, cfm = bf16
    with G.knobs(**kv):
        n, md = _site_launches(model, cfm, B, N)
    lnf1 = [bool(md["lnf"]) and l > 0 for l in range(DEPTH)]
    ln1 = sum((0 if md["ink_qkv"] else 1) if f else 1 for f in lnf1)
    ln2 = DEPTH * ((0 if md["ink_ff1"] else 1) if md["lnf"] else 1)
    print(f"{B} x {N} {kv}: {md}; launches per site {n}")
    assert md["lnf"] == (0 if kv.get("ln_fold") == 0 or kv.get("resid_rmw") == 0 else 1), md
    assert n["qkv"] == n["ff1"] == STEPS * DEPTH, n
    assert n["ln1"] == STEPS * ln1 and n["ln2"] == STEPS * ln2, (n, md)
    assert model.residual_fallbacks() == 0
