"""Attention dropout at model level (DiT.set_attn_dropout) on the tiny golden architectures.  The oracle is
oracle/cpu_ref.py unchanged: for the duration of an oracle call torch.softmax is replaced by one that multiplies every 4-D result -- an
attention's probabilities [b, h, q, k] -- by keep / (1 - p) from the host mask of tests/dropout_ref.py, a call counter supplying the
evaluation, branch and block (cpu_ref.sample runs the conditional forward, then the null forward, per evaluation; cpu_ref's forwards run their
blocks in order).  The masks move these outputs by 1e-3 and more, the fp32 bounds are 1e-4 / 2e-4 and the matches come out near 1e-7: the
comparisons pin the numbering (call word = base + e * depth + l, batch word = branch * B + b) exactly, not statistically."""
import ast
import contextlib
import ctypes as C

import pytest
import torch

import dropout_ref as R
from conftest import golden_arch, golden_weights, load_golden, rel_l2
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
TOL = {"fp32": 2e-4, "bf16": 2e-2}        # tests/test_gpu_model.py
STAGE_TOL = {"fp32": 1e-4, "bf16": 1.5e-2}
P, SEED = 0.1, 0x5EED0123456789AB


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@contextlib.contextmanager
def oracle_dropout(depth, seed, *, base=0, branches=1, bw0=lambda branch: 0, p=P):
    """torch.softmax with the library's mask on 4-D results.  Call c (counted over the 4-D calls): block l = c % depth, branch = (c // depth) %
    branches, evaluation e = c // (depth * branches); call word base + e * depth + l; batch item b is drawn with batch word bw0(branch) + b."""
    real, count = torch.softmax, [0]

    def softmax(x, *a, **kw):
        r = real(x, *a, **kw)
        if r.ndim != 4:
            return r
        c = count[0]
        count[0] += 1
        l, branch, e = c % depth, (c // depth) % branches, c // (depth * branches)
        B, H, nq, nk = r.shape
        assert nq == nk
        keep = R.keep_mask(seed, base + e * depth + l, bw0(branch), B, H, nk, p)
        return r * torch.from_numpy(keep).to(r.dtype) / (1.0 - p)

    torch.softmax = softmax
    try:
        yield count
    finally:
        torch.softmax = real


def _opt(model, key):
    from eraxvif5tts_amd import _lib
    vals = []
    for _, h in model._plans:
        v = C.c_int(-1)
        _lib.check(_lib.load().f5_plan_get_option(h, key.encode(), C.byref(v)))
        vals.append(v.value)
    return vals


def _gen_rows(t, dur):
    return torch.cat([t[b, : int(d)] for b, d in enumerate(dur)])


# ----------------------------------------------------------------------------- 1. one DiT forward, twice on one plan
def test_dit_forward_fp32_with_key_mask_and_the_second_forwards_call_words():
    import gpu_helpers as G
    z = load_golden("tiny_base")
    arch, W = golden_arch(z), golden_weights(z)
    m = G.make_dit(arch, int(z["vocab"]), W, "fp32")
    x, cond, text, t = [torch.from_numpy(z[k]) for k in ("trace_x", "trace_cond", "text", "trace_t")]
    mask = cpu_ref.lens_to_mask(torch.from_numpy(z["duration"]))
    B, depth = x.shape[0], arch["depth"]
    assert B == 2 and not mask.all()
    m.set_attn_dropout(P, SEED)
    for call in range(2):
        out = m(x=x.cuda(), cond=cond.cuda(), text=text.cuda(), time=t.cuda(), mask=mask.cuda(), drop_audio_cond=False, drop_text=False).cpu()
        with oracle_dropout(depth, SEED, base=call * depth) as n:
            ref = cpu_ref.dit_forward(W, arch, x, cond, text, t, False, False, mask=mask)
        assert n[0] == depth
        err = rel_l2(out[mask], ref[mask])
        print(f"  forward {call}: rel-L2 {err:.3e}")
        assert err < STAGE_TOL["fp32"]
        assert _opt(m, "attn_dropout_base") == [(call + 1) * depth] and _opt(m, "attn_dropout_on") == [1]
    plain = cpu_ref.dit_forward(W, arch, x, cond, text, t, False, False, mask=mask)
    assert rel_l2(out[mask], plain[mask]) > STAGE_TOL["fp32"]  # (the masks move the output by more than the bound they are pinned under)


# ----------------------------------------------------------------------------- 2. CFM.sample
@pytest.mark.parametrize("name", ["tiny_base", "tiny_v1"])
@pytest.mark.parametrize("method,steps,cfg", [("euler", 4, 2.0), ("midpoint", 2, 2.0), ("euler", 4, 0.0)], ids=["euler_cfg2", "midpoint_cfg2", "euler_cfg0"])
def test_sample_fp32_matches_the_oracle_on_the_same_masks(name, method, steps, cfg):
    import gpu_helpers as G
    z = load_golden(name)
    arch, W = golden_arch(z), golden_weights(z)
    c = G.make_cfm(arch, int(z["vocab"]), W, "fp32", method=method)
    cond, text, dur, lens, y0 = [torch.from_numpy(z[k]) for k in ("cond", "text", "duration", "lens", "y0")]
    B, depth = cond.shape[0], arch["depth"]
    assert B == 2 and int(dur[0]) != int(dur[1])
    c.transformer.set_attn_dropout(P, SEED)
    out, _ = c.sample(cond=cond.cuda(), text=text.cuda(), duration=dur.cuda(), lens=lens.cuda(), steps=steps, cfg_strength=cfg, sway_sampling_coef=-1.0,
                      y0=y0, use_graph=False, return_trajectory=False)
    nbr = 2 if cfg else 1
    with oracle_dropout(depth, SEED, branches=nbr, bw0=lambda branch: branch * B) as n:
        ref, _ = cpu_ref.sample(W, arch, cond, text, dur, lens=lens, steps=steps, cfg_strength=cfg, sway_sampling_coef=-1.0, y0=y0, method=method,
                                return_trajectory=False)
    evals = steps * (2 if method == "midpoint" else 1)
    assert n[0] == evals * nbr * depth
    err = rel_l2(_gen_rows(out.cpu(), dur), _gen_rows(ref, dur))
    print(f"  rel-L2 {err:.3e}")
    assert err < TOL["fp32"]
    assert _opt(c.transformer, "attn_dropout_base") == [evals * depth]


# ----------------------------------------------------------------------------- 3. the other backbones
def test_unett_forward_fp32_counts_the_time_token_as_position_zero():
    from eraxvif5tts_amd.model import UNetT
    z = load_golden("tiny_unett")
    arch = ast.literal_eval(str(z["a.arch"]))
    V = int(z["a.vocab"])
    W = cpu_ref.random_unett_weights(arch, V, seed=int(z["a.seed"]))
    m = UNetT(**arch, text_num_embeds=V, mel_dim=100, precision="fp32")
    m.load_state_dict({k: v for k, v in W.items() if k in m.state_dict()}, strict=False)
    m = m.cuda()
    x, cond, text, mask, t = [torch.from_numpy(z[f"a.{k}"]) for k in ("x", "cond", "text", "mask", "t")]
    m.set_attn_dropout(P, SEED)
    out = m(x=x.cuda(), cond=cond.cuda(), text=text.cuda(), time=t.cuda(), mask=mask.cuda(), drop_audio_cond=False, drop_text=False).cpu()
    with oracle_dropout(arch["depth"], SEED) as n:  # (the oracle's softmax runs over N + 1 tokens, time token first)
        ref = cpu_ref.unett_forward(W, arch, x, cond, text, t, False, False, mask=mask)
    assert n[0] == arch["depth"]
    err = rel_l2(out[mask], ref[mask])
    print(f"  rel-L2 {err:.3e}")
    assert err < STAGE_TOL["fp32"]


def test_mmdit_forward_fp32_uses_the_joint_sequence():
    from eraxvif5tts_amd.model import MMDiT
    z = load_golden("tiny_mmdit")
    arch = ast.literal_eval(str(z["a.arch"]))
    V = int(z["a.vocab"])
    W = cpu_ref.random_mmdit_weights(arch, V, seed=int(z["a.seed"]))
    m = MMDiT(**arch, text_num_embeds=V, mel_dim=100, precision="fp32")
    m.load_state_dict({**W, "rotary_embed.inv_freq": m.state_dict()["rotary_embed.inv_freq"]}, strict=True)
    m = m.cuda()
    x, cond, text, mask, t = [torch.from_numpy(z[f"a.{k}"]) for k in ("x", "cond", "text", "mask", "t")]
    m.set_attn_dropout(P, SEED)
    out = m(x=x.cuda(), cond=cond.cuda(), text=text.cuda(), time=t.cuda(), mask=mask.cuda(), drop_audio_cond=False, drop_text=False).cpu()
    with oracle_dropout(arch["depth"], SEED) as n:  # (softmax over [frames | text])
        ref = cpu_ref.mmdit_forward(W, arch, x, cond, text, t, False, False, mask=mask)
    assert n[0] == arch["depth"]
    err = rel_l2(out[mask], ref[mask])
    print(f"  rel-L2 {err:.3e}")
    assert err < STAGE_TOL["fp32"]


# ----------------------------------------------------------------------------- 4. ragged sampler
def _ragged_inputs(V):
    g = torch.Generator().manual_seed(77)
    nc, durs = 90, [300, 257]
    cond = torch.randn(1, nc, 100, generator=g) * 2 - 3
    texts = [torch.randint(0, V, (1, n), generator=g) for n in (31, 12)]
    y0s = [torch.randn(1, d, 100, generator=g) for d in durs]
    return nc, durs, cond, texts, y0s


def test_sample_ragged_fp32_draws_batch_word_branch_times_b_plus_u():
    import gpu_helpers as G
    z = load_golden("tiny_base")
    arch, V, W = golden_arch(z), int(z["vocab"]), golden_weights(z)
    cfm = G.make_cfm(arch, V, W, "fp32")
    nc, durs, cond, texts, y0s = _ragged_inputs(V)
    cfm.transformer.set_attn_dropout(P, SEED)
    got = cfm.sample_ragged(cond.cuda(), [t.cuda() for t in texts], durs, y0s=[y.cuda() for y in y0s], steps=2, cfg_strength=2.0, sway_sampling_coef=-1.0,
                            use_graph=False)
    for u, d in enumerate(durs):
        with oracle_dropout(arch["depth"], SEED, branches=2, bw0=lambda branch, u=u: branch * len(durs) + u):
            ref, _ = cpu_ref.sample(W, arch, cond, texts[u], d, steps=2, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0s[u], return_trajectory=False)
        err = rel_l2(got[u].cpu()[:, nc:], ref[:, nc:])
        print(f"  utterance {u}: rel-L2 {err:.3e}")
        assert err < TOL["fp32"]
    assert _opt(cfm.transformer, "attn_dropout_base") == [2 * arch["depth"]]


# ----------------------------------------------------------------------------- 5. bf16 against fp32, same masks
def test_sample_bf16_against_the_fp32_mode_with_the_same_seed():
    import gpu_helpers as G
    z = load_golden("tiny_base")
    arch, V, W = golden_arch(z), int(z["vocab"]), golden_weights(z)
    g = torch.Generator().manual_seed(5)
    dur = torch.tensor([300, 257])
    cond = torch.randn(2, 90, 100, generator=g) * 2 - 3
    text = torch.randint(0, V, (2, 31), generator=g)
    y0 = torch.randn(2, 300, 100, generator=g)
    y0[1, 257:] = 0
    outs = {}
    for prec in ("fp32", "bf16"):
        c = G.make_cfm(arch, V, W, prec)
        c.transformer.set_attn_dropout(P, SEED)
        outs[prec], _ = c.sample(cond=cond.cuda(), text=text.cuda(), duration=dur.cuda(), lens=torch.tensor([90, 90]).cuda(), steps=2, cfg_strength=2.0,
                                 sway_sampling_coef=-1.0, y0=y0, use_graph=False, return_trajectory=False)
        assert c.transformer.residual_fallbacks() == 0
    err = rel_l2(_gen_rows(outs["bf16"].cpu(), dur), _gen_rows(outs["fp32"].cpu(), dur))
    print(f"  rel-L2 {err:.3e}")
    assert err < TOL["bf16"]


# ----------------------------------------------------------------------------- 6. graph replay
def test_graph_replay_reads_the_current_base():
    """Model A: an eager call, the capture + first replay, a cached replay.  Model B, fresh, same seed: three eager calls.  The base word is
    read through its pointer and advanced by the loop's last node, so call i of A equals call i of B bit for bit; and call 2 is not call 1."""
    import gpu_helpers as G
    z = load_golden("tiny_base")
    arch, W = golden_arch(z), golden_weights(z)
    kw = dict(cond=torch.from_numpy(z["cond"]).cuda(), text=torch.from_numpy(z["text"]).cuda(), duration=torch.from_numpy(z["duration"]).cuda(),
              lens=torch.from_numpy(z["lens"]).cuda(), steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=torch.from_numpy(z["y0"]), return_trajectory=False)
    a, b = [G.make_cfm(arch, int(z["vocab"]), W, "bf16") for _ in range(2)]
    a.transformer.set_attn_dropout(P, SEED)
    b.transformer.set_attn_dropout(P, SEED)
    outs_a = [a.sample(**kw, use_graph=ug)[0].clone() for ug in (False, True, True)]
    outs_b = [b.sample(**kw, use_graph=False)[0].clone() for _ in range(3)]
    for i, (x, y) in enumerate(zip(outs_a, outs_b)):
        assert torch.equal(x, y), (i, float((x - y).abs().max()))
    assert not torch.equal(outs_a[0], outs_a[1]) and not torch.equal(outs_a[1], outs_a[2])
    assert _opt(a.transformer, "attn_dropout_base") == _opt(b.transformer, "attn_dropout_base") == [3 * 4 * arch["depth"]]


# ----------------------------------------------------------------------------- 7. off again
def test_turning_the_mode_off_restores_the_default_path(monkeypatch):
    """tuned kernels forced so that the LayerNorm fold and pre-scaled q run at this size (tests/test_gpu_attention_prescale_model.py): while the
    mode is on q is never pre-scaled; after set_attn_dropout(None) the model computes the bits of one that never had the mode on."""
    import gpu_helpers as G
    monkeypatch.setenv("F5HIP_GEMM_KERNEL", "1")
    monkeypatch.setenv("F5HIP_ATTN_KERNEL", "1")
    z = load_golden("tiny_base")
    arch, W = golden_arch(z), golden_weights(z)
    kw = dict(cond=torch.from_numpy(z["cond"]).cuda(), text=torch.from_numpy(z["text"]).cuda(), duration=torch.from_numpy(z["duration"]).cuda(),
              lens=torch.from_numpy(z["lens"]).cuda(), steps=int(z["steps"]), cfg_strength=2.0, sway_sampling_coef=-1.0, y0=torch.from_numpy(z["y0"]),
              return_trajectory=False)
    never = G.make_cfm(arch, int(z["vocab"]), W, "bf16")
    ref = never.sample(**kw, use_graph=False)[0].clone()
    c = G.make_cfm(arch, int(z["vocab"]), W, "bf16")
    first = c.sample(**kw, use_graph=True)[0].clone()  # (a captured graph of the default path exists when the mode goes on)
    assert torch.equal(first, ref)
    c.transformer.set_attn_dropout(P, SEED)
    assert _opt(c.transformer, "attn_prescale_active") == [0] and _opt(c.transformer, "attn_dropout_on") == [1]
    on = c.sample(**kw, use_graph=True)[0].clone()
    assert torch.isfinite(on).all() and not torch.equal(on, ref)
    c.transformer.set_attn_dropout(None)
    assert _opt(c.transformer, "attn_dropout_on") == [0] and _opt(c.transformer, "attn_dropout_base") == [0]
    assert _opt(c.transformer, "attn_prescale_active") == _opt(never.transformer, "attn_prescale_active")
    for ug in (True, False):
        assert torch.equal(c.sample(**kw, use_graph=ug)[0], ref)
    assert c.transformer.residual_fallbacks() == 0


# ----------------------------------------------------------------------------- 8. the range guard's fp32 rerun
def test_range_guard_rerun_repeats_the_calls_own_masks():
    """The checkpoint of test_fp16_residual_range_guard_falls_back_to_fp32_storage (input projection scaled until the fp16 stream overflows): the
    library repeats the loop with fp32 residual storage.  With dropout on the rerun must start from the call's own base word: the result equals,
    bit for bit, a model that stored fp32 from the start (same seed), and the base has advanced once, not twice."""
    import gpu_helpers as G
    arch = dict(dim=256, depth=2, heads=4, ff_mult=2, text_dim=128, conv_layers=2, pe_attn_head=1, text_mask_padding=False)
    V = 60
    W = cpu_ref.random_dit_weights(arch, V, seed=77)
    big = dict(W)
    for k in ("input_embed.proj.weight", "input_embed.proj.bias"):
        big[k] = W[k] * 3.0e5
    g = torch.Generator().manual_seed(78)
    B, N = 2, 96
    cond = (torch.randn(B, 30, 100, generator=g) * 2 - 3).cuda()
    text = torch.randint(0, V, (B, 20), generator=g).cuda()
    lens, dur = torch.tensor([30, 24]).cuda(), torch.tensor([96, 80]).cuda()
    y0 = torch.randn(B, N, 100, generator=g)
    y0[1, 80:] = 0
    kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, return_trajectory=False)
    cfm = G.make_cfm(arch, V, big, "bf16")
    cfm.transformer.set_attn_dropout(P, SEED)
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        out = cfm.sample(use_graph=False, **kw)[0].clone()
    assert cfm.transformer.residual_fallbacks() == 1
    assert _opt(cfm.transformer, "attn_dropout_base") == [3 * arch["depth"]]
    second = cfm.sample(use_graph=False, **kw)[0].clone()  # (fp32 storage now; the next call's words)
    with G.knobs(residual_f16=0):  # fp32 residual storage from the start
        ref_cfm = G.make_cfm(arch, V, big, "bf16")
        ref_cfm.transformer.set_attn_dropout(P, SEED)
        ref = [ref_cfm.sample(use_graph=False, **kw)[0].clone() for _ in range(2)]
    assert torch.equal(out, ref[0]) and torch.equal(second, ref[1]) and not torch.equal(out, second)
