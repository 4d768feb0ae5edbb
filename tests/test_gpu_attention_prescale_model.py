"""Pre-scaled q at model level: sample() with the plan option / knob "attn_prescale" on against off, eager and graph
replay, within the bf16 contract of tests/test_gpu_model.py (rel-L2 <= 2e-2 on the generated frames); and the option's read-back."""
import ctypes as C

import pytest
import torch

from conftest import golden_arch, golden_weights, load_golden, rel_l2

pytestmark = pytest.mark.gpu
TOL_BF16 = 2e-2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _active(model):
    """"attn_prescale_active" of the model's live plans"""
    from eraxvif5tts_amd import _lib
    vals = []
    for _, h in model._plans:
        v = C.c_int(-1)
        _lib.check(_lib.load().f5_plan_get_option(h, b"attn_prescale_active", C.byref(v)))
        vals.append(v.value)
    return vals


def _gen_rows(t, dur):
    return torch.cat([t[b, : int(d)] for b, d in enumerate(dur)])


def test_tiny_dit_sample_on_against_off(monkeypatch):
    """tiny DiT (tests/golden/tiny_base.npz), the tuned kernels forced so that the LayerNorm fold -- and with it the pre-scaled q -- runs at this
    size: on and off both hold the golden's tolerance, differ by no more than it, and graph replay equals eager bit for bit in both forms."""
    import gpu_helpers as G
    monkeypatch.setenv("F5HIP_GEMM_KERNEL", "1")
    monkeypatch.setenv("F5HIP_ATTN_KERNEL", "1")
    z = load_golden("tiny_base")
    arch, W = golden_arch(z), golden_weights(z)
    kw = dict(cond=torch.from_numpy(z["cond"]).cuda(), text=torch.from_numpy(z["text"]).cuda(), duration=torch.from_numpy(z["duration"]).cuda(),
              lens=torch.from_numpy(z["lens"]).cuda(), steps=int(z["steps"]), cfg_strength=float(z["cfg_strength"]), sway_sampling_coef=float(z["sway"]),
              y0=torch.from_numpy(z["y0"]))
    dur, ref = z["duration"], torch.from_numpy(z["out"])
    outs = {}
    for on in (1, 0):
        with G.knobs(attn_prescale=on):
            c = G.make_cfm(arch, int(z["vocab"]), W, "bf16")
            eager = c.sample(**kw, use_graph=False)[0].cpu()
            assert _active(c.transformer) == [on]
            assert torch.equal(c.sample(**kw, use_graph=True)[0].cpu(), eager)
            assert c.transformer.residual_fallbacks() == 0
            outs[on] = eager
            del c
    e_on, e_off = [rel_l2(_gen_rows(outs[k], dur), _gen_rows(ref, dur)) for k in (1, 0)]
    d = rel_l2(_gen_rows(outs[1], dur), _gen_rows(outs[0], dur))
    print(f"tiny_base vs golden: pre-scaled {e_on:.3e}, as projected {e_off:.3e}; on vs off {d:.3e}")
    assert e_on < TOL_BF16 and e_off < TOL_BF16 and d < TOL_BF16


def test_c1_shape_sample_on_against_off_and_taps_switch_it_off():
    """C1 (F5TTS_Base, 1 x 256 frames, NFE 8, cfg 1 -> 512 token rows, where the default kernel choice starts to fold): on against
    off, eager and graph; the same with the 64-queries-per-wave kernel forced (its reference-free build inside the model); and a plan with a
    stage tap reports the option as inactive."""
    import bench
    import gpu_helpers as G
    from eraxvif5tts_amd.model import CFM, DiT
    B, N = 1, 256
    cond, text, lens, dur = bench.synth_batch(B, N, "cuda", seed=61)
    y0 = torch.randn(B, N, 100, generator=torch.Generator().manual_seed(62))
    kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=8, cfg_strength=1.0, sway_sampling_coef=-1.0, y0=y0, return_trajectory=False)
    torch.manual_seed(1234)
    model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision="bf16"), seed=0)
    cfm = CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()
    outs = {}
    for on in (1, 0):
        with G.knobs(attn_prescale=on):
            outs[on] = cfm.sample(**kw, use_graph=False)[0].cpu()
            assert _active(model) == [on]
            assert torch.equal(cfm.sample(**kw, use_graph=True)[0].cpu(), outs[on])
    with G.knobs(attn_prescale=1):
        with G.knobs(attn_variant=2):
            outs["wide"] = cfm.sample(**kw, use_graph=False)[0].cpu()
        assert model.residual_fallbacks() == 0
        (_, plan), = model._plans
        tap = torch.zeros(B, N, bench.BASE_ARCH["dim"], device="cuda")
        model.set_tap(plan, "blk0.n1", tap)
        try:
            assert _active(model) == [0]
        finally:
            model.set_tap(plan, None, None)
        assert _active(model) == [1]
    n_ref = cond.shape[1]
    gen = lambda t: t[0, n_ref:N]
    d, dw = rel_l2(gen(outs[1]), gen(outs[0])), rel_l2(gen(outs["wide"]), gen(outs[0]))
    print(f"C1 shape, on vs off: {d:.3e}; on with the 64-queries-per-wave kernel vs off: {dw:.3e}")
    assert all(torch.isfinite(o).all() for o in outs.values())
    assert d < TOL_BF16 and dw < TOL_BF16
