"""CFM.forward / CFM.flow_loss / eval.validate.validation_loss on the device, over the tiny DiT, UNetT and MMDiT of tests/test_gpu_model.py.

B = 2 with different lengths, every draw injected, both values of the drop flags.  `pred` against the CPU oracle's forward on the kernel's own phi
and cond, at the tolerance test_gpu_model.py's forward-parity tests use for the backbone and precision (STAGE_TOL, imported from there); `loss`
against the fp64 formula on the returned pred (equal or one fp32 ulp apart); validation_loss twice for identical bits; sample() before and after
a forward() for identical bits (the forward leaves plan caches and captured graphs sound)."""
import ast
import math
import random

import numpy as np
import pytest
import torch

from conftest import golden_arch, golden_weights, load_golden, rel_l2
from oracle import cpu_ref
from test_gpu_model import STAGE_TOL, _make_mmdit, _make_unett

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _build(backbone, prec):
    """(cfm, oracle forward(x, cond, text, time, drop_audio_cond, drop_text), vocab)"""
    import gpu_helpers as G
    if backbone == "dit":
        z = load_golden("tiny_base")
        arch, W, V = golden_arch(z), golden_weights(z), int(z["vocab"])
        return G.make_cfm(arch, V, W, prec), lambda *a: cpu_ref.dit_forward(W, arch, *a), V
    z = load_golden("tiny_unett" if backbone == "unett" else "tiny_mmdit")
    arch, V, seed = ast.literal_eval(str(z["a.arch"])), int(z["a.vocab"]), int(z["a.seed"])
    if backbone == "unett":
        W = cpu_ref.random_unett_weights(arch, V, seed=seed)
        return _make_unett(arch, V, W, prec)[1], lambda *a: cpu_ref.unett_forward(W, arch, *a), V
    W = cpu_ref.random_mmdit_weights(arch, V, seed=seed)
    return _make_mmdit(arch, V, W, prec)[1], lambda *a: cpu_ref.mmdit_forward(W, arch, *a), V


def _batch(V, B=2, N=56, seed=5):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([N, N - 12][:B])
    mel = torch.randn(B, N, 100, generator=g) * 2 - 3
    mel = torch.where(torch.arange(N)[None, :, None] < lens[:, None, None], mel, torch.zeros(()))
    text = torch.randint(0, V, (B, 18), generator=g)
    text[B - 1, 13:] = -1
    return mel, text, lens, g


def _ulps_apart(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("backbone,prec", [("dit", "fp32"), ("dit", "bf16"), ("unett", "fp32"), ("mmdit", "fp32")])
def test_flow_loss_on_the_device(backbone, prec, drop):
    cfm, oracle, V = _build(backbone, prec)
    mel, text, lens, g = _batch(V)
    x0 = torch.randn(mel.shape, generator=g)
    time = torch.tensor([0.3, 0.85])
    span = torch.zeros(mel.shape[:2], dtype=torch.bool)
    span[0, 9:50] = True
    span[1, 2:40] = True
    state, pstate = torch.get_rng_state(), random.getstate()
    r = cfm.flow_loss(mel.cuda(), text.cuda(), lens=lens.cuda(), x0=x0, time=time, rand_span_mask=span, drop_audio_cond=drop, drop_text=drop)
    assert torch.equal(torch.get_rng_state(), state) and random.getstate() == pstate  # every draw was given: none is made
    assert r.pred.is_cuda and r.loss.is_cuda and not r.pred.requires_grad and (r.drop_audio_cond, r.drop_text) == (drop, drop)
    # the kernel's phi is what the backbone saw; rebuild it the torch way (bit-equal: tests/test_gpu_cfm_loss.py) and hand it to the oracle
    t = time[:, None, None]
    phi = (1 - t) * x0 + t * mel
    cond = torch.where(span[..., None], torch.zeros_like(mel), mel)
    assert torch.equal(r.cond.cpu(), cond) and torch.equal(r.rand_span_mask.cpu(), span) and torch.equal(r.x0.cpu(), x0)
    want = oracle(phi, cond, text, time, drop, drop)
    err = rel_l2(r.pred.cpu(), want)
    print(f"  {backbone} {prec} drop={drop}: pred rel-L2 {err:.3e} (bound {STAGE_TOL[prec]})")
    assert err < STAGE_TOL[prec]
    # the loss of the returned pred: fp32 squares, fp64 sum
    pred = r.pred.cpu().float()
    flow = mel - x0
    d = pred - flow
    sq = (d * d).double()
    sums = torch.stack([sq[b][span[b]].sum() for b in range(2)])
    counts = span.sum(dim=1) * 100
    assert torch.equal(r.counts.cpu(), counts)
    assert all(abs(float(a) - float(b)) <= 1e-12 * float(b) for a, b in zip(r.sums.cpu(), sums))
    assert _ulps_apart(float(r.loss), float(sums.sum()) / int(counts.sum())) <= 1
    # forward() is the same computation behind the reference's signature
    random.seed(1)
    torch.manual_seed(1)
    loss, cond2, pred2 = cfm(mel.cuda(), text.cuda(), lens=lens.cuda())
    assert loss.ndim == 0 and math.isfinite(float(loss)) and cond2.shape == pred2.shape == mel.shape


def test_validation_loss_twice_gives_the_same_bits():
    from eraxvif5tts_amd.eval import validation_loss
    cfm, _, V = _build("dit", "bf16")
    batches = []
    for N, seed in ((56, 1), (41, 2)):
        mel, text, lens, _ = _batch(V, N=N, seed=seed)
        batches.append((mel.cuda(), text.cuda(), lens.tolist()))
    a = validation_loss(cfm, batches, seed=11)
    b = validation_loss(cfm, batches, seed=11)
    assert a.loss == b.loss and torch.equal(a.sums, b.sums) and torch.equal(a.counts, b.counts)
    assert math.isfinite(a.loss) and a.loss == math.fsum(a.sums.tolist()) / int(a.counts.sum())
    parts = []
    for i, (mel, text, lens) in enumerate(batches):
        torch.manual_seed(11 + i)
        random.seed(11 + i)
        parts.append(cfm.flow_loss(mel, text, lens=torch.tensor(lens).cuda(), drop_audio_cond=False, drop_text=False))
    assert torch.equal(a.sums, torch.cat([p.sums for p in parts]).cpu()) and torch.equal(a.counts, torch.cat([p.counts for p in parts]).cpu())
    assert a.frames == int(sum(int(p.rand_span_mask.sum()) for p in parts))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sample_is_unchanged_by_a_forward_in_between(prec):
    cfm, _, V = _build("dit", prec)
    z = load_golden("tiny_base")
    kw = dict(cond=torch.from_numpy(z["cond"]).cuda(), text=torch.from_numpy(z["text"]).cuda(), duration=torch.from_numpy(z["duration"]).cuda(),
              lens=torch.from_numpy(z["lens"]).cuda(), steps=int(z["steps"]), cfg_strength=float(z["cfg_strength"]), sway_sampling_coef=float(z["sway"]),
              y0=torch.from_numpy(z["y0"]))
    first = cfm.sample(**kw)[0].clone()    # eager
    second = cfm.sample(**kw)[0].clone()   # the shape recurs: captured and replayed
    mel, text, lens, _ = _batch(V, N=int(z["duration"].max()))  # the sampler's own (B, N): the forward meets the same plan bucket
    for seed in (1, 2):
        torch.manual_seed(seed)
        random.seed(seed)
        loss, _, _ = cfm(mel.cuda(), text.cuda(), lens=lens.cuda())
        assert math.isfinite(float(loss))
    third = cfm.sample(**kw)[0]            # replayed after the forwards
    assert torch.equal(first, second) and torch.equal(second, third)
