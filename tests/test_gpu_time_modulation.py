"""The time path per element: compute_modulation (csrc/eval_common.hip) -- time_sinus_kernel, then gemv_rows_kernel three times (Linear -> SiLU,
Linear, Linear(SiLU(t_emb)) for the AdaLN rows of every block and the final norm) -- read back through the stage taps "t_sin", "t_emb" and "adaln"
of one forward with per-sample times t = [0, 1e-3, 0.37, 0.999, 1], against float64 on the model's fp32 weights.

gemv_rows_kernel has three instances, picked by K alone: KV = 1 (K <= 256), KV = 4 (K <= 1024), KV = 8 (K <= 2048); the first gemv has K = 256, the
other two K = dim.  The dims below put every instance's whole and partial vector counts behind the second and third gemv: 256 (KV = 1), 384 (KV =
4, 96 of 256 vectors), 1024 (KV = 4, full), 1280 (KV = 8, 320 of 512 vectors), 2048 (KV = 8, full).  One MMDiT at dim 384, depth 2: its modulation
row is [x 6D | c 6D] per block, [x 6D | c 2D] in the last, then 2D.

Bound: gpu_helpers.check_rounded(precision = fp32), |out - ref| <= 1e-5 |ref| + 8 fp32 ulps of `scale`, with
    sinusoid        scale = 1 + |1000 t f_j|            (the argument is itself an fp32 product; row t = 0 is held to [0.., 1..] exactly)
    each Linear     scale = |b| + sum_k |w_k x_k|, plus the bound of its inputs carried through sum_k |w_k| (SiLU's slope is at most 1.1)
That chain bound is wide by construction: the sinusoid's slack at |argument| = 1000 is 1e-3, and two more layers of sum |w| bring it to 2e-2 ..
5e-2 at t_emb and 0.2 .. 0.8 at the AdaLN rows, whose values are about 0.1 (measured: the kernels use 0.001 of it).  So t_emb is also held to the
same bound taken from the DEVICE's t_sin, and the AdaLN rows from the device's t_emb: there only the fp32 evaluation of the gemv under test is in
the bound (about 2e-4 of a value; measured share 0.001 and 0.010 .. 0.016), and a dropped or doubled vector group of any instance's tail, an
error of the order of the value, cannot pass.  The path is fp32 in every precision mode: the three modes must give the same bits."""
import math

import pytest
import torch

import gpu_helpers as G
from gpu_helpers import P_FP32
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
V, B, N = 200, 5, 64
TIMES = [0.0, 1e-3, 0.37, 0.999, 1.0]
U8 = 8 * 2.0 ** -23  # check_rounded's slack per unit of scale


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@pytest.fixture(autouse=True)
def _launcher_defaults(monkeypatch):
    for k in ("F5HIP_GEMM_KERNEL", "F5HIP_ATTN_KERNEL", "F5HIP_PRECISION", "F5HIP_ROPE_LAYOUT"):
        monkeypatch.delenv(k, raising=False)


def _silu(x):
    return x * torch.sigmoid(x)


def _linear_terms(W, b, x, xbound):
    """fp64 Linear of x [n, K] and the per-element bound of its fp32 evaluation: check_rounded's own (1e-5 |ref| + U8 scale) with the inputs'
    bound carried through sum_k |w_k|, folded into `scale`.  -> (ref, scale, bound)"""
    W, b = W.double(), b.double()
    ref = x @ W.t() + b
    scale = b.abs()[None] + x.abs() @ W.abs().t() + (xbound @ W.abs().t()) / U8
    return ref, scale, 1e-5 * ref.abs() + U8 * scale


def _silu_terms(ref, bound):
    """SiLU of a value known to `bound`: slope at most 1.1, evaluated in fp32 to a few ulps of itself"""
    y = _silu(ref)
    return y, 1.1 * bound + U8 * y.abs()


def _adaln_weights(W, arch, mmdit):
    names = []
    for i in range(arch["depth"]):
        p = f"transformer_blocks.{i}."
        names += [p + "attn_norm_x.linear.", p + "attn_norm_c.linear."] if mmdit else [p + "attn_norm.linear."]
    names.append("norm_out.linear.")
    return torch.cat([W[n + "weight"] for n in names]), torch.cat([W[n + "bias"] for n in names])


def _reference(W, arch, mmdit):
    t = torch.tensor(TIMES, dtype=torch.float32).double()  # (the fp32 values the kernel reads)
    k = math.log(10000) / 127
    f = torch.exp(torch.arange(128, dtype=torch.float64) * -k)
    arg = 1000.0 * t[:, None] * f[None, :]
    sin = torch.cat([arg.sin(), arg.cos()], dim=-1)
    s_scale = torch.cat([1 + arg.abs(), 1 + arg.abs()], dim=-1)
    s_bound = 1e-5 * sin.abs() + U8 * s_scale
    s_bound[0] = 0.0  # t = 0: exactly [0.., 1..]
    a1, _, b1 = _linear_terms(W["time_embed.time_mlp.0.weight"], W["time_embed.time_mlp.0.bias"], sin, s_bound)
    h, bh = _silu_terms(a1, b1)
    temb, temb_scale, temb_bound = _linear_terms(W["time_embed.time_mlp.2.weight"], W["time_embed.time_mlp.2.bias"], h, bh)
    Wd = {k_: v.double() for k_, v in W.items() if k_.startswith("time_embed.")}
    # the oracle's own on the weights cast to double: the same function (its sinusoid argument stays an fp32 product, hence the tolerance)
    oracle = cpu_ref.timestep_embedding(Wd, t)
    assert float((temb - oracle).norm() / oracle.norm()) < 1e-3
    x, bx = _silu_terms(temb, temb_bound)
    wa, ba = _adaln_weights(W, arch, mmdit)
    mod, mod_scale, _ = _linear_terms(wa, ba, x, bx)
    return dict(sin=sin, s_scale=s_scale, temb=temb, temb_scale=temb_scale, mod=mod, mod_scale=mod_scale, wa=wa, ba=ba)


def _run(model, mmdit, modrow, D):
    g = torch.Generator().manual_seed(11)
    x, cond = torch.randn(B, N, 100, generator=g), torch.randn(B, N, 100, generator=g)
    text = torch.randint(0, V, (B, 12), generator=g)
    plan = model.plan(B, model._plan_seq(N, text.shape[1]), 1)
    taps = {"t_sin": torch.full((B, 256), float("nan")), "t_emb": torch.full((B, D), float("nan")), "adaln": torch.full((B, modrow), float("nan"))}
    taps = {k: v.cuda() for k, v in taps.items()}
    for k, v in taps.items():
        model.set_tap(plan, k, v)
    out = model(x=x.cuda(), cond=cond.cuda(), text=text.cuda(), time=torch.tensor(TIMES).cuda(), drop_audio_cond=False, drop_text=False)
    torch.cuda.synchronize()
    model.set_tap(plan, None, None)
    assert torch.isfinite(out).all()
    return {k: v.cpu() for k, v in taps.items()}


def _check(tag, arch, W, make, mmdit):
    D = arch["dim"]
    ref = _reference(W, arch, mmdit)
    modrow = ref["mod"].shape[1]
    assert modrow == ((12 * arch["depth"] - 2) * D if mmdit else (6 * arch["depth"] + 2) * D)
    first = None
    for prec in ("fp32", "bf16", "fp16"):
        m = make(prec)
        got = _run(m, mmdit, modrow, D)
        del m
        torch.cuda.empty_cache()
        if first is None:
            first = got
            continue
        for k in got:  # the path is fp32 in every mode
            assert torch.equal(got[k], first[k]), (tag, prec, k, float((got[k] - first[k]).abs().max()))
    sin = first["t_sin"]
    assert torch.equal(sin[0], torch.cat([torch.zeros(128), torch.ones(128)])), "t = 0: the sinusoid row is exactly [0.., 1..]"
    G.check_rounded(f"{tag} t_sin", sin, ref["sin"], ref["s_scale"], P_FP32)
    G.check_rounded(f"{tag} t_emb (K = 256, then K = {D})", first["t_emb"], ref["temb"], ref["temb_scale"], P_FP32)
    G.check_rounded(f"{tag} adaln from the reference's t_emb (K = {D}, N = {modrow})", first["adaln"], ref["mod"], ref["mod_scale"], P_FP32)
    # The sinusoid's slack at |argument| = 1000 is 1e-3 and grows through two more layers: the chain bounds above are wide.  What holds each
    # gemv instance's tail is the same bound taken from the DEVICE's own values of the stage before, where only fp32 evaluation error remains.
    sd = sin.double()
    a1, _, b1 = _linear_terms(W["time_embed.time_mlp.0.weight"], W["time_embed.time_mlp.0.bias"], sd, torch.zeros_like(sd))
    h, bh = _silu_terms(a1, b1)
    local, lscale, _ = _linear_terms(W["time_embed.time_mlp.2.weight"], W["time_embed.time_mlp.2.bias"], h, bh)
    G.check_rounded(f"{tag} t_emb from the device's t_sin (the first two gemv alone)", first["t_emb"], local, lscale, P_FP32)
    xd = _silu(first["t_emb"].double())
    local, lscale, _ = _linear_terms(ref["wa"], ref["ba"], xd, U8 * xd.abs())
    G.check_rounded(f"{tag} adaln from the device's t_emb (the third gemv alone)", first["adaln"], local, lscale, P_FP32)


@pytest.mark.parametrize("dim", [256, 384, 1024, 1280, 2048])
def test_dit_time_modulation_rows_against_fp64(dim):
    arch = dict(dim=dim, depth=1, heads=2, ff_mult=2, text_dim=128, conv_layers=0, pe_attn_head=1)
    W = cpu_ref.random_dit_weights(arch, V, seed=9000 + dim)
    _check(f"dit{dim}", arch, W, lambda prec: G.make_dit(arch, V, W, prec), False)


def test_mmdit_384_time_modulation_rows_against_fp64():
    from test_gpu_model import _make_mmdit
    arch = dict(dim=384, depth=2, heads=2, ff_mult=2, text_mask_padding=True)
    W = cpu_ref.random_mmdit_weights(arch, V, seed=9384)
    _check("mmdit384", arch, W, lambda prec: _make_mmdit(arch, V, W, prec)[0], True)
