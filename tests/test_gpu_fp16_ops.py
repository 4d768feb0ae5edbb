"""The fp16 precision mode (F5_PREC_FP16, include/f5hip.h) at op level: every kernel family of the mode against fp64 references computed from
exactly the values the kernel reads (inputs are rounded to fp16 on the host first, so the kernel's own input conversion is exact).

The bound is element-wise and derived from the number formats, none of it measured:
    linear / conv outputs   |out - ref| <= 1 fp16 ulp(ref) + 8 fp32 ulps of sum |a w|
        (one rounding of the stored element; the fp32 accumulation, bias add and epilogue arithmetic against the magnitude they work on)
    attention additionally  + 2^-11 sum_k p_k |v_k| / l      one fp16 rounding of each un-normalised numerator
                            + N 2^-25 max |v|                numerators in fp16's subnormal range (spacing 2^-24) against l >= 1: the exponent
                                                             reference is always a score of the row, so some numerator is at least 1
    where sum |a w| covers both products: the PV sum (sum_k p_k |v_k| / l) and, through the exponential, the score sum -- an error ds of a score
    is a relative error ds of its numerator, once in the numerator and once in l: 2 max_k(sum_d |q_d k_d| / 8) sum_k p_k |v_k| / l."""
import math

import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import fp16_ulp, knobs
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
P_BF16, P_FP16 = 0, 2
F32_ULPS = 8 * 2.0 ** -23


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def f16r(t):
    return t.half().float()


def check_f16(name, out, ref, scale, extra=None):
    """|out - ref| <= 1 fp16 ulp(ref) + 8 fp32 ulps of `scale` (+ extra), element-wise; prints the worst share of the bound before it asserts
    (gpu_helpers.check_elementwise: the comparator shared with test_gpu_gemm_tiles.py)."""
    import gpu_helpers as G
    return G.check_elementwise(name, out, ref, scale, P_FP16, extra)


def op_linear_fused_p(*args, **kw):
    import gpu_helpers as G
    return G.op_linear_fused_p(*args, **kw)


def op_ln_fold_p(*args, **kw):
    import gpu_helpers as G
    return G.op_ln_fold_p(*args, **kw)


def _problem(M, N, K, seed):
    import gpu_helpers as G
    return G.linear_problem(P_FP16, M, N, K, seed)


def _linear_ref(A, W, b, act):
    import gpu_helpers as G
    return G.linear_ref(A, W, b, act)


# ----------------------------------------------------------------------------- 1. generic tile kernel
@pytest.mark.parametrize("shape", [(100, 72, 96), (300, 1024, 512)])
@pytest.mark.parametrize("act", ["none", "gelu_tanh"])
def test_generic_tile_kernel(shape, act):
    import gpu_helpers as G
    M, N, K = shape
    _, A, W, b = _problem(M, N, K, M * 7 + N)
    ref, scale = _linear_ref(A, W, b, act)
    check_f16(f"tile {shape} {act}", G.op_linear(P_FP16, 0, A, W, b, act), ref, scale)


# ----------------------------------------------------------------------------- 2. tuned GEMM
KNOB_SETS = [{}, {"gemm_persist": 0, "gemm_lean": 0}]
KNOB_IDS = ["default_persistent_grid", "generic_epilogue"]


@pytest.mark.parametrize("kn", KNOB_SETS, ids=KNOB_IDS)
@pytest.mark.parametrize("shape", [(512, 1024, 1024), (300, 3072, 128), (77, 512, 640)])
@pytest.mark.parametrize("act", ["none", "gelu_tanh"])
def test_tuned_gemm(shape, act, kn):
    import gpu_helpers as G
    M, N, K = shape
    _, A, W, b = _problem(M, N, K, M + N + K)
    ref, scale = _linear_ref(A, W, b, act)
    with knobs(**kn):
        out = G.op_linear(P_FP16, 1, A, W, b, act)
    check_f16(f"tuned {shape} {act} {kn}", out, ref, scale)


def _fused_case(epi_name, M, N, K, seq, seed):
    """Inputs, the launch and the fp64 reference + fp32 magnitude of one fused epilogue (gpu_helpers.fused_case in fp16 mode)."""
    import gpu_helpers as G
    return G.fused_case(P_FP16, epi_name, M, N, K, seq, seed)


@pytest.mark.parametrize("kn", KNOB_SETS, ids=KNOB_IDS)
@pytest.mark.parametrize("epi_name", ["store", "rope", "resid", "gate"])
def test_tuned_gemm_epilogues(kn, epi_name):
    """(512, 1024, 256): the smallest whole-tile persistent case; lean epilogues by default, the generic one with the knobs."""
    M, N, K = 512, 1024, 256
    if epi_name == "rope":
        N = 768
    run, ref, scale = _fused_case(epi_name, M, N, K, 256, M + 3 * N + K)
    with knobs(**kn):
        out = run()
    check_f16(f"fused {epi_name} {kn}", out, ref, scale)
    check_f16(f"fused {epi_name} tile kernel", run(0), ref, scale)


# ----------------------------------------------------------------------------- 3. one-wave-per-SIMD kernel
@pytest.mark.parametrize("epi_name,shape,seq", [("rope", (2048, 3072, 1024), 1024), ("store", (2048, 2048, 1024), 0), ("resid", (6144, 1024, 2048), 0)])
def test_w4_kernel(epi_name, shape, seq):
    """The partly-filled-grid shapes of the one-wave-per-SIMD kernel in fp16: against fp64, and bit-equal to the 8-wave kernel."""
    M, N, K = shape
    run, ref, scale = _fused_case(epi_name, M, N, K, seq, M + 11 * N + K)
    new = run()
    with knobs(gemm_w4=0):
        old = run()
    check_f16(f"w4 {epi_name} {shape}", new, ref, scale)
    assert torch.equal(new, old)


# ----------------------------------------------------------------------------- 4. LayerNorm fold site
@pytest.mark.parametrize("M,D,N,Kb,epi", [(300, 128, 384, 128, 4), (300, 128, 256, 256, 0)], ids=["qkv_rope", "ff1_gelu"])
def test_layernorm_fold_site(M, D, N, Kb, epi):
    """One fold site at offset 40 through f5_op_ln_fold_p: the output now carries fp16 rounding; the stream and the statistics are bit-equal to
    the bf16-mode call on the same inputs (A and Wo hold values exact in both 16-bit types).  The reference of the folded projection is
    rstd (x . W'^T - mean c1) + c2 in fp64 from the kernel's own stream, statistics and table (f5_op_fold_weights)."""
    import gpu_helpers as G
    args, kw = G.ln_fold_inputs(M, D, N, Kb, epi)
    xs, stats, out = op_ln_fold_p(P_FP16, epi, *args, **kw)
    xs_b, stats_b, _ = op_ln_fold_p(P_BF16, epi, *args, **kw)
    assert torch.equal(xs, xs_b) and torch.equal(stats, stats_b)
    ref, mag = G.ln_fold_ref(args, kw, epi, xs, stats)
    check_f16(f"ln_fold epi {epi}", out, ref, mag)
    assert torch.equal(out, out.half().float())  # the values are fp16 numbers


# ----------------------------------------------------------------------------- 5. position conv
def position_conv_case(dim, B, N):
    """Inputs of mish(conv(mish(conv(x)))) rounded to fp16, its fp64 reference with the intermediate ROUNDED to fp16, the magnitude of the
    second sum and the propagated term of the intermediate's own ulp (test_position_conv)."""
    g = torch.Generator().manual_seed(dim + N)
    x = f16r(torch.randn(B, N, dim, generator=g))
    cg = dim // 16
    w0, w1 = [f16r(torch.randn(dim, cg, 31, generator=g) / math.sqrt(cg * 31)) for _ in range(2)]
    b0, b1 = torch.randn(dim, generator=g) * 0.1, torch.randn(dim, generator=g) * 0.1

    def conv(inp, w, b):  # [B, N, dim] fp64, grouped Conv1d(k = 31, padding = 15, groups = 16) and the sum of magnitudes
        t = inp.transpose(1, 2)
        return (F.conv1d(t, w.double(), b.double(), padding=15, groups=16).transpose(1, 2),
                F.conv1d(t.abs(), w.double().abs(), b.double().abs(), padding=15, groups=16).transpose(1, 2))

    c1, s1 = conv(x.double(), w0, b0)
    m1 = F.mish(c1)
    m1h = m1.half().double()  # what the kernel stores between the two convolutions, up to one ulp
    c2, s2 = conv(m1h, w1, b1)
    ref = F.mish(c2)
    # an intermediate element off by one fp16 ulp (+ its own fp32 slack) moves the second sum by |w1| times that
    d1 = fp16_ulp(m1) + 1.1 * F32_ULPS * s1
    prop, _ = conv(d1, w1.abs(), torch.zeros_like(b1))
    return (x, w0, b0, w1, b1), ref, 1.1 * s2, 1.1 * prop


@pytest.mark.parametrize("conv31", [1, 0], ids=["halo_tile_kernel", "implicit_gemm"])
@pytest.mark.parametrize("dim,B,N", [(1024, 2, 70), (1024, 1, 700)])
def test_position_conv(conv31, dim, B, N):
    """mish(conv(mish(conv(x)))) with the tuned kernels as dit_eval launches them (the second conv stores its branch): the intermediate
    activation is an fp16 buffer, so the second conv's reference is taken from the first conv's fp64 result ROUNDED to fp16 -- the bound
    allows the first conv one ulp of its own: a one-ulp change of an intermediate element moves the output by |w| ulp(c1) (mish' < 1.1)."""
    import gpu_helpers as G
    args, ref, scale, prop = position_conv_case(dim, B, N)
    with knobs(op_conv_kernel=1, conv31=conv31):
        out = G.op_conv_pos(P_FP16, *args)
    check_f16(f"conv31={conv31} {(dim, B, N)}", out, ref, scale, extra=prop)


@pytest.mark.parametrize("dim,B,N", [(128, 2, 70), (1024, 1, 40)])
def test_position_conv_untuned(dim, B, N):
    """op_conv_kernel = 0 (the entry point's default): the GEMM_CONV31 path of the generic tile kernel in fp16 -- the first conv stores its fp16
    intermediate, the second accumulates into an fp32 buffer, so the output's own fp16 ulp in the bound is an allowance here.  Reference and
    bound of test_position_conv, its propagated term for the fp16 intermediate included."""
    import gpu_helpers as G
    args, ref, scale, prop = position_conv_case(dim, B, N)
    with knobs(op_conv_kernel=0):
        out = G.op_conv_pos(P_FP16, *args)
    check_f16(f"untuned position conv {(dim, B, N)}", out, ref, scale, extra=prop)


# ----------------------------------------------------------------------------- 6. / 7. attention
def _attn_ref(qkv, mask):
    """fp64 softmax attention and the terms of the bound (module docstring): (ref, fp32 magnitude, numerator-rounding allowance) -- the fp16
    terms of gpu_helpers.attn_ref_terms, the reference the bf16 element-wise tests share."""
    import gpu_helpers as G
    return G.attn_ref_terms(qkv, mask, P_FP16)


def _run_attention(qkv, mask, variant):
    import gpu_helpers as G
    with knobs(attn_variant=variant):
        return G.op_attention(P_FP16, 1, qkv, mask)


@pytest.mark.parametrize("variant", [0, 2, 5], ids=["by_grid_size", "64_queries_per_wave", "pipelined_32_queries_per_wave"])
@pytest.mark.parametrize("B,N,H,masked", [(2, 200, 3, True), (1, 1024, 2, False), (2, 1024, 4, True), (1, 2050, 2, False)])
def test_attention(B, N, H, masked, variant):
    g = torch.Generator().manual_seed(N + H)
    qkv = f16r(torch.randn(B, N, 3, H, 64, generator=g) * 1.5)
    mask = None
    if masked:
        lens = torch.tensor([N, max(1, N - 13)][:B])
        mask = torch.arange(N)[None, :] < lens[:, None]
    ref, mag, extra = _attn_ref(qkv, mask)
    out = _run_attention(qkv, mask, variant)
    valid = slice(None) if mask is None else mask
    assert torch.isfinite(out).all()
    check_f16(f"attention {(B, N, H, masked)} variant {variant}", out[valid], ref[valid], mag[valid], extra[valid])


@pytest.mark.parametrize("B,N,H,masked", [(2, 70, 2, True), (1, 200, 3, False)])
def test_attention_reference_kernel(B, N, H, masked):
    """attn_ref_kernel<f16_t> (attention kernel 0 in fp16 mode) against the same element-wise bound.  The reference kernel keeps its
    numerators in fp32, so the bound's numerator-rounding term is an allowance here, not a requirement."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(N + H)
    qkv = f16r(torch.randn(B, N, 3, H, 64, generator=g) * 1.5)
    mask = None
    if masked:
        lens = torch.tensor([N, max(1, N - 13)][:B])
        mask = torch.arange(N)[None, :] < lens[:, None]
    ref, mag, extra = _attn_ref(qkv, mask)
    out = G.op_attention(P_FP16, 0, qkv, mask)
    valid = slice(None) if mask is None else mask
    check_f16(f"attention reference kernel {(B, N, H, masked)}", out[valid], ref[valid], mag[valid], extra[valid])


@pytest.mark.parametrize("variant", [2, 5], ids=["64_queries_per_wave", "pipelined_32_queries_per_wave"])
@pytest.mark.parametrize("jump", [20.0, 14.5])
def test_attention_range(variant, jump):
    """Where the mode can go wrong and bf16 cannot: a key of the LAST tile whose score exceeds every earlier score of its row by `jump` log2
    units.  20 is past 2^15, so both kernels must move their exponent reference (left where it is, the numerator 2^20 is inf in fp16); 14.5
    is inside the wide kernel's limit (row sums below 2^15 stay on the common path) and at the pipelined kernel's (more than 14 moves the
    reference).  Construction of test_attention_wide_kernel_range_guard / test_attention_deferred_rescale_thresholds: unit queries scaled to
    |q| = 8, so q . k / 8 = |k| cos; values such as 32768 that are exact in both formats keep the reference exact."""
    g = torch.Generator().manual_seed(21)
    B, N, H = 2, 1024, 2
    LOG2E = 1.4426950408889634
    qkv = torch.randn(B, N, 3, H, 64, generator=g) * 0.5
    spiked = {5: 1000, 37: 990, 90: 1023, 200: 961, 700: 975}  # query -> a key of the last tile
    for bb in range(B):
        qn = qkv[bb, :, 0] / qkv[bb, :, 0].norm(dim=-1, keepdim=True)
        for q, key in spiked.items():
            qkv[bb, q, 0] = qn[q] * 8.0
    qkv = f16r(qkv)
    # Every spike key is set so that its score sits `jump` log2 units above the largest OTHER score of its row -- the other rows' spike keys
    # included, which score a few nats against every query: three passes over all spikes from the rounded values, then the margins are
    # measured once more below, on the values the kernel reads.
    def others_max(bb, q, key, hh):
        s = (qkv[bb, :, 1, hh].double() @ qkv[bb, q, 0, hh].double()) / 8.0
        s[key] = -1e9
        return float(s.max())

    for _ in range(3):
        for bb in range(B):
            for q, key in spiked.items():
                for hh in range(H):
                    qv = qkv[bb, q, 0, hh].double()
                    want = others_max(bb, q, key, hh) + jump / LOG2E
                    qkv[bb, key, 1, hh] = f16r((qv / (qv @ qv) * 8.0 * want).float())
    qkv[0, 3, 2] = 32768.0  # a value row at the top of the range, exact in both formats
    qkv = f16r(qkv)
    for bb in range(B):  # every spiked row has the stated margin (log2 units) over every other score of its row, to the rounding of the key
        for q, key in spiked.items():
            for hh in range(H):
                own = float(qkv[bb, key, 1, hh].double() @ qkv[bb, q, 0, hh].double()) / 8.0
                margin = (own - others_max(bb, q, key, hh)) * LOG2E
                assert abs(margin - jump) < 0.1, (bb, q, hh, margin)
    ref, mag, extra = _attn_ref(qkv, None)
    out = _run_attention(qkv, None, variant)
    assert torch.isfinite(out).all()
    check_f16(f"attention range jump {jump} variant {variant}", out, ref, mag, extra)


# ----------------------------------------------------------------------------- 8. saturation
@pytest.mark.parametrize("kernel", [0, 1], ids=["tile_kernel", "tuned_kernel"])
def test_activation_store_saturates(kernel):
    """A linear whose exact output is 70000 in one element stores 65504 there (the fp16 activation stores clip, they never write inf), and the
    neighbours are unaffected."""
    import gpu_helpers as G
    M, N, K = 256, 256, 64
    g = torch.Generator().manual_seed(8)
    A, W, b = f16r(torch.randn(M, K, generator=g)), f16r(torch.randn(N, K, generator=g) / 8.0), torch.zeros(N)
    A[17] = 0.0
    A[17, 0] = 250.0   # row 17: 250 * 280 = 70000 in column 33, 250 * w elsewhere
    W[33, 0] = 280.0
    W[200, 0] = -280.0
    ref = A.double() @ W.double().t()
    assert ref[17, 33] == 70000.0 and ref[17, 200] == -70000.0
    out = op_linear_fused_p(P_FP16, kernel, G.EPI_STORE_T, A, W, b, "none")
    assert out[17, 33] == 65504.0 and out[17, 200] == -65504.0
    ref[17, 33], ref[17, 200] = 65504.0, -65504.0
    check_f16("saturating store", out, ref, A.double().abs() @ W.double().abs().t())


def test_non_finite_weight_fails_finalize_with_its_name():
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    arch = dict(dim=128, depth=1, heads=2, ff_mult=2, text_dim=64, conv_layers=0, pe_attn_head=1, text_mask_padding=False)
    W = dict(cpu_ref.random_dit_weights(arch, 20, seed=5))
    name = "transformer_blocks.0.ff.ff.2.weight"
    W[name] = W[name].clone()
    W[name][3, 7] = float("inf")
    with pytest.raises(_lib.F5HipError, match=name.replace(".", r"\.")):
        G.make_dit(arch, 20, W, "fp16").native()
    W[name][3, 7] = 70000.0  # finite in fp32 and in bf16, inf after the rounding to fp16
    with pytest.raises(_lib.F5HipError, match=name.replace(".", r"\.")):
        G.make_dit(arch, 20, W, "fp16").native()
    G.make_dit(arch, 20, W, "bf16").native()
    # a matrix the library keeps in fp32 (the time MLP) may hold such a value: only what is rounded to fp16 is tested
    W[name][3, 7] = 0.5
    big = "time_embed.time_mlp.0.weight"
    W[big] = W[big].clone()
    W[big][0, 0] = 70000.0
    G.make_dit(arch, 20, W, "fp16").native()
