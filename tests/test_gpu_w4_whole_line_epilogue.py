"""The whole-line store epilogue of the one-wave-per-SIMD block GEMM (csrc/gemm_w4.hip, 256-row tiles of the store builds: QKV + RoPE, FF1 + GELU).

There the MFMA's operand roles are swapped (tokens on the row index) and the weight rows are permuted on their way into LDS, so that a lane holds
eight consecutive features of one token per (token tile, component) and 16 adjacent lanes store 256 contiguous bytes.  Products, K order, start
value and epilogue arithmetic are unchanged, so every case is BIT-EQUAL to the 8-wave kernel (knob gemm_w4 = 0) and within the fp64 tolerance of
the store epilogues (rel-L2 3e-3: bf16 output rounding).  Bias, gate, c1 and c2 are random per feature: a permutation error in the new indexing
(feature 8 c + i of lane column c, token 16 j + 4 q + r) moves values between columns and shows in both checks.

The in-place residual epilogue (EPI_RESID) and the 128-row tiles keep the old lane map: no case here for them (test_gpu_ops.py has theirs)."""
import math

import pytest
import torch

from conftest import rel_l2
from test_gpu_ops import _fused_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _both(run, bm=256):
    """(one-wave-per-SIMD kernel at tile height bm, 8-wave kernel)"""
    import gpu_helpers as G
    with G.knobs(gemm_w4_bm=bm):
        new = run()
    with G.knobs(gemm_w4=0):
        return new, run()


def test_store_gelu_second_tile_and_shortest_loop():
    """(a) 22 528 x 768 x 256: 88 x 3 = 264 tall tiles on 256 CUs, so eight workgroups walk a second tile (the next tile's bias is loaded in the new
    per-lane form in front of the first tile's stores); K / 64 = 4 is the shortest main loop; three feature tiles use both wave columns."""
    import gpu_helpers as G
    M, N, K = 22528, 768, 256
    g = torch.Generator().manual_seed(M + 7 * N + K)
    A, W, b = G.bf16_round(torch.randn(M, K, generator=g)), G.bf16_round(torch.randn(N, K, generator=g) / math.sqrt(K)), torch.randn(N, generator=g)
    new, old = _both(lambda: G.op_linear_fused(1, G.EPI_STORE_T, A, W, b, "gelu_tanh"))
    ref = _fused_ref(G.EPI_STORE_T, A, W, b, "gelu_tanh", None, None, None, 0, 0)
    e_new, e_old = rel_l2(new, ref), rel_l2(old, ref)
    print(f"store+gelu {M}x{N}x{K}: rel-L2 {e_new:.2e} (8-wave {e_old:.2e})")
    assert e_new < 3e-3 and e_old < 3e-3
    assert torch.equal(new, old)


@pytest.mark.parametrize("heads", [1, 4], ids=["one_rotating_half", "every_head"])
def test_rope_position_wraps_inside_a_wave(heads):
    """(b) 19 200 x 768, seq = 400: 75 x 3 = 225 tall tiles (the launcher's own choice from three quarters of the CUs on; the forced height asks for a
    tile per CU); a wave's 128 token rows cross an utterance boundary in most tiles, so the per-token position wraps between the four components
    of a lane and between token tiles.  rope_heads 1: wave column 0 holds one rotating and one plain half (per-lane select); 4: q and k rotate
    whole, v not."""
    import gpu_helpers as G
    M, N, K, seq = 19200, 768, 256, 400
    g = torch.Generator().manual_seed(M + 7 * N + K + heads)
    A, W, b = G.bf16_round(torch.randn(M, K, generator=g)), G.bf16_round(torch.randn(N, K, generator=g) / math.sqrt(K)), torch.randn(N, generator=g)
    ang = torch.rand(seq, 32, generator=g) * 6.28
    rope = torch.stack([ang.cos(), ang.sin()], dim=-1)
    new, old = _both(lambda: G.op_linear_fused(1, G.EPI_ROPE_T, A, W, b, "none", None, None, rope, heads, seq), bm=0)
    ref = _fused_ref(G.EPI_ROPE_T, A, W, b, "none", None, None, rope, heads, seq)
    e_new, e_old = rel_l2(new, ref), rel_l2(old, ref)
    print(f"rope heads={heads} {M}x{N}x{K} seq={seq}: rel-L2 {e_new:.2e} (8-wave {e_old:.2e})")
    assert e_new < 3e-3 and e_old < 3e-3
    assert torch.equal(new, old)


def _fold_problem(N, epi, seed):
    import gpu_helpers as G
    M, D, Kb, seq = 16384, 1024, 256, 2048
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g) * 1.7 + torch.randn(M, 1, generator=g) * 0.5
    A = G.bf16_round(torch.randn(M, Kb, generator=g))
    Wo = G.bf16_round(torch.randn(D, Kb, generator=g) / Kb ** 0.5)
    bo, gate = torch.randn(D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.3
    W, bias = torch.randn(N, D, generator=g) / D ** 0.5, torch.randn(N, generator=g) * 0.1
    scale, shift = torch.randn(D, generator=g) * 0.2, torch.randn(D, generator=g) * 0.3
    rope = None
    if epi == 4:
        ang = torch.arange(seq)[:, None] * (1.0 / 10000.0 ** (torch.arange(0, 64, 2) / 64.0))[None, :]
        rope = torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(seq, 64).float()
    args = (epi, x, A, Wo, bo, gate, W, bias, scale, shift)
    kw = dict(pivot=None, act="gelu_tanh" if epi == 0 else "none", rope=rope, rope_heads=1, seq=seq)
    return args, kw


def _fold_ref(xs, args, kw):
    """fp64: Linear(LN(x) (1 + scale) + shift) (+ GELU / RoPE of the first head of q and k) from the STORED stream rows"""
    epi, _, _, _, _, _, W, bias, scale, shift = args
    M, N = xs.shape[0], W.shape[0]
    mean, var = xs.double().mean(dim=1), xs.double().var(dim=1, unbiased=False)
    h = (xs.double() - mean[:, None]) / torch.sqrt(var + 1e-6)[:, None] * (1 + scale.double()) + shift.double()
    ref = h @ W.double().t() + bias.double()
    if epi == 0:
        return 0.5 * ref * (1 + torch.tanh(0.7978845608028654 * (ref + 0.044715 * ref ** 3)))
    inner, seq = N // 3, kw["seq"]
    cs = kw["rope"].double()[torch.arange(M) % seq].reshape(M, 32, 2)
    r = ref.clone()
    for part in (0, 1):
        c0 = part * inner
        blk = ref[:, c0: c0 + 64].reshape(M, 32, 2)
        r[:, c0: c0 + 64] = torch.stack([blk[..., 0] * cs[..., 0] - blk[..., 1] * cs[..., 1], blk[..., 1] * cs[..., 0] + blk[..., 0] * cs[..., 1]],
                                        dim=-1).reshape(M, 64)
    return r


@pytest.mark.parametrize("N,epi", [(1536, 4), (1024, 0)], ids=["qkv_rope", "ff1_gelu"])
def test_fold_site_on_tall_tiles(N, epi):
    """(c) the LayerNorm fold's consumers on 256-row tiles (M = 16 384, D = 1024: 64 x 6 / 64 x 4 tall tiles): c1 and c2 per lane feature, (mean,
    rstd) per lane token, the accumulator starts from 0; epi 4 with rope_heads 1, epi 0 with GELU.  Stream, statistics and output bit for bit
    against the 8-wave kernel, the output against fp64."""
    import gpu_helpers as G
    args, kw = _fold_problem(N, epi, N + epi)
    new, old = _both(lambda: G.op_ln_fold(*args, **kw))
    err = rel_l2(new[2], _fold_ref(new[0], args, kw))
    print(f"fold site N={N} epi={epi}: rel-L2 {err:.2e}")
    assert err < 3e-3  # bf16 output rounding + fp16 rounding of the folded weights
    for a, c in zip(new, old):
        assert torch.isfinite(a).all() and torch.equal(a, c)


# ----------------------------------------------------------------------------- (e) fp16 precision mode: the EL = f16_t builds of the same kernel
def test_fp16_mode_store_gelu():
    """The store case of (a) in the fp16 precision mode: saturating fp16 pack, element-wise bound of the fp16 op tests, bit-equal to the 8-wave kernel."""
    import test_gpu_fp16_ops as H
    run, ref, scale = H._fused_case("store", 22528, 768, 256, 0, 22528 + 7 * 768 + 256)
    new, old = _both(run)
    H.check_f16("w4 whole-line store fp16", new, ref, scale)
    assert torch.equal(new, old)


def test_fp16_mode_fold_site():
    """The FF1 fold site of (c) in the fp16 precision mode: bit-equal to the 8-wave kernel, and inside the store epilogues' fp64 tolerance (the fp16
    output rounds finer than bf16)."""
    import test_gpu_fp16_ops as H
    args, kw = _fold_problem(1024, 0, 1024 + 16)
    new, old = _both(lambda: H.op_ln_fold_p(H.P_FP16, *args, **kw))
    err = rel_l2(new[2], _fold_ref(new[0], args, kw))
    print(f"fold site fp16 mode: rel-L2 {err:.2e}")
    assert err < 3e-3
    for a, c in zip(new, old):
        assert torch.isfinite(a).all() and torch.equal(a, c)
