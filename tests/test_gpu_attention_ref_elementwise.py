"""The reference attention kernel (csrc/attention.hip: attn_ref_kernel) per element against fp64, in fp32 -- the only attention kernel of the
fp32 mode, the on-device oracle of the full-size tests -- and in bf16:

    |out - ref| <= 1 ulp(ref) of the stored type + 8 fp32 ulps of mag          on every element of every compared query row
        mag    pv (1 + 2 max_k sum_d |q_d k_d| scale), pv = sum_k p_k |v_k|     (gpu_helpers.attn_ref_terms)
The kernel keeps its numerators in fp32, so the numerator-rounding term of the flash kernels' bound does not appear.  The fp16 instantiation
is held to the same form in test_gpu_fp16_ops.py.  tests/test_tile_kernel_bound_host.py asserts on the CPU that the kernel's arithmetic,
restated in float32, meets this bound and that a leaked padding key of the last partial tile does not.

Cases: N in {1, 63, 64, 65, 127, 128, 129, 200} (one to four 64-key tiles, ragged and whole last tiles), H in {1, 3}, B = 2 with a length
mask on one item; a mask with holes whose first whole 64-key tile is masked (the running maximum stays -inf through a tile); every key counted
once (q = 0, one-hot values: count / n_valid); the pre-scaled form (f5_op_attention_prescaled, kernel 0, bf16) against the base-2 reference.

Measured on MI355X (worst share of the bound): fp32 0.072, every key counted once 0.065; bf16 0.498, counted once 0.488, pre-scaled 0.497
(the bf16 figures are the one rounding of the stored element).  No case exceeded the bound: no defect found.  The module runs in about 1 s."""
import functools

import pytest
import torch

import gpu_helpers as G
from gpu_helpers import P_BF16, P_FP32

pytestmark = pytest.mark.gpu
PRECISIONS = [P_FP32, P_BF16]
PREC_IDS = ["fp32", "bf16"]
SWEEP_N = (1, 63, 64, 65, 127, 128, 129, 200)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()
    yield
    for k in sorted(WORST):
        print(f"\n  worst share of the bound, attn_ref_kernel {k}: {WORST[k]:.3f}", end="")
    print()


def _check(key, name, out, terms, rows, precision):
    ref, mag, _ = terms
    assert torch.isfinite(out).all(), name
    v = slice(None) if rows is None else rows
    w = G.check_elementwise(name, out[v], ref[v], mag[v], precision)
    WORST[key] = max(WORST.get(key, 0.0), w)


def key_mask(kind, N):
    """-> (key mask [2, N] or None, the query rows to compare).  lens: (N, max(1, N - 13)), the rows inside each length; holes (N > 64): item 0
    without its whole first 64-key tile and without keys 70 and 71, item 1 with exactly one valid key -- the mask hides keys, every query row
    is computed and compared."""
    if kind == "none":
        return None, None
    if kind == "lens":
        mask = torch.arange(N)[None, :] < torch.tensor([N, max(1, N - 13)])[:, None]
        return mask, mask
    assert kind == "holes" and N > 64
    mask = torch.ones(2, N, dtype=torch.bool)
    mask[0, :64] = False
    mask[0, 70:72] = False
    mask[1] = False
    mask[1, 3 * (N - 1) // 4] = True
    return mask, None


@functools.lru_cache(maxsize=None)
def _case(N, H, precision, mask_kind, prescaled=False):
    """randn * 1.5 in the mode's type (fp32: as drawn); shared by the tests, nobody modifies it"""
    g = torch.Generator().manual_seed(10 * N + H)
    qkv = torch.randn(2, N, 3, H, 64, generator=g) * 1.5
    if precision == P_BF16:
        qkv = G.bf16_round(qkv)
    if prescaled:
        qkv[:, :, 0] = G.bf16_round(qkv[:, :, 0] * G.QSCALE)
    mask, rows = key_mask(mask_kind, N)
    return qkv, mask, rows, G.attn_ref_terms(qkv, mask, precision, base2=prescaled)


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("H", [1, 3])
def test_small_shapes_with_a_length_mask(H, precision):
    for N in SWEEP_N:
        qkv, mask, rows, terms = _case(N, H, precision, "lens")
        _check(G.PREC_NAMES[precision], f"attn_ref_kernel {G.PREC_NAMES[precision]} N={N} H={H} lens", G.op_attention(precision, 0, qkv, mask), terms, rows, precision)


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
def test_first_key_tile_masked_out(precision):
    """The whole first 64-key tile of item 0 is masked: m_i stays -inf through it (alpha = 0, every numerator 0) and the first valid tile must
    start the row sum from nothing.  Item 1 has one valid key: every output row is that key's value row."""
    for N in (65, 129, 200):
        qkv, mask, rows, terms = _case(N, 3, precision, "holes")
        out = G.op_attention(precision, 0, qkv, mask)
        _check(G.PREC_NAMES[precision], f"attn_ref_kernel {G.PREC_NAMES[precision]} N={N} holes", out, terms, rows, precision)
        only = qkv[1, 3 * (N - 1) // 4, 2].reshape(-1)
        assert torch.equal(out[1], only[None, :].expand(N, -1)), N


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("mask_kind", ["none", "lens", "holes"])
def test_every_key_counted_once(mask_kind, precision):
    """q = 0: every numerator is expf(0) = 1.  V[k, d] = (d == k % 64): out[q, d] = count_d / n_valid over the valid keys, from exact fp32
    integer sums.  A key dropped, counted twice or leaked moves a column by at least 1 / (n_valid + 1) of its value.  Bit equality where
    n_valid is a power of two (1 / l is exact)."""
    B, H = 2, 2
    for N in (64, 65, 129, 192, 257):
        if mask_kind == "holes" and N <= 64:
            continue  # (no tile to mask out whole)
        mask, rows = key_mask(mask_kind, N)
        qkv = torch.zeros(B, N, 3, H, 64)
        qkv[:, torch.arange(N), 2, :, torch.arange(N) % 64] = 1.0
        out = G.op_attention(precision, 0, qkv, mask)
        terms = G.attn_ref_terms(qkv, mask, precision)
        _check(G.PREC_NAMES[precision] + " counted once", f"counted once {G.PREC_NAMES[precision]} N={N} {mask_kind}", out, terms, rows, precision)
        valid = torch.ones(B, N, dtype=torch.bool) if mask is None else mask
        for b in range(B):
            n_valid = int(valid[b].sum())
            count = torch.bincount(torch.arange(N)[valid[b]] % 64, minlength=64).double()
            exact = (count / n_valid)[None, None, :].expand(N, H, 64)
            got = out[b].view(N, H, 64)
            got, exact = (got, exact) if rows is None else (got[rows[b]], exact[rows[b]])
            assert (got[exact == 0] == 0).all(), (N, b)  # a column none of the valid keys feeds
            if n_valid & (n_valid - 1) == 0:
                assert torch.equal(got.double(), G.round_to(precision, exact).double()), (N, b)


@pytest.mark.parametrize("mask_kind", ["none", "lens"])
def test_prescaled_form(mask_kind):
    """f5_op_attention_prescaled with kernel 0 (bf16): q carries softmax_scale * log2(e), the kernel multiplies the scores by ln 2."""
    for N in (63, 65, 128, 200):
        qkv, mask, rows, terms = _case(N, 3, P_BF16, mask_kind, True)
        _check("bf16 pre-scaled", f"attn_ref_kernel bf16 pre-scaled N={N} {mask_kind}", G.op_attention_prescaled(0, qkv, mask), terms, rows, P_BF16)
