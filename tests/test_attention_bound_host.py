"""The element-wise bound of the bf16 attention tests, tested on the CPU (no GPU needed): tests/test_gpu_attention_bf16_elementwise.py holds
every bf16 flash kernel to
    |out - ref| <= 1 bf16 ulp(ref) + 8 fp32 ulps of mag + 2^-8 pv        (gpu_helpers.attn_ref_terms, gpu_helpers.check_elementwise)
per element, and to a mean signed relative error |m| <= 2^-12.  A bound proves something only if correct arithmetic meets it and defective
arithmetic does not.  gpu_helpers.attn_emulate_bf16 restates the kernels' arithmetic on the CPU (fp32 scores, exp2 against a reference, the
row sum from the unrounded numerators, the numerators rounded once to bf16 for the PV product, one bf16 rounding of the output) together
with four defects; this module asserts, on the shapes and inputs the device tests use,
  * `rne` (the documented arithmetic) lies within the bound;
  * a key dropped (`drop_last_valid_key`) or leaked (`leak_first_masked_key`) exceeds it;
  * the bias statistic separates rounding from truncation with a factor 4 to spare on either side of the device test's 2^-12:
    |m| <= 2^-14 for `rne`, |m| >= 2^-10 for `trunc_p` and `trunc_out` -- so the device test can neither pass vacuously nor fail on correct
    arithmetic.

Measured on the CPU (torch 2.x, fp32 matmul and exp2 of the host):
    worst share of the bound, (B, N, H, masked)      rne     drop_last_valid_key   leak_first_masked_key
        (2, 33, 2, T)                                0.481   181 x                 913 x
        (1, 65, 2, F)                                0.464   311 x                 83 x
        (2, 200, 3, T)                               0.476   193 x                 142 x
        (1, 257, 2, F)                               0.496   64 x                  55 x
        (2, 1024, 2, T)                              0.414   82 x                  204 x
    mean signed relative error m                     rne        trunc_p     trunc_out
        (2, 200, 3, T)                               -1.81e-05  -2.56e-03   -2.61e-03
        (1, 1024, 2, F)                              -9.15e-06  -2.66e-03   -2.43e-03
(truncating the numerators alone stays INSIDE the element-wise bound -- at most 0.79 of it on these shapes, truncating the outputs alone
0.72 -- which is why the bias statistic exists.)"""
import functools

import pytest
import torch

import gpu_helpers as G

SHAPES = [(2, 33, 2, True), (1, 65, 2, False), (2, 200, 3, True), (1, 257, 2, False), (2, 1024, 2, True)]
BIAS_SHAPES = [(2, 200, 3, True), (1, 1024, 2, False)]


@functools.lru_cache(maxsize=None)
def _case(B, N, H, masked, positive_v=False):
    qkv, mask = G.attn_randn_case(B, N, H, masked, positive_v=positive_v)
    return qkv, mask, G.attn_ref_terms(qkv, mask, G.P_BF16)


def _share(shape, variant):
    qkv, mask, (ref, mag, extra) = _case(*shape)
    out = G.attn_emulate_bf16(qkv, mask, variant)
    valid = slice(None) if mask is None else mask
    err = (out.double() - ref).abs()[valid]
    bound = (G.bf16_ulp(ref) + G.F32_ULPS * mag.abs() + extra)[valid]
    return out, float((err / bound).max())


@pytest.mark.parametrize("shape", SHAPES)
def test_documented_arithmetic_lies_within_the_bound(shape):
    qkv, mask, (ref, mag, extra) = _case(*shape)
    out, share = _share(shape, "rne")
    print(f"  {shape} rne: {share:.3f} of the bound; trunc_p {_share(shape, 'trunc_p')[1]:.3f}, trunc_out {_share(shape, 'trunc_out')[1]:.3f}")
    valid = slice(None) if mask is None else mask
    G.check_elementwise(f"rne {shape}", out[valid], ref[valid], mag[valid], G.P_BF16, extra[valid])


def test_documented_arithmetic_with_prescaled_q_lies_within_the_bound():
    """the pre-scaled form (q times QSCALE rounded to bf16, scores in log2 units, base2 terms) on (2, 200, 3, T): measured 0.456 of the bound"""
    qkv, mask, _ = _case(2, 200, 3, True)
    qs = qkv.clone()
    qs[:, :, 0] = G.bf16_round(qkv[:, :, 0] * G.QSCALE)
    ref, mag, extra = G.attn_ref_terms(qs, mask, G.P_BF16, base2=True)
    out = G.attn_emulate_bf16(qs, mask, "rne", base2=True)
    G.check_elementwise("rne, pre-scaled q", out[mask], ref[mask], mag[mask], G.P_BF16, extra[mask])


@pytest.mark.parametrize("variant", ["drop_last_valid_key", "leak_first_masked_key"])
@pytest.mark.parametrize("shape", SHAPES)
def test_a_dropped_or_leaked_key_exceeds_the_bound(shape, variant):
    qkv, mask, (ref, mag, extra) = _case(*shape)
    out, share = _share(shape, variant)
    print(f"  {shape} {variant}: {share:.1f} x the bound")
    assert share > 1.0
    valid = slice(None) if mask is None else mask
    with pytest.raises(AssertionError, match="out of bound"):
        G.check_elementwise(f"{variant} {shape}", out[valid], ref[valid], mag[valid], G.P_BF16, extra[valid])


@pytest.mark.parametrize("shape", BIAS_SHAPES)
def test_bias_statistic_separates_rounding_from_truncation(shape):
    """V = bf16(|V| + 0.5): every output is at least 0.5 and pv = ref, so (out - ref) / ref is a relative error of the rounding steps alone."""
    qkv, mask, (ref, mag, extra) = _case(*shape, positive_v=True)
    assert float(ref.min()) >= 0.5 and torch.equal(ref * 2.0 ** -8, extra)
    valid = slice(None) if mask is None else mask
    m = {v: G.mean_signed_error(G.attn_emulate_bf16(qkv, mask, v), ref, valid) for v in ("rne", "trunc_p", "trunc_out")}
    print(f"  {shape}: m = " + ", ".join(f"{k} {v:+.2e}" for k, v in m.items()))
    assert abs(m["rne"]) <= 2.0 ** -14
    assert m["trunc_p"] <= -(2.0 ** -10) and m["trunc_out"] <= -(2.0 ** -10)
