"""The checks of tests/test_gpu_tile_kernel.py and tests/test_gpu_attention_ref_elementwise.py, tested on the CPU (no GPU needed).  Those
modules hold gemm_tile_kernel and attn_ref_kernel to bit equality on exact inputs and, on random real data, to
    |out - ref| <= 1 ulp(ref) of the stored type + 8 fp32 ulps of the magnitude sum        (gpu_helpers.check_elementwise)
per element.  A check proves something only if correct arithmetic meets it and defective arithmetic does not.  gpu_helpers.tile_emulate and
gpu_helpers.attn_emulate_ref restate the two kernels' arithmetic in float32 on the CPU; this module asserts, on shapes and inputs of the
device tests,
  (a) the restatement is bit-equal on the exact inputs and within the bound on the real ones, in bf16, fp16 and fp32;
  (b) each planted defect -- the last 32-wide K chunk dropped, a tail column taking its neighbour's bias, the gate of batch item b - 1 on the
      rows of a straddling tile, a RoPE pair swapped, a_row_mod ignored, a key of the last partial attention tile leaked -- breaks bit
      equality on the exact inputs AND exceeds the bound on the real ones.

Measured on the CPU (torch 2.x, fp32 matmul and exp of the host):
    share of the bound, restatement      tile kernel: bf16 0.500, fp16 0.499 (the one rounding of the stored element), fp32 0.134 .. 0.186 (an fp32
                                         output of a 16-bit mode: 0.06 .. 0.22); attention: fp32 0.042 .. 0.065, bf16 0.498
    factor by which a defect misses the bound on real inputs, worst element / median of the elements it touches; on the exact inputs the
    number of touched elements whose bits differ
                                         bf16                fp16                fp32                exact inputs
        drop_last_k_chunk (K = 704)      2.7e4 / 26          3.2e4 / 201         5.2e4 / 8.1e3       8550 of 9100
        tail_column_neighbour_bias       2.7e4 / 885         1.7e5 / 7.0e3       9.8e5 / 7.2e5       130 of 130
        gate_of_previous_batch           6.6e5 / 259         5.3e6 / 2.0e3       1.5e9 / 2.4e5       3723 of 4410
        rope_pair_swapped                2.8e5 / 255         5.2e5 / 2.0e3       1.2e6 / 1.5e5       6470 of 8320
        a_row_mod_ignored                5.0e5 / 55          5.0e5 / 435         5.0e5 / 8.5e4       4345 of 4550
        (untouched-but-equal elements: the planted value happens to coincide, e.g. two equal gates)
    a leaked padding key, real inputs / every key counted once
        fp32   N = 63: 283 / 1.5e4    65: 290 / 1.5e4    129: 75 / 7.6e3    200: 52 / 4.9e3
        bf16   N = 63: 2.7 / 2.0      65: 2.6 / 4.1      129: 1.05 / 2.0    200: 0.94 / 0.84   (one key in 201 is below one bf16 ulp: see the test)"""
import functools

import pytest
import torch

import gpu_helpers as G
from gpu_helpers import P_BF16, P_FP16, P_FP32

PRECISIONS = [P_BF16, P_FP16, P_FP32]
PREC_IDS = [G.PREC_NAMES[p] for p in PRECISIONS]


def _real_case(precision, epi, M, N, K, act="none", mod=0, nb=1):
    """random real inputs of one epilogue as test_gpu_tile_kernel.py::test_rounded draws them -> (args, kw of tile_emulate, kw of fused_ref)"""
    g, A, W, b = G.linear_problem(precision, M, N, K, seed=M + N + K)
    seq = M // nb
    kw = dict(act=act)
    if epi in ("gate", "resid"):
        kw.update(gate=torch.randn(nb, N, generator=g), rowmask=torch.rand(M, generator=g) > 0.2, rows_per_batch=seq)
    if epi == "resid":
        kw["x"] = (torch.randn(M, N, generator=g) * 3).half().float()
    if epi == "add2":
        kw["addend"] = (torch.randn(M, N, generator=g) * 3).half().float()
        if mod:
            A = A[:mod].contiguous()
            kw["a_row_mod"] = mod
    if epi == "rope":
        ang = torch.rand(seq, 32, generator=g) * 6.28
        kw.update(rope=torch.stack([ang.cos(), ang.sin()], dim=-1), rope_heads=1, seq=seq)
    return (A, W, b), kw


def _ref(epi, args, kw):
    """fp64 reference and magnitude for the keyword arguments of tile_emulate"""
    A, W, b = args
    M = (kw["x"] if "x" in kw else kw["addend"] if "addend" in kw else A).shape[0]
    rk = {k: v for k, v in kw.items() if k not in ("rows_per_batch", "a_row_mod")}
    if kw.get("gate") is not None and kw["gate"].dim() == 2:
        rk["gate"] = G.expand_gate(kw["gate"], M, kw["rows_per_batch"])
    if kw.get("a_row_mod"):
        A = A[torch.arange(M) % kw["a_row_mod"]]
    return G.fused_ref(epi.replace("store_f32", "store"), A, W, b, **rk)


def _shares(precision, epi, f16_stream, outs, ref, scale):
    """share of the bound per element, over the outputs the epilogue writes: the largest, and the tensor of the first output"""
    worst, first = 0.0, None
    for out, stored in ((outs[0], precision), (outs[1], P_FP16 if f16_stream else P_FP32)):
        if out is not None:
            r = (out.double() - ref).abs() / (G.stored_ulp(stored, ref) + G.F32_ULPS * scale.abs())
            worst, first = max(worst, float(r.max())), (r if first is None else first)
    return worst, first


REAL = [("store", "gelu_tanh"), ("store", "gelu_erf"), ("store", "mish"), ("store_f32", "gelu_erf"), ("gate", "gelu_tanh"), ("resid", "none"),
        ("add2", "none"), ("rope", "none")]


# ----------------------------------------------------------------------------- a. the restatement meets the checks
@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi,act", REAL, ids=[f"{e}_{a}" for e, a in REAL])
def test_restated_tile_arithmetic_lies_within_the_bound(epi, act, precision):
    for M, N, K in [(130, 70, 704), (63, 62, 32)]:
        N = 192 if epi == "rope" else N
        even = M % 2 == 0
        args, kw = _real_case(precision, epi, M, N, K, act, mod=M // 2 if even else 0, nb=2 if even else 1)
        ref, scale = _ref(epi, args, kw)
        for f16_stream in ([False, True] if epi in ("resid", "add2") else [False]):
            outs = G.tile_emulate(precision, epi, *args, f16_stream=f16_stream, **kw)
            for name, out, stored in (("out_t", outs[0], precision), ("out_f", outs[1], P_FP16 if f16_stream else P_FP32)):
                if out is not None:
                    G.check_elementwise(f"restated {epi} {act} {G.PREC_NAMES[precision]} {(M, N, K)} f16_stream={f16_stream} {name}", out, ref, scale, stored)


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
def test_restated_tile_arithmetic_is_bit_equal_on_exact_inputs(precision):
    for epi, f16_stream in [("store", False), ("gate", False), ("resid", False), ("resid", True), ("add2", False), ("add2", True), ("rope", False)]:
        M, N, K = 130, (192 if epi == "rope" else 70), 704
        args, kw = G.exact_case(epi, M, N, K, 65, 1, True, seed=M + N + K, gate_batches=2 if epi in ("gate", "resid") else 0,
                                a_rows=65 if epi == "add2" else None)
        kw.update(rows_per_batch=65) if "gate" in kw else None
        kw.update(a_row_mod=65) if epi == "add2" else None
        ref, _ = _ref(epi, args, kw)
        outs = G.tile_emulate(precision, epi, *args, f16_stream=f16_stream, **kw)
        want = G.tile_stored(precision, epi, f16_stream, ref)
        for o, w in zip(outs, want):
            assert (o is None and w is None) or torch.equal(o, w), (epi, f16_stream)


@functools.lru_cache(maxsize=None)
def _attn_case(N, H, precision, prescaled=False):
    g = torch.Generator().manual_seed(N + H)
    qkv = G.bf16_round(torch.randn(2, N, 3, H, 64, generator=g) * 1.5) if precision == P_BF16 else torch.randn(2, N, 3, H, 64, generator=g) * 1.5
    if prescaled:
        qkv[:, :, 0] = G.bf16_round(qkv[:, :, 0] * G.QSCALE)
    mask = torch.arange(N)[None, :] < torch.tensor([N, max(1, N - 13)])[:, None]
    return qkv, mask, G.attn_ref_terms(qkv, mask, precision, base2=prescaled)


@pytest.mark.parametrize("precision", [P_FP32, P_BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [63, 65, 129, 200])
def test_restated_attention_arithmetic_lies_within_the_bound(N, precision):
    qkv, mask, (ref, mag, _) = _attn_case(N, 3, precision)
    out = G.attn_emulate_ref(qkv, mask, precision)
    G.check_elementwise(f"restated attn_ref_kernel {G.PREC_NAMES[precision]} N={N}", out[mask], ref[mask], mag[mask], precision)
    if precision == P_BF16:
        qkv, mask, (ref, mag, _) = _attn_case(N, 3, precision, True)
        out = G.attn_emulate_ref(qkv, mask, precision, base2=True)
        G.check_elementwise(f"restated attn_ref_kernel bf16 pre-scaled N={N}", out[mask], ref[mask], mag[mask], precision)


# ----------------------------------------------------------------------------- b. the planted defects do not
# defect -> (epilogue, (M, N, K), batches of the gate, a_row_mod, the elements the defect touches: a function of (M, N) -> bool [M, N])
def _rows(lo, hi):
    return lambda M, N: ((torch.arange(M) >= lo) & (torch.arange(M) < hi))[:, None].expand(M, N)


DEFECTS = {
    "drop_last_k_chunk": ("store", (130, 70, 704), 1, 0, lambda M, N: torch.ones(M, N, dtype=torch.bool)),
    "tail_column_neighbour_bias": ("store", (130, 70, 64), 1, 0, lambda M, N: (torch.arange(N) == N - 1)[None, :].expand(M, N)),
    "gate_of_previous_batch": ("gate", (129, 70, 64), 3, 0, lambda M, N: _rows(43, 64)(M, N) | _rows(86, 128)(M, N)),
    "rope_pair_swapped": ("rope", (65, 192, 64), 1, 0, lambda M, N: (torch.arange(N) < 128)[None, :].expand(M, N)),
    "a_row_mod_ignored": ("add2", (130, 70, 64), 1, 65, _rows(65, 130)),
}


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_a_planted_tile_defect_fails_both_checks(defect, precision):
    epi, (M, N, K), nb, mod, touched = DEFECTS[defect]
    hit = touched(M, N)
    # exact inputs: bit equality breaks, and only where the defect reaches
    args, kw = G.exact_case(epi, M, N, K, M // nb, 1, False, seed=M + N + K, gate_batches=nb if nb > 1 else 0, a_rows=mod or None)
    kw.update(rows_per_batch=M // nb) if "gate" in kw else None
    kw.update(a_row_mod=mod) if mod else None
    ref, _ = _ref(epi, args, kw)
    want = G.tile_stored(precision, epi, False, ref)[0]
    assert torch.equal(G.tile_emulate(precision, epi, *args, **kw)[0], want)
    bad = G.tile_emulate(precision, epi, *args, defect=defect, **kw)[0] != want
    assert bad.any() and not (bad & ~hit).any()
    # real inputs: the bound is exceeded
    args, kw = _real_case(precision, epi, M, N, K, "none", mod=mod, nb=nb)
    kw.pop("rowmask", None)
    ref, scale = _ref(epi, args, kw)
    ok, _ = _shares(precision, epi, False, G.tile_emulate(precision, epi, *args, **kw), ref, scale)
    worst, r = _shares(precision, epi, False, G.tile_emulate(precision, epi, *args, defect=defect, **kw), ref, scale)
    print(f"  {defect} {G.PREC_NAMES[precision]}: exact inputs {int(bad.sum())} of {int(hit.sum())} touched elements differ; real inputs "
          f"{worst:.3g} x the bound at worst, {float(r[hit].median()):.3g} x in the median of the touched elements (restatement: {ok:.3f})")
    assert ok <= 1.0 and worst > 1.0
    with pytest.raises(AssertionError, match="out of bound"):
        G.check_elementwise(defect, G.tile_emulate(precision, epi, *args, defect=defect, **kw)[0], ref, scale, precision)


@pytest.mark.parametrize("precision", [P_FP32, P_BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [63, 65, 129, 200])
def test_a_leaked_padding_key_fails_both_checks(N, precision):
    """real inputs: the element-wise bound; exact inputs: the every-key-counted-once construction (q = 0, one-hot values: count / n_valid)"""
    qkv, mask, (ref, mag, _) = _attn_case(N, 3, precision)
    out = G.attn_emulate_ref(qkv, mask, precision, leak_padding_key=True)
    share = float(((out.double() - ref).abs() / (G.stored_ulp(precision, ref) + G.F32_ULPS * mag))[mask].max())
    once = torch.zeros(2, N, 3, 2, 64)
    once[:, torch.arange(N), 2, :, torch.arange(N) % 64] = 1.0
    t = G.attn_ref_terms(once, None, precision)
    good, leak = G.attn_emulate_ref(once, None, precision), G.attn_emulate_ref(once, None, precision, leak_padding_key=True)
    counted = float(((leak.double() - t[0]).abs() / (G.stored_ulp(precision, t[0]) + G.F32_ULPS * t[1])).max())
    print(f"  leaked padding key {G.PREC_NAMES[precision]} N={N}: {share:.3g} x the bound on real inputs, {counted:.3g} x on the counted-once inputs")
    G.check_elementwise("counted once, restated", good, t[0], t[1], precision)
    # One leaked zero key moves an output by about 1 / (n_valid + 1) of its value: far outside the fp32 bound at every N, but below one bf16
    # ulp (2^-8 .. 2^-7 of the value) from N = 200 on.  The bf16 build is the same template as the fp32 one, conversions apart, so the fp32
    # check is what holds the shared tile bookkeeping at every N; the bf16 check adds the short sequences.
    if precision == P_FP32:
        assert share > 1.0 and counted > 1.0
    else:
        assert counted > 1.0 or N > 129
        assert share > 1.0 or N > 65
