"""The check of tests/test_gpu_text_embed.py, tested on the CPU (no GPU needed).  That module holds compute_text_embed (csrc/eval_common.hip:
token gather, position table, filler mask, up to four ConvNeXt-V2 blocks) to a bound PER TOKEN ROW:
    e[b, p] = max_c |X - R| / max_c |R[b, p, :]|  <=  TEXT_MARGIN x max over rows of e(E_p)      (gpu_helpers.check_text_rows)
with R the oracle's text embedding evaluated in float64 and E_p the float32 restatement of the kernel chain with the mode's storage roundings
(gpu_helpers.text_emulate), and to exact zeros on the rows R zeroes.  A check proves something only if correct arithmetic meets it and
defective arithmetic does not.  This module asserts, on the cases of the device test (gpu_helpers.TEXT_CASES),
  (a) the restatement lies within its own bound (trivially) and is exactly zero where R is, in bf16, fp16 and fp32;
  (b) each planted defect of gpu_helpers.TEXT_DEFECTS is rejected -- a row out of bound or a non-zero element on a zeroed row -- on at least
      one row of at least one case, and prints the defect's whole-tensor rel-L2 beside it: the figure the 1.5e-2 stage taps of the model tests
      see;
  (c) the id clamp as a pure function: ids {-5, -1, 0, vocab - 1, vocab, vocab + 7} give the bits of the clamped ids.
Every test prints its figures (the restatement's worst row error per precision and case, the margin in force, per defect the worst row's share of
the bound and the rel-L2).

Measured on the CPU (torch 2.x, fp32 matmul / erf / rsqrt of the host):
    restatement's worst row e(E_p)       bf16 4.1e-3 .. 4.9e-3, fp16 4.6e-4 .. 6.2e-4, fp32 2.5e-7 .. 6.2e-7 (text blocks); 5e-8 .. 7e-8 (MMDiT: one
                                         fp32 add); 0 (the gather alone).  On the device the kernels sit at 0.23 .. 0.27 (16-bit) and 0.33 .. 0.60
                                         (fp32) of the bound: they need a margin of 1.1 (16-bit) to 2.4 (fp32: another accumulation order).
    a defect's worst row / the bound, strongest case (its whole-tensor rel-L2); "zeros": caught by the exact-zero check
                                         bf16            fp16            fp32
        last_token_gathers_filler        4.6e6 x on the MMDiT cases in every mode (rel-L2 3.6e-2); unbounded on the gather alone (bound 0)
        position_off_by_one              1.5e6 x (1.4e-1), the MMDiT cases; 12 (bf16) .. 2.7e5 x (fp32) on the text-block cases
        mask_after_drop_text             52 .. 67 x      458 .. 608 x    4.2e5 .. 1.2e6 x  (text blocks; MMDiT 4e6 x; rel-L2 1: every row zeroed)
        conv_across_batch                47 x            427 x           7.8e5 x         (4.5e-1 at 2 x 5; 8e-2 at 3 x 77)
        grn_over_flattened_batch         1.9 x           15 x            2.8e4 x         (8e-3 .. 2.2e-2: the one defect whose rel-L2 can pass 1.5e-2)
        no_mask_after_last_block         zeros           zeros           zeros           (rel-L2 1.6e-1; the non-zero rows are untouched)
        position_wraps                   2.8e6 x in every mode, the MMDiT cases alone (rel-L2 3.7e-2 .. 5.6e-2)
    The margin is bounded from above by the bf16 GRN defect: 4 x 1.9 = 7.5; from below by the kernels: 2.4.  4 is what the check uses."""
import pytest
import torch

import gpu_helpers as G
from gpu_helpers import P_BF16, P_FP16, P_FP32

PRECISIONS = [P_BF16, P_FP16, P_FP32]
PREC_IDS = [G.PREC_NAMES[p] for p in PRECISIONS]
DEFECTS = [d for d in G.TEXT_DEFECTS if d != "none"]


def _rel_l2(X, R):
    return float((X.double() - R.double()).norm() / R.double().norm().clamp(min=1e-300))


def _verdict(X, R, E):
    """(worst row's share of the bound, non-zero elements on zeroed rows) of X under the check of gpu_helpers.check_text_rows"""
    eE, _ = G.text_row_errors(E, R)
    eX, zero = G.text_row_errors(X, R)
    bound = G.TEXT_MARGIN * float(eE.max())
    worst = float(eX.max())
    return (worst / bound if bound > 0 else (0.0 if worst == 0 else float("inf"))), int((X[zero] != 0).sum())


# ----------------------------------------------------------------------------- a. the restatement
@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("cid", list(G.TEXT_CASES))
def test_restated_text_path_meets_the_row_check(cid, precision):
    c = G.text_case(cid)
    for drop in (False, True):
        R, E = G.text_case_terms(cid, precision, drop)
        assert R.dtype == torch.float64 and E.dtype == torch.float32 and R.shape == E.shape
        G.check_text_rows(f"restated {cid} {G.PREC_NAMES[precision]} drop_text={drop}", E, R, E)
        e, zero = G.text_row_errors(E, R)
        # the stored type's own rounding is the order of the restatement's error: an fp32 chain of at most 4 blocks stays below 1e-5 of a
        # row's largest element, a 16-bit one below a few ulps of the type (2^-8 bf16, 2^-11 fp16) per block
        cap = {P_FP32: 1e-5, P_FP16: 4 * 4 * 2.0 ** -11, P_BF16: 4 * 4 * 2.0 ** -8}[precision]
        assert float(e.max()) < cap, (cid, precision, drop, float(e.max()))
        mp = c["arch"].get("text_mask_padding", True) and (c["mmdit"] or c["arch"].get("conv_layers", 0) > 0)
        filler = torch.zeros(R.shape[:2], dtype=torch.bool)
        n = min(c["text"].shape[1], R.shape[1])
        filler[:, :n] = c["text"][:, :n] == -1
        filler[:, n:] = True
        assert torch.equal(zero, filler if mp else torch.zeros_like(filler)), "the rows the reference zeroes are the filler rows under text_mask_padding"
    if c["backbone"] == "unett":  # the gather alone: equality with the table rows is exact
        R, E = G.text_case_terms(cid, precision, False)
        assert torch.equal(E.double(), R)


# ----------------------------------------------------------------------------- b. the planted defects
@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("defect", DEFECTS)
def test_a_planted_text_defect_is_rejected(defect, precision):
    caught = []
    for cid in G.TEXT_CASES:
        c = G.text_case(cid)
        for drop in (False, True):
            R, E = G.text_case_terms(cid, precision, drop)
            X = G.text_emulate(precision, c["W"], c["arch"], c["text"], c["N"], drop, c["mmdit"], defect=defect)
            if torch.equal(X, E):
                continue  # the defect does not reach this case
            share, nz = _verdict(X, R, E)
            hit = share > 1.0 or nz > 0
            print(f"  {defect} {G.PREC_NAMES[precision]} {cid} drop_text={drop}: worst row {share:.3g} x the bound, {nz} non-zero elements on zeroed rows, "
                  f"whole-tensor rel-L2 {_rel_l2(X, R):.3e} (restatement {_rel_l2(E, R):.3e}) -> {'rejected' if hit else 'passes'}")
            if hit:
                caught.append((cid, drop))
                with pytest.raises(AssertionError, match="out of bound|rows the reference zeroes"):
                    G.check_text_rows(defect, X, R, E)
    assert caught, f"{defect}: no case rejects it"


# ----------------------------------------------------------------------------- c. the id clamp
@pytest.mark.parametrize("cid", ["td512_c4_mask_3x77", "mmdit128_mask_nt1030"])
def test_out_of_table_ids_equal_the_clamped_ids(cid):
    c = G.text_case(cid)
    V = G.TEXT_V
    wild = c["text"].clone()
    vals = torch.tensor([-5, -1, 0, V - 1, V, V + 7])
    wild[0, 3:3 + len(vals)] = vals
    wild[1, 10:10 + len(vals)] = vals.flip(0)
    tame = G.text_clamp_ids(wild, V)
    assert tame.min() == -1 and tame.max() == V - 1 and not torch.equal(tame, wild)
    assert tame[0, 3:9].tolist() == [-1, -1, 0, V - 1, V - 1, V - 1]
    for drop in (False, True):
        a = G.text_emulate(P_BF16, c["W"], c["arch"], wild, c["N"], drop, c["mmdit"])
        b = G.text_emulate(P_BF16, c["W"], c["arch"], tame, c["N"], drop, c["mmdit"])
        assert torch.equal(a, b)
        if c["arch"]["text_mask_padding"]:
            assert (a[0, 3:5] == 0).all() and (a[0, 5:9] != 0).any(dim=-1).all()  # -5 is a filler row like -1
