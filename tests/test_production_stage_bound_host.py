"""The check of tests/test_gpu_production_stages.py, tested on the CPU (no GPU needed).  That module holds every probed stage of the production-mode
DiT evaluation (fp16 stream, in-place residual epilogues, LayerNorm fold, pre-scaled q; include/f5hip.h: f5_plan_set_probe) to a bound PER ROW:
    e[r] = max_c |X - R| / max_c |R[r, :]|  <=  STAGE_MARGIN x max over the sampled rows of e(E)      (gpu_helpers.stage_shares)
with R the fp64 restatement of that ONE stage from the probe of the stage before it and E the float32 restatement with the kernel's roundings
(gpu_helpers.stage_emulate) from the same inputs; q | k | v are judged apart, statistics as (mean error / the row's deviation, relative rstd
error).  A second figure per row is held to the restatement's in the same way: the signed row sum |sum_c (X - R) sign(R)| / sum_c |R|
(gpu_helpers.stage_row_bias), in which roundings average out and a wrong row factor or offset -- a row's rstd or mean, a gate -- does not.  A check proves something only if correct arithmetic meets it and defective arithmetic does not.  Here the device is replaced by
gpu_helpers.stage_chain -- the whole folded evaluation restated stage after stage over all rows -- at dim 512, 8 heads, ff 1024, depth 3 (block 0
with its unfolded first LayerNorm, a fully folded block, a last block followed by the final AdaLN) on two layouts: 2 x 96 frames with a key mask
(durations 96, 67; CFG-doubled) and a ragged call of 90 and 100 frames.  It asserts
  (a) the clean chain lies within the bound at every stage, and the restatement's own error is the order of the stored type's rounding;
  (b) each planted defect of gpu_helpers.STAGE_DEFECTS is rejected -- some stage out of bound on some layout -- and prints, per defect, the stage
      that rejects it most clearly and by how much.
Every test prints its figures.

Measured on the CPU (torch 2.x, fp32 matmul of the host), bf16 mode with pre-scaled q / fp16 mode:
    restatement's worst row e(E)   n1, final_norm 2.8e-3 .. 3.7e-3 / 3.3e-4 .. 4.5e-4; qkv 3.4e-3 .. 4.3e-3 / 4.7e-4 .. 5.8e-4; ctx 3.6e-3 .. 4.4e-3 /
                                   4.4e-4 .. 5.3e-4; ff1 2.8e-3 .. 2.9e-3 / 4.9e-4 .. 5.8e-4; x_attn, x_ff 4.1e-4 .. 5.4e-4 (the fp16 stream in both
                                   modes); statistics 0.9e-7 .. 1.8e-7; vout 2.7e-3 .. 3.1e-3 / 3.6e-4.  The signed row sum (stage_row_bias) of the
                                   same stages is 10 to 20 times smaller: 2e-4 .. 3e-4 / 2.5e-5 .. 5e-5, the stream 2.5e-5 .. 4e-5.
    a defect's clearest stage, worst row / the bound at STAGE_MARGIN = 3, bf16 / fp16
        stats_quarter_row            statistics 5e5 x; the folded projections 160 .. 290 x
        stats_of_previous_site       blk1 / blk2 qkv 12 .. 16 x / 65 .. 89 x (ff1 3 .. 7 x / 15 .. 35 x) -- by the signed row sum; the first metric
                                     alone sees 1.1 .. 1.2 x in bf16: the attention branch moves a row's mean and deviation by little
        v_c1_c2_shifted_by_inner     blk1.qkv 160 x / 1 200 x
        fold_rows_of_another_time    qkv, ff1 83 .. 89 x / 460 x
        q_not_scaled                 qkv 5 600 x        q_scaled_twice  1 100 x        blk0_unscaled_weight_copy  blk0.qkv 3 700 .. 4 100 x
        gate_mlp_for_gate_msa        x_attn 69 .. 86 x in both modes
        final_pair_swapped           final_norm 66 .. 75 x / 520 .. 590 x
        rope_position_is_row_index   qkv 180 x / 1 300 x on the ragged layout; a uniform batch cannot see it (the row index IS the position)
    The margin is bounded from above by the narrowest defect, the previous site's statistics in bf16: 3 x 12 = 35 here, and 3 x 2.2 = 6.5 where the
    same defect was planted in the library itself at dim 1024; from below by the device, whose worst stage sits at 2.03 x the
    restatement's worst row (block 0's first LayerNorm in the fp16 mode: the pass normalises the fp32 sum it is about to store as fp16, the
    restatement the stored fp16 values).  3 is what the check uses."""
import pytest
import torch

import gpu_helpers as G
from gpu_helpers import P_BF16, P_FP16

ARCH = dict(dim=512, depth=3, heads=8, ff_mult=2, text_dim=64, conv_layers=0, pe_attn_head=1)
D, DEPTH, HEADS = ARCH["dim"], ARCH["depth"], ARCH["heads"]
LAYOUTS = {"masked_2x96": dict(nb=4, N=96, durations=[96, 67, 96, 67]), "ragged_90_100": dict(nb=2, N=240, frames=[90, 100])}
Q_DEFECTS = ("q_not_scaled", "q_scaled_twice", "blk0_unscaled_weight_copy")
_CACHE = {}


def _model():
    """seeded weights, the AdaLN rows of two evaluation times in the plan's layout (every block's six slots, then the final pair)"""
    if "m" not in _CACHE:
        from oracle import cpu_ref
        W = cpu_ref.random_dit_weights(ARCH, 50, seed=41)
        rows = []
        for t in (0.35, 0.8):
            emb = cpu_ref.silu(cpu_ref.timestep_embedding(W, torch.tensor([t])))
            names = [f"transformer_blocks.{i}.attn_norm.linear" for i in range(DEPTH)] + ["norm_out.linear"]
            rows.append(torch.cat([cpu_ref._lin(emb, W[n + ".weight"], W[n + ".bias"]).reshape(-1) for n in names]))
        _CACHE["m"] = (G.stage_weights(W, DEPTH), rows[0], rows[1])
    return _CACHE["m"]


def _chain(lid, precision, defect):
    key = (lid, precision, defect)
    if key not in _CACHE:
        Wst, ada, ada_other = _model()
        lay = G.stage_layout(**LAYOUTS[lid])
        g = torch.Generator().manual_seed(17)
        x_in = (torch.randn(lay["rows"], D, generator=g) * 1.2 + torch.randn(lay["rows"], 1, generator=g) * 0.4).half().float()
        probes = G.stage_chain(precision, Wst, ada, lay, x_in, precision == P_BF16, DEPTH, 1, HEADS, defect=defect, ada_other=ada_other)
        valid, _ = G.stage_sample_rows(lay)
        lines = []
        _CACHE[key] = (G.stage_shares(probes, Wst, lay, valid, precision, precision == P_BF16, DEPTH, 1, HEADS, say=lines.append), lines, probes, lay)
    return _CACHE[key]


@pytest.mark.parametrize("precision", [P_BF16, P_FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("lid", list(LAYOUTS))
def test_restated_evaluation_meets_the_stage_check(lid, precision):
    shares, lines, probes, lay = _chain(lid, precision, "none")
    print("\n".join(lines))
    G.stage_check(f"restated {lid}", shares)
    ulp = 2.0 ** -8 if precision == P_BF16 else 2.0 ** -11
    for name, (share, eE, eX) in shares.items():
        # one rounding of the stored type (half an ulp of the row's largest element) plus the operand roundings of one contraction
        cap = 1e-6 if "stats" in name else 2.0 ** -11 * 2 if name.endswith(("x_attn", "x_ff")) else 4 * ulp
        assert eE < cap, (name, eE, cap)
        assert share <= 1.0 / G.STAGE_MARGIN + 0.2, (name, share)  # (the chain IS the restatement, up to the host matmul's blocking)
    pad = (~lay["key"]) & (lay["seg"] >= 0)
    if pad.any():  # a padded query row keeps its bits through the out-projection
        assert torch.equal(probes["blk1.x_attn"][pad], probes["blk0.x_ff"][pad])


# (the fp16 mode never pre-scales q: the three q defects have no place to sit there)
PLANTED = [(d, p) for d in G.STAGE_DEFECTS if d != "none" for p in (P_BF16, P_FP16) if not (p == P_FP16 and d in Q_DEFECTS)]


@pytest.mark.parametrize("defect,precision", PLANTED, ids=[f"{d}-{G.PREC_NAMES[p]}" for d, p in PLANTED])
def test_a_planted_stage_defect_is_rejected(defect, precision):
    caught = []
    for lid in LAYOUTS:
        shares, _, _, _ = _chain(lid, precision, defect)
        worst = max(shares, key=lambda k: shares[k][0])
        hit = shares[worst][0] > 1.0
        out = {k: round(v[0], 2) for k, v in shares.items() if v[0] > 1.0}
        print(f"  {defect} {G.PREC_NAMES[precision]} {lid}: clearest at {worst}, {shares[worst][0]:.3g} x the bound -> {'rejected' if hit else 'passes'}; out of bound: {out}")
        if hit:
            caught.append(lid)
            with pytest.raises(AssertionError, match="stages out of bound"):
                G.stage_check(defect, shares)
    assert caught, f"{defect}: no layout rejects it"
    if defect == "rope_position_is_row_index":
        assert caught == ["ragged_90_100"]  # (in a uniform batch the row index IS the position)
