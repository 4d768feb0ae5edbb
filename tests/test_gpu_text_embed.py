"""The text path per token row: f5_text_embed (DiT._text_embed / MMDiT._text_embed -> compute_text_embed, csrc/eval_common.hip: text_gather_kernel,
mask_rows_kernel, and per ConvNeXt-V2 block dwconv7_ln, pwconv1 + GELU, GRN, pwconv2 with the in-place residual epilogue) against the oracle's
text embedding evaluated in float64, in bf16, fp16 and fp32 and with drop_text off and on.

The model tests reach this path through stage taps and outputs held to a whole-tensor rel-L2 (1.5e-2 in the 16-bit modes); a defect confined to one
token row -- the last real token, the row at a batch boundary, a filler row that must be zero, a position past the table -- passes that.  Here
every row is held to
    max_c |X - R| / max_c |R[b, p, :]|  <=  TEXT_MARGIN (4) x the worst row of the float32 restatement E_p of the kernel chain
(gpu_helpers.check_text_rows; tests/test_text_embed_bound_host.py shows on the CPU that the restatement meets the check and that each planted defect
-- filler gathered for the last token, position off by one, mask taken after drop_text, conv across the batch boundary, GRN over the flattened
batch, no mask after the last block, positions wrapping -- does not), with exact zeros on the rows the reference zeroes.  The cases are
gpu_helpers.TEXT_CASES; the backbone width does not enter the text path, so every model is the smallest create() accepts (dim 128).

Also: the drop_text output of two texts with one filler pattern is bit-identical; batch item b equals the same item run alone at B = 1 bit for
bit (the conv and GRN may not see neighbours; where the batch's GEMMs take the tuned kernel and the single item's row count would not, the single
item is run with the tuned kernel too: include/f5hip.h promises equal bits within one kernel family); ids outside the table give the bits of the
clamped ids.  Every test prints the kernel's worst row as a share of the bound."""
import pytest
import torch

import gpu_helpers as G
from gpu_helpers import P_BF16, P_FP16, P_FP32

pytestmark = pytest.mark.gpu
PRECISIONS = [P_BF16, P_FP16, P_FP32]
PREC_IDS = [G.PREC_NAMES[p] for p in PRECISIONS]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@pytest.fixture(autouse=True)
def _launcher_defaults(monkeypatch):
    for k in ("F5HIP_GEMM_KERNEL", "F5HIP_ATTN_KERNEL", "F5HIP_PRECISION", "F5HIP_ROPE_LAYOUT"):
        monkeypatch.delenv(k, raising=False)


def _model(case, precision):
    from eraxvif5tts_amd.model import DiT, MMDiT, UNetT
    cls = {"dit": DiT, "unett": UNetT, "mmdit": MMDiT}[case["backbone"]]
    m = cls(**case["arch"], text_num_embeds=G.TEXT_V, mel_dim=100, precision=G.PREC_NAMES[precision])
    sd = m.state_dict()
    missing = [k for k in sd if k not in case["W"] and k != "rotary_embed.inv_freq"]
    assert not missing, missing
    m.load_state_dict({k: v for k, v in case["W"].items() if k in sd}, strict=False)
    return m.cuda()


def _embed(m, plan, text, N, drop):
    """f5_text_embed on DEVICE-resident int32 ids -> [B, N, td] on the host"""
    out = m._text_embed(plan, text.to(device="cuda", dtype=torch.int32), N, drop)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("cid", list(G.TEXT_CASES))
def test_text_embed_rows_against_fp64(cid, precision):
    c = G.text_case(cid)
    B, N, text = c["B"], c["N"], c["text"]
    m = _model(c, precision)
    plan = m.plan(B, m._plan_seq(N, text.shape[1]), 1)
    blocks = 0 if c["mmdit"] else c["arch"].get("conv_layers", 0)
    for drop in (False, True):
        R, E = G.text_case_terms(cid, precision, drop)
        X = _embed(m, plan, text, N, drop)
        assert X.shape == R.shape
        G.check_text_rows(f"f5_text_embed {cid} {G.PREC_NAMES[precision]} drop_text={drop}", X, R, E)
        if c["backbone"] == "unett":  # the gather alone: the table's rows, exactly
            assert torch.equal(X.double(), R)
        # batch item b alone at B = 1: the same bits
        tuned = blocks > 0 and precision != P_FP32 and B * N >= 512 > N
        if tuned:
            m.set_kernels(gemm=1)
        try:
            for b in range(B):
                solo = _embed(m, plan, text[b:b + 1], N, drop)
                assert torch.equal(solo[0], X[b]), (cid, drop, b, float((solo[0] - X[b]).abs().max()))
        finally:
            if tuned:
                m.set_kernels(gemm=-1)
    # drop_text: two texts with one filler pattern give the same bits (only the flags of the ids survive)
    X2 = _embed(m, plan, c["text2"], N, True)
    assert torch.equal((c["text2"] == -1), (text == -1)) and not torch.equal(c["text2"], text)
    assert torch.equal(X2, X), (cid, float((X2 - X).abs().max()))
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("cid", ["td512_c4_mask_3x77", "mmdit128_mask_nt1030"])
def test_out_of_table_ids_give_the_bits_of_the_clamped_ids(cid, precision):
    """text_gather_kernel clamps an id outside [-1, vocab) into the table (201 rows here): ids {-5, -1, 0, vocab - 1, vocab, vocab + 7} on the
    device give exactly what the clamped ids give, and -5 is a filler row like -1."""
    c = G.text_case(cid)
    V, N = G.TEXT_V, c["N"]
    wild = c["text"].clone()
    vals = torch.tensor([-5, -1, 0, V - 1, V, V + 7])
    wild[0, 3:3 + len(vals)] = vals
    wild[1, 10:10 + len(vals)] = vals.flip(0)
    tame = G.text_clamp_ids(wild, V)
    assert not torch.equal(tame, wild)
    m = _model(c, precision)
    plan = m.plan(c["B"], m._plan_seq(N, wild.shape[1]), 1)
    for drop in (False, True):
        a, b = _embed(m, plan, wild, N, drop), _embed(m, plan, tame, N, drop)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (cid, drop, float((a - b).abs().max()))
        assert (a[0, 3:5] == 0).all() and (a[0, 5:9] != 0).any(dim=-1).all()
        R = G.text_reference(c["W"], c["arch"], tame, N, drop, c["mmdit"])
        E = G.text_emulate(precision, c["W"], c["arch"], tame, N, drop, c["mmdit"])
        G.check_text_rows(f"f5_text_embed {cid} {G.PREC_NAMES[precision]} clamped ids drop_text={drop}", a, R, E)
    del m
    torch.cuda.empty_cache()
