"""Pre-scaled q at op level: attn_wide_kernel's reference-free build (q arrives multiplied by softmax_scale * log2 e,
P = exp2(s) against reference 0, a high-side and a low-side range guard) against the fp64 softmax, the same inputs through the scaling build,
and the fold-table builder's scaled q rows.

Tolerances are the ones tests/test_gpu_ops.py states for this kernel: rel-L2 < 6e-3 and max |error| < 0.05 over an output (P is rounded to
bf16 in front of the PV product and the output is bf16: 2^-9 relative each), and, on a row that a guard case plants,
max |error| < 0.03 * max(1, max |reference|) (test_attention_wide_kernel_range_guard)."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
QSCALE = 0.125 * 1.4426950408889634  # what the q projection carries: 1/sqrt(64) * log2(e)
REL_TOL, ABS_TOL, ROW_TOL = 6e-3, 0.05, 0.03


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def attn_ref_base2(qkv, mask):
    """fp64 softmax of pre-scaled scores: P = 2^(q . k) / sum (the scale and log2 e are in q)."""
    q, k, v = [qkv[:, :, i].transpose(1, 2).double() for i in range(3)]  # [B,H,N,64]
    s = q @ k.transpose(-1, -2) * 0.6931471805599453
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    o = torch.softmax(s, dim=-1) @ v
    return o.transpose(1, 2).reshape(qkv.shape[0], qkv.shape[1], -1).float()


def attn_ref_unscaled(qkv, mask):
    q, k, v = [qkv[:, :, i].transpose(1, 2).double() for i in range(3)]
    s = q @ k.transpose(-1, -2) / 8.0
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    o = torch.softmax(s, dim=-1) @ v
    return o.transpose(1, 2).reshape(qkv.shape[0], qkv.shape[1], -1).float()


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def make_case(case, H):
    """-> (qkv [B, N, 3, H, 64] with PRE-SCALED q, bf16-exact; mask or None; planted rows [(b, query, head)]; twin or None).
    One 256-query block = one workgroup per (batch, head); wave w owns queries 64 w .. 64 w + 63; key tile t = keys 64 t .. 64 t + 63.
    `twin`: the same inputs with the planted rows made ordinary (low_rerun: the run that needs no re-run)."""
    g = torch.Generator().manual_seed(100 + H + sum(map(ord, case)))
    B, N = 2, (300 if case == "masked" else 256)
    qkv = torch.randn(B, N, 3, H, 64, generator=g) * 1.5
    qkv[:, :, 0] *= QSCALE
    mask, rows, twin = None, [], None
    if case == "high_trip":
        # scores 70, 200 (exp2 overflows) and 66 log2 units in key tile 2, on queries of waves 0, 1 and 3; the other 63 / 62 queries of those
        # waves stay ordinary and take the classic step with them, wave 2 never leaves the reference-free loop
        for b in range(B):
            qn = _unit(qkv[b, :, 0])
            for q, (key, s) in {5: (130, 70.0), 70: (150, 200.0), 75: (170, 66.0), 200: (140, 66.0)}.items():
                qkv[b, q, 0] = qn[q] * 8.0
                qkv[b, key, 1] = qn[q] * (s / 8.0)
                rows += [(b, q, h) for h in range(H)]
    elif case in ("low_rerun", "tiny_then_ordinary"):
        # item (batch 0, head 1): every key (low_rerun) or the keys of tiles 0..2 (tiny_then_ordinary) carry 8 in feature 0; the planted query
        # is -30 there: its scaled scores against those keys are -240 +- a few, and exp2 of that is ZERO in fp32 (smallest subnormal 2^-149).
        # low_rerun: against reference 0 the row's l is 0 and its output 0 -- only the vote and the re-run give the fp64 result
        twin = qkv.clone()
        nk = 256 if case == "low_rerun" else 192
        for t in (qkv, twin):
            t[0, :nk, 1, 1, 0] = 8.0
            t[0, nk:, 1, 1, 0] = 0.0
        qkv[0, 133, 0, 1] *= 0.5
        qkv[0, 133, 0, 1, 0] = -30.0
        rows = [(0, 133, 1)]
    elif case == "masked":
        mask = torch.arange(N)[None, :] < torch.tensor([N, N - 13])[:, None]
        mask[0, 64:128] = False  # key tile 1 of utterance 0 is masked out as a whole; the last tile holds 44 (31) keys
    else:
        assert case == "ordinary"
    qkv = bf16_round(qkv)
    return qkv, mask, rows, (None if twin is None else bf16_round(twin))


CASES = ["ordinary", "high_trip", "low_rerun", "tiny_then_ordinary", "masked"]


def check_against_ref(out, ref, mask, rows):
    """the stated bounds; returns the figures (printed by the callers in front of their assertions)"""
    valid = slice(None) if mask is None else mask
    fig = dict(rel=rel_l2(out[valid], ref[valid]), amax=float((out[valid] - ref[valid]).abs().max()), rows=[])
    for b, q, h in rows:
        o, r = out[b, q, 64 * h:64 * h + 64], ref[b, q, 64 * h:64 * h + 64]
        fig["rows"].append((b, q, h, float((o - r).abs().max()), ROW_TOL * max(1.0, float(r.abs().max()))))
    return fig


def assert_fig(fig):
    assert fig["rel"] < REL_TOL and fig["amax"] < ABS_TOL, fig
    for b, q, h, err, bound in fig["rows"]:
        assert err < bound, (b, q, h, err, bound)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _run(qkv, mask, prescaled, variant=2):
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    B, N, three, H, dh = qkv.shape
    q = qkv.cuda().float().contiguous()
    mk = None if mask is None else mask.cuda().to(torch.uint8).contiguous()
    out = torch.empty(B, N, H * 64, device="cuda")
    with G.knobs(attn_variant=variant):  # 2: the 64-queries-per-wave kernel whatever the grid size
        if prescaled:
            _lib.check(lib.f5_op_attention_prescaled(1, B, N, H, _lib.ptr(q), _lib.ptr(mk), _lib.ptr(out), _lib.stream_ptr()))
        else:
            _lib.check(lib.f5_op_attention(0, 1, B, N, H, _lib.ptr(q), _lib.ptr(mk), _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu()


@pytest.mark.parametrize("H", [4, 3], ids=["xcd_remap", "no_remap"])
@pytest.mark.parametrize("case", CASES)
def test_reference_free_build_against_fp64(case, H):
    """B = 2, H = 4 (B * H % 8 == 0: the XCD-aware workgroup order) and H = 3, N = 256 (one 256-query block, four 64-key tiles), masked N = 300:
    ordinary inputs; a high-side trip in tile 2 (in-place classic step from reference 0, subtracting loop for the rest of the item); a row whose
    every score is near -240, so that exp2 against reference 0 is 0 (vote, whole-item re-run; the other items of the launch are bit-identical to a launch without the planted row,
    the other rows of its own item agree with it to the bf16 roundings); a row that is 0 in tiles 0..2 and ordinary in tile 3 (no re-run: the
    item's other rows are bit-identical to the launch without the planted row); masked:
    one fully masked tile and a ragged last tile."""
    qkv, mask, rows, twin = make_case(case, H)
    assert torch.isfinite(qkv).all()
    out = _run(qkv, mask, prescaled=True)
    assert torch.isfinite(out).all()
    fig = check_against_ref(out, attn_ref_base2(qkv, mask), mask, rows)
    worst = max((err / bound for *_, err, bound in fig["rows"]), default=0.0)
    print(f"{case} H={H}: rel-L2 {fig['rel']:.3e}, max abs {fig['amax']:.3e}, {len(fig['rows'])} planted rows at most {worst:.3f} of their bound")
    assert_fig(fig)
    if twin is not None:
        out2 = _run(twin, mask, prescaled=True)
        fig2 = check_against_ref(out2, attn_ref_base2(twin, mask), mask, [])
        print(f"{case} H={H} (twin without the planted row): rel-L2 {fig2['rel']:.3e}, max abs {fig2['amax']:.3e}")
        assert_fig(fig2)
        (b, q, h), = rows
        same = torch.ones(out.shape[0], out.shape[2] // 64, dtype=torch.bool)
        same[b, h] = False  # every other (batch, head) item saw identical inputs
        for bb in range(out.shape[0]):
            for hh in range(out.shape[2] // 64):
                if same[bb, hh]:
                    assert torch.equal(out[bb, :, 64 * hh:64 * hh + 64], out2[bb, :, 64 * hh:64 * hh + 64]), (bb, hh)
        # the ordinary rows of the planted row's own item
        keep = torch.ones(out.shape[1], dtype=torch.bool)
        keep[q] = False
        o1, o2 = out[b, keep, 64 * h:64 * h + 64], out2[b, keep, 64 * h:64 * h + 64]
        d = float((o1 - o2).abs().max())
        print(f"{case} H={H}: ordinary rows of the planted item, with vs without the planted row: max abs {d:.3e}")
        if case == "tiny_then_ordinary":  # no re-run: the same loop ran on the same inputs
            assert torch.equal(o1, o2)
        else:
            # the re-run forms P against each row's first-tile maximum, the twin against 0: the same sums up to the bf16 rounding of P
            # (2^-9 relative on every term of sum p v / l, so at most 2^-9 max|v|) and of the output (2^-9 |o| <= 2^-9 max|v|), in either
            # run: 2 * 2 * 2^-9 max|v| between the two
            assert d <= 2.0 ** -7 * float(qkv[b, :, 2, h].abs().max())
        # the planted row itself is not zero (what reference 0 alone would leave: l = 0)
        assert float(out[b, q, 64 * h:64 * h + 64].abs().max()) > 0


def test_prescaled_against_unscaled_same_inputs():
    """B = 1, H = 8, N = 512: q * c rounded to bf16 through the reference-free build against the unscaled q through the scaling build.  With
    e_u, e_s their rel-L2 distances from the fp64 softmax of the unscaled inputs, the two outputs differ by no more than 2 * min(e_u, e_s)
    (the triangle inequality alone would allow e_u + e_s): bf16 rounding of q and of P, nothing structural."""
    g = torch.Generator().manual_seed(77)
    qkv = bf16_round(torch.randn(1, 512, 3, 8, 64, generator=g) * 1.5)
    qs = qkv.clone()
    qs[:, :, 0] = bf16_round(qkv[:, :, 0] * QSCALE)
    ref = attn_ref_unscaled(qkv, None)
    out_u, out_s = _run(qkv, None, prescaled=False), _run(qs, None, prescaled=True)
    e_u, e_s, d = rel_l2(out_u, ref), rel_l2(out_s, ref), float((out_s - out_u).norm() / ref.norm())
    print(f"unscaled build vs fp64 {e_u:.3e}, pre-scaled build vs fp64 {e_s:.3e}, pre-scaled vs unscaled {d:.3e}")
    assert e_u < REL_TOL and e_s < REL_TOL
    assert d <= 2 * min(e_u, e_s)


@pytest.mark.parametrize("variant", [0, 5], ids=["by_grid_size", "pipelined"])
def test_other_kernels_take_prescaled_q_with_unit_scale(variant):
    """the pipelined kernel (small grids) only receives c = 1 for pre-scaled q: ordinary and masked inputs against the fp64 softmax"""
    for case in ("ordinary", "masked"):
        qkv, mask, rows, _ = make_case(case, 3)
        out = _run(qkv, mask, prescaled=True, variant=variant)
        fig = check_against_ref(out, attn_ref_base2(qkv, mask), mask, rows)
        print(f"{case} variant {variant}: rel-L2 {fig['rel']:.3e}, max abs {fig['amax']:.3e}")
        assert torch.isfinite(out).all()
        assert_fig(fig)


def test_fold_table_q_rows_carry_the_scale():
    """fold_weights_kernel at D = 128, one block (inner = 128, ff = 256; the builder has no host form): with the option on, the q rows of W', c1
    and c2 equal c times the exact (fp64) option-off values to fp16 / fp32 rounding; k, v and ff rows are unchanged bit for bit."""
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    D, inner, ff = 128, 128, 256
    R = 3 * inner + ff
    g = torch.Generator().manual_seed(5)
    W = torch.randn(R, D, generator=g) / D ** 0.5
    bias = torch.randn(R, generator=g) * 0.1
    mods = [torch.randn(D, generator=g) * 0.3 for _ in range(4)]  # scale_msa, shift_msa, scale_mlp, shift_mlp
    dev = [t.cuda().contiguous() for t in (W, bias, *mods)]
    res = {}
    for on in (0, 1):
        Wt, c1, c2 = torch.empty(R, D, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
        _lib.check(lib.f5_op_fold_weights(R, 3 * inner, inner, D, on, *[_lib.ptr(t) for t in dev], _lib.ptr(Wt), _lib.ptr(c1), _lib.ptr(c2),
                                          _lib.stream_ptr()))
        res[on] = [t.cpu() for t in (Wt, c1, c2)]
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a[inner:], b[inner:])  # k, v, ff rows
    W64, b64 = W.double(), bias.double()
    sc, sh = mods[0].double(), mods[1].double()
    x = QSCALE * W64[:inner] * (1 + sc)                       # exact scaled W' of the q rows
    Wt, c1, c2 = [t[:inner].double() for t in res[1]]
    # fp16 rounding (2^-11 relative, 2^-25 absolute below the normal range) behind two fp32 products (2^-24 each)
    assert ((Wt - x).abs() <= x.abs() * (2.0 ** -11 + 2.0 ** -22) + 2.0 ** -25).all()
    # c1 = fp32 sum of the rounded values in a fixed order: D additions of 2^-24 relative on the magnitudes summed
    assert ((c1 - Wt.sum(1)).abs() <= D * 2.0 ** -24 * Wt.abs().sum(1)).all()
    assert ((c1 - x.sum(1)).abs() <= (2.0 ** -11 + D * 2.0 ** -23) * x.abs().sum(1) + D * 2.0 ** -25).all()
    c2x = QSCALE * (b64[:inner] + (W64[:inner] * sh).sum(1))
    mag = QSCALE * (b64[:inner].abs() + (W64[:inner] * sh).abs().sum(1))
    assert ((c2 - c2x).abs() <= (D + 4) * 2.0 ** -24 * mag).all()
    # and the option-off values are the unscaled ones
    x0 = W64[:inner] * (1 + sc)
    assert ((res[0][0][:inner].double() - x0).abs() <= x0.abs() * (2.0 ** -11 + 2.0 ** -23) + 2.0 ** -25).all()
