"""The ragged sampler's attention call at op level (f5_op_attention_ragged -> launch_attention_ragged_all, the launcher dit_eval.hip uses)
against the fp64 softmax of every utterance.

Layout, as f5_sample_ragged builds it: `nbr` branches (CFG) of `rows` rows each -- the batch stride of every launch -- and inside a branch
utterance u on rows off[u] .. off[u] + n[u], every offset a multiple of 16 and at least 16 gap rows behind every utterance.  Gap rows (and
padding columns) of qkv hold 50.0: a key read across an utterance's end swamps the softmax.  `out` is pre-filled with 776.0
(seven significant bits: exact in bf16, so it survives the staging of `out` into the activation type; 777.0 would not).

Every result-checking test asserts, for every utterance and branch,
  (a) bit equality with the utterance's own packed launch, op_attention(prec, kind, qkv_u) with qkv_u [nbr, n, 3, H, 64], under the same
      attn_variant: the contract of kernels.h / attention_pipe.hip ("every block computes exactly what it computes in a launch over its
      utterance alone").  The own launch has B = nbr, as launch_attention_ragged states it and as the batch-1 sample() makes it: by grid size
      (attn_variant 0) the kernel choice depends on B;
  (b) accuracy against the fp64 softmax of that utterance, with the bounds the packed-form tests of test_gpu_ops.py use at this input scale
      (tuned bf16 kernels: rel-L2 < 6e-3, max-abs < 0.05, all finite, and next to them the ELEMENT-WISE fp64 bound of
      test_gpu_attention_bf16_elementwise.py: 1 bf16 ulp + 8 fp32 ulps of the sums of magnitudes + 2^-8 sum_k p_k |v_k|, per utterance and
      branch; reference kernels: rel-L2 < 3e-6 in fp32, < 4e-3 in bf16, and element-wise 1 ulp of the stored type (fp32 / bf16) + 8 fp32
      ulps of the sums of magnitudes, the bound of test_gpu_attention_ref_elementwise.py); in the
      fp16 mode (P_FP16: utterances rounded to fp16, a cache entry of their own) the ELEMENT-WISE fp64 bound of test_gpu_fp16_ops.py
      (1 fp16 ulp + 8 fp32 ulps of the sums of magnitudes + the numerator-rounding terms) per utterance and branch, no rel-L2 number;
  (c) no stray write: every element of `out` outside the utterances' rows and head columns, in every branch, still holds 776.0."""
import functools

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
P_BF16, P_FP32, P_FP16 = 0, 1, 2
SENTINEL, POISON = 776.0, 50.0  # both exact in bf16 and in fp16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _layout(lens, first=0):
    """The sampler's rule: utterance u owns round_up(n_u + 16, 16) rows.  Returns (offsets, rows of one branch)."""
    off, o = [], first
    for n in lens:
        off.append(o)
        o += (n + 16 + 15) // 16 * 16
    return off, o


@functools.lru_cache(maxsize=2)
def _case(lens, nbr, H, first, ref_heads, fp16=False):
    """Seeded utterances [nbr, n, 3, H, 64] (rounded to bf16, or to fp16 for the fp16 mode), their layout, and the fp64 reference of each over
    the heads `ref_heads` (None: all): the triple (reference, fp32 magnitude, numerator-rounding allowance) of gpu_helpers.attn_ref_terms in
    the 16-bit type the utterances were rounded to.  Shared by the parametrisations that differ only in the schedule; nobody modifies it."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(sum(lens) + 131 * nbr + 7 * H + first)
    rnd = (lambda t: t.half().float()) if fp16 else G.bf16_round
    utts = [rnd(torch.randn(nbr, n, 3, H, 64, generator=g) * 1.5) for n in lens]
    off, rows = _layout(lens, first)
    heads = list(range(H)) if ref_heads is None else list(ref_heads)
    refs = [G.attn_ref_terms(u[:, :, :, heads], None, P_FP16 if fp16 else P_BF16) for u in utts]
    return utts, off, rows, heads, refs


def _pack(utts, off, rows, nbr, H, ldq_extra):
    ldq = 3 * H * 64 + ldq_extra
    qkv = torch.full((nbr, rows, ldq), POISON)
    for u, o in zip(utts, off):
        n = u.shape[1]
        qkv[:, o:o + n, :3 * H * 64] = u.reshape(nbr, n, 3 * H * 64)
    return qkv.reshape(nbr * rows, ldq)


def _run(prec, attn_kernel, variant, lens, nbr, H, first=0, ldq_extra=0, ldo_extra=0, ref_heads=None):
    """One ragged call under `variant`, with assertions (a), (b), (c).  Returns the raw output [nbr, rows, H * 64 + ldo_extra]."""
    import gpu_helpers as G
    utts, off, rows, heads, refs = _case(tuple(lens), nbr, H, first, None if ref_heads is None else tuple(ref_heads), prec == P_FP16)
    inner, ldo = H * 64, H * 64 + ldo_extra
    qkv = _pack(utts, off, rows, nbr, H, ldq_extra)
    out0 = torch.full((nbr * rows, ldo), SENTINEL)
    kind = 1 if (prec in (P_BF16, P_FP16) and attn_kernel != 0) else 0  # the tuned kernels exist for both 16-bit modes
    with G.knobs(attn_variant=variant):
        out = G.op_attention_ragged(prec, attn_kernel, nbr, off, list(lens), H, rows, qkv, out0, ldq_extra, ldo_extra).view(nbr, rows, ldo)
        own = [G.op_attention(prec, kind, u) for u in utts]
    untouched = torch.ones(nbr, rows, ldo, dtype=torch.bool)
    cols = torch.cat([torch.arange(h * 64, h * 64 + 64) for h in heads])
    for u, (o, n) in enumerate(zip(off, lens)):
        got = out[:, o:o + n, :inner]
        untouched[:, o:o + n, :inner] = False
        assert torch.isfinite(got).all(), f"utterance {u} (n = {n})"
        bad = (got != own[u]).any(dim=-1).nonzero()
        assert torch.equal(got, own[u]), f"(a) utterance {u} (n = {n}) differs from its own launch, first at (branch, row) {bad[0].tolist()} of {len(bad)} rows"
        if prec == P_FP16:
            from test_gpu_fp16_ops import check_f16
            ref, mag, extra = refs[u]
            for br in range(nbr):
                check_f16(f"(b) utterance {u} n={n} branch {br}", got[br][:, cols], ref[br], mag[br], extra[br])
            continue
        ref, mag, extra = refs[u]
        for br in range(nbr):
            g, r = got[br][:, cols], ref[br].float()
            rl, ma = rel_l2(g, r), float((g - r).abs().max())
            print(f"  utterance {u} n={n} branch {br}: rel-L2 {rl:.3e}, max-abs {ma:.3e}")
            if kind == 1:
                assert rl < 6e-3 and ma < 0.05, f"(b) utterance {u} (n = {n}) branch {br}: rel-L2 {rl:.3e}, max-abs {ma:.3e}"
                G.check_elementwise(f"(b) utterance {u} n={n} branch {br}", g, ref[br], mag[br], P_BF16, extra[br])
            else:
                assert rl < (3e-6 if prec == P_FP32 else 4e-3), f"(b) utterance {u} (n = {n}) branch {br}: rel-L2 {rl:.3e}"
                # the reference kernel keeps its numerators in fp32: no numerator-rounding term in either type
                G.check_elementwise(f"(b) reference kernel, utterance {u} n={n} branch {br}", g, ref[br], mag[br], prec)
    stray = (out != SENTINEL) & untouched
    assert not stray.any(), f"(c) {int(stray.sum())} elements outside the utterances were written, first at (branch, row, col) {stray.nonzero()[0].tolist()}"
    return out


MIX = (256, 257, 1024, 1000, 64 * 5, 333)


# BH = H * nbr * (utterances of the launch): the XCD remap of attn_pipe_kernel is taken when BH % 8 == 0
@pytest.mark.parametrize("lens,nbr,H,first", [
    ((256, 320, 1024), 2, 2, 0),       # unmasked SEG build alone; BH = 12: no remap
    ((257, 411, 300), 2, 2, 0),        # masked SEG build alone; BH = 12
    (MIX, 2, 2, 0),                    # both builds write into one buffer; BH = 12 each
    (MIX, 1, 2, 0),                    # CFG off: one branch; BH = 6 each
    (MIX, 2, 4, 48),                   # BH = 24 each: remap taken in both launches; the first utterance starts at row 48
    ((256, 320, 1024, 512), 1, 2, 0),  # CFG off, BH = 8: remap taken, unmasked
    ((257, 411), 2, 2, 0),             # BH = 8: remap taken, masked
], ids=["unmasked", "masked", "mixed", "mixed_cfg_off", "mixed_remap_first_offset", "unmasked_cfg_off_remap", "masked_remap"])
def test_ragged_pipelined_seg_builds(lens, nbr, H, first):
    """attn_pipe_kernel<..., SEG = true> (attn_variant 5: everything pipelined): the unmasked build (every n % 64 == 0), the masked build, both
    in one call, one and two branches, the XCD-aware block order taken and skipped over the mixed grid (query blocks past a short utterance's
    end leave before the remapped index is used for anything else)."""
    _run(P_BF16, 1, 5, lens, nbr, H, first)


@pytest.mark.parametrize("variant", [5, 0], ids=["pipelined", "by_grid_size"])
def test_ragged_short_utterance_next_to_long(variant):
    """Lengths 1 .. 129 beside 1500 in one masked launch: nearly all query blocks of the short ones exit early, and the clamps key = N - 1 and
    qrow = N - 1 must use the utterance's own N and stay inside its own rows (the gap behind it holds 50.0)."""
    _run(P_BF16, 1, variant, (1, 31, 64, 127, 129, 1500), 2, 2)


def test_ragged_wide_kernel_with_batch_stride():
    """attn_variant 2: every utterance gets its own launch of attn_wide_kernel with bstride = rows != n, unmasked (256, 1024) and masked (300,
    2050) builds."""
    _run(P_BF16, 1, 2, (256, 300, 1024, 2050), 2, 2)


def test_ragged_routing_by_grid_size_in_one_call():
    """attn_variant 0 at 16 heads, two branches: by nbr * H * ceil(n / 256) >= CUs the 2048-frame utterance goes to the wide kernel on a
    256-CU part while 1024 and 777 share pipelined launches, all into one buffer.  The route depends on the CU count and is NOT asserted: (a)
    compares with the own launch, which takes the same route on the same part.  (b) is computed for heads 0, 7 and 15 only (the fp64
    scores of 16 heads at 2048 frames are large); (a) and (c) cover every head."""
    _run(P_BF16, 1, 0, (2048, 1024, 777), 2, 16, ref_heads=(0, 7, 15))


@pytest.mark.parametrize("cnt", [13, 25])
def test_ragged_more_utterances_than_one_table(cnt):
    """More than AttnSegs::MAX = 12 utterances: launch_attention_ragged_all cuts the list into tables (12 + 1; 12 + 12 + 1).  An utterance
    dropped or shifted at a table boundary (the 12th, 13th, 24th, 25th) keeps the sentinel or fails (a)."""
    lens = tuple([256, 257, 320, 300][i % 4] for i in range(cnt))
    assert _layout(lens)[1] < 16384
    _run(P_BF16, 1, 5, lens, 2, 2)


@pytest.mark.parametrize("prec", [P_FP32, P_BF16], ids=["fp32", "bf16"])
def test_ragged_reference_kernels_with_batch_stride(prec):
    """attn_kernel 0: attn_ref_kernel in both activation types, one launch per utterance with bstride = rows."""
    _run(prec, 0, 0, (41, 200, 64), 2, 2)


@pytest.mark.parametrize("variant", [5, 2], ids=["pipelined", "64_queries_per_wave"])
def test_ragged_padded_leading_dimensions(variant):
    """ldq = 3 * H * 64 + 64, ldo = H * 64 + 8: the padding columns of qkv hold 50.0, those of `out` keep the sentinel (assertion (c) covers
    them, inside the utterances' rows too)."""
    out = _run(P_BF16, 1, variant, (256, 300), 2, 2, ldq_extra=64, ldo_extra=8)
    assert (out[:, :, 2 * 64:] == SENTINEL).all()


def _refused(prec, attn_kernel, off, n, rows, ldq_extra=0, H=2, nbr=2):
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    qkv = torch.zeros(nbr * rows, 3 * H * 64 + ldq_extra)
    out0 = torch.full((nbr * rows, H * 64), SENTINEL)
    with G.knobs(attn_variant=5):
        rc, out = G.op_attention_ragged_rc(prec, attn_kernel, nbr, off, n, H, rows, qkv, out0, ldq_extra, 0)
        msg = _lib.last_error()
    assert rc != 0
    assert (out == SENTINEL).all(), "a refused call wrote to `out`"
    return msg


def test_ragged_refusals():
    """Refused with a message and without a write: an utterance past the end of a branch, before its start, an empty one (also behind a valid
    one), and a leading dimension the tuned kernels' 16-byte accesses cannot take."""
    assert "lies outside" in _refused(P_BF16, 1, [0, 272], [256, 257], 528)     # off + n = 529 > rows
    assert "lies outside" in _refused(P_BF16, 1, [-16, 272], [256, 256], 528)
    assert "has no rows" in _refused(P_BF16, 1, [0, 272], [256, 0], 528)
    assert "has no rows" in _refused(P_FP32, 0, [0], [0], 16)
    assert "attention_fast: ldq and ldo must be multiples of 8" in _refused(P_BF16, 1, [0, 272], [256, 257], 544, ldq_extra=4)


# ----------------------------------------------------------------------------- the fp16 mode: launch_attention_pipe_segs_f16 (both SEG builds),
# launch_attention_wide_f16 with bstride != N and attn_ref_kernel<f16_t>, with assertions (a), (b) element-wise, (c)
@pytest.mark.parametrize("lens,nbr,H,first", [
    ((256, 320, 1024), 2, 2, 0),      # unmasked SEG build alone
    ((257, 411, 300), 2, 2, 0),       # masked SEG build alone
    ((256, 257, 320, 333), 2, 4, 48),  # both in one call, BH = 16 each: XCD remap taken; the first utterance starts at row 48
], ids=["unmasked", "masked", "mixed_remap_first_offset"])
def test_ragged_fp16_pipelined_seg_builds(lens, nbr, H, first):
    _run(P_FP16, 1, 5, lens, nbr, H, first)


@pytest.mark.parametrize("variant", [5, 0], ids=["pipelined", "by_grid_size"])
def test_ragged_fp16_short_utterance_next_to_long(variant):
    _run(P_FP16, 1, variant, (1, 31, 64, 127, 129, 1500), 2, 2)


def test_ragged_fp16_wide_kernel_with_batch_stride():
    """attn_variant 2: launch_attention_wide_f16 per utterance with bstride = rows != n, unmasked (256, 1024) and masked (300) builds."""
    _run(P_FP16, 1, 2, (256, 300, 1024), 2, 2)


def test_ragged_fp16_more_utterances_than_one_table():
    lens = tuple([256, 257, 320, 300][i % 4] for i in range(13))
    _run(P_FP16, 1, 5, lens, 2, 2)


def test_ragged_fp16_reference_kernel_with_batch_stride():
    """attn_kernel 0: attn_ref_kernel<f16_t>, one launch per utterance with bstride = rows."""
    _run(P_FP16, 0, 0, (41, 200, 64), 2, 2)


@pytest.mark.parametrize("variant", [5, 2], ids=["pipelined", "64_queries_per_wave"])
def test_ragged_fp16_padded_leading_dimensions(variant):
    out = _run(P_FP16, 1, variant, (256, 300), 2, 2, ldq_extra=64, ldo_extra=8)
    assert (out[:, :, 2 * 64:] == SENTINEL).all()
