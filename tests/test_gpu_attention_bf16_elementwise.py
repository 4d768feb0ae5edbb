"""The bf16 flash-attention kernels -- the production path -- per element against fp64, with a bound that comes from the number formats alone
(gpu_helpers.attn_ref_terms, gpu_helpers.check_elementwise; nothing in it is measured on the device):

    |out - ref| <= 1 bf16 ulp(ref) + 8 fp32 ulps of mag + 2^-8 pv          on every element of every valid query row
        1 bf16 ulp(ref)   the one rounding of the stored output
        mag               pv (1 + 2 max_k sum_d |q_d k_d| scale), pv = sum_k p_k |v_k|: what the fp32 arithmetic works on, the PV sum and,
                          through the exponential, the score sum
        2^-8 pv           each un-normalised numerator is rounded ONCE, to nearest even, to bf16 in front of the PV product: half an ulp of 7
                          stored bits.  The row sum comes from the unrounded numerators, so nothing cancels it.
tests/test_attention_bound_host.py asserts on the CPU that the documented arithmetic meets this bound (0.41 .. 0.50 of it) and that a dropped
or leaked key exceeds it 55 to 900 times.  The rel-L2 < 6e-3 / max-abs < 0.05 of the older tests admit truncated numerators (a -2.4e-3
relative bias on every output) and an error of a few percent confined to one 32-query block of a long sequence; this bound and the bias
statistic below admit neither.

Which template build a case reaches (attention_fast.hip: launch_attention_fast, picks_wide, launch_wide; attention_pipe.hip), with
masked = a key mask is given or N % 64 != 0; every case forces its kernel with G.knobs(attn_variant = ...):
    attn_variant 2, f5_op_attention             attn_wide_kernel<MASKED = masked, QS = false>    (64 queries per wave)
    attn_variant 2, f5_op_attention_prescaled   attn_wide_kernel<MASKED = masked, QS = true>     (reference-free build, q carries QSCALE)
    attn_variant 5, either entry point          attn_pipe_kernel<MASKED = masked, 4>             (pipelined, 32 queries per wave; the pre-scaled
                                                                                                  entry hands it c = 1)
    attn_variant 0 (by grid size)               the wide kernel from B * H * ceil(N / 256) >= CUs on, the pipelined one below: section c's 32 and
                                                36 workgroups are below the CU count of any part this runs on
    attn_variant 5, f5_op_attention_ragged      attn_pipe_kernel<MASKED = n % 64 != 0, 4, 0, 2, SEG = true>   (tests/test_gpu_attention_ragged.py
                                                holds them to the same bound, assertion (b); here: the bias statistic)
    f5_op_attention_dropout(..., kernel = 1)    attn_dropout_kernel (attention_dropout.hip)

Sections: (a) a sweep over the small N at which the tile bookkeeping changes (1 .. 257: one to five key tiles, ragged and whole last tiles,
the three branches of the wide kernel's prologue wait, the XCD remap at B * H % 8 == 0), three key masks, two input kinds; (b) the adversarial
constructions of test_gpu_ops.py and test_gpu_attention_prescale.py, planted rows included -- a planted score of hundreds of log2 units makes
`mag` large on its own row only; (c) one long shape per build; (d) every key counted once: q = 0 and one-hot values make every output a
count / n_valid that fp32 holds exactly; (e) the dropout MFMA kernel on the host's keep mask; and the rounding-bias statistic
test_numerators_and_outputs_round_to_nearest: m = mean (out - ref) / ref on positive values, |m| <= 2^-12 -- a factor 4 above what the CPU
restatement must meet with rounding and a factor 4 below what it must exceed with truncation (both asserted in
test_attention_bound_host.py).

Measured on MI355X (worst share of the bound per kernel build over every case of this module; m per case of the bias test):
    attn_wide_kernel<MASKED = false, QS = false>   0.665        attn_pipe_kernel<MASKED = false>   0.636  (by grid size, section c: 0.608)
    attn_wide_kernel<MASKED = true,  QS = false>   0.655        attn_pipe_kernel<MASKED = true>    0.644  (by grid size, section c: 0.527)
    attn_wide_kernel<MASKED = false, QS = true>    0.650        attn_dropout_kernel                0.458
    attn_wide_kernel<MASKED = true,  QS = true>    0.711
    the ragged op's launches (test_gpu_attention_ragged.py, assertion (b), SEG builds and per-utterance wide launches together):
        n % 64 == 0   0.723        n % 64 != 0   0.627
    every key counted once: at most 0.462 bf16 ulp of count / n_valid; bit-equal wherever n_valid is a power of two
    m, (2, 200, 3, lens)      variant 2: -2.44e-05 scaling, -3.57e-06 pre-scaled    variant 5: -2.44e-05, -7.00e-06    ragged op: -2.21e-05
    m, (1, 1024, 2, no mask)  variant 2: -3.90e-06 scaling, +2.28e-06 pre-scaled    variant 5: -3.90e-06, -4.95e-06    ragged op: -3.90e-06
    (2^-12 = 2.44e-04; truncated numerators would give -2.6e-03.)  No kernel exceeded the bound: no defect found, no term added."""
import functools

import pytest
import torch

import gpu_helpers as G

pytestmark = pytest.mark.gpu
P_BF16 = G.P_BF16
WORST, BIAS = {}, {}  # kernel build -> worst share of the bound; case -> m (printed when the module is done)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()
    yield
    for k in sorted(WORST):
        print(f"\n  worst share of the bound, {k}: {WORST[k]:.3f}", end="")
    for k, m in BIAS.items():
        print(f"\n  m, {k}: {m:+.2e}", end="")
    print()


def build_of(variant, N, mask, entry):
    masked = "true" if (mask is not None or N % 64 != 0) else "false"
    if variant == 2:
        return f"attn_wide_kernel<MASKED={masked}, QS={'true' if entry == 'prescaled' else 'false'}>"
    return f"attn_pipe_kernel<MASKED={masked}>" + ("" if variant == 5 else " (by grid size)")


def run(qkv, mask, variant, entry):
    with G.knobs(attn_variant=variant):
        if entry == "prescaled":
            return G.op_attention_prescaled(1, qkv, mask)
        return G.op_attention(P_BF16, 1, qkv, mask)


def prescale(qkv):
    """the same inputs as the pre-scaled entry point takes them: q times QSCALE, rounded to bf16"""
    qs = qkv.clone()
    qs[:, :, 0] = G.bf16_round(qkv[:, :, 0] * G.QSCALE)
    return qs


def terms_by_head(qkv, mask, **kw):
    """attn_ref_terms one head at a time (a long sequence's [N, N] fp64 temporaries): the same values"""
    parts = [G.attn_ref_terms(qkv[:, :, :, h:h + 1], mask, P_BF16, **kw) for h in range(qkv.shape[3])]
    return tuple(torch.cat([p[i] for p in parts], dim=-1) for i in range(3))


def check(build, name, out, terms, rows=None):
    ref, mag, extra = terms
    assert torch.isfinite(out).all(), name
    v = slice(None) if rows is None else rows
    w = G.check_elementwise(f"{name} [{build}]", out[v], ref[v], mag[v], P_BF16, extra[v])
    WORST[build] = max(WORST.get(build, 0.0), w)


def key_mask(kind, B, N):
    """-> (key mask [B, N] or None, the query rows to compare).  none; lens = (N, max(1, N - 13)): the rows inside each length; holes: item 0
    without keys 63 and 64 and, from three key tiles on, without the whole tile 1 (keys 64 .. 127), item 1 with exactly ONE valid key -- the
    mask hides keys, every query row is computed against the same valid keys and is compared."""
    if kind == "none":
        return None, None
    if kind == "lens":
        mask = torch.arange(N)[None, :] < torch.tensor([N, max(1, N - 13)][:B])[:, None]
        return mask, mask
    assert kind == "holes" and B == 2
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[0, 63:65] = False
    if N > 128:
        mask[0, 64:128] = False
    if not mask[0].any():
        mask[0] = True  # (N = 1 has no key to hide)
    mask[1] = False
    mask[1, 3 * (N - 1) // 4] = True
    return mask, None


# ----------------------------------------------------------------------------- a. small shapes
SWEEP_N = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
SWEEP = [(N, 2) for N in SWEEP_N] + [(N, 4) for N in (64, 129, 257)]  # (N, H) at B = 2; H = 4: B * H % 8 == 0, the XCD remap


@functools.lru_cache(maxsize=None)
def sweep_case(N, H, mask_kind, flat, entry):
    """randn * 1.5 (flat: q times 0.05 -- nearly uniform probabilities), rounded to bf16; shared by the variants, nobody modifies it"""
    g = torch.Generator().manual_seed(10000 * flat + 10 * N + H)
    qkv = torch.randn(2, N, 3, H, 64, generator=g) * 1.5
    if flat:
        qkv[:, :, 0] *= 0.05
    qkv = G.bf16_round(qkv)
    if entry == "prescaled":
        qkv = prescale(qkv)
    mask, rows = key_mask(mask_kind, 2, N)
    return qkv, mask, rows, G.attn_ref_terms(qkv, mask, P_BF16, base2=entry == "prescaled")


@pytest.mark.parametrize("mask_kind", ["none", "lens", "holes"])
@pytest.mark.parametrize("entry", ["scaling", "prescaled"])
@pytest.mark.parametrize("variant", [2, 5], ids=["64_queries_per_wave", "pipelined_32_queries_per_wave"])
def test_small_shapes(variant, entry, mask_kind):
    for N, H in SWEEP:
        for flat in (0, 1):
            qkv, mask, rows, terms = sweep_case(N, H, mask_kind, flat, entry)
            out = run(qkv, mask, variant, entry)
            check(build_of(variant, N, mask, entry), f"N={N} H={H} {mask_kind} {'flat' if flat else 'randn'} {entry}", out, terms, rows)


# ----------------------------------------------------------------------------- b. the adversarial constructions
@functools.lru_cache(maxsize=None)
def adversarial_case(name):
    """-> (qkv, mask, rows to compare, terms, entry point)"""
    if name == "deferred_rescale":
        qkv, mask = G.attn_case_deferred_rescale()[0], None
    elif name.startswith("range_guard"):
        qkv, mask, _ = G.attn_case_range_guard(name == "range_guard_masked")
    elif name == "spiked_512":
        qkv, mask = G.attn_case_spiked_512(), None
    else:  # the pre-scaled cases: "prescale/<case>/<H>"
        from test_gpu_attention_prescale import make_case
        _, case, H = name.split("/")
        qkv, mask, _, _ = make_case(case, int(H))
        return qkv, mask, mask, G.attn_ref_terms(qkv, mask, P_BF16, base2=True), "prescaled"
    return qkv, mask, mask, G.attn_ref_terms(qkv, mask, P_BF16), "scaling"


PRESCALE_CASES = ["ordinary", "high_trip", "low_rerun", "tiny_then_ordinary", "masked"]
ADVERSARIAL = ([("deferred_rescale", v) for v in (2, 5)] + [("range_guard_unmasked", 2), ("range_guard_masked", 2)] + [("spiked_512", v) for v in (2, 5)] +
               [(f"prescale/{c}/{H}", 2) for c in PRESCALE_CASES for H in (4, 3)] + [(f"prescale/{c}/3", 5) for c in ("ordinary", "masked")])


@pytest.mark.parametrize("name,variant", ADVERSARIAL, ids=[f"{n}-variant{v}" for n, v in ADVERSARIAL])
def test_adversarial_constructions(name, variant):
    """Every valid row under the bound, the planted rows included: the variants the older tests run these inputs through (the 512-key spiked
    case, which they leave to the grid size, through both kernels)."""
    qkv, mask, rows, terms, entry = adversarial_case(name)
    out = run(qkv, mask, variant, entry)
    check(build_of(variant, qkv.shape[1], mask, entry), name, out, terms, rows)


# ----------------------------------------------------------------------------- c. one long shape per build
@functools.lru_cache(maxsize=None)
def long_case(masked, entry):
    B, N, H = (2, 2050, 2) if masked else (1, 4096, 2)
    g = torch.Generator().manual_seed(N)
    qkv = G.bf16_round(torch.randn(B, N, 3, H, 64, generator=g) * 1.5)
    if entry == "prescaled":
        qkv = prescale(qkv)
    mask = (torch.arange(N)[None, :] < torch.tensor([2050, 1013])[:, None]) if masked else None
    return qkv, mask, terms_by_head(qkv, mask, base2=entry == "prescaled")


@pytest.mark.parametrize("variant,entry", [(0, "scaling"), (2, "scaling"), (2, "prescaled"), (5, "scaling"), (5, "prescaled")])
@pytest.mark.parametrize("masked", [False, True], ids=["4096_unmasked", "2050_ragged_lens"])
def test_long_sequences(masked, variant, entry):
    qkv, mask, terms = long_case(masked, entry)
    out = run(qkv, mask, variant, entry)
    check(build_of(variant, qkv.shape[1], mask, entry), f"long {tuple(qkv.shape[:2])} {entry}", out, terms, mask)


# ----------------------------------------------------------------------------- d. every key counted once
@pytest.mark.parametrize("mask_kind", ["none", "lens", "holes"])
@pytest.mark.parametrize("entry", ["scaling", "prescaled"])
@pytest.mark.parametrize("variant", [2, 5], ids=["64_queries_per_wave", "pipelined_32_queries_per_wave"])
def test_every_key_counted_once(variant, entry, mask_kind):
    """q = 0: every numerator is exp2(0) = 1 in every build, whatever the reference.  V[k, d] = (d == k % 64): out[q, d] is count_d / n_valid
    over the valid keys, and the fp32 sums behind it are exact integers -- exact up to 1 / l and the output rounding at ANY flatness, where
    the bound of the other tests scales with the values.  A key dropped, counted twice or leaked moves a column by at least 1 / 17 of its
    value at N <= 1024 (at most 16 keys share a column): 15 bf16 ulps.  Bit equality where n_valid is a power of two (the division is exact)."""
    B, H = 2, 2
    for N in (64, 65, 192, 257, 1024):
        mask, rows = key_mask(mask_kind, B, N)
        qkv = torch.zeros(B, N, 3, H, 64)
        qkv[:, torch.arange(N), 2, :, torch.arange(N) % 64] = 1.0
        out = run(qkv, mask, variant, entry).view(B, N, H, 64)
        valid = torch.ones(B, N, dtype=torch.bool) if mask is None else mask
        for b in range(B):
            n_valid = int(valid[b].sum())
            count = torch.bincount(torch.arange(N)[valid[b]] % 64, minlength=64).double()
            exact = (count / n_valid)[None, None, :].expand(N, H, 64)
            got = out[b] if rows is None else out[b][rows[b]]
            exact = exact if rows is None else exact[rows[b]]
            err = (got.double() - exact).abs()
            worst = float((err / G.bf16_ulp(exact)).max())
            print(f"  N={N} {mask_kind} item {b}: {n_valid} valid keys, worst {worst:.3f} bf16 ulp")
            assert (err <= G.bf16_ulp(exact)).all(), (N, b, worst)
            assert (got[exact == 0] == 0).all(), (N, b)  # a column none of the valid keys feeds
            if n_valid & (n_valid - 1) == 0:
                assert torch.equal(got.double(), exact), (N, b)


# ----------------------------------------------------------------------------- e. the dropout MFMA kernel
@pytest.mark.parametrize("B,N,H,masked", [(2, 200, 3, True), (1, 257, 2, False)])
def test_dropout_mfma_kernel(B, N, H, masked):
    """attn_dropout_kernel on the keep mask of tests/dropout_ref.py, p = 0.1: the kept probabilities times 1 / (1 - p) in ref and in pv (the
    kernel takes the row sum from the undropped numerators and rounds the kept ones to bf16)."""
    import dropout_ref as R
    from test_gpu_attention_dropout import op_attention_dropout
    qkv, mask = G.attn_randn_case(B, N, H, masked)
    keep = torch.from_numpy(R.keep_mask(R.SEED, R.STREAM, R.BATCH0, B, H, N, R.P))
    terms = G.attn_ref_terms(qkv, mask, P_BF16, keep=keep, p=R.P)
    out = op_attention_dropout(P_BF16, 1, qkv, mask)
    check("attn_dropout_kernel", f"dropout {(B, N, H, masked)}", out, terms, mask)


# ----------------------------------------------------------------------------- no rounding bias
@functools.lru_cache(maxsize=None)
def bias_case(B, N, H, masked, entry):
    qkv, mask = G.attn_randn_case(B, N, H, masked, positive_v=True)
    if entry == "prescaled":
        qkv = prescale(qkv)
    ref = G.attn_ref_terms(qkv, mask, P_BF16, base2=entry == "prescaled")[0]
    assert float(ref.min()) >= 0.5
    return qkv, mask, ref


def run_ragged(qkv):
    """qkv [nbr, n, 3, H, 64] as one utterance of a ragged call under attn_variant 5 -> [nbr, n, H * 64]"""
    from test_gpu_attention_ragged import POISON, SENTINEL, _layout, _pack
    nbr, n, _, H, _ = qkv.shape
    off, rows = _layout((n,))
    assert POISON == 50.0
    packed = _pack([qkv], off, rows, nbr, H, 0)
    with G.knobs(attn_variant=5):
        out = G.op_attention_ragged(P_BF16, 1, nbr, off, [n], H, rows, packed, torch.full((nbr * rows, H * 64), SENTINEL))
    return out.view(nbr, rows, H * 64)[:, off[0]:off[0] + n]


BIAS_RUNS = [(2, "scaling"), (2, "prescaled"), (5, "scaling"), (5, "prescaled"), (5, "ragged")]


@pytest.mark.parametrize("variant,entry", BIAS_RUNS, ids=[f"variant{v}-{e}" for v, e in BIAS_RUNS])
@pytest.mark.parametrize("B,N,H,masked", [(2, 200, 3, True), (1, 1024, 2, False)])
def test_numerators_and_outputs_round_to_nearest(B, N, H, masked, variant, entry):
    """V = bf16(|V| + 0.5): every output is at least 0.5 and pv = ref.  m = mean over the valid elements of (out - ref) / ref.  Rounding to
    nearest leaves |m| <= 2^-14 in the CPU restatement, truncating the numerators or the outputs puts it beyond 2^-10 (both asserted in
    test_attention_bound_host.py); 2^-12 lies a factor 4 from either.  The ragged op (SEG builds) takes the shape as one utterance of
    B branches without a key mask."""
    if entry == "ragged":
        qkv, mask, ref = bias_case(B, N, H, False, "scaling")
        out = run_ragged(qkv)
    else:
        qkv, mask, ref = bias_case(B, N, H, masked, entry)
        out = run(qkv, mask, variant, entry)
    assert torch.isfinite(out).all()
    m = G.mean_signed_error(out, ref, mask)
    BIAS[f"{(B, N, H, masked)} variant {variant} {entry}"] = m
    print(f"  {(B, N, H, masked)} variant {variant} {entry}: m = {m:+.2e}")
    assert abs(m) <= 2.0 ** -12
