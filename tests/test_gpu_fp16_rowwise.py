"""The row-wise kernels of the fp16 precision mode (F5_PREC_FP16) at op level against fp64: the f16_t instantiations of the LayerNorm pass of
the residual stream (generic kernel in its three storage forms, the 16-byte dim-1024 kernel, the multi-row kernel) with the range guard
compiled into them, qk_norm + RoPE, the depthwise conv + LayerNorm, GRN and RMSNorm -- the constructions and references of
test_gpu_elementwise.py with every input the kernel reads as 16 bits rounded to fp16 on the host.

Bounds (gpu_helpers.check_rounded, precision 2): every element within 1 fp16 ulp of the fp64 reference + 8 fp32 ulps of the largest term the
kernel evaluates for it; the signed mean error over the elements whose fp32 slack is below 0.05 ulp stays under 0.05 ulp (a truncating
conversion sits near -0.5).  An fp16 ulp is 8 times smaller than a bf16 ulp and the fp32 slack is the same, so these are the sharper check of
the fp32 arithmetic the two modes share.  The bias check never skips: a case of at least 2000 output elements asserts that it covered at
least half of them (from the reference alone the kept share is 0.94 - 0.97 at mean offset 0 and 0.60 at offset 40); GRN, whose slack is taken
4 times wider, states its kept share and checks the bias where at least 1000 elements are kept.

A NaN survives every fp16 activation store (out-of-range values clip to +-65504, a NaN stays a NaN): the NaN tests at the end and the "nan"
case of the guard grid pin that.  Run with -s to see the worst error, the signed mean error and the kept share of every case."""
import math

import pytest
import torch

import test_gpu_elementwise as E
from test_gpu_elementwise import F16_MAX, P_FP16, _f16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _bias_check(name, sums, total, need_cover=True):
    """Signed mean error of the kept elements under 0.05 fp16 ulp.  Never skipped; with `need_cover` a case of >= 2000 elements must have
    kept at least half of them.  (A uniform rounding error has a standard deviation of 0.29 ulp: over the 600 elements of the smallest case
    here the mean's is 0.012 ulp, so 0.05 is four of them away.)"""
    s, n = sums
    print(f"  {name}: signed mean error {s / max(n, 1):+.4f} fp16 ulp over {n} of {total} elements (kept share {n / total:.2f})")
    if need_cover and total >= 2000:
        assert 2 * n >= total, f"{name}: the bias check covers {n} of {total} elements, less than half"
    assert n > 0, f"{name}: the bias check kept no element"
    assert abs(s / n) < 0.05, f"{name}: output rounding is biased ({s / n:+.4f} ulp): a truncating conversion?"


# ----------------------------------------------------------------------------- 1. LayerNorm pass of the residual stream
_WIDE = [(3, 1032, 1, True, 0, 40), (5, 1028, 1, False, 0, 0), (37, 1024, 0, True, 1, 0), (37, 1032, 1, False, 1, 40), (4097, 1024, 1, False, 0, 0)]
assert all(s in E._WIDE_SHAPES for s in _WIDE)


@pytest.mark.parametrize("shape", _WIDE, ids=lambda s: f"r{s[0]}-ld{s[1]}-wide{s[2]}-{'pb' if s[3] else 'mod0'}-one{s[4]}-off{s[5]}")
@pytest.mark.parametrize("inplace", [1, 0])
@pytest.mark.parametrize("ymode", [0, 1, 2, 3])
def test_layernorm_res_dim1024_against_fp64(ymode, inplace, shape):
    """dim 1024, fp16 stream, fp16 branches and output: layernorm1024_h_kernel<0..3, f16_t> where ldx % 8 == 0 and ln_wide is on, the generic
    layernorm_kernel<f16_t, ..., _Float16, _Float16> otherwise.  The written-back stream is bit-exact against clamp(v, +-65504).half()."""
    import gpu_helpers as G
    rows, ldx, wide, per_batch, add_one, offset = shape
    name = f"fp16 dim1024 ymode {ymode} inplace {inplace} rows {rows} ldx {ldx} wide {wide} per-batch {per_batch} add_one {add_one} offset {offset}"
    with G.knobs(ln_wide=wide):
        sums = E._run_ln_case(name, P_FP16, 1, 1, rows, 1024, ymode, add_one, per_batch, inplace, offset, ldx=ldx, seed=rows * 13 + ldx + ymode)
    _bias_check(name, sums, rows * 1024)


@pytest.mark.parametrize("pair", [(P_FP16, 0, 0), (P_FP16, 0, 1), (P_FP16, 1, 1)], ids=lambda p: f"fp16-in{'16' if p[1] else '32'}-out{'16' if p[2] else '32'}")
@pytest.mark.parametrize("dim", [128, 768, 1000, 2048])
def test_layernorm_res_generic_kernel_against_fp64(dim, pair):
    """layernorm_kernel<f16_t, ...> in its three storage forms (fp32 -> fp32, fp32 -> fp16, fp16 -> fp16 stream), full and partial rows, with the
    four-ymode rotation of the bf16 test."""
    prec, xi, xo = pair
    inplace = 1 if xi == xo else 0
    total = [0.0, 0]
    for k, ymode in enumerate((1, 3, 0, 2)):
        s = E._run_ln_case(f"fp16 dim {dim} {pair} ymode {ymode}", prec, xi, xo, 37, dim, ymode, k % 2, k < 2, inplace, 40 * (k % 2), seed=dim + k)
        _bias_check(f"fp16 dim {dim} {pair} ymode {ymode}", s, 37 * dim)  # each run of 37 x dim >= 4736 elements covers half of its own
        total[0] += s[0]
        total[1] += s[1]
    _bias_check(f"fp16 dim {dim} {pair}", total, 4 * 37 * dim)


@pytest.mark.parametrize("rows", [7, 9, 17])
@pytest.mark.parametrize("ln_rows", [2, 4])
def test_layernorm_rows_kernel_equals_one_row_kernel(ln_rows, rows):
    """layernorm1024_h_rows_kernel<2 | 4, f16_t> (threshold lowered to 1 row) bit for bit against the one-row 16-byte kernel in fp16 mode, and
    within the bound."""
    import gpu_helpers as G
    out, one, ref, scale = E._rows_case(rows, rows * 31 + ln_rows, ln_rows, 1, add_one=rows % 2, prec=P_FP16)
    assert torch.equal(out, one), f"rows kernel ({ln_rows} per wave, {rows} rows) differs from the one-row kernel in {(out != one).sum()} elements"
    _, sums = G.check_rounded(f"fp16 rows kernel {ln_rows} x {rows}", out, ref, scale, P_FP16)
    _bias_check(f"fp16 rows kernel {ln_rows} x {rows}", sums, rows * 1024)


def test_layernorm_rows_kernel_default_threshold():
    """The production dispatch (ln_rows 2, ln_rows_min 16384) at 16384 rows in fp16 mode."""
    import gpu_helpers as G
    out, one, ref, scale = E._rows_case(16384, 16384, 2, 16384, prec=P_FP16)
    assert torch.equal(out, one)
    _, sums = G.check_rounded("fp16 default dispatch, 16384 rows", out, ref, scale, P_FP16)
    _bias_check("fp16 default dispatch, 16384 rows", sums, 16384 * 1024)


def test_layernorm_res_refusals():
    """fp16 mode: an fp16 -> fp32 write-back (ymode 1 or 3) is refused by the launcher with F5_EINVAL; the same storage with ymode 2 is built."""
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    for ymode in (1, 3):
        rc = G.op_layernorm_res_rc(P_FP16, 1, 0, 8, 1024, ymode, 0, 1024)
        assert rc == -1, f"ymode {ymode}: expected F5_EINVAL, got {rc} ({_lib.last_error()})"
        assert "layernorm" in _lib.last_error(), f"ymode {ymode}: refused by the op, not by the launcher: {_lib.last_error()}"
    assert G.op_layernorm_res_rc(P_FP16, 1, 0, 8, 1024, 2, 0, 1024) == 0


# ----------------------------------------------------------------------------- 2. the range guard inside the fp16-output kernels
@pytest.mark.parametrize("kernel,case", E._GUARD_GRID)
def test_range_guard_fires_at_the_fp16_limit(kernel, case):
    """The grid of the bf16 test in fp16 mode.  The branch values that form the offending element (64, 32, 4608 added to 65440) are exact in
    fp16.  An infinite branch element does not reach an fp16-mode kernel as inf -- the staging store saturates it --, so the write-back
    kernels form 65440 + 65504 and word 1 holds exactly that; a NaN branch element stays a NaN, fires and sets word 2."""
    value, fires = E._GUARD_CASES[case]
    rows, r = 12, 9
    x, y, y2, ymode, out, xb, guard = E._guard_run(kernel, rows, [r], value, prec=P_FP16)
    v = E._formed(x, y, y2, ymode)
    print(f"  fp16 {kernel} {case}: guard words {[hex(w) for w in guard]}")
    if not fires:
        assert guard == [0] * 6, f"{kernel}: {case} fired the guard: {guard}"
    else:
        assert guard[0] == 1, f"{kernel}: {case} did not fire the guard"
        amax = E._bits_f(guard[1])
        assert math.isfinite(amax), f"word 1 holds a non-finite value: {guard[1]:#x}"
        if math.isfinite(value):
            assert guard[1] == E._fbits(abs(value)), f"word 1: {amax} for a formed {value}"
        elif math.isinf(value) and ymode != 0:
            assert guard[1] == E._fbits(65440.0 + F16_MAX), f"word 1: {amax} for 65440 + a branch element saturated to 65504"
        assert guard[2] == (1 if math.isnan(value) else 0)
        assert guard[3] == 1 << (E._TAG & 15) and guard[4] == 1 << (E._TAG >> 4)
        assert guard[5] == 0x7fffffff - r
    if ymode != 0:  # the stored stream: saturated, never inf
        want = _f16(v.clamp(-F16_MAX, F16_MAX))
        keep = ~torch.isnan(v)
        assert torch.equal(xb[keep], want[keep]), f"{kernel} {case}: written-back stream differs from clamp(v).half()"
        assert torch.isfinite(xb[keep]).all()
    else:
        assert torch.equal(xb[~torch.isnan(x)], x[~torch.isnan(x)])
    ok = torch.ones(rows, dtype=torch.bool)
    ok[r] = False
    assert torch.isfinite(out[ok]).all()


@pytest.mark.parametrize("kernel", list(E._GUARD_KERNELS))
def test_range_guard_reports_the_smallest_offending_row(kernel):
    _, _, _, _, _, _, guard = E._guard_run(kernel, 64, [40, 5], F16_MAX, prec=P_FP16)
    assert guard[0] == 1 and guard[5] == 0x7fffffff - 5, [hex(w) for w in guard]


@pytest.mark.parametrize("rows", [9, 17, 18])
@pytest.mark.parametrize("kernel", ["rows2", "rows4"])
def test_range_guard_rows_kernel_tail(kernel, rows):
    _, _, _, _, _, _, guard = E._guard_run(kernel, rows, [rows - 1], F16_MAX, prec=P_FP16)
    assert guard[0] == 1 and guard[5] == 0x7fffffff - (rows - 1), [hex(w) for w in guard]
    _, _, _, _, _, _, guard = E._guard_run(kernel, rows, [], F16_MAX, prec=P_FP16)
    assert guard == [0] * 6


# ----------------------------------------------------------------------------- 4. the other row-wise kernels
def _qknorm_inputs(heads, rope_heads, g, rpb=37, B=3):
    rows, inner = rpb * B, heads * 64
    qkv = _f16(torch.randn(rows, 3 * inner, generator=g) * (0.5 + 3 * torch.rand(rows, 1, generator=g)))
    wq, wk = 1 + 0.3 * torch.randn(64, generator=g), 1 + 0.3 * torch.randn(64, generator=g)
    return qkv, wq, wk, E._rope_table(rpb, g), rpb


@pytest.mark.parametrize("heads,rope_heads", [(1, 1), (12, 1), (16, 16), (12, 0)])
def test_qknorm_rope_against_fp64(heads, rope_heads):
    import gpu_helpers as G
    g = torch.Generator().manual_seed(heads * 10 + rope_heads + P_FP16)
    qkv, wq, wk, rope, rpb = _qknorm_inputs(heads, rope_heads, g)
    rows, inner = qkv.shape[0], heads * 64
    out = G.op_qknorm_rope(P_FP16, qkv, heads, rope_heads, rpb, wq, wk, rope)
    assert torch.equal(out[:, 2 * inner:], qkv[:, 2 * inner:]), "the v third changed"
    ref, sc = E._qknorm_ref(qkv, wq, wk, rope, heads, rope_heads, rpb)
    name = f"qknorm fp16 heads {heads} rope_heads {rope_heads}"
    _, sums = G.check_rounded(name, out[:, :2 * inner].reshape(rows, 2, heads, 64), ref, sc, P_FP16)
    _bias_check(name, sums, ref.numel())


def _dwconv_inputs(N, C, g, B=3):
    x = E._utterances(B, N, C, g)
    wt, cb = torch.randn(7, C, generator=g) * 0.4, torch.randn(C, generator=g)
    lw, lb = 1 + 0.3 * torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    return x, wt, cb, lw, lb


@pytest.mark.parametrize("C", [512, 328])
@pytest.mark.parametrize("N", [1, 7, 8, 300])
def test_dwconv7_ln_against_fp64(N, C):
    """dwconv7_ln_kernel<f16_t, 4, false>: fp32 input, fp16 output; three utterances of different level."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(N * 7 + C + P_FP16)
    x, wt, cb, lw, lb = _dwconv_inputs(N, C, g)
    out = G.op_dwconv7_ln(P_FP16, x, wt, cb, lw, lb)
    ref, scale = E._dwconv7_ln_ref(x, wt, cb, lw, lb)
    name = f"dwconv7_ln fp16 N {N} C {C}"
    _, sums = G.check_rounded(name, out, ref, scale, P_FP16)
    _bias_check(name, sums, ref.numel())


@pytest.mark.parametrize("C", [1024, 328])
@pytest.mark.parametrize("N", [1, 7, 300])
def test_grn_against_fp64(N, C):
    """grn_sumsq_kernel<f16_t> + grn_apply_kernel<f16_t> (in place on fp16 rows).  The slack is taken 4 times wider, as in the bf16 test (the
    sum of squares over the sequence and the mean over the channels sit in front of every element), which thins the set the bias check keeps:
    its share is printed from the reference, and the bias is asserted where at least 1000 elements are kept."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(N * 3 + C + P_FP16)
    h = _f16(E._utterances(3, N, C, g))
    gamma, beta = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
    out = G.op_grn(P_FP16, h, gamma, beta)
    ref, scale = E._grn_ref(h, gamma, beta)
    name = f"grn fp16 N {N} C {C}"
    _, sums = G.check_rounded(name, out, ref, scale * 4, P_FP16)
    print(f"  {name}: the bias check keeps {sums[1]} of {ref.numel()} elements (share {sums[1] / ref.numel():.2f})")
    if sums[1] >= 1000:
        _bias_check(name, sums, ref.numel(), need_cover=False)


@pytest.mark.parametrize("rows,dim", [(1, 1024), (37, 1024), (7, 100)])
def test_rmsnorm_against_fp64(rows, dim):
    """rmsnorm_kernel<f16_t>, the construction of the bf16 test: row rows // 2 is all zero and stays zero (with one row that is the row)."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(rows + dim + P_FP16)
    x = torch.randn(rows, dim, generator=g) * (0.1 + 5 * torch.rand(rows, 1, generator=g))
    x[rows // 2] = 0.0
    gw = 1 + 0.3 * torch.randn(dim, generator=g)
    out = G.op_rmsnorm(P_FP16, x, gw)
    assert torch.equal(out[rows // 2], torch.zeros(dim)), "an all-zero row must stay zero"
    ref = E._rmsnorm_ref(x, gw)
    name = f"rmsnorm fp16 rows {rows} dim {dim}"
    _, sums = G.check_rounded(name, out, ref, ref.abs(), P_FP16)
    _bias_check(name, sums, ref.numel())


# ----------------------------------------------------------------------------- 4. saturation
# One gain or modulation value is scaled so that exactly ONE known output element has an fp64 reference of about +-70000: that element is
# stored as +-65504, never inf, and every other element stays within its bound.  The element is made an outlier of its row first, so that
# the scaled gain leaves the other rows of its column inside the range; "exactly one" is asserted from the reference.
TARGET = 70000.0


def _check_saturated(name, out, ref, scale, where, sign):
    import gpu_helpers as G
    beyond = ref.abs() > F16_MAX
    assert int(beyond.sum()) == 1 and bool(beyond[where]), f"{name}: the construction must put exactly the element {where} beyond +-65504"
    assert ref[where] * sign > F16_MAX
    assert torch.isfinite(out).all(), f"{name}: a non-finite value was stored"
    assert float(out[where]) == sign * F16_MAX, f"{name}: the out-of-range element was stored as {float(out[where])}"
    ref = ref.clone()
    ref[where] = sign * F16_MAX
    G.check_rounded(name, out, ref, scale, P_FP16)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
@pytest.mark.parametrize("dim,ldx", [(768, 768), (1024, 1024)], ids=["generic_kernel", "wide_kernel"])
def test_layernorm_output_saturates(dim, ldx, sign):
    import gpu_helpers as G
    g = torch.Generator().manual_seed(dim)
    rows, r, c = 9, 5, 301
    x = E._stream(rows, dim, 0, g)
    x[r, c] = _f16(x[r].mean() + 25 * x[r].std())  # normalised value near 20, the other rows of the column stay below 5
    mul, add = E._mods(rows, dim, 0, 0, g)
    n = E._ln_ref(x, torch.zeros(dim), torch.zeros(dim), 0, rows, 1)[0][r, c]
    mul[c] = float((sign * TARGET - add[c].double()) / n - 1.0)
    out, xb, guard = G.op_layernorm_res(P_FP16, x, None, None, 0, mul, add, 0, 0, 1, 1, 1, 1, ldx=ldx, ldy=ldx, ldo=ldx)
    ref, scale = E._ln_ref(x, mul, add, 0, rows, 1)
    assert torch.equal(xb, x) and guard == [0] * 6  # the guard watches the stream, not the activation
    _check_saturated(f"layernorm dim {dim} saturating {sign:+.0f}", out, ref, scale, (r, c), sign)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
def test_rmsnorm_output_saturates(sign):
    import gpu_helpers as G
    g = torch.Generator().manual_seed(3)
    rows, dim, r, c = 9, 1024, 4, 77
    x = torch.randn(rows, dim, generator=g) * (0.1 + 5 * torch.rand(rows, 1, generator=g))
    x[r, c] = 25 * x[r].std()
    gw = 1 + 0.3 * torch.randn(dim, generator=g)
    gw[c] = float(sign * TARGET / E._rmsnorm_ref(x, torch.ones(dim))[r, c])
    out = G.op_rmsnorm(P_FP16, x, gw)
    ref = E._rmsnorm_ref(x, gw)
    _check_saturated(f"rmsnorm saturating {sign:+.0f}", out, ref, ref.abs(), (r, c), sign)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
def test_qknorm_rope_output_saturates(sign):
    """The q weight of one feature is scaled; the element sits in a head that is not rotated (head 5 of 12, one RoPE head), so no pair partner
    carries the scaled value."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(5)
    heads, rope_heads, hd, lane, r = 12, 1, 5, 41, 50
    qkv, wq, wk, rope, rpb = _qknorm_inputs(heads, rope_heads, g)
    rows, inner = qkv.shape[0], heads * 64
    qkv[r, hd * 64 + lane] = _f16(30 * qkv[r, hd * 64:hd * 64 + 64].std())  # normalised value near 7.7 (of at most 8)
    n = E._qknorm_ref(qkv, torch.ones(64), wk, rope, heads, rope_heads, rpb)[0][r, 0, hd, lane]
    wq[lane] = float(sign * TARGET / n)
    out = G.op_qknorm_rope(P_FP16, qkv, heads, rope_heads, rpb, wq, wk, rope)
    assert torch.equal(out[:, 2 * inner:], qkv[:, 2 * inner:]), "the v third changed"
    ref, sc = E._qknorm_ref(qkv, wq, wk, rope, heads, rope_heads, rpb)
    # (the rotated head 0 carries the scaled weight of `lane` into its pair partner too: both stay in range, the helper asserts it)
    _check_saturated(f"qknorm saturating {sign:+.0f}", out[:, :2 * inner].reshape(rows, 2, heads, 64), ref, sc, (r, 0, hd, lane), sign)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
def test_dwconv7_ln_output_saturates(sign):
    """Channel c keeps its centre tap only, so the outlier frame does not spread over its six neighbours; its LayerNorm weight is scaled."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(7)
    N, C, b, n0, c = 40, 328, 1, 17, 99
    x, wt, cb, lw, lb = _dwconv_inputs(N, C, g)
    wt[:, c] = 0.0
    wt[3, c] = 1.0
    x[b, n0, c] = 400.0  # an outlier of its row (utterance 1: level 6, spread 2): normalised value near 17, of at most sqrt(C - 1) = 18
    lw1 = lw.clone()
    lw1[c] = 1.0
    nrm = (E._dwconv7_ln_ref(x, wt, cb, lw1, lb)[0][b, n0, c] - lb[c].double())
    lw[c] = float((sign * TARGET - lb[c].double()) / nrm)
    out = G.op_dwconv7_ln(P_FP16, x, wt, cb, lw, lb)
    ref, scale = E._dwconv7_ln_ref(x, wt, cb, lw, lb)
    _check_saturated(f"dwconv7_ln saturating {sign:+.0f}", out, ref, scale, (b, n0, c), sign)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
def test_grn_output_saturates(sign):
    import gpu_helpers as G
    g = torch.Generator().manual_seed(11)
    N, C, b, n0, c = 40, 328, 2, 23, 200
    h = _f16(E._utterances(3, N, C, g))
    h[b, n0, c] = 120.0  # exact in fp16; 30 spreads of utterance 2
    gamma, beta = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
    g1 = gamma.clone()
    g1[c] = 1.0
    hnx = E._grn_ref(h, g1, torch.zeros(C))[0][b, n0, c] - h[b, n0, c].double()  # h Nx of the element
    gamma[c] = float((sign * TARGET - beta[c].double() - h[b, n0, c].double()) / hnx)
    out = G.op_grn(P_FP16, h, gamma, beta)
    ref, scale = E._grn_ref(h, gamma, beta)
    _check_saturated(f"grn saturating {sign:+.0f}", out, ref, scale * 4, (b, n0, c), sign)


# ----------------------------------------------------------------------------- 3. a NaN survives every fp16 activation store
@pytest.mark.parametrize("kernel", [0, 1], ids=["tile_kernel", "tuned_kernel"])
def test_linear_propagates_nan(kernel):
    """One NaN in A[r, 0]: row r of the product is NaN in every column (the staging store of A into fp16 must keep it), every other row is
    within its bound."""
    import gpu_helpers as G
    from test_gpu_fp16_ops import _linear_ref, _problem, check_f16
    M, N, K, r = 77, 512, 640, 33
    _, A, W, b = _problem(M, N, K, M + N + K)
    ref, scale = _linear_ref(A, W, b, "none")
    A[r, 0] = math.nan
    out = G.op_linear(P_FP16, kernel, A, W, b)
    assert out[r].isnan().all(), f"row {r} holds {int((~out[r].isnan()).sum())} numbers (first {float(out[r, 0])}): the NaN was lost"
    ok = torch.arange(M) != r
    check_f16(f"linear kernel {kernel} beside a NaN row", out[ok], ref[ok], scale[ok])


def test_rmsnorm_propagates_nan():
    import gpu_helpers as G
    g = torch.Generator().manual_seed(1)
    rows, dim, r = 9, 1024, 6
    x = torch.randn(rows, dim, generator=g)
    gw = 1 + 0.3 * torch.randn(dim, generator=g)
    ref = E._rmsnorm_ref(x, gw)
    x[r, 500] = math.nan
    out = G.op_rmsnorm(P_FP16, x, gw)
    assert out[r].isnan().all(), f"row {r} holds {int((~out[r].isnan()).sum())} numbers (first {float(out[r, 0])}): the NaN was lost"
    ok = torch.arange(rows) != r
    assert torch.isfinite(out[ok]).all(), f"the NaN leaked into another row: {int((~torch.isfinite(out[ok])).sum())} non-finite elements beside row {r}"
    G.check_rounded("rmsnorm beside a NaN row", out[ok], ref[ok], ref[ok].abs(), P_FP16)
