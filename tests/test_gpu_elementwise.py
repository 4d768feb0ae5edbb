"""Op-level parity of the row-wise kernels of the bf16 path against fp64 (through the test entry points of include/f5hip.h, which call the
production launchers): the LayerNorm pass of the residual stream in all its kernels (16-byte dim-1024 kernel, multi-row kernel, generic kernel),
the fp16 range guard inside them and inside the fp32 -> fp16 copy, qk_norm + RoPE, the ConvNeXtV2 depthwise conv + LayerNorm, GRN and RMSNorm.

Every reference is computed in fp64 from exactly the values the kernel read: the fp16-rounded stream, the bf16-rounded branches, and the
formed row v = (x + y) + y2 added in fp32 in that order (the kernels normalise v itself, not its fp16 rounding).  Bounds:
  fp16 write-back   bit-exact against clamp(v, +-65504).half()
  bf16 outputs      every element within 1 bf16 ulp of the reference + 8 fp32 ulps of the largest term the kernel evaluates for it, and a
                    signed mean error under 0.05 ulp (a truncating conversion sits near -0.5)
  fp32 outputs      within 1e-5 relative + the same slack
  multi-row kernel  bit-identical to the one-row 16-byte kernel (same arithmetic per row)
Run with -s to see the worst error of every case."""
import math
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu
P_BF16, P_FP32, P_FP16 = 0, 1, 2
F16_MAX = 65504.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _bias_check(name, sums):
    s, n = sums
    if n >= 1000:
        print(f"  {name}: signed mean error {s / n:+.4f} bf16 ulp over {n} elements")
        assert abs(s / n) < 0.05, f"{name}: output rounding is biased ({s / n:+.4f} ulp): a truncating conversion?"


def _f16(t):
    return t.half().float()


def _bf16(t):
    return t.to(torch.bfloat16).float()


# ----------------------------------------------------------------------------- LayerNorm pass of the residual stream
def _stream(rows, dim, offset, g, fp16=True):
    """Rows with their own mean (around `offset`) and spread: a kernel that reuses one row's statistics for another shows it."""
    mu = offset + torch.randn(rows, 1, generator=g) * (1 + 0.1 * offset)
    sd = 0.5 + 3 * torch.rand(rows, 1, generator=g)
    x = mu + torch.randn(rows, dim, generator=g) * sd
    return _f16(x) if fp16 else x


def _mods(rows, dim, mod_bstride, rows_per_batch, g):
    if mod_bstride:
        nb = -(-rows // rows_per_batch)
        mul, add = torch.randn(nb, mod_bstride, generator=g) * 0.5, torch.randn(nb, mod_bstride, generator=g)
    else:
        mul, add = torch.randn(dim, generator=g) * 0.5, torch.randn(dim, generator=g)
    return mul, add


def _ln_ref(v, mul, add, mod_bstride, rows_per_batch, add_one):
    """fp64 LayerNorm(eps 1e-6) of the formed rows v, times (add_one + mul) plus add; also the scale of the fp32 slack (largest term)."""
    rows, dim = v.shape
    vd = v.double()
    mean = vd.mean(1, keepdim=True)
    d = vd - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + 1e-6)
    if mod_bstride:
        b = torch.arange(rows) // rows_per_batch
        m, a = mul.double()[b, :dim], add.double()[b, :dim]
    else:
        m, a = mul.double()[None, :dim], add.double()[None, :dim]
    f = add_one + m
    out = d * rstd * f + a
    # largest fp32 term: the uncentred value (the mean is taken in fp32 next to it) through rstd and the modulation, or the shift
    scale = vd.abs().amax(1, keepdim=True) * rstd * f.abs() + a.abs()
    return out, scale


def _formed(x, y, y2, ymode):
    v = x.clone()
    if ymode != 0:
        v = v + y  # fp32, in the kernels' order
    if ymode == 3:
        v = v + y2
    return v


def _run_ln_case(name, prec, xin_f16, xout_f16, rows, dim, ymode, add_one, per_batch, inplace, offset, ldx=None, seed=0):
    import gpu_helpers as G
    g = torch.Generator().manual_seed(seed)
    x = _stream(rows, dim, offset, g, fp16=bool(xin_f16))
    y = torch.randn(rows, dim, generator=g) * 0.7
    y2 = torch.randn(rows, dim, generator=g) * 0.7
    if prec == P_BF16:
        y, y2 = _bf16(y), _bf16(y2)
    elif prec == P_FP16:
        y, y2 = _f16(y), _f16(y2)
    rpb = max(1, rows // 3) if per_batch else 0
    mbs = dim + 8 if per_batch else 0
    mul, add = _mods(rows, dim, mbs, rpb, g)
    out, xb, guard = G.op_layernorm_res(prec, x, y, y2, ymode, mul, add, mbs, rpb, add_one, inplace, xin_f16, xout_f16, ldx=ldx, ldy=ldx, ldo=ldx)
    v = _formed(x, y, y2, ymode)
    ref, scale = _ln_ref(v, mul, add, mbs, rpb or rows, add_one)
    _, sums = G.check_rounded(name, out, ref, scale, prec)
    # the written-back stream
    if ymode in (1, 3):
        want = _f16(v.clamp(-F16_MAX, F16_MAX)) if xout_f16 else v
    else:
        want = x if inplace else torch.zeros_like(x)
    assert torch.equal(xb, want), f"{name}: written-back stream differs"
    assert guard == [0] * 6, f"{name}: the range guard fired on an in-range stream: {guard}"
    return sums


# (rows, ldx, ln_wide, per-batch modulation, add_one, mean offset): every row count, leading dimension and knob value of the issue, with the
# modulation forms and the offsets spread over them
_WIDE_SHAPES = [(1, 1024, 1, False, 1, 0), (3, 1032, 1, True, 0, 40), (4, 1024, 1, True, 1, 40), (5, 1028, 1, False, 0, 0),
                (37, 1024, 0, True, 1, 0), (4097, 1032, 1, True, 1, 40), (37, 1028, 1, True, 0, 40), (5, 1024, 0, False, 1, 40),
                (4097, 1024, 1, False, 0, 0), (37, 1032, 1, False, 1, 40)]


@pytest.mark.parametrize("shape", _WIDE_SHAPES, ids=lambda s: f"r{s[0]}-ld{s[1]}-wide{s[2]}-{'pb' if s[3] else 'mod0'}-one{s[4]}-off{s[5]}")
@pytest.mark.parametrize("inplace", [1, 0])
@pytest.mark.parametrize("ymode", [0, 1, 2, 3])
def test_layernorm_res_dim1024_against_fp64(ymode, inplace, shape):
    """The production shape of the bf16 mode (dim 1024, fp16 stream, bf16 branches and output): the 16-byte kernel where ldx % 8 == 0 and
    ln_wide is on, the generic kernel otherwise (ldx 1028, ln_wide 0); the multi-row kernel stays out (its own threshold, 16384 rows)."""
    import gpu_helpers as G
    rows, ldx, wide, per_batch, add_one, offset = shape
    name = f"dim1024 ymode {ymode} inplace {inplace} rows {rows} ldx {ldx} wide {wide} per-batch {per_batch} add_one {add_one} offset {offset}"
    with G.knobs(ln_wide=wide):
        sums = _run_ln_case(name, P_BF16, 1, 1, rows, 1024, ymode, add_one, per_batch, inplace, offset, ldx=ldx, seed=rows * 13 + ldx + ymode)
    _bias_check(name, sums)


_PAIRS = [(P_FP32, 0, 0), (P_BF16, 0, 0), (P_BF16, 0, 1), (P_BF16, 1, 1)]


@pytest.mark.parametrize("pair", _PAIRS, ids=lambda p: f"{'bf16' if p[0] == P_BF16 else 'fp32'}-in{'16' if p[1] else '32'}-out{'16' if p[2] else '32'}")
@pytest.mark.parametrize("dim", [128, 512, 768, 1000, 1280, 2048])
def test_layernorm_res_generic_kernel_against_fp64(dim, pair):
    """The generic kernel (dim != 1024: F5TTS_Small, MMDiT) with every storage pair the launcher builds, full (dim = 256 MAXV) and partial rows."""
    prec, xi, xo = pair
    inplace = 1 if xi == xo else 0
    total = [0.0, 0]
    for k, ymode in enumerate((1, 3, 0, 2)):
        name = f"dim {dim} {pair} ymode {ymode}"
        s = _run_ln_case(name, prec, xi, xo, 37, dim, ymode, k % 2, k < 2, inplace, 40 * (k % 2), seed=dim + k)
        total[0] += s[0]
        total[1] += s[1]
    _bias_check(f"dim {dim} {pair}", total)


def _rows_case(rows, seed, ln_rows, ln_rows_min, add_one=1, prec=P_BF16):
    """In-place read-only pass (ymode 0, one modulation row): the multi-row kernel's form.  Returns (out, reference run of the one-row kernel)."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(seed)
    x = _stream(rows, 1024, 40 * (seed % 2), g)
    mul, add = _mods(rows, 1024, 0, 0, g)
    with G.knobs(ln_rows=ln_rows, ln_rows_min=ln_rows_min):
        out, xb, guard = G.op_layernorm_res(prec, x, None, None, 0, mul, add, 0, 0, add_one, 1)
    with G.knobs(ln_rows=1):
        one, _, _ = G.op_layernorm_res(prec, x, None, None, 0, mul, add, 0, 0, add_one, 1)
    assert torch.equal(xb, x) and guard == [0] * 6
    ref, scale = _ln_ref(x, mul, add, 0, rows, add_one)
    return out, one, ref, scale


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 15, 16, 17])
@pytest.mark.parametrize("ln_rows", [2, 4])
def test_layernorm_rows_kernel_equals_one_row_kernel(ln_rows, rows):
    """layernorm1024_h_rows_kernel (2 or 4 rows per wave; the threshold lowered to 1 row) against the one-row 16-byte kernel, bit for bit,
    at row counts around the wave's row group: the tail rows are computed on the last row and must not be stored."""
    import gpu_helpers as G
    out, one, ref, scale = _rows_case(rows, rows * 31 + ln_rows, ln_rows, 1, add_one=rows % 2)
    assert torch.equal(out, one), f"rows kernel ({ln_rows} per wave, {rows} rows) differs from the one-row kernel in {(out != one).sum()} elements"
    _, sums = G.check_rounded(f"rows kernel {ln_rows} x {rows}", out, ref, scale, P_BF16)
    _bias_check(f"rows kernel {ln_rows} x {rows}", sums)


@pytest.mark.parametrize("rows", [16383, 16384])
def test_layernorm_rows_kernel_default_threshold(rows):
    """The production dispatch (ln_rows 2, ln_rows_min 16384): one row below and at the threshold, both bit-identical to the one-row kernel."""
    import gpu_helpers as G
    out, one, ref, scale = _rows_case(rows, rows, 2, 16384)
    assert torch.equal(out, one)
    _, sums = G.check_rounded(f"default dispatch, {rows} rows", out, ref, scale, P_BF16)
    _bias_check(f"default dispatch, {rows} rows", sums)


def test_layernorm_res_refusals():
    """The launcher refuses what it does not build, with F5_EINVAL, before any launch of its own."""
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    cases = [("dim % 4", (P_BF16, 1, 1, 8, 1022, 1, 1, 1024)), ("dim > 2048", (P_BF16, 0, 0, 8, 2052, 1, 1, 2052)),
             ("fp16 stream, fp32 output", (P_FP32, 1, 1, 8, 1024, 1, 1, 1024)), ("fp16 stream in, fp32 out", (P_FP32, 0, 1, 8, 1024, 1, 0, 1024)),
             ("fp16 -> fp32 write-back", (P_BF16, 1, 0, 8, 1024, 1, 0, 1024)), ("fp16 -> fp32 write-back, ymode 3", (P_BF16, 1, 0, 8, 1024, 3, 0, 1024))]
    for what, (prec, xi, xo, rows, dim, ymode, inplace, ldx) in cases:
        rc = G.op_layernorm_res_rc(prec, xi, xo, rows, dim, ymode, inplace, ldx)
        assert rc == -1, f"{what}: expected F5_EINVAL, got {rc} ({_lib.last_error()})"
        assert "layernorm" in _lib.last_error(), f"{what}: refused by the op, not by the launcher: {_lib.last_error()}"
    # fp16 -> fp32 without a write-back (ymode 0 / 2) is built
    assert G.op_layernorm_res_rc(P_BF16, 1, 0, 8, 1024, 2, 0, 1024) == 0


# ----------------------------------------------------------------------------- fp16 range guard
def _fbits(f):
    return struct.unpack("I", struct.pack("f", f))[0]


def _bits_f(b):
    return struct.unpack("f", struct.pack("I", b & 0xffffffff))[0]


# kernel -> (ymode, knobs that select it)
_GUARD_KERNELS = {"wide": (1, {}), "wide_ro": (0, {"ln_rows": 1}), "rows2": (0, {"ln_rows": 2, "ln_rows_min": 1}),
                  "rows4": (0, {"ln_rows": 4, "ln_rows_min": 1}), "generic": (3, {"ln_wide": 0})}
_GUARD_CASES = {"65504": (F16_MAX, True), "-65504": (-F16_MAX, True), "65472": (65472.0, False), "-65472": (-65472.0, False),
                "70048": (70048.0, True), "-70048": (-70048.0, True), "inf": (math.inf, True), "-inf": (-math.inf, True), "nan": (math.nan, True)}
_TAG = 2 | (5 << 4)  # the second LayerNorm of block 5


def _guard_run(kernel, rows, offenders, value, prec=P_BF16):
    """Rows of an in-range stream with `value` formed at one element of each offending row.  Write-back kernels form it as x + y (or
    (x + y) + y2: generic), x = 65440 in the same place of every row; the read-only kernels read it from the stream itself."""
    import gpu_helpers as G
    ymode, kn = _GUARD_KERNELS[kernel]
    g = torch.Generator().manual_seed(rows)
    x = _stream(rows, 1024, 0, g)
    y = torch.zeros(rows, 1024)
    y2 = torch.zeros(rows, 1024)
    col = 517
    mul, add = _mods(rows, 1024, 0, 0, g)
    if ymode == 0:
        for r in offenders:
            x[r, col] = value
    else:
        x[:, col] = 65440.0 * (-1 if value < 0 else 1)
        br = y2 if ymode == 3 else y
        for r in offenders:
            br[r, col] = value - x[r, col] if math.isfinite(value) else value
        rnd = _bf16 if prec == P_BF16 else _f16
        assert torch.equal(rnd(br).nan_to_num(), br.nan_to_num())  # the branch values are exact in the branch type
    with G.knobs(**kn):
        out, xb, guard = G.op_layernorm_res(prec, x, y, y2, ymode, mul, add, 0, 0, 1, 1, 1, 1, sat_tag=_TAG)
    return x, y, y2, ymode, out, xb, guard


# (a read-only pass cannot be handed a formed value beyond 65504: the stream it reads saturates there)
_GUARD_GRID = [(k, c) for k in _GUARD_KERNELS for c in _GUARD_CASES if _GUARD_KERNELS[k][0] != 0 or "70048" not in c]


@pytest.mark.parametrize("kernel,case", _GUARD_GRID)
def test_range_guard_fires_at_the_fp16_limit(kernel, case):
    """A formed element of exactly +-65504 fires the guard, +-65472 (the next fp16 value below) in an otherwise equal row does not; a formed
    +-70048 is stored as +-65504, never inf; +-inf fires and leaves word 1 finite; NaN fires and sets word 2.  Word 3 carries the pass bit of
    sat_tag, word 4 the block bit, word 5 the offending row."""
    value, fires = _GUARD_CASES[case]
    rows, r = 12, 9
    x, y, y2, ymode, out, xb, guard = _guard_run(kernel, rows, [r], value)
    v = _formed(x, y, y2, ymode)
    print(f"  {kernel} {case}: guard words {[hex(w) for w in guard]}")
    if not fires:
        assert guard == [0] * 6, f"{kernel}: {case} fired the guard: {guard}"
    else:
        assert guard[0] == 1, f"{kernel}: {case} did not fire the guard"
        amax = _bits_f(guard[1])
        assert math.isfinite(amax), f"word 1 holds a non-finite value: {guard[1]:#x}"
        if math.isfinite(value):
            assert guard[1] == _fbits(abs(value)), f"word 1: {amax} for a formed {value}"
        assert guard[2] == (1 if math.isnan(value) else 0)
        assert guard[3] == 1 << (_TAG & 15) and guard[4] == 1 << (_TAG >> 4)
        assert guard[5] == 0x7fffffff - r
    if ymode != 0:  # the stored stream: saturated, never inf
        want = _f16(v.clamp(-F16_MAX, F16_MAX))
        keep = ~torch.isnan(v)
        assert torch.equal(xb[keep], want[keep]), f"{kernel} {case}: written-back stream differs from clamp(v).half()"
        assert torch.isfinite(xb[keep]).all()
    else:
        assert torch.equal(xb[~torch.isnan(x)], x[~torch.isnan(x)])
    # the rows that did not offend are normalised as usual
    ok = torch.ones(rows, dtype=torch.bool)
    ok[r] = False
    assert torch.isfinite(out[ok]).all()


@pytest.mark.parametrize("kernel", list(_GUARD_KERNELS))
def test_range_guard_reports_the_smallest_offending_row(kernel):
    """Rows 5 and 40 of 64 both offend: word 5 names row 5."""
    _, _, _, _, _, _, guard = _guard_run(kernel, 64, [40, 5], F16_MAX)
    assert guard[0] == 1 and guard[5] == 0x7fffffff - 5, [hex(w) for w in guard]


@pytest.mark.parametrize("rows", [9, 17, 18])
@pytest.mark.parametrize("kernel", ["rows2", "rows4"])
def test_range_guard_rows_kernel_tail(kernel, rows):
    """The multi-row kernel computes the rows past `rows` on the last row: an offending last row is reported as itself, never as a row
    past the end, and an in-range tail reports nothing."""
    _, _, _, _, _, _, guard = _guard_run(kernel, rows, [rows - 1], F16_MAX)
    assert guard[0] == 1 and guard[5] == 0x7fffffff - (rows - 1), [hex(w) for w in guard]
    _, _, _, _, _, _, guard = _guard_run(kernel, rows, [], F16_MAX)
    assert guard == [0] * 6


def _half_sat(t):
    return t.clamp(-F16_MAX, F16_MAX).half().float()


@pytest.mark.parametrize("n", [4, 1020, 4096 * 256 * 4 + 1028])
def test_f32_to_f16_against_torch(n):
    """The hoisted input-embedding copy: every in-range value equals torch's .half() bit for bit (normals, subnormals, underflow to zero);
    65519 rounds to 65504 and fires the guard (it is at or beyond the limit before rounding), 65520 saturates to 65504 (torch: inf) and fires;
    65503 rounds to 65504 without firing.  The largest n exceeds the 4096-block grid cap, so the grid-stride loop carries the offender."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=g) * 300
    if n >= 8:
        src[1:4] = torch.tensor([3e-5, -2.5e-7, 1e-9])  # fp16 subnormals and an underflow
    dst, guard = G.op_f32_to_f16(src)
    assert torch.equal(dst, src.half().float()) and guard == [0] * 6
    for value, fires in ((65503.0, False), (65519.0, True), (-65520.0, True), (F16_MAX, True), (1e6, True), (math.inf, True)):
        s = src.clone()
        s[n - 1] = value
        dst, guard = G.op_f32_to_f16(s)
        assert torch.equal(dst, _half_sat(s)), f"n {n}, {value}: stored {float(dst[n - 1])}"
        assert guard[0] == (1 if fires else 0), f"n {n}, {value}: guard {guard}"
        if fires:
            assert guard[3] == 1 and guard[4] == 1 and guard[5] == 0x7fffffff and math.isfinite(_bits_f(guard[1]))
            if math.isfinite(value):
                assert guard[1] == _fbits(abs(value))
    s = src.clone()
    s[n // 2] = math.nan
    _, guard = G.op_f32_to_f16(s)
    assert guard[0] == 1 and guard[2] == 1


# ----------------------------------------------------------------------------- qk_norm + RoPE
def _rope_table(seq, g):
    inv = 1.0 / (10000 ** (torch.arange(32).double() / 32))
    ang = torch.arange(seq).double()[:, None] * inv[None, :] + torch.rand(1, generator=g).double()
    return torch.stack([ang.cos(), ang.sin()], dim=-1).float()  # [seq][32][2]


def _qknorm_ref(qkv, wq, wk, rope, heads, rope_heads, rpb):
    """fp64 qk_norm + RoPE of the q and k thirds [rows, 2, heads, 64] and the scale of the fp32 slack."""
    rows, inner = qkv.shape[0], heads * 64
    x = qkv[:, :2 * inner].double().reshape(rows, 2, heads, 64)
    w = torch.stack([wq, wk]).double()[None, :, None, :]
    rs = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + 1e-6)
    y = x * rs * w
    scale = (x.abs().amax(-1, keepdim=True) * rs * w.abs()).expand_as(y).clone()
    cs = rope.double()[torch.arange(rows) % rpb]  # [rows, 32, 2]
    c, s = cs[..., 0][:, None, None, :], cs[..., 1][:, None, None, :]
    yr = y.reshape(rows, 2, heads, 32, 2)
    a0, a1 = yr[..., 0], yr[..., 1]
    rot = torch.stack([a0 * c - a1 * s, a1 * c + a0 * s], dim=-1).reshape(rows, 2, heads, 64)
    ref = y.clone()
    ref[:, :, :rope_heads] = rot[:, :, :rope_heads]
    sc = scale.reshape(rows, 2, heads, 32, 2).amax(-1, keepdim=True).expand(rows, 2, heads, 32, 2).reshape(rows, 2, heads, 64) * 2
    return ref, sc


@pytest.mark.parametrize("prec", [P_BF16, P_FP32])
@pytest.mark.parametrize("heads,rope_heads", [(1, 0), (1, 1), (12, 0), (12, 1), (12, 12), (16, 1), (16, 16)])
def test_qknorm_rope_against_fp64(heads, rope_heads, prec):
    """RMSNorm over the 64 features of every q and k head (eps 1e-6, per-feature weights), then the interleaved-pair rotation on the first
    rope_heads heads at position row % rows_per_batch (positions restart at every utterance); the v third comes back bit-unchanged."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(heads * 10 + rope_heads + prec)
    rpb, B = 37, 3
    rows, inner = rpb * B, heads * 64
    qkv = torch.randn(rows, 3 * inner, generator=g) * (0.5 + 3 * torch.rand(rows, 1, generator=g))
    wq, wk = 1 + 0.3 * torch.randn(64, generator=g), 1 + 0.3 * torch.randn(64, generator=g)
    rope = _rope_table(rpb, g)
    if prec == P_BF16:
        qkv = _bf16(qkv)
    out = G.op_qknorm_rope(prec, qkv, heads, rope_heads, rpb, wq, wk, rope)
    assert torch.equal(out[:, 2 * inner:], qkv[:, 2 * inner:]), "the v third changed"
    ref, sc = _qknorm_ref(qkv, wq, wk, rope, heads, rope_heads, rpb)
    name = f"qknorm {'bf16' if prec == P_BF16 else 'fp32'} heads {heads} rope_heads {rope_heads}"
    _, sums = G.check_rounded(name, out[:, :2 * inner].reshape(rows, 2, heads, 64), ref, sc, prec)
    _bias_check(name, sums)


# ----------------------------------------------------------------------------- ConvNeXtV2: depthwise conv k=7 + LayerNorm, GRN
def _utterances(B, N, C, g):
    """B utterances of very different level and spread: a window or a statistic that reads a neighbour shows it."""
    lvl = torch.tensor([0.0, 6.0, -3.0])[:B, None, None]
    sd = torch.tensor([0.5, 2.0, 4.0])[:B, None, None]
    return lvl + sd * torch.randn(B, N, C, generator=g)


def _dwconv7_ln_ref(x, wt, cb, lw, lb):
    """fp64 depthwise conv (7 taps, zero padding inside each utterance) + bias + LayerNorm(eps 1e-6, affine), and the scale of the fp32 slack."""
    N = x.shape[1]
    xp = torch.nn.functional.pad(x.double(), (0, 0, 3, 3))  # [B, N + 6, C]: zeros past both ends of each utterance
    a = cb.double() + sum(xp[:, t:t + N] * wt.double()[t] for t in range(7))
    mag = cb.double().abs() + sum(xp[:, t:t + N].abs() * wt.double()[t].abs() for t in range(7))
    mean = a.mean(-1, keepdim=True)
    d = a - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + 1e-6)
    ref = d * rstd * lw.double() + lb.double()
    scale = mag.amax(-1, keepdim=True) * rstd * lw.double().abs() + lb.double().abs()
    return ref, scale


@pytest.mark.parametrize("prec", [P_BF16, P_FP32])
@pytest.mark.parametrize("C", [512, 1024, 328])
@pytest.mark.parametrize("N", [1, 3, 7, 8, 300])
def test_dwconv7_ln_against_fp64(N, C, prec):
    """x f32 [3, N, C] -> depthwise conv (7 taps, zero padding inside each utterance: the window crosses both sequence ends for N < 7 and
    must never read the neighbouring utterance) + bias, then LayerNorm(eps 1e-6) with affine weights."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(N * 7 + C + prec)
    B = 3
    x = _utterances(B, N, C, g)
    wt, cb = torch.randn(7, C, generator=g) * 0.4, torch.randn(C, generator=g)
    lw, lb = 1 + 0.3 * torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    out = G.op_dwconv7_ln(prec, x, wt, cb, lw, lb)
    ref, scale = _dwconv7_ln_ref(x, wt, cb, lw, lb)
    name = f"dwconv7_ln {'bf16' if prec == P_BF16 else 'fp32'} N {N} C {C}"
    _, sums = G.check_rounded(name, out, ref, scale, prec)
    _bias_check(name, sums)


def _grn_ref(h, gamma, beta):
    """fp64 GRN over each utterance's own tokens and the sum of the magnitudes of its terms."""
    hd = h.double()
    Gx = torch.sqrt((hd * hd).sum(1, keepdim=True))
    nx = Gx / (Gx.mean(-1, keepdim=True) + 1e-6)
    ref = gamma.double() * (hd * nx) + beta.double() + hd
    scale = (gamma.double() * hd * nx).abs() + beta.double().abs() + hd.abs()
    return ref, scale


@pytest.mark.parametrize("prec", [P_BF16, P_FP32])
@pytest.mark.parametrize("C", [512, 1024, 328])
@pytest.mark.parametrize("N", [1, 7, 300])
def test_grn_against_fp64(N, C, prec):
    """GRN on [3, N, C]: G[b][c] = ||h[b, :, c]|| over the utterance's own tokens, Nx = G / (mean_c G + 1e-6), out = gamma (h Nx) + beta + h."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(N * 3 + C + prec)
    B = 3
    h = _utterances(B, N, C, g)
    if prec == P_BF16:
        h = _bf16(h)
    gamma, beta = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
    out = G.op_grn(prec, h, gamma, beta)
    ref, scale = _grn_ref(h, gamma, beta)
    name = f"grn {'bf16' if prec == P_BF16 else 'fp32'} N {N} C {C}"
    _, sums = G.check_rounded(name, out, ref, scale * 4, prec)
    _bias_check(name, sums)


# ----------------------------------------------------------------------------- RMSNorm (UNetT)
def _rmsnorm_ref(x, gw):
    xd = x.double()
    sc = math.sqrt(x.shape[1]) / torch.sqrt((xd * xd).sum(-1, keepdim=True)).clamp(min=1e-12)
    return xd * sc * gw.double()


@pytest.mark.parametrize("prec", [P_BF16, P_FP32])
@pytest.mark.parametrize("rows,dim", [(1, 1024), (6, 512), (37, 1024), (7, 100)])
def test_rmsnorm_against_fp64(rows, dim, prec):
    """out = x / max(||x||, 1e-12) sqrt(dim) g, rows not a multiple of the 4 rows of a workgroup; an all-zero row comes back zero."""
    import gpu_helpers as G
    g = torch.Generator().manual_seed(rows + dim + prec)
    x = torch.randn(rows, dim, generator=g) * (0.1 + 5 * torch.rand(rows, 1, generator=g))
    x[rows // 2] = 0.0
    gw = 1 + 0.3 * torch.randn(dim, generator=g)
    out = G.op_rmsnorm(prec, x, gw)
    assert torch.equal(out[rows // 2], torch.zeros(dim)), "an all-zero row must stay zero"
    ref = _rmsnorm_ref(x, gw)
    name = f"rmsnorm {'bf16' if prec == P_BF16 else 'fp32'} rows {rows} dim {dim}"
    _, sums = G.check_rounded(name, out, ref, ref.abs(), prec)
    _bias_check(name, sums)


# ----------------------------------------------------------------------------- the guard at the production width, end to end
SPIKE, BOOST = 32768.0, 49152.0  # both exact in bf16 and fp16


def _witness_weights(arch, V, boost):
    """Seeded F5TTS_Base-width weights with one feature column j of the residual stream under control: the input projection maps cond
    channel 0 to column j with weight SPIKE (only the frames whose cond channel 0 the test sets to 1 get it), and the last block's FF2 adds
    exactly `boost` to column j of every token row (its weight row j zeroed, its AdaLN gate_mlp for j pinned to 1 at every time).  The stream
    then leaves fp16's range after the last block exactly in the spiked rows: SPIKE + BOOST > 65504 > BOOST, SPIKE."""
    from oracle import cpu_ref
    W = cpu_ref.random_dit_weights(arch, V, seed=91)
    D, L, j = arch["dim"], arch["depth"] - 1, 300
    pre = f"transformer_blocks.{L}."
    for k in ("input_embed.proj.weight", pre + "attn_norm.linear.weight", pre + "attn_norm.linear.bias", pre + "ff.ff.2.weight", pre + "ff.ff.2.bias"):
        W[k] = W[k].clone()  # (the generator's results are shared by the session: edit copies)
    W["input_embed.proj.weight"][:, 100] *= 0.0
    W["input_embed.proj.weight"][j, 100] = SPIKE
    W[pre + "attn_norm.linear.weight"][5 * D + j] = 0.0  # gate_mlp (chunk 5 of the AdaLN row) of column j = its bias = 1
    W[pre + "attn_norm.linear.bias"][5 * D + j] = 1.0
    W[pre + "ff.ff.2.weight"][j] = 0.0
    W[pre + "ff.ff.2.bias"][j] = boost
    return W


@pytest.mark.parametrize("B,N", [(3, 700), (8, 1024)])
def test_range_guard_at_production_width(B, N):
    """dim 1024, 16 heads, depth 2, CFG 2: 4200 token rows (the final AdaLN pass takes the one-row 16-byte kernel) and 16384 (the multi-row
    kernel).  The stream leaves fp16's range only in the last block's FF2 update, which is no folded producer (dit_eval.hip: lnf_next), so the
    only pass that can see it is the final AdaLN pass, tag 3 (pass bit 3, block bit 0).  Asserted: exactly one fallback, the output equals a
    run with fp32 residual storage from the start bit for bit, the diagnostics name that pass and the smallest spiked row (cond half: row
    b N + n), and the same model without the boost never fires."""
    import warnings

    import bench
    import gpu_helpers as G
    arch = dict(bench.BASE_ARCH, depth=2)
    V = 300
    g = torch.Generator().manual_seed(B * N)
    nc = 60
    cond = torch.randn(B, nc, 100, generator=g) * 2 - 3
    cond[:, :, 0] = 0.0
    spikes = [(1, 37), (2, 5), (B - 1, 59)]
    for b, n in spikes:
        cond[b, n, 0] = 1.0
    text = torch.randint(0, V, (B, 40), generator=g)
    lens, dur = torch.full((B,), nc), torch.full((B,), N)
    y0 = torch.randn(B, N, 100, generator=g)
    kw = dict(cond=cond.cuda(), text=text.cuda(), duration=dur.cuda(), lens=lens.cuda(), steps=2, cfg_strength=2.0, sway_sampling_coef=-1.0,
              y0=y0, return_trajectory=False)

    ctrl = G.make_cfm(arch, V, _witness_weights(arch, V, 0.05), "bf16")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ctrl.sample(use_graph=False, **kw)
    assert ctrl.transformer.residual_fallbacks() == 0
    del ctrl

    W = _witness_weights(arch, V, BOOST)
    cfm = G.make_cfm(arch, V, W, "bf16")
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        out, _ = cfm.sample(use_graph=False, **kw)
    words = G.plan_guard_words(cfm.transformer)
    print(f"  {B} x {N} ({2 * B * N} token rows): {words}")
    assert words["residual_fallbacks"] == 1 and torch.isfinite(out).all()
    assert words["residual_guard_pass"] == 1 << 3, f"passes {words['residual_guard_pass']:#x}: only the final AdaLN pass can see the overflow"
    assert words["residual_guard_blocks"] == 1 and words["residual_guard_nan"] == 0
    assert words["residual_guard_row"] == min(b * N + n for b, n in spikes)
    assert _bits_f(words["residual_guard_amax_bits"]) == F16_MAX  # what the saturating FF2 store left in the stream
    del cfm
    with G.knobs(residual_f16=0):
        ref, _ = G.make_cfm(arch, V, W, "bf16").sample(use_graph=False, **kw)
    assert torch.equal(out, ref)
    torch.cuda.empty_cache()
