"""BigVGAN at the production widths and over the config space `f5_bigvgan_create` accepts.

`BIGVGAN_TINY` (upsample_initial_channel 192: snake widths 96 .. 3) never reaches `bv_aa_snake_kernel<64, ...>`, which carries the 768-, 384- and
192-channel stages of the published model, and uses one (k, u) family, three AMP blocks and 100 mels only.  This module pins

a. the anti-aliased snake kernel alone (`f5_op_bigvgan_snake`, the launch `bv_snake` makes for one utterance) against a float64 restatement of its
   documented formula, element by element, over C in {3, 32, 33, 64, 96, 128, 192, 768} x T in {1, 2, 5, 6, 7, 31, 32, 33, 64, 70}: both
   instantiations, 1 / 2 / 3 / 12 channel blocks of the 64-wide one, a partial channel block, replicate clamps that meet from both sides, tiles
   that end at, before and after T.  The explicit filters are ASYMMETRIC and differ between up- and down-sampling, so a reversed or swapped tap
   index shows (the Kaiser-sinc filters are symmetric and would hide it); the restatement is itself checked against `cpu_ref._aa_snake`.
   Bound, per element: |gpu - ref64| <= 4 E32 + 2^-23 max|ref64|, E32 = the largest error of `cpu_ref._aa_snake` in float32 on the same input
   (4 x: two fp32 evaluations of one 18-tap graph that differ in summation order, FMA use and the sine).  `out` is NaN-filled with a guard row
   on either side, `x` has NaN guard rows too.
b. the ragged form (`f5_op_bigvgan_snake_ragged`: the `UttExtents` path with its tables of 64): every utterance bit-identical to the
   one-utterance op on its own rows, and unchanged when every other row of the input is NaN.
c. one- and two-stage networks at the widths of the published model and at the corners of the accepted config space, through `BigVGAN(hp)` and
   the ragged decode, against `cpu_ref.bigvgan_forward` in float64.  Bounds: fewer than 1 % of |ref64| at 0.999 (a condition on the reference);
   rel-L2(gpu, ref64) <= 8 x rel-L2(fp32 oracle, ref64) and <= 1e-4; max|gpu - ref64| <= 8 x max|fp32 oracle - ref64| + 2^-23 max|ref64|
   (8 x: two fp32 runs of a deep network with K up to 3072 in different summation orders).  The fp32 oracle's deviations are computed on
   every run.
d. the refusal of a transposed convolution with k > 3u (`F5_ENOTSUP`): its scatter would need a gather row the workspace does not have.

Measured on MI355X (error / bound, so 1.0 is the limit):
a. worst over T per (C, input): 0.23 .. 0.55; the largest are 0.552 (C = 3, ramp: 32-wide kernel) and 0.536 (C = 192, large sine arguments: 64-wide
   kernel); with the library's own taps at most 0.393.
c. rel-L2(gpu) / rel-L2(fp32 oracle) = 1.30 .. 2.78 against the bound of 8 (absolute 8.5e-8 .. 3.3e-6, far below 1e-4); largest sample error
   0.125 .. 0.362 of its bound; w768 is the largest in both.  No probe's reference reaches 0.999.
"""
import ctypes as C
import math

import pytest
import torch

from conftest import rel_l2
from oracle import cpu_ref

gpu = pytest.mark.gpu
F5_ENOTSUP = -5
NAN_BITS = 0x7FC00000
EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- a. the snake kernel
SNAKE_C = [3, 32, 33, 64, 96, 128, 192, 768]
SNAKE_T = [1, 2, 5, 6, 7, 31, 32, 33, 64, 70]
KINDS = ["randn", "large", "ramp"]


def snake_ref64(x, a, invb, up_f, dn_f):
    """The kernel's documented formula in float64.  x [T, C]; a, invb [C]; 12 taps each.  xpad = x replicate-padded by 5;
    w[n] = 2 sum_m xpad[m] up_f[n + 15 - 2m] (n in [0, 2T): the 2x polyphase up-sampling, times 2); z = w + invb sin^2(w a);
    out[t] = sum_j z[clamp(2t + j - 5, 0, 2T - 1)] dn_f[j] (replicate padding 5 left, 6 right; 12 taps, stride 2)."""
    x, a, invb, up_f, dn_f = (v.double() for v in (x, a, invb, up_f, dn_f))
    T = x.shape[0]
    xpad = x[(torch.arange(T + 10) - 5).clamp(0, T - 1)]
    n = torch.arange(2 * T)
    w = torch.zeros(2 * T, x.shape[1], dtype=torch.float64)
    for tap in range(12):
        ns = n[(n + 15 - tap) % 2 == 0]
        w[ns] += xpad[(ns + 15 - tap) // 2] * up_f[tap]
    w = 2.0 * w
    z = w + invb * torch.sin(w * a) ** 2
    out = torch.zeros_like(x)
    for j in range(12):
        out += z[(2 * torch.arange(T) + j - 5).clamp(0, 2 * T - 1)] * dn_f[j]
    return out


def _oracle_snake(x, a, beta, up_f, dn_f):
    """cpu_ref._aa_snake ([b, C, T], alpha / beta not in log scale) on a time-major [T, C] input, in the dtype of x"""
    return cpu_ref._aa_snake(x.t()[None], a, beta, up_f, dn_f, False)[0].t()


def _snake_case(C_, T, kind, seed=0):
    """x [T, C], a, beta, invb (fp32; invb = 1 / (beta + 1e-9f) in fp32, as the library's upload computes it) and asymmetric filters"""
    g = torch.Generator().manual_seed(1000 * C_ + 10 * T + KINDS.index(kind) + seed)
    a = torch.exp(torch.randn(C_, generator=g) * 0.3)
    beta = torch.exp(torch.randn(C_, generator=g) * 0.3)
    if kind == "randn":
        x = torch.randn(T, C_, generator=g)
    elif kind == "large":  # sine arguments in the hundreds
        x = torch.randn(T, C_, generator=g) * 50
        a = torch.exp(torch.rand(C_, generator=g) * 4 - 2)
    else:  # a ramp whose first and last rows are outliers: a clamp to the wrong row shows
        x = torch.arange(T, dtype=torch.float32)[:, None] * 0.05 + torch.arange(C_, dtype=torch.float32)[None] * 0.002 - 0.5
        x[0] = 100.0
        x[-1] = -100.0
    invb = 1.0 / (beta + 1e-9)
    base = cpu_ref.kaiser_sinc_filter1d(0.25, 0.3, 12)
    up_f = base * (1 + 0.2 * torch.randn(12, generator=g))
    dn_f = base * (1 + 0.2 * torch.randn(12, generator=g))
    return x, a, beta, invb, up_f / up_f.sum(), dn_f / dn_f.sum()


def _taps(f):
    return None if f is None else (C.c_float * 12)(*[float(v) for v in f])


def _guarded(rows, cols, fill=None):
    """[rows + 2, cols] on the GPU, all NaN; returns (buffer, the contiguous view of rows 1 .. rows)"""
    buf = torch.full((rows + 2, cols), float("nan"), device="cuda")
    if fill is not None:
        buf[1:-1] = fill.cuda()
    return buf, buf[1:-1]


def _guards_intact(buf):
    bits = buf.view(torch.int32)
    return bool((bits[0] == NAN_BITS).all()) and bool((bits[-1] == NAN_BITS).all())


def _run_snake(lib, x, a, invb, up_f, dn_f):
    """f5_op_bigvgan_snake on x [T, C] (host tensors) -> out [T, C] on the host; asserts that the guard rows of out keep their bits"""
    from eraxvif5tts_amd import _lib
    T, C_ = x.shape
    xbuf, xd = _guarded(T, C_, x)
    obuf, od = _guarded(T, C_)
    ad, ibd = a.cuda(), invb.cuda()
    _lib.check(lib.f5_op_bigvgan_snake(T, C_, _lib.ptr(xd), _lib.ptr(ad), _lib.ptr(ibd), _taps(up_f), _taps(dn_f), _lib.ptr(od), _lib.stream_ptr()),
               "f5_op_bigvgan_snake")
    torch.cuda.synchronize()
    assert _guards_intact(obuf), f"C = {C_}, T = {T}: a guard row of out was written"
    return od.cpu()


def test_snake_reference_matches_the_oracle_in_float64():
    """The float64 restatement used below == cpu_ref._aa_snake (conv_transpose1d / conv1d form) in float64, with asymmetric filters and at the
    lengths where both replicate clamps meet."""
    for C_, T, kind in ((3, 1, "randn"), (5, 2, "ramp"), (4, 5, "large"), (33, 6, "randn"), (7, 7, "ramp"), (2, 70, "large")):
        x, a, beta, invb, up_f, dn_f = _snake_case(C_, T, kind)
        mine = snake_ref64(x, a, invb, up_f, dn_f)
        beta64 = 1.0 / invb.double() - 1e-9  # so that the oracle's 1 / (beta + 1e-9) is the fp32-rounded invb
        theirs = _oracle_snake(x.double(), a.double(), beta64, up_f.double(), dn_f.double())
        assert mine.shape == theirs.shape == (T, C_)
        assert float((mine - theirs).abs().max()) <= 1e-12 * float(theirs.abs().max()), (C_, T, kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C_", SNAKE_C)
def test_snake_op_matches_fp64_per_element(lib, C_, kind):
    worst = 0.0
    for T in SNAKE_T:
        x, a, beta, invb, up_f, dn_f = _snake_case(C_, T, kind)
        runs = [("own taps", up_f, dn_f, up_f, dn_f)]
        if kind == "randn":  # null filters = the library's Bessel-series Kaiser-sinc, against the taps torch computes in float64
            k64 = cpu_ref.kaiser_sinc_filter1d(0.25, 0.3, 12, dtype=torch.float64).float()
            runs.append(("library taps", None, None, k64, k64))
        for what, gu, gd, ru, rd in runs:
            ref = snake_ref64(x, a, invb, ru, rd)
            e32 = float((_oracle_snake(x, a, beta, ru, rd).double() - ref).abs().max())
            got = _run_snake(lib, x, a, invb, gu, gd)
            assert bool(torch.isfinite(got).all()), (C_, T, what)
            err = (got.double() - ref).abs()
            bound = 4 * e32 + EPS32 * float(ref.abs().max())
            ratio = float(err.max()) / bound
            worst = max(worst, ratio)
            print(f"snake C = {C_} T = {T} {kind} ({what}): max err {float(err.max()):.3e}, E32 {e32:.3e}, bound {bound:.3e}, ratio {ratio:.3f}")
            assert float(err.max()) <= bound, (C_, T, kind, what, float(err.max()), bound)
    print(f"snake C = {C_} {kind}: worst ratio to the bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- b. the ragged snake op
def _run_snake_ragged(lib, frames, up, x, a, invb, up_f, dn_f):
    from eraxvif5tts_amd import _lib
    rows, C_ = x.shape
    assert rows == sum(frames) * up
    xbuf, xd = _guarded(rows, C_, x)
    obuf, od = _guarded(rows, C_)
    ad, ibd = a.cuda(), invb.cuda()
    _lib.check(lib.f5_op_bigvgan_snake_ragged(len(frames), (C.c_int32 * len(frames))(*frames), up, C_, _lib.ptr(xd), _lib.ptr(ad), _lib.ptr(ibd),
                                              _taps(up_f), _taps(dn_f), _lib.ptr(od), _lib.stream_ptr()), "f5_op_bigvgan_snake_ragged")
    torch.cuda.synchronize()
    assert _guards_intact(obuf)
    return od.cpu()


RAGGED_CASES = [([1, 2, 33, 7], up, C_) for up in (1, 4) for C_ in (64, 128, 96, 192, 768)]
RAGGED_CASES.append(([1 + (7 * i) % 9 for i in range(70)], 2, 128))  # 70 utterances: two tables (64 + 6)


@gpu
@pytest.mark.parametrize("frames,up,C_", RAGGED_CASES, ids=[f"{len(f)}utt-up{u}-C{c}" for f, u, c in RAGGED_CASES])
def test_ragged_snake_op_is_the_one_utterance_op_per_utterance(lib, frames, up, C_):
    """Bit-identical to f5_op_bigvgan_snake on each utterance alone (so part a's bound holds for the ragged form too); NaN in every row that is not
    the utterance's own changes none of its bits."""
    _, a, _, invb, up_f, dn_f = _snake_case(C_, 1, "randn", seed=7)
    rows = sum(frames) * up
    x = torch.randn(rows, C_, generator=torch.Generator().manual_seed(rows + C_))
    got = _run_snake_ragged(lib, frames, up, x, a, invb, up_f, dn_f)
    assert bool(torch.isfinite(got).all())
    r = 0
    alone = 0
    for i, t in enumerate(frames):
        n = t * up
        one = _run_snake(lib, x[r: r + n], a, invb, up_f, dn_f)
        assert torch.equal(got[r: r + n], one), (i, t)
        if len(frames) <= 8 or i in (0, 1, 62, 63, 64, 65, 69):  # around the table boundary of the long list
            dirty = torch.full_like(x, float("nan"))
            dirty[r: r + n] = x[r: r + n]
            assert torch.equal(_run_snake_ragged(lib, frames, up, dirty, a, invb, up_f, dn_f)[r: r + n], one), (i, t)
            alone += 1
        r += n
    assert alone >= min(len(frames), 7)


# ---------------------------------------------------------------------------------------------------------------- c. networks at the widths
def _hp(C0, rates, kernels, blocks, dil, mels, **kw):
    return dict(num_mels=mels, upsample_initial_channel=C0, upsample_rates=rates, upsample_kernel_sizes=kernels, resblock="1",
                resblock_kernel_sizes=blocks, resblock_dilation_sizes=[list(dil) for _ in blocks], activation="snakebeta",
                snake_logscale=True, use_tanh_at_final=False, use_bias_at_final=False, **kw)


PROBES = {
    "w1536": _hp(1536, [4], [8], [3], [1, 3, 5], 100),              # 768-channel snake; polyphase GEMM N = 3072, K = 3072
    "w768": _hp(768, [4], [8], [7], [1, 3, 5], 100),                # 384 channels; K = 7 x 384
    "w384": _hp(384, [2], [4], [11], [1, 3, 5], 100),               # 192 channels; K = 11 x 192
    "w256_two": _hp(256, [4, 2], [8, 4], [3, 7, 11], [1, 3, 5], 100),  # 128 then 64 channels: the hand-over between two stages
    "u8k16_m80": _hp(64, [8, 2], [16, 6], [3, 5], [1, 2, 4], 80),   # u = 8; R = 3 with u = 2; two blocks per stage; other dilations
    "r1_r3_m128": _hp(96, [4, 4], [4, 12], [5, 3, 7, 9], [1, 3, 5], 128),  # R = 1 with pad 0; R = 3 (k = 3u, the largest accepted); four blocks
    "u8k16_m80_tanh_bias": dict(_hp(64, [8, 2], [16, 6], [3, 5], [1, 2, 4], 80), use_tanh_at_final=True, use_bias_at_final=True, snake_logscale=False),
    "w768_k3": _hp(768, [4], [8], [3], [1, 3, 5], 100),             # w768's widths with its one AMP block at the shortest kernel (K = 3 x 384)
}
SEED = 5
PROBE_T = (3, 9)  # 9 frames are 36 rows at u = 4: the snake crosses a time tile
RAGGED_FRAMES = [3, 1, 9]


def _total_up(hp):
    return math.prod(hp["upsample_rates"])


@pytest.fixture(scope="module")
def probe(request, lib):
    """One probe, built once: the HIP generator, and for T in PROBE_T the mel, the float64 reference and the fp32 oracle's output."""
    from eraxvif5tts_amd.bigvgan import BigVGAN
    hp = PROBES[request.param]
    W = cpu_ref.random_bigvgan_weights(hp, seed=SEED)
    if not hp["snake_logscale"]:
        for k in W:
            if k.endswith(".alpha") or k.endswith(".beta"):
                W[k] = W[k].abs() + 0.5
    W["conv_post.weight"] = W["conv_post.weight"] * 0.0015
    W64 = {k: v.double() for k, v in W.items()}
    g = torch.Generator().manual_seed(SEED)
    cases = {}
    for T in PROBE_T:
        mel = torch.randn(2, hp["num_mels"], T, generator=g) * 2 - 3
        cases[T] = (mel, cpu_ref.bigvgan_forward(W64, hp, mel.double()), cpu_ref.bigvgan_forward(W, hp, mel))
    voc = BigVGAN(hp)
    voc.load_state_dict(W)
    yield request.param, hp, voc.eval().cuda(), cases
    voc._drop_native()


@gpu
@pytest.mark.parametrize("T", PROBE_T)
@pytest.mark.parametrize("probe", list(PROBES), indirect=True)
def test_probe_matches_the_float64_oracle(probe, T):
    name, hp, voc, cases = probe
    mel, ref64, ref32 = cases[T]
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32 and ref64.shape == ref32.shape == (2, 1, T * _total_up(hp))
    sat = float((ref64.abs() >= 0.999).double().mean())
    assert sat < 0.01, f"{name}: {sat:.4f} of the reference is clamped"  # a condition on the reference, not on the code under test
    got = voc(mel.cuda()).cpu()
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all())
    r32, r = rel_l2(ref32, ref64), rel_l2(got, ref64)
    m32, m = float((ref32.double() - ref64).abs().max()), float((got.double() - ref64).abs().max())
    mbound = 8 * m32 + EPS32 * float(ref64.abs().max())
    print(f"probe {name} T = {T}: rel-L2 gpu {r:.3e} / fp32 oracle {r32:.3e} = {r / r32:.2f} (bound 8); max err gpu {m:.3e} / bound {mbound:.3e} = "
          f"{m / mbound:.3f}; saturated {sat:.4f}")
    assert r <= 8 * r32 and r <= 1e-4, (name, T, r, r32)
    assert m <= mbound, (name, T, m, mbound)


@gpu
@pytest.mark.parametrize("probe", list(PROBES), indirect=True)
def test_probe_ragged_decode_equals_batch1_forward_bit_for_bit(probe):
    name, hp, voc, _ = probe
    mels, up = hp["num_mels"], _total_up(hp)
    rows = (torch.randn(sum(RAGGED_FRAMES), mels, generator=torch.Generator().manual_seed(SEED + 1)) * 2 - 3).cuda()
    waves = voc.decode_ragged(rows, [0, 3, 4], RAGGED_FRAMES)
    for w, s, t in zip(waves, [0, 3, 4], RAGGED_FRAMES):
        one = voc(rows[s: s + t].t()[None])
        assert w.shape == one.shape == (1, 1, t * up) and bool(torch.isfinite(one).all())
        assert torch.equal(w, one), (name, t)


# ---------------------------------------------------------------------------------------------------------------- d. k > 3u is refused
@gpu
@pytest.mark.parametrize("rates,kernels,stage", [([4, 4], [8, 16], 1), ([2, 4], [8, 8], 0), ([4, 2, 2], [8, 4, 8], 2), ([1], [5], 0)])
def test_create_refuses_a_kernel_above_three_rates(lib, rates, kernels, stage):
    """pad = (k - u) / 2 > u makes the scatter read gather row T + 1, which neither the GEMM nor the workspace has: f5_bigvgan_create answers
    F5_ENOTSUP, names the stage and leaves *out null.  k = 3u is the largest accepted (probe r1_r3_m128 computes it)."""
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.bigvgan import BigVGAN
    hp = _hp(64, rates, kernels, [3], [1, 3, 5], 100)
    cfg = _lib.BigVGANConfig(num_mels=100, upsample_initial_channel=64, num_upsamples=len(rates), num_kernels=1, snake_logscale=1)
    for i, (u, k) in enumerate(zip(rates, kernels)):
        cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
    cfg.resblock_kernel_sizes[0] = 3
    for t, d in enumerate((1, 3, 5)):
        cfg.resblock_dilations[0][t] = d
    hd = C.c_void_p(0xDEAD0)
    assert lib.f5_bigvgan_create(C.byref(cfg), C.byref(hd)) == F5_ENOTSUP
    msg = _lib.last_error()
    assert f"stage {stage}" in msg and f"kernel {kernels[stage]}" in msg and f"rate {rates[stage]}" in msg, msg
    assert not hd.value
    with pytest.raises(_lib.F5HipError, match=f"stage {stage}"):
        BigVGAN(hp).native()
