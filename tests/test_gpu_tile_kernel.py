"""The reference tile kernel (csrc/gemm.hip: gemm_tile_kernel, epilogues in csrc/gemm_epilogue.h) per element, in bf16, fp16 and fp32, through
f5_op_tile_gemm (gpu_helpers.op_tile_gemm).  It is the only GEMM of the fp32 mode -- the on-device oracle of the full-size tests -- of Vocos,
BigVGAN and the mel front-end, and the `base` cross-check of every tuned-GEMM test.

Every launch is confirmed by the launch record (f5_debug_last_gemm): the 64 x 64 tile family with the element-type and conv flags of the case.
Every output buffer is [M + 2, ld] filled with NaN: padding columns and guard rows must come back as NaN (asserted inside op_tile_gemm).

  exact     the inputs of test_gpu_gemm_tiles.py (G.exact_case: integers and halves, every product, partial sum and epilogue value exact in
            fp32 at K <= 704): out_t must equal the fp64 result rounded once to the mode's type, out_f the fp64 result itself (fp32 stream)
            or rounded once to fp16 (fp16 stream), BIT FOR BIT.  M in {1, 63, 64, 65, 130}, N in {1, 2, 62, 64, 66, 70} (a partial 4-lane
            group, a partial tile, a second tile), K in {32, 64, 704}; leading dimensions N, N + 1, N + 4 and, where N % 4 != 0, the next
            multiple of 4 (vector stores with a partial last group); RoPE at N = 192 and 384 with one head and with all; a per-batch gate over
            3 items of 43 rows (tiles straddle items); row masks; EPI_ADD2 with a_row_mod = M / 2 and both addend types; conv31 with integer
            weights drawn per tap.
  rounded   random real data through GELU-tanh, GELU-erf and Mish: gpu_helpers.check_elementwise,
            |out - ref| <= 1 ulp(ref) of the stored type + 8 fp32 ulps of sum |a w| (x 1.13 through GELU, x 1.1 through Mish) over what the
            epilogue adds.  Nothing in the bound is measured; tests/test_tile_kernel_bound_host.py shows on the CPU that a sequential fp32 FMA
            chain stays inside it and that each defect this module is there for leaves it.  Every case prints its worst share.

Measured on MI355X: every exact case bit-equal in all three precisions; no defect found.  Worst share of the bound over the rounded cases
(out_t in the mode's type / an fp32 out_f / an fp16-stream out_f):
            store gelu_tanh  gelu_erf  mish    store_f32 tanh / erf   gate    resid f32 / f16 stream   add2 t / f32 / f16   rope    conv31 mish / resid
    bf16    0.500            0.500     0.499   0.069 / 0.077          0.499   0.109 / 0.499            0.500 / 0.063 / 0.497   0.500   0.499 / 0.074
    fp16    0.497            0.498     0.498   0.086 / 0.091          0.496   0.080 / 0.499            0.499 / 0.088 / 0.499   0.498   0.497 / 0.074
    fp32    0.161            0.185     0.163   0.161 / 0.185          0.156   0.174 / 0.499            0.162 / 0.162 / 0.499   0.186   0.108 / 0.112
(the 16-bit figures are the one rounding of the stored element; the fp32 ones are the kernel's arithmetic against 8 fp32 ulps of sum |a w|).
The module runs in about 3 s."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

import gpu_helpers as G
from gpu_helpers import P_BF16, P_FP16, P_FP32

pytestmark = pytest.mark.gpu
PRECISIONS = [P_BF16, P_FP16, P_FP32]
PREC_IDS = [G.PREC_NAMES[p] for p in PRECISIONS]
MS, NS, KS = (1, 63, 64, 65, 130), (1, 2, 62, 64, 66, 70), (32, 64, 704)
WORST = {}  # (precision, epilogue) -> worst share of the bound over the rounded cases (printed when the module is done)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()
    yield
    for (p, e), w in sorted(WORST.items()):
        print(f"\n  worst share of the bound, {G.PREC_NAMES[p]} {e}: {w:.3f}", end="")
    print()


def _pads(N):
    """leading dimension - N: N, N + 1, N + 4 and the next multiple of 4 above an N that is none"""
    return sorted({0, 1, 4, -N % 4})


def _shapes():
    """(M, N, K, pad): the whole M x N x K grid, the pads taking turns so that every N meets each of its pads at every K; then six shapes at
    K = 64 with every pad"""
    out = []
    for (i, M), (j, N), (k, K) in itertools.product(enumerate(MS), enumerate(NS), enumerate(KS)):
        pads = _pads(N)
        out.append((M, N, K, pads[(i + j + k) % len(pads)]))
    for M, N in [(1, 1), (63, 2), (64, 64), (65, 66), (130, 70), (130, 62)]:
        out += [(M, N, 64, pad) for pad in _pads(N)]
    return out


def _assert_equal(what, name, out, want):
    if not torch.equal(out, want):  # (a NaN the kernel left in [M, N] differs from everything)
        bad = (out != want).nonzero()
        raise AssertionError(f"{what}: {name}: {len(bad)} elements differ from the rounded fp64 result, first at {bad[0].tolist()}: "
                             f"{float(out[tuple(bad[0])])} != {float(want[tuple(bad[0])])}; rows hit {sorted(set(bad[:, 0].tolist()))[:8]}, "
                             f"columns hit {sorted(set(bad[:, 1].tolist()))[:8]}")


def _run_exact(what, precision, epi, args, kw, f16_stream=False, pad=0, a_row_mod=0, rows_per_batch=0, gate_bstride=0, conv=False, lin=None):
    """one launch on exact inputs: the record, bit equality of both outputs, the mask contract"""
    A, W, b = args
    ref_kw = dict(kw)
    M = (kw.get("x") if "x" in kw else kw.get("addend") if "addend" in kw else A).shape[0] if not conv else A.shape[0] * A.shape[1]
    if gate_bstride:
        ref_kw["gate"] = G.expand_gate(kw["gate"], M, rows_per_batch)
    Aref = A[torch.arange(M) % a_row_mod] if a_row_mod else A
    ref, _ = G.fused_ref(epi.replace("store_f32", "store"), Aref, W, b, lin=lin, **ref_kw)
    out_t, out_f = G.op_tile_gemm(precision, epi, A, W, b, f16_stream=f16_stream, pad=pad, a_row_mod=a_row_mod, rows_per_batch=rows_per_batch,
                                  gate_bstride=gate_bstride, conv=conv, **kw)
    G.expect_tile_launch(what, precision, conv)
    want_t, want_f = G.tile_stored(precision, epi, f16_stream, ref)
    for name, out, want in (("out_t", out_t, want_t), ("out_f", out_f, want_f)):
        assert (out is None) == (want is None), what
        if out is not None:
            _assert_equal(what, name, out, want)
    mask = kw.get("rowmask")
    if mask is not None:  # (implied by the equality above; stated because it is the contract)
        if epi == "resid":
            assert torch.equal(out_f[~mask], G.round_to(P_FP16 if f16_stream else P_FP32, kw["x"])[~mask]), what
        else:
            assert (out_t[~mask] == 0).all(), what


# (epilogue, fp16 stream): every dense (mode, epilogue) pair of dispatch_tile but RoPE, the in-place and two-output ones on both stream types
DENSE = [("store", False), ("store_f32", False), ("gate", False), ("resid", False), ("resid", True), ("add2", False), ("add2", True)]
DENSE_IDS = [e + ("_f16_stream" if f else "") for e, f in DENSE]


# ----------------------------------------------------------------------------- 1. exact inputs: shapes, leading dimensions, epilogues
@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi,f16_stream", DENSE, ids=DENSE_IDS)
def test_exact_shapes_and_leading_dimensions(epi, f16_stream, precision):
    """Gate and residual cases carry a row mask (RESID leaves masked rows untouched, GATE_T writes zeros); EPI_ADD2 reads A through
    a_row_mod = M / 2 where M is even (both CFG branches read the same rows)."""
    name = epi.replace("store_f32", "store")
    for M, N, K, pad in _shapes():
        mod = M // 2 if epi == "add2" and M % 2 == 0 else 0
        args, kw = G.exact_case(name, M, N, K, M, 0, True, seed=M + 3 * N + K + pad, a_rows=mod or None)
        _run_exact(f"{epi} {G.PREC_NAMES[precision]} M={M} N={N} K={K} ld=N+{pad} a_row_mod={mod}", precision, epi, args, kw, f16_stream, pad, mod)


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi,f16_stream", [("gate", False), ("resid", False), ("resid", True)], ids=["gate", "resid", "resid_f16_stream"])
def test_exact_per_batch_gate_straddling_tiles(epi, f16_stream, precision):
    """3 batch items of 43 rows with gate_bstride = N: the item boundaries (rows 43, 86) fall inside the 64-row tiles; each row must take the
    gate of its own item.  Masked and unmasked."""
    seq, nb = 43, 3
    for N, K, pad, masked in [(64, 64, 0, False), (70, 32, 1, True), (62, 704, 2, True), (130, 64, 0, False)]:
        args, kw = G.exact_case(epi, nb * seq, N, K, seq, 0, masked, seed=N + K, gate_batches=nb)
        _run_exact(f"per-batch gate {epi} {G.PREC_NAMES[precision]} N={N} K={K} ld=N+{pad}", precision, epi, args, kw, f16_stream, pad,
                   rows_per_batch=seq, gate_bstride=N)


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("N", [192, 384])
def test_exact_rope(N, precision):
    """Fused QKV + RoPE at inner = 64 and 128, one head and all heads roped, positions wrapping inside a tile (seq = M / 2 at M = 130) and not."""
    for (M, seq), K, heads, pad in itertools.product([(1, 1), (63, 63), (64, 64), (65, 65), (130, 65)], (32, 704), sorted({1, N // 192}), (0, 1, 4)):
        if pad and K == 704 and M not in (65, 130):
            continue
        args, kw = G.exact_case("rope", M, N, K, seq, heads, False, seed=M + N + K + heads)
        _run_exact(f"rope {G.PREC_NAMES[precision]} M={M} N={N} K={K} heads={heads} seq={seq} ld=N+{pad}", precision, "rope", args, kw, pad=pad)


# ----------------------------------------------------------------------------- 2. conv31 through the tile kernel
CONV_L = (1, 15, 16, 31, 65)


@functools.lru_cache(maxsize=None)
def _conv_case(dim, L, real):
    """B = 3 utterances; exact: x in {-2 .. 2}, integer weights drawn independently per tap, an accumulator of halves, gates of +-1/2, 1, 2;
    real: randn values exact in bf16 and in fp16.  -> (x, w, b, gate, acc0, rowmask, (fp64 conv, magnitude))"""
    g = torch.Generator().manual_seed(dim + L + real)
    cg, B = dim // 16, 3
    both = lambda t: torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t.to(torch.bfloat16).float())
    if real:
        x, w, b = both(torch.randn(B, L, dim, generator=g)), both(torch.randn(dim, cg, 31, generator=g) / (cg * 31) ** 0.5), torch.randn(dim, generator=g) * 0.1
        gate, acc0 = torch.randn(dim, generator=g), torch.randn(B * L, dim, generator=g).half().float()
    else:
        x, w, b = G.ints(g, (B, L, dim), -2, 2), G.ints(g, (dim, cg, 31), -1, 1), G.ints(g, (dim,), -8, 8)
        gate = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[torch.randint(0, 6, (dim,), generator=g)]
        acc0 = G.ints(g, (B * L, dim), -128, 128) * 0.5
    mask = torch.rand(B * L, generator=g) > 0.2
    lin = (G.conv31_ref(x, w, b).reshape(B * L, dim), G.conv31_ref(x.abs(), w.abs(), b.abs()).reshape(B * L, dim))
    return x, w, b, gate, acc0, mask, lin


CONV_CASES = [(128, p) for p in PRECISIONS] + [(1024, P_FP32)]


@pytest.mark.parametrize("dim,precision", CONV_CASES, ids=[f"dim{d}-{G.PREC_NAMES[p]}" for d, p in CONV_CASES])
def test_exact_conv31(dim, precision):
    """GEMM_CONV31 x {STORE_T, RESID onto a nonzero accumulator (fp32, and the fp16 stream form), GATE_T with a row mask}, B = 3 (a read across
    an utterance boundary picks up the neighbour), lengths below, at and above the 15-row halo and above one tile.  dim 1024 in fp32 -- the
    mode whose only conv kernel this is; test_gpu_gemm_tiles.py::test_conv31_routes runs the 16-bit store form there -- and dim 128 (8 channels
    per group) in all three."""
    for L in CONV_L:
        x, w, b, gate, acc0, mask, lin = _conv_case(dim, L, 0)
        what = f"conv31 {G.PREC_NAMES[precision]} dim={dim} L={L}"
        _run_exact(what + " store", precision, "store", (x, w, b), {}, conv=True, lin=lin)
        _run_exact(what + " resid", precision, "resid", (x, w, b), dict(gate=gate, x=acc0), conv=True, lin=lin)
        _run_exact(what + " gate", precision, "gate", (x, w, b), dict(gate=gate, rowmask=mask), conv=True, lin=lin)
        if L in (16, 65):
            _run_exact(what + " resid, fp16 stream, masked", precision, "resid", (x, w, b), dict(gate=gate, x=acc0, rowmask=mask), f16_stream=True,
                       conv=True, lin=lin)


# ----------------------------------------------------------------------------- 3. rounded: random real data, the three activations
def _check_rounded(what, precision, epi, f16_stream, outs, ref, scale):
    for name, out, stored in (("out_t", outs[0], precision), ("out_f", outs[1], P_FP16 if f16_stream else P_FP32)):
        if out is not None:
            w = G.check_elementwise(f"{what} {name}", out, ref, scale, stored)
            key = (precision, epi + ("_f16_stream" if f16_stream else "") + ("." + name if epi.startswith("add2") else ""))
            WORST[key] = max(WORST.get(key, 0.0), w)


ROUNDED = [("store", "gelu_tanh", False), ("store", "gelu_erf", False), ("store", "mish", False), ("store_f32", "gelu_erf", False),
           ("store_f32", "gelu_tanh", False), ("gate", "gelu_tanh", False), ("resid", "none", False), ("resid", "none", True),
           ("add2", "none", False), ("add2", "none", True), ("rope", "none", False)]


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi,act,f16_stream", ROUNDED, ids=[f"{e}_{a}" + ("_f16_stream" if f else "") for e, a, f in ROUNDED])
def test_rounded(epi, act, f16_stream, precision):
    """randn operands in the mode's type (fp32: as drawn), K = 32, 128 and 704, partial tiles and a partial 4-lane group; per-batch gates with
    a row mask on the gated epilogues, a_row_mod on EPI_ADD2."""
    name = epi.replace("store_f32", "store")
    for M, N, K, pad in [(130, 70, 704, 0), (63, 62, 32, 2), (65, 66, 128, 1)]:
        if epi == "rope":
            N = 192
        seq, nb = (M // 2 if M % 2 == 0 else M), (2 if M % 2 == 0 else 1)
        g, A, W, b = G.linear_problem(precision, M, N, K, seed=M + N + K)
        kw, run_kw = dict(act=act), {}
        if epi in ("gate", "resid"):
            kw.update(gate=torch.randn(nb, N, generator=g), rowmask=torch.rand(M, generator=g) > 0.2)
            run_kw = dict(rows_per_batch=seq, gate_bstride=N)
        if epi == "resid":
            kw["x"] = (torch.randn(M, N, generator=g) * 3).half().float()
        if epi == "add2":
            kw["addend"] = (torch.randn(M, N, generator=g) * 3).half().float()
            if M % 2 == 0:
                A, run_kw = A[:M // 2].contiguous(), dict(a_row_mod=M // 2)
        if epi == "rope":
            ang = torch.rand(seq, 32, generator=g) * 6.28
            kw.update(rope=torch.stack([ang.cos(), ang.sin()], dim=-1), rope_heads=1, seq=seq)
        ref_kw = dict(kw)
        if "gate" in kw:
            ref_kw["gate"] = G.expand_gate(kw["gate"], M, seq)
        Aref = A[torch.arange(M) % (M // 2)] if "a_row_mod" in run_kw else A
        ref, scale = G.fused_ref(name, Aref, W, b, **ref_kw)
        what = f"{epi} {act} {G.PREC_NAMES[precision]} M={M} N={N} K={K} ld=N+{pad}"
        outs = G.op_tile_gemm(precision, epi, A, W, b, f16_stream=f16_stream, pad=pad, **run_kw, **kw)
        G.expect_tile_launch(what, precision)
        if "rowmask" in kw:  # masked rows: untouched (resid) or zeros (gate) exactly; the bound is for the rows the kernel computes
            keep = kw["rowmask"]
            got = outs[1] if epi == "resid" else outs[0]
            assert torch.equal(got[~keep], kw["x"][~keep] if epi == "resid" else torch.zeros_like(got[~keep])), what
        _check_rounded(what, precision, epi + "_" + act, f16_stream, outs, ref, scale)


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
def test_rounded_conv31_mish(precision):
    """Mish conv store (the first convolution of the position embedding) and the gated residual form on real data, dim 128, B = 3."""
    for L in (15, 65):
        x, w, b, gate, acc0, mask, (lin, mag) = _conv_case(128, L, 1)
        what = f"conv31 mish {G.PREC_NAMES[precision]} L={L}"
        outs = G.op_tile_gemm(precision, "store", x, w, b, act="mish", conv=True)
        G.expect_tile_launch(what, precision, conv=True)
        _check_rounded(what, precision, "conv31_store_mish", False, outs, F.mish(lin), 1.1 * mag)
        outs = G.op_tile_gemm(precision, "resid", x, w, b, gate=gate, x=acc0, conv=True)
        G.expect_tile_launch(what, precision, conv=True)
        _check_rounded(what + " resid", precision, "conv31_resid", False, outs, acc0.double() + gate.double() * lin, acc0.double().abs() + gate.double().abs() * mag)
