"""Every tile, schedule and element type of the tuned 16-bit GEMM (csrc/gemm_fast.hip and its fp16 / LayerNorm-fold translation units,
csrc/gemm_w4.hip) and both builds of the halo-tile convolution (csrc/conv31.hip) at op level, per element.

Every launch is confirmed by the host-side launch record (f5_debug_last_gemm): a forced tile the rule refuses, or another kernel family taking
the launch, fails the case instead of silently testing something else.

Two kinds of input, two kinds of assertion:

  exact     A in {-2 .. 2}, W in {-1, 0, 1}, integer bias in +-8, gate in {+-1/2, +-1, +-2}, a residual stream of multiples of 1/2 in +-64, RoPE
            tables of (cos, sin) in {(1, 0), (0, 1), (-1, 0), (0, -1), (1/2, 1/2)}.  With K <= 704 every product, partial sum and epilogue value
            is a multiple of 1/4 below 2^13, exact in fp32 in any order with or without FMA contraction: the output must equal the fp64 result
            rounded once to the stored type BIT FOR BIT (torch.equal).  Masked rows are zeros (gate) / untouched (residual).
  rounded   GELU-tanh store, Mish conv, LayerNorm fold, random real data: |out - ref| <= 1 ulp(ref) of the stored type + 8 fp32 ulps of the
            magnitude sum (x 1.13 through GELU, x 1.1 through Mish) per element -- gpu_helpers.check_elementwise, the bound test_gpu_fp16_ops.py
            derives, with bf16's ulp in bf16 mode.  Nothing in it is measured; every case prints its worst share of the bound.

Cases the kernels' own launch conditions refuse (left out, nothing changed to admit them):
  * gemm_w4_bm = 256 at M = 768, N = 512 under gemm_persist_grid = 8: the forced height needs one 256-row tile per workgroup (6 < 8).  The same
    shape takes 256-row tiles by the unforced rule (6 tiles >= 3/4 of 8), and M = 1024 takes them forced; both run here.
  * f5_bench_gemm_site reaches the four block linears in bf16 without the LayerNorm fold and with the store form of the gated epilogues; it
    cannot launch conv31, the fold builds or the in-place residual epilogue (those are covered by cases 1 - 6 only).
"""
import ctypes as C
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

import gpu_helpers as G
from gpu_helpers import FAM_CONV31, FAM_FAST, FAM_TILE, FAM_W4, FLAG_CONV, FLAG_F16, FLAG_LNF, SCHED_PERSISTENT, SCHED_PLAIN, SCHED_STAGGERED

pytestmark = pytest.mark.gpu
P_BF16, P_FP16 = 0, 2
PRECISIONS = [P_BF16, P_FP16]
PREC_IDS = ["bf16", "fp16"]
TILES = [(256, 256), (256, 128), (256, 64), (128, 128), (128, 64)]
TILE_IDS = [f"{bm}x{bn}" for bm, bn in TILES]
EPILOGUES = ["store", "gate", "rope", "resid"]

# (family, bm, bn, schedule, LayerNorm-fold build) of every tuned-GEMM build cases 1 - 6 launch, in both element types.  Case 7 asserts that
# what the product's call sites launch is inside this set.
COVERED = frozenset(
    [(FAM_FAST, 256, 256, s, lnf) for s in (SCHED_PLAIN, SCHED_STAGGERED, SCHED_PERSISTENT) for lnf in (0, 1)] +
    [(FAM_FAST, bm, 128, s, lnf) for bm in (256, 128) for s in (SCHED_PLAIN, SCHED_STAGGERED) for lnf in (0, 1)] +
    [(FAM_FAST, bm, 64, SCHED_PLAIN, lnf) for bm in (256, 128) for lnf in (0, 1)] +
    [(FAM_W4, bm, 256, SCHED_PERSISTENT, 0) for bm in (128, 256)] +
    [(FAM_CONV31, tok, 64, SCHED_PLAIN, 0) for tok in (128, 256)])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus & ~7 == 256, f"the tile tables are worked out for a 256-CU persistent grid, this device has {cus} CUs"


def _expect(what, family, bm, bn, schedule, precision, lnf=0, conv=0):
    """the launch record names the intended kernel family, tile, schedule, element type and build"""
    rec = G.last_gemm()
    want = (family, bm, bn, schedule, (FLAG_F16 if precision == P_FP16 else 0) | (FLAG_LNF if lnf else 0) | (FLAG_CONV if conv else 0))
    assert rec == want, f"{what}: launched (family, bm, bn, schedule, flags) = {rec}, intended {want}"
    if not conv and family != FAM_TILE:
        assert (family, bm, bn, schedule, lnf) in COVERED, rec


def _fast_schedule(bn, kn, M, N, K, seq_ok=True):
    """launch_fast's schedule for a dense launch of the op (bias given, 16-bit output or fp16 stream, per-launch gate, row bits)"""
    if kn.get("gemm_variant", 1) == 0:
        return SCHED_PLAIN
    if bn == 256:
        persist = kn.get("gemm_persist", 1) and M % 256 == 0 and N % 256 == 0 and -(-K // 64) * 64 >= 128 and seq_ok
        return SCHED_PERSISTENT if persist else SCHED_STAGGERED
    return SCHED_STAGGERED if bn == 128 else SCHED_PLAIN


def _stored(precision, epi, ref):
    """the fp64 result rounded once to the stored type: the fp16 residual stream for the in-place epilogue, else the mode's 16-bit type"""
    return G.round_to(P_FP16 if epi == "resid" else precision, ref)


def _check_exact(what, out, precision, epi, ref, kw):
    want = _stored(precision, epi, ref)
    if not torch.equal(out, want):
        bad = (out != want).nonzero()
        raise AssertionError(f"{what}: {len(bad)} elements differ from the rounded fp64 result, first at {bad[0].tolist()}: "
                             f"{float(out[tuple(bad[0])])} != {float(want[tuple(bad[0])])}; rows hit {sorted(set(bad[:, 0].tolist()))[:8]}")
    mask = kw.get("rowmask")
    if mask is not None:  # (implied by the equality above; stated because it is the contract)
        assert torch.equal(out[~mask], kw["x"][~mask] if epi == "resid" else torch.zeros_like(out[~mask])), what


def _check_rounded(what, out, precision, epi, ref, scale):
    return G.check_elementwise(what, out, ref, scale, P_FP16 if epi == "resid" else precision)


SCHEDULE_KNOBS = [{}, {"gemm_persist": 0}, {"gemm_persist": 0, "gemm_lean": 0}, {"gemm_variant": 0}]


def _epi_variants(epi, bn):
    """(rope_heads, masked) variants of one epilogue: RoPE needs N = 3 * inner, run with one head and with all"""
    if epi == "rope":
        return sorted({(1, False), (bn // 64, False)})
    if epi == "resid":
        return [(1, False), (1, True)]
    return [(1, epi == "gate")]


# ----------------------------------------------------------------------------- 1. forced tile x epilogue x type x schedule
@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
def test_forced_tile_exact(tile, epi, precision):
    """Whole-tile shape (2 bm x 2 bn; RoPE 3 bn wide, seq = M / 2 so the position wraps inside a tile) and ragged shape (bm + 37 rows: a last
    tile of two whole 16-row fragments and a partial one; 3 bn wide), K = 64 / 128 / 192 / 704 (2, 4, 6, 22 K-steps of 32: fewer than the ring,
    exactly the ring, first wrap, many wraps with a remainder) on the store case, 64 and 704 elsewhere, under the four schedule knob sets:
    bit-equal to the rounded fp64 result."""
    bm, bn = tile
    for (M, nt, whole), K in itertools.product([(2 * bm, 2, True), (bm + 37, 3, False)], [64, 128, 192, 704] if epi == "store" else [64, 704]):
        N = 3 * bn if epi == "rope" else nt * bn
        seq = M // 2 if whole else M
        for heads, masked in _epi_variants(epi, bn):
            args, kw = G.exact_case(epi, M, N, K, seq, heads, masked, seed=M + 3 * N + K + heads)
            ref, _ = G.fused_ref(epi, *args, **kw)
            for kn in SCHEDULE_KNOBS:
                what = f"{bm}x{bn} {epi} {PREC_IDS[precision // 2]} M={M} N={N} K={K} heads={heads} masked={masked} {kn}"
                with G.knobs(gemm_tile=bm * 1000 + bn, gemm_w4=0, **kn):
                    out = G.run_fused(precision, 1, epi, *args, **kw)
                _expect(what, FAM_FAST, bm, bn, _fast_schedule(bn, kn, M, N, K), precision)
                _check_exact(what, out, precision, epi, ref, kw)


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
def test_forced_tile_gelu(tile, precision):
    """GELU-tanh store on random real data at the shapes of the exact case, K = 64 and 704: within the element-wise bound, and the same bits
    under every schedule of the tile."""
    bm, bn = tile
    for (M, nt), K in itertools.product([(2 * bm, 2), (bm + 37, 3)], [64, 704]):
        N = nt * bn
        _, A, W, b = G.linear_problem(precision, M, N, K, seed=M + N + K)
        ref, scale = G.fused_ref("store", A, W, b, act="gelu_tanh")
        outs = []
        for kn in SCHEDULE_KNOBS:
            what = f"{bm}x{bn} gelu {PREC_IDS[precision // 2]} M={M} N={N} K={K} {kn}"
            with G.knobs(gemm_tile=bm * 1000 + bn, gemm_w4=0, **kn):
                outs.append(G.run_fused(precision, 1, "store", A, W, b, act="gelu_tanh"))
            _expect(what, FAM_FAST, bm, bn, _fast_schedule(bn, kn, M, N, K), precision)
            _check_rounded(what, outs[-1], precision, "store", ref, scale)
            assert torch.equal(outs[-1], outs[0]), f"{what}: bits differ from the default schedule"


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi", EPILOGUES + ["gelu"])
def test_persistent_grid_walk_256x256(epi, precision):
    """The persistent 256 x 256 build on a grid of 8 workgroups (gemm_persist_grid = 8): 6 tiles (768 x 512: two workgroups idle), 10 tiles
    (1280 x 512: two workgroups walk a second tile, six do not), and the 10 tiles in L2 patches of 1 and 3 token tiles (gemm_group)."""
    real = epi == "gelu"
    name = "store" if real else epi
    N = 768 if epi == "rope" else 512
    for (M, group), K in itertools.product([(768, 0), (1280, 0), (1280, 1), (1280, 3)], [128, 704]):
        seq = M // 2 if epi == "rope" else M
        if real:
            _, A, W, b = G.linear_problem(precision, M, N, K, seed=M + K)
            args, kw = (A, W, b), dict(act="gelu_tanh")
        else:
            args, kw = G.exact_case(epi, M, N, K, seq, N // 192 if epi == "rope" else 1, epi in ("gate", "resid"), seed=M + K + group)
        ref, scale = G.fused_ref(name, *args, **kw)
        what = f"persistent 256x256 on 8 workgroups {epi} {PREC_IDS[precision // 2]} M={M} K={K} group={group}"
        with G.knobs(gemm_tile=256256, gemm_w4=0, gemm_persist_grid=8, gemm_group=group):
            out = G.run_fused(precision, 1, name, *args, **kw)
        _expect(what, FAM_FAST, 256, 256, SCHED_PERSISTENT, precision)
        if real:
            _check_rounded(what, out, precision, name, ref, scale)
        else:
            _check_exact(what, out, precision, name, ref, kw)


# ----------------------------------------------------------------------------- 2. the tile rule itself, N tails
# (M, N, K, gemm_bm128) -> tile gemm_fast_tile picks on a 256-CU device, evaluated by hand from the rule (a change of the rule shows up here)
NATURAL = {
    (300, 164, 128, 1): (256, 128),  # N % 256 != 0 and N % 64 != 0: a 36-wide last feature tile
    (300, 100, 192, 1): (256, 128),  # one partial feature tile
    (520, 320, 128, 1): (128, 64),   # 5 x 3 = 15 tiles of 256 x 64 leave CUs idle: 128-row tiles; a last token tile of 8 rows
    (512, 1024, 256, 0): (256, 64),
    (512, 1024, 256, 1): (128, 64),
    (512, 1024, 256, 2): (128, 64),
    (2002, 2304, 768, 0): (256, 64),
    (2002, 2304, 768, 1): (128, 128),  # 16 x 18 = 288 tiles of 128 x 128 fill the CUs
    (2002, 2304, 768, 2): (128, 64),   # ... but fewer than the 320 the forced-128 rule asks for
}


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi", ["gelu", "resid"])
@pytest.mark.parametrize("case", list(NATURAL), ids=lambda c: "M{}_N{}_K{}_bm128_{}".format(*c))
def test_natural_tile_rule(case, epi, precision):
    """No forcing: GELU store (bound) and exact in-place residual (bits) on the tile the rule picks, which must be the one NATURAL names."""
    M, N, K, bm128 = case
    bm, bn = NATURAL[case]
    what = f"natural {case} {epi} {PREC_IDS[precision // 2]}"
    if epi == "gelu":
        _, A, W, b = G.linear_problem(precision, M, N, K, seed=M + N + K)
        args, kw, name = (A, W, b), dict(act="gelu_tanh"), "store"
    else:
        (args, kw), name = G.exact_case("resid", M, N, K, M, 1, True, seed=M + N), "resid"
    ref, scale = G.fused_ref(name, *args, **kw)
    with G.knobs(gemm_bm128=bm128):
        out = G.run_fused(precision, 1, name, *args, **kw)
    _expect(what, FAM_FAST, bm, bn, _fast_schedule(bn, {}, M, N, K), precision)
    if epi == "gelu":
        _check_rounded(what, out, precision, name, ref, scale)
    else:
        _check_exact(what, out, precision, name, ref, kw)


# ----------------------------------------------------------------------------- 3. tile independence
@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi", EPILOGUES)
def test_tile_independence(epi, precision):
    """gemm_fast_tile's comment -- every accumulator sums K in the same order whatever the tile, so the result bits do not change -- on one
    real-valued problem per epilogue and type (549 x 768 x 704): each forced tile within the bound against fp64 (which decides whether a TILE
    is wrong), and all five outputs bit-equal (which decides whether the COMMENT is)."""
    M, N, K = 512 + 37, 768, 704
    run, ref, scale = G.fused_case(precision, epi, M, N, K, M, seed=M + N + K)
    outs = {}
    for bm, bn in TILES:
        with G.knobs(gemm_tile=bm * 1000 + bn, gemm_w4=0):
            outs[bm, bn] = run()
        what = f"tile independence {epi} {PREC_IDS[precision // 2]} {bm}x{bn}"
        _expect(what, FAM_FAST, bm, bn, _fast_schedule(bn, {}, M, N, K), precision)
        _check_rounded(what, outs[bm, bn], precision, epi, ref, scale)
    for t in TILES[1:]:
        diff = (outs[t] != outs[TILES[0]])
        assert not diff.any(), f"{epi} {PREC_IDS[precision // 2]}: tile {t} differs from 256x256 in {int(diff.sum())} elements, first at {diff.nonzero()[0].tolist()}"


# ----------------------------------------------------------------------------- 4. LayerNorm fold on every tile
@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("epi", [4, 0], ids=["qkv_rope", "ff1_gelu"])
@pytest.mark.parametrize("M", [300, 512])
def test_layernorm_fold_every_tile(M, epi, precision):
    """The fold site of test_layernorm_fold_site (offset 40, pivots) at D = 256, N = 768, Kb = 128 under each forced tile: the LNF build of that
    tile ran (at M = 512 the 256-wide one on the persistent grid, its statistics staged through LDS), `out` is within the element-wise bound
    of the reference built from the kernel's own stream and statistics, and stream, statistics and `out` are bit-equal across tiles."""
    D, N, Kb = 256, 768, 128
    args, kw = G.ln_fold_inputs(M, D, N, Kb, epi)
    got = {}
    for bm, bn in TILES:
        with G.knobs(gemm_tile=bm * 1000 + bn, gemm_w4=0):
            xs, stats, out = G.op_ln_fold_p(precision, epi, *args, **kw)
        what = f"ln_fold epi {epi} {PREC_IDS[precision // 2]} M={M} {bm}x{bn}"
        _expect(what, FAM_FAST, bm, bn, _fast_schedule(bn, {}, M, N, D), precision, lnf=1)
        ref, mag = G.ln_fold_ref(args, kw, epi, xs, stats)
        G.check_elementwise(what, out, ref, mag, precision)
        got[bm, bn] = (xs, stats, out)
    for t in TILES[1:]:
        for name, a, b in zip(("stream", "statistics", "out"), got[t], got[TILES[0]]):
            assert torch.equal(a, b), f"ln_fold epi {epi} {PREC_IDS[precision // 2]} M={M}: {name} under tile {t} differs from 256x256 in {int((a != b).sum())} elements"


# ----------------------------------------------------------------------------- 5. one-wave-per-SIMD kernel at small shapes
# (M, N, gemm_w4_bm) -> tile height w4_tile_rows picks under gemm_persist_grid = 8
W4_SHAPES = {(512, 512, 0): 128, (768, 512, 0): 256, (1024, 512, 256): 256, (512, 768, 128): 128, (768, 768, 256): 256}


# RoPE runs the N = 3 * inner shapes, the other epilogues the N = 512 ones
W4_CASES = [(s, e) for s in W4_SHAPES for e in ["store", "gelu", "rope", "resid"] if (e == "rope") == (s[1] == 768)]


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("shape,epi", W4_CASES, ids=["M{}_N{}_bm{}_{}".format(*s, e) for s, e in W4_CASES])
def test_w4_kernel_small_shapes(shape, epi, precision):
    """gemm_w4.hip with a persistent grid of 8 workgroups, where it takes launches of a few tiles: both tile heights, K = 256 and 384, the
    whole-line store / RoPE epilogues and the in-place residual.  Exact cases bit for bit; GELU within the bound and bit-equal to the 8-wave
    kernel (gemm_w4 = 0)."""
    M, N, w4_bm = shape
    rows = W4_SHAPES[shape]
    real = epi == "gelu"
    name = "store" if real else epi
    for K in (256, 384):
        if real:
            _, A, W, b = G.linear_problem(precision, M, N, K, seed=M + N + K)
            args, kw = (A, W, b), dict(act="gelu_tanh")
        else:
            args, kw = G.exact_case(epi, M, N, K, M // 2, N // 192, True, seed=M + N + K)
        ref, scale = G.fused_ref(name, *args, **kw)
        what = f"w4 {rows}-row tiles {epi} {PREC_IDS[precision // 2]} M={M} N={N} K={K}"
        with G.knobs(gemm_persist_grid=8, gemm_w4_bm=w4_bm):
            out = G.run_fused(precision, 1, name, *args, **kw)
            _expect(what, FAM_W4, rows, 256, SCHED_PERSISTENT, precision)
            with G.knobs(gemm_w4=0):
                old = G.run_fused(precision, 1, name, *args, **kw)
                assert G.last_gemm()[0] == FAM_FAST, what
        if real:
            _check_rounded(what, out, precision, name, ref, scale)
        else:
            _check_exact(what, out, precision, name, ref, kw)
        assert torch.equal(out, old), f"{what}: differs from the 8-wave kernel"


# ----------------------------------------------------------------------------- 6. conv31, both builds
CONV_DIM = 1024
CONV_LENGTHS = [1, 7, 15, 16, 31, 127, 128, 129, 255, 256, 257, 300, 513]
# route -> (knobs, kernel argument of f5_op_conv31, intended record without the element-type flag)
CONV_ROUTES = {
    "conv31_128": (dict(conv31_tok=128), 1, (FAM_CONV31, 128, 64, SCHED_PLAIN, 0)),
    "conv31_256": (dict(conv31_tok=256), 1, (FAM_CONV31, 256, 64, SCHED_PLAIN, 0)),
    "implicit_gemm": (dict(conv31=0), 1, (FAM_FAST, 256, 64, SCHED_PLAIN, 1)),
    "tile_kernel": (dict(), 0, (FAM_TILE, 64, 64, SCHED_PLAIN, 1)),
}


@functools.lru_cache(maxsize=None)
def _conv_weights():
    """exact (integer, drawn independently per tap: a shifted or dropped tap cannot cancel) and real (exact in bf16 and in fp16) weights and biases"""
    g = torch.Generator().manual_seed(31)
    cg = CONV_DIM // 16
    both = lambda t: torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t.to(torch.bfloat16).float())
    return (G.ints(g, (CONV_DIM, cg, 31), -1, 1), G.ints(g, (CONV_DIM,), -8, 8),
            both(torch.randn(CONV_DIM, cg, 31, generator=g) / (cg * 31) ** 0.5), torch.randn(CONV_DIM, generator=g) * 0.1)


@pytest.mark.parametrize("L", CONV_LENGTHS)
@pytest.mark.parametrize("B", [1, 3])
def test_conv31_routes(B, L):
    """One convolution alone (f5_op_conv31) at dim = 1024: utterances shorter than the halo, tile edges of both builds at +-1, a last tile of
    one row; with B = 3 a kernel that reads across an utterance boundary instead of the zero page picks up the neighbour's values.  act = none
    on exact inputs: every route bit-equal to the rounded fp64 convolution.  act = mish on real data (values exact in both 16-bit types, so
    one reference serves both): every route within the bound (mish' < 1.1), the two conv31 builds bit-equal."""
    wi, bi, wr, br = _conv_weights()
    g = torch.Generator().manual_seed(B * 1000 + L)
    both = lambda t: torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t.to(torch.bfloat16).float())
    xi, xr = G.ints(g, (B, L, CONV_DIM), -2, 2), both(torch.randn(B, L, CONV_DIM, generator=g))
    ref_i = G.conv31_ref(xi, wi, bi)
    lin, mag = G.conv31_ref(xr, wr, br), G.conv31_ref(xr.abs(), wr.abs(), br.abs())
    ref_m = F.mish(lin)
    for precision in PRECISIONS:
        mish = {}
        for route, (kn, kernel, rec) in CONV_ROUTES.items():
            what = f"conv31 {route} {PREC_IDS[precision // 2]} B={B} L={L}"
            with G.knobs(**kn):
                out = G.op_conv31(precision, kernel, xi, wi, bi, "none")
                _expect(what, *rec[:4], precision, conv=rec[4])
                mish[route] = G.op_conv31(precision, kernel, xr, wr, br, "mish")
                _expect(what, *rec[:4], precision, conv=rec[4])
            want = G.round_to(precision, ref_i)
            assert torch.equal(out, want), (f"{what}: {int((out != want).sum())} elements differ from the rounded fp64 convolution, first at "
                                            f"{(out != want).nonzero()[0].tolist()}")
            G.check_elementwise(what + " mish", mish[route], ref_m, 1.1 * mag, precision)
        assert torch.equal(mish["conv31_128"], mish["conv31_256"]), f"conv31 builds differ, {PREC_IDS[precision // 2]} B={B} L={L}"


# ----------------------------------------------------------------------------- 7. what the product launches is what was tested
@pytest.mark.parametrize("dim", [1024, 768])
def test_product_call_sites_launch_covered_builds(dim):
    """The four block linears as the sampler launches them (f5_bench_gemm_site: bf16, no fold; it cannot reach conv31 or the fold builds) at
    2 x B x 1024 token rows, B = 1, 2, 4, 8: every (family, tile, schedule) launched is one cases 1 - 6 cover.  A tuning change that routes a
    site to an untested build fails here."""
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    seen = {}
    for B, site in itertools.product([1, 2, 4, 8], range(4)):
        ms = C.c_float(0.0)
        _lib.check(lib.f5_bench_gemm_site(1, site, 2 * B * 1024, 1024, dim, dim // 64, 2 * dim, 1, C.byref(ms), _lib.stream_ptr()))
        fam, bm, bn, sched, flags = G.last_gemm()
        seen[B, site] = (fam, bm, bn, sched, flags)
        assert flags == 0 and (fam, bm, bn, sched, 0) in COVERED, f"dim {dim}, {2 * B * 1024} rows, site {site}: launched {(fam, bm, bn, sched, flags)}, which no op-level case covers"
    print(f"  dim {dim}: " + ", ".join(f"B={b} site {s}: {v[:4]}" for (b, s), v in seen.items()))
