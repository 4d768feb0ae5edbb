"""The whole-line in-place residual epilogue of the one-wave-per-SIMD block GEMM (csrc/gemm_w4.hip, 256-row tiles of EPI_RESID: attention
out-projection and FF2, which update the fp16 residual stream in place and write the LayerNorm fold's partial row statistics).

With the MFMA's operand roles swapped and the weight rows permuted on their way into LDS, a lane holds eight consecutive features of one token per
(token tile, component): one 16-byte load and one 16-byte store of the stream, 16 lanes = one 256-byte run of a row.  Products, K order, start
value and the arithmetic per element are unchanged, and the row statistics are summed in their old lane map from the values just stored (through a
per-wave patch of LDS; tests/test_w4_resid_map_host.py has the maps), so every case asserts

  * the stream is BIT-EQUAL to the 8-wave kernel's (knob gemm_w4 = 0),
  * the partial planes are BIT-EQUAL to the 8-wave kernel's (and with them stats_finalize's (mean, rstd) and the range guard's words),
  * the stream is within the fp64 bound test_gpu_ops.py uses for the in-place epilogue (taken from that file, below),

with per-feature random bias and gate (a permutation error in the new indexing moves values between columns), a stream with per-row offsets, and
statistics both with pivots near the row means and without pivots."""
import ctypes as C
import inspect
import math
import re

import pytest
import torch

import test_gpu_ops
from conftest import rel_l2
from test_gpu_w4_whole_line_epilogue import _both

pytestmark = pytest.mark.gpu

# the fp64 bound of the in-place epilogue as test_gpu_ops.py states it (rel-L2: one fp16 rounding of the result, 2^-11 relative) -- read from the
# test that compares this kernel with the 8-wave kernel, not restated here
RESID_TOL = float(re.search(r"ref, tol = \(x\.double\(\) \+ upd\)\.float\(\), ([0-9.e-]+)\n",
                            inspect.getsource(test_gpu_ops.test_w4_kernel_equals_the_8_wave_kernel)).group(1))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def op_resid_stats(precision, x, A, W, bias, gate, rowmask=None, pivot=None):
    """include/f5hip.h: f5_op_resid_stats_p.  Returns (stream [M, N] as f32, planes [N / 64, M, 2], stats [M, 2], guard words: 6 ints,
    launch record of the GEMM)."""
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[0]
    dev = [None if t is None else t.cuda().float().contiguous() for t in (A, W, bias, gate, pivot)]
    mk = None if rowmask is None else rowmask.cuda().to(torch.uint8).contiguous()
    xs = x.cuda().float().contiguous().clone()
    planes = torch.empty(N // 64, M, 2, device="cuda")
    stats = torch.empty(M, 2, device="cuda")
    guard = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.f5_op_resid_stats_p(precision, M, N, K, _lib.ptr(xs), _lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]),
                                       _lib.ptr(mk), _lib.ptr(dev[4]), _lib.ptr(planes), _lib.ptr(stats), _lib.ptr(guard), _lib.stream_ptr()),
               "f5_op_resid_stats_p")
    return xs.cpu(), planes.cpu(), stats.cpu(), [int(v) & 0xffffffff for v in guard.cpu().tolist()], G.last_gemm()


def _problem(M, N, K, precision=0, stream_scale=1.7, gate_scale=1.0):
    import gpu_helpers as G
    g = torch.Generator().manual_seed(M + 7 * N + K + precision)
    A = G.round_to(precision, torch.randn(M, K, generator=g))
    W = G.round_to(precision, torch.randn(N, K, generator=g) / math.sqrt(K))
    bias, gate = torch.randn(N, generator=g) * 0.5, torch.randn(N, generator=g) * gate_scale
    x = (torch.randn(M, N, generator=g) * 1.7 + torch.randn(M, 1, generator=g) * 3.0) * (stream_scale / 1.7)
    x = x.clamp(-65504.0, 65504.0).half().float()  # the stream as stored
    return A, W, bias, gate, x


def _check(M, N, K, precision=0, rowmask=None, stream_scale=1.7, gate_scale=1.0):
    """both pivot forms on both kernels; returns the whole-line kernel's (stream, planes, stats, guard) without pivots"""
    import gpu_helpers as G
    A, W, bias, gate, x = _problem(M, N, K, precision, stream_scale, gate_scale)
    upd = gate.double() * (A.double() @ W.double().t() + bias.double())
    if rowmask is not None:
        upd = upd * rowmask[:, None].double()
    ref = (x.double() + upd).clamp(-65504.0, 65504.0).float()  # (the stream saturates at the fp16 range: gemm.h, EPI_RESID)
    first = None
    for pivot in (None, torch.stack([x.mean(dim=1) + 0.01, torch.ones(M)], dim=1)):  # "previous mean": near, not equal to, the new one
        new, old = _both(lambda: op_resid_stats(precision, x, A, W, bias, gate, rowmask, pivot))
        assert new[4][:3] == (G.FAM_W4, 256, 256), new[4]      # the launch under test took the one-wave-per-SIMD kernel's tall tile ...
        assert old[4][0] == G.FAM_FAST, old[4]                  # ... and its yardstick the 8-wave kernel
        err = rel_l2(new[0], ref)
        print(f"resid whole-line {M}x{N}x{K} prec={precision} pivot={'yes' if pivot is not None else 'no'}: rel-L2 {err:.2e} (bound {RESID_TOL:g}), "
              f"guard {new[3]}")
        assert torch.isfinite(new[0]).all() and torch.isfinite(new[1]).all()
        assert torch.equal(new[0], old[0])                      # stream
        assert torch.equal(new[1], old[1])                      # partial planes
        assert torch.equal(new[2], old[2]) and new[3] == old[3]  # what the finalize makes of them, and the guard's words
        assert err < RESID_TOL
        if first is None:
            first = new
        else:
            assert torch.equal(new[0], first[0])                # the stream does not depend on the pivots
    if rowmask is not None:
        assert torch.equal(first[0][~rowmask], x[~rowmask])     # masked rows keep their bits
    return first, x


@pytest.mark.parametrize("M,N,K", [(16384, 1024, 256), (16896, 1024, 256), (22528, 768, 256), (16384, 1024, 2048)],
                         ids=["one_tile_per_cu_shortest_loop", "second_tile", "three_feature_tiles", "ff2_loop_length"])
def test_stream_and_planes_equal_the_8_wave_kernel(M, N, K):
    """16 384 x 1024 x 256: 64 x 4 = 256 tall tiles, K / 64 = 4 is the shortest main loop.  16 896 rows: 264 tiles, eight workgroups walk a second
    tile (the next tile's bias start from LDS, the first fragments read behind the epilogue).  22 528 x 768: three feature tiles, so a wave column
    without a partner tile.  K = 2048: FF2's loop length."""
    _check(M, N, K)


def test_row_mask():
    """One launch with whole-kept waves, wholly masked waves and waves with some of their eight token tiles / some of their rows masked (a wave owns
    128 consecutive token rows): masked rows keep their bits, and their statistics are those of the kept values."""
    M, N, K = 16384, 1024, 256
    g = torch.Generator().manual_seed(11)
    keep = torch.ones(M, dtype=torch.bool)
    wave = torch.arange(M) // 128
    keep[wave % 4 == 1] = False
    tile = (torch.arange(M) % 128) // 16
    keep[(wave % 4 == 2) & ((tile == 1) | (tile == 4) | (tile == 6))] = False
    keep[(wave % 4 == 3) & (torch.rand(M, generator=g) < 0.3)] = False
    first, x = _check(M, N, K, rowmask=keep)
    assert not torch.equal(first[0][keep], x[keep])


def test_clipping_at_the_fp16_range():
    """A stream scaled so that elements clip at +-65504 -- elements near the end of the range that an update of a few hundred carries past it (without
    the clamp their conversion gives infinity) and elements that sit on it already: the clipped bits, the planes and the range guard's words are
    the 8-wave kernel's."""
    first, x = _check(16384, 1024, 256, stream_scale=16000.0, gate_scale=200.0)
    clipped = int(((first[0].abs() == 65504.0) & (x.abs() < 65504.0)).sum())
    print(f"elements clipped by the update: {clipped}; guard {first[3]}")
    assert clipped > 0 and first[3][0] == 1  # the guard was raised


def test_fp16_precision_mode():
    """The first shape on the EL = f16_t build of the kernel (fp16 operands; the stream and the statistics are fp16 / fp32 in both modes)."""
    import gpu_helpers as G
    _check(16384, 1024, 256, precision=G.P_FP16)
