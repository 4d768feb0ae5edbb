"""Op-level tests of the flow-matching kernels (include/f5hip.h: f5_cfm_noise, f5_cfm_loss; csrc/cfm_loss.hip) against the torch expressions of
reference cfm.py:257-283 run as separate eager ops on the device.

f5_cfm_noise: phi and cond bit for bit.  f5_cfm_loss: the elementwise values F.mse_loss(pred, x1 - x0, reduction="none") forms in fp32 are the
bits the kernel forms, so the reference sums the selected ones in fp64 on the host: `sums` to 1e-12 relative (non-negative terms, the same
fp32 values added in fp64, only the order differs; the kernel's order is a few sequential terms per lane and then trees, and every term passes
through fewer than 64 additions: under 1e-14 relative), `counts` exact, `loss` equal or one fp32 ulp apart, NaN for an empty selection, a
second run bit-equal.
Shapes: one row; a row count and width off the vector and workgroup sizes; an utterance spanning many workgroups; a width that is no
multiple of 4 (element loads); tensors 4 bytes off a 16-byte boundary (element loads at width 100)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eraxvif5tts_amd import _lib

pytestmark = pytest.mark.gpu
F5_EINVAL = -1
SHAPES = [(3, 37, 100), (1, 1, 100), (2, 1030, 100), (2, 5, 7)]
SPANS = ["random", "all", "none_for_one", "none", "padding"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _dev(t, misalign):
    """`t` on the device, contiguous; misalign: its first element 4 bytes behind a 16-byte boundary."""
    if not misalign:
        return t.cuda().contiguous()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _case(B, N, mel, span_kind, seed=0, misalign=False):
    g = torch.Generator().manual_seed(seed + 1000 * B + N + mel)
    x1 = torch.randn(B, N, mel, generator=g) * 2 - 3
    x0 = torch.randn(B, N, mel, generator=g)
    pred = torch.randn(B, N, mel, generator=g) * 1.5
    lens = torch.randint(1, N + 1, (B,), generator=g)
    lens[0] = N
    valid = torch.arange(N)[None, :] < lens[:, None]
    if span_kind == "random":
        span = torch.rand(B, N, generator=g) < 0.7
    elif span_kind == "all":
        span = torch.ones(B, N, dtype=torch.bool)
    elif span_kind == "none_for_one":
        span = torch.rand(B, N, generator=g) < 0.7
        span[B - 1] = False
    elif span_kind == "none":
        span = torch.zeros(B, N, dtype=torch.bool)
    else:  # a span inside each utterance's own frames, false on the padding rows (cfm.py:244-245)
        span = (torch.rand(B, N, generator=g) < 0.8) & valid
    x1, x0, pred = [_dev(t, misalign) for t in (x1, x0, pred)]
    return x1, x0, pred, span.cuda()


def _noise(x1, x0, time, span):
    lib = _lib.load()
    B, N, mel = x1.shape
    s8 = span.to(torch.uint8).contiguous()
    phi = torch.full_like(x1, float("nan"))
    cond = torch.full_like(x1, float("nan"))
    _lib.check(lib.f5_cfm_noise(B, N, mel, _lib.ptr(x1), _lib.ptr(x0), _lib.ptr(time), _lib.ptr(s8), _lib.ptr(phi), _lib.ptr(cond),
                                _lib.stream_ptr()), "f5_cfm_noise")
    return phi, cond


def _loss(pred, x1, x0, span):
    lib = _lib.load()
    B, N, mel = x1.shape
    s8 = span.to(torch.uint8).contiguous()
    nbytes = lib.f5_cfm_loss_workspace(B, N, mel)
    assert nbytes >= 8
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device="cuda")  # NaN bit patterns: a partial the kernels do not write shows
    sums = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    counts = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    loss = torch.full((1,), -1.0, device="cuda")
    _lib.check(lib.f5_cfm_loss(B, N, mel, _lib.ptr(pred), _lib.ptr(x1), _lib.ptr(x0), _lib.ptr(s8), _lib.ptr(sums), _lib.ptr(counts),
                               _lib.ptr(loss), _lib.ptr(work), _lib.stream_ptr()), "f5_cfm_loss")
    return loss.cpu(), sums.cpu(), counts.cpu()


def _times(B, seed):
    """time vectors holding t = 0 and t = 1"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(B, generator=g)
    a[0] = 1.0
    b = torch.rand(B, generator=g)
    b[B - 1] = 0.0
    return [a.cuda(), b.cuda()]


def _check_noise(x1, x0, span, time):
    phi, cond = _noise(x1, x0, time, span)
    t = time.unsqueeze(-1).unsqueeze(-1)
    want_phi = (1 - t) * x0 + t * x1  # cfm.py:259 as four eager ops
    want_cond = torch.where(span[..., None], torch.zeros_like(x1), x1)  # cfm.py:263
    assert torch.equal(phi, want_phi)
    assert torch.equal(cond, want_cond)


def _ulps_apart(a, b):
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))


def _check_loss(x1, x0, pred, span):
    B, N, mel = x1.shape
    loss, sums, counts = _loss(pred, x1, x0, span)
    elem = F.mse_loss(pred, x1 - x0, reduction="none").cpu()  # the fp32 values the kernel forms
    sp = span.cpu()
    want_sums = torch.stack([elem[b][sp[b]].double().sum() for b in range(B)])
    want_counts = sp.sum(dim=1) * mel
    print(f"  sums {sums.tolist()} want {want_sums.tolist()} loss {float(loss)}")
    assert torch.equal(counts, want_counts)
    for b in range(B):
        if int(want_counts[b]) == 0:
            assert float(sums[b]) == 0.0
        else:
            assert abs(float(sums[b]) - float(want_sums[b])) <= 1e-12 * float(want_sums[b]), b
    total = int(want_counts.sum())
    if total == 0:
        assert bool(torch.isnan(loss).all())  # mean() of an empty tensor
    else:
        want = np.float32(float(want_sums.sum()) / total)
        assert _ulps_apart(float(loss), want) <= 1, (float(loss), float(want))
    again = _loss(pred, x1, x0, span)
    assert np.array_equal(sums.numpy().view(np.int64), again[1].numpy().view(np.int64))  # bit-equal, NaN-proof
    assert np.array_equal(loss.numpy().view(np.int32), again[0].numpy().view(np.int32)) and torch.equal(counts, again[2])
    return loss, sums, counts


@pytest.mark.parametrize("span_kind", SPANS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_is_torch_bit_for_bit(shape, span_kind):
    B, N, mel = shape
    x1, x0, _, span = _case(B, N, mel, span_kind)
    for time in _times(B, seed=N):
        _check_noise(x1, x0, span, time)


@pytest.mark.parametrize("span_kind", SPANS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_matches_fp64_sum_of_the_fp32_squares(shape, span_kind):
    B, N, mel = shape
    x1, x0, pred, span = _case(B, N, mel, span_kind)
    _check_loss(x1, x0, pred, span)


def test_rows_outside_the_span_are_not_read():
    """NaN in every tensor on the rows outside the span: the loss is that of the selected rows alone."""
    x1, x0, pred, span = _case(3, 37, 100, "random")
    clean = _loss(pred, x1, x0, span)
    hole = (~span)[..., None]
    nan = torch.full_like(x1, float("nan"))
    dirty = _loss(torch.where(hole, nan, pred), torch.where(hole, nan, x1), torch.where(hole, nan, x0), span)
    assert torch.equal(clean[1], dirty[1]) and torch.equal(clean[0], dirty[0]) and bool(torch.isfinite(dirty[1]).all())


@pytest.mark.parametrize("shape", [(3, 37, 100), (2, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_tensors_take_element_loads(shape):
    B, N, mel = shape
    x1, x0, pred, span = _case(B, N, mel, "random", misalign=True)
    _check_noise(x1, x0, span, _times(B, seed=3)[0])
    got = _check_loss(x1, x0, pred, span)
    aligned = _loss(pred.clone(), x1.clone(), x0.clone(), span)  # the vector path at width 100: another order inside a lane, the same partition
    assert torch.equal(got[2], aligned[2])
    for b in range(B):
        assert abs(float(got[1][b]) - float(aligned[1][b])) <= 1e-12 * float(aligned[1][b])


def test_refusals():
    lib = _lib.load()
    B, N, mel = 2, 5, 8
    x = torch.zeros(B, N, mel, device="cuda")
    t = torch.zeros(B, device="cuda")
    s8 = torch.zeros(B, N, dtype=torch.uint8, device="cuda")
    sums, counts = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
    loss = torch.zeros(1, device="cuda")
    work = torch.zeros(lib.f5_cfm_loss_workspace(B, N, mel), dtype=torch.uint8, device="cuda")
    P, st = _lib.ptr, _lib.stream_ptr()
    phi, cond = torch.zeros_like(x), torch.zeros_like(x)
    noise_args = [P(x), P(x), P(t), P(s8), P(phi), P(cond)]
    loss_args = [P(x), P(x), P(x), P(s8), P(sums), P(counts), P(loss), P(work)]
    assert lib.f5_cfm_noise(B, N, mel, *noise_args, st) == 0 and lib.f5_cfm_loss(B, N, mel, *loss_args, st) == 0
    for bad in ((0, N, mel), (B, 0, mel), (B, N, 0), (-1, N, mel)):
        assert lib.f5_cfm_noise(*bad, *noise_args, st) == F5_EINVAL and _lib.last_error()
        assert lib.f5_cfm_loss(*bad, *loss_args, st) == F5_EINVAL and _lib.last_error()
        assert lib.f5_cfm_loss_workspace(*bad) == F5_EINVAL
    for i in range(len(noise_args)):
        a = list(noise_args)
        a[i] = None
        assert lib.f5_cfm_noise(B, N, mel, *a, st) == F5_EINVAL and "null" in _lib.last_error()
    for i in range(len(loss_args)):
        a = list(loss_args)
        a[i] = None
        assert lib.f5_cfm_loss(B, N, mel, *a, st) == F5_EINVAL and "null" in _lib.last_error()
    torch.cuda.synchronize()
