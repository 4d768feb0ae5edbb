"""Op-level tests of the distillation-loss kernel (include/f5hip.h: f5_distill_loss; csrc/distill_loss.hip) against the torch expressions of the
reference's distillation script (src/f5_tts/train/distil_reload.py:1070-1093) run as separate eager ops on the device.

The elementwise values F.mse_loss / F.l1_loss(reduction="none") form in fp32 are the bits the kernel forms, so the reference sums the selected
ones in fp64 on the host: each of the four sums per utterance to 1e-12 relative -- the bound tests/test_gpu_cfm_loss.py holds f5_cfm_loss to, for
the same summation scheme (non-negative terms, the same fp32 values added in fp64, only the order differs; every term passes through fewer than
64 additions: under 1e-14 relative) --, `frames` exact, each `batch` scalar within one fp32 ulp of the fp64 quotient, zeros for an empty span, a
second run bit-equal.
Shapes: two utterances over several workgroups; a row count off every vector and workgroup size; (1, 41, 100) = 4100 elements: two full chunks of
2048 and a ragged third; a width that is no multiple of 4 (element loads)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eraxvif5tts_amd import _lib

pytestmark = pytest.mark.gpu
F5_EINVAL = -1
SHAPES = [(2, 56, 100), (3, 37, 100), (1, 41, 100), (2, 5, 7)]
SPANS = ["random", "all", "none_for_one", "none"]


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
    teacher = torch.randn(B, N, mel, generator=g) * 1.5
    student = teacher + torch.randn(B, N, mel, generator=g) * 0.1
    if span_kind == "random":
        span = torch.rand(B, N, generator=g) < 0.7
    elif span_kind == "all":
        span = torch.ones(B, N, dtype=torch.bool)
    elif span_kind == "none_for_one":
        span = torch.rand(B, N, generator=g) < 0.7
        span[B - 1] = False
    else:
        span = torch.zeros(B, N, dtype=torch.bool)
    student, teacher, x1, x0 = [_dev(t, misalign) for t in (student, teacher, x1, x0)]
    return student, teacher, x1, x0, span.cuda()


def _run(student, teacher, x1, x0, span):
    lib = _lib.load()
    B, N, mel = x1.shape
    s8 = span.to(torch.uint8).contiguous()
    nbytes = lib.f5_distill_loss_workspace(B, N, mel)
    assert nbytes == B * -(-N * mel // 2048) * 4 * 8
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device="cuda")  # NaN bit patterns: a partial the kernels do not write shows
    sums = torch.full((B, 4), float("nan"), dtype=torch.float64, device="cuda")
    frames = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    batch = torch.full((4,), -1.0, device="cuda")
    _lib.check(lib.f5_distill_loss(B, N, mel, _lib.ptr(student), _lib.ptr(teacher), _lib.ptr(x1), _lib.ptr(x0), _lib.ptr(s8), _lib.ptr(sums),
                                   _lib.ptr(frames), _lib.ptr(batch), _lib.ptr(work), _lib.stream_ptr()), "f5_distill_loss")
    return sums.cpu(), frames.cpu(), batch.cpu()


def _ulps_apart(a, b):
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))


def _check(student, teacher, x1, x0, span):
    B, N, mel = x1.shape
    sums, frames, batch = _run(student, teacher, x1, x0, span)
    flow = x1 - x0  # distil_reload.py:1051, then :1070, (the teacher's own loss), :1075, :1077 -- the fp32 values the kernel forms
    elems = [e.cpu() for e in (F.mse_loss(student, flow, reduction="none"), F.mse_loss(teacher, flow, reduction="none"),
                               F.mse_loss(student, teacher, reduction="none"), F.l1_loss(student, teacher, reduction="none"))]
    sp = span.cpu()
    want = torch.stack([torch.stack([e[b][sp[b]].double().sum() for e in elems]) for b in range(B)])
    want_frames = sp.sum(dim=1)
    print(f"  sums {sums.tolist()} want {want.tolist()} batch {batch.tolist()}")
    assert torch.equal(frames, want_frames)
    for b in range(B):
        for k in range(4):
            if int(want_frames[b]) == 0:
                assert float(sums[b, k]) == 0.0
            else:
                assert abs(float(sums[b, k]) - float(want[b, k])) <= 1e-12 * float(want[b, k]), (b, k)
    total = int(want_frames.sum())
    for k in range(4):
        if total == 0:
            assert float(batch[k]) == 0.0  # the script's clamp(min=1): zero, not NaN
        else:
            assert _ulps_apart(float(batch[k]), np.float32(float(want[:, k].sum()) / total)) <= 1, (k, float(batch[k]))
    if total == 0:
        assert frames.tolist() == [0] * B
    again = _run(student, teacher, x1, x0, span)
    assert np.array_equal(sums.numpy().view(np.int64), again[0].numpy().view(np.int64))  # bit-equal, NaN-proof
    assert np.array_equal(batch.numpy().view(np.int32), again[2].numpy().view(np.int32)) and torch.equal(frames, again[1])
    return sums, frames, batch


@pytest.mark.parametrize("span_kind", SPANS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_match_fp64_sums_of_the_fp32_terms(shape, span_kind):
    B, N, mel = shape
    _check(*_case(B, N, mel, span_kind))


def test_student_equal_to_teacher_gives_exact_zeros():
    student, teacher, x1, x0, span = _case(3, 37, 100, "random")
    sums, _, batch = _run(teacher, teacher, x1, x0, span)
    assert sums[:, 2].tolist() == [0.0] * 3 and sums[:, 3].tolist() == [0.0] * 3 and batch[2:].tolist() == [0.0, 0.0]
    assert torch.equal(sums[:, 0], sums[:, 1]) and bool((sums[:, 0] > 0).all())


def test_rows_outside_the_span_are_not_read():
    """NaN in every tensor on the rows outside the span: the sums are those of the selected rows alone."""
    student, teacher, x1, x0, span = _case(3, 37, 100, "random")
    clean = _run(student, teacher, x1, x0, span)
    hole = (~span)[..., None]
    nan = torch.full_like(x1, float("nan"))
    dirty = _run(*[torch.where(hole, nan, t) for t in (student, teacher, x1, x0)], span)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[2], dirty[2]) and bool(torch.isfinite(dirty[0]).all())


@pytest.mark.parametrize("shape", [(3, 37, 100), (2, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_tensors_take_element_loads(shape):
    B, N, mel = shape
    student, teacher, x1, x0, span = _case(B, N, mel, "random", misalign=True)
    got = _check(student, teacher, x1, x0, span)
    aligned = _run(student.clone(), teacher.clone(), x1.clone(), x0.clone(), span)  # the vector path at width 100: another order inside a lane
    assert torch.equal(got[1], aligned[1])
    for b in range(B):
        for k in range(4):
            assert abs(float(got[0][b, k]) - float(aligned[0][b, k])) <= 1e-12 * float(aligned[0][b, k])


def test_refusals():
    lib = _lib.load()
    B, N, mel = 2, 5, 8
    x = torch.zeros(B, N, mel, device="cuda")
    s8 = torch.zeros(B, N, dtype=torch.uint8, device="cuda")
    sums, frames = torch.zeros(B, 4, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
    batch = torch.zeros(4, device="cuda")
    work = torch.zeros(lib.f5_distill_loss_workspace(B, N, mel) + 8, dtype=torch.uint8, device="cuda")
    P, st = _lib.ptr, _lib.stream_ptr()
    args = [P(x), P(x), P(x), P(x), P(s8), P(sums), P(frames), P(batch), P(work)]
    assert lib.f5_distill_loss(B, N, mel, *args, st) == 0
    for bad in ((0, N, mel), (B, 0, mel), (B, N, 0), (-1, N, mel)):
        assert lib.f5_distill_loss(*bad, *args, st) == F5_EINVAL and _lib.last_error()
        assert lib.f5_distill_loss_workspace(*bad) == F5_EINVAL
    assert lib.f5_distill_loss_workspace(1, 1 << 20, 1 << 12) == F5_EINVAL  # N * mel beyond 2^31: the limits of the flow-matching loss
    for i in range(len(args)):
        a = list(args)
        a[i] = None
        assert lib.f5_distill_loss(B, N, mel, *a, st) == F5_EINVAL and "null" in _lib.last_error()
    a = list(args)
    a[8] = _lib.C.c_void_p(work.data_ptr() + 4)  # a workspace that is not 8-byte aligned
    assert lib.f5_distill_loss(B, N, mel, *a, st) == F5_EINVAL and "aligned" in _lib.last_error()
    torch.cuda.synchronize()
