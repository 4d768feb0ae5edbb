"""The duration-validation kernels (include/f5hip.h: f5_align_similarity, f5_align_viterbi, f5_align_window, f5_duration_loss; csrc/align.hip)
and their Python surface (model/alignment_utils.py, eval/validate.py: duration_validation_loss).

The searches: alignment and durations equal the matrices captured from the reference (tests/golden/alignment.npz) and the numpy restatement
(tests/alignment_ref.py) element for element, no tolerance, on every case; where the reference's window search raises (an empty search
window, nt > T) there is no golden and the restatement alone stands, with the rule f5hip.h documents.
Similarity against the fp64 restatement: -inf positions identical, finite entries within (K + 2 mel + 16) * 2^-23 absolute -- the worst-case
fp32 dot-product bound for unit-norm operands (K products and adds of terms whose absolute sum is at most 1: K * 2^-24 * 2) plus the
projection's own mel-term dot products on both sides of its normalisation and the roundings of the norms, divisions and the + 3.0 bias.
Derived, not measured.  The search is then checked END TO END on the device's own similarity: the restatement aligns the copied buffer, so
similarity rounding can neither hide a search error nor cause a false one.
Loss: the per-utterance sums against fp64 host sums of the same fp32 inputs to 1e-12 relative (N < 1000 terms: N * 2^-52 plus a few ulp of
log / exp), counts exact."""
import functools

import numpy as np
import pytest
import torch

import alignment_ref as R
from conftest import load_golden
from eraxvif5tts_amd import _lib

pytestmark = pytest.mark.gpu
F5_EINVAL = -1
CASE_NAMES = list(R.generate_cases())


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@functools.lru_cache(maxsize=None)
def _golden():
    return R.golden_cases(load_golden("alignment"))


@functools.lru_cache(maxsize=None)
def _restated(name, alg):
    out = R.SEARCH[alg](_golden()[name][0])
    out.setflags(write=False)
    return out


def _search(sim, alg, want_alignment=True):
    """Raw entry point on a device fp32 [B, nt, T]; outputs pre-filled with NaN and the workspace with 0xff: a cell the kernel skips shows."""
    lib = _lib.load()
    B, nt, T = sim.shape
    nbytes = lib.f5_align_workspace(B, nt, T)
    assert nbytes == B * nt * T * 4
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device="cuda")
    dur = torch.full((B, nt), float("nan"), device="cuda")
    ali = torch.full((B, nt, T), float("nan"), device="cuda") if want_alignment else None
    fn = {"viterbi": lib.f5_align_viterbi, "window": lib.f5_align_window}[alg]
    _lib.check(fn(B, nt, T, _lib.ptr(sim), _lib.ptr(dur), _lib.ptr(ali), _lib.ptr(work), _lib.stream_ptr()), alg)
    return (ali.cpu().numpy() if want_alignment else None), dur.cpu().numpy()


def _check_search(sim_np, alg, want):
    sim = torch.from_numpy(sim_np).cuda().contiguous()
    ali, dur = _search(sim, alg)
    assert np.array_equal(ali, want), f"{int((ali != want).sum())} of {want.size} cells differ"
    assert np.array_equal(ali.sum(axis=1), np.ones((sim.shape[0], sim.shape[2]), np.float32))  # every column has one owner
    assert np.array_equal(dur, want.sum(axis=2))
    _, dur_only = _search(sim, alg, want_alignment=False)
    assert np.array_equal(dur_only, dur)


@pytest.mark.parametrize("alg", R.ALGORITHMS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_search_equals_reference_and_restatement_exactly(name, alg):
    sim, golden = _golden()[name]
    want = _restated(name, alg)
    if golden[alg] is not None:
        assert np.array_equal(want, golden[alg])
    else:
        assert alg == "window" and R.window_has_empty_search(sim)
    _check_search(sim, alg, want)


@pytest.mark.parametrize("alg", R.ALGORITHMS)
def test_python_surface_returns_the_same_matrices(alg):
    from eraxvif5tts_amd.model.alignment_utils import alignment_durations, get_durations_from_alignment, monotonic_alignment_search
    for name in ("ragged", "nt70_T33", "integer"):
        sim = torch.from_numpy(_golden()[name][0])
        a = monotonic_alignment_search(sim.cuda(), algorithm=alg)
        assert a.is_cuda and np.array_equal(a.cpu().numpy(), _restated(name, alg))
        d = alignment_durations(sim, alg)  # (a host tensor is moved)
        assert torch.equal(d, get_durations_from_alignment(a))
    assert np.array_equal(monotonic_alignment_search(torch.from_numpy(_golden()["ragged"][0]).cuda()).cpu().numpy(), _restated("ragged", "viterbi"))


# ----------------------------------------------------------------------------- similarity
def _similarity_case(K, mel, B, nt, T, p_lens, m_lens, seed):
    g = torch.Generator().manual_seed(seed)
    rows = 23
    embed = torch.randn(rows, K, generator=g)
    ids = torch.randint(0, rows, (B, nt), generator=g, dtype=torch.int32)
    melspec = torch.randn(B, T, mel, generator=g) * 2 - 1
    proj = torch.randn(mel, K, generator=g) / mel ** 0.5
    return embed, ids, torch.tensor(p_lens, dtype=torch.int32), melspec, torch.tensor(m_lens, dtype=torch.int32), proj


def _device_similarity(embed, ids, p_lens, melspec, m_lens, proj):
    lib = _lib.load()
    B, nt = ids.shape
    T, mel = melspec.shape[1:]
    rows, K = embed.shape
    dev = [t.cuda().contiguous() for t in (embed, ids, p_lens, melspec, m_lens, proj)]
    sim = torch.full((B, nt, T), float("nan"), device="cuda")
    _lib.check(lib.f5_align_similarity(B, nt, T, mel, K, rows, *[_lib.ptr(t) for t in dev], _lib.ptr(sim), _lib.stream_ptr()), "similarity")
    return sim


SIM_SHAPES = [(192, 100, 3, 9, 37, (9, 5, 0), (37, 21, 30)), (7, 5, 3, 9, 37, (9, 5, 0), (37, 21, 30)),
              (192, 100, 2, 70, 130, (70, 33), (101, 130)), (7, 5, 2, 70, 130, (70, 33), (101, 130))]


@pytest.mark.parametrize("shape", SIM_SHAPES, ids=lambda s: f"K{s[0]}_mel{s[1]}_{s[2]}x{s[3]}x{s[4]}")
def test_similarity_within_the_fp32_bound_and_search_end_to_end(shape):
    K, mel = shape[:2]
    case = _similarity_case(*shape, seed=K + shape[3])
    sim = _device_similarity(*case)
    got = sim.cpu().numpy()
    want = R.similarity64(*[t.numpy() for t in case])
    assert not np.isnan(got).any()
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isposinf(got).any()
    finite = np.isfinite(want)
    err = float(np.abs(got[finite].astype(np.float64) - want[finite]).max())
    bound = (K + 2 * mel + 16) * 2.0 ** -23
    print(f"  similarity max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float(want[finite].max()) > 2.0  # the + 3.0 bias is in the picture
    for alg in R.ALGORITHMS:
        ali, dur = _search(sim, alg)
        ref = R.SEARCH[alg](got)
        assert np.array_equal(ali, ref) and np.array_equal(dur, ref.sum(axis=2)), alg


def test_similarity_of_an_id_outside_the_table_reads_nothing():
    case = list(_similarity_case(7, 5, 1, 4, 6, (4,), (6,), seed=1))
    case[1] = torch.tensor([[0, 23, -1, 2 ** 30]], dtype=torch.int32)
    got = _device_similarity(*case).cpu().numpy()
    want = R.similarity64(torch.cat([case[0], torch.zeros(1, 7)]).numpy(), np.array([[0, 23, 23, 23]]), [4], case[3].numpy(), [6], case[5].numpy())
    assert np.abs(got - want).max() <= (7 + 2 * 5 + 16) * 2.0 ** -23


# ----------------------------------------------------------------------------- loss
def _ulps_apart(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _device_loss(logw, dur, p_lens):
    lib = _lib.load()
    B, nt = logw.shape
    sq = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    ab = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    cnt = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    pair = torch.full((2,), float("nan"), device="cuda")
    _lib.check(lib.f5_duration_loss(B, nt, _lib.ptr(logw), _lib.ptr(dur), _lib.ptr(p_lens), _lib.ptr(sq), _lib.ptr(ab), _lib.ptr(cnt),
                                    _lib.ptr(pair), _lib.stream_ptr()), "f5_duration_loss")
    return sq.cpu().numpy(), ab.cpu().numpy(), cnt.cpu().numpy(), pair.cpu().numpy()


def _check_loss(logw, dur, p_lens):
    got = _device_loss(logw.cuda().contiguous(), dur.cuda().contiguous(), p_lens.cuda().contiguous())
    sq, ab, cnt, loss, mae = R.duration_loss64(logw.numpy(), dur.numpy(), p_lens.numpy())
    print(f"  sq {got[0].tolist()} want {sq.tolist()}; ab {got[1].tolist()} want {ab.tolist()}; pair {got[3].tolist()} want {(loss, mae)}")
    assert np.array_equal(got[2], cnt)
    for b in range(len(cnt)):
        if cnt[b] == 0:
            assert got[0][b] == 0.0 and got[1][b] == 0.0
        else:
            assert abs(got[0][b] - sq[b]) <= 1e-12 * sq[b] and abs(got[1][b] - ab[b]) <= 1e-12 * ab[b], b
    assert _ulps_apart(got[3][0], loss) <= 1 and _ulps_apart(got[3][1], mae) <= 1  # fp64 ratios with the + 1e-8 denominator, rounded to fp32
    again = _device_loss(logw.cuda().contiguous(), dur.cuda().contiguous(), p_lens.cuda().contiguous())
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    return got


def test_duration_loss_sums_against_fp64():
    g = torch.Generator().manual_seed(5)
    B, nt = 3, 300
    logw = torch.randn(B, nt, generator=g) * 3
    logw[0, :4] = torch.tensor([12.0, -11.0, 10.0, -10.0])  # both sides of the clamp
    dur = torch.randint(0, 9, (B, nt), generator=g).float()  # zeros take the 0.1 floor
    got = _check_loss(logw, dur, torch.tensor([300, 117, 0], dtype=torch.int32))
    assert got[2].tolist() == [300, 117, 0] and got[0][2] == 0.0 and got[1][2] == 0.0
    _check_loss(logw[:, :1].contiguous(), dur[:, :1].contiguous(), torch.tensor([1, 1, 1], dtype=torch.int32))


def test_duration_loss_of_an_empty_batch_is_zero_over_1e_minus_8():
    got = _check_loss(torch.randn(2, 5), torch.ones(2, 5), torch.tensor([0, 0], dtype=torch.int32))
    assert got[3].tolist() == [0.0, 0.0] and got[2].tolist() == [0, 0]


# ----------------------------------------------------------------------------- duration_validation_loss
def _predictor(seed=0):
    from eraxvif5tts_amd.model import DurationPredictor
    torch.manual_seed(seed)
    return DurationPredictor(text_num_embeds=30, in_channels=24, filter_channels=32, kernel_size=3, p_dropout=0.1).cuda().eval()


def _batches():
    g = torch.Generator().manual_seed(11)
    out = []
    for B, nt, T, p_lens, m_lens in ((3, 9, 41, (9, 9, 6), (41, 30, 41)), (2, 5, 17, (5, 5), (17, 12))):
        out.append((torch.randn(B, T, 10, generator=g), torch.tensor(m_lens), torch.randint(0, 30, (B, nt), generator=g), torch.tensor(p_lens)))
    return out


@pytest.mark.parametrize("alg", R.ALGORITHMS)
def test_duration_validation_loss_is_the_composition_of_its_pieces(alg):
    from eraxvif5tts_amd.eval import duration_validation_loss
    from eraxvif5tts_amd.model.alignment_utils import alignment_durations, alignment_similarity
    pred, batches = _predictor(), _batches()
    r = duration_validation_loss(pred, batches, algorithm=alg, seed=3)
    proj = torch.randn(10, 24, generator=torch.Generator().manual_seed(3)) / 10 ** 0.5
    at, sq_all, ab_all, cnt_all = 0, [], [], []
    for i, (mel, m_lens, ids, p_lens) in enumerate(batches):
        B, nt = ids.shape
        sim = alignment_similarity(pred, ids, p_lens, mel, m_lens, proj)
        dur = alignment_durations(sim, alg)
        assert np.array_equal(dur.cpu().numpy(), R.SEARCH[alg](sim.cpu().numpy()).sum(axis=2))
        mask = torch.arange(nt)[None, :] < p_lens[:, None]
        logw = pred(ids, mask).reshape(B, nt)
        sq, ab, cnt, loss, mae = R.duration_loss64(logw.cpu().numpy(), dur.cpu().numpy(), p_lens.numpy())
        assert r.counts[at:at + B].tolist() == cnt.tolist()
        assert np.allclose(r.sq_sums[at:at + B].numpy(), sq, rtol=1e-12, atol=0) and np.allclose(r.abs_sums[at:at + B].numpy(), ab, rtol=1e-12, atol=0)
        assert _ulps_apart(r.batch_losses[i][0], loss) <= 1 and _ulps_apart(r.batch_losses[i][1], mae) <= 1
        sq_all += sq.tolist()
        ab_all += ab.tolist()
        cnt_all += cnt.tolist()
        at += B
    assert r.loss == pytest.approx(sum(sq_all) / sum(cnt_all), rel=1e-12) and r.mae == pytest.approx(sum(ab_all) / sum(cnt_all), rel=1e-12)
    again = duration_validation_loss(pred, batches, algorithm=alg, seed=3)
    assert again.sq_sums.numpy().tobytes() == r.sq_sums.numpy().tobytes() and again.abs_sums.numpy().tobytes() == r.abs_sums.numpy().tobytes()
    assert again.batch_losses == r.batch_losses and again.loss == r.loss and again.mae == r.mae
    given = duration_validation_loss(pred, batches, algorithm=alg, mel_proj_matrix=proj)
    assert given.sq_sums.numpy().tobytes() == r.sq_sums.numpy().tobytes()


def test_duration_validation_loss_refuses_what_it_cannot_run():
    from eraxvif5tts_amd.eval import duration_validation_loss
    pred, batches = _predictor(), _batches()
    mel, m_lens, ids, p_lens = batches[1]
    for bad in (30, 31, -1):  # forward() embeds id + 1 in a table of 31 rows
        ids_bad = ids.clone()
        ids_bad[1, 2] = bad
        with pytest.raises(ValueError, match="batch 1"):
            duration_validation_loss(pred, [batches[0], (mel, m_lens, ids_bad, p_lens)])
    with pytest.raises(ValueError):
        duration_validation_loss(pred, batches, algorithm="progressive")
    with pytest.raises(ValueError):
        duration_validation_loss(pred, [])


def test_shapes_beyond_the_limits_are_refused():
    lib = _lib.load()
    P, st = _lib.ptr, _lib.stream_ptr()
    x = torch.zeros(2 * 3 * 4, device="cuda")
    i32 = torch.ones(8, dtype=torch.int32, device="cuda")
    work = torch.zeros(2 * 3 * 4, dtype=torch.int32, device="cuda")
    assert lib.f5_align_workspace(2, 1024, 4096) == 2 * 1024 * 4096 * 4
    for bad in ((2, 1025, 4), (2, 3, 65537), (0, 3, 4), (2, 0, 4), (2, 3, 0), (-1, 3, 4)):
        assert lib.f5_align_workspace(*bad) == F5_EINVAL and _lib.last_error()
        assert lib.f5_align_viterbi(*bad, P(x), P(x), P(x), P(work), st) == F5_EINVAL and "align" in _lib.last_error()
        assert lib.f5_align_window(*bad, P(x), P(x), P(x), P(work), st) == F5_EINVAL
        assert lib.f5_align_similarity(*bad, 5, 7, 8, P(x), P(i32), P(i32), P(x), P(i32), P(x), P(x), st) == F5_EINVAL
    assert lib.f5_align_similarity(1, 2, 3, 2, 769, 2, P(x), P(i32), P(i32), P(x), P(i32), P(x), P(x), st) == F5_EINVAL and "K" in _lib.last_error()
    assert lib.f5_align_viterbi(2, 3, 4, None, P(x), P(x), P(work), st) == F5_EINVAL and "null" in _lib.last_error()
    assert lib.f5_align_viterbi(2, 3, 4, P(x), P(x), None, None, st) == F5_EINVAL and "null" in _lib.last_error()
    assert lib.f5_align_window(2, 3, 4, P(x), None, None, None, st) == F5_EINVAL and "null" in _lib.last_error()
    f64, i64 = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    assert lib.f5_duration_loss(0, 3, P(x), P(x), P(i32), P(f64), P(f64), P(i64), P(x), st) == F5_EINVAL
    assert lib.f5_duration_loss(2, 3, P(x), P(x), P(i32), P(f64), None, P(i64), P(x), st) == F5_EINVAL and "null" in _lib.last_error()
    d = torch.zeros(2 * 3, device="cuda")
    assert lib.f5_align_viterbi(2, 3, 4, P(x), P(d), None, P(work), st) == 0 and lib.f5_align_window(2, 3, 4, P(x), P(d), None, None, st) == 0
    torch.cuda.synchronize()
