"""Silence removal on the device (`f5_op_silence_ranges`, `f5_wave_remove_silence`, `utils_infer.remove_silence`, `generate(remove_silence=True)`)
against the host functions it restates: `audio.split_on_silence` on `Segment(rounded PCM)`.  Every comparison is exact.  Small windows, steps and
paddings let waves of a few thousand samples reach every branch: the midpoint rule, the extra last window, leading and trailing silence, the
all-silent, no-silence and shorter-than-a-window cases, two silent ranges that must not merge, rates at which a millisecond is no whole number of
samples (unaligned heads and tails of the 16-byte loads) and sample counts that are no whole number of milliseconds."""
import numpy as np
import pytest
import torch

from eraxvif5tts_amd.infer import audio
from eraxvif5tts_amd.infer import utils_infer as U
from test_gpu_wave_tail import SR, TEXTS, _tts
from test_silence_host import _wave

pytestmark = pytest.mark.gpu
F5_EINVAL = -1

LAYOUTS = {
    "A": [(31, 8000), (47, 60), (29, 9000), (26, 50), (12, 7000), (55, 0), (23, 6000)],
    "B": [(40, 30), (50, 9000), (45, 20)],
    "C": [(90, 20)],
    "D": [(90, 9000)],
    "E": [(15, 9000)],
    "F": [(33, 9000), (21, 40), (9, 9000), (22, 40), (30, 8000)],
}
RULES = [(20, 7, 3), (20, 30, 3), (25, 5, 10), (20, 0, 1)]  # (min_silence_len, keep_silence, seek_step)
EXTRA = {"A": (7, 0.25), "B": (0, 0.0), "C": (13, 0.0), "D": (0, 0.0), "E": (5, 0.25), "F": (1, 0.25)}  # samples behind the last whole millisecond


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _truncating(x):
    return np.clip(np.trunc(x.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)


def _oracle(x, rate, L, db, keep, step):
    """host functions on Segment(rounded PCM): window flags, parts as sample ranges, the parts' PCM"""
    pcm = U.rounded_pcm16(x)
    seg = audio.Segment(pcm, rate, 2)
    n_ms = len(seg)
    flags = []
    if n_ms >= L:
        thresh = (10 ** (db / 20.0)) * seg.max_possible_amplitude
        last = n_ms - L
        starts = list(range(0, last + 1, step)) + ([last] if last % step else [])
        flags = [1 if seg.slice_ms(i, i + L).rms <= thresh else 0 for i in starts]
    parts = audio.split_on_silence(seg, L, db, keep, step)
    ranges = audio.split_sample_ranges(seg, L, db, keep, step)
    assert len(parts) == len(ranges) and all(np.array_equal(p.samples[:, 0], pcm[a:b]) for p, (a, b) in zip(parts, ranges))
    return np.array(flags, np.uint8), ranges, pcm


def _check(x, rate, L, db, keep, step, tag):
    """all of one case: the decision (flags, table, counts) and the three gathered outputs"""
    flags, ranges, pcm = _oracle(x, rate, L, db, keep, step)
    rule = dict(min_silence_len=L, silence_thresh=db, keep_silence=keep, seek_step=step)
    dev = torch.from_numpy(x).cuda()
    got_flags, table, kept, parts = U.silence_ranges(dev, rate, **rule)
    assert np.array_equal(got_flags, flags), (tag, "flags")
    want_table = np.zeros((len(ranges), 3), np.int32)
    pos = 0
    for k, (a, b) in enumerate(ranges):
        want_table[k] = (a, b, pos)
        pos += b - a
    assert parts == len(ranges) and kept == pos and np.array_equal(table, want_table), (tag, "table", table, want_table)
    trunc = _truncating(x)
    out, rounded, kept_pcm, parts2 = U.remove_silence_device(dev, rate, pcm16=torch.from_numpy(trunc).cuda(), want_rounded=True, **rule)
    cat = lambda a: np.concatenate([a[i:j] for i, j in ranges]) if ranges else a[:0]  # noqa: E731
    assert parts2 == len(ranges) and out.dtype == dev.dtype and out.numel() == rounded.numel() == kept_pcm.numel() == pos, (tag, "counts")
    assert out.cpu().numpy().tobytes() == cat(x).tobytes(), (tag, "float")
    assert np.array_equal(rounded.cpu().numpy(), cat(pcm)), (tag, "rounded PCM")
    assert np.array_equal(kept_pcm.cpu().numpy(), cat(trunc)), (tag, "truncating PCM")
    return len(ranges)


@pytest.mark.parametrize("rule", RULES, ids=lambda r: "L%d-keep%d-step%d" % r)
@pytest.mark.parametrize("rate", [24000, 22050, 16000])
def test_sweep_equals_split_on_silence(rate, rule):
    L, keep, step = rule
    seen = set()
    for name, layout in LAYOUTS.items():
        base = _wave(layout, rate, seed=ord(name))
        base = np.concatenate([base, np.full(*EXTRA[name])])
        for dtype in (np.float32, np.float64):
            x = np.ascontiguousarray(base.astype(dtype))
            seen.add(_check(x, rate, L, -50, keep, step, (name, rate, rule, np.dtype(dtype).name)))
    assert min(seen) == 0 and max(seen) >= 3  # nothing kept (C) .. several parts (A)


def test_unaligned_wave_pointers():
    """the wave starts 1, 2, 3 elements behind a 16-byte boundary (a slice of a tensor): heads and tails of the vector loads move"""
    layout = LAYOUTS["A"]
    for dtype in (np.float32, np.float64):
        base = _wave(layout, 22050, seed=5).astype(dtype)
        for shift in (1, 2, 3):
            flags, ranges, pcm = _oracle(base, 22050, 20, -50, 7, 3)
            buf = torch.zeros(len(base) + 8, dtype=torch.from_numpy(base).dtype, device="cuda")
            dev = buf[shift: shift + len(base)]
            dev.copy_(torch.from_numpy(base))
            got_flags, table, kept, parts = U.silence_ranges(dev, 22050, min_silence_len=20, silence_thresh=-50, keep_silence=7, seek_step=3)
            assert np.array_equal(got_flags, flags) and parts == len(ranges) and kept == sum(b - a for a, b in ranges)
            assert [tuple(r[:2]) for r in table.tolist()] == [tuple(r) for r in ranges]


def test_conversion_is_write_wavs(tmp_path):
    """ties, clipping and the value just below -1: the rounded PCM of the kept samples is what `write_wav` stores at those indices"""
    g = np.random.default_rng(4)
    k = g.integers(-32768, 32767, size=3000)
    ties = (k + 0.5) / 32767.0
    special = np.array([1.5, -1.5, -1.0000305, 1.0, -1.0, 0.5 / 32767.0, -0.5 / 32767.0, 1.5 / 32767.0, 2.5 / 32767.0, 32766.5 / 32767.0])
    base = np.concatenate([ties[:1500], special, np.zeros(int(0.06 * SR)), ties[1500:], special[::-1], np.full(int(0.03 * SR), 1e-4)])
    path = str(tmp_path / "c.wav")
    for dtype in (np.float64, np.float32):
        x = np.ascontiguousarray(base.astype(dtype))
        audio.write_wav(path, x, SR)
        with open(path, "rb") as fh:
            stored = np.frombuffer(fh.read()[44:], dtype="<i2")
        assert np.array_equal(stored, U.rounded_pcm16(x))
        assert _check(x, SR, 20, -50, 7, 3, ("conversion", np.dtype(dtype).name)) == 2
        ranges = audio.split_sample_ranges(audio.Segment(stored, SR, 2), 20, -50, 7, 3)
        _, rounded, _, _ = U.remove_silence_device(torch.from_numpy(x).cuda(), SR, min_silence_len=20, silence_thresh=-50, keep_silence=7,
                                                   seek_step=3, want_wave=False, want_rounded=True)
        assert np.array_equal(rounded.cpu().numpy(), np.concatenate([stored[a:b] for a, b in ranges]))


@pytest.mark.parametrize("amp,removed", [(103, 2400), (104, 0)])
def test_full_scale_windows_and_the_exact_threshold(amp, removed):
    """2 s at 24 kHz at the production values: everything at -32768 except 1.1 s of exactly `amp`.  floor(thresh) = 103: the 103 stretch is
    silent (0.1 s of it goes), the 104 stretch is not.  A window over the full-scale part sums to 2.58e13: 32-bit sums would wrap."""
    assert audio.silence_threshold_floor(-50) == 103
    x = np.full(2 * SR, -1.5)
    x[int(0.4 * SR): int(1.5 * SR)] = amp / 32767.0
    for dtype in (np.float32, np.float64):
        y = np.ascontiguousarray(x.astype(dtype))
        assert set(np.unique(U.rounded_pcm16(y))) == {-32768, amp}
        _check(y, SR, 1000, -50, 500, 10, ("width", amp, np.dtype(dtype).name))
        kept = U.remove_silence(torch.from_numpy(y).cuda(), SR)
        assert kept.numel() == 2 * SR - removed


def test_refusals_name_the_argument_and_touch_nothing():
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    n = 2400
    wave = torch.full((n,), 0.3, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((n,), 7.0, device="cuda")
    pcm = torch.full((n,), 7, dtype=torch.int16, device="cuda")
    counts = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    flags = torch.full((256,), 9, dtype=torch.uint8, device="cuda")
    table = torch.full((64, 3), -3, dtype=torch.int32, device="cuda")
    cases = [("min_silence_len", dict(L=174763)),  # 174763 ms at 24 kHz: 2^22 samples and more
             ("seek_step", dict(step=0)), ("keep_silence", dict(keep=-1))]
    for name, kw in cases:
        a = dict(L=20, keep=7, step=3)
        a.update(kw)
        rc = lib.f5_wave_remove_silence(_lib.ptr(wave), 0, n, SR, 100, a["L"], 103, a["keep"], a["step"], None, _lib.ptr(ws), ws.numel(),
                                        _lib.ptr(out), _lib.ptr(pcm), None, _lib.ptr(counts), _lib.stream_ptr())
        assert rc == F5_EINVAL and name in _lib.last_error(), (name, rc, _lib.last_error())
        rc = lib.f5_op_silence_ranges(_lib.ptr(wave), 0, n, SR, 100, a["L"], 103, a["keep"], a["step"], _lib.ptr(ws), ws.numel(), _lib.ptr(flags),
                                      _lib.ptr(table), _lib.ptr(counts), _lib.stream_ptr())
        assert rc == F5_EINVAL and name in _lib.last_error(), (name, rc, _lib.last_error())
        assert lib.f5_wave_remove_silence_workspace(n, SR, a["L"], a["step"]) == (F5_EINVAL if name != "keep_silence" else
                                                                                  lib.f5_wave_remove_silence_workspace(n, SR, 20, 3))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((pcm == 7).all()) and bool((counts == -5).all()) and bool((flags == 9).all())
    assert bool((table == -3).all()) and bool((ws == 0).all())
    # ... and the same call with the arguments in range runs
    rc = lib.f5_wave_remove_silence(_lib.ptr(wave), 0, n, SR, 100, 20, 103, 7, 3, None, _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.ptr(pcm),
                                    None, _lib.ptr(counts), _lib.stream_ptr())
    assert rc == 0 and counts.cpu().tolist() == [n, 1] and bool((out == 0.3).all())


# ---------------------------------------------------------------------------------------------------------------- the wrapper
@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    return _tts(tmp_path_factory.mktemp("silence_tts"), "bf16")


def _bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("cross_fade", [0.0, 0.15], ids=["fp32", "fp64"])
def test_generate_remove_silence_equals_the_file_route(tts, tmp_path, cross_fade):
    tts.target_rms = 0.2
    text, kw = TEXTS[2], dict(nfe_step=3, cross_fade_duration=cross_fade, return_numpy=True)
    plain, with_rs = str(tmp_path / "plain.wav"), str(tmp_path / "rs.wav")
    torch.manual_seed(41)
    wave, _ = tts.generate(text, output_path=plain, **kw)
    assert wave.dtype == (np.float64 if cross_fade > 0 else np.float32)
    untouched = _bytes(plain)
    torch.manual_seed(41)
    kept, rate, spec = tts.generate(text, output_path=with_rs, return_spectrogram=True, remove_silence=True, **kw)
    torch.manual_seed(41)
    wave_again, _, spec_plain = tts.generate(text, return_spectrogram=True, **kw)
    assert np.array_equal(wave_again, wave) and np.array_equal(spec, spec_plain)  # off: as before; the spectrogram is untouched
    U.remove_silence_for_generated_wav(plain)
    assert _bytes(with_rs) == _bytes(plain) and rate == SR
    want = U.remove_silence(wave, SR)
    assert kept.dtype == wave.dtype and kept.tobytes() == want.tobytes()
    audio.write_wav(plain, kept, SR)
    assert _bytes(plain) == _bytes(with_rs)
    print(f"generate(remove_silence) [{cross_fade}]: {len(wave)} samples, {len(kept)} kept, file unchanged: {_bytes(with_rs) == untouched}")
    torch.manual_seed(41)
    pcm, _ = tts.generate(text, return_pcm16=True, **kw)
    torch.manual_seed(41)
    kept_pcm, _ = tts.generate(text, return_pcm16=True, remove_silence=True, **kw)
    _, want_pcm = U.remove_silence(wave, SR, pcm16=pcm)
    assert kept_pcm.dtype == np.int16 and np.array_equal(kept_pcm, want_pcm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_post_tail_step_on_a_wave_with_pauses(tts, tmp_path, dtype):
    """random weights give no pauses, so the step behind the tail also runs on a constructed 3 s wave, at the production values"""
    x = _wave([(400, 9000), (1100, 20), (500, 8000), (1000, 0)], SR, seed=8)
    x = x.astype(np.float32 if dtype == torch.float32 else np.float64)
    trunc = _truncating(x)
    path = str(tmp_path / "w.wav")
    audio.write_wav(path, x, SR)
    U.remove_silence_for_generated_wav(path)
    kept, kept_pcm = tts._silence_step(torch.from_numpy(x).cuda(), torch.from_numpy(trunc).cuda())
    assert kept.is_cuda and kept.dtype == dtype and kept_pcm.is_cuda and 0 < kept.numel() < len(x)
    want, want_pcm = tts._silence_step(x, trunc)  # the host route of the same step
    assert kept.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(kept_pcm.cpu().numpy(), want_pcm)
    audio.write_wav(str(tmp_path / "k.wav"), kept.cpu().numpy(), SR)
    assert _bytes(str(tmp_path / "k.wav")) == _bytes(path)
    only, none = tts._silence_step(torch.from_numpy(x).cuda())
    assert none is None and torch.equal(only, kept)
    # all silent: empty arrays, a header-only file
    quiet = torch.zeros(3 * SR, dtype=dtype, device="cuda")
    kept, kept_pcm = tts._silence_step(quiet, torch.zeros(3 * SR, dtype=torch.int16, device="cuda"))
    assert kept.numel() == 0 and kept_pcm.numel() == 0 and kept.dtype == dtype
    audio.write_wav(path, kept.cpu().numpy(), SR)
    assert len(_bytes(path)) == 44


def test_host_tail_takes_the_host_route(tts):
    """a foreign vocoder object keeps the per-utterance host loop; the option then runs the host functions on its result"""
    vocos = tts.vocoder

    class Foreign(torch.nn.Module):
        def decode(self, mel):
            wave = torch.tanh(mel.mean(dim=1)).repeat_interleave(256, dim=1)[:, 256:] * 0.5
            wave[:, 2000: 2000 + int(1.3 * SR)] = 0.0  # a pause
            return wave

    tts.vocoder = Foreign()
    try:
        for kw in ({}, {"return_pcm16": True}):
            torch.manual_seed(12)
            plain, _ = tts.generate(TEXTS[2], nfe_step=3, return_numpy=True, cross_fade_duration=0.0, **kw)
            torch.manual_seed(12)
            kept, _ = tts.generate(TEXTS[2], nfe_step=3, return_numpy=True, cross_fade_duration=0.0, remove_silence=True, **kw)
            assert kept.dtype == plain.dtype and len(kept) <= len(plain)
            if not kw:
                wave = plain
                assert np.array_equal(kept, U.remove_silence(wave, SR))
            else:
                assert np.array_equal(kept, U.remove_silence(wave, SR, pcm16=plain)[1])
    finally:
        tts.vocoder = vocos
