"""Silence removal, the host side: the three C entries are declared, bound and exported; `remove_silence_for_generated_wav` is
`audio.split_on_silence` at the reference's four values; the integer decision the device takes (`S < (R + 1)^2 n`) is `Segment.rms <= thresh`;
`remove_silence` on a numpy array is the file route; `generate()` has the keyword and `generate_stream()` has not.  Everything is exact."""
import inspect
import math
import os
import re

import numpy as np
import torch

from eraxvif5tts_amd.infer import audio
from eraxvif5tts_amd.infer import utils_infer as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 24000
ENTRIES = ("f5_wave_remove_silence", "f5_wave_remove_silence_workspace", "f5_op_silence_ranges")


def _wave(layout, rate=SR, seed=0):
    """(ms, amplitude) stretches -> float64 wave: a tone of that peak amplitude in int16 units (0: digital silence)"""
    g = np.random.default_rng(seed)
    parts = []
    for ms, amp in layout:
        n = int(ms * rate / 1000)
        parts.append(amp / 32767.0 * np.sin(2 * np.pi * 220 * np.arange(n) / rate + g.uniform(0, 6)))
    return np.concatenate(parts)


# every default matters: a 1.2 s pause (cut), a 0.8 s one (below min_silence_len: kept), two pauses 0.7 s of speech apart, speech that starts
# and ends the file.  (A silent range is never shorter than min_silence_len = 2 keep_silence, so at the reference's values padded neighbours
# can touch but not overlap: the midpoint rule is reached with keep_silence > min_silence_len / 2, in the last-but-one test and on the GPU.)
SPEECH = [(600, 9000), (1200, 20), (700, 8000), (1300, 0), (900, 7000), (800, 30), (500, 9000), (1100, 10), (400, 6000)]


def test_header_protos_and_exports_agree():
    from eraxvif5tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    declared = set(re.findall(r"\b(f5_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load(build_if_missing=True)
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.f5_version() == 400
    # the size entry needs no device: it answers bytes, or the refusal's code
    assert lib.f5_wave_remove_silence_workspace(30 * SR, SR, 1000, 10) >= (30000 + 1) * 8
    assert lib.f5_wave_remove_silence_workspace(100, SR, 1000, 0) == -1 and "seek_step" in _lib.last_error()
    assert lib.f5_wave_remove_silence_workspace(100, 999, 1000, 10) == -1 and "sample_rate" in _lib.last_error()
    assert lib.f5_wave_remove_silence_workspace(100, SR, 174763, 10) == -1 and "min_silence_len" in _lib.last_error()
    assert lib.f5_wave_remove_silence_workspace(1 << 31, SR, 1000, 10) == -1 and "n_samples" in _lib.last_error()


def test_file_route_is_split_on_silence_at_the_reference_defaults(tmp_path):
    wave = _wave(SPEECH)
    path = str(tmp_path / "gen.wav")
    audio.write_wav(path, wave, SR)
    seg = audio.Segment.from_file(path)
    parts = audio.split_on_silence(seg, min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10)
    assert len(parts) == 4
    want = np.concatenate([p.samples[:, 0] for p in parts])
    # each default matters: another value gives another result
    for other in (dict(min_silence_len=1250), dict(silence_thresh=-70), dict(keep_silence=100), dict(seek_step=700)):
        rule = dict(U.SILENCE_DEFAULTS, **other)
        got = audio.split_on_silence(seg, **rule)
        assert not np.array_equal(np.concatenate([p.samples[:, 0] for p in got]), want), other
    U.remove_silence_for_generated_wav(path)
    out, rate, width = audio.read_wav(path)
    assert rate == SR and width == 2 and 0 < len(want) < len(wave) and np.array_equal(out[:, 0], want)
    with open(path, "rb") as fh:
        assert len(fh.read()) == 44 + 2 * len(want)
    # an all-silent file becomes a header-only file
    audio.write_wav(path, _wave([(2500, 20)]), SR)
    U.remove_silence_for_generated_wav(path)
    with open(path, "rb") as fh:
        assert len(fh.read()) == 44


def test_integer_decision_equals_segment_rms():
    """`S < (R + 1)^2 * n` against `Segment.rms <= thresh` on 20 000 random windows of 1 .. 2999 samples whose amplitudes straddle the
    threshold, for the reference's -50 dB and two others; R comes from the helper the device route uses."""
    g = np.random.default_rng(11)
    for db, count in ((-50, 14000), (-40, 3000), (-16.5, 3000)):
        thresh = (10 ** (db / 20.0)) * 32768.0
        R = audio.silence_threshold_floor(db)
        assert R == math.floor(thresh)
        bad = 0
        for _ in range(count):
            n = int(g.integers(1, 3000))
            kind = g.integers(0, 3)
            if kind == 0:  # constant near the threshold, a few samples off by one
                x = np.full(n, R + int(g.integers(-1, 3)), dtype=np.int64)
                x[g.integers(0, n, size=max(1, n // 50))] += int(g.integers(-1, 2))
            elif kind == 1:  # noise whose rms is near the threshold
                x = np.rint(g.normal(0, R + g.uniform(-1.5, 2.5), size=n)).astype(np.int64)
            else:  # a sine whose rms is near the threshold
                x = np.rint((R + g.uniform(-1, 2)) * math.sqrt(2) * np.sin(np.arange(n) * g.uniform(0.01, 3) + g.uniform(0, 6))).astype(np.int64)
            x = np.clip(x, -32768, 32767)
            host = audio.Segment(x, SR, 2).rms <= thresh
            S = int(np.sum(x * x))
            bad += host != (S < (R + 1) ** 2 * n)
        assert bad == 0, (db, bad)
    assert audio.silence_threshold_floor(-50) == 103 and audio.silence_threshold_floor(40) == 32768
    # the widest case: full scale over a production window stays inside 64 bits and is loud
    assert 24000 * 32768 ** 2 > 2 ** 32 and not (24000 * 32768 ** 2 < 104 ** 2 * 24000)


def test_numpy_route_equals_the_file_route(tmp_path):
    wave = _wave(SPEECH, seed=3)
    wave[1000] = 1.5  # clipped in the file
    path = str(tmp_path / "gen.wav")
    for dtype in (np.float64, np.float32):
        x = wave.astype(dtype)
        audio.write_wav(path, x, SR)
        U.remove_silence_for_generated_wav(path)
        with open(path, "rb") as fh:
            want = fh.read()
        kept = U.remove_silence(x, SR)
        assert kept.dtype == dtype and 0 < len(kept) < len(x)
        audio.write_wav(path, kept, SR)
        with open(path, "rb") as fh:
            assert fh.read() == want
        trunc = (x.astype(np.float64) * 32767).clip(-32768, 32767).astype(np.int16)
        kept2, kept_pcm = U.remove_silence(x, SR, pcm16=trunc)
        assert np.array_equal(kept2, kept) and kept_pcm.dtype == np.int16 and len(kept_pcm) == len(kept)
        ranges = audio.split_sample_ranges(audio.Segment(U.rounded_pcm16(x), SR, 2), **U.SILENCE_DEFAULTS)
        assert np.array_equal(kept_pcm, np.concatenate([trunc[a:b] for a, b in ranges]))
        # a CPU tensor takes the same route and comes back as a tensor
        t = U.remove_silence(torch.from_numpy(x), SR)
        assert torch.is_tensor(t) and np.array_equal(t.numpy(), kept)
    # all silent: empty arrays
    kept, kept_pcm = U.remove_silence(np.zeros(3 * SR, np.float32), SR, pcm16=np.zeros(3 * SR, np.int16))
    assert kept.dtype == np.float32 and len(kept) == 0 and len(kept_pcm) == 0


def test_split_sample_ranges_cuts_where_split_on_silence_cuts():
    for rate, n_extra in ((SR, 0), (22050, 7), (16000, 3)):
        x = _wave([(31, 8000), (47, 60), (29, 9000), (26, 50), (12, 7000), (55, 0), (23, 6000)], rate)
        pcm = U.rounded_pcm16(np.concatenate([x, np.full(n_extra, 0.2)]))
        seg = audio.Segment(pcm, rate, 2)
        for L, keep, step in ((20, 7, 3), (20, 30, 3), (25, 5, 10), (20, 0, 1)):
            parts = audio.split_on_silence(seg, L, -50, keep, step)
            ranges = audio.split_sample_ranges(seg, L, -50, keep, step)
            assert len(parts) == len(ranges)
            for p, (a, b) in zip(parts, ranges):
                assert np.array_equal(p.samples[:, 0], pcm[a:b])


def test_generate_has_the_keyword_last_and_generate_stream_has_not():
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    params = list(inspect.signature(F5TTSWrapper.generate).parameters.values())
    assert params[-1].name == "remove_silence" and params[-1].default is False
    assert "remove_silence" not in inspect.signature(F5TTSWrapper.generate_stream).parameters
    sig = inspect.signature(U.remove_silence)
    assert [sig.parameters[k].default for k in ("min_silence_len", "silence_thresh", "keep_silence", "seek_step")] == [1000, -50, 500, 10]
    assert sig.parameters["sample_rate"].default == U.target_sample_rate and sig.parameters["pcm16"].default is None
