"""The reference-voice rule as tables and integers (no GPU): `audio.edge_threshold_integers` against the float dBFS comparisons over every
integer rms, `audio.reference_sample_ranges` against ``remove_silence_edges(clip_reference(seg))`` on clips that reach each branch, and the
wrapper's ``on_device`` keyword on the host route.  The clip builders and the parametrised oracle are shared with tests/test_gpu_reference.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eraxvif5tts_amd.infer import audio  # noqa: E402

MSG = "Audio is over 12s, clipping short. (%d)"
REAL = dict(passes=((1000, -50), (100, -40)), keep=1000, step=10, soft=6000, hard=12000, T=-42, chunk=10, pad=50)


# ----------------------------------------------------------------------------- clips
def build_clip(layout, rate, channels, seed=0, extra=0, loud=3000.0):
    """``layout``: (kind, milliseconds) pieces -> a 16-bit Segment.  "speech": noise of rms ``loud`` (about -21 dB at 3000); "pause": noise of
    rms 20 (-64 dB: silent for every threshold used); "quiet": +-200 with random signs, rms exactly 200 over any slice (-44 dB: kept at -50 dB, silent at -40 and below the -42 dB edge).
    ``extra`` more frames of speech at the end keep the length off a whole millisecond.  The second channel is an independent draw."""
    rng = np.random.RandomState(seed)
    level = dict(speech=loud, pause=20.0)

    def piece(kind, count):
        return 200.0 * rng.choice([-1.0, 1.0], count) if kind == "quiet" else rng.normal(0.0, level[kind], count)

    cols = []
    for _ in range(channels):
        pieces = [piece(kind, int(ms * rate / 1000.0)) for kind, ms in layout]
        pieces.append(rng.normal(0.0, loud, extra))
        cols.append(np.concatenate(pieces))
    x = np.clip(np.round(np.stack(cols, axis=1)), -32768, 32767).astype(np.int32)
    return audio.Segment(x, rate, 2)


def repeat(pattern, total_ms):
    out, t = [], 0
    while t < total_ms:
        for kind, ms in pattern:
            out.append((kind, ms))
            t += ms
    return out


# kind -> (layout in ms, the (n) of the messages the host route shows)
REAL_CLIPS = {
    "short": ([("speech", 2500)], []),
    "long_pauses": (repeat([("speech", 3400), ("pause", 1200)], 13800) + [("speech", 3400)], [1]),
    "short_pauses": (repeat([("speech", 1200), ("pause", 280)], 14500), [2]),
    "no_pause": ([("speech", 12600)], [3]),
    "quiet_edges": ([("quiet", 430), ("speech", 2000), ("quiet", 310)], []),
    "all_silent": ([("pause", 1800)], []),
    "under_a_window": ([("speech", 640)], []),
}


# ----------------------------------------------------------------------------- the rule with its numbers as parameters
def oracle(seg, clip_short=True, passes=REAL["passes"], keep=1000, step=10, soft=6000, hard=12000, T=-42, chunk=10, pad=50):
    """clip_reference / remove_silence_edges / the pad with every constant a parameter, from `audio.split_on_silence`, `Segment` and
    `audio.detect_leading_silence`; with the defaults it is those functions (test_oracle_is_the_host_route)."""
    n = seg.samples.shape[0]

    def gather(min_len, thresh):
        out, rows = seg.silent_like(0), []
        parts = audio.split_on_silence(seg, min_len, thresh, keep, step)
        ranges = audio.split_sample_ranges(seg, min_len, thresh, keep, step)
        assert [p.samples.shape[0] for p in parts] == [b - a for a, b in ranges]
        for part, r in zip(parts, ranges):
            if len(out) > soft and len(out + part) > hard:
                return out, rows, True
            out, rows = out + part, rows + [r]
        return out, rows, False

    clip, pass2 = 0, False
    if clip_short:
        wave, rows, hit = gather(*passes[0])
        clip |= int(hit)
        pass2 = len(wave) > hard
        if pass2:
            wave, rows, hit = gather(*passes[1])
            clip |= 2 * int(hit)
        if len(wave) > hard:
            wave = wave.slice_ms(0, hard)
            rows = audio.cut_sample_ranges(rows, 0, wave.samples.shape[0])
            clip |= 4
    else:
        wave, rows = seg, [(0, n)]
    assert np.array_equal(wave.samples, np.concatenate([seg.samples[a:b] for a, b in rows]) if rows else seg.samples[:0])
    lead = audio.detect_leading_silence(wave, T, chunk)
    edge = wave.slice_ms(lead, None)
    trail = 0
    for ms in range(len(edge) - 1, -1, -1):
        if edge.slice_ms(ms, ms + 1).dBFS > T:
            break
        trail += 1
    cut_ms = audio.trailing_cut_ms(edge.samples.shape[0], seg.frame_rate, trail)
    final = edge.slice_ms(0, cut_ms)
    return dict(rows=[r for r in rows if r[1] > r[0]], clip=clip, pass2=int(pass2), gathered=wave.samples.shape[0], gathered_ms=len(wave),
                lead_ms=lead, lead_frame=min(wave._frame(lead), wave.samples.shape[0]), edge_frames=edge.samples.shape[0], edge_ms=len(edge),
                trail_ms=trail, cut_ms=cut_ms, kept=final.samples.shape[0], final=final, padded=final + final.silent_like(pad))


def host_route(seg, clip_short=True):
    said = []
    out = audio.clip_reference(seg, said.append) if clip_short else seg
    return audio.remove_silence_edges(out), said


# ----------------------------------------------------------------------------- tests
@pytest.mark.parametrize("T,expect", [(-42, 261), (-50, 104), (-40, 328)])
def test_edge_threshold_integers_are_the_float_comparisons(T, expect):
    r_lead, r_trail = audio.edge_threshold_integers(T)
    assert (r_lead, r_trail) == (expect, expect)
    below, above = [], []
    for r in range(32769):
        seg_dbfs = -float("inf") if r == 0 else 20.0 * math.log10(r / 32768.0)  # Segment.dBFS at rms r
        below.append(seg_dbfs < T)
        above.append(seg_dbfs > T)
    assert below == [r < r_lead for r in range(32769)]  # (so the predicate is monotone: true up to r_lead - 1, false from there)
    assert above == [r >= r_trail for r in range(32769)]
    # the float predicate and Segment agree on what dBFS is
    probe = audio.Segment(np.full((64, 1), expect, np.int32), 8000, 2)
    assert probe.rms == expect and probe.dBFS == 20.0 * math.log10(expect / 32768.0)


def test_edge_threshold_integers_without_a_crossing():
    assert audio.edge_threshold_integers(0.0) == (32768, 32769)  # dBFS reaches 0 at full scale and never exceeds it
    assert audio.edge_threshold_integers(-200.0) == (1, 1)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [8000, 22050, 24000, 44100])
@pytest.mark.parametrize("kind", list(REAL_CLIPS))
def test_reference_sample_ranges_is_the_host_route(kind, rate, channels):
    layout, numbers = REAL_CLIPS[kind]
    seg = build_clip(layout, rate, channels, seed=len(kind) + rate % 97, extra=0 if kind == "quiet_edges" else 5)  # (loud frames at the end)
    want, said = host_route(seg)
    assert said == [MSG % k for k in numbers]  # the branch this clip is here for
    ranges, messages = audio.reference_sample_ranges(seg)
    assert messages == said
    assert all(0 <= a < b <= seg.samples.shape[0] for a, b in ranges) and all(b <= c for (_, b), (c, _) in zip(ranges, ranges[1:]))
    got = np.concatenate([seg.samples[a:b] for a, b in ranges]) if ranges else seg.samples[:0]
    assert got.shape == want.samples.shape and np.array_equal(got, want.samples)
    if kind == "quiet_edges":
        assert ranges[0][0] >= int(0.4 * rate) and ranges[-1][1] <= seg.samples.shape[0] - int(0.25 * rate)  # both edges were trimmed
    if kind == "all_silent":
        assert ranges == []


@pytest.mark.parametrize("rate,channels", [(8000, 1), (22050, 2)])
def test_reference_sample_ranges_without_clipping(rate, channels):
    seg = build_clip(REAL_CLIPS["no_pause"][0], rate, channels, seed=3, extra=2)
    want, said = host_route(seg, clip_short=False)
    ranges, messages = audio.reference_sample_ranges(seg, clip_short=False)
    assert said == messages == [] and len(want) > 12000
    assert np.array_equal(np.concatenate([seg.samples[a:b] for a, b in ranges]), want.samples)


@pytest.mark.parametrize("kind", list(REAL_CLIPS))
def test_oracle_is_the_host_route(kind):
    """the parametrised restatement the device tests compare with is, at the real constants, the host functions themselves"""
    layout, numbers = REAL_CLIPS[kind]
    seg = build_clip(layout, 11025, 2, seed=11, extra=4)
    want, said = host_route(seg)
    o = oracle(seg)
    assert [MSG % (k + 1) for k in range(3) if o["clip"] >> k & 1] == said == [MSG % k for k in numbers]
    assert np.array_equal(o["final"].samples, want.samples)
    assert audio.cut_sample_ranges(o["rows"], o["lead_frame"], o["kept"]) == audio.reference_sample_ranges(seg)[0]


def test_trailing_cut_is_the_loop_of_remove_silence_edges():
    seg = build_clip([("speech", 700), ("pause", 333)], 22050, 1, seed=5)
    trimmed = audio.remove_silence_edges(seg)
    assert trimmed.samples.shape[0] == seg.slice_ms(0, audio.trailing_cut_ms(seg.samples.shape[0], 22050, 333)).samples.shape[0]
    assert audio.cut_sample_ranges([(10, 20), (20, 20), (40, 50)], 5, 10) == [(15, 20), (40, 45)]


def _bare_wrapper():
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    w = F5TTSWrapper.__new__(F5TTSWrapper)
    w.device, w.target_rms, w.target_sample_rate, w.hop_length = "cpu", 0.1, 24000, 256
    w.reference_on_device, w.last_reference_route = False, None
    w.ref_audio_processed = w.ref_text = w.ref_audio_len = None
    return w


def test_wrapper_keyword_off_is_the_host_route(tmp_path, capsys):
    import inspect
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    for fn in (F5TTSWrapper.preprocess_reference, F5TTSWrapper.add_voice):
        assert inspect.signature(fn).parameters["on_device"].default is None
    seg = build_clip(REAL_CLIPS["quiet_edges"][0], 24000, 1, seed=2)
    path = os.path.join(str(tmp_path), "clip.wav")
    audio.write_wav_pcm16(path, seg.samples[:, 0], 24000)
    w = _bare_wrapper()
    got, text = w.preprocess_reference(path, "a short clip", on_device=False)
    assert w.last_reference_route == "host" and text == "a short clip. "
    trimmed = audio.remove_silence_edges(audio.clip_reference(seg))
    x = audio.segment_to_float(trimmed + trimmed.silent_like(50))
    rms = torch.sqrt(torch.mean(torch.square(x)))
    assert rms < 0.1 and torch.equal(got, x * 0.1 / rms)
    assert w.ref_audio_len == got.shape[-1] // 256
    again, _ = w.preprocess_reference(path, "a short clip")  # None: the attribute, off by default
    assert w.last_reference_route == "host" and torch.equal(again, got)
    out = capsys.readouterr().out
    assert out.count("Converting audio...") == 2 and "clipping short" not in out
    with pytest.raises(RuntimeError, match="No reference text"):
        w.preprocess_reference(path, "  ", on_device=False)
