"""The reference-voice front-end on the device (csrc/reference.hip, infer/reference.py) against the host route, exactly: the decision at op level
with small rule parameters (every branch of the clip rule on waves of a few thousand samples), `prepare_reference_device` at the real constants,
and the wrapper's ``on_device`` keyword.  The one comparison that is not exact is stated where it is made (the host's own fp32 rms)."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_reference_host import MSG, REAL_CLIPS, build_clip, oracle, repeat  # noqa: E402

from eraxvif5tts_amd.infer import audio  # noqa: E402

gpu = pytest.mark.gpu

# windows 20 / 6 ms, keep 7, step 3, limits 60 / 120 ms, leading chunk 2 ms, pad 5 ms; the thresholds are the real ones
SMALL = dict(passes=((20, -50), (6, -40)), keep=7, step=3, soft=60, hard=120, T=-42, chunk=2, pad=5)
# name -> (layout in ms, extra frames, overrides of SMALL / clip_short, expected clip bits, pass 2 entered)
SMALL_CASES = {
    "no_clipping": ([("speech", 25), ("pause", 24), ("speech", 20)], 3, {}, 0, 0),
    "clip_in_pass_1": (repeat([("speech", 30), ("pause", 26)], 160) + [("speech", 30)], 3, {}, 1, 0),
    "clip_in_pass_2": (repeat([("speech", 14), ("pause", 9)], 200), 3, {}, 2, 1),  # (its 9 ms pauses pad to overlapping parts: midpoints)
    "hard_cut": ([("speech", 150)], 3, {}, 4, 1),
    "first_part_over_the_limit": ([("speech", 130), ("pause", 26), ("speech", 30)], 3, {}, 7, 1),
    "midpoint_in_pass_1": ([("speech", 30), ("pause", 24), ("speech", 30)], 3, dict(keep=15), 0, 0),
    "all_silent": ([("pause", 70)], 0, {}, 0, 0),
    "under_both_windows": ([("speech", 4)], 3, {}, 0, 0),
    "under_the_long_window": ([("speech", 12)], 3, {}, 0, 0),
    "lead_takes_everything": ([("quiet", 50)], 0, {}, 0, 0),
    "quiet_edges": ([("quiet", 9), ("speech", 30), ("quiet", 7)], 0, {}, 0, 0),
    "not_clipped_on_request": ([("speech", 150)], 3, dict(clip_short=False), 0, 0),
}
RATES = [8000, 11025, 22050, 24000, 44100]


def _small(name, rate, channels):
    layout, extra, over, clip, pass2 = SMALL_CASES[name]
    seg = build_clip(layout, rate, channels, seed=len(name) * 7 + rate % 89 + channels, extra=extra)
    return seg, {**SMALL, **over}, clip, pass2


def _check_branch(name, o, seg):
    """the case reaches what it is named for"""
    rows = o["rows"]
    if name == "clip_in_pass_2":
        assert any(b == c for (_, b), (c, _) in zip(rows, rows[1:]))  # neighbours that met at a midpoint
    if name == "midpoint_in_pass_1":
        assert len(rows) == 2 and rows[0][1] == rows[1][0]
    if name == "first_part_over_the_limit":
        assert len(rows) == 1 and o["gathered_ms"] == 120
    if name == "all_silent":
        assert rows == [] and o["gathered"] == 0 and o["kept"] == 0
    if name.startswith("under"):
        assert len(seg) < 20 and rows == [(0, min(seg._frame(len(seg)), seg.samples.shape[0]))]
    if name == "lead_takes_everything":
        assert o["gathered"] > 0 and o["lead_ms"] == o["gathered_ms"] and o["kept"] == 0
    if name == "quiet_edges":
        assert o["lead_ms"] >= 8 and o["trail_ms"] >= 6 and o["kept"] > 0
    if name == "not_clipped_on_request":
        assert o["gathered"] == seg.samples.shape[0] and o["gathered_ms"] > 120


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_small_cases_reach_their_branches(name, rate, channels):
    seg, kw, clip, pass2 = _small(name, rate, channels)
    o = oracle(seg, **kw)
    assert (o["clip"], o["pass2"]) == (clip, pass2)
    _check_branch(name, o, seg)


def _rule(kw, target_rms=0.1):
    from eraxvif5tts_amd.infer import reference
    return reference.make_rule(kw.get("clip_short", True), target_rms, passes=kw["passes"], keep_silence=kw["keep"], seek_step=kw["step"],
                               soft_limit_ms=kw["soft"], hard_limit_ms=kw["hard"], silence_threshold=kw["T"], lead_chunk_ms=kw["chunk"],
                               pad_ms=kw["pad"])


def _upload(seg):
    return torch.from_numpy(np.ascontiguousarray(seg.samples, dtype=np.int16)).cuda()


def _mono_float(padded):
    """the host route's wave before the boost: int / 32768 in fp32, the mean over channels"""
    x = audio.segment_to_float(padded)
    return torch.mean(x, dim=0, keepdim=True) if x.shape[0] > 1 else x


def _exact_rms32(padded):
    """(S, rms32): the int64 sum of the squared channel sums and float32(sqrt(S / (ch^2 32768^2 n))), fp64 inside"""
    s = padded.samples.astype(np.int64).sum(axis=1)
    S, (n, ch) = int(np.sum(s * s)), padded.samples.shape
    return S, np.float32(np.sqrt(np.float64(S) / np.float64(ch * ch * 32768.0 * 32768.0 * n)))


@gpu
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_plan_and_kept_integers_equal_the_host_rule(name, rate, channels):
    from eraxvif5tts_amd.infer import reference
    seg, kw, clip, pass2 = _small(name, rate, channels)
    o = oracle(seg, **kw)
    assert (o["clip"], o["pass2"]) == (clip, pass2)
    _check_branch(name, o, seg)
    pcm, rule = _upload(seg), _rule(kw)
    rec, table = reference.reference_plan(pcm, rate, rule)
    assert [(int(a), int(b)) for a, b, _ in table if b > a] == o["rows"]
    pos = 0
    for a, b, p in table:  # the third column: where the part starts among the gathered frames
        assert p == pos or b == a
        pos += b - a
    for key in ("clip", "pass2", "gathered", "gathered_ms", "lead_ms", "trail_ms", "lead_frame", "edge_frames", "edge_ms"):
        assert rec[key] == o[key], (key, rec[key], o[key])
    # the whole call in one go (planned = 0), the cut given as the host forms it from the counts
    call = reference._Call(pcm, rate, rule)
    cut_ms = audio.trailing_cut_ms(rec["edge_frames"], rate, rec["trail_ms"])
    assert cut_ms == o["cut_ms"]
    kept, total = call.out_frames(rec, cut_ms)
    padded = o["padded"]
    assert (kept, total) == (o["kept"], padded.samples.shape[0])
    wave, ints = call.prepare(cut_ms, total, planned=False, want_pcm=True)
    late, _ = call.read()
    assert late["kept"] == kept and late["out_frames"] == total
    assert np.array_equal(ints.cpu().numpy(), padded.samples.astype(np.int16))
    S, rms32 = _exact_rms32(padded)
    x = _mono_float(padded).reshape(-1)
    if total:
        assert late["sumsq"] == S and late["rms_bits"] == int(rms32.view(np.uint32))
        assert late["boost"] == int(rms32 < np.float32(0.1))
        want = (x * torch.tensor(0.1, dtype=torch.float32)) / torch.tensor(rms32) if late["boost"] else x
        if S == 0:  # nothing but the pad: rms 0, and the boost is 0 * target / 0 on both routes
            assert late["boost"] == 1 and bool(torch.isnan(want).all()) and bool(torch.isnan(wave).all())
        else:
            assert torch.equal(wave.cpu(), want)
    else:
        assert late["boost"] == 0 and wave.numel() == 0


@gpu
def test_refusals_come_before_any_launch():
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.infer import reference
    seg = build_clip([("speech", 40)], 8000, 1)
    pcm = _upload(seg)
    for bad in (dict(step=0), dict(keep=-1), dict(chunk=0), dict(pad=-1), dict(soft=200), dict(passes=((0, -50), (6, -40)))):
        with pytest.raises(_lib.F5HipError, match="code -1"):
            reference._Call(pcm, 8000, _rule({**SMALL, **bad}))
    with pytest.raises(_lib.F5HipError, match="sample_rate"):
        reference._Call(pcm, 999, _rule(SMALL))
    three = torch.zeros(16, 3, dtype=torch.int16, device="cuda")
    with pytest.raises(_lib.F5HipError, match="channels"):
        reference._Call(three, 8000, _rule(SMALL))
    call = reference._Call(pcm, 8000, _rule(SMALL))
    call.ws = call.ws[:-16]
    with pytest.raises(_lib.F5HipError, match="workspace"):
        call.plan()


# ----------------------------------------------------------------------------- the real constants
# (kind, rate, channels, rms of the speech): one clip louder than the target (never boosted), the others quieter
REAL_CASES = [("short", 8000, 1, 6500.0), ("long_pauses", 8000, 1, 3000.0), ("short_pauses", 8000, 1, 3000.0), ("no_pause", 8000, 1, 3000.0),
              ("short_pauses", 44100, 2, 3000.0)]


def _host_voice(seg, target_rms=0.1, clip_short=True):
    """F5TTSWrapper._preprocess_voice's host steps: (padded segment, wave before the boost, wave, messages)"""
    said = []
    aseg = audio.clip_reference(seg, said.append) if clip_short else seg
    aseg = audio.remove_silence_edges(aseg)
    aseg = aseg + aseg.silent_like(50)
    x = _mono_float(aseg)
    rms = torch.sqrt(torch.mean(torch.square(x)))
    return aseg, x, (x * target_rms / rms if rms < target_rms else x), said


@gpu
@pytest.mark.parametrize("kind,rate,channels,loud", REAL_CASES)
def test_prepare_reference_device_equals_the_host_route(kind, rate, channels, loud):
    from eraxvif5tts_amd.infer.reference import prepare_reference_device
    layout, numbers = REAL_CLIPS[kind]
    seg = build_clip(layout, rate, channels, seed=41, extra=5, loud=loud)
    assert seg.duration_seconds <= 15.0 or rate == 8000
    aseg, x, boosted, said = _host_voice(seg)
    assert said == [MSG % k for k in numbers]
    shown = []
    wave, sr, rec = prepare_reference_device(seg, True, 0.1, shown.append, want_pcm=True)
    assert sr == rate and shown == said == rec["messages"]
    assert rec["ranges"] == audio.reference_sample_ranges(seg)[0]
    # the integers before the float conversion, byte for byte
    assert rec["pcm"].dtype == torch.int16 and np.array_equal(rec["pcm"].cpu().numpy(), aseg.samples.astype(np.int16))
    # the fp32 mono wave before the boost, byte for byte
    plain, _, rec0 = prepare_reference_device(seg, True, 0.1, lambda m: None, unboosted=True)
    assert rec0["boost"] == 0 and plain.shape == x.shape and torch.equal(plain.cpu(), x)
    # the boost: the exact rms, the decision, and the two fp32 operations
    S, rms32 = _exact_rms32(aseg)
    target = np.float32(0.1)
    assert abs(float(rms32) / float(target) - 1.0) > 1e-5  # (a clip whose decision no rounding can turn)
    assert rec["sumsq"] == S and rec["rms32"].view(np.uint32) == rms32.view(np.uint32)
    assert rec["boost"] == int(rms32 < target) == int(loud < 5000.0)
    want = (x * torch.tensor(target)) / torch.tensor(rms32) if rec["boost"] else x
    assert wave.dtype == torch.float32 and wave.shape == want.shape and torch.equal(wave.cpu(), want)
    # the host route's own wave: its rms is torch's fp32 reduction (a sanity bound, two orders above what was observed)
    torch.testing.assert_close(wave.cpu(), boosted, rtol=1e-5, atol=0)


@gpu
def test_prepare_reference_device_without_clipping_and_from_a_path(tmp_path):
    from eraxvif5tts_amd.infer.reference import prepare_reference_device
    seg = build_clip(REAL_CLIPS["no_pause"][0], 8000, 1, seed=9, extra=1)
    path = os.path.join(str(tmp_path), "clip.wav")
    audio.write_wav_pcm16(path, seg.samples[:, 0], 8000)
    aseg, x, boosted, said = _host_voice(seg, clip_short=False)
    wave, sr, rec = prepare_reference_device(path, False, 0.1, said.append, want_pcm=True)
    assert said == [] and rec["clip"] == 0 and len(aseg) > 12000
    assert np.array_equal(rec["pcm"].cpu().numpy(), aseg.samples.astype(np.int16))
    torch.testing.assert_close(wave.cpu(), boosted, rtol=1e-5, atol=0)
    with pytest.raises(ValueError, match="device route"):
        prepare_reference_device(audio.Segment(seg.samples, 8000, 3))


# ----------------------------------------------------------------------------- the wrapper
def _write_pcm_wav(path, samples, rate, width):
    """[n, ch] integers -> a PCM WAV of `width` bytes per sample"""
    n, ch = samples.shape
    if width == 2:
        body = samples.astype("<i2").tobytes()
    else:
        body = b"".join(int(v).to_bytes(width, "little", signed=True) for v in samples.reshape(-1))
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * ch * width, ch * width, 8 * width))
        f.write(b"data" + struct.pack("<I", len(body)) + body)
    return path


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    from test_gpu_wave_tail import _tts
    return _tts(tmp_path_factory.mktemp("reference"), "fp32")


@gpu
def test_wrapper_takes_the_device_route_on_request(tts, tmp_path, capsys):
    from eraxvif5tts_amd.infer.reference import prepare_reference_device
    assert tts.reference_on_device is False and tts.last_reference_route == "host"  # (the fixture's own voice went the host's way)
    seg = build_clip(REAL_CLIPS["long_pauses"][0], 8000, 2, seed=17, extra=5)  # clips with message (1); 8 kHz: through the resampler
    path = _write_pcm_wav(os.path.join(str(tmp_path), "voice.wav"), seg.samples, 8000, 2)
    capsys.readouterr()
    host_audio, host_text = tts.preprocess_reference(path, "two long pauses", on_device=False)
    host_len, host_out = tts.ref_audio_len, capsys.readouterr().out
    assert tts.last_reference_route == "host" and MSG % 1 in host_out

    item, sr, _ = prepare_reference_device(path, True, tts.target_rms, lambda m: None)
    item = audio.resample(item, sr, 24000)
    dev_audio, dev_text = tts.preprocess_reference(path, "two long pauses", on_device=True)
    assert tts.last_reference_route == "device" and capsys.readouterr().out == host_out  # the same prints in the same order
    assert dev_audio.is_cuda and torch.equal(dev_audio, item) and tts.ref_audio_processed is dev_audio
    assert dev_text == host_text == tts.ref_text and tts.ref_audio_len == host_len and dev_audio.shape == host_audio.shape

    town, town_text = tts.add_voice("town", path, "two long pauses", on_device=True)
    try:
        assert tts.last_reference_route == "device" and torch.equal(town, item) and town_text == host_text
        assert tts.voices["town"]["ref_audio_len"] == host_len and torch.equal(tts.voices["town"]["audio"], item)
    finally:
        tts.remove_voice("town")
    tts.reference_on_device = True  # the attribute is what None means
    try:
        again, _ = tts.preprocess_reference(path, "two long pauses")
        assert tts.last_reference_route == "device" and torch.equal(again, item)
        with pytest.raises(RuntimeError, match="No reference text"):
            tts.preprocess_reference(path, " ")
    finally:
        tts.reference_on_device = False


@gpu
@pytest.mark.parametrize("width,channels", [(3, 1), (2, 3)])
def test_wrapper_sends_other_formats_the_host_way(tts, tmp_path, width, channels):
    seg = build_clip([("quiet", 120), ("speech", 900), ("pause", 200)], 24000, channels, seed=23)
    samples = seg.samples * (256 if width == 3 else 1)
    path = _write_pcm_wav(os.path.join(str(tmp_path), "other.wav"), samples, 24000, width)
    host_audio, _ = tts.preprocess_reference(path, "another format", on_device=False)
    assert tts.last_reference_route == "host"
    dev_audio, _ = tts.preprocess_reference(path, "another format", on_device=True)
    assert tts.last_reference_route == "host" and torch.equal(dev_audio, host_audio)
