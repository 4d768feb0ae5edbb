"""`F5TTSWrapper.generate_multi` / `generate_multi_stream` / `add_voice`: one script in several voices through ONE ragged batch and one
segmented wave tail.  Acceptance is exactness, the oracle the serial route composed from calls that existed before: after one
``torch.manual_seed`` and with attention dropout off, ``generate_multi(script)`` is byte for byte
``np.concatenate([generate(piece) with that voice's fields installed for voice, piece in split_voice_script(script, voices)])`` -- float
(dtype included), ``return_pcm16``, the written file -- and `remove_silence` of that concatenation with ``remove_silence=True``.  The tiny
wrapper and texts are those of tests/test_gpu_wave_tail.py, at 3 function evaluations."""
import contextlib
import os

import numpy as np
import pytest
import torch

from test_gpu_wave_tail import SR, TEXTS, _todays_loop, _tts

pytestmark = pytest.mark.gpu
NFE = 3
# three voices, five pieces; the two long pieces make two chunks each, and the short lines have fewer frames than the long prompt of "deep"
SCRIPT = f"yo. [town] {TEXTS[2]} [deep] ok. [main] {TEXTS[2]} [town] bye."
SEGMENTS = [1, 2, 1, 2, 1]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _tone(path, seconds, amp, freq):
    from eraxvif5tts_amd.infer import audio
    t = np.arange(int(seconds * SR)) / SR
    audio.write_wav(path, amp * np.sin(2 * np.pi * freq * t + 0.3) * (1 + 0.3 * np.sin(2 * np.pi * 3 * t)), SR)
    return path


def _voices_tts(tmp_path, prec):
    """main: the 2 s prompt of `_tts`, boosted to rms 0.1; "town": about as long, boosted to 0.1 as well; "deep": more than twice as long and
    loud (rms about 0.3, never boosted).  With target_rms = 0.2 afterwards main and town take the gain and deep does not."""
    tts = _tts(tmp_path, prec)
    tts.add_voice("town", _tone(os.path.join(str(tmp_path), "town.wav"), 2.0, 0.05, 310), "a quiet horn")  # (main's length and byte budget)
    tts.add_voice("deep", _tone(os.path.join(str(tmp_path), "deep.wav"), 4.6, 0.45, 120), "a deep and rather long tone")
    tts.target_rms = 0.2
    v = tts.voices
    assert list(v) == ["main", "town", "deep"] and v["deep"]["ref_audio_len"] >= 2 * v["main"]["ref_audio_len"]
    assert float(v["main"]["rms"]) < 0.2 and float(v["town"]["rms"]) < 0.2 < float(v["deep"]["rms"])
    return tts


@contextlib.contextmanager
def _installed(tts, voice):
    kept = tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len
    tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len = voice["audio"], voice["ref_text"], voice["ref_audio_len"]
    try:
        yield
    finally:
        tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len = kept


def _serial(tts, script, seed, **kw):
    """the right-hand side of the contract: one generate() per piece with that voice's fields in the main fields, noise drawn call after call"""
    from eraxvif5tts_amd.infer.utils_infer import split_voice_script
    voices = dict(tts.voices)
    torch.manual_seed(seed)
    outs = []
    for name, piece in split_voice_script(script, voices):
        with _installed(tts, voices[name]):
            outs.append(tts.generate(piece, nfe_step=NFE, return_numpy=True, **kw)[0])
    return np.concatenate(outs), outs


def _multi(tts, script, seed, **kw):
    torch.manual_seed(seed)
    return tts.generate_multi(script, nfe_step=NFE, return_numpy=True, **kw)[0]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_generate_multi_equals_the_serial_route(tmp_path, prec):
    from eraxvif5tts_amd.infer import audio
    from eraxvif5tts_amd.infer.utils_infer import remove_silence
    tts = _voices_tts(tmp_path, prec)
    want, parts = _serial(tts, SCRIPT, 11)
    print(f"generate_multi [{prec}]: {len(want)} samples in {len(parts)} pieces, max |x| = {np.abs(want).max():.3f}")
    assert len(parts) == 5 and [p.dtype for p in parts] == [np.float64 if g == 2 else np.float32 for g in SEGMENTS] and want.dtype == np.float64
    got = _multi(tts, SCRIPT, 11)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    # int16: every piece's own PCM (the fp32 product for a piece of one chunk, the fp64 product behind a cross-fade)
    want_pcm, _ = _serial(tts, SCRIPT, 12, return_pcm16=True)
    got_pcm = _multi(tts, SCRIPT, 12, return_pcm16=True)
    assert got_pcm.dtype == want_pcm.dtype == np.int16 and got_pcm.tobytes() == want_pcm.tobytes()
    # cross-fade off: float32 throughout
    want32, _ = _serial(tts, SCRIPT, 13, cross_fade_duration=0.0)
    torch.manual_seed(13)
    got32, _, spec = tts.generate_multi(SCRIPT, nfe_step=NFE, cross_fade_duration=0.0, return_numpy=True, return_spectrogram=True)
    assert got32.dtype == want32.dtype == np.float32 and np.array_equal(got32, want32)
    assert spec.shape == (100, len(want32) // 256 + sum(SEGMENTS))
    # remove_silence applies to the whole result
    plain, _ = _serial(tts, SCRIPT, 14)
    kept = remove_silence(plain, SR)
    got_kept = _multi(tts, SCRIPT, 14, remove_silence=True)
    assert got_kept.dtype == kept.dtype and np.array_equal(got_kept, kept)
    # the written file
    torch.manual_seed(11)
    path = tts.generate_multi(SCRIPT, os.path.join(str(tmp_path), "out", "multi.wav"), nfe_step=NFE)
    ref_path = os.path.join(str(tmp_path), "serial.wav")
    audio.write_wav(ref_path, want, SR)
    with open(path, "rb") as a, open(ref_path, "rb") as b:
        assert a.read() == b.read()
    # the main fields are as they were
    assert tts.ref_text == "a quiet tone. " and tts.ref_audio_processed is tts.voices["main"]["audio"]


def test_one_ragged_call_carries_several_voices(tmp_path):
    """All 7 utterances go to ONE sample_ragged call with a prompt each; an utterance of a short-prompt voice has fewer frames than the long
    prompt the batch is padded to (the pad of its condition rows is negative and must only cut its own zero rows)."""
    tts = _voices_tts(tmp_path, "bf16")
    calls, singles = [], []
    sample, sample_ragged = tts.model.sample, tts.model.sample_ragged

    def counting_sample(*a, **kw):
        singles.append(1)
        return sample(*a, **kw)

    def counting_sample_ragged(cond, texts, durations, lens=None, **kw):
        calls.append((tuple(cond.shape), [int(x) for x in lens], [int(d) for d in durations], [float(c.abs().sum()) for c in cond]))
        return sample_ragged(cond, texts, durations, lens=lens, **kw)

    tts.model.sample, tts.model.sample_ragged = counting_sample, counting_sample_ragged
    _multi(tts, SCRIPT, 3)
    assert singles == [] and len(calls) == 1
    shape, lens, durations, prompts = calls[0]
    frames = {name: int(v["mel"].shape[1]) for name, v in tts.voices.items()}
    assert shape == (7, frames["deep"], 100) and lens == [frames[n] for n in ("main", "town", "town", "deep", "main", "main", "town")]
    assert len(set(prompts)) == 3 and len(set(lens)) == 2 and min(durations) >= 256  # three prompts (main and town are equally long)
    assert min(durations) < frames["deep"]  # the pitfall: fewer frames than the padded prompt


def test_host_tails_keep_the_contract(tmp_path):
    tts = _voices_tts(tmp_path, "fp32")
    # a cross-fade longer than the chunks: the segmented tail answers F5_ENOTSUP, the decoded waves are joined on the host
    want, _ = _serial(tts, SCRIPT, 21, cross_fade_duration=30.0)
    got = _multi(tts, SCRIPT, 21, cross_fade_duration=30.0)
    assert got.dtype == want.dtype and np.array_equal(got, want)

    class Foreign(torch.nn.Module):  # plug point B with an object the library knows nothing about
        def decode(self, mel):
            return torch.tanh(mel.mean(dim=1)).repeat_interleave(256, dim=1)[:, 256:] * 0.5

    tts.vocoder = Foreign()
    for kw in ({}, {"return_pcm16": True}, {"remove_silence": True, "cross_fade_duration": 0.0}):
        want, _ = _serial(tts, SCRIPT, 22, **{k: v for k, v in kw.items() if k != "remove_silence"})
        if "remove_silence" in kw:
            from eraxvif5tts_amd.infer.utils_infer import remove_silence
            want = remove_silence(want, SR)
        got = _multi(tts, SCRIPT, 22, **kw)
        assert got.dtype == want.dtype and np.array_equal(got, want), kw


@pytest.mark.parametrize("kw", [{}, {"return_pcm16": True}, {"cross_fade_duration": 0.0}], ids=["float", "pcm16", "xfade_off"])
def test_generate_multi_stream_concatenates_to_generate_multi(tmp_path, kw):
    tts = _voices_tts(tmp_path, "bf16")
    want = _multi(tts, SCRIPT, 31, **kw)
    torch.manual_seed(31)
    pieces = [p for p, rate in tts.generate_multi_stream(SCRIPT, nfe_step=NFE, **kw) if rate == SR]
    assert len(pieces) == 2 and all(p.dtype == want.dtype for p in pieces)  # the first utterance, then the other six as one group
    assert np.array_equal(np.concatenate(pieces), want)
    tts.ragged_chunks = 2  # groups of [1], [2], [2], [2]: pushes that end a piece, begin one, and cut one in two
    want = _multi(tts, SCRIPT, 32, **kw)
    torch.manual_seed(32)
    pieces = [p for p, _ in tts.generate_multi_stream(SCRIPT, nfe_step=NFE, **kw)]
    assert len(pieces) == 4 and np.array_equal(np.concatenate(pieces), want)


def test_the_first_piece_of_a_multi_stream_needs_one_utterance(tmp_path):
    tts = _voices_tts(tmp_path, "bf16")
    sampled = []
    sample, sample_ragged = tts.model.sample, tts.model.sample_ragged

    def counting_sample(*a, **kw):
        sampled.append(1)
        return sample(*a, **kw)

    def counting_sample_ragged(cond, texts, durations, **kw):
        sampled.append(len(durations))
        return sample_ragged(cond, texts, durations, **kw)

    tts.model.sample, tts.model.sample_ragged = counting_sample, counting_sample_ragged
    torch.manual_seed(3)
    stream = tts.generate_multi_stream(SCRIPT, nfe_step=NFE, return_pcm16=True)
    assert sampled == []  # a generator: nothing runs before the first next()
    first, _ = next(stream)
    assert sampled == [1] and len(first) > 0
    rest = [p for p, _ in stream]
    assert sampled == [1, 6] and len(rest) == 1
    # the streamed tail does not apply (the joints chain): exactly one piece, generate_multi()'s result
    want = _multi(tts, SCRIPT, 4, cross_fade_duration=30.0)
    torch.manual_seed(4)
    pieces = [p for p, _ in tts.generate_multi_stream(SCRIPT, nfe_step=NFE, cross_fade_duration=30.0)]
    assert len(pieces) == 1 and np.array_equal(pieces[0], want)


def test_voice_names_tags_and_empty_scripts(tmp_path):
    tts = _voices_tts(tmp_path, "bf16")
    tone = os.path.join(str(tmp_path), "town.wav")
    for bad in ("main", "a-b", "", "two words"):
        with pytest.raises(ValueError):
            tts.add_voice(bad, tone, "some text")
    assert list(tts.voices) == ["main", "town", "deep"]
    with pytest.raises(TypeError):
        tts.voices["more"] = {}  # a read-only view
    # an unknown tag falls back to main
    a = _multi(tts, "[ghost] yo there, friend. [town] bye.", 41)
    b = _multi(tts, "[main] yo there, friend. [town] bye.", 41)
    c = _multi(tts, "[town] yo there, friend. [town] bye.", 41)
    assert np.array_equal(a, b) and not (a.shape == c.shape and np.array_equal(a, c))
    want, _ = _serial(tts, "[ghost] yo there, friend. [town] bye.", 41)
    assert a.dtype == want.dtype == np.float32 and np.array_equal(a, want)
    for empty in ("[town] [deep]", "   ", "[town]"):
        with pytest.raises(RuntimeError, match="No audio generated"):
            tts.generate_multi(empty, nfe_step=NFE)
    tts.remove_voice("town")
    assert list(tts.voices) == ["main", "deep"]
    with pytest.raises(ValueError):
        tts.remove_voice("main")
    fresh = type(tts).__new__(type(tts))  # no reference voice at all
    fresh.ref_audio_processed = fresh.ref_text = fresh.ref_audio_len = None
    fresh._voices = {}
    assert dict(fresh.voices) == {}
    with pytest.raises(ValueError):
        fresh.generate_multi("hello.")


def test_the_single_voice_entry_points_are_as_they_were(tmp_path):
    """preprocess_reference() stores what its steps, restated here, give; generate() and generate_stream() with further voices stored are the
    per-utterance loop of tests/test_gpu_wave_tail.py"""
    from eraxvif5tts_amd.infer import audio
    tts = _voices_tts(tmp_path, "fp32")
    aseg = audio.Segment.from_file(os.path.join(str(tmp_path), "ref.wav"))
    aseg = audio.remove_silence_edges(audio.clip_reference(aseg), -42)
    aseg = aseg + aseg.silent_like(50)
    wave = audio.segment_to_float(aseg)
    rms = torch.sqrt(torch.mean(torch.square(wave)))
    assert rms < 0.1
    wave = (wave * 0.1 / rms).to("cuda")
    assert torch.equal(tts.ref_audio_processed, wave) and tts.ref_text == "a quiet tone. " and tts.ref_audio_len == wave.shape[-1] // 256
    tts.target_rms = 0.1  # (the prompt is boosted to the target of the moment)
    got_audio, got_text = tts.preprocess_reference(os.path.join(str(tmp_path), "ref.wav"), "a quiet tone.", clip_short=True)
    tts.target_rms = 0.2
    assert torch.equal(got_audio, wave) and got_text == "a quiet tone. " and tts.ref_audio_processed is got_audio
    assert torch.equal(tts.voices["main"]["audio"], wave) and list(tts.voices) == ["main", "town", "deep"]
    want, n = _todays_loop(tts, TEXTS[2], NFE, tts.cross_fade_duration, seed=51)
    torch.manual_seed(51)
    got, _ = tts.generate(TEXTS[2], nfe_step=NFE, return_numpy=True)
    assert n == 2 and got.dtype == want.dtype and np.array_equal(got, want)
    torch.manual_seed(51)
    pieces = [p for p, _ in tts.generate_stream(TEXTS[2], nfe_step=NFE)]
    assert len(pieces) == 2 and np.array_equal(np.concatenate(pieces), want)
    # one voice, no tags: generate_multi() is generate()
    torch.manual_seed(51)
    assert np.array_equal(tts.generate_multi(TEXTS[2], nfe_step=NFE, return_numpy=True)[0], want)
