"""`F5TTSWrapper.generate_batch`: independent requests -- each with its own voice, step count, guidance strength, speed, cross-fade and
``remove_silence`` -- through ragged sampler calls with one guidance strength per utterance, one ragged decode and one segmented wave tail per
cross-fade length.  Acceptance is exactness against calls that existed before: after one ``torch.manual_seed`` entry i is byte for byte (dtype
included) the i-th of the ``generate(..., return_numpy=True)`` calls made in order after the same seed with voice i's fields installed; a
request with ``seed`` does not depend on its neighbours.  The tiny wrapper, texts and voices are those of tests/test_gpu_multi_voice.py, at 3
function evaluations (one request at 2)."""
import os

import numpy as np
import pytest
import torch

from test_gpu_multi_voice import _installed, _tone, _voices_tts
from test_gpu_wave_tail import SENTENCE, SR, TEXTS

pytestmark = pytest.mark.gpu
NFE = 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _requests(**last):
    """every voice; guidance 2.0 (the default), 1.2 and 0.0; one request at another step count; one slower; a two-chunk text with the default
    cross-fade and one without; one with remove_silence"""
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    return [TTSJob(TEXTS[2]),
            TTSJob(SENTENCE * 2, voice="town", cfg_strength=1.2),
            TTSJob(SENTENCE, voice="deep", cfg_strength=0.0),
            TTSJob(SENTENCE * 2 + "more.", nfe_step=2),
            TTSJob(TEXTS[2], voice="town", speed=0.8, cross_fade_duration=0.0),
            TTSJob(SENTENCE + "bye now.", voice="deep", remove_silence=True, **last)]


def _tts(tmp_path, prec):
    tts = _voices_tts(tmp_path, prec)
    tts.nfe_step = NFE  # (a request's None is the wrapper's attribute, as in generate())
    return tts


def _serial(tts, reqs, seed, **kw):
    """the right-hand side of the contract: one generate() per request, in order, with that voice's fields in the main fields"""
    voices = dict(tts.voices)
    if seed is not None:
        torch.manual_seed(seed)
    outs = []
    for q in reqs:
        with _installed(tts, voices[q.voice]):
            outs.append(tts.generate(q.text, nfe_step=q.nfe_step, cfg_strength=q.cfg_strength, sway_sampling_coef=q.sway_sampling_coef, speed=q.speed,
                                     fix_duration=q.fix_duration, cross_fade_duration=q.cross_fade_duration,
                                     use_duration_predictor=q.use_duration_predictor, remove_silence=q.remove_silence, return_numpy=True, **kw))
    return outs


def _batch(tts, reqs, seed, **kw):
    if seed is not None:
        torch.manual_seed(seed)
    return tts.generate_batch(reqs, **kw)


def _same(got, want, what=""):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b) and a[1] == b[1] == SR, (what, i)
        assert a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes(), (what, i, a[0].dtype, b[0].dtype)
        if len(a) == 3:
            assert a[2].dtype == b[2].dtype and np.array_equal(a[2], b[2]), (what, i)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_generate_batch_equals_the_generate_calls_in_order(tmp_path, prec):
    tts = _tts(tmp_path, prec)
    reqs = _requests()
    want = _serial(tts, reqs, 11)
    assert [w[0].dtype for w in want] == [np.float64, np.float32, np.float32, np.float32, np.float32, np.float32]
    got = _batch(tts, reqs, 11)
    print(f"generate_batch [{prec}]: {[len(g[0]) for g in got]} samples")
    _same(got, want, "float")
    assert tts.ref_text == "a quiet tone. " and tts.ref_audio_processed is tts.voices["main"]["audio"]  # the main fields are as they were
    if prec == "fp16":
        return  # (one case in fp16)
    _same(_batch(tts, reqs, 12, return_pcm16=True), _serial(tts, reqs, 12, return_pcm16=True), "pcm16")
    assert all(g[0].dtype == np.int16 for g in _batch(tts, reqs, 12, return_pcm16=True))
    _same(_batch(tts, reqs, 13, return_spectrogram=True), _serial(tts, reqs, 13, return_spectrogram=True), "spectrogram")
    # plain dicts with the same keys
    _same(_batch(tts, [dict(text=q.text, voice=q.voice, cfg_strength=q.cfg_strength, nfe_step=q.nfe_step, speed=q.speed,
                            cross_fade_duration=q.cross_fade_duration, remove_silence=q.remove_silence) for q in reqs], 11), want, "dicts")


@pytest.mark.parametrize("noise_device", [None, "cpu"])
def test_a_seeded_request_does_not_depend_on_its_neighbours(tmp_path, noise_device):
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    tts = _tts(tmp_path, "bf16")
    tts.model.noise_device = noise_device
    plain = _requests()
    seeded = TTSJob(TEXTS[2], voice="town", cfg_strength=1.5, seed=7)
    alone = _batch(tts, [seeded], 1)[0]
    assert alone[0].dtype == np.float64 and len(alone[0]) > 0
    for name, reqs, at in (("first", [seeded] + plain, 0), ("last", plain + [seeded], len(plain)), ("between", plain[:3] + [seeded] + plain[3:], 3),
                           ("fewer neighbours", plain[1:2] + [seeded] + plain[4:5], 1)):
        got = _batch(tts, reqs, 2 + at)  # (another global seed every time: it must not reach the seeded request)
        _same([got[at]], [alone], name)
    # the unseeded requests around it equal the serial route over the unseeded requests alone
    got = _batch(tts, plain[:3] + [seeded] + plain[3:], 21)
    _same(got[:3] + got[4:], _serial(tts, plain, 21), "the others")
    # two seeded requests with the same seed and text hear the same noise
    twice = _batch(tts, [seeded, plain[1], seeded], 3)
    _same([twice[2]], [twice[0]], "same seed")


def test_the_jobs_of_one_key_share_one_ragged_call(tmp_path):
    """r0 (2 chunks), r1, r4 (2 chunks) and r5 share (nfe 3, sway -1, guided): ONE sample_ragged call with the guidance vector; the cfg = 0
    request and the request at nfe 2 are groups of one job and take sample()."""
    tts = _tts(tmp_path, "bf16")
    calls, singles = [], []
    sample, sample_ragged = tts.model.sample, tts.model.sample_ragged

    def counting_sample(*a, **kw):
        singles.append((kw["steps"], kw["cfg_strength"], kw.get("y0") is not None))
        return sample(*a, **kw)

    def counting_sample_ragged(cond, texts, durations, lens=None, **kw):
        calls.append((len(durations), kw["steps"], kw["cfg_strength"], [y is not None for y in kw["y0s"]], [int(x) for x in lens]))
        return sample_ragged(cond, texts, durations, lens=lens, **kw)

    tts.model.sample, tts.model.sample_ragged = counting_sample, counting_sample_ragged
    got = _batch(tts, _requests(), 5)
    frames = {name: int(v["mel"].shape[1]) for name, v in tts.voices.items()}
    assert len(got) == 6 and len(calls) == 1
    assert calls[0] == (6, NFE, [2.0, 2.0, 1.2, 2.0, 2.0, 2.0], [True] * 6, [frames[n] for n in ("main", "main", "town", "town", "town", "deep")])
    assert singles == [(NFE, 0.0, True), (2, 2.0, True)]
    # two requests at the odd step count: a group of two eligible jobs, one more ragged call
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    del calls[:], singles[:]
    _batch(tts, _requests() + [TTSJob(SENTENCE * 2, voice="deep", nfe_step=2, cfg_strength=3.0)], 5)
    assert [c[:3] for c in calls] == [(6, NFE, [2.0, 2.0, 1.2, 2.0, 2.0, 2.0]), (2, 2, [2.0, 3.0])] and singles == [(NFE, 0.0, True)]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_unguided_requests_keep_the_groups_of_their_own_generate_calls(tmp_path, prec):
    """cfg_strength = 0 is the reference's single pass: the batch is not doubled, so a job of 256 .. 511 frames meets the tuned kernels only
    next to other rows.  Two short unguided requests therefore take sample() each, as their generate() calls do, while the two chunks of one
    unguided request share the ragged call generate() makes for them."""
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    tts = _tts(tmp_path, prec)
    reqs = [TTSJob("hello you.", cfg_strength=0.0), TTSJob(SENTENCE * 2, voice="town"), TTSJob("hello there.", cfg_strength=0.0),
            TTSJob(TEXTS[2], voice="town", cfg_strength=0.0), TTSJob(SENTENCE * 2 + "more.")]
    want = _serial(tts, reqs, 41)
    calls, singles = [], []
    sample, sample_ragged = tts.model.sample, tts.model.sample_ragged

    def counting_sample(*a, **kw):
        singles.append((kw["duration"], kw["cfg_strength"]))
        return sample(*a, **kw)

    def counting_sample_ragged(cond, texts, durations, **kw):
        calls.append(([int(d) for d in durations], kw["cfg_strength"]))
        return sample_ragged(cond, texts, durations, **kw)

    tts.model.sample, tts.model.sample_ragged = counting_sample, counting_sample_ragged
    _same(_batch(tts, reqs, 41), want, prec)
    assert len(singles) == 2 and all(256 <= d < 512 and c == 0.0 for d, c in singles)  # (the case that needs the rule: under 512 rows alone)
    assert [c for _, c in calls] == [[2.0, 2.0], [0.0, 0.0]] and min(calls[1][0]) >= 256


def test_host_tails_keep_the_order_contract(tmp_path):
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    tts = _tts(tmp_path, "fp32")
    # a cross-fade longer than the chunks: the segmented tail answers F5_ENOTSUP for that request, which is joined on the host
    reqs = _requests() + [TTSJob(TEXTS[2], voice="deep", cross_fade_duration=30.0)]
    _same(_batch(tts, reqs, 21), _serial(tts, reqs, 21), "chained joints")
    _same(_batch(tts, reqs, 22, return_pcm16=True), _serial(tts, reqs, 22, return_pcm16=True), "chained joints, pcm16")

    class Foreign(torch.nn.Module):  # plug point B with an object the library knows nothing about
        def decode(self, mel):
            return torch.tanh(mel.mean(dim=1)).repeat_interleave(256, dim=1)[:, 256:] * 0.5

    tts.vocoder = Foreign()
    for kw in ({}, {"return_pcm16": True}, {"return_spectrogram": True}):
        _same(_batch(tts, reqs, 23, **kw), _serial(tts, reqs, 23, **kw), f"foreign vocoder {kw}")


def test_refusals_come_before_any_sampling(tmp_path):
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    tts = _tts(tmp_path, "bf16")
    sampled = []
    tts.model.sample = lambda *a, **kw: sampled.append(1)
    tts.model.sample_ragged = lambda *a, **kw: sampled.append(1)
    good = TTSJob(SENTENCE)
    with pytest.raises(ValueError, match="request 1.*ghost"):
        tts.generate_batch([good, TTSJob(SENTENCE, voice="ghost")])
    with pytest.raises(ValueError, match="no requests"):
        tts.generate_batch([])
    with pytest.raises(ValueError, match="request 2.*nfe_step"):
        tts.generate_batch([good, good, TTSJob(SENTENCE, nfe_step=0)])
    with pytest.raises(ValueError, match="request 0.*empty text"):
        tts.generate_batch([TTSJob("  "), good])
    with pytest.raises(ValueError, match="request 1.*pitch"):
        tts.generate_batch([good, dict(text=SENTENCE, pitch=2)])
    assert sampled == []


def test_a_voice_speaks_at_its_own_speed(tmp_path):
    """add_voice(speed=): generate_multi uses it for that voice's pieces when the call names no speed, generate_batch when the request names
    none; the serial reference calls generate(speed=0.8) for that voice."""
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    from eraxvif5tts_amd.infer.utils_infer import split_voice_script
    tts = _tts(tmp_path, "bf16")
    tts.add_voice("slow", _tone(os.path.join(str(tmp_path), "slow.wav"), 2.0, 0.05, 250), "a slow horn", speed=0.8)
    assert tts.voices["slow"]["speed"] == 0.8 and "speed" not in tts.voices["town"]
    script = f"[slow] {SENTENCE * 2} [town] {SENTENCE} [slow] {TEXTS[2]}"
    voices = dict(tts.voices)

    def serial(seed, **kw):
        torch.manual_seed(seed)
        outs = []
        for name, piece in split_voice_script(script, voices):
            with _installed(tts, voices[name]):
                outs.append(tts.generate(piece, return_numpy=True, **({"speed": 0.8} if name == "slow" and "speed" not in kw else {}), **kw)[0])
        return outs

    want = serial(31)
    torch.manual_seed(31)
    got = tts.generate_multi(script, return_numpy=True)[0]
    assert got.dtype == np.float64 and np.array_equal(got, np.concatenate(want))
    with _installed(tts, voices["slow"]):  # the speed is heard: the same piece at the wrapper's speed is shorter
        torch.manual_seed(31)
        assert len(tts.generate(SENTENCE * 2, return_numpy=True)[0]) < len(want[0])
    # a speed given by the call wins
    want = serial(32, speed=1.1)
    torch.manual_seed(32)
    assert np.array_equal(tts.generate_multi(script, speed=1.1, return_numpy=True)[0], np.concatenate(want))
    # generate_batch: the voice's speed where the request names none
    torch.manual_seed(33)
    got = tts.generate_batch([TTSJob(SENTENCE * 2, voice="slow"), TTSJob(SENTENCE * 2, voice="slow", speed=1.0)])
    torch.manual_seed(33)
    with _installed(tts, voices["slow"]):
        want = [tts.generate(SENTENCE * 2, speed=s, return_numpy=True) for s in (0.8, 1.0)]
    _same(got, want, "per-voice speed")
    with pytest.raises(ValueError):
        tts.add_voice("bad", os.path.join(str(tmp_path), "slow.wav"), "a slow horn", speed=0.0)
