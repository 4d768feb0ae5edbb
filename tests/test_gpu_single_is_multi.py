"""A single-voice call is a multi-voice call with one voice and one segment: for a text without tags `generate_multi` returns what `generate`
returns and `generate_multi_stream` yields what `generate_stream` yields -- dtype, shape and bytes, for every return form, after the same
``torch.manual_seed`` (attention dropout off).  The tiny wrapper, its three voices and the texts are those of tests/test_gpu_multi_voice.py, at
3 function evaluations; the gain applies (target_rms 0.2 above the main prompt's rms)."""
import os

import numpy as np
import pytest
import torch

from test_gpu_multi_voice import NFE, _voices_tts
from test_gpu_wave_tail import SENTENCE, SR, TEXTS

pytestmark = pytest.mark.gpu
# name -> (text, speed, frames asked for per chunk are all >= 256): one short chunk (a batch-1 sample() call), two chunks of which the second
# is short (two sample() calls on two chunk streams), and two long chunks (one ragged call)
CASES = {"one_short_chunk": ("hello there.", 5.0, [False]),
         "long_then_short": (SENTENCE * 4 + "and a little bit more.", 5.0, [True, False]),
         "two_chunks": (TEXTS[2], None, [True, True])}
FORMS = [{}, {"return_pcm16": True}, {"cross_fade_duration": 0.0}, {"cross_fade_duration": 30.0}, {"remove_silence": True}]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def tts(request, tmp_path_factory):
    return _voices_tts(tmp_path_factory.mktemp("single_is_multi"), request.param)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("case", list(CASES))
def test_generate_multi_of_an_untagged_text_is_generate(tts, tmp_path, case):
    from eraxvif5tts_amd.infer.utils_infer import chunk_text
    text, speed, long_enough = CASES[case]
    secs = tts.ref_audio_processed.shape[-1] / SR
    chunks = chunk_text(text, max_chars=int(len(tts.ref_text.encode("utf-8")) / secs * (22 - secs)))
    rate = speed if speed is not None else tts.speed
    assert min(len(c.encode("utf-8")) for c in chunks) >= 10  # (below that the duration rule takes 0.3 for the speed)
    asked = [tts.ref_audio_len + int(tts.ref_audio_len / len(tts.ref_text.encode("utf-8")) * len(c.encode("utf-8")) / rate) for c in chunks]
    assert [d >= 256 for d in asked] == long_enough, asked  # (the case is the one its name says)
    kw = dict(nfe_step=NFE, speed=speed)
    for seed, form in enumerate(FORMS):
        torch.manual_seed(60 + seed)
        want, want_rate = tts.generate(text, return_numpy=True, **kw, **form)
        torch.manual_seed(60 + seed)
        got, got_rate = tts.generate_multi(text, return_numpy=True, **kw, **form)
        assert got_rate == want_rate == SR and len(want) > 0
        _same(got, want, (case, form))
    # the written file, the returned path, and the three-part return
    one, other = str(tmp_path / "a" / "generate.wav"), str(tmp_path / "b" / "multi.wav")
    torch.manual_seed(70)
    assert tts.generate(text, one, **kw) == one
    torch.manual_seed(70)
    assert tts.generate_multi(text, other, **kw) == other
    assert _bytes(one) == _bytes(other) and len(_bytes(one)) > 44
    torch.manual_seed(71)
    want = tts.generate(text, one, return_numpy=True, return_spectrogram=True, **kw)
    torch.manual_seed(71)
    got = tts.generate_multi(text, other, return_numpy=True, return_spectrogram=True, **kw)
    _same(got[0], want[0], case)
    _same(got[2], want[2], case)
    assert _bytes(one) == _bytes(other) and _bytes(os.path.splitext(one)[0] + "_spec.npy") == _bytes(os.path.splitext(other)[0] + "_spec.npy")


@pytest.mark.parametrize("form", [{}, {"return_pcm16": True}], ids=["float", "pcm16"])
def test_generate_multi_stream_of_an_untagged_text_is_generate_stream(tts, form):
    text = TEXTS[4]
    try:
        for seed, (group_max, pieces_expected) in enumerate([(8, 2), (2, 3)]):  # 1 | 3 chunks, and 1 | 2 | 1
            tts.ragged_chunks = group_max
            torch.manual_seed(80 + seed)
            want = list(tts.generate_stream(text, nfe_step=NFE, **form))
            torch.manual_seed(80 + seed)
            got = list(tts.generate_multi_stream(text, nfe_step=NFE, **form))
            assert len(got) == len(want) == pieces_expected
            for (a, ra), (b, rb) in zip(got, want):
                assert ra == rb == SR and len(b) > 0
                _same(a, b, (form, group_max))
    finally:
        tts.ragged_chunks = 8
