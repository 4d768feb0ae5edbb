"""`F5TTSWrapper.generate_stream()` on the tiny wrapper of tests/test_gpu_wave_tail.py (2 blocks, 128 wide, NFE 3): the pieces, concatenated, are
byte for byte what `generate()` returns after the same seed; the first piece needs the first chunk only; the cases the streamed tail does not
take yield once, with `generate()`'s result; an abandoned generator leaves the wrapper as it was; `stream_audio(stream_groups=True)` sends the
same bytes in more blocks."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from test_gpu_vocoder_wrapper import BIGVGAN_TINY
from test_gpu_wave_tail import SR, TEXTS, _tts

pytestmark = pytest.mark.gpu
NFE = 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _pieces(tts, text, seed, **kw):
    torch.manual_seed(seed)
    out = list(tts.generate_stream(text, nfe_step=NFE, **kw))
    assert all(rate == SR for _, rate in out)
    return [p for p, _ in out]


def _whole(tts, text, seed, **kw):
    torch.manual_seed(seed)
    return tts.generate(text, nfe_step=NFE, return_numpy=True, **kw)[0]


def _chunk_samples(tts, text):
    """sample counts of the chunks' waves, from the host rule alone (Vocos: (T - 1) * hop)"""
    _, jobs, voices, _ = tts._plan_jobs(text)
    return [(t - 1) * tts.hop_length for t in tts._generated_frames(jobs, voices)]


@pytest.mark.parametrize("nchunks", [2, 4])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_pieces_concatenate_to_generate_byte_for_byte(tmp_path, prec, nchunks):
    tts = _tts(tmp_path, prec)
    tts.target_rms = 0.2  # above the prompt's rms: the gain applies
    text = TEXTS[nchunks]
    pcm = _whole(tts, text, 77, return_pcm16=True)
    pieces = _pieces(tts, text, 77, return_pcm16=True)
    assert len(pieces) == 2 and all(p.dtype == np.int16 for p in pieces)
    assert b"".join(p.tobytes() for p in pieces) == pcm.tobytes()
    wave = _whole(tts, text, 78)
    pieces = _pieces(tts, text, 78)
    assert wave.dtype == np.float64 and np.abs(wave).max() < 1 and all(p.dtype == wave.dtype for p in pieces)
    assert np.array_equal(np.concatenate(pieces), wave)
    wave32 = _whole(tts, text, 79, cross_fade_duration=0.0)
    pieces = _pieces(tts, text, 79, cross_fade_duration=0.0)
    assert wave32.dtype == np.float32 and all(p.dtype == np.float32 for p in pieces) and np.array_equal(np.concatenate(pieces), wave32)


def test_group_counts_and_sizes(tmp_path):
    from eraxvif5tts_amd.infer.utils_infer import plan_wave_tail
    tts = _tts(tmp_path, "fp32")
    for nchunks in (2, 4):
        samples = _chunk_samples(tts, TEXTS[nchunks])
        assert len(samples) == nchunks
        plan = plan_wave_tail(samples, tts.cross_fade_duration, SR)
        assert plan["device_ok"]
        pieces = _pieces(tts, TEXTS[nchunks], 5, return_pcm16=True)
        assert len(pieces) == 2 and len(pieces[0]) == plan["out_offsets"][1] and sum(len(p) for p in pieces) == plan["total"]
    whole = _whole(tts, TEXTS[4], 6, return_pcm16=True)
    tts.ragged_chunks = 2
    pieces = _pieces(tts, TEXTS[4], 6, return_pcm16=True)  # 1 | 2 | 1
    assert [len(p) for p in pieces] == [plan["out_offsets"][1], plan["out_offsets"][3] - plan["out_offsets"][1], plan["total"] - plan["out_offsets"][3]]
    assert np.array_equal(np.concatenate(pieces), _whole(tts, TEXTS[4], 6, return_pcm16=True))
    tts.ragged_chunks = 8
    tts.stream_first_chunks = 4
    pieces = _pieces(tts, TEXTS[4], 6, return_pcm16=True)
    assert len(pieces) == 1 and np.array_equal(pieces[0], whole)


def test_the_first_piece_needs_the_first_chunk_only(tmp_path):
    tts = _tts(tmp_path, "bf16")
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
    stream = tts.generate_stream(TEXTS[4], nfe_step=NFE, return_pcm16=True)
    assert sampled == []  # a generator: nothing runs before the first next()
    first, _ = next(stream)
    assert sum(sampled) == 1 and len(first) > 0
    rest = [p for p, _ in stream]
    assert sum(sampled) == 4 and len(rest) == 1


def test_fallbacks_yield_once_and_equal_generate(tmp_path):
    from eraxvif5tts_amd.bigvgan import BigVGAN
    tts = _tts(tmp_path, "fp32")
    tts.target_rms = 0.2
    # a cross-fade longer than the chunks: the joints chain, generate() joins on the host
    pieces = _pieces(tts, TEXTS[2], 5, cross_fade_duration=30.0)
    assert len(pieces) == 1 and np.array_equal(pieces[0], _whole(tts, TEXTS[2], 5, cross_fade_duration=30.0))
    vocos = tts.vocoder

    class Foreign(torch.nn.Module):  # plug point B with an object the library knows nothing about
        def decode(self, mel):
            return torch.tanh(mel.mean(dim=1)).repeat_interleave(256, dim=1)[:, 256:] * 0.5

    tts.vocoder = Foreign()
    for kw in ({}, {"return_pcm16": True}):
        pieces = _pieces(tts, TEXTS[2], 10, **kw)
        want = _whole(tts, TEXTS[2], 10, **kw)
        assert len(pieces) == 1 and pieces[0].dtype == want.dtype and np.array_equal(pieces[0], want)
    # the tiny HIP BigVGAN: streamed (T * up samples per chunk), equal
    W = cpu_ref.random_bigvgan_weights(dict(BIGVGAN_TINY), seed=3)
    W["conv_post.weight"] = W["conv_post.weight"] * 0.0015
    big = BigVGAN(dict(BIGVGAN_TINY))
    big.load_state_dict(W)
    tts.vocoder, tts.mel_spec_type = big.eval().cuda(), "bigvgan"
    for kw in ({}, {"return_pcm16": True}):
        pieces = _pieces(tts, TEXTS[2], 9, **kw)
        want = _whole(tts, TEXTS[2], 9, **kw)
        assert len(pieces) == 2 and np.abs(_whole(tts, TEXTS[2], 9)).max() < 1
        assert np.concatenate(pieces).dtype == want.dtype and np.array_equal(np.concatenate(pieces), want)
    tts.vocoder, tts.mel_spec_type = vocos, "vocos"


def test_closing_early_leaves_the_wrapper_usable(tmp_path):
    tts = _tts(tmp_path, "bf16")
    fresh = _whole(tts, TEXTS[4], 21, return_pcm16=True)
    torch.manual_seed(4)
    stream = tts.generate_stream(TEXTS[4], nfe_step=NFE, return_pcm16=True)
    first, _ = next(stream)
    stream.close()
    with pytest.raises(StopIteration):
        next(stream)
    assert len(first) > 0 and np.array_equal(_whole(tts, TEXTS[4], 21, return_pcm16=True), fresh)
    # ... and a stream after an abandoned one is whole again
    assert b"".join(p.tobytes() for p in _pieces(tts, TEXTS[4], 21, return_pcm16=True)) == fresh.tobytes()


def test_stream_audio_with_stream_groups(tmp_path):
    from eraxvif5tts_amd.streaming.wire import ReferenceCache, create_wave_header, stream_audio
    tts = _tts(tmp_path, "bf16")
    tts.target_rms = 0.2
    cache = ReferenceCache()
    cache.entries["spk"] = {"loaded": True, "processed_mel": tts.ref_audio_processed.clone(), "processed_text": tts.ref_text,
                            "processed_mel_len": tts.ref_audio_len}
    chunks = ["hello there.", TEXTS[4]]
    torch.manual_seed(31)
    blocks = list(stream_audio(tts, cache, "spk", chunks, nfe_step=NFE))
    torch.manual_seed(31)
    parts = list(stream_audio(tts, cache, "spk", chunks, stream_groups=True, nfe_step=NFE))
    assert parts[0] == blocks[0] == create_wave_header(SR)
    assert len(blocks) == 3 and len(parts) == 1 + 1 + 2  # one piece for the one-chunk text, two for the four-chunk text
    assert b"".join(parts) == b"".join(blocks)
    assert tts.ref_audio_processed is None and tts.ref_text is None
