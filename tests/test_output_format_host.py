"""Output formats, host side (no GPU): the numpy statement of G.711 against CPython's audioop and the ITU spot values, the G.711 WAV file and
stream header parsed back, the emitted counts of a conversion stream from the extents alone, `F5TTSWrapper.set_output_format`'s validation, the
pinned signatures it must leave alone, and the new symbols in the header and the export list."""
import dataclasses
import inspect
import math
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("f5_op_g711_encode", "f5_wave_convert", "f5_wave_convert_stream_create", "f5_wave_convert_stream_push",
               "f5_wave_convert_stream_destroy")
# input -> (mu-law, A-law)
SPOTS = {0: (0xFF, 0xD5), -1: (0x7E, 0x55), 1000: (0xCE, 0xFA), -1000: (0x4E, 0x7A), 32767: (0x80, 0xAA), -32768: (0x00, 0x2A)}


def test_g711_spot_values():
    from eraxvif5tts_amd.infer.deliver import g711_encode
    for s, (mu, a) in SPOTS.items():
        x = np.array([s], dtype=np.int16)
        assert int(g711_encode(x, "mulaw")[0]) == mu and int(g711_encode(x, 0)[0]) == mu, s
        assert int(g711_encode(x, "alaw")[0]) == a and int(g711_encode(x, 1)[0]) == a, s
    assert g711_encode(np.zeros((2, 3), np.int16), "alaw").shape == (2, 3) and g711_encode(np.zeros(4, np.int16), 0).dtype == np.uint8
    with pytest.raises(ValueError):
        g711_encode(np.zeros(4, np.int16), "g722")
    with pytest.raises(ValueError):
        g711_encode(np.zeros(4, np.float32), "mulaw")


def test_g711_equals_audioop_over_all_int16():
    audioop = pytest.importorskip("audioop")
    from eraxvif5tts_amd.infer.deliver import g711_encode
    every = np.arange(-32768, 32768).astype(np.int16)
    assert g711_encode(every, "mulaw").tobytes() == audioop.lin2ulaw(every.tobytes(), 2)
    assert g711_encode(every, "alaw").tobytes() == audioop.lin2alaw(every.tobytes(), 2)


def _parse_g711(data):
    """-> (format tag, channels, rate, byte rate, block align, bits, cbSize, fact count, riff size, data size, offset of the samples)"""
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE" and data[12:16] == b"fmt " and struct.unpack("<I", data[16:20])[0] == 18
    fmt = struct.unpack("<HHIIHHH", data[20:38])
    assert data[38:42] == b"fact" and struct.unpack("<I", data[42:46])[0] == 4
    assert data[50:54] == b"data"
    return fmt + (struct.unpack("<I", data[46:50])[0], struct.unpack("<I", data[4:8])[0], struct.unpack("<I", data[54:58])[0], 58)


@pytest.mark.parametrize("law,tag", [("mulaw", 7), ("alaw", 6)])
def test_write_wav_g711_parses_back(tmp_path, law, tag):
    from eraxvif5tts_amd.infer.audio import write_wav_g711
    for n in (320, 321, 0):  # (an odd count takes RIFF's pad byte)
        codes = (np.arange(n) * 7 % 256).astype(np.uint8)
        path = str(tmp_path / f"{law}_{n}.wav")
        write_wav_g711(path, codes, 8000, law)
        data = open(path, "rb").read()
        assert _parse_g711(data) == (tag, 1, 8000, 8000, 1, 8, 0, n, 50 + n + (n & 1), n, 58)
        assert len(data) == 58 + n + (n & 1) and data[58: 58 + n] == codes.tobytes()
    with pytest.raises(ValueError):
        write_wav_g711(str(tmp_path / "x.wav"), np.zeros(4, np.int16), 8000, law)


def test_create_stream_header():
    from eraxvif5tts_amd.streaming.wire import create_stream_header, create_wave_header
    for rate in (8000, 16000, 24000, 48000):
        assert create_stream_header(rate, "pcm16") == create_wave_header(rate) == create_stream_header(rate, None) == create_stream_header(rate)
    for law, tag in (("mulaw", 7), ("alaw", 6)):
        head = create_stream_header(8000, law)
        assert len(head) == 58 and _parse_g711(head) == (tag, 1, 8000, 8000, 1, 8, 0, 0, 50, 0, 58)  # unknown sizes
    with pytest.raises(ValueError):
        create_stream_header(8000, "opus")


CUTS_997 = ([997], [1, 996], [5, 1, 991], [3, 3, 3, 988], [18, 1, 1, 1, 976], [400, 1, 596], [996, 1], [100] * 9 + [97])


@pytest.mark.parametrize("out_rate", [8000, 44100])
def test_stream_convert_counts_follow_the_formula(out_rate):
    from eraxvif5tts_amd.infer.deliver import converted_length, resample_plan, stream_convert_counts
    g = math.gcd(24000, out_rate)
    orig, new = 24000 // g, out_rate // g
    width = math.ceil(6 * orig / (min(orig, new) * 0.99))
    assert resample_plan(24000, out_rate) == (orig, new, width, 2 * width + orig)
    n = 997
    target = math.ceil(new * n / orig)
    assert converted_length(n, 24000, out_rate) == target
    for cuts in CUTS_997:
        assert sum(cuts) == n
        counts = stream_convert_counts(cuts, 24000, out_rate)
        taken, out = 0, 0
        for i, (length, count) in enumerate(zip(cuts, counts)):
            taken += length
            out += count
            assert out == (target if i == len(cuts) - 1 else new * max(0, (taken - width) // orig)), (cuts, i)
        assert sum(counts) == target and all(c >= 0 for c in counts)
    assert stream_convert_counts([1, 996], 24000, out_rate)[0] == 0  # a one-sample push: no block has its support yet


def test_resample_taps_are_the_oracles_table():
    """the table the library multiplies by is fp32-exact and agrees with the direct formula of oracle/cpu_ref.resample (which orders the last
    two factors differently: at most an fp32 ulp apart after the cast)"""
    from eraxvif5tts_amd.infer.deliver import resample_taps_host
    for out_rate in (8000, 16000, 22050, 44100, 48000):
        h = resample_taps_host(24000, out_rate)
        g = math.gcd(24000, out_rate)
        orig, new = 24000 // g, out_rate // g
        base = min(orig, new) * 0.99
        width = math.ceil(6 * orig / base)
        assert h.dtype == np.float64 and h.shape == (new, 2 * width + orig) and np.array_equal(h, h.astype(np.float32).astype(np.float64))
        k = np.arange(2 * width + orig, dtype=np.float64)
        for j in (0, new - 1):
            t = np.clip(((k - width) / orig - j / new) * base, -6.0, 6.0)
            tp = t * math.pi
            with np.errstate(invalid="ignore", divide="ignore"):
                want = np.where(tp == 0.0, 1.0, np.sin(tp) / tp) * np.cos(t * math.pi / 12.0) ** 2 * (base / orig)
            assert np.abs(h[j] - want).max() <= 2.0 ** -23 * np.abs(want).max()


def _bare_wrapper():
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    w = F5TTSWrapper.__new__(F5TTSWrapper)
    w.target_sample_rate = 24000
    return w


def test_set_output_format_validation_and_defaults():
    w = _bare_wrapper()
    assert w.output_format is None
    for args in ((), (None, None), (24000, None), (None, "pcm16"), (24000, "pcm16")):
        w.set_output_format(8000, "mulaw")
        w.set_output_format(*args)
        assert w.output_format is None, args
    w.set_output_format(8000)
    assert w.output_format == (8000, "pcm16")
    w.set_output_format(sample_rate=16000, encoding="pcm16")
    assert w.output_format == (16000, "pcm16")
    w.set_output_format(encoding="alaw")
    assert w.output_format == (24000, "alaw")
    w.set_output_format(8000, "mulaw")
    assert w.output_format == (8000, "mulaw")
    for bad in ((0, None), (-8000, None), (8000.0, None), ("8000", None), (True, None), (8000, "opus"), (8000, "PCM16"), (None, 7), (None, "")):
        with pytest.raises(ValueError):
            w.set_output_format(*bad)
        assert w.output_format == (8000, "mulaw"), bad  # a refused call changes nothing
    with pytest.raises(ValueError):
        w.set_output_format(24001)  # coprime with 24000: a table of 24001 phases is beyond what the library takes


def test_pinned_signatures_are_untouched():
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper, TTSJob
    assert list(inspect.signature(F5TTSWrapper.generate_batch).parameters) == ["self", "requests", "return_pcm16", "return_spectrogram"]
    assert [f.name for f in dataclasses.fields(TTSJob)] == ["text", "voice", "nfe_step", "cfg_strength", "sway_sampling_coef", "speed", "fix_duration",
                                                            "cross_fade_duration", "use_duration_predictor", "remove_silence", "seed"]
    for name in ("generate", "generate_stream", "generate_multi", "generate_multi_stream"):
        params = inspect.signature(getattr(F5TTSWrapper, name)).parameters
        assert "sample_rate" not in params and "encoding" not in params and "output_format" not in params
    assert list(inspect.signature(F5TTSWrapper.set_output_format).parameters) == ["self", "sample_rate", "encoding"]
    assert isinstance(F5TTSWrapper.output_format, property)


def test_new_symbols_are_declared_and_exported():
    from eraxvif5tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    for name in NEW_SYMBOLS:
        decl = re.search(r"F5_API\s+int\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl and name in _lib.EXPORTS, name
        assert len(decl[1].split(",")) == len(_lib._PROTOS[name][1]), name
    assert re.search(r"#define F5HIP_VERSION 400\b", header)  # detected by symbol: the number stays
    lib = _lib.load(build_if_missing=True)
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS) and lib.f5_version() == 400


def test_stream_audio_forwards_the_format_of_a_duck_typed_model():
    """a model with `output_format` gets that format's header and its uint8 pieces as they are; one without gets today's bytes"""
    from eraxvif5tts_amd.streaming.wire import ReferenceCache, create_stream_header, create_wave_header, stream_audio

    class Model:
        device, target_sample_rate = "cpu", 24000
        ref_audio_processed = ref_text = ref_audio_len = None

        def __init__(self, fmt):
            if fmt != "absent":
                self.output_format = fmt

        def generate(self, text, return_numpy=False, return_pcm16=False):
            fmt = getattr(self, "output_format", None)
            if fmt and fmt[1] != "pcm16":
                return np.arange(len(text), dtype=np.uint8) + 200, fmt[0]
            return np.arange(len(text), dtype=np.int16) - 3, fmt[0] if fmt else 24000

    cache = ReferenceCache()
    cache.entries["spk"] = {"loaded": True, "processed_mel": np.zeros(4), "processed_text": "x", "processed_mel_len": 1}
    blocks = list(stream_audio(Model((8000, "mulaw")), cache, "spk", ["abcd"]))
    assert blocks == [create_stream_header(8000, "mulaw"), bytes([200, 201, 202, 203])]
    blocks = list(stream_audio(Model((16000, "pcm16")), cache, "spk", ["abcd"]))
    assert blocks == [create_wave_header(16000), (np.arange(4, dtype=np.int16) - 3).tobytes()]
    for fmt in ("absent", None):
        blocks = list(stream_audio(Model(fmt), cache, "spk", ["abcd"]))
        assert blocks == [create_wave_header(24000), (np.arange(4, dtype=np.int16) - 3).tobytes()]
