"""Output formats on the device (csrc/deliver.hip): the G.711 encoder over every int16 value; the one-shot conversion bit for bit against a
restatement written here -- the ordered fp64 loop over the taps of include/f5hip.h, with the table the library is handed -- and, inside the
project's resampler bounds, against oracle/cpu_ref.resample; every way of cutting a signal into pushes gives the one-shot bytes; the refusals;
and the wrapper's `set_output_format` through all five entry points and the wire generator, on the tiny wrapper of tests/test_gpu_wave_tail.py."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from test_gpu_wave_tail import SR, TEXTS, _tts

pytestmark = pytest.mark.gpu
NFE = 3
RATES = (8000, 16000, 22050, 44100, 48000)
SIZES = (1, 40, 997, 4801)
F5_EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


# ----------------------------------------------------------------------------- the restatement
def restate(x, out_rate, in_rate=SR):
    """include/f5hip.h, f5_wave_convert, in numpy: per output ONE fp64 accumulator from 0.0 that takes the fp64 products over ascending k (numpy
    multiplies and adds in separate passes: nothing is contracted), a tap outside [0, n) skipped; then (float)acc, the fp32 product with 32767,
    truncation with saturation.  -> (float32, int16)"""
    from eraxvif5tts_amd.infer.deliver import resample_taps_host
    g = math.gcd(in_rate, out_rate)
    orig, new = in_rate // g, out_rate // g
    width = math.ceil(6 * orig / (min(orig, new) * 0.99))
    kw = 2 * width + orig
    taps = resample_taps_host(in_rate, out_rate)
    assert taps.shape == (new, kw)
    x64 = np.asarray(x).astype(np.float64)
    n = len(x64)
    j = np.arange(math.ceil(new * n / orig))
    blk, ph = j // new, j % new
    acc = np.zeros(len(j), dtype=np.float64)
    for k in range(kw):
        idx = blk * orig - width + k
        ok = (idx >= 0) & (idx < n)
        prod = x64[np.clip(idx, 0, n - 1)] * taps[ph, k]
        acc = np.where(ok, acc + prod, acc)
    f = acc.astype(np.float32)
    p = f * np.float32(32767.0)
    assert p.dtype == np.float32
    pcm = np.where(p >= 32767.0, 32767.0, np.where(p <= -32768.0, -32768.0, np.trunc(p))).astype(np.int16)
    return f, pcm


def _noise(n, dtype, seed=0):
    return (np.random.default_rng(1000 * seed + n).standard_normal(n) * 0.3).astype(dtype)


def _square():
    return np.where((np.arange(960) % 74) < 37, 1.0, -1.0).astype(np.float32)  # full scale, period 74


def _impulses(n=997):
    x = np.zeros(n, dtype=np.float32)
    x[0], x[-1] = 1.0, 1.0
    return x


_REF = {}


def _reference(name, out_rate, make):
    """restatement and codes of one signal at one rate, computed once and shared"""
    from eraxvif5tts_amd.infer.deliver import g711_encode
    key = (name, out_rate)
    if key not in _REF:
        x = make()
        f, pcm = restate(x, out_rate)
        _REF[key] = (x, f, pcm, g711_encode(pcm, "mulaw"), g711_encode(pcm, "alaw"))
    return _REF[key]


def _convert_all(x, out_rate):
    """(float32, int16, mu-law codes, A-law codes) of the device conversion, on the host"""
    from eraxvif5tts_amd.infer.deliver import convert_wave
    t = torch.from_numpy(x).cuda()
    f, pcm = convert_wave(t, SR, out_rate, "pcm16", want_float=True, want_codes=True)
    f2, mu = convert_wave(t, SR, out_rate, "mulaw", want_float=True, want_codes=True)
    _, al = convert_wave(t, SR, out_rate, "alaw", want_float=False, want_codes=True)
    assert torch.equal(f, f2) and f.dtype == torch.float32 and pcm.dtype == torch.int16 and mu.dtype == al.dtype == torch.uint8
    return f.cpu().numpy(), pcm.cpu().numpy(), mu.cpu().numpy(), al.cpu().numpy()


def _assert_bits(got, want, what):
    f, pcm, mu, al = got
    _, rf, rpcm, rmu, ral = want
    assert f.shape == rf.shape, what
    assert f.tobytes() == rf.tobytes(), f"{what}: {int((f.view(np.uint32) != rf.view(np.uint32)).sum())} float32 values differ"
    assert pcm.tobytes() == rpcm.tobytes(), f"{what}: int16"
    assert mu.tobytes() == rmu.tobytes() and al.tobytes() == ral.tobytes(), f"{what}: G.711"


# ----------------------------------------------------------------------------- G.711
@pytest.mark.parametrize("law", ["mulaw", "alaw"])
def test_g711_encoder_over_every_int16(law):
    from eraxvif5tts_amd.infer.deliver import g711_encode, g711_encode_device
    every = np.arange(-32768, 32768).astype(np.int16)
    got = g711_encode_device(torch.from_numpy(every).cuda(), law).cpu().numpy()
    want = g711_encode(every, law)
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), f"{law}: first difference at {every[np.nonzero(got != want)[0][:1]]}"


# ----------------------------------------------------------------------------- one shot
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("out_rate", RATES)
def test_one_shot_equals_the_restatement_bit_for_bit(out_rate, dtype):
    for n in SIZES:
        name = f"noise{n}_{np.dtype(dtype).name}"
        want = _reference(name, out_rate, lambda: _noise(n, dtype))
        g = math.gcd(SR, out_rate)
        assert len(want[1]) == math.ceil(out_rate // g * n / (SR // g))
        _assert_bits(_convert_all(want[0], out_rate), want, f"{SR} -> {out_rate}, n = {n}, {np.dtype(dtype).name}")


@pytest.mark.parametrize("out_rate", RATES)
def test_edge_impulses_and_a_saturating_square(out_rate):
    want = _reference("impulses", out_rate, _impulses)
    _assert_bits(_convert_all(want[0], out_rate), want, f"{SR} -> {out_rate}, impulses at the first and the last sample")
    want = _reference("square", out_rate, _square)
    clipped = int(((want[2] == 32767) | (want[2] == -32768)).sum())
    print(f"square wave at {out_rate} Hz: peak {np.abs(want[1]).max():.3f}, {clipped} of {len(want[2])} samples saturate")
    assert clipped >= 1 and np.abs(want[1]).max() > 1.0  # the restatement itself takes the saturation branch
    _assert_bits(_convert_all(want[0], out_rate), want, f"{SR} -> {out_rate}, full-scale square wave")


@pytest.mark.parametrize("out_rate", RATES)
def test_one_shot_inside_the_oracles_bounds(out_rate):
    """oracle/cpu_ref.resample (float64, a direct polyphase sum) with the resampler bounds of tests/test_gpu_audio_configs.py"""
    from eraxvif5tts_amd.infer.deliver import convert_wave
    cases = [(f"noise{n}_{np.dtype(d).name}", (lambda n=n, d=d: _noise(n, d))) for n in SIZES for d in (np.float32, np.float64)]
    cases += [("impulses", _impulses), ("square", _square)]
    for name, make in cases:
        x = _reference(name, out_rate, make)[0]
        ref = cpu_ref.resample(torch.from_numpy(x), SR, out_rate).double()
        out = convert_wave(torch.from_numpy(x).cuda(), SR, out_rate)[0].cpu()
        assert out.dtype == torch.float32 and out.shape == ref.shape
        rel = float((out.double() - ref).norm() / ref.norm().clamp_min(1e-30))
        peak = float((out.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        print(f"{SR} -> {out_rate} {name}: rel-L2 {rel:.2e}, max error / max |ref| {peak:.2e}")
        assert rel <= 1e-5 and peak <= 1e-6, (name, rel, peak)


# ----------------------------------------------------------------------------- pushes
CUTS = ([997], [1, 996], [5, 1, 991], [3, 3, 3, 988], [18, 1, 1, 1, 976], [400, 1, 596], [996, 1], [100] * 9 + [97])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("out_rate", [8000, 44100])
def test_every_cut_gives_the_one_shot_bytes(out_rate, dtype):
    """the lists hold a single push, one-sample pushes and pushes shorter than width (19 samples at 8 kHz, 7 at 44.1 kHz)"""
    from eraxvif5tts_amd.infer.deliver import ConvertStream, stream_convert_counts
    want = _reference(f"noise997_{np.dtype(dtype).name}", out_rate, lambda: _noise(997, dtype))
    x = torch.from_numpy(want[0]).cuda()
    for enc, codes_want in (("pcm16", want[2]), ("mulaw", want[3]), ("alaw", want[4])):
        for cuts in CUTS:
            counts = stream_convert_counts(cuts, SR, out_rate)
            s = ConvertStream(SR, out_rate, enc, is_f64=dtype is np.float64, want_float=True, want_codes=True)
            floats, codes, at = [], [], 0
            for i, (length, count) in enumerate(zip(cuts, counts)):
                f, c = s.push(x[at: at + length], last=i == len(cuts) - 1)
                assert f.numel() == c.numel() == count, (cuts, i)
                floats.append(f.cpu().numpy())
                codes.append(c.cpu().numpy())
                at += length
            s.close()
            assert np.concatenate(floats).tobytes() == want[1].tobytes(), (enc, cuts)
            assert np.concatenate(codes).tobytes() == codes_want.tobytes(), (enc, cuts)


def _raw_stream(out_rate, taps, is_f64=0, law=0):
    from eraxvif5tts_amd import _lib
    h = C.c_void_p()
    rc = _lib.load().f5_wave_convert_stream_create(SR, out_rate, _lib.ptr(taps), is_f64, law, C.byref(h))
    return rc, h


def test_query_form_and_refusals_leave_the_session_unchanged():
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.infer.deliver import resample_taps
    lib = _lib.load()
    want = _reference("noise997_float32", 8000, lambda: _noise(997, np.float32))
    x = torch.from_numpy(want[0]).cuda()
    taps = resample_taps(SR, 8000)
    rc, h = _raw_stream(8000, taps)
    assert rc == 0
    got = C.c_int64(-1)
    out, pieces, at = torch.zeros(400, device="cuda"), [], 0

    def push(n, last, with_out=True, ptr=None):
        return lib.f5_wave_convert_stream_push(h, _lib.ptr(x[at:]) if ptr is None else ptr, n, last, _lib.ptr(out) if with_out else None, None, None,
                                               C.byref(got), _lib.stream_ptr())

    for n, last in ((300, 0), (200, 0), (497, 1)):
        for _ in range(3):  # the question, asked as often as one likes, moves nothing
            assert push(n, last, with_out=False) == 0
        asked = got.value
        assert push(0, last) == F5_EINVAL and push(-5, last) == F5_EINVAL  # refused: the session stays where it was
        assert push(n, last) == 0 and got.value == asked
        pieces.append(out[:asked].cpu().numpy().copy())
        at += n
    assert [len(p) for p in pieces] == [93, 67, 173]  # (300 - 19) // 3, (500 - 19) // 3 - 93, ceil(997 / 3) - 160
    assert np.concatenate(pieces).tobytes() == want[1].tobytes()
    assert push(1, 0, ptr=_lib.ptr(x)) == F5_EINVAL and push(1, 1, ptr=_lib.ptr(x)) == F5_EINVAL  # a push after the last one
    assert lib.f5_wave_convert_stream_destroy(h) == 0
    # creation and the one-shot call
    assert _raw_stream(SR, taps)[0] == F5_EINVAL and _raw_stream(0, taps)[0] == F5_EINVAL and _raw_stream(-8000, taps)[0] == F5_EINVAL
    assert _raw_stream(24001, taps)[0] == F5_EINVAL  # 24001 phases of 24014 taps: beyond 2^20 table entries

    def one_shot(n, in_rate, out_rate):
        return lib.f5_wave_convert(_lib.ptr(x), 0, n, in_rate, out_rate, _lib.ptr(taps), 0, _lib.ptr(out), None, None, C.byref(got), _lib.stream_ptr())

    out.fill_(7.0)
    for args in ((0, SR, 8000), (-1, SR, 8000), (997, SR, SR), (997, 0, 8000), (997, SR, -1), (997, SR, 24001)):
        assert one_shot(*args) == F5_EINVAL, args
    assert lib.f5_wave_convert(_lib.ptr(x), 0, 997, SR, 8000, _lib.ptr(taps), 2, None, None, _lib.ptr(torch.zeros(400, dtype=torch.uint8, device="cuda")),
                               C.byref(got), _lib.stream_ptr()) == F5_EINVAL  # a law that is neither
    assert lib.f5_op_g711_encode(4, _lib.ptr(torch.zeros(4, dtype=torch.int16, device="cuda")), 2,
                                 _lib.ptr(torch.zeros(4, dtype=torch.uint8, device="cuda")), _lib.stream_ptr()) == F5_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # a refused call writes nothing
    assert lib.f5_wave_convert(None, 0, 997, SR, 8000, None, 0, None, None, None, C.byref(got), None) == 0 and got.value == 333  # the extent alone


# ----------------------------------------------------------------------------- the wrapper
@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    """the tiny wrapper of tests/test_gpu_wave_tail.py (fp32), a second voice from the same file, the gain on"""
    root = tmp_path_factory.mktemp("output_format")
    w = _tts(root, "fp32")
    w.add_voice("town", os.path.join(str(root), "ref.wav"), "a quiet tone")
    w.target_rms = 0.2
    w.root = str(root)
    return w


@pytest.fixture(autouse=True)
def _unset(request):
    yield
    if "tts" in request.fixturenames:
        request.getfixturevalue("tts").set_output_format()


def _gen(tts, seed, text=None, entry="generate", **kw):
    torch.manual_seed(seed)
    return getattr(tts, entry)(TEXTS[2] if text is None else text, nfe_step=NFE, return_numpy=True, **kw)


def _pieces(tts, seed, text, entry, **kw):
    torch.manual_seed(seed)
    out = list(getattr(tts, entry)(text, nfe_step=NFE, **kw))
    return [p for p, _ in out], {rate for _, rate in out}


def test_set_then_unset_changes_nothing(tts):
    before = [_gen(tts, 41), _gen(tts, 41, return_pcm16=True), _gen(tts, 41, cross_fade_duration=0.0)]
    tts.set_output_format(8000, "mulaw")
    assert _gen(tts, 41)[1] == 8000
    tts.set_output_format()
    after = [_gen(tts, 41), _gen(tts, 41, return_pcm16=True), _gen(tts, 41, cross_fade_duration=0.0)]
    for (a, ra), (b, rb) in zip(before, after):
        assert ra == rb == SR and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_alaw_at_the_native_rate_encodes_the_tails_pcm(tts):
    from eraxvif5tts_amd.infer.deliver import g711_encode
    pcm, _ = _gen(tts, 42, return_pcm16=True)
    plain, _ = _gen(tts, 42)
    tts.set_output_format(None, "alaw")
    codes, rate = _gen(tts, 42, return_pcm16=True)
    assert rate == SR and codes.dtype == np.uint8 and codes.tobytes() == g711_encode(pcm, "alaw").tobytes()
    wave, rate = _gen(tts, 42)
    assert rate == SR and wave.dtype == plain.dtype and np.array_equal(wave, plain)  # nothing is resampled


def test_mulaw_at_8k_equals_the_restated_conversion_and_the_file_holds_it(tts):
    from eraxvif5tts_amd.infer.deliver import g711_encode
    plain, _ = _gen(tts, 43)
    assert plain.dtype == np.float64  # two chunks, cross-faded
    f, pcm = restate(plain, 8000)
    want = g711_encode(pcm, "mulaw")
    tts.set_output_format(8000, "mulaw")
    codes, rate = _gen(tts, 43, return_pcm16=True)
    assert rate == 8000 and codes.dtype == np.uint8 and codes.tobytes() == want.tobytes()
    wave, rate = _gen(tts, 43)
    assert rate == 8000 and wave.dtype == np.float32 and wave.tobytes() == f.tobytes()
    path = os.path.join(tts.root, "out", "mulaw.wav")
    torch.manual_seed(43)
    assert tts.generate(TEXTS[2], path, nfe_step=NFE) == path
    data = open(path, "rb").read()
    assert struct.unpack("<HHIIHHH", data[20:38]) == (7, 1, 8000, 8000, 1, 8, 0) and data[38:42] == b"fact" and data[50:54] == b"data"
    assert struct.unpack("<I", data[46:50])[0] == struct.unpack("<I", data[54:58])[0] == len(want) and data[58: 58 + len(want)] == want.tobytes()
    # PCM16 at another rate: the int16 of the restatement; the file is `write_wav` of the float at that rate
    tts.set_output_format(16000)
    f16, pcm16 = restate(plain, 16000)
    got, rate = _gen(tts, 43, return_pcm16=True)
    assert rate == 16000 and got.dtype == np.int16 and got.tobytes() == pcm16.tobytes()
    from eraxvif5tts_amd.infer import audio
    torch.manual_seed(43)
    path = tts.generate(TEXTS[2], os.path.join(tts.root, "out", "pcm.wav"), nfe_step=NFE)
    audio.write_wav(os.path.join(tts.root, "want.wav"), f16, 16000)
    assert open(path, "rb").read() == open(os.path.join(tts.root, "want.wav"), "rb").read()


@pytest.mark.parametrize("fade", [None, 0.0])  # the wrapper's 0.15 s (an fp64 tail) and none (fp32)
@pytest.mark.parametrize("entry", ["generate", "generate_multi"])
def test_streamed_pieces_equal_the_one_shot_result(tts, entry, fade):
    text = TEXTS[4] if entry == "generate" else f"[main] {TEXTS[2]} [town] {TEXTS[2]}"  # four chunks either way: groups of 1 and 3
    kw = {} if fade is None else {"cross_fade_duration": fade}
    for fmt, pcm in (((8000, "mulaw"), True), ((44100, None), False), ((44100, None), True), ((None, "alaw"), True)):
        tts.set_output_format(*fmt)
        whole, rate = _gen(tts, 44, text, entry, return_pcm16=pcm, **kw)
        pieces, rates = _pieces(tts, 44, text, entry + "_stream", return_pcm16=pcm, **kw)
        assert rates == {rate} and rate == (fmt[0] or SR) and len(pieces) == 2
        assert all(p.dtype == whole.dtype for p in pieces) and np.concatenate(pieces).tobytes() == whole.tobytes(), (entry, fade, fmt, pcm)
        assert whole.dtype == (np.uint8 if fmt[1] else np.int16 if pcm else np.float32)
    # the fallback's single yield is the converted one-shot result (a cross-fade longer than the chunks: the joints chain, the host joins)
    tts.set_output_format(8000, "mulaw")
    whole, _ = _gen(tts, 45, text, entry, return_pcm16=True, cross_fade_duration=30.0)
    pieces, rates = _pieces(tts, 45, text, entry + "_stream", return_pcm16=True, cross_fade_duration=30.0)
    assert len(pieces) == 1 and rates == {8000} and pieces[0].dtype == np.uint8 and pieces[0].tobytes() == whole.tobytes()


def test_generate_batch_equals_the_generate_calls(tts):
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    reqs = [TTSJob(TEXTS[2], nfe_step=NFE), TTSJob("hello there.", voice="town", nfe_step=NFE, remove_silence=True)]
    for fmt, pcm in (((8000, "mulaw"), True), ((48000, None), False), ((None, "alaw"), True)):
        tts.set_output_format(*fmt)
        torch.manual_seed(46)
        want = []
        for q in reqs:
            with tts._voice_installed(tts.voices[q.voice]):
                want.append(tts.generate(q.text, nfe_step=NFE, return_numpy=True, return_pcm16=pcm, remove_silence=q.remove_silence))
        torch.manual_seed(46)
        got = tts.generate_batch(reqs, return_pcm16=pcm)
        for (a, ra), (b, rb) in zip(got, want):
            assert ra == rb == (fmt[0] or SR) and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (fmt, pcm)


def test_stream_audio_sends_the_g711_header_and_the_codes(tts):
    from eraxvif5tts_amd.streaming.wire import ReferenceCache, create_stream_header, stream_audio
    cache = ReferenceCache()
    cache.entries["spk"] = {"loaded": True, "processed_mel": tts.ref_audio_processed.clone(), "processed_text": tts.ref_text,
                            "processed_mel_len": tts.ref_audio_len}
    kept = tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len
    try:
        tts.set_output_format(8000, "mulaw")
        codes, _ = _gen(tts, 47, TEXTS[4], return_pcm16=True)
        for grouped in (False, True):
            torch.manual_seed(47)
            blocks = list(stream_audio(tts, cache, "spk", [TEXTS[4]], stream_groups=grouped, nfe_step=NFE))
            tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len = kept
            assert blocks[0] == create_stream_header(8000, "mulaw") and len(blocks[0]) == 58 and len(blocks) == (3 if grouped else 2)
            assert b"".join(blocks[1:]) == codes.tobytes()
    finally:
        tts.ref_audio_processed, tts.ref_text, tts.ref_audio_len = kept
