"""The wave tail with a carry (`f5_wave_stream_create / _push / _destroy`, `utils_infer.WaveStream`) at op level, on random waves with
|x| <= 0.99.  Acceptance is exactness: for every way of cutting an utterance list into consecutive pushes the emitted pieces, concatenated, are
byte-identical to ONE `f5_wave_finish` (`finish_waves`) over the whole list, float and PCM."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_generate_stream_host import compositions
from test_gpu_wave_segments import D as D16, _lengths as _seg_lengths  # a cross-fade of 16 samples, lengths from {16 .. 257} within the rule
from test_gpu_wave_tail import DURATIONS, HOST_RMS, LENGTHS, SR, _host_tail

pytestmark = pytest.mark.gpu
F5_EINVAL, F5_ENOTSUP = -1, -5  # include/f5hip.h
TARGET = 0.1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _waves(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(sum(lengths), generator=g) * 2 - 1) * 0.99).cuda()


def _rms(gain):
    return {"none": None, "host_list": HOST_RMS, "dev_applied": torch.tensor(0.07, device="cuda"),
            "dev_not_applied": torch.tensor(0.13, device="cuda")}[gain]


def _push_all(buf, lengths, sizes, d, rms, poison=False, counts=None):
    """the list in consecutive pushes of `sizes` utterances, each from a buffer of its own -> (float pieces, pcm pieces) on the host"""
    from eraxvif5tts_amd.infer.utils_infer import WaveStream
    ws = WaveStream(lengths, d, SR, rms=rms, target_rms=TARGET, want_float=True, want_pcm16=True)
    assert ws.ok
    sigs, pcms, k, at = [], [], 0, 0
    try:
        for i, size in enumerate(sizes):
            samples = lengths[k: k + size]
            wave = buf[at: at + sum(samples)].clone()
            sig, pcm = ws.push(wave, samples)
            if poison:
                wave.fill_(float("nan"))  # same stream, behind the push: the carry must not live in the caller's buffer
            if counts is not None:
                assert sig.numel() == pcm.numel() == counts[i]
            sigs.append(sig)
            pcms.append(pcm)
            k, at = k + size, at + sum(samples)
        return [s.cpu().numpy() for s in sigs], [p.cpu().numpy() for p in pcms]
    finally:
        ws.close()


@pytest.mark.parametrize("gain", ["none", "host_list", "dev_applied", "dev_not_applied"])
@pytest.mark.parametrize("dname", ["off", "default", "one_sample"])
def test_every_cut_gives_the_one_shot_bytes(dname, gain):
    from eraxvif5tts_amd.infer.utils_infer import finish_waves, stream_emitted_counts
    d, rms = DURATIONS[dname], _rms(gain)
    buf = _waves(LENGTHS, seed=len(dname) * 5 + len(gain))
    want_sig, want_pcm = (t.cpu().numpy() for t in finish_waves(buf, LENGTHS, d, SR, rms=rms, target_rms=TARGET, want_pcm16=True))
    cuts = compositions(len(LENGTHS))
    assert len(cuts) == 16
    for sizes in cuts:
        counts, dtype = stream_emitted_counts(LENGTHS, sizes, d, SR)
        sigs, pcms = _push_all(buf, LENGTHS, sizes, d, rms, counts=counts)
        assert all(s.dtype == dtype == want_sig.dtype for s in sigs), sizes
        got = np.concatenate(sigs)
        assert got.dtype == want_sig.dtype and np.array_equal(got, want_sig), sizes
        assert np.concatenate(pcms).tobytes() == want_pcm.tobytes(), sizes


def test_streamed_pieces_equal_the_host_functions_byte_for_byte():
    """The one-shot call runs the kernel and the host path of a push, so this cut is compared with the host functions themselves: torch's gain
    per wave, numpy's `cross_fade_concat`, `pcm16_bytes` of that array.  Every product lies inside int16, so numpy's cast is defined for every
    sample and all of them are compared."""
    from eraxvif5tts_amd.streaming.wire import pcm16_bytes
    d = DURATIONS["default"]
    buf = _waves(LENGTHS, seed=71)
    ref = _host_tail(list(torch.split(buf, LENGTHS)), d, HOST_RMS, TARGET)
    assert ref.dtype == np.float64 and len(ref) == sum(LENGTHS) - 4 * int(d * SR)
    assert (np.abs(ref * 32767) < 32767).all()
    sigs, pcms = _push_all(buf, LENGTHS, [2, 2, 1], d, HOST_RMS, poison=True)
    got = np.concatenate(sigs)
    assert got.dtype == np.float64 and got.tobytes() == ref.tobytes()
    assert np.concatenate(pcms).tobytes() == pcm16_bytes(ref)


def test_a_push_with_both_carries_across_a_table_split():
    """70 utterances in one segment, pushed as 3, 66 and 1: the middle push reads a carry, spans two kernel tables (64, and 3 that overlap by one)
    and writes a carry"""
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    lengths = _seg_lengths([70], 70)
    buf = _waves(lengths, seed=70)
    rms = torch.tensor(0.07, device="cuda")
    want_sig, want_pcm = finish_waves(buf, lengths, D16, SR, rms=rms, target_rms=TARGET, want_pcm16=True)
    assert want_sig.dtype == torch.float64 and want_sig.numel() == sum(lengths) - 16 * 69
    sigs, pcms = _push_all(buf, lengths, [3, 66, 1], D16, rms, poison=True)
    assert torch.equal(torch.from_numpy(np.concatenate(sigs)), want_sig.cpu())
    assert torch.equal(torch.from_numpy(np.concatenate(pcms)), want_pcm.cpu())


def test_the_first_push_alone_decides_nothing_about_the_dtype():
    from eraxvif5tts_amd.infer.utils_infer import finish_waves, plan_wave_tail
    lengths, d = [60000, LENGTHS[1]], 0.15  # (long enough that the fp32 and the fp64 PCM product disagree on a few samples: about 1 in 3000)
    buf = _waves(lengths, seed=41)
    rms = torch.tensor(0.07, device="cuda")
    want_sig, want_pcm = (t.cpu().numpy() for t in finish_waves(buf, lengths, d, SR, rms=rms, target_rms=TARGET, want_pcm16=True))
    sigs, pcms = _push_all(buf, lengths, [1, 1], d, rms)
    first = plan_wave_tail(lengths, d, SR)["out_offsets"][1]
    assert sigs[0].dtype == np.float64 and len(sigs[0]) == first == lengths[0] - 3600
    assert np.array_equal(sigs[0], want_sig[:first]) and pcms[0].tobytes() == want_pcm[:first].tobytes()
    # ... which an fp32 product would not give: the float32 route of a lone utterance differs on some samples
    _, pcm32 = finish_waves(buf[: lengths[0]].clone(), lengths[:1], d, SR, rms=rms, target_rms=TARGET, want_pcm16=True)
    assert (pcm32.cpu().numpy()[:first] != want_pcm[:first]).any()
    assert np.array_equal(np.concatenate(sigs), want_sig) and np.concatenate(pcms).tobytes() == want_pcm.tobytes()
    # one utterance in all: float32, everything emitted, the one-shot call's bytes
    want_sig, want_pcm = (t.cpu().numpy() for t in finish_waves(buf[: lengths[0]].clone(), lengths[:1], d, SR, rms=rms, target_rms=TARGET,
                                                                want_pcm16=True))
    sigs, pcms = _push_all(buf, lengths[:1], [1], d, rms)
    assert sigs[0].dtype == want_sig.dtype == np.float32 and len(sigs[0]) == lengths[0]
    assert np.array_equal(sigs[0], want_sig) and pcms[0].tobytes() == want_pcm.tobytes()


def test_the_carry_is_the_sessions():
    from eraxvif5tts_amd.infer.utils_infer import WaveStream, finish_waves
    d = 0.15
    buf_a, buf_b = _waves(LENGTHS, seed=51), _waves(LENGTHS[::-1], seed=52)
    want = {}
    for name, buf, lengths, rms in (("a", buf_a, LENGTHS, HOST_RMS), ("b", buf_b, LENGTHS[::-1], None)):
        want[name] = tuple(t.cpu().numpy() for t in finish_waves(buf, lengths, d, SR, rms=rms, target_rms=TARGET, want_pcm16=True))
    # the pushed buffer is overwritten behind every push
    for sizes in ([1, 1, 1, 1, 1], [2, 1, 2]):
        sigs, pcms = _push_all(buf_a, LENGTHS, sizes, d, HOST_RMS, poison=True)
        assert np.array_equal(np.concatenate(sigs), want["a"][0]) and np.concatenate(pcms).tobytes() == want["a"][1].tobytes()
    # two sessions pushed alternately
    sa = WaveStream(LENGTHS, d, SR, rms=HOST_RMS, target_rms=TARGET, want_pcm16=True)
    sb = WaveStream(LENGTHS[::-1], d, SR, rms=None, target_rms=TARGET, want_pcm16=True)
    got = {"a": [], "b": []}
    try:
        at_a = at_b = 0
        for i in range(5):
            la, lb = LENGTHS[i], LENGTHS[::-1][i]
            wa, wb = buf_a[at_a: at_a + la].clone(), buf_b[at_b: at_b + lb].clone()
            got["a"].append(sa.push(wa, [la]))
            got["b"].append(sb.push(wb, [lb]))
            wa.fill_(float("nan"))
            wb.fill_(float("nan"))
            at_a, at_b = at_a + la, at_b + lb
    finally:
        sa.close()
        sb.close()
    for name in ("a", "b"):
        sig = np.concatenate([s.cpu().numpy() for s, _ in got[name]])
        pcm = np.concatenate([p.cpu().numpy() for _, p in got[name]])
        assert np.array_equal(sig, want[name][0]) and pcm.tobytes() == want[name][1].tobytes()


def test_more_utterances_than_a_table_holds():
    """the 150 utterances of test_wave_finish_many_utterances_and_saturation, n = 1 and n = 40"""
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    g = torch.Generator().manual_seed(2)
    lengths = [int(x) for x in torch.randint(80, 400, (150,), generator=g)]
    buf = ((torch.rand(sum(lengths), generator=g) * 2 - 1) * 0.99).cuda()
    rms = [0.02 + 0.001 * i for i in range(150)]
    for d in (1 / 24000, 40 / 24000 + 1e-9):
        want_sig, want_pcm = (t.cpu().numpy() for t in finish_waves(buf, lengths, d, SR, rms=rms, target_rms=TARGET, want_pcm16=True))
        for sizes in ([1, 149], [75, 75]):
            sigs, pcms = _push_all(buf, lengths, sizes, d, rms, poison=True)
            got = np.concatenate(sigs)
            assert got.dtype == want_sig.dtype and np.array_equal(got, want_sig), (d, sizes)
            assert np.concatenate(pcms).tobytes() == want_pcm.tobytes(), (d, sizes)


def _raw_session(total, n):
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.infer.utils_infer import _xfade_weights
    tables = _xfade_weights(n, torch.device("cuda", torch.cuda.current_device())) if n > 0 and total >= 2 else (None, None)
    handle = C.c_void_p()
    _lib.check(_lib.load().f5_wave_stream_create(total, n, _lib.ptr(tables[0]), _lib.ptr(tables[1]), None, TARGET, 0, C.byref(handle)))
    return handle, tables


def _raw_push(handle, wave, samples, sig, pcm):
    from eraxvif5tts_amd import _lib
    got = C.c_int64(-1)
    rc = _lib.load().f5_wave_stream_push(handle, len(samples), _lib.ptr(wave), (C.c_int32 * len(samples))(*samples), None, None, None, _lib.ptr(sig),
                                         _lib.ptr(pcm), C.byref(got), _lib.stream_ptr())
    return rc, got.value


def test_refusals_are_return_codes_and_leave_the_session_unchanged():
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.infer.utils_infer import WaveStream, finish_waves, plan_wave_tail
    lib = _lib.load()
    lengths = LENGTHS[:3]
    buf = _waves(lengths, seed=61)
    # a cross-fade longer than the utterances: the joints chain
    n = int(DURATIONS["longer_than_shortest"] * SR)
    assert not plan_wave_tail(lengths, DURATIONS["longer_than_shortest"], SR)["device_ok"]
    assert not WaveStream(lengths, DURATIONS["longer_than_shortest"], SR).ok
    handle, _tables = _raw_session(3, n)
    sig, pcm = torch.empty(sum(lengths), device="cuda", dtype=torch.float64), torch.empty(sum(lengths), device="cuda", dtype=torch.int16)
    rc, _ = _raw_push(handle, buf, lengths[:1], sig, pcm)
    assert rc == F5_ENOTSUP and "chain" in _lib.last_error()
    assert lib.f5_wave_stream_destroy(handle) == 0
    # n = 3600: the list is taken; a question first, then the same push with outputs, then one push too many
    d = 0.15
    want_sig, want_pcm = (t.cpu().numpy() for t in finish_waves(buf, lengths, d, SR, want_pcm16=True))
    handle, _tables = _raw_session(3, 3600)
    try:
        rc, count = _raw_push(handle, buf, lengths, None, None)
        assert rc == 0 and count == len(want_sig)
        rc, count = _raw_push(handle, None, lengths[:2], None, None)  # (a question needs no wave either)
        assert rc == 0 and count == plan_wave_tail(lengths, d, SR)["out_offsets"][2]
        assert _raw_push(handle, buf, [9000, 7700, 12000, 8000], None, None)[0] == F5_EINVAL  # more than the stream's total
        assert _raw_push(handle, buf, [9000, 0], None, None)[0] == F5_EINVAL
        assert _raw_push(handle, buf, [9000, 7000, 12000], None, None)[0] == F5_ENOTSUP  # an inner utterance below 2 n
        sig[:] = 0
        rc, count = _raw_push(handle, buf, lengths, sig, pcm)
        assert rc == 0 and count == len(want_sig)
        assert np.array_equal(sig[:count].cpu().numpy(), want_sig) and pcm[:count].cpu().numpy().tobytes() == want_pcm.tobytes()
        rc, _ = _raw_push(handle, buf, lengths[:1], sig, pcm)
        assert rc == F5_EINVAL and "left" in _lib.last_error()
    finally:
        assert lib.f5_wave_stream_destroy(handle) == 0
