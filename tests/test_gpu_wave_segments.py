"""The segmented wave tail (`f5_wave_finish_segments`, `f5_wave_stream_create_segments`; `utils_infer.finish_waves` / `WaveStream` with
``segments`` and ``rms_index``) at op level.  Acceptance is exactness.  The oracle is the host route of a script in several voices: per
utterance torch's ``w * rms / target`` on the GPU tensor where ``rms < target``, `cross_fade_concat` per segment in numpy, `np.concatenate`
of the segments, and `streaming.wire.pcm16_bytes` of that array -- float (dtype included) and PCM byte-equal.  The waves are random with
|x| < 1.2, so some samples saturate; the cross-fade is 16 samples and the lengths come from {16, 32, 33, 100, 257} within the chaining rule.

Where a product reaches +-32768 numpy's cast to int16 is undefined (`pcm16_bytes` may wrap) and `f5_wave_finish` documents
saturation instead, as `test_wave_finish_many_utterances_and_saturation` pins it.  The PCM oracle here is therefore `pcm16_bytes` on every
sample whose product lies inside int16 -- checked against `pcm16_bytes` itself -- and the documented saturated value on the others; every
sample is compared, none is left out."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_generate_stream_host import compositions

pytestmark = pytest.mark.gpu
F5_EINVAL, F5_ENOTSUP = -1, -5  # include/f5hip.h
SR, N, TARGET = 24000, 16, 0.1
D = N / SR + 1e-9  # int(D * SR) == 16
CHOICES = [16, 32, 33, 100, 257]
VOICE_RMS = [0.05, 0.1, 0.3]  # against target 0.1: applied, not applied at equality, not applied


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _seg_start(seg_sizes):
    return [1 if i == 0 else 0 for g in seg_sizes for i in range(g)]


def _lengths(seg_sizes, seed):
    """drawn from CHOICES; where the chaining rule asks for n or 2 n samples, from the choices that hold them"""
    g, start = np.random.default_rng(seed), _seg_start(seg_sizes)
    out = []
    for k in range(len(start)):
        need = N * ((0 if start[k] else 1) + (1 if k + 1 < len(start) and not start[k + 1] else 0))
        out.append(int(g.choice([c for c in CHOICES if c >= need])))
    return out


def _waves(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(sum(lengths), generator=g) * 2 - 1) * 1.2).cuda()


def _oracle(buf, lengths, seg_sizes, d, rms=None):
    """``rms``: None, or one value per utterance (Python numbers, or 0-dim fp32 GPU tensors as a prompt's rms is)"""
    from eraxvif5tts_amd.infer.utils_infer import cross_fade_concat
    waves = []
    for i, w in enumerate(torch.split(buf, lengths)):
        if rms is not None and rms[i] < TARGET:
            w = w * rms[i] / TARGET
        waves.append(w.cpu().numpy())
    parts, k = [], 0
    for g in seg_sizes:
        parts.append(cross_fade_concat(waves[k: k + g], d, SR))
        k += g
    return np.concatenate(parts), parts


def _pcm(ref):
    """`pcm16_bytes(ref)` as an int16 array, with the products outside int16 (numpy: undefined) saturated as the library documents"""
    from eraxvif5tts_amd.streaming.wire import pcm16_bytes
    product = np.asarray(ref) * 32767  # in the array's own precision, as pcm16_bytes multiplies
    inside = (product > -32768) & (product < 32768)
    want = np.clip(product, -32768, 32767).astype(np.int16)
    assert np.array_equal(want[inside], np.frombuffer(pcm16_bytes(ref), np.int16)[inside])
    return want


def _check(done, ref):
    assert done is not None
    sig, pcm = done[0].cpu().numpy(), done[1].cpu().numpy()
    assert sig.dtype == ref.dtype and sig.shape == ref.shape and np.array_equal(sig, ref)
    assert pcm.dtype == np.int16 and pcm.tobytes() == _pcm(ref).tobytes()


@pytest.mark.parametrize("seg_sizes", [[1], [1, 1], [2], [1, 2], [2, 1], [3, 1, 2]], ids=str)
def test_segments_equal_the_host_functions_byte_for_byte(seg_sizes):
    from eraxvif5tts_amd.infer.utils_infer import finish_waves, plan_wave_tail_segments
    for seed in range(3):
        lengths = _lengths(seg_sizes, seed * 11 + len(seg_sizes))
        buf = _waves(lengths, seed)
        assert float(buf.abs().max()) > 1.0  # some products saturate
        ref, _ = _oracle(buf, lengths, seg_sizes, D)
        assert (ref.dtype == np.float32) == (max(seg_sizes) == 1)
        plan = plan_wave_tail_segments(lengths, seg_sizes, D, SR)
        assert plan["device_ok"] and plan["total"] == len(ref)
        _check(finish_waves(buf, lengths, D, SR, want_pcm16=True, segments=seg_sizes), ref)
        # cross-fade off: every list is plain concatenation in float32
        ref0, _ = _oracle(buf, lengths, seg_sizes, 0.0)
        assert ref0.dtype == np.float32
        _check(finish_waves(buf, lengths, 0.0, SR, want_pcm16=True, segments=seg_sizes), ref0)


@pytest.mark.parametrize("boundary", [62, 63, 64, 65])
def test_a_segment_boundary_at_the_table_split(boundary):
    """70 utterances: the kernel tables hold 64 and overlap by one (utterance 63), so the boundary falls before, on and behind the overlap"""
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    seg_sizes = [boundary, 70 - boundary]
    lengths = _lengths(seg_sizes, boundary)
    buf = _waves(lengths, boundary)
    index = [k % 3 for k in range(70)]
    vec = torch.tensor(VOICE_RMS, device="cuda")
    ref, _ = _oracle(buf, lengths, seg_sizes, D, rms=[vec[i] for i in index])
    assert ref.dtype == np.float64 and len(ref) == sum(lengths) - N * 68
    _check(finish_waves(buf, lengths, D, SR, rms=vec, target_rms=TARGET, want_pcm16=True, segments=seg_sizes, rms_index=index), ref)


def test_three_voices_on_the_device_and_on_the_host():
    """rms 0.05 / 0.1 / 0.3 against target 0.1: the gain applied, not applied at equality, not applied -- decided in the kernel from the
    device vector, with the left operand of a joint taking the left utterance's voice; the host form gives the same bytes"""
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    seg_sizes, index = [3, 1, 2, 2], [0, 1, 2, 0, 1, 0, 2, 2]
    lengths = _lengths(seg_sizes, 5)
    buf = _waves(lengths, 5)
    vec = torch.tensor(VOICE_RMS, device="cuda")
    ref, _ = _oracle(buf, lengths, seg_sizes, D, rms=[vec[i] for i in index])
    plain, _ = _oracle(buf, lengths, seg_sizes, D)
    assert not np.array_equal(ref, plain)
    dev = finish_waves(buf, lengths, D, SR, rms=vec, target_rms=TARGET, want_pcm16=True, segments=seg_sizes, rms_index=index)
    _check(dev, ref)
    host = finish_waves(buf, lengths, D, SR, rms=[VOICE_RMS[i] for i in index], target_rms=TARGET, want_pcm16=True, segments=seg_sizes)
    assert torch.equal(host[0], dev[0]) and torch.equal(host[1], dev[1])
    # one voice for all, through the index: the scalar form's bytes
    for voice in range(3):
        one = finish_waves(buf, lengths, D, SR, rms=vec, target_rms=TARGET, want_pcm16=True, segments=seg_sizes, rms_index=[voice] * 8)
        scalar = finish_waves(buf, lengths, D, SR, rms=vec[voice].clone(), target_rms=TARGET, want_pcm16=True, segments=seg_sizes)
        assert torch.equal(one[0], scalar[0]) and torch.equal(one[1], scalar[1])
    with pytest.raises(AssertionError):
        finish_waves(buf, lengths, D, SR, rms=vec, target_rms=TARGET, segments=seg_sizes, rms_index=[3] * 8)


def test_utterances_exactly_at_the_rule():
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    seg_sizes, lengths = [3, 2, 1], [N, 2 * N, N, N, N, 5]  # ends of exactly n, an inner one of exactly 2 n: every sample of those is mixed
    buf = _waves(lengths, 8)
    ref, _ = _oracle(buf, lengths, seg_sizes, D)
    assert len(ref) == 2 * N + N + 5
    _check(finish_waves(buf, lengths, D, SR, want_pcm16=True, segments=seg_sizes), ref)


def _raw_finish(buf, lengths, seg_start, n, rms_dev=None, n_rms=0, index=None, pcm_f32=None):
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.infer.utils_infer import _xfade_weights
    B = len(lengths)
    down, up = _xfade_weights(n, buf.device) if n > 0 else (None, None)
    out = torch.zeros(sum(lengths), device="cuda", dtype=torch.float64)
    got = C.c_int64(-1)
    rc = _lib.load().f5_wave_finish_segments(B, _lib.ptr(buf), (C.c_int32 * B)(*lengths), (C.c_uint8 * B)(*seg_start) if seg_start else None, None,
                                             None, _lib.ptr(rms_dev), n_rms, (C.c_int32 * B)(*index) if index else None, TARGET, 0, n,
                                             _lib.ptr(down), _lib.ptr(up), (C.c_uint8 * B)(*pcm_f32) if pcm_f32 else None, None, _lib.ptr(out),
                                             None, C.byref(got), _lib.stream_ptr())
    return rc, got.value, out


def _raw_finish_plain(buf, lengths, n, rms):
    """`f5_wave_finish` itself, the entry point without segments -> (signal, pcm); ``rms``: None, a 0-dim fp32 GPU tensor, or one host value per
    utterance (the decision taken as `_oracle` takes it)"""
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.infer.utils_infer import _xfade_weights
    B, mixed = len(lengths), n > 0
    down, up = _xfade_weights(n, buf.device) if mixed else (None, None)
    gains = applies = rms_dev = None
    if torch.is_tensor(rms):
        rms_dev = rms
    elif rms is not None:
        gains, applies = (C.c_float * B)(*rms), (C.c_uint8 * B)(*[1 if r < TARGET else 0 for r in rms])
    total = sum(lengths) - n * (B - 1)
    out = torch.zeros(total, device="cuda", dtype=torch.float64 if mixed else torch.float32)
    pcm = torch.zeros(total, device="cuda", dtype=torch.int16)
    got = C.c_int64(-1)
    rc = _lib.load().f5_wave_finish(B, _lib.ptr(buf), (C.c_int32 * B)(*lengths), gains, applies, _lib.ptr(rms_dev), TARGET, 0, n, _lib.ptr(down),
                                    _lib.ptr(up), None if mixed else _lib.ptr(out), _lib.ptr(out) if mixed else None, _lib.ptr(pcm),
                                    C.byref(got), _lib.stream_ptr())
    assert rc == 0 and got.value == total
    return out, pcm


def test_refusals():
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.infer.utils_infer import finish_waves, plan_wave_tail_segments
    lengths = [33, 2 * N - 1, 33, 100, 100]
    buf = _waves(lengths, 9)
    # an inner utterance of 2 n - 1 samples: the joints chain
    assert not plan_wave_tail_segments(lengths, [3, 2], D, SR)["device_ok"]
    assert finish_waves(buf, lengths, D, SR, segments=[3, 2]) is None
    rc, _, _ = _raw_finish(buf, lengths, [1, 0, 0, 1, 0], N)
    assert rc == F5_ENOTSUP and "utterance 1 " in _lib.last_error() and "chain" in _lib.last_error()
    # the same length as a segment of its own is taken
    ref, _ = _oracle(buf, lengths, [1, 1, 1, 2], D)
    _check(finish_waves(buf, lengths, D, SR, want_pcm16=True, segments=[1, 1, 1, 2]), ref)
    rc, total, out = _raw_finish(buf, lengths, [1, 1, 1, 1, 0], N)
    assert rc == 0 and total == sum(lengths) - N and np.array_equal(out[:total].cpu().numpy(), ref)
    # an end utterance below n
    assert finish_waves(buf, [33, 100, N - 1, 100, 49], D, SR, segments=[1, 2, 2]) is None
    # arguments
    vec = torch.tensor(VOICE_RMS, device="cuda")
    assert _raw_finish(buf, lengths, [1, 1, 1, 1, 0], N, rms_dev=vec, n_rms=3, index=[0, 1, 2, 3, 0])[0] == F5_EINVAL
    assert _raw_finish(buf, lengths, [1, 1, 1, 1, 0], N, rms_dev=vec, n_rms=0)[0] == F5_EINVAL
    assert _raw_finish(buf, lengths, [1, 1, 1, 1, 0], N, pcm_f32=[0, 0, 0, 1, 0])[0] == F5_EINVAL  # a flag for a segment of one only
    assert _raw_finish(buf, lengths, [1, 1, 1, 1, 0], N, pcm_f32=[1, 1, 1, 0, 0])[0] == 0


def test_one_segment_is_the_existing_entry_point():
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    lengths = [257, 100, 33, 100, 32]
    buf = _waves(lengths, 10)
    for d in (D, 0.0):
        for rms in (None, torch.tensor(0.07, device="cuda"), [0.05, 0.2, 0.0999, 0.1, 0.03]):
            old = _raw_finish_plain(buf, lengths, int(d * SR), rms)  # (`finish_waves` always takes the segmented entry point)
            new = finish_waves(buf, lengths, d, SR, rms=rms, target_rms=TARGET, want_pcm16=True, segments=[5])
            assert old[0].dtype == new[0].dtype and torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    rc, total, out = _raw_finish(buf, lengths, None, N)  # no array at all: one segment
    old = finish_waves(buf, lengths, D, SR)
    assert rc == 0 and total == old[0].numel() and torch.equal(out[:total], old[0])


def test_a_segment_of_one_can_keep_the_pcm_of_its_own_call():
    """`pcm_f32`: inside a float64 result the flagged one-utterance segments carry trunc(fp32(x * 32767)) -- what a call over that utterance
    alone gives, and what concatenating per-piece results needs -- where the default is `pcm16_bytes` of the float64 array; the two differ"""
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    from eraxvif5tts_amd.streaming.wire import pcm16_bytes
    seg_sizes, lengths = [1, 2, 1], [60000, 100, 257, 60000]
    buf = _waves(lengths, 12) * 0.8
    ref, parts = _oracle(buf, lengths, seg_sizes, D)
    own = np.concatenate([np.frombuffer(pcm16_bytes(p), np.int16) for p in parts])
    assert ref.dtype == np.float64 and parts[0].dtype == np.float32 and own.tobytes() != pcm16_bytes(ref)
    sig, pcm = finish_waves(buf, lengths, D, SR, want_pcm16=True, segments=seg_sizes, pcm_f32=[True, False, False, True])
    assert np.array_equal(sig.cpu().numpy(), ref) and pcm.cpu().numpy().tobytes() == own.tobytes()
    _check(finish_waves(buf, lengths, D, SR, want_pcm16=True, segments=seg_sizes), ref)


# ---------------------------------------------------------------------------------------------------------------- stream
STREAM_SEGS = [3, 1, 2]
STREAM_INDEX = [0, 1, 1, 2, 0, 2]


def _push_all(buf, lengths, sizes, d, counts, **kw):
    from eraxvif5tts_amd.infer.utils_infer import WaveStream
    ws = WaveStream(lengths, d, SR, target_rms=TARGET, want_float=True, want_pcm16=True, segments=STREAM_SEGS, **kw)
    assert ws.ok
    sigs, pcms, k, at = [], [], 0, 0
    try:
        for i, size in enumerate(sizes):
            samples = lengths[k: k + size]
            wave = buf[at: at + sum(samples)].clone()
            sig, pcm = ws.push(wave, samples)
            wave.fill_(float("nan"))  # same stream, behind the push: the carry must not live in the caller's buffer
            assert sig.numel() == pcm.numel() == counts[i]
            sigs.append(sig)
            pcms.append(pcm)
            k, at = k + size, at + sum(samples)
        return [s.cpu().numpy() for s in sigs], [p.cpu().numpy() for p in pcms]
    finally:
        ws.close()


@pytest.mark.parametrize("form", ["device_vector", "host_list", "own_pcm", "xfade_off"])
def test_every_cut_of_a_segmented_list_gives_the_one_shot_bytes(form):
    from eraxvif5tts_amd.infer.utils_infer import finish_waves, stream_emitted_counts
    lengths = _lengths(STREAM_SEGS, 21)
    buf = _waves(lengths, 21)
    d = 0.0 if form == "xfade_off" else D
    kw = {"device_vector": dict(rms=torch.tensor(VOICE_RMS, device="cuda"), rms_index=STREAM_INDEX),
          "host_list": dict(rms=[VOICE_RMS[i] for i in STREAM_INDEX]),
          "own_pcm": dict(rms=torch.tensor(VOICE_RMS, device="cuda"), rms_index=STREAM_INDEX, pcm_f32=[0, 0, 0, 1, 0, 0]),
          "xfade_off": dict(rms=torch.tensor(VOICE_RMS, device="cuda"), rms_index=STREAM_INDEX)}[form]
    want_sig, want_pcm = (t.cpu().numpy() for t in finish_waves(buf, lengths, d, SR, target_rms=TARGET, want_pcm16=True, segments=STREAM_SEGS, **kw))
    vec = torch.tensor(VOICE_RMS, device="cuda")
    ref, _ = _oracle(buf, lengths, STREAM_SEGS, d, rms=[vec[i] for i in STREAM_INDEX])
    assert np.array_equal(want_sig, ref) and want_sig.dtype == ref.dtype == (np.float32 if form == "xfade_off" else np.float64)
    cuts = compositions(6)
    assert len(cuts) == 32
    for sizes in cuts:
        counts, dtype = stream_emitted_counts(lengths, sizes, d, SR, segments=STREAM_SEGS)
        sigs, pcms = _push_all(buf, lengths, sizes, d, counts, **kw)
        assert all(s.dtype == dtype == want_sig.dtype for s in sigs), sizes
        assert np.array_equal(np.concatenate(sigs), want_sig), sizes
        assert np.concatenate(pcms).tobytes() == want_pcm.tobytes(), sizes


def test_a_question_leaves_the_session_unchanged():
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.infer.utils_infer import _xfade_weights, finish_waves, plan_wave_tail_segments
    lib = _lib.load()
    lengths = _lengths(STREAM_SEGS, 22)
    buf = _waves(lengths, 22)
    want = finish_waves(buf, lengths, D, SR, segments=STREAM_SEGS)[0]
    offsets = plan_wave_tail_segments(lengths, STREAM_SEGS, D, SR)["out_offsets"] + [want.numel()]
    down, up = _xfade_weights(N, buf.device)
    handle = C.c_void_p()
    _lib.check(lib.f5_wave_stream_create_segments(6, (C.c_uint8 * 6)(*_seg_start(STREAM_SEGS)), N, _lib.ptr(down), _lib.ptr(up), None, 0, None, TARGET,
                                                  0, None, C.byref(handle)))

    def push(first, count, out):
        samples, got = lengths[first: first + count], C.c_int64(-1)
        wave = buf[sum(lengths[:first]): sum(lengths[: first + count])].clone() if out is not None else None
        rc = lib.f5_wave_stream_push(handle, count, _lib.ptr(wave), (C.c_int32 * count)(*samples), None, None, None, _lib.ptr(out), None,
                                     C.byref(got), _lib.stream_ptr())
        return rc, got.value
    try:
        out = torch.zeros(want.numel(), device="cuda", dtype=torch.float64)
        for count in (6, 1, 3, 4, 2, 2):  # questions, again and again: always answered for the list's first utterances
            assert push(0, count, None) == (0, offsets[count])
        assert push(0, 2, out) == (0, offsets[2])
        assert push(2, 1, None) == (0, offsets[3] - offsets[2]) and push(2, 4, None) == (0, offsets[6] - offsets[2])
        assert push(2, 1, out[offsets[2]:]) == (0, offsets[3] - offsets[2])  # ends the first segment: all of it, nothing carried
        assert push(3, 2, None) == (0, offsets[5] - offsets[3])
        assert push(3, 3, out[offsets[3]:]) == (0, offsets[6] - offsets[3])
        assert torch.equal(out, want)
        assert push(0, 1, out)[0] == F5_EINVAL and "left" in _lib.last_error()
    finally:
        assert lib.f5_wave_stream_destroy(handle) == 0
