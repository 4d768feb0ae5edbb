"""Output formats behind the wave tail (csrc/deliver.hip, include/f5hip.h ``f5_wave_convert`` / ``f5_wave_convert_stream_*`` /
``f5_op_g711_encode``): the finished 24 kHz signal at another sample rate, as float32, as the truncating int16 PCM of the wave tail, and as
G.711 mu-law / A-law -- one shot (`convert_wave`) or in pushes (`ConvertStream`) whose pieces, concatenated, are the one-shot bytes.

The resampler is torchaudio's ``sinc_interp_hann`` at its defaults, the definition ``f5_frontend_resample`` and ``oracle/cpu_ref.resample`` use.
Its tap table is computed HERE (`resample_taps_host`: float64 numpy, cast to fp32 and back as torchaudio casts its kernel to the waveform's dtype)
and handed to the library, which multiplies by exactly these doubles; the sums run on the device only -- there is no CPU resampler in this package,
a host array is uploaded once.  `g711_encode` is the host statement of the G.711 rule (CPython's ``audioop.lin2ulaw`` / ``lin2alaw`` for 16-bit
input) and the yardstick of the device encoder.
"""
from __future__ import annotations

import math

import numpy as np
import torch

ENCODINGS = ("pcm16", "mulaw", "alaw")
LAWS = {"mulaw": 0, "alaw": 1}  # the library's `law`; "pcm16" has none


def check_output_format(sample_rate, encoding, native_rate):
    """`F5TTSWrapper.set_output_format`'s arguments -> None (nothing set: ``sample_rate`` None or the native rate, ``encoding`` None or "pcm16")
    or ``(output rate, encoding)`` with the encoding spelled out.  Anything else raises ValueError."""
    if encoding is not None and (not isinstance(encoding, str) or encoding not in ENCODINGS):
        raise ValueError(f"encoding {encoding!r}: one of None, {', '.join(repr(e) for e in ENCODINGS)}")
    if sample_rate is not None and (isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or int(sample_rate) <= 0):
        raise ValueError(f"sample_rate {sample_rate!r}: None or a positive int")
    rate = int(native_rate) if sample_rate is None else int(sample_rate)
    encoding = encoding or "pcm16"
    if rate != int(native_rate):
        resample_plan(int(native_rate), rate)  # (a ratio whose table the library refuses is refused here, before any work)
    if rate == int(native_rate) and encoding == "pcm16":
        return None
    return rate, encoding


def g711_encode(pcm16, law):
    """int16 samples -> uint8 G.711 codes in numpy; ``law``: "mulaw" / 0 or "alaw" / 1.  ITU-T G.711 as ``audioop.lin2ulaw(b, 2)`` /
    ``audioop.lin2alaw(b, 2)`` implement it, in closed form (include/f5hip.h states both):
      mu-law  v = s >> 2, m = min(|v|, 8158) + 33, seg = floor(log2 m) - 5, code = seg << 4 | ((m >> (seg + 1)) & 15), ^ 0x7F for v < 0, else ^ 0xFF
      A-law   v = s >> 3, m = v or -v - 1 (v < 0), seg = 0 for m < 32 else floor(log2 m) - 4, code = seg << 4 | ((m >> (1 if seg < 2 else seg)) & 15),
              ^ 0x55 for v < 0, else ^ 0xD5"""
    law = LAWS.get(law, law)
    if law not in (0, 1):
        raise ValueError(f"law {law!r}: \"mulaw\" / 0 or \"alaw\" / 1")
    a = np.asarray(pcm16)
    if a.dtype != np.int16:
        raise ValueError(f"g711_encode takes int16 samples, not {a.dtype}")
    s = a.astype(np.int32)
    log2 = lambda m: np.frexp(m.astype(np.float64))[1].astype(np.int32) - 1  # noqa: E731  (floor(log2 m), exact for these integers)
    if law == 0:
        v = s >> 2
        m = np.minimum(np.abs(v), 8158) + 33
        seg = log2(m) - 5
        code = (seg << 4) | ((m >> (seg + 1)) & 15)
        return (code ^ np.where(v < 0, 0x7F, 0xFF)).astype(np.uint8)
    v = s >> 3
    m = np.where(v >= 0, v, -v - 1)
    seg = np.where(m < 32, 0, log2(np.maximum(m, 1)) - 4)
    code = (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 15)
    return (code ^ np.where(v < 0, 0x55, 0xD5)).astype(np.uint8)


def resample_plan(in_rate, out_rate):
    """``(orig, new, width, kw)`` of a conversion: the reduced rates, the half width of the filter in input samples and the taps per output phase
    (``2 * width + orig``).  ValueError for rates the library refuses: not positive, equal, or a table above 2^20 entries."""
    in_rate, out_rate = int(in_rate), int(out_rate)
    if in_rate <= 0 or out_rate <= 0 or in_rate == out_rate:
        raise ValueError(f"resampling {in_rate} -> {out_rate} Hz: two different positive rates")
    g = math.gcd(in_rate, out_rate)
    orig, new = in_rate // g, out_rate // g
    width = int(math.ceil(6.0 * orig / (min(orig, new) * 0.99)))
    kw = 2 * width + orig
    if new * kw > 1 << 20:
        raise ValueError(f"resampling {in_rate} -> {out_rate} Hz: a table of {new} x {kw} taps is beyond 2^20 entries")
    return orig, new, width, kw


def resample_taps_host(in_rate, out_rate):
    """The tap table [new][kw] in float64: torchaudio's ``_get_sinc_resample_kernel`` (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) in
    float64 numpy, cast to fp32 and back."""
    orig, new, width, kw = resample_plan(in_rate, out_rate)
    base = min(orig, new) * 0.99
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx
    t = np.clip(t * base, -6.0, 6.0)
    window = np.cos(t * math.pi / 6.0 / 2.0) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0.0, 1.0, np.sin(t) / t)
    h = sinc * (window * (base / orig))
    assert h.shape == (new, kw)
    return np.ascontiguousarray(h.astype(np.float32).astype(np.float64))


_taps = {}


def resample_taps(in_rate, out_rate, device=None):
    """`resample_taps_host` on the device, uploaded once per rate pair and device (the kernel multiplies by exactly these doubles)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (int(in_rate), int(out_rate), str(dev))
    if key not in _taps:
        _taps[key] = torch.from_numpy(resample_taps_host(in_rate, out_rate)).to(dev)
    return _taps[key]


def converted_length(n, in_rate, out_rate):
    """``ceil(new * n / orig)``: the samples a signal of ``n`` has at the other rate"""
    orig, new, _, _ = resample_plan(in_rate, out_rate)
    return -(-new * int(n) // orig)


def stream_convert_counts(lengths, in_rate, out_rate):
    """Output samples each push of a `ConvertStream` emits when a signal is pushed in consecutive pieces of these ``lengths`` (the last one is
    the final push), from the extents alone: after a non-final push that brings the input to N samples, ``new * max(0, (N - width) // orig)``
    samples are out in all -- the blocks whose whole support has arrived -- and the final push emits up to ``ceil(new * N / orig)``."""
    orig, new, width, _ = resample_plan(in_rate, out_rate)
    lengths = [int(x) for x in lengths]
    assert lengths and all(x > 0 for x in lengths)
    counts, taken, out = [], 0, 0
    for i, length in enumerate(lengths):
        taken += length
        upto = -(-new * taken // orig) if i == len(lengths) - 1 else new * max(0, (taken - width) // orig)
        counts.append(upto - out)
        out = upto
    return counts


def _device_signal(signal):
    """a finished signal -> a contiguous 1-D fp32 / fp64 tensor on the GPU (a host array -- the host tails -- is uploaded once)"""
    if not torch.is_tensor(signal):
        signal = torch.from_numpy(np.ascontiguousarray(np.asarray(signal).reshape(-1)))
    if signal.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"a signal is float32 or float64, not {signal.dtype}")
    if not signal.is_cuda:
        signal = signal.to(torch.device("cuda", torch.cuda.current_device()))
    return signal.reshape(-1).contiguous()


def _outputs(count, dev, encoding, want_float, want_codes):
    # (a zero-sized tensor has no address: one element at least, cut off by the caller)
    out = torch.empty(max(count, 1), device=dev, dtype=torch.float32) if want_float else None
    law = LAWS.get(encoding)
    codes = torch.empty(max(count, 1), device=dev, dtype=torch.int16 if law is None else torch.uint8) if want_codes else None
    return out, codes, law


def _check_encoding(encoding):
    encoding = encoding or "pcm16"
    if encoding not in ENCODINGS:
        raise ValueError(f"encoding {encoding!r}: one of None, {', '.join(repr(e) for e in ENCODINGS)}")
    return encoding


def g711_encode_device(pcm16, law):
    """``f5_op_g711_encode``: int16 on the GPU -> uint8 codes on the GPU (`g711_encode`'s rule)."""
    from .. import _lib
    law = LAWS.get(law, law)
    assert pcm16.is_cuda and pcm16.dtype == torch.int16
    flat = pcm16.reshape(-1).contiguous()
    out = torch.empty(flat.numel(), device=flat.device, dtype=torch.uint8)
    if flat.numel():
        _lib.check(_lib.load().f5_op_g711_encode(flat.numel(), _lib.ptr(flat), int(law), _lib.ptr(out), _lib.stream_ptr()), "op_g711_encode")
    return out


def convert_wave(signal, in_rate, out_rate, encoding=None, want_float=True, want_codes=False):
    """``f5_wave_convert``: a finished mono signal (fp32 / fp64; a GPU tensor, or a host array / CPU tensor that is uploaded once) at ``out_rate``
    -> ``(float32 signal, codes)`` as device tensors, None where not asked for.  ``codes``: int16 -- ``trunc(float32 * 32767)``, saturating, the
    wave tail's rule -- under ``encoding`` None / "pcm16", the uint8 G.711 codes of that int16 under "mulaw" / "alaw".  The rates differ (a caller
    that does not resample keeps its signal: ValueError)."""
    import ctypes as C

    from .. import _lib
    encoding = _check_encoding(encoding)
    resample_plan(in_rate, out_rate)
    assert want_float or want_codes
    x = _device_signal(signal)
    n = x.numel()
    count = converted_length(n, in_rate, out_rate)
    out, codes, law = _outputs(count, x.device, encoding, want_float, want_codes)
    if n:
        got = C.c_int64(0)
        taps = resample_taps(in_rate, out_rate, x.device)
        rc = _lib.load().f5_wave_convert(_lib.ptr(x), int(x.dtype == torch.float64), n, int(in_rate), int(out_rate), _lib.ptr(taps), int(law or 0),
                                         _lib.ptr(out), _lib.ptr(codes) if law is None else None, _lib.ptr(codes) if law is not None else None,
                                         C.byref(got), _lib.stream_ptr())
        _lib.check(rc, "wave_convert")
        assert got.value == count
    return (out[:count] if out is not None else None), (codes[:count] if codes is not None else None)


class ConvertStream:
    """`convert_wave` in consecutive pushes (``f5_wave_convert_stream_*``): ``push(signal, last)`` hands over the next samples of one signal --
    every piece in the dtype given at construction (``is_f64``: a property of the whole stream, as a `WaveStream`'s pieces have one dtype) -- and
    returns ``(float32, codes)`` device tensors holding what has become final (`stream_convert_counts`; possibly nothing).  The pieces,
    concatenated, are byte for byte `convert_wave` of the whole signal.  ``close()`` frees the session."""

    def __init__(self, in_rate, out_rate, encoding=None, is_f64=False, want_float=True, want_codes=False, device=None):
        import ctypes as C

        from .. import _lib
        self.encoding = _check_encoding(encoding)
        resample_plan(in_rate, out_rate)
        assert want_float or want_codes
        self.in_rate, self.out_rate, self.is_f64 = int(in_rate), int(out_rate), bool(is_f64)
        self.want_float, self.want_codes, self.finished, self._handle = want_float, want_codes, False, None
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._taps = resample_taps(in_rate, out_rate, self.device)  # (kept alive with the session, which reads it in every push)
        handle = C.c_void_p()
        _lib.check(_lib.load().f5_wave_convert_stream_create(self.in_rate, self.out_rate, _lib.ptr(self._taps), int(self.is_f64),
                                                             int(LAWS.get(self.encoding, 0)), C.byref(handle)), "wave_convert_stream_create")
        self._handle = handle

    def push(self, signal, last=False):
        import ctypes as C

        from .. import _lib
        lib = _lib.load()
        assert self._handle is not None and not self.finished, "the stream is closed or has had its last push"
        x = _device_signal(signal)
        assert (x.dtype == torch.float64) == self.is_f64, "every piece of a stream has the dtype given at construction"
        n = x.numel()
        if n == 0:  # (the library takes no empty push; nothing arrived, so nothing becomes final)
            if last:
                raise ValueError("the last push of a ConvertStream holds at least one sample")
            out, codes, _ = _outputs(0, self.device, self.encoding, self.want_float, self.want_codes)
            return (out[:0] if out is not None else None), (codes[:0] if codes is not None else None)
        got = C.c_int64(0)
        _lib.check(lib.f5_wave_convert_stream_push(self._handle, None, n, int(bool(last)), None, None, None, C.byref(got), None),
                   "wave_convert_stream_push")
        count = got.value
        out, codes, law = _outputs(count, x.device, self.encoding, self.want_float, self.want_codes)
        _lib.check(lib.f5_wave_convert_stream_push(self._handle, _lib.ptr(x), n, int(bool(last)), _lib.ptr(out),
                                                   _lib.ptr(codes) if law is None else None, _lib.ptr(codes) if law is not None else None,
                                                   C.byref(got), _lib.stream_ptr()), "wave_convert_stream_push")
        assert got.value == count
        self.finished = bool(last)
        return (out[:count] if out is not None else None), (codes[:count] if codes is not None else None)

    def close(self):
        if self._handle is not None:
            from .. import _lib
            _lib.load().f5_wave_convert_stream_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass
