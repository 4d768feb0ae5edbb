"""The two audio ends of the pipeline at every configuration their create() calls accept, against float64 oracles: the prompt front-end
(csrc/frontend.hip: log-mel of either type, sample-rate conversion) and the Vocos vocoder (csrc/vocoder.hip, csrc/vocos.hip: ISTFT head by FFT
and by the dense inverse-DFT GEMM, other n_fft / hop / n_mels / widths, a caller's window, the NOLA refusal).  Every case is a few frames.

Mel inputs (audio_cases.mel_wave): a batch of two, row 0 a 300 Hz sine plus noise, row 1 zeros with impulses at samples 0, 1, nw // 2, nw - 2,
nw - 1, which make an off-by-one of the reflect map an O(1) error (test_audio_oracles_host.py shows that three wrong variants of the oracle miss
the bounds below by a factor of 10 or more, and that 70.6 % - 100 % of the bins of every case are strong).

Mel bounds.  Per case, audio_cases.mel_fp32_emulation restates the kernel in float32 on the CPU (frames and windowed DFT matrix rounded to
float32, sequential float32 accumulation over n, float32 magnitude, float32 filterbank product, float32 log); its error against
cpu_ref.mel_spectrogram_f64 is measured as max |d log-mel| on the strong bins (oracle above log 1e-4), rel-L2 of the linear mel over all bins and
max |d log-mel| over all bins.  The bound for the device is 8 x that, rounded up to one significant digit, never looser than the old 2e-3 / 1e-4
(and 0.2 / 5e-2 over all bins).  The factor 8 covers what a CPU cannot measure: the MFMA's accumulation order (chains of 4-term blocks instead
of one sequential sum) and a few ulps of the device's sqrtf / logf.  No bound was set from, or widened after, what the device returned.

    mel type, n_fft/hop/win, n_mels, rate, nw (T)        emulation: strong   rel-L2    all      bound: strong  rel-L2  all
    vocos   1024/256/1024 100 24000    513  (3)                     1.76e-06 5.04e-07 1.76e-06          2e-05   5e-06   2e-05
    vocos   1024/256/1024 100 24000   2048  (9)                     6.28e-06 4.00e-07 6.28e-06          6e-05   4e-06   6e-05
    vocos    512/128/400   80 16000   1300 (11)                     5.97e-06 2.99e-07 5.97e-06          5e-05   3e-06   5e-05
    vocos   2048/512/1200 128 44100   5000 (10)                     1.87e-05 3.98e-07 1.87e-05          2e-04   4e-06   2e-04
    vocos   1024/256/640  100 24000   1025  (5)                     1.48e-05 2.57e-07 1.48e-05          2e-04   3e-06   2e-04
    vocos   1024/300/1024 100 22050   4000 (14)                     1.21e-05 3.63e-07 1.21e-05          1e-04   3e-06   1e-04
    vocos   1024/256/1024 100 24000  15872 (63), batch 1            1.37e-05 3.63e-07 1.37e-05          2e-04   3e-06   2e-04
    vocos   1024/256/1024 100 24000  16128 (64), batch 1            1.08e-05 3.67e-07 1.08e-05          9e-05   3e-06   9e-05
    vocos   1024/256/1024 100 24000  16384 (65), batch 1            2.51e-05 3.62e-07 2.51e-05          3e-04   3e-06   3e-04
    bigvgan 1024/256/1024 100 24000    385  (1)                     1.24e-06 3.07e-07 1.24e-06          1e-05   3e-06   1e-05
    bigvgan 1024/256/1024 100 24000   2048  (8)                     1.44e-05 3.52e-07 1.44e-05          2e-04   3e-06   2e-04
    bigvgan 1024/255/1024 100 24000   3000 (11)                     6.66e-06 3.94e-07 6.66e-06          6e-05   4e-06   6e-05
    bigvgan  512/128/400   80 16000   1300 (10)                     6.92e-06 2.48e-07 6.92e-06          6e-05   2e-06   6e-05

(In every case the largest error sits on a strong bin: the weak bins of row 1 are frames the impulses do not reach, exactly the floor on both
sides.)  The workspace-regrowth test derives its bounds from the same emulation at run time, by the same rule.  One thing the emulation
shares with the oracle and the device does not: the HTK filterbank.  frontend.hip builds it with float32 scalar arithmetic, the oracle with
torch.linspace; the band edges are float32 values of some kHz whose differences are tens of Hz, so a last-bit difference in an edge moves a
weight by 1e-5 (rel-L2 between the two tables, restated on the CPU: 3e-6 - 7e-6).  That is inside the rel-L2 bounds, and is most of what the
device shows there for the vocos type; the Slaney table of the bigvgan type is float64 arithmetic on both sides.

The other tolerances are the project's own: resampling rel-L2 <= 1e-5 against cpu_ref.resample (float64), and max error <= 1e-6 max |ref| for
outputs of at most 40 samples; ISTFT head rel-L2 <= 1e-5 against cpu_ref.head_to_wave_f64; Vocos decode rel-L2 <= 1e-4 against
cpu_ref.vocos_decode; a ragged decode equals every utterance's own decode bit for bit (the contract stated in vocoder.hip)."""
import ctypes as C
import math

import pytest
import torch

import audio_cases as A
from conftest import rel_l2
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

IDS = [A.mel_case_id(c) for c in A.ALL_MEL_CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _melspec(case):
    from eraxvif5tts_amd.model.modules import MelSpec
    mt, b, n_fft, hop, win, n_mels, sr, nw = case
    return MelSpec(n_fft=n_fft, hop_length=hop, win_length=win, n_mel_channels=n_mels, target_sample_rate=sr, mel_spec_type=mt)


def _check_mel(case, out, ref, bounds):
    err = A.mel_errors(out, ref)
    print(f"{A.mel_case_id(case)}: device strong {err[0]:.2e} rel-L2 {err[1]:.2e} all {err[2]:.2e}   bounds {bounds}")
    assert torch.isfinite(out).all() and (out >= math.log(1e-5) - 1e-6).all()
    assert err[0] <= bounds[0] and err[1] <= bounds[1] and err[2] <= bounds[2], (err, bounds)


# ----------------------------------------------------------------------------- log-mel
@pytest.mark.parametrize("case", A.ALL_MEL_CASES, ids=IDS)
def test_mel_matches_the_f64_oracle(case):
    mt, b, n_fft, hop, win, n_mels, sr, nw = case
    wav, ref = A.mel_case_data(case)
    ms = _melspec(case)
    out = ms(wav.cuda()).cpu()
    assert out.dtype == torch.float32 and out.shape == ref.shape == (b, n_mels, ms.frame_count(nw))
    _check_mel(case, out, ref, A.MEL_BOUNDS[case])


@pytest.mark.parametrize("case", [A.ALL_MEL_CASES[2], A.ALL_MEL_CASES[-2]], ids=[IDS[2], IDS[-2]])
def test_mel_wrapper_takes_a_channel_axis_and_fp16(case):
    """a [b, 1, nw] waveform and an fp16 waveform give what the plain call gives, in the waveform's dtype"""
    wav, _ = A.mel_case_data(case)
    ms = _melspec(case)
    plain = ms(wav.cuda())
    assert torch.equal(ms(wav[:, None, :].cuda()), plain)
    half = ms(wav.half().cuda())
    assert half.dtype == torch.float16 and half.shape == plain.shape
    assert torch.equal(half, ms(wav.half().float().cuda()).half())


@pytest.mark.parametrize("mel_type,nw", [("vocos", 512), ("bigvgan", 384)])
def test_mel_refuses_a_wave_of_pad_samples(mel_type, nw):
    """nw == pad: one sample short of what reflect padding needs.  F5HipError through the wrapper; at the C ABI an error code and an untouched output."""
    from eraxvif5tts_amd import _lib, frontend
    from eraxvif5tts_amd.model.modules import MelSpec
    wav = A.mel_wave(nw, 24000).cuda()
    with pytest.raises(_lib.F5HipError):
        MelSpec(mel_spec_type=mel_type)(wav)
    h = frontend._handle(0, 1024, 256, 1024, 100, 24000, {"vocos": _lib.F5_MEL_VOCOS, "bigvgan": _lib.F5_MEL_BIGVGAN}[mel_type])
    out = torch.full((2, 100, 4), 7.5, device="cuda")
    with torch.cuda.device(0):
        rc = _lib.load().f5_frontend_mel(h, 2, nw, _lib.ptr(wav), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and (out == 7.5).all()
    # one sample more is accepted
    assert MelSpec(mel_spec_type=mel_type)(A.mel_wave(nw + 1, 24000).cuda()).shape == (2, 100, 3 if mel_type == "vocos" else 1)


@pytest.mark.parametrize("n_fft,win", [(1000, 1000), (1024, 1025)])
def test_mel_refuses_a_bad_config(n_fft, win):
    """n_fft not a multiple of 32, win > n_fft: f5_frontend_create fails, no handle comes back and no mel is computed"""
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.model.modules import MelSpec
    with pytest.raises(_lib.F5HipError):
        MelSpec(n_fft=n_fft, win_length=win)(A.mel_wave(2048, 24000).cuda())
    cfg = _lib.MelConfig(n_fft=n_fft, hop=256, win=win, n_mels=100, sample_rate=24000, mel_type=_lib.F5_MEL_VOCOS)
    h = C.c_void_p()
    assert _lib.load().f5_frontend_create(C.byref(cfg), C.byref(h)) != 0 and not h.value


def test_mel_workspace_regrowth():
    """One handle (a config no other test uses, so its workspace starts empty): 3 frames, 200 frames x 2, 3 frames, 400 frames -- the workspace is
    released and reallocated twice and reused smaller once; a stale pointer or row count shows in the results."""
    from eraxvif5tts_amd.model.modules import MelSpec
    ms = MelSpec(n_fft=512, hop_length=100, win_length=512, n_mel_channels=64, target_sample_rate=16000)
    for b, nw in ((1, 280), (2, 19950), (1, 280), (1, 39920)):
        case = ("vocos", b, 512, 100, 512, 64, 16000, nw)
        wav, ref = A.mel_case_data(case)
        out = ms(wav.cuda()).cpu()
        assert out.shape == ref.shape == (b, 64, nw // 100 + 1)
        _check_mel(case, out, ref, A.bounds_from_error(A.emulation_error(case), "vocos"))


# ----------------------------------------------------------------------------- sample-rate conversion
def _resample_input(rows, n, orig, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / orig
    return torch.stack([(0.5 - 0.1 * r) * torch.sin(2 * math.pi * (440 + 130 * r) * t + r) + 0.1 * torch.randn(n, generator=g) for r in range(rows)])


def _check_resample(out, ref, what):
    err, peak = rel_l2(out, ref), float((out.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))
    print(f"resample {what}: rel-L2 {err:.2e}, max error / max |ref| {peak:.2e}")
    assert out.dtype == torch.float32 and out.shape == ref.shape
    assert err <= 1e-5
    if ref.shape[-1] <= 40:
        assert peak <= 1e-6


RESAMPLE_CASES = [(8000, 24000, 1), (8000, 24000, 5), (8000, 24000, 100), (11025, 24000, 13), (11025, 24000, 1000), (32000, 24000, 7),
                  (32000, 24000, 1000), (96000, 24000, 3), (96000, 24000, 50), (96000, 24000, 1000),
                  (44100, 24000, 1), (44100, 24000, 171), (44100, 24000, 172),  # 147 -> 80: 171 taps, the window just inside / just past the signal
                  (24000, 16000, 100)]


@pytest.mark.parametrize("orig,new,n", RESAMPLE_CASES)
def test_resample_matches_oracle(orig, new, n):
    from eraxvif5tts_amd import frontend
    wav = _resample_input(3, n, orig, seed=orig + n)
    ref = cpu_ref.resample(wav, orig, new)
    g = math.gcd(orig, new)
    assert ref.shape == (3, -(-(new // g) * n // (orig // g)))
    _check_resample(frontend.resample(wav.cuda(), orig, new).cpu(), ref, f"{orig} -> {new}, n = {n}")


@pytest.mark.parametrize("orig,new,n", [(44100, 24000, 172), (8000, 24000, 5), (96000, 24000, 50)])
def test_resample_edge_impulses(orig, new, n):
    """impulses at samples 0 and n - 1 only: every output is one tap of the filter, placed by the zero-padding guards"""
    from eraxvif5tts_amd import frontend
    wav = torch.zeros(3, n)
    wav[0, 0], wav[1, n - 1] = 1.0, -0.7
    wav[2, 0], wav[2, n - 1] = 0.5, 0.25
    ref = cpu_ref.resample(wav, orig, new)
    out = frontend.resample(wav.cuda(), orig, new).cpu()
    _check_resample(out, ref, f"{orig} -> {new}, n = {n}, edge impulses")
    assert float((out.double() - ref.double()).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_resample_keeps_leading_axes():
    from eraxvif5tts_amd import frontend
    n = 333
    wav = _resample_input(6, n, 11025, seed=9).reshape(2, 3, n)
    ref = cpu_ref.resample(wav, 11025, 24000)
    out = frontend.resample(wav.cuda(), 11025, 24000).cpu()
    assert out.shape == ref.shape == (2, 3, math.ceil(320 * n / 147))
    _check_resample(out, ref, "[2, 3, 333] 11025 -> 24000")
    assert frontend.resample(wav.half().cuda(), 11025, 24000).dtype == torch.float16


# ----------------------------------------------------------------------------- ISTFT head
_heads = {}


def _head_vocos(n_fft, hop, window=None):
    """a Vocos with a one-layer 64-wide backbone (the head tests use only its ISTFT), one per (n_fft, hop, window)"""
    from eraxvif5tts_amd.vocos import Vocos
    key = (n_fft, hop, window)
    if key not in _heads:
        v = Vocos(n_mels=8, dim=64, intermediate_dim=128, num_layers=1, n_fft=n_fft, hop_length=hop)
        if window == "hamming":
            v.load_state_dict({"head.istft.window": torch.hamming_window(n_fft)}, strict=False)
        _heads[key] = v.cuda()
    return _heads[key]


def _check_head(voc, n_fft, hop, T, window, what):
    head = A.random_head(2, T, n_fft, seed=n_fft + hop + T)
    ref = cpu_ref.head_to_wave_f64(head, n_fft, hop, window)
    out = voc.istft_head(head.cuda()).cpu()
    err = rel_l2(out, ref)
    print(f"istft head {what} n_fft {n_fft} hop {hop} T {T}: rel-L2 {err:.2e}")
    assert out.shape == ref.shape == (2, (T - 1) * hop) and torch.isfinite(out).all()
    assert err <= 1e-5


def _dense(fn):
    import gpu_helpers as G
    with G.knobs(vocos_fft=0):
        fn()


@pytest.mark.parametrize("T", [2, 3, 7])  # fewer frames than one full overlap, and just past it
@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (512, 128), (512, 256), (2048, 512), (768, 192), (1024, 128), (256, 64), (1024, 512)])
def test_istft_head_matches_the_f64_oracle(n_fft, hop, T):
    voc = _head_vocos(n_fft, hop)
    _check_head(voc, n_fft, hop, T, None, "fft" if n_fft == 1024 else "dense")
    if n_fft == 1024:  # the dense inverse-DFT GEMM every other n_fft takes, at 1024 too
        _dense(lambda: _check_head(voc, n_fft, hop, T, None, "dense"))


@pytest.mark.parametrize("T", [2, 3, 7])
@pytest.mark.parametrize("n_fft,hop", [(512, 128), (1024, 256), (1024, 1024)])
def test_istft_head_with_a_callers_window(n_fft, hop, T):
    """head.istft.window from the state dict: a Hamming window (non-zero ends, so hop == n_fft satisfies NOLA too)"""
    voc = _head_vocos(n_fft, hop, "hamming")
    w = torch.hamming_window(n_fft).double()
    _check_head(voc, n_fft, hop, T, w, "hamming fft" if n_fft == 1024 else "hamming dense")
    if n_fft == 1024:
        _dense(lambda: _check_head(voc, n_fft, hop, T, w, "hamming dense"))


def test_vocos_refuses_a_window_that_violates_nola():
    """hop == n_fft under the default Hann window: the overlap-added squared window is 0 at the first sample of every hop and the ISTFT would
    write 0 / 0.  torch.istft refuses it (NOLA, 1e-11); so does f5_vocoder_finalize, naming n_fft, hop and the condition."""
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.vocos import Vocos
    v = Vocos(n_mels=8, dim=64, intermediate_dim=128, num_layers=1, n_fft=1024, hop_length=1024).cuda()
    with pytest.raises(_lib.F5HipError) as e:
        v.native()
    assert "NOLA" in str(e.value) and "n_fft 1024" in str(e.value) and "hop 1024" in str(e.value)
    assert v._native is None
    with pytest.raises(_lib.F5HipError):
        v.istft_head(A.random_head(1, 3, 1024, seed=1).cuda())
    # the same configuration under a window that satisfies NOLA, and half overlap under Hann, still load
    assert _head_vocos(1024, 1024, "hamming").native() and _head_vocos(512, 256).native()


# ----------------------------------------------------------------------------- Vocos decode
def _vocos(V, **hp):
    from eraxvif5tts_amd.vocos import Vocos
    v = Vocos(**hp)
    v.load_state_dict({k: t for k, t in V.items() if k in v.state_dict()}, strict=False)
    return v.cuda()


VOCOS_CASES = [(80, 96, 160, 2, 512, 128, 2, 9), (100, 1024, 1024, 1, 1024, 256, 1, 5),  # dim 1024: create()'s maximum width
               (128, 64, 128, 2, 2048, 512, 2, 4)]


@pytest.mark.parametrize("n_mels,dim,inter,layers,n_fft,hop,B,T", VOCOS_CASES)
def test_vocos_decode_matches_oracle(n_mels, dim, inter, layers, n_fft, hop, B, T):
    V = cpu_ref.random_vocos_weights(seed=11, dim=dim, inter=inter, layers=layers, n_mels=n_mels, n_fft=n_fft)
    voc = _vocos(V, n_mels=n_mels, dim=dim, intermediate_dim=inter, num_layers=layers, n_fft=n_fft, hop_length=hop)
    mel = torch.randn(B, n_mels, T, generator=torch.Generator().manual_seed(T)) * 2 - 3
    ref = cpu_ref.vocos_decode(V, mel, n_fft, hop)
    out = voc.decode(mel.cuda()).cpu()
    err = rel_l2(out, ref)
    print(f"vocos decode n_mels {n_mels} dim {dim} n_fft {n_fft} hop {hop} ({B}, {T}): rel-L2 {err:.2e}")
    assert out.shape == ref.shape == (B, (T - 1) * hop) and torch.isfinite(out).all()
    assert err <= 1e-4


def test_vocos_decode_ragged_equals_each_decode():
    n_mels, dim, inter, layers, n_fft, hop = VOCOS_CASES[0][:6]
    V = cpu_ref.random_vocos_weights(seed=11, dim=dim, inter=inter, layers=layers, n_mels=n_mels, n_fft=n_fft)
    voc = _vocos(V, n_mels=n_mels, dim=dim, intermediate_dim=inter, num_layers=layers, n_fft=n_fft, hop_length=hop)
    starts, frames = [3, 9, 19], [2, 9, 5]
    rows = (torch.randn(24, n_mels, generator=torch.Generator().manual_seed(5)) * 2 - 3).cuda()
    waves = voc.decode_ragged(rows, starts, frames)
    for s, t, w in zip(starts, frames, waves):
        own = voc.decode(rows[s: s + t].t()[None].contiguous())
        assert w.shape == own.shape == (1, (t - 1) * hop) and torch.equal(w, own)
    ref = cpu_ref.vocos_decode(V, rows[9:18].t()[None].cpu(), n_fft, hop)
    assert rel_l2(waves[1].cpu(), ref) <= 1e-4


def test_vocos_workspace_regrowth():
    """one instance, decode at T = 7, 129, 7, 300: the workspace is released and reallocated twice and reused smaller once"""
    V = cpu_ref.random_vocos_weights(seed=12, dim=64, inter=128, layers=2)
    voc = _vocos(V, dim=64, intermediate_dim=128, num_layers=2)
    for B, T in ((1, 7), (2, 129), (1, 7), (1, 300)):
        mel = torch.randn(B, 100, T, generator=torch.Generator().manual_seed(T)) * 2 - 3
        ref = cpu_ref.vocos_decode(V, mel)
        out = voc.decode(mel.cuda()).cpu()
        err = rel_l2(out, ref)
        print(f"vocos regrowth ({B}, {T}): rel-L2 {err:.2e}")
        assert out.shape == ref.shape and err <= 1e-4
