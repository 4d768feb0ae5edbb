"""The float64 oracles of the two audio ends (oracle/cpu_ref.py: mel_spectrogram_f64, istft_f64, head_to_wave_f64, vocos_decode with ISTFT
hyper-parameters) on the CPU: (1) they agree with the existing float32 oracles, the BigVGAN golden and torch.istft at the default config, within
what separates fp32 from fp64 there (1e-4 in log-mel, 1e-5 rel-L2); (2) the inputs of tests/test_gpu_audio_configs.py can see the bugs they
are meant for: three deliberately wrong variants of the mel oracle miss that module's bounds by a factor of 10 or more in every case they apply
to; (3) at least 70 % of all bins of every mel case are "strong", so the elementwise comparison cannot hide most of the picture; (4) the bounds
themselves are what the fp32 emulation of the kernel gives under the stated rule.  No GPU code runs or is mutated here."""
import math

import numpy as np
import pytest
import torch

import audio_cases as A
from conftest import load_golden, rel_l2
from oracle import cpu_ref

IDS = [A.mel_case_id(c) for c in A.ALL_MEL_CASES]


# ----------------------------------------------------------------------------- (1) agreement at the default config
def _agree(new, old):
    strong, lin, _ = A.mel_errors(new, old.double())
    assert new.dtype == torch.float64 and new.shape == old.shape
    assert strong < 1e-4 and lin < 1e-5, (strong, lin)


@pytest.mark.parametrize("nw", [513, 2048, 12000])
def test_mel_f64_agrees_with_the_fp32_oracle(nw):
    wav = A.mel_wave(nw, 24000)
    _agree(cpu_ref.mel_spectrogram_f64(wav), cpu_ref.mel_spectrogram(wav))


@pytest.mark.parametrize("nw", [385, 2048, 7777])
def test_bigvgan_mel_f64_agrees_with_the_fp32_oracle(nw):
    wav = A.mel_wave(nw, 24000)
    _agree(cpu_ref.mel_spectrogram_f64(wav, mel_type="bigvgan"), cpu_ref.bigvgan_mel_spectrogram(wav))


def test_bigvgan_mel_f64_agrees_with_the_reference_golden():
    z = load_golden("bigvgan_mel")
    wave = torch.from_numpy(z["wave"])
    _agree(cpu_ref.mel_spectrogram_f64(wave, mel_type="bigvgan"), torch.from_numpy(z["mel"]))
    _agree(cpu_ref.mel_spectrogram_f64(wave[:1, :7777], mel_type="bigvgan"), torch.from_numpy(z["mel_7777"]))


@pytest.mark.parametrize("n_fft,hop,T,window", [(1024, 256, 9, "hann"), (512, 128, 2, "hann"), (768, 192, 7, "hann"), (512, 128, 5, "hamming"),
                                                (1024, 1024, 3, "hamming")])
def test_istft_f64_agrees_with_torch_istft(n_fft, hop, T, window):
    F = n_fft // 2 + 1
    head = A.random_head(2, T, n_fft, seed=n_fft + T).double()
    mag = torch.exp(head[..., :F]).clamp(max=1e2).transpose(1, 2)
    ph = head[..., F:].transpose(1, 2)
    re, im = mag * torch.cos(ph), mag * torch.sin(ph)
    w = torch.hann_window(n_fft, dtype=torch.float64) if window == "hann" else torch.hamming_window(n_fft, dtype=torch.float64)
    ref = torch.istft(torch.complex(re, im), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True)
    out = cpu_ref.istft_f64(re, im, n_fft, hop, None if window == "hann" else w)
    assert out.dtype == torch.float64 and out.shape == ref.shape == (2, (T - 1) * hop)
    assert rel_l2(out, ref) < 1e-12
    assert rel_l2(cpu_ref.head_to_wave_f64(head.float(), n_fft, hop, None if window == "hann" else w), ref) < 1e-12
    if window == "hann":  # the float32 oracle the vocoder tests have used so far
        assert rel_l2(cpu_ref.istft_center(re.float(), im.float(), n_fft, hop), out) < 1e-5


def test_vocos_decode_passes_the_istft_parameters_through():
    V = cpu_ref.random_vocos_weights(seed=2, dim=32, inter=64, layers=1, n_mels=20, n_fft=256)
    mel = torch.randn(1, 20, 6, generator=torch.Generator().manual_seed(1))
    hann = cpu_ref.vocos_decode(V, mel, 256, 64)
    assert hann.shape == (1, 5 * 64) and hann.dtype == torch.float32
    assert rel_l2(cpu_ref.vocos_decode(V, mel, 256, 64, torch.hann_window(256, dtype=torch.float64)), hann) < 1e-5
    assert rel_l2(cpu_ref.vocos_decode(V, mel, 256, 64, torch.hamming_window(256)), hann) > 1e-2  # the window is used
    assert cpu_ref.vocos_decode(V, mel, 256, 128).shape == (1, 5 * 128)


# ----------------------------------------------------------------------------- (2) the inputs see the bugs
def _variant(case, index=cpu_ref.reflect_index, window=None, origin=0):
    mt, b, n_fft, hop, win, n_mels, sr, nw = case
    wav, _ = A.mel_case_data(case)
    pad, T = cpu_ref.mel_frame_geometry(nw, n_fft, hop, mt)
    frames = cpu_ref.mel_frames_f64(wav, n_fft, hop, pad - origin, T, index)
    w = cpu_ref.hann_in_frame_f64(win, n_fft) if window is None else window
    return torch.from_numpy(cpu_ref.log_mel_from_frames_f64(frames, w, cpu_ref.mel_filterbank_f64(n_fft, n_mels, sr, mt), 1e-9 if mt == "bigvgan" else 0.0))


def _misses_by_10(case, out):
    _, ref = A.mel_case_data(case)
    strong, lin, _ = A.mel_errors(out, ref)
    b = A.MEL_BOUNDS[case]
    assert strong >= 10 * b[0] and lin >= 10 * b[1], (strong, lin, b)


def _edge_repeating_index(s, nw):
    """the wrong reflect map: mirrors about the half sample outside the wave, so that the edge sample appears twice ("symmetric" padding)"""
    s = np.where(s < 0, -s - 1, s)
    return np.where(s >= nw, 2 * nw - 1 - s, s)


@pytest.mark.parametrize("case", A.ALL_MEL_CASES, ids=IDS)
def test_unmodified_variant_is_the_oracle(case):
    assert torch.equal(_variant(case), A.mel_case_data(case)[1])


@pytest.mark.parametrize("case", A.ALL_MEL_CASES, ids=IDS)
def test_inputs_see_a_reflect_that_repeats_the_edge(case):
    _misses_by_10(case, _variant(case, index=_edge_repeating_index))


@pytest.mark.parametrize("case", A.ALL_MEL_CASES, ids=IDS)
def test_inputs_see_a_frame_origin_off_by_one(case):
    _misses_by_10(case, _variant(case, origin=1))
    _misses_by_10(case, _variant(case, origin=-1))


@pytest.mark.parametrize("case", [c for c in A.ALL_MEL_CASES if c[4] < c[2]], ids=[i for i, c in zip(IDS, A.ALL_MEL_CASES) if c[4] < c[2]])
def test_inputs_see_a_short_window_left_aligned(case):
    n_fft, win = case[2], case[4]
    w = np.zeros(n_fft)
    w[:win] = 0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(win) / win)
    _misses_by_10(case, _variant(case, window=w))


# ----------------------------------------------------------------------------- (3) the strong-bin cap
@pytest.mark.parametrize("case", A.ALL_MEL_CASES, ids=IDS)
def test_at_least_70_percent_of_the_bins_are_strong(case):
    _, ref = A.mel_case_data(case)
    assert float((ref > A.STRONG).double().mean()) >= 0.70


# ----------------------------------------------------------------------------- (4) where the bounds come from
@pytest.mark.parametrize("case", A.ALL_MEL_CASES, ids=IDS)
def test_mel_bounds_follow_from_the_fp32_emulation(case):
    """MEL_BOUNDS = min(old ceiling, 8 x emulation error rounded up to one significant digit).  The emulation is deterministic IEEE float32, but
    its float64 inputs (sin, cos) may differ in the last bit between math libraries, so a value that sits on a rounding edge may move by 2 %."""
    err = A.emulation_error(case)
    print(f"{A.mel_case_id(case)}: emulation strong {err[0]:.2e} rel-L2 {err[1]:.2e} all {err[2]:.2e} -> bounds {A.MEL_BOUNDS[case]}")
    for i in range(3):
        assert A.MEL_BOUNDS[case][i] in {A.bounds_from_error(err, case[0], s)[i] for s in (0.98, 1.0, 1.02)}
        assert A.MEL_BOUNDS[case][i] <= A.MEL_CEILING[case[0]][i]
