"""Cases, inputs, error measures and bounds shared by test_audio_oracles_host.py (CPU: the oracles and what the inputs can see) and
test_gpu_audio_configs.py (the device front-end against the float64 oracle).  Not a test module."""
import math

import numpy as np
import torch

from oracle import cpu_ref

# (n_fft, hop, win, n_mels, sample rate, nw)
MEL_VOCOS_CASES = [
    (1024, 256, 1024, 100, 24000, 513),   # the shortest wave the library takes (pad + 1)
    (1024, 256, 1024, 100, 24000, 2048),  # an exact multiple of hop
    (512, 128, 400, 80, 16000, 1300),     # win < n_fft: the window centred inside the frame
    (2048, 512, 1200, 128, 44100, 5000),
    (1024, 256, 640, 100, 24000, 1025),
    (1024, 300, 1024, 100, 22050, 4000),  # hop does not divide n_fft
]
# the default config, batch of one, T = 63, 64, 65 frames: either side of the 64-row GEMM tile
MEL_TILE_CASES = [(1024, 256, 1024, 100, 24000, 62 * 256), (1024, 256, 1024, 100, 24000, 63 * 256), (1024, 256, 1024, 100, 24000, 64 * 256)]
MEL_BIGVGAN_CASES = [
    (1024, 256, 1024, 100, 24000, 385),   # the shortest accepted wave: one frame
    (1024, 256, 1024, 100, 24000, 2048),
    (1024, 255, 1024, 100, 24000, 3000),  # n_fft - hop odd
    (512, 128, 400, 80, 16000, 1300),
]
ALL_MEL_CASES = ([("vocos", 2) + c for c in MEL_VOCOS_CASES] + [("vocos", 1) + c for c in MEL_TILE_CASES]
                 + [("bigvgan", 2) + c for c in MEL_BIGVGAN_CASES])  # (mel_type, batch, n_fft, hop, win, n_mels, sr, nw)

STRONG = math.log(1e-4)  # the elementwise comparison looks at bins above 10 x the 1e-5 floor

# Bounds of the device against mel_spectrogram_f64 per case: (max |d log-mel| on strong bins, rel-L2 of the linear mel over all bins,
# max |d log-mel| over all bins) = 8 x the error of mel_fp32_emulation below against the same oracle, rounded up to one significant digit, and
# never looser than the ceilings of test_gpu_frontend.py (2e-3, 1e-4, and 0.2 / 5e-2 over all bins for vocos / bigvgan).  The factor 8 is for
# what a CPU cannot measure: the MFMA accumulates chains of 4-term blocks instead of one sequential sum, and the device's sqrtf / logf are
# a few ulps off.  test_audio_oracles_host.py::test_mel_bounds_follow_from_the_fp32_emulation re-derives every row.
MEL_CEILING = {"vocos": (2e-3, 1e-4, 0.2), "bigvgan": (2e-3, 1e-4, 5e-2)}
#                     emulation error (strong, rel-L2, all)   ->   bound (strong, rel-L2, all)
_BOUND_ROWS = [
    (2e-05, 5e-06, 2e-05),    # vocos 1024/256/1024 nw 513        1.76e-06 5.04e-07 1.76e-06
    (6e-05, 4e-06, 6e-05),    # vocos 1024/256/1024 nw 2048       6.28e-06 4.00e-07 6.28e-06
    (5e-05, 3e-06, 5e-05),    # vocos 512/128/400 16 kHz          5.97e-06 2.99e-07 5.97e-06
    (2e-04, 4e-06, 2e-04),    # vocos 2048/512/1200 44.1 kHz      1.87e-05 3.98e-07 1.87e-05
    (2e-04, 3e-06, 2e-04),    # vocos 1024/256/640 nw 1025        1.48e-05 2.57e-07 1.48e-05
    (1e-04, 3e-06, 1e-04),    # vocos 1024/300/1024 22.05 kHz     1.21e-05 3.63e-07 1.21e-05
    (2e-04, 3e-06, 2e-04),    # vocos default, T = 63             1.37e-05 3.63e-07 1.37e-05
    (9e-05, 3e-06, 9e-05),    # vocos default, T = 64             1.08e-05 3.67e-07 1.08e-05
    (3e-04, 3e-06, 3e-04),    # vocos default, T = 65             2.51e-05 3.62e-07 2.51e-05
    (1e-05, 3e-06, 1e-05),    # bigvgan 1024/256/1024 nw 385      1.24e-06 3.07e-07 1.24e-06
    (2e-04, 3e-06, 2e-04),    # bigvgan 1024/256/1024 nw 2048     1.44e-05 3.52e-07 1.44e-05
    (6e-05, 4e-06, 6e-05),    # bigvgan 1024/255/1024 nw 3000     6.66e-06 3.94e-07 6.66e-06
    (6e-05, 2e-06, 6e-05),    # bigvgan 512/128/400 16 kHz        6.92e-06 2.48e-07 6.92e-06
]
MEL_BOUNDS = dict(zip(ALL_MEL_CASES, _BOUND_ROWS))
assert len(_BOUND_ROWS) == len(ALL_MEL_CASES)


def mel_case_id(case):
    mt, b, n_fft, hop, win, n_mels, sr, nw = case
    return f"{mt}-b{b}-{n_fft}-{hop}-{win}-{n_mels}-{sr}-nw{nw}"


def mel_wave(nw, sr, batch=2):
    """[2, nw] float32: row 0 a 300 Hz sine of amplitude 0.3 plus 0.05 randn; row 1 zeros with impulses at samples 0, 1, nw // 2, nw - 2, nw - 1
    (0.5, -0.3, 0.1, 0.2, 0.4): the edge impulses make an off-by-one of the reflect map an O(1) error.  batch = 1: the sum of the two rows."""
    g = torch.Generator().manual_seed(nw)
    t = torch.arange(nw, dtype=torch.float64) / sr
    row0 = (0.3 * torch.sin(2 * math.pi * 300 * t)).float() + 0.05 * torch.randn(nw, generator=g)
    row1 = torch.zeros(nw)
    for i, a in ((0, 0.5), (1, -0.3), (nw // 2, 0.1), (nw - 2, 0.2), (nw - 1, 0.4)):
        row1[i] = a
    return torch.stack([row0, row1]) if batch == 2 else (row0 + row1)[None]


_ref_cache = {}


def mel_case_data(case):
    """(wave, float64 oracle) of a case, computed once per session and never modified"""
    if case not in _ref_cache:
        mt, b, n_fft, hop, win, n_mels, sr, nw = case
        wav = mel_wave(nw, sr, b)
        _ref_cache[case] = (wav, cpu_ref.mel_spectrogram_f64(wav, n_fft, hop, win, n_mels, sr, mt))
    return _ref_cache[case]


def mel_errors(out, ref):
    """(max |d log-mel| on the strong bins of ref, rel-L2 of the linear mel over all bins, max |d log-mel| over all bins)"""
    out, ref = torch.as_tensor(out).double(), torch.as_tensor(ref).double()
    d = (out - ref).abs()
    strong = ref > STRONG
    lin = float((out.exp() - ref.exp()).norm() / ref.exp().norm())
    return float(d[strong].max()) if strong.any() else 0.0, lin, float(d.max())


def mel_fp32_emulation(wave, n_fft, hop, win, n_mels, sr, mel_type):
    """What csrc/frontend.hip computes, in float32 on the CPU: frames and the windowed DFT matrix rounded to float32, the product accumulated
    sequentially over n in float32 (every product and every sum rounded), float32 magnitude, the float32 filterbank product accumulated
    sequentially over the bins, float32 log.  [b, nw] -> float32 array [b, n_mels, T]."""
    f32 = np.float32
    pad, T = cpu_ref.mel_frame_geometry(wave.shape[-1], n_fft, hop, mel_type)
    frames = cpu_ref.mel_frames_f64(wave, n_fft, hop, pad, T).astype(f32)
    b = frames.shape[0]
    frames = frames.reshape(b * T, n_fft)
    cos, sin = cpu_ref.dft_matrices_f64(n_fft)
    w = cpu_ref.hann_in_frame_f64(win, n_fft)
    W = np.concatenate([w * cos, -(w * sin)]).astype(f32)  # [2F, n_fft]
    F = n_fft // 2 + 1
    acc = np.zeros((b * T, 2 * F), dtype=f32)
    for n in range(n_fft):
        acc += frames[:, n, None] * W[None, :, n]
    re, im = acc[:, :F], acc[:, F:]
    mag = np.sqrt(re * re + im * im + f32(1e-9 if mel_type == "bigvgan" else 0.0))
    fb = cpu_ref.mel_filterbank_f64(n_fft, n_mels, sr, mel_type).astype(f32)  # [n_mels, F] (float32 values already)
    mel = np.zeros((b * T, n_mels), dtype=f32)
    for k in range(F):
        mel += mag[:, k, None] * fb[None, :, k]
    return np.log(np.maximum(mel, f32(1e-5))).reshape(b, T, n_mels).transpose(0, 2, 1)


def round_up_1sig(x):
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x))
    return float(f"{math.ceil(x / 10 ** e - 1e-9) * 10 ** e:.0e}")


def emulation_error(case):
    """mel_errors of the fp32 emulation against the float64 oracle"""
    mt, b, n_fft, hop, win, n_mels, sr, nw = case
    wav, ref = mel_case_data(case)
    return mel_errors(torch.from_numpy(mel_fp32_emulation(wav, n_fft, hop, win, n_mels, sr, mt)), ref)


def bounds_from_error(err, mel_type, scale=1.0):
    """the rule above: 8 x (scale x) the emulation error, one significant digit, capped by the old ceilings"""
    return tuple(min(c, round_up_1sig(8 * scale * e)) for e, c in zip(err, MEL_CEILING[mel_type]))


def random_head(B, T, n_fft, seed):
    """head.out activations [B, T, n_fft + 2]: log-magnitude 0.5 randn, phase 3 randn, and one frame whose first 40 log-magnitudes are 7
    (exp(7) > 1e2: the clip is live)"""
    F = n_fft // 2 + 1
    g = torch.Generator().manual_seed(seed)
    head = torch.cat([0.5 * torch.randn(B, T, F, generator=g), 3.0 * torch.randn(B, T, F, generator=g)], dim=-1)
    head[0, T // 2, :40] = 7.0
    return head
