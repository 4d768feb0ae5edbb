"""Ragged Vocos decode (`f5_vocoder_decode_ragged`) and the on-device wave tail (`f5_wave_finish`: rms gain, cross-fade, int16 PCM), through the
C ABI.  Acceptance is exactness, not a tolerance:

* a ragged call gives every utterance the bits of its own batch-1 `Vocos.decode` (same fp32 arithmetic in the same order), whatever its
  neighbours, the skipped prompt rows and the rows between utterances hold;
* the tail gives the bytes of the host functions it replaces: torch's `wave * rms / target_rms`, `cross_fade_concat` (float64 after a mixed
  joint, float32 otherwise) and `pcm16_bytes`;
* `generate()`, `infer_batch_process()` and `infer_prompts()` return what their per-utterance host loops returned, restated here.
The one toleranced check is the oracle comparison, with the bound `test_vocos_decode_matches_oracle` already states (rel-L2 < 1e-4)."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import cpu_ref
from test_gpu_vocoder_wrapper import BIGVGAN_TINY, _write_tiny_assets

pytestmark = pytest.mark.gpu
SR = 24000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@pytest.fixture(scope="module")
def voc():
    from eraxvif5tts_amd.vocos import Vocos
    V = cpu_ref.random_vocos_weights(seed=3)
    v = Vocos()
    v.load_state_dict({k: t for k, t in V.items() if k in v.state_dict()}, strict=False)
    return v.cuda(), V


def _layout(frames, prefix, gap, ld=100, seed=0):
    """mel rows [R, ld]: per utterance `prefix` prompt rows (skipped by row_start), its own T rows, then `gap` rows that belong to nobody"""
    g = torch.Generator().manual_seed(seed)
    total = gap + sum(prefix + t + gap for t in frames)
    buf = torch.randn(total, ld, generator=g) * 2 - 3
    starts, r = [], gap
    for t in frames:
        starts.append(r + prefix)
        r += prefix + t + gap
    return buf, starts


RANDOM32 = [int(x) for x in np.random.default_rng(20).integers(50, 901, 32)]
FRAME_LISTS = {"short_next_to_long": [2, 3, 7, 64, 683], "long_short_long": [683, 2, 300], "single": [129], "random32": RANDOM32,
               "more_than_one_table": [int(x) for x in np.random.default_rng(21).integers(2, 21, 70)]}


@pytest.mark.parametrize("fft", [1, 0])
@pytest.mark.parametrize("prefix", [0, 5])
@pytest.mark.parametrize("name", list(FRAME_LISTS))
def test_ragged_decode_equals_batch1_decode_bit_for_bit(voc, name, prefix, fft):
    """Check 1.  No tolerance: both sides are the same fp32 arithmetic in the same order (FFT head and dense-DFT head)."""
    import gpu_helpers as G
    voc, _ = voc
    frames = FRAME_LISTS[name]
    buf, starts = _layout(frames, prefix, gap=0 if prefix == 0 else 2, seed=len(frames))
    rows = buf.cuda()
    with G.knobs(vocos_fft=fft):
        waves = voc.decode_ragged(rows, starts, frames)
        assert len(waves) == len(frames)
        base = waves[0].data_ptr()
        for i, (s, t) in enumerate(zip(starts, frames)):
            one = voc.decode(rows[s: s + t].t()[None])
            assert waves[i].shape == one.shape == (1, (t - 1) * 256)
            assert waves[i].data_ptr() == base + 4 * 256 * sum(x - 1 for x in frames[:i])  # views of ONE buffer, back to back
            assert torch.equal(waves[i], one), (name, i, t)


@pytest.mark.parametrize("ld", [100, 104])
def test_ragged_decode_does_not_leak_between_utterances(voc, ld):
    """Check 2.  Overwriting utterance j's mel rows, the skipped prompt rows, the rows between utterances and the padding columns with other
    values, NaN and Inf included, leaves every other utterance's wave bit-unchanged."""
    voc, _ = voc
    frames = [5, 2, 40, 3, 130, 2]
    buf, starts = _layout(frames, prefix=4, gap=3, ld=ld, seed=9)
    clean = [w.clone() for w in voc.decode_ragged(buf.cuda(), starts, frames)]
    own = torch.zeros(buf.shape[0], dtype=torch.bool)
    for s, t in zip(starts, frames):
        own[s: s + t] = True
    for j in range(len(frames)):
        dirty = buf.clone()
        junk = torch.full_like(dirty, float("nan"))
        junk[::3] = float("inf")
        junk[1::3] = 1e30
        dirty[~own] = junk[~own]                            # prompt prefixes and gaps
        dirty[:, 100:] = float("nan")                       # columns past n_mels (ld = 104)
        dirty[starts[j]: starts[j] + frames[j], :100] = junk[starts[j]: starts[j] + frames[j], :100]  # utterance j itself
        got = voc.decode_ragged(dirty.cuda(), starts, frames)
        for i in range(len(frames)):
            if i != j:
                assert torch.equal(got[i], clean[i]), (j, i)


def test_ragged_decode_matches_oracle(voc):
    """Check 3: against the CPU oracle per utterance (T >= 7), the bound of test_vocos_decode_matches_oracle."""
    voc, V = voc
    frames = [7, 40, 129, 9, 300]
    buf, starts = _layout(frames, prefix=3, gap=1, seed=4)
    waves = voc.decode_ragged(buf.cuda(), starts, frames)
    for w, s, t in zip(waves, starts, frames):
        ref = cpu_ref.vocos_decode(V, buf[s: s + t].t()[None])
        err = rel_l2(w.cpu(), ref)
        print(f"decode_ragged vs oracle, T = {t}: rel-L2 {err:.2e}")
        assert err < 1e-4


def test_ragged_decode_refuses_bad_extents(voc):
    from eraxvif5tts_amd import _lib
    voc, _ = voc
    rows = torch.zeros(20, 100, device="cuda")
    with pytest.raises(AssertionError):
        voc.decode_ragged(rows, [0, 15], [10, 10])  # past the end of the rows
    import ctypes as C
    wave = torch.zeros(4096, device="cuda")
    rc = _lib.load().f5_vocoder_decode_ragged(voc.native(), 2, (C.c_int32 * 2)(0, 10), (C.c_int32 * 2)(10, 1), _lib.ptr(rows), 100, _lib.ptr(wave), None,
                                              _lib.stream_ptr())
    assert rc != 0 and "T >= 2" in _lib.last_error()


# ---------------------------------------------------------------------------------------------------------------- wave_finish
LENGTHS = [9000, 7700, 12000, 8000, 7300]
HOST_RMS = [0.05, 0.2, 0.0999, 0.1, 0.03]  # target 0.1: applied, not, applied, not (equal is not less), applied
DURATIONS = {"off": 0.0, "default": 0.15, "one_sample": 1 / 24000, "longer_than_shortest": 0.5}


def _host_tail(waves_gpu, d, rms, target, on_cpu=False):
    """the host path: torch's gain on each wave (on the GPU tensor as the entry points have it, or on a CPU tensor), numpy's cross-fade"""
    out = []
    for i, w in enumerate(waves_gpu):
        r = rms[i] if isinstance(rms, list) else rms
        w = w.cpu() if on_cpu else w
        if r is not None and r < target:
            w = w * r / target
        out.append(w.cpu().numpy())
    from eraxvif5tts_amd.infer.utils_infer import cross_fade_concat
    return cross_fade_concat(out, d)


@pytest.mark.parametrize("gain", ["none", "host_list", "host_tensor", "dev_applied", "dev_not_applied", "host_list_true_divide"])
@pytest.mark.parametrize("dname", list(DURATIONS))
@pytest.mark.parametrize("B", [1, 2, 5])
def test_wave_finish_equals_the_host_functions_byte_for_byte(B, dname, gain):
    """Check 4 on random waves, |x| <= 0.99 (after gain: every gain here is below 1)."""
    from eraxvif5tts_amd.infer.utils_infer import finish_waves, plan_wave_tail
    from eraxvif5tts_amd.streaming.wire import pcm16_bytes
    d, lengths, target = DURATIONS[dname], LENGTHS[:B], 0.1
    g = torch.Generator().manual_seed(B * 7 + len(dname))
    buf = ((torch.rand(sum(lengths), generator=g) * 2 - 1) * 0.99).cuda()
    waves = list(torch.split(buf, lengths))
    rms = {"none": None, "host_list": HOST_RMS[:B], "host_list_true_divide": HOST_RMS[:B], "host_tensor": torch.tensor(0.0625),
           "dev_applied": torch.tensor(0.07, device="cuda"), "dev_not_applied": torch.tensor(0.13, device="cuda")}[gain]
    ref = _host_tail(waves, d, rms, target, on_cpu=gain == "host_list_true_divide")
    done = finish_waves(buf, lengths, d, SR, rms=rms, target_rms=target, want_float=True, want_pcm16=True, gain_divide=gain == "host_list_true_divide")
    plan = plan_wave_tail(lengths, d, SR)
    if dname == "longer_than_shortest" and B > 1:
        # utterances shorter than the cross-fade: the joints chain, the library answers F5_ENOTSUP and the caller keeps the host functions
        assert done is None and not plan["device_ok"]
        return
    assert plan["device_ok"] and done is not None
    sig, pcm = done[0].cpu().numpy(), done[1].cpu().numpy()
    assert sig.dtype == ref.dtype == plan["dtype"] and (sig.dtype == np.float64) == (B > 1 and dname in ("default", "one_sample"))
    assert sig.shape == ref.shape and np.array_equal(sig, ref)
    assert pcm.dtype == np.int16 and pcm.tobytes() == pcm16_bytes(ref)
    pcm_only = finish_waves(buf, lengths, d, SR, rms=rms, target_rms=target, want_float=False, want_pcm16=True,
                            gain_divide=gain == "host_list_true_divide")
    assert pcm_only[0] is None and torch.equal(pcm_only[1].cpu(), done[1].cpu())


def test_wave_finish_many_utterances_and_saturation():
    """More utterances than one kernel table holds (the tables overlap by one utterance: a joint needs its left neighbour), n = 1 and n = 40; and
    the documented saturation of products at or beyond +-32768, which numpy's cast leaves undefined."""
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    from eraxvif5tts_amd.streaming.wire import pcm16_bytes
    g = torch.Generator().manual_seed(2)
    lengths = [int(x) for x in torch.randint(80, 400, (150,), generator=g)]
    buf = ((torch.rand(sum(lengths), generator=g) * 2 - 1) * 0.99).cuda()
    rms = [0.02 + 0.001 * i for i in range(150)]
    for d in (1 / 24000, 40 / 24000 + 1e-9, 0.0):
        ref = _host_tail(list(torch.split(buf, lengths)), d, rms, 0.1)
        sig, pcm = finish_waves(buf, lengths, d, SR, rms=rms, target_rms=0.1, want_pcm16=True)
        assert np.array_equal(sig.cpu().numpy(), ref) and pcm.cpu().numpy().tobytes() == pcm16_bytes(ref)
    loud = torch.tensor([1.5, -1.5, 1.0, -1.0, 32768.0 / 32767.0, 0.999999], device="cuda")
    _, pcm = finish_waves(loud, [6], 0.0, SR, want_pcm16=True)
    assert pcm.cpu().tolist() == [32767, -32768, 32767, -32767, 32767, 32766]


def test_wave_finish_on_decoded_waves(voc):
    """Check 4 on decoded waves: ragged decode -> wave_finish against batch-1 decodes -> host functions."""
    from eraxvif5tts_amd.infer.utils_infer import finish_waves
    from eraxvif5tts_amd.streaming.wire import pcm16_bytes
    voc, _ = voc
    frames = [40, 64, 33, 90]
    buf, starts = _layout(frames, prefix=6, gap=0, seed=12)
    rows = buf.cuda()
    wave, samples = voc.decode_ragged_buffer(rows, starts, frames)
    wave = wave * (0.9 / float(wave.abs().max()))  # inside (-1, 1): the int16 cast is defined
    singles = []
    off = 0
    for s, t in zip(starts, frames):
        singles.append(wave[off: off + (t - 1) * 256].clone())
        off += (t - 1) * 256
    rms = torch.tensor(0.08, device="cuda")
    for d in (0.15, 0.0):
        ref = _host_tail(singles, d, rms, 0.1)
        sig, pcm = finish_waves(wave, samples, d, SR, rms=rms, target_rms=0.1, want_pcm16=True)
        assert sig.cpu().numpy().dtype == ref.dtype and np.array_equal(sig.cpu().numpy(), ref)
        assert pcm.cpu().numpy().tobytes() == pcm16_bytes(ref)


# ---------------------------------------------------------------------------------------------------------------- end to end
ARCH = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2, pe_attn_head=1, text_mask_padding=False)
SENTENCE = "hello there, this is a test. "
TEXTS = {2: SENTENCE * 3 + "and one more sentence to force a second chunk, because the budget is small.",
         4: (SENTENCE * 3 + "and one more sentence to force another chunk, because the budget is small. ") * 3}


def _tts(tmp_path, prec):
    from eraxvif5tts_amd.infer import audio
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    W = cpu_ref.random_dit_weights(ARCH, 32, seed=25)
    VW = cpu_ref.random_vocos_weights(seed=26, dim=64, inter=128, layers=2)
    cfg_path, ckpt, vdir, vocab = _write_tiny_assets(str(tmp_path), ARCH, 32, W, dict(dim=64, intermediate_dim=128, num_layers=2), VW)
    t = np.arange(int(2.0 * SR)) / SR
    wav = 0.03 * np.sin(2 * np.pi * 190 * t + 0.7) * (1 + 0.3 * np.sin(2 * np.pi * 5 * t)) + 0.01 * np.sin(2 * np.pi * 1370 * t)
    ref_wav = os.path.join(str(tmp_path), "ref.wav")
    audio.write_wav(ref_wav, wav, SR)
    tts = F5TTSWrapper(model_name=cfg_path, ckpt_path=ckpt, vocab_file=vocab, use_local_vocoder=True, vocoder_path=vdir, precision=prec)
    tts.preprocess_reference(ref_wav, "a quiet tone")
    return tts


def _todays_loop(tts, text, nfe_step, cross_fade_duration, seed):
    """generate() as it was before the device tail: the chunks' mels from the sampler, then PER UTTERANCE the permuted slice through
    Vocos.decode (or the generator), the rms rule with its host comparison, a copy to the host, and cross_fade_concat in numpy."""
    from eraxvif5tts_amd.infer.utils_infer import chunk_text, cross_fade_concat
    from eraxvif5tts_amd.model.utils import convert_char_to_pinyin
    secs = tts.ref_audio_processed.shape[-1] / SR
    chunks = chunk_text(text, max_chars=int(len(tts.ref_text.encode("utf-8")) / secs * (22 - secs)))
    jobs = []
    for c in chunks:
        speed = 0.3 if len(c.encode("utf-8")) < 10 else tts.speed
        jobs.append((convert_char_to_pinyin([tts.ref_text + c]),
                     tts.ref_audio_len + int(tts.ref_audio_len / len(tts.ref_text.encode("utf-8")) * len(c.encode("utf-8")) / speed)))
    if seed is not None:
        torch.manual_seed(seed)
    with torch.inference_mode():
        if len(jobs) >= 2 and min(d for _, d in jobs) >= 256:
            mels = tts.model.sample_ragged(tts.ref_audio_processed, [j[0][0] for j in jobs], [j[1] for j in jobs], steps=nfe_step,
                                           cfg_strength=tts.cfg_strength, sway_sampling_coef=tts.sway_sampling_coef)
        else:
            mels = [tts.model.sample(cond=tts.ref_audio_processed, text=j[0], duration=j[1], steps=nfe_step, cfg_strength=tts.cfg_strength,
                                     sway_sampling_coef=tts.sway_sampling_coef, return_trajectory=False)[0] for j in jobs]
        waves = []
        for generated in mels:
            generated = generated.to(torch.float32)[:, tts.ref_audio_len:, :].permute(0, 2, 1)
            wave = tts.vocoder.decode(generated) if tts.mel_spec_type == "vocos" else tts.vocoder(generated)
            rms = torch.sqrt(torch.mean(torch.square(tts.ref_audio_processed)))
            if rms < tts.target_rms:
                wave = wave * rms / tts.target_rms
            waves.append(wave.squeeze().cpu().numpy())
    return cross_fade_concat(waves, cross_fade_duration, SR), len(chunks)


@pytest.mark.parametrize("prec,nchunks,target", [("fp32", 2, 0.2), ("fp32", 4, 0.2), ("bf16", 2, 0.05), ("bf16", 4, 0.2)])
def test_generate_equals_todays_loop(tmp_path, prec, nchunks, target):
    """Check 5: generate() through the device tail == the per-utterance host loop, float and PCM, with the gain applied (target 0.2 above the
    prompt's rms of about 0.1) and not (0.05)."""
    from eraxvif5tts_amd.streaming.wire import pcm16_bytes
    tts = _tts(tmp_path, prec)
    tts.target_rms = target
    text = TEXTS[nchunks]
    want, n = _todays_loop(tts, text, 3, tts.cross_fade_duration, seed=77)
    print(f"generate() [{prec}, {nchunks} chunks]: {len(want)} samples, max |x| = {np.abs(want).max():.3f}")
    assert n == nchunks and want.dtype == np.float64 and np.abs(want).max() < 1  # inside what the int16 cast defines
    torch.manual_seed(77)
    wave, rate = tts.generate(text, nfe_step=3, return_numpy=True)
    assert rate == SR and wave.dtype == want.dtype and np.array_equal(wave, want)
    torch.manual_seed(77)
    pcm, _ = tts.generate(text, nfe_step=3, return_numpy=True, return_pcm16=True)
    assert pcm.dtype == np.int16 and pcm.tobytes() == pcm16_bytes(want)
    # cross-fade off: plain concatenation, float32, and the PCM product in float32
    want32, _ = _todays_loop(tts, text, 3, 0.0, seed=78)
    torch.manual_seed(78)
    pcm32, _, spec = tts.generate(text, nfe_step=3, cross_fade_duration=0.0, return_numpy=True, return_pcm16=True, return_spectrogram=True)
    assert want32.dtype == np.float32 and pcm32.tobytes() == pcm16_bytes(want32) and spec.shape == (100, len(want32) // 256 + nchunks)


def test_generate_short_chunks_take_the_host_functions(tmp_path):
    """A cross-fade longer than the chunks: f5_wave_finish answers F5_ENOTSUP and generate() joins the (ragged-decoded) waves on the host."""
    tts = _tts(tmp_path, "fp32")
    tts.target_rms = 0.2
    want, n = _todays_loop(tts, TEXTS[2], 2, 30.0, seed=5)
    torch.manual_seed(5)
    wave, _ = tts.generate(TEXTS[2], nfe_step=2, cross_fade_duration=30.0, return_numpy=True)
    assert n == 2 and np.array_equal(wave, want)


def test_generate_with_bigvgan_and_with_a_foreign_vocoder(tmp_path):
    """BigVGAN: the generator still runs per utterance, the tail on the device.  A vocoder object of somebody else's (no decode_ragged): the
    host loop, as before."""
    from eraxvif5tts_amd.bigvgan import BigVGAN
    from eraxvif5tts_amd.infer.utils_infer import device_tail_kind
    tts = _tts(tmp_path, "fp32")
    tts.target_rms = 0.2
    vocos = tts.vocoder
    W = cpu_ref.random_bigvgan_weights(dict(BIGVGAN_TINY), seed=3)
    W["conv_post.weight"] = W["conv_post.weight"] * 0.0015
    big = BigVGAN(dict(BIGVGAN_TINY))
    big.load_state_dict(W)
    tts.vocoder, tts.mel_spec_type = big.eval().cuda(), "bigvgan"
    assert device_tail_kind(tts.vocoder, tts.ref_audio_processed) == "bigvgan"
    want, n = _todays_loop(tts, TEXTS[2], 2, 0.15, seed=9)
    torch.manual_seed(9)
    wave, _ = tts.generate(TEXTS[2], nfe_step=2, return_numpy=True)
    assert n == 2 and np.abs(want).max() < 1 and np.array_equal(wave, want)

    class Foreign(torch.nn.Module):  # plug point B with an object the library knows nothing about
        def decode(self, mel):
            return torch.tanh(mel.mean(dim=1)).repeat_interleave(256, dim=1)[:, 256:] * 0.5

    tts.vocoder, tts.mel_spec_type = Foreign(), "vocos"
    assert device_tail_kind(tts.vocoder, tts.ref_audio_processed) is None and device_tail_kind(vocos, tts.ref_audio_processed) == "vocos"
    want, _ = _todays_loop(tts, TEXTS[2], 2, 0.15, seed=10)
    torch.manual_seed(10)
    wave, _ = tts.generate(TEXTS[2], nfe_step=2, return_numpy=True)
    assert np.array_equal(wave, want)


def test_stream_audio_sends_the_same_bytes(tmp_path):
    """stream_audio over the wrapper takes the int16 from the device; the bytes on the wire are pcm16_bytes of the host loop's floats."""
    from eraxvif5tts_amd.streaming.wire import ReferenceCache, create_wave_header, pcm16_bytes, stream_audio
    tts = _tts(tmp_path, "bf16")
    tts.target_rms = 0.2
    cache = ReferenceCache()
    cache.entries["spk"] = {"loaded": True, "processed_mel": tts.ref_audio_processed.clone(), "processed_text": tts.ref_text,
                            "processed_mel_len": tts.ref_audio_len}
    chunks = ["hello there.", "and a second one, a little longer than the first."]
    torch.manual_seed(31)
    parts = list(stream_audio(tts, cache, "spk", chunks, nfe_step=3))
    assert parts[0] == create_wave_header(SR) and len(parts) == 3
    cache.install(tts, "spk")
    torch.manual_seed(31)
    for text, got in zip(chunks, parts[1:]):
        want, _ = _todays_loop(tts, text, 3, tts.cross_fade_duration, seed=None)  # (no reseeding: the stream draws its chunks' noise call after call)
        assert np.abs(want).max() < 1 and got == pcm16_bytes(want)


def test_infer_batch_process_equals_todays_loop(tmp_path):
    """Check 5 for utils_infer.infer_batch_process: the ORIGINAL-rms rule from a CPU scalar, ragged and single batches."""
    from eraxvif5tts_amd.infer import utils_infer as U
    from eraxvif5tts_amd.model.utils import convert_char_to_pinyin
    tts = _tts(tmp_path, "fp32")
    model, vocoder = tts.model, tts.vocoder
    t = np.arange(int(1.5 * SR)) / SR
    a = torch.from_numpy(0.02 * np.sin(2 * np.pi * 200 * t) * (1 + 0.4 * np.sin(2 * np.pi * 2 * t))).float()[None]  # quieter than the target
    ref_text = "a quiet tone. "
    ref_text_used = ref_text + " "  # infer_batch_process appends a space behind a single-byte last character
    batches = U.chunk_text(TEXTS[4], max_chars=60)[:3]

    def todays(batch_list, d, seed):
        audio = a
        rms = torch.sqrt(torch.mean(torch.square(audio)))
        assert rms < 0.1
        audio = (audio * 0.1 / rms).to("cuda")
        ref_len = audio.shape[-1] // 256
        jobs = [(convert_char_to_pinyin([ref_text_used + g]),
                 ref_len + int(ref_len / len(ref_text_used.encode()) * len(g.encode()) / (0.3 if len(g.encode()) < 10 else 1))) for g in batch_list]
        torch.manual_seed(seed)
        with torch.inference_mode():
            if len(jobs) >= 2 and min(x for _, x in jobs) >= 256:
                mels = model.sample_ragged(audio, [j[0][0] for j in jobs], [j[1] for j in jobs], steps=2, cfg_strength=2.0, sway_sampling_coef=-1)
            else:
                mels = [model.sample(cond=audio, text=j[0], duration=j[1], steps=2, cfg_strength=2.0, sway_sampling_coef=-1, return_trajectory=False)[0]
                        for j in jobs]
            waves, specs = [], []
            for generated in mels:
                generated = generated.to(torch.float32)[:, ref_len:, :].permute(0, 2, 1)
                wave = vocoder.decode(generated)
                if rms < 0.1:
                    wave = wave * rms / 0.1
                waves.append(wave.squeeze().cpu().numpy())
                specs.append(generated[0].cpu().numpy())
        return U.cross_fade_concat(waves, d), np.concatenate(specs, axis=1)

    for batch_list, d, seed in ((batches, 0.15, 3), (batches, 0.0, 4), (batches[:1], 0.15, 5)):
        want, want_spec = todays(batch_list, d, seed)
        torch.manual_seed(seed)
        wave, rate, spec = next(U.infer_batch_process((a, SR), ref_text, batch_list, model, vocoder, nfe_step=2, device="cuda", cross_fade_duration=d))
        assert rate == SR and wave.dtype == want.dtype and np.array_equal(wave, want) and np.array_equal(spec, want_spec)


def test_infer_prompts_bucket_equals_todays_loop():
    """Check 5 for eval.prompts.infer_prompts: one bucket, one ragged vocoder call; per-utterance host rms values, some applied and some not."""
    from eraxvif5tts_amd.eval import prompts as P
    from eraxvif5tts_amd.vocos import Vocos
    from test_gpu_prompts import _cfm
    cfm = _cfm("fp32")
    VW = cpu_ref.random_vocos_weights(seed=27, dim=64, inter=128, layers=2)
    voc = Vocos(dim=64, intermediate_dim=128, num_layers=2)
    voc.load_state_dict({k: t for k, t in VW.items() if k in voc.state_dict()}, strict=False)
    voc = voc.cuda()
    meta = P.synthetic_metainfo(14, seed=5, min_secs=3.2, max_secs=9.0)
    buckets = P.get_inference_prompt(meta, tokenizer="char", infer_batch_size=1400, num_buckets=8, min_secs=3, max_secs=40, device="cuda")
    bucket = max(buckets, key=lambda b: len(b[0]))
    utts, ref_rms, _, ref_lens, totals, _ = bucket
    assert len(utts) >= 2 and P.ragged_ok(cfm, bucket)
    target = float(sorted(float(r) for r in ref_rms)[len(ref_rms) // 2])  # the median: applied to some utterances, not to others
    assert any(r < target for r in ref_rms) and not all(r < target for r in ref_rms)
    kw = dict(nfe_step=3, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=11)
    got = list(P.infer_prompts(cfm, [bucket], vocoder=voc, target_rms=target, **kw))
    generated, _ = P.ragged_sample_fn(cfm)(**P.sample_kwargs(bucket, "cuda", 3, 2.0, -1.0, 11, False))
    assert [g[0] for g in got] == list(utts)
    for i, (_, mel, wave) in enumerate(got):
        gen = generated[i][ref_lens[i]: totals[i], :].unsqueeze(0).permute(0, 2, 1).to(torch.float32)
        want = voc.decode(gen)
        if ref_rms[i] < target:
            want = want * ref_rms[i] / target
        assert torch.equal(mel, gen) and wave.shape == want.shape and torch.equal(wave, want), utts[i]
