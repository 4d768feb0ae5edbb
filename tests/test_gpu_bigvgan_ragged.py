"""Ragged BigVGAN decode (`f5_bigvgan_decode_ragged`): all utterances of a call through one set of launches, through the C ABI.

Acceptance is exactness: a ragged call gives every utterance the bits of its own batch-1 `BigVGAN.forward` (the same fp32 arithmetic in the same
order: the GEMMs keep their K, the row-crossing kernels stop at the utterance's own ends), whatever its neighbours, the skipped prompt rows, the
rows between utterances and the padding columns hold; cutting the call into several launch sets (`bigvgan_group_frames`) changes no bit; and
`generate()`, `infer_batch_process()` and `infer_prompts()` return what their per-utterance loops returned, restated here.  The one toleranced
check is the oracle comparison, with the bound and the non-saturation condition `test_bigvgan_forward_matches_oracle` states (rel-L2 < 1e-4,
fewer than 1 % of the reference's samples at |x| >= 0.999)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import cpu_ref
from test_gpu_vocoder_wrapper import BIGVGAN_TINY, _write_tiny_assets

pytestmark = pytest.mark.gpu
SR = 24000
UP = 256
F5_EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _hp(variant):
    hp = dict(BIGVGAN_TINY)
    if variant == "tanh_bias":
        hp.update(use_tanh_at_final=True, use_bias_at_final=True, snake_logscale=False)
    return hp


def _weights(variant, seed):
    """the weights of test_bigvgan_forward_matches_oracle: random, conv_post scaled so that the final clamp / tanh is not saturated"""
    hp = _hp(variant)
    W = cpu_ref.random_bigvgan_weights(hp, seed=seed)
    if not hp["snake_logscale"]:
        for k in W:
            if k.endswith(".alpha") or k.endswith(".beta"):
                W[k] = W[k].abs() + 0.5
    W["conv_post.weight"] = W["conv_post.weight"] * 0.0015
    return hp, W


def _bigvgan(variant, seed):
    from eraxvif5tts_amd.bigvgan import BigVGAN
    hp, W = _weights(variant, seed)
    voc = BigVGAN(hp)
    voc.load_state_dict(W)
    return voc.eval().cuda(), hp, W


@pytest.fixture(scope="module")
def vocs():
    return {"v2": _bigvgan("v2", 13), "tanh_bias": _bigvgan("tanh_bias", 77)}


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


FRAME_LISTS = {"short_next_to_long": [1, 2, 3, 7, 64, 300], "long_short_long": [300, 1, 129], "single": [129],
               "random32": [int(x) for x in np.random.default_rng(20).integers(5, 121, 32)],
               "more_than_one_table": [int(x) for x in np.random.default_rng(21).integers(1, 9, 70)]}


@pytest.mark.parametrize("variant", ["v2", "tanh_bias"])
@pytest.mark.parametrize("ld", [100, 104])
@pytest.mark.parametrize("prefix", [0, 5])
@pytest.mark.parametrize("name", list(FRAME_LISTS))
def test_ragged_decode_equals_batch1_forward_bit_for_bit(vocs, name, prefix, ld, variant):
    """Check 1.  No tolerance: both sides are the same fp32 arithmetic in the same order."""
    voc = vocs[variant][0]
    frames = FRAME_LISTS[name]
    buf, starts = _layout(frames, prefix, gap=0 if prefix == 0 else 2, ld=ld, seed=len(frames))
    rows = buf.cuda()
    waves = voc.decode_ragged(rows, starts, frames)
    assert len(waves) == len(frames)
    base = waves[0].data_ptr()
    for i, (s, t) in enumerate(zip(starts, frames)):
        one = voc(rows[s: s + t, :100].t()[None])
        assert waves[i].shape == one.shape == (1, 1, t * UP)
        assert waves[i].data_ptr() == base + 4 * UP * sum(frames[:i])  # views of ONE buffer, back to back
        assert torch.equal(waves[i], one), (name, i, t)


@pytest.mark.parametrize("ld", [100, 104])
def test_ragged_decode_does_not_leak_between_utterances(vocs, ld):
    """Check 2.  Overwriting utterance j's mel rows, the skipped prompt rows, the rows between utterances and the padding columns with other
    values, NaN and Inf included, leaves every other utterance's wave bit-unchanged."""
    voc = vocs["v2"][0]
    frames = [5, 1, 40, 3, 70, 2]
    buf, starts = _layout(frames, prefix=4, gap=3, ld=ld, seed=9)
    clean = [w.clone() for w in voc.decode_ragged(buf.cuda(), starts, frames)]
    assert all(bool(torch.isfinite(w).all()) for w in clean)
    own = torch.zeros(buf.shape[0], dtype=torch.bool)
    for s, t in zip(starts, frames):
        own[s: s + t] = True
    for j in range(len(frames)):
        dirty = buf.clone()
        junk = torch.full_like(dirty, float("nan"))
        junk[::3] = float("inf")
        junk[1::3] = 1e30
        dirty[~own] = junk[~own]                            # prompt prefixes and gaps
        dirty[:, 100:] = float("nan")                       # columns past num_mels (ld = 104)
        dirty[starts[j]: starts[j] + frames[j], :100] = junk[starts[j]: starts[j] + frames[j], :100]  # utterance j itself
        got = voc.decode_ragged(dirty.cuda(), starts, frames)
        for i in range(len(frames)):
            if i != j:
                assert torch.equal(got[i], clean[i]), (j, i)


def test_launch_sets_do_not_change_a_bit(vocs):
    """Check 3.  `bigvgan_group_frames` = 50 cuts [30, 20, 90, 10, 45, 5] into [30, 20] [90] [10] [45, 5]: four launch sets, one of them a single
    utterance longer than the budget.  Same bits as the default (one set)."""
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    voc = vocs["v2"][0]
    frames = [30, 20, 90, 10, 45, 5]
    buf, starts = _layout(frames, prefix=2, gap=1, seed=33)
    rows = buf.cuda()
    whole, samples = voc.decode_ragged_buffer(rows, starts, frames)
    assert samples == [t * UP for t in frames]
    lib = _lib.load()
    for budget in (50, 1):  # (1: every utterance a set of its own)
        with G.knobs(bigvgan_group_frames=budget):
            cut, _ = voc.decode_ragged_buffer(rows, starts, frames)
            assert torch.equal(cut, whole), budget
    assert lib.f5_tuning_set(b"bigvgan_group_frames", 0) == F5_EINVAL


# Seeds for which the reference ALONE meets the non-saturation condition on these inputs (checked on the CPU when the test was written: the
# fraction of reference samples at |x| >= 0.999 is 0 for both).
ORACLE_CASES = {"v2": 13, "tanh_bias": 77}
ORACLE_FRAMES = [5, 40, 13, 77, 1]


@pytest.mark.parametrize("variant", list(ORACLE_CASES))
def test_ragged_decode_matches_oracle(vocs, variant):
    """Check 4: per utterance against oracle/cpu_ref.bigvgan_forward, with the bound and the non-saturation condition of
    test_bigvgan_forward_matches_oracle."""
    voc, hp, W = vocs[variant]
    buf, starts = _layout(ORACLE_FRAMES, prefix=3, gap=1, seed=4)
    waves = voc.decode_ragged(buf.cuda(), starts, ORACLE_FRAMES)
    for w, s, t in zip(waves, starts, ORACLE_FRAMES):
        ref = cpu_ref.bigvgan_forward(W, hp, buf[s: s + t].t()[None])
        sat = float((ref.abs() >= 0.999).float().mean())
        err = rel_l2(w.cpu(), ref)
        print(f"decode_ragged vs oracle [{variant}], T = {t}: rel-L2 {err:.2e}, saturated {sat:.4f}")
        assert ref.shape == w.shape == (1, 1, t * UP) and sat < 0.01
        assert err < 1e-4


def test_ragged_decode_refuses_bad_extents(vocs):
    """Check 5.  Every bad extent answers F5_EINVAL before any launch (the wave buffer keeps its fill); a good call afterwards is still exact."""
    from eraxvif5tts_amd import _lib
    voc = vocs["v2"][0]
    lib = _lib.load()
    rows = torch.randn(40, 104, generator=torch.Generator().manual_seed(1)).cuda() * 2 - 3
    with pytest.raises(AssertionError):
        voc.decode_ragged(rows, [0, 35], [10, 10])  # past the end of the rows
    wave = torch.full((40 * UP,), 7.0, device="cuda")
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731

    def call(B, starts, frames, ld):
        return lib.f5_bigvgan_decode_ragged(voc.native(), B, starts, frames, _lib.ptr(rows), ld, _lib.ptr(wave), None, _lib.stream_ptr())

    bad = {"B = 0": (0, i32(0), i32(10), 104), "B < 0": (-1, i32(0), i32(10), 104), "ld < num_mels": (2, i32(0, 10), i32(10, 10), 99),
           "negative row start": (2, i32(0, -1), i32(10, 10), 104), "zero frames": (2, i32(0, 10), i32(10, 0), 104),
           "negative frames": (2, i32(0, 10), i32(10, -3), 104),
           "rows beyond 32 bits": (2, i32(0, 0), i32(1 << 22, 1 << 22), 104),        # 2^23 frames x 256 = 2^31 rows of the last stage
           "one utterance beyond 32 bits": (1, i32(0), i32((1 << 31) - 1), 104)}
    for what, args in bad.items():
        assert call(*args) == F5_EINVAL, what
        assert _lib.last_error(), what
    torch.cuda.synchronize()
    assert bool((wave == 7.0).all())
    got = voc.decode_ragged(rows, [0, 12], [10, 20])
    for w, s, t in zip(got, [0, 12], [10, 20]):
        assert torch.equal(w, voc(rows[s: s + t, :100].t()[None]))


# ---------------------------------------------------------------------------------------------------------------- wrappers
ARCH = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2, pe_attn_head=1, text_mask_padding=False)
SENTENCE = "hello there, this is a test. "
TEXT = (SENTENCE * 3 + "and one more sentence to force another chunk, because the budget is small. ") * 3


def _tts(tmp_path):
    """the tiny assets of tests/test_gpu_wave_tail.py, with the HIP BigVGAN at plug point B"""
    from eraxvif5tts_amd.infer import audio
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    W = cpu_ref.random_dit_weights(ARCH, 32, seed=25)
    VW = cpu_ref.random_vocos_weights(seed=26, dim=64, inter=128, layers=2)
    cfg_path, ckpt, vdir, vocab = _write_tiny_assets(str(tmp_path), ARCH, 32, W, dict(dim=64, intermediate_dim=128, num_layers=2), VW)
    t = np.arange(int(2.0 * SR)) / SR
    wav = 0.03 * np.sin(2 * np.pi * 190 * t + 0.7) * (1 + 0.3 * np.sin(2 * np.pi * 5 * t)) + 0.01 * np.sin(2 * np.pi * 1370 * t)
    ref_wav = os.path.join(str(tmp_path), "ref.wav")
    audio.write_wav(ref_wav, wav, SR)
    tts = F5TTSWrapper(model_name=cfg_path, ckpt_path=ckpt, vocab_file=vocab, use_local_vocoder=True, vocoder_path=vdir, precision="fp32")
    tts.preprocess_reference(ref_wav, "a quiet tone")
    tts.vocoder, tts.mel_spec_type = _bigvgan("v2", 3)[0], "bigvgan"
    return tts


class _Calls:
    """counts BigVGAN.forward and BigVGAN.decode_ragged_buffer calls while it is armed"""

    def __init__(self, monkeypatch):
        from eraxvif5tts_amd.bigvgan import BigVGAN
        self.forward = self.ragged = 0
        self.armed = False
        fwd, rag = BigVGAN.forward, BigVGAN.decode_ragged_buffer

        def forward(this, x):
            self.forward += self.armed
            return fwd(this, x)

        def decode_ragged_buffer(this, *a, **k):
            self.ragged += self.armed
            return rag(this, *a, **k)
        monkeypatch.setattr(BigVGAN, "forward", forward)
        monkeypatch.setattr(BigVGAN, "decode_ragged_buffer", decode_ragged_buffer)

    def __enter__(self):
        self.forward = self.ragged = 0
        self.armed = True
        return self

    def __exit__(self, *exc):
        self.armed = False


def _per_utterance_loop(tts, text, nfe_step, cross_fade_duration, seed):
    """generate() as it was while the generator ran per utterance: the chunks' mels from the sampler, then PER UTTERANCE the permuted slice through
    BigVGAN.forward, the rms rule with its host comparison, a copy to the host, and cross_fade_concat in numpy."""
    from eraxvif5tts_amd.infer.utils_infer import chunk_text, cross_fade_concat
    from eraxvif5tts_amd.model.utils import convert_char_to_pinyin
    secs = tts.ref_audio_processed.shape[-1] / SR
    chunks = chunk_text(text, max_chars=int(len(tts.ref_text.encode("utf-8")) / secs * (22 - secs)))
    jobs = []
    for c in chunks:
        speed = 0.3 if len(c.encode("utf-8")) < 10 else tts.speed
        jobs.append((convert_char_to_pinyin([tts.ref_text + c]),
                     tts.ref_audio_len + int(tts.ref_audio_len / len(tts.ref_text.encode("utf-8")) * len(c.encode("utf-8")) / speed)))
    torch.manual_seed(seed)
    with torch.inference_mode():
        assert len(jobs) >= 2 and min(d for _, d in jobs) >= 256
        mels = tts.model.sample_ragged(tts.ref_audio_processed, [j[0][0] for j in jobs], [j[1] for j in jobs], steps=nfe_step,
                                       cfg_strength=tts.cfg_strength, sway_sampling_coef=tts.sway_sampling_coef)
        waves = []
        for generated in mels:
            generated = generated.to(torch.float32)[:, tts.ref_audio_len:, :].permute(0, 2, 1)
            wave = tts.vocoder(generated)
            rms = torch.sqrt(torch.mean(torch.square(tts.ref_audio_processed)))
            if rms < tts.target_rms:
                wave = wave * rms / tts.target_rms
            waves.append(wave.squeeze().cpu().numpy())
    return cross_fade_concat(waves, cross_fade_duration, SR), [d - tts.ref_audio_len for _, d in jobs]


def test_generate_equals_the_per_utterance_loop(tmp_path, monkeypatch):
    """Check 6: generate() with four chunks of at least 256 frames each == the per-utterance loop, float and PCM, through ONE ragged call and no
    `forward`."""
    from eraxvif5tts_amd.infer.utils_infer import device_tail_kind
    from eraxvif5tts_amd.streaming.wire import pcm16_bytes
    tts = _tts(tmp_path)
    tts.target_rms = 0.2
    assert device_tail_kind(tts.vocoder, tts.ref_audio_processed) == "bigvgan"
    calls = _Calls(monkeypatch)
    want, gen_frames = _per_utterance_loop(tts, TEXT, 3, tts.cross_fade_duration, seed=77)
    print(f"generate() with BigVGAN: generated frames per chunk {gen_frames}, {len(want)} samples, max |x| = {np.abs(want).max():.3f}")
    assert len(gen_frames) >= 3 and min(gen_frames) >= 256 and want.dtype == np.float64 and np.abs(want).max() < 1
    with calls:
        torch.manual_seed(77)
        wave, rate = tts.generate(TEXT, nfe_step=3, return_numpy=True)
    assert (calls.ragged, calls.forward) == (1, 0)
    assert rate == SR and wave.dtype == want.dtype and np.array_equal(wave, want)
    with calls:
        torch.manual_seed(77)
        pcm, _ = tts.generate(TEXT, nfe_step=3, return_numpy=True, return_pcm16=True)
    assert (calls.ragged, calls.forward) == (1, 0)
    assert pcm.dtype == np.int16 and pcm.tobytes() == pcm16_bytes(want)


def test_infer_batch_process_equals_the_per_utterance_loop(tmp_path, monkeypatch):
    """Check 6 for utils_infer.infer_batch_process(mel_spec_type="bigvgan"): one ragged call, no `forward`, the bytes of the loop."""
    from eraxvif5tts_amd.infer import utils_infer as U
    from eraxvif5tts_amd.model.utils import convert_char_to_pinyin
    tts = _tts(tmp_path)
    model, vocoder = tts.model, tts.vocoder
    t = np.arange(int(1.5 * SR)) / SR
    a = torch.from_numpy(0.02 * np.sin(2 * np.pi * 200 * t) * (1 + 0.4 * np.sin(2 * np.pi * 2 * t))).float()[None]  # quieter than the target
    ref_text = "a quiet tone. "
    ref_text_used = ref_text + " "  # infer_batch_process appends a space behind a single-byte last character
    batches = U.chunk_text(TEXT, max_chars=60)[:3]
    calls = _Calls(monkeypatch)

    def loop(d, seed):
        rms = torch.sqrt(torch.mean(torch.square(a)))
        assert rms < 0.1
        audio = (a * 0.1 / rms).to("cuda")
        ref_len = audio.shape[-1] // 256
        jobs = [(convert_char_to_pinyin([ref_text_used + g]),
                 ref_len + int(ref_len / len(ref_text_used.encode()) * len(g.encode()) / (0.3 if len(g.encode()) < 10 else 1))) for g in batches]
        assert min(x for _, x in jobs) >= 256
        torch.manual_seed(seed)
        with torch.inference_mode():
            mels = model.sample_ragged(audio, [j[0][0] for j in jobs], [j[1] for j in jobs], steps=2, cfg_strength=2.0, sway_sampling_coef=-1)
            waves, specs = [], []
            for generated in mels:
                generated = generated.to(torch.float32)[:, ref_len:, :].permute(0, 2, 1)
                wave = vocoder(generated)
                if rms < 0.1:
                    wave = wave * rms / 0.1
                waves.append(wave.squeeze().cpu().numpy())
                specs.append(generated[0].cpu().numpy())
        return U.cross_fade_concat(waves, d), np.concatenate(specs, axis=1)

    want, want_spec = loop(0.15, 3)
    with calls:
        torch.manual_seed(3)
        wave, rate, spec = next(U.infer_batch_process((a, SR), ref_text, batches, model, vocoder, mel_spec_type="bigvgan", nfe_step=2, device="cuda",
                                                      cross_fade_duration=0.15))
    assert (calls.ragged, calls.forward) == (1, 0)
    assert rate == SR and wave.dtype == want.dtype and np.array_equal(wave, want) and np.array_equal(spec, want_spec)


def test_infer_prompts_bucket_equals_the_per_utterance_loop(monkeypatch):
    """Check 6 for eval.prompts.infer_prompts: one bucket, one ragged call; per-utterance host rms values, some applied and some not."""
    from eraxvif5tts_amd.eval import prompts as P
    from test_gpu_prompts import _cfm
    cfm = _cfm("fp32")
    voc = _bigvgan("v2", 3)[0]
    meta = P.synthetic_metainfo(14, seed=5, min_secs=3.2, max_secs=9.0)
    buckets = P.get_inference_prompt(meta, tokenizer="char", infer_batch_size=1400, num_buckets=8, min_secs=3, max_secs=40, device="cuda")
    bucket = max(buckets, key=lambda b: len(b[0]))
    utts, ref_rms, _, ref_lens, totals, _ = bucket
    assert len(utts) >= 2 and P.ragged_ok(cfm, bucket)
    target = float(sorted(float(r) for r in ref_rms)[len(ref_rms) // 2])  # the median: applied to some utterances, not to others
    assert any(r < target for r in ref_rms) and not all(r < target for r in ref_rms)
    kw = dict(nfe_step=3, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=11)
    calls = _Calls(monkeypatch)
    with calls:
        got = list(P.infer_prompts(cfm, [bucket], vocoder=voc, target_rms=target, **kw))
    assert (calls.ragged, calls.forward) == (1, 0)
    generated, _ = P.ragged_sample_fn(cfm)(**P.sample_kwargs(bucket, "cuda", 3, 2.0, -1.0, 11, False))
    assert [g[0] for g in got] == list(utts)
    for i, (_, mel, wave) in enumerate(got):
        gen = generated[i][ref_lens[i]: totals[i], :].unsqueeze(0).permute(0, 2, 1).to(torch.float32)
        want = voc(gen).squeeze(0)
        if ref_rms[i] < target:
            want = want * ref_rms[i] / target
        assert torch.equal(mel, gen) and wave.shape == want.shape and torch.equal(wave, want), utts[i]
