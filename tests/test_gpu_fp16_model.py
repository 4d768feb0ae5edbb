"""The fp16 precision mode (F5_PREC_FP16, include/f5hip.h) at model level: DiT / CFM composed with precision="fp16" against the golden
vectors captured from the reference, the CPU oracle and the library's own exact-fp32 mode.

Stated tolerances: final mel rel-L2 <= 5e-3, per stage <= 3.75e-3 -- this project's bf16 contract (2e-2 / 1.5e-2, tests/test_gpu_model.py)
divided by 4: three more mantissa bits give 8, half of that is margin for the parts that are fp32 or fp16 in both modes."""
import ast
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
import yaml

from conftest import golden_arch, golden_weights, load_golden, rel_l2
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
TOL, STAGE_TOL = 5e-3, 3.75e-3
BASE = dict(dim=1024, depth=22, heads=16, ff_mult=2, text_dim=512, text_mask_padding=False, conv_layers=4, pe_attn_head=1)  # configs/F5TTS_Base.yaml
BASE_VOCAB, BASE_SEED = 2545, 1234


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@pytest.fixture(params=["reference-kernels", "tuned-kernels"])
def kernels(request, monkeypatch):
    """as tests/test_gpu_model.py: reference tile kernels only / tuned kernels forced wherever they support the problem"""
    v = "0" if request.param == "reference-kernels" else "1"
    monkeypatch.setenv("F5HIP_GEMM_KERNEL", v)
    monkeypatch.setenv("F5HIP_ATTN_KERNEL", v)
    return request.param


def _gen_rows(t, dur):
    return torch.cat([t[..., b, : int(d), :].reshape(-1, t.shape[-1]) for b, d in enumerate(dur)])


# ----------------------------------------------------------------------------- 1. the tiny goldens
@pytest.mark.parametrize("name", ["tiny_base", "tiny_v1"])
def test_forward_of_both_cfg_branches(name, kernels):
    import gpu_helpers as G
    z = load_golden(name)
    arch, W = golden_arch(z), golden_weights(z)
    m = G.make_dit(arch, int(z["vocab"]), W, "fp16")
    x, cond, text = [torch.from_numpy(z[k]).cuda() for k in ("trace_x", "trace_cond", "text")]
    mask = cpu_ref.lens_to_mask(torch.from_numpy(z["duration"])).cuda()
    t = torch.from_numpy(z["trace_t"]).cuda()
    for drop, tag in ((False, "trc"), (True, "tru")):
        out = m(x=x, cond=cond, text=text, time=t, mask=mask, drop_audio_cond=drop, drop_text=drop, cache=False)
        err = rel_l2(out.cpu(), z[f"{tag}.out"])
        print(f"  {name} {tag} [{kernels}]: {err:.2e}")
        assert err < STAGE_TOL


@pytest.mark.parametrize("name", ["tiny_base", "tiny_v1"])
def test_sample_matches_reference_golden(name, kernels):
    import gpu_helpers as G
    z = load_golden(name)
    arch, W = golden_arch(z), golden_weights(z)
    c = G.make_cfm(arch, int(z["vocab"]), W, "fp16")
    kw = dict(cond=torch.from_numpy(z["cond"]).cuda(), text=torch.from_numpy(z["text"]).cuda(), duration=torch.from_numpy(z["duration"]).cuda(),
              lens=torch.from_numpy(z["lens"]).cuda(), steps=int(z["steps"]), cfg_strength=float(z["cfg_strength"]),
              sway_sampling_coef=float(z["sway"]), y0=torch.from_numpy(z["y0"]))
    dur = z["duration"]
    outs = []
    for graph in (False, True, True):
        out, traj = c.sample(use_graph=graph, **kw)
        e_out = rel_l2(_gen_rows(out.cpu(), dur), _gen_rows(torch.from_numpy(z["out"]), dur))
        e_traj = rel_l2(_gen_rows(traj.cpu(), dur), _gen_rows(torch.from_numpy(z["traj"]), dur))
        print(f"  {name} graph={graph} [{kernels}]: out {e_out:.2e} traj {e_traj:.2e}")
        assert e_out < TOL and e_traj < TOL
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])  # graph replay is bit-equal to eager
    assert c.transformer.residual_fallbacks() == 0


# ----------------------------------------------------------------------------- 2. / 3. against the fp32 mode, production kernels
def _base_problem(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    nc = 200
    cond = (torch.randn(B, nc, 100, generator=g) * 2 - 3).cuda()
    text = torch.randint(0, BASE_VOCAB, (B, 120), generator=g).cuda()
    y0 = torch.randn(B, N, 100, generator=g)
    return nc, dict(cond=cond, text=text, duration=N, steps=2, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, return_trajectory=False, use_graph=False)


def _run(arch, V, W, prec, kw):
    import gpu_helpers as G
    cfm = G.make_cfm(arch, V, W, prec)
    out = cfm.sample(**kw)[0].cpu()
    fb = cfm.transformer.residual_fallbacks()
    del cfm
    torch.cuda.empty_cache()
    return out, fb


def test_fp16_is_closer_to_fp32_than_bf16_tiny():
    z = load_golden("tiny_v1")
    arch, V, W = golden_arch(z), int(z["vocab"]), golden_weights(z)
    kw = dict(cond=torch.from_numpy(z["cond"]).cuda(), text=torch.from_numpy(z["text"]).cuda(), duration=torch.from_numpy(z["duration"]).cuda(),
              lens=torch.from_numpy(z["lens"]).cuda(), steps=int(z["steps"]), cfg_strength=float(z["cfg_strength"]),
              sway_sampling_coef=float(z["sway"]), y0=torch.from_numpy(z["y0"]), return_trajectory=False, use_graph=False)
    dur = z["duration"]
    outs = {p: _gen_rows(_run(arch, V, W, p, kw)[0], dur) for p in ("fp32", "bf16", "fp16")}
    e16, eb = rel_l2(outs["fp16"], outs["fp32"]), rel_l2(outs["bf16"], outs["fp32"])
    print(f"  tiny_v1 against the fp32 mode: fp16 mode {e16:.3e}, bf16 mode {eb:.3e}")
    assert e16 < eb


def test_fp16_is_closer_to_fp32_than_bf16_base_arch():
    """F5TTS_Base arch, B = 1, N = 512, NFE 2, CFG 2: 1024 token rows, so the LayerNorm fold and the tuned kernels run."""
    W = cpu_ref.random_dit_weights(BASE, BASE_VOCAB, seed=BASE_SEED)
    nc, kw = _base_problem(1, 512, 31)
    outs = {p: _run(BASE, BASE_VOCAB, W, p, kw)[0][:, nc:] for p in ("fp32", "bf16", "fp16")}
    e16, eb = rel_l2(outs["fp16"], outs["fp32"]), rel_l2(outs["bf16"], outs["fp32"])
    print(f"  F5TTS_Base 1 x 512 against the fp32 mode: fp16 mode {e16:.3e}, bf16 mode {eb:.3e}")
    assert e16 < eb


def test_production_kernels_at_a_production_shape():
    """F5TTS_Base arch, B = 2 x 1024, NFE 2, CFG 2: 4096 token rows, so the 256-row one-wave-per-SIMD tiles, the LayerNorm fold and the wide
    attention kernel all run; the fp16 mode stays within 5e-3 of the fp32 mode, with no range-guard fallback."""
    from eraxvif5tts_amd import _lib
    import gpu_helpers as G
    W = cpu_ref.random_dit_weights(BASE, BASE_VOCAB, seed=BASE_SEED)
    nc, kw = _base_problem(2, 1024, 32)
    ref, _ = _run(BASE, BASE_VOCAB, W, "fp32", kw)
    cfm = G.make_cfm(BASE, BASE_VOCAB, W, "fp16")
    out = cfm.sample(**kw)[0].cpu()
    v = C.c_int(-1)
    (_, h), = cfm.transformer._plans
    _lib.check(_lib.load().f5_plan_get_option(h, b"ln_fold_active", C.byref(v)))
    assert v.value == 1
    err = rel_l2(out[:, nc:], ref[:, nc:])
    print(f"  F5TTS_Base 2 x 1024 fp16 mode against the fp32 mode: {err:.3e}")
    assert torch.isfinite(out).all() and err < TOL
    assert cfm.transformer.residual_fallbacks() == 0


# ----------------------------------------------------------------------------- 4. ragged equals batch-1
@pytest.mark.parametrize("fixture", ["tiny_base", "tiny_v1"])
def test_ragged_sample_equals_batch1_samples(fixture):
    import gpu_helpers as G
    z = load_golden(fixture)
    arch, V, W = golden_arch(z), int(z["vocab"]), golden_weights(z)
    cfm = G.make_cfm(arch, V, W, "fp16", method="midpoint")
    g = torch.Generator().manual_seed(77)
    nc = 90
    cond = (torch.randn(1, nc, 100, generator=g) * 2 - 3).cuda()
    durs = [300, 257, 411]
    texts = [torch.randint(0, V, (1, n), generator=g).cuda() for n in (31, 12, 45)]
    y0s = [torch.randn(1, d, 100, generator=g).cuda() for d in durs]
    kw = dict(steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0)
    ref = [cfm.sample(cond=cond, text=t, duration=d, y0=y, return_trajectory=False, use_graph=False, **kw)[0] for t, d, y in zip(texts, durs, y0s)]
    got = cfm.sample_ragged(cond, texts, durs, y0s=y0s, **kw)
    for a, b, d in zip(got, ref, durs):
        assert a.shape == (1, d, 100) and torch.isfinite(a).all()
        assert torch.equal(a, b), (d, float((a - b).abs().max()))


# ----------------------------------------------------------------------------- 5. range guard
def test_residual_range_guard_falls_back_to_fp32_storage():
    """The checkpoint of test_fp16_residual_range_guard_falls_back_to_fp32_storage in fp16 mode: one warning, one fallback, finite output."""
    import gpu_helpers as G
    arch = dict(dim=256, depth=2, heads=4, ff_mult=2, text_dim=128, conv_layers=2, pe_attn_head=1, text_mask_padding=False)
    V = 60
    W = cpu_ref.random_dit_weights(arch, V, seed=77)
    big = dict(W)
    for k in ("input_embed.proj.weight", "input_embed.proj.bias"):
        big[k] = W[k] * 3.0e5 / 8.0  # (3e5 / 8 x the unit-scale weights stays finite in fp16; the stream still leaves the range)
    assert float(big["input_embed.proj.weight"].abs().max()) < 65504.0
    g = torch.Generator().manual_seed(78)
    B, N = 2, 96
    cond = (torch.randn(B, 30, 100, generator=g) * 2 - 3).cuda()
    text = torch.randint(0, V, (B, 20), generator=g).cuda()
    lens, dur = torch.tensor([30, 24]).cuda(), torch.tensor([96, 80]).cuda()
    y0 = torch.randn(B, N, 100, generator=g)
    y0[1, 80:] = 0
    kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, return_trajectory=False)
    cfm = G.make_cfm(arch, V, big, "fp16")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out, _ = cfm.sample(use_graph=True, **kw)
    assert sum("fp16 range" in str(w.message) for w in caught) == 1
    assert cfm.transformer.residual_fallbacks() == 1 and torch.isfinite(out).all()
    small = G.make_cfm(arch, V, W, "fp16")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        small.sample(use_graph=False, **kw)
    assert small.transformer.residual_fallbacks() == 0


# ----------------------------------------------------------------------------- 6. options, the other backbones
def test_plan_options_of_an_fp16_plan():
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    z = load_golden("tiny_base")
    arch, V, W = golden_arch(z), int(z["vocab"]), golden_weights(z)
    m = G.make_dit(arch, V, W, "fp16")
    plan = m.plan(2, 64, 2)
    v = C.c_int(-1)
    _lib.check(lib.f5_plan_set_option(plan, b"attn_prescale", 1))
    _lib.check(lib.f5_plan_get_option(plan, b"attn_prescale_active", C.byref(v)))
    assert v.value == 0
    _lib.check(lib.f5_plan_get_option(plan, b"residual_f16", C.byref(v)))
    assert v.value == 1
    assert lib.f5_plan_set_attn_dropout(plan, 0.1, 7) == _lib.F5_ENOTSUP and b"fp16" in lib.f5_last_error()
    assert lib.f5_plan_set_attn_dropout(plan, 0.0, 0) == 0
    with pytest.raises(NotImplementedError):
        m.set_attn_dropout(0.1)


def test_unett_forward_against_the_oracle():
    from eraxvif5tts_amd.model import UNetT
    z = load_golden("tiny_unett")
    for tag in ("a", "b"):
        arch = ast.literal_eval(str(z[f"{tag}.arch"]))
        V = int(z[f"{tag}.vocab"])
        W = cpu_ref.random_unett_weights(arch, V, seed=int(z[f"{tag}.seed"]))
        m = UNetT(**arch, text_num_embeds=V, mel_dim=100, precision="fp16")
        m.load_state_dict({k: v for k, v in W.items() if k in m.state_dict()}, strict=False)
        m = m.cuda()
        x, cond, text, mask, t = [torch.from_numpy(z[f"{tag}.{k}"]) for k in ("x", "cond", "text", "mask", "t")]
        for drop in (False, True):
            ref = cpu_ref.unett_forward(W, arch, x, cond, text, t, drop, drop, mask=mask)
            out = m(x=x.cuda(), cond=cond.cuda(), text=text.cuda(), time=t.cuda(), mask=mask.cuda(), drop_audio_cond=drop, drop_text=drop)
            err = rel_l2(out.cpu()[mask], ref[mask])
            print(f"  UNetT {tag} drop={drop}: {err:.2e}")
            assert err < STAGE_TOL


def test_mmdit_forward_against_the_oracle():
    from eraxvif5tts_amd.model import MMDiT
    z = load_golden("tiny_mmdit")
    for tag in ("a", "b"):
        arch = ast.literal_eval(str(z[f"{tag}.arch"]))
        V = int(z[f"{tag}.vocab"])
        W = cpu_ref.random_mmdit_weights(arch, V, seed=int(z[f"{tag}.seed"]))
        m = MMDiT(**arch, text_num_embeds=V, mel_dim=100, precision="fp16")
        m.load_state_dict({**W, "rotary_embed.inv_freq": m.state_dict()["rotary_embed.inv_freq"]}, strict=True)
        m = m.cuda()
        x, cond, text, mask, t = [torch.from_numpy(z[f"{tag}.{k}"]) for k in ("x", "cond", "text", "mask", "t")]
        for drop in (False, True):
            ref = cpu_ref.mmdit_forward(W, arch, x, cond, text, t, drop, drop, mask=mask)
            out = m(x=x.cuda(), cond=cond.cuda(), text=text.cuda(), time=t.cuda(), mask=mask.cuda(), drop_audio_cond=drop, drop_text=drop)
            err = rel_l2(out.cpu()[mask], ref[mask])
            print(f"  MMDiT {tag} drop={drop}: {err:.2e}")
            assert err < STAGE_TOL


# ----------------------------------------------------------------------------- 7. the wrapper
def _write_tiny_assets(tmp, arch, V, W, vocos_hp, VW):
    cfg = {"model": {"name": "tiny_custom", "backbone": "DiT", "arch": arch,
                     "mel_spec": {"target_sample_rate": 24000, "n_mel_channels": 100, "hop_length": 256, "win_length": 1024, "n_fft": 1024,
                                  "mel_spec_type": "vocos"}}}
    cfg_path = os.path.join(tmp, "tiny_custom.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    ema = {"ema_model.transformer." + k: v for k, v in W.items()}
    ema.update({"initted": torch.tensor(True), "step": torch.tensor(7), "ema_model.mel_spec.mel_stft.spectrogram.window": torch.hann_window(1024)})
    ckpt = os.path.join(tmp, "model_7.pt")
    torch.save({"ema_model_state_dict": ema}, ckpt)
    vdir = os.path.join(tmp, "vocos")
    os.makedirs(vdir)
    with open(os.path.join(vdir, "config.yaml"), "w") as f:
        yaml.safe_dump({"feature_extractor": {"init_args": {"n_fft": 1024, "hop_length": 256, "n_mels": 100}},
                        "backbone": {"init_args": {"input_channels": 100, "dim": vocos_hp["dim"], "intermediate_dim": vocos_hp["intermediate_dim"],
                                                   "num_layers": vocos_hp["num_layers"]}},
                        "head": {"init_args": {"dim": vocos_hp["dim"], "n_fft": 1024, "hop_length": 256}}}, f)
    torch.save({**VW, "feature_extractor.mel_spec.spectrogram.window": torch.hann_window(1024)}, os.path.join(vdir, "pytorch_model.bin"))
    vocab = os.path.join(tmp, "vocab.txt")
    with open(vocab, "w", encoding="utf-8") as f:
        f.write(" \n" + "\n".join(list("abcdefghijklmnopqrstuvwxyz.,!?'")) + "\n")
    return cfg_path, ckpt, vdir, vocab


def test_wrapper_generate_matches_the_oracle_chain(tmp_path):
    """The prec = "fp16" leg of the chain test_generate_end_to_end_matches_the_oracle_chain builds (tests/test_gpu_vocoder_wrapper.py): wav ->
    preprocess_reference -> generate() with two text chunks against cpu_ref.generate_chain.  Mel within 5e-3, wave within 2.5e-2 (the bf16
    bound of 1e-1 divided by 4)."""
    from eraxvif5tts_amd.infer import audio
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    from eraxvif5tts_amd.infer.utils_infer import chunk_text
    from eraxvif5tts_amd.model.utils import convert_char_to_pinyin, list_str_to_idx
    from eraxvif5tts_amd import _lib
    arch = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2, pe_attn_head=1, text_mask_padding=False)
    V = 32
    W = cpu_ref.random_dit_weights(arch, V, seed=25)
    hp = dict(dim=64, intermediate_dim=128, num_layers=2)
    VW = cpu_ref.random_vocos_weights(seed=26, dim=64, inter=128, layers=2)
    cfg_path, ckpt, vdir, vocab = _write_tiny_assets(str(tmp_path), arch, V, W, hp, VW)
    sr = 24000
    t = np.arange(int(2.0 * sr)) / sr
    wav = 0.03 * np.sin(2 * np.pi * 190 * t + 0.7) * (1 + 0.3 * np.sin(2 * np.pi * 5 * t)) + 0.01 * np.sin(2 * np.pi * 1370 * t)
    ref_wav = os.path.join(str(tmp_path), "ref.wav")
    audio.write_wav(ref_wav, wav, sr)
    pcm = np.clip(np.round(wav * 32767.0), -32768, 32767).astype(np.float32) / np.float32(32768.0)
    prompt = torch.from_numpy(np.concatenate([pcm, np.zeros(int(0.05 * sr), np.float32)]))[None]
    prompt = prompt * 0.1 / torch.sqrt(torch.mean(torch.square(prompt)))

    tts = F5TTSWrapper(model_name=cfg_path, ckpt_path=ckpt, vocab_file=vocab, use_local_vocoder=True, vocoder_path=vdir, precision="fp16")
    assert tts.model.transformer.precision == _lib.F5_PREC_FP16
    tts.model.noise_device = "cpu"
    aud, ref_text = tts.preprocess_reference(ref_wav, "a quiet tone")
    text = "hello there, this is a test. " * 3 + "and one more sentence to force a second chunk, because the budget is small."
    max_chars = int(len(ref_text.encode()) / (prompt.shape[-1] / sr) * (22 - prompt.shape[-1] / sr))
    chunks = chunk_text(text, max_chars=max_chars)
    assert len(chunks) == 2
    torch.manual_seed(1234)
    wave, rate, spec = tts.generate(text, nfe_step=4, return_numpy=True, return_spectrogram=True)
    vmap = tts.vocab_char_map
    oracle_chunks = [(list_str_to_idx(convert_char_to_pinyin([ref_text + c]), vmap), len(c.encode("utf-8"))) for c in chunks]
    torch.manual_seed(1234)
    ref_wave, ref_mels = cpu_ref.generate_chain(W, arch, VW, prompt, len(ref_text.encode("utf-8")), oracle_chunks, nfe_step=4)
    ref_spec = np.concatenate(ref_mels, axis=1)
    assert spec.shape == ref_spec.shape and wave.shape == ref_wave.shape
    mel_err, wave_err = rel_l2(spec, ref_spec), rel_l2(wave, ref_wave)
    print(f"  generate() vs oracle chain [fp16]: mel rel-L2 {mel_err:.2e}, wave rel-L2 {wave_err:.2e}")
    assert mel_err < 5e-3
    assert wave_err < 2.5e-2
