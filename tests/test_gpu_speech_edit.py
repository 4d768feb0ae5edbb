"""Speech editing on the native sampler: CFM.sample(edit_mask=...) through f5_sample_masked (per-frame condition mask in pack_base /
final_where, staged into the plan so hipGraph replays read the current call's mask), and infer/speech_edit.edit_speech end to end.
Stated tolerances are the ones of the matching unmasked tests: rel-L2 <= 2e-4 (fp32 mode) / 2e-2 (bf16 mode) against the reference or the
oracle, waveforms 2e-3 / 1e-1 (test_gpu_vocoder_wrapper.py)."""
import ast
import warnings

import pytest
import torch

from conftest import golden_arch, golden_weights, load_golden, rel_l2
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
TOL = {"fp32": 2e-4, "bf16": 2e-2}
SMALL = dict(dim=256, depth=2, heads=4, ff_mult=2, text_dim=128, conv_layers=2, pe_attn_head=1, text_mask_padding=False)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def _gen_rows(t, dur):
    return torch.cat([t[..., b, : int(d), :].reshape(-1, t.shape[-1]) for b, d in enumerate(dur)])


def _no_python_driver(monkeypatch):
    from eraxvif5tts_amd.model import CFM

    def boom(*a, **k):
        raise AssertionError("the edit_mask call took the Python driver")
    monkeypatch.setattr(CFM, "_sample_python", boom)


def _edit_mask(B, n, spans):
    """bool [B, n]: False over each row's [a, b) spans"""
    m = torch.ones(B, n, dtype=torch.bool)
    for b, row in enumerate(spans):
        for a, e in row:
            m[b, a:e] = False
    return m


def _small_problem(B, N, seed, nc=None, V=60):
    g = torch.Generator().manual_seed(seed)
    nc = nc or N // 2
    cond = (torch.randn(B, nc, 100, generator=g) * 2 - 3).cuda()
    text = torch.randint(0, V, (B, 24), generator=g).cuda()
    y0 = torch.randn(B, N, 100, generator=g)
    return cond, text, y0


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_edit_option_golden_on_the_native_sampler(prec, monkeypatch):
    """tests/golden/tiny_options.npz, edit case (the reference's own CFM.sample with edit_mask, B = 2 with a key mask), on the native sampler:
    the Python driver is patched to raise."""
    import gpu_helpers as G
    from test_oracle_golden import option_kwargs
    _no_python_driver(monkeypatch)
    z, zb = load_golden("tiny_options"), load_golden("tiny_base")
    c = G.make_cfm(golden_arch(zb), int(zb["vocab"]), golden_weights(zb), prec)
    ref_traj, ref_out = torch.from_numpy(z["traj_edit"]), torch.from_numpy(z["out_edit"])
    N = ref_traj.shape[2]
    dur = z["duration"].tolist()
    y0 = []
    for d in dur:
        torch.manual_seed(int(z["seed"]))
        y0.append(torch.nn.functional.pad(torch.randn(d, 100), (0, 0, 0, N - d)))
    for use_graph in (False, True, True):
        out, traj = c.sample(cond=torch.from_numpy(z["cond"]).cuda(), text=torch.from_numpy(z["text"]).cuda(), y0=torch.stack(y0),
                             use_graph=use_graph, **option_kwargs(z, "edit", as_cuda=True))
        assert out.shape == ref_out.shape and traj.shape == ref_traj.shape
        assert rel_l2(_gen_rows(traj.cpu(), dur), _gen_rows(ref_traj, dur)) < TOL[prec]
        assert rel_l2(_gen_rows(out.cpu(), dur), _gen_rows(ref_out, dur)) < TOL[prec]
        keep = torch.nn.functional.pad(torch.from_numpy(z["edit_mask"]) & cpu_ref.lens_to_mask(torch.from_numpy(z["lens"])), (0, N - 22))
        assert torch.equal(out.cpu()[keep], torch.nn.functional.pad(torch.from_numpy(z["cond"]), (0, 0, 0, N - 22))[keep])


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_native_edit_matches_the_python_driver_in_fp32_mode(B, method):
    """fp32 mode: the fused masked sampler against the Python ODE driver over DiT.forward (edit_native=False), rel-L2 <= 1e-5 on output and
    trajectory; B = 2 with different masks and durations (key mask on)."""
    import gpu_helpers as G
    zb = load_golden("tiny_base")
    c = G.make_cfm(golden_arch(zb), int(zb["vocab"]), golden_weights(zb), "fp32", method=method)
    cond, text = torch.from_numpy(zb["cond"])[:B].cuda(), torch.from_numpy(zb["text"])[:B].cuda()
    lens, dur = torch.from_numpy(zb["lens"])[:B].cuda(), torch.from_numpy(zb["duration"])[:B].cuda()
    edit = _edit_mask(B, cond.shape[1], [[(3, 9), (15, 18)], [(0, 2), (10, 20)]][:B]).cuda()
    N = int(dur.max())
    y0 = torch.randn(B, N, 100, generator=torch.Generator().manual_seed(5))
    for b in range(B):
        y0[b, int(dur[b]):] = 0
    kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=5, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, edit_mask=edit)
    nat, ntraj = c.sample(**kw)
    py, ptraj = c.sample(edit_native=False, **kw)
    d = dur.cpu()
    assert rel_l2(_gen_rows(nat.cpu(), d), _gen_rows(py.cpu(), d)) <= 1e-5
    assert rel_l2(_gen_rows(ntraj.cpu(), d), _gen_rows(ptraj.cpu(), d)) <= 1e-5
    keep = torch.nn.functional.pad(edit.cpu() & cpu_ref.lens_to_mask(lens.cpu()), (0, N - cond.shape[1]))
    assert torch.equal(nat.cpu()[keep], torch.nn.functional.pad(cond.cpu(), (0, 0, 0, N - cond.shape[1]))[keep])


@pytest.mark.parametrize("keymask", [False, True])
def test_prefix_mask_is_bit_identical_to_the_lens_form(keymask):
    """f5_sample_masked with cond_mask = (frame < lens) computes exactly what f5_sample computes: tuned bf16 kernels forced, N = 256."""
    import gpu_helpers as G
    V, B, N = 60, 2, 256
    W = cpu_ref.random_dit_weights(SMALL, V, seed=31)
    m = G.make_dit(SMALL, V, W, "bf16")
    m.set_kernels(gemm=1, attn=1)
    cond, text, y0 = _small_problem(B, N, 32)
    cond = torch.nn.functional.pad(cond, (0, 0, 0, N - cond.shape[1]))
    lens = torch.tensor([128, 97]).cuda()
    dur = torch.tensor([N, 230 if keymask else N]).cuda()
    y0[1, int(dur[1]):] = 0
    tg = cpu_ref.time_grid(6, -1.0)
    prefix = torch.arange(N, device="cuda")[None, :] < lens[:, None]
    kw = dict(use_mask=keymask, return_trajectory=True, use_graph=False)
    a, ta = m.native_sample(cond, text, lens, dur, y0, tg, 6, 2.0, **kw)
    b, tb = m.native_sample(cond, text, lens, dur, y0, tg, 6, 2.0, cond_mask=prefix, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(ta, tb)


def test_graph_replay_reads_the_current_calls_mask():
    """Capture with mask A, replay with mask B: bit-identical to an eager run with mask B (a mask baked into the capture would give A's
    result), and masked / unmasked calls of one shape keep separate captures."""
    import gpu_helpers as G
    V, B, N = 60, 2, 256
    W = cpu_ref.random_dit_weights(SMALL, V, seed=41)
    cfm = G.make_cfm(SMALL, V, W, "bf16")
    cfm.transformer.set_kernels(gemm=1, attn=1)
    cond, text, y0 = _small_problem(B, N, 42, nc=200)
    lens, dur = torch.tensor([200, 180]).cuda(), torch.tensor([N, N]).cuda()
    mask_a = _edit_mask(B, 200, [[(10, 60)], [(100, 150)]]).cuda()
    mask_b = _edit_mask(B, 200, [[(120, 190)], [(5, 40), (60, 70)]]).cuda()
    kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, return_trajectory=False)
    eager_a, _ = cfm.sample(edit_mask=mask_a, use_graph=False, **kw)
    eager_b, _ = cfm.sample(edit_mask=mask_b, use_graph=False, **kw)
    plain, _ = cfm.sample(use_graph=False, **kw)
    assert not torch.equal(eager_a, eager_b)
    graph_a, _ = cfm.sample(edit_mask=mask_a, use_graph=True, **kw)  # capture
    graph_b, _ = cfm.sample(edit_mask=mask_b, use_graph=True, **kw)  # replay of A's capture
    graph_plain, _ = cfm.sample(use_graph=True, **kw)                # a capture of its own
    graph_b2, _ = cfm.sample(edit_mask=mask_b, use_graph=True, **kw)
    assert torch.equal(graph_a, eager_a)
    assert torch.equal(graph_b, eager_b) and torch.equal(graph_b2, eager_b)
    assert torch.equal(graph_plain, plain)


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_full_size_masked_bf16_against_fp32_mode(method):
    """F5TTS_Base, B = 2, N = 1024 (durations 1024 / 900: key mask on), tuned kernels forced (gemm_w4 + LayerNorm fold + wide attention),
    the masked bf16 path against the fp32 parity mode with the same mask: rel-L2 <= 2e-2 on the generated frames (the tolerance of the
    unmasked test_true_depth_bf16_sampler_stays_within_tolerance_of_fp32_mode); every kept frame equals cond exactly."""
    import bench
    import gpu_helpers as G
    from eraxvif5tts_amd.model import CFM, DiT
    B, N = 2, 1024
    cond, text, lens, dur = bench.synth_batch(B, N, "cuda", seed=51)
    dur[1] = 900
    nc = cond.shape[1]
    edit = _edit_mask(B, nc, [[(40, 120), (nc - 30, nc)], [(0, 25), (150, 200)]]).cuda()
    g = torch.Generator().manual_seed(52)
    y0 = torch.randn(B, N, 100, generator=g)
    y0[1, 900:] = 0
    steps = 32 if method == "euler" else 16
    kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=steps, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0,
              return_trajectory=False, edit_mask=edit)
    outs = {}
    with G.knobs(gemm_w4=1, ln_fold=1):
        for prec in ("fp32", "bf16"):
            torch.manual_seed(1234)
            model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision=prec), seed=0)
            if prec == "bf16":
                model.set_kernels(gemm=1, attn=1)
            cfm = CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}, odeint_kwargs={"method": method}).cuda()
            outs[prec] = cfm.sample(use_graph=False, **kw)[0].cpu()
            if prec == "bf16":
                assert torch.equal(cfm.sample(use_graph=True, **kw)[0].cpu(), outs[prec])
                assert model.residual_fallbacks() == 0
            del cfm, model
            torch.cuda.empty_cache()
    keep = torch.nn.functional.pad(edit.cpu() & cpu_ref.lens_to_mask(lens.cpu()), (0, N - nc))
    regen = ~keep & cpu_ref.lens_to_mask(dur.cpu(), N)
    err = rel_l2(outs["bf16"][regen], outs["fp32"][regen])
    print(f"masked {method}, 22 blocks x {steps} steps: bf16 vs fp32 mode rel-L2 {err:.3e}")
    assert torch.isfinite(outs["bf16"]).all() and err < 2e-2
    cond_p = torch.nn.functional.pad(cond.cpu(), (0, 0, 0, N - nc))
    assert torch.equal(outs["bf16"][keep], cond_p[keep]) and torch.equal(outs["fp32"][keep], cond_p[keep])


@pytest.mark.parametrize("backbone", ["UNetT", "MMDiT"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_other_backbones_with_an_edit_mask_match_the_oracle(backbone, prec, monkeypatch):
    """The tiny UNetT / MMDiT goldens' architectures (both inherit native_sample) with an edit mask, B = 2 with a key mask, on the native
    sampler, against cpu_ref.sample(edit_mask=...)."""
    from eraxvif5tts_amd.model import CFM, MMDiT, UNetT
    _no_python_driver(monkeypatch)
    z = load_golden({"UNetT": "tiny_unett", "MMDiT": "tiny_mmdit"}[backbone])
    arch = ast.literal_eval(str(z["a.arch"]))
    V = int(z["a.vocab"])
    rand = {"UNetT": cpu_ref.random_unett_weights, "MMDiT": cpu_ref.random_mmdit_weights}[backbone]
    W = rand(arch, V, seed=int(z["a.seed"]))
    m = {"UNetT": UNetT, "MMDiT": MMDiT}[backbone](**arch, text_num_embeds=V, mel_dim=100, precision=prec)
    sd = m.state_dict()
    m.load_state_dict({k: v for k, v in W.items() if k in sd}, strict=False)
    cfm = CFM(transformer=m.cuda(), mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()
    g = lambda k: torch.from_numpy(z[f"a.{k}"])
    cond, text, lens, dur = g("cond")[:, :16], g("text"), g("lens"), g("duration")
    edit = _edit_mask(2, 16, [[(2, 7)], [(0, 3), (9, 12)]])
    y0 = g("sample_traj")[0]
    ref, ref_traj = cpu_ref.sample(W, {**arch, "backbone": backbone}, cond, text, dur, lens=lens, steps=4, cfg_strength=2.0,
                                   sway_sampling_coef=-1.0, y0=y0, edit_mask=edit)
    for use_graph in (False, True, True):
        out, traj = cfm.sample(cond=cond.cuda(), text=text.cuda(), duration=dur.cuda(), lens=lens.cuda(), steps=4, cfg_strength=2.0,
                               sway_sampling_coef=-1.0, y0=y0, edit_mask=edit.cuda(), use_graph=use_graph)
        assert rel_l2(_gen_rows(out.cpu(), dur), _gen_rows(ref, dur)) < TOL[prec]
        assert rel_l2(_gen_rows(traj.cpu(), dur), _gen_rows(ref_traj, dur)) < TOL[prec]


def test_deferred_guard_and_fp32_fallback_keep_the_staged_mask():
    """defer_guard=True + finish_pending() gives the synchronous call's output bit for bit; and on a checkpoint that leaves the fp16 range the
    fallback rerun (deferred to finish_pending) reuses the staged mask: equal to a run with fp32 residual storage from the start."""
    import gpu_helpers as G
    V, B, N = 60, 2, 96
    W = cpu_ref.random_dit_weights(SMALL, V, seed=77)
    cond, text, y0 = _small_problem(B, N, 78, nc=30)
    lens, dur = torch.tensor([30, 24]).cuda(), torch.tensor([96, 80]).cuda()
    y0[1, 80:] = 0
    edit = _edit_mask(B, 30, [[(4, 12)], [(0, 6), (18, 22)]]).cuda()
    kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, edit_mask=edit)

    cfm = G.make_cfm(SMALL, V, W, "bf16")
    sync, straj = cfm.sample(use_graph=False, **kw)
    deferred, dtraj = cfm.sample(use_graph=False, defer_guard=True, **kw)
    cfm.transformer.finish_pending()
    assert torch.equal(sync, deferred) and torch.equal(straj, dtraj)

    big = dict(W)
    for k in ("input_embed.proj.weight", "input_embed.proj.bias"):
        big[k] = W[k] * 3.0e5
    cfm = G.make_cfm(SMALL, V, big, "bf16")
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        out, traj = cfm.sample(use_graph=False, defer_guard=True, **kw)
        cfm.transformer.finish_pending()
    assert cfm.transformer.residual_fallbacks() == 1 and torch.isfinite(out).all()
    with G.knobs(residual_f16=0):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ref, ref_traj = G.make_cfm(SMALL, V, big, "bf16").sample(use_graph=False, **kw)
    assert torch.equal(out, ref) and torch.equal(traj, ref_traj)
    keep = torch.nn.functional.pad(edit & cpu_ref.lens_to_mask(lens.cpu()).cuda(), (0, N - 30))
    assert torch.equal(out[keep], torch.nn.functional.pad(cond, (0, 0, 0, N - 30))[keep])


def _tiny_tts(tmp_path, prec):
    from test_gpu_vocoder_wrapper import _write_tiny_assets
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    arch = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2, pe_attn_head=1, text_mask_padding=False)
    V = 32
    W = cpu_ref.random_dit_weights(arch, V, seed=25)
    hp = dict(dim=64, intermediate_dim=128, num_layers=2)
    VW = cpu_ref.random_vocos_weights(seed=26, dim=64, inter=128, layers=2)
    cfg_path, ckpt, vdir, vocab = _write_tiny_assets(str(tmp_path), arch, V, W, hp, VW)
    tts = F5TTSWrapper(model_name=cfg_path, ckpt_path=ckpt, vocab_file=vocab, use_local_vocoder=True, vocoder_path=vdir, precision=prec)
    tts.model.noise_device = "cpu"  # the noise the reference's CPU path draws for the same seed
    mel_fn = lambda a: tts.model.mel_spec(a[None].cuda()).permute(0, 2, 1)[0].cpu()  # noqa: E731
    return tts, arch, W, VW, mel_fn


def _tone(seconds, f0, sr=24000):
    import numpy as np
    t = torch.arange(int(seconds * sr), dtype=torch.float64) / sr
    w = 0.03 * torch.sin(2 * np.pi * f0 * t + 0.7) * (1 + 0.3 * torch.sin(2 * np.pi * 5 * t)) + 0.01 * torch.sin(2 * np.pi * 1370 * t)
    return w.float()


def _oracle_edit(arch, W, VW, vmap, waves, texts, parts, fixes, seed, nfe, mel_fn, hop=256):
    """reference infer/speech_edit.py:126-189 on the CPU oracle, the jobs as one padded batch: rms boost, mel (mel_fn: the device front end,
    which test_gpu_frontend.py pins to cpu_ref.mel_spectrogram on its own), cpu_ref.sample(edit_mask=...), each job's frames (its resolved
    duration) -> Vocos -> rms restore.  -> ([wave [1, n]], [mel [1, 100, frames]], [kept frames: bool [frames]])"""
    from torch.nn.utils.rnn import pad_sequence
    from eraxvif5tts_amd.infer.speech_edit import build_edit_mask
    from eraxvif5tts_amd.model.utils import convert_char_to_pinyin, list_str_to_idx
    rmss, conds, masks, durs = [], [], [], []
    for wave, pts, fix in zip(waves, parts, fixes):
        # the rms boost as edit_speech computes it (on the device): a last-bit difference in the gain moves weak log-mel bins of the front end
        # by up to ~2e-2 (inside its stated bound), which would then be compared as if it were sampler error
        audio = wave.cuda()
        rms = torch.sqrt(torch.mean(torch.square(audio)))
        audio = (audio * 0.1 / rms if rms < 0.1 else audio).cpu()
        rms = rms.cpu()
        rmss.append(rms)
        conds.append(mel_fn(audio))
        masks.append(build_edit_mask(audio.shape[-1], pts, fix, hop_length=hop))
        durs.append(audio.shape[-1] // hop)
    lens = torch.tensor([c.shape[0] for c in conds])
    ids = list_str_to_idx(convert_char_to_pinyin(list(texts)), vmap)
    dur = torch.tensor(durs)
    out, _ = cpu_ref.sample(W, arch, pad_sequence(conds, batch_first=True), ids, dur, lens=lens, steps=nfe, cfg_strength=2.0,
                            sway_sampling_coef=-1.0, seed=seed, edit_mask=pad_sequence(masks, batch_first=True, padding_value=True),
                            return_trajectory=False)
    frames = torch.maximum(torch.maximum((ids != -1).sum(-1), lens) + 1, dur).tolist()
    ws, ms, keeps = [], [], []
    for i, n in enumerate(frames):
        mel = out[i : i + 1, :n].float().permute(0, 2, 1)
        w = cpu_ref.vocos_decode(VW, mel).reshape(1, -1)
        ws.append(w * rmss[i] / 0.1 if rmss[i] < 0.1 else w)
        ms.append(mel)
        keeps.append(torch.nn.functional.pad(masks[i], (0, n - masks[i].shape[0]), value=False))
    return ws, ms, keeps


def _check_edit_mel(got, ref, keep, tol):
    """regenerated frames: the sampler's tolerance; kept frames: the prompt's mel itself, exactly"""
    got = got.cpu()
    err = rel_l2(got[..., ~keep], ref[..., ~keep])
    assert err < tol, err
    assert torch.equal(got[..., keep], ref[..., keep])
    return err


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_edit_speech_end_to_end_matches_the_oracle_chain(tmp_path, prec, monkeypatch):
    """edit_speech on a 2 s synthetic wave with random tiny weights (HIP mel, masked native sampler, HIP Vocos) against the reference script's
    chain on the oracle from the same prompt mel (cpu_ref.sample(edit_mask=...) -> Vocos -> rms restore), same seed; regenerated mel frames
    rel-L2 <= 2e-4 / 2e-2, kept frames = the prompt mel, wave 2e-3 / 1e-1."""
    from eraxvif5tts_amd.infer.speech_edit import edit_speech
    _no_python_driver(monkeypatch)
    tts, arch, W, VW, mel_fn = _tiny_tts(tmp_path, prec)
    wave = _tone(2.0, 190)
    text, parts, fix = "a quiet tone, edited.", [[0.3, 0.7], [1.2, 1.5]], [0.5, 0.3]
    got_w, got_m = edit_speech(tts.model, tts.vocoder, wave.cuda(), 24000, text, parts, fix_duration=fix, nfe_step=4, seed=11)
    (ref_w,), (ref_m,), (keep,) = _oracle_edit(arch, W, VW, tts.vocab_char_map, [wave], [text], [parts], [fix], 11, 4, mel_fn)
    assert got_m.shape == ref_m.shape and got_w.shape == ref_w.shape
    assert 0 < int(keep.sum()) < keep.shape[0]
    mel_err, wave_err = _check_edit_mel(got_m, ref_m, keep, TOL[prec]), rel_l2(got_w.cpu(), ref_w)
    print(f"edit_speech vs oracle [{prec}]: regenerated mel rel-L2 {mel_err:.2e}, wave rel-L2 {wave_err:.2e}")
    assert wave_err < {"fp32": 2e-3, "bf16": 1e-1}[prec]


def test_edit_speech_batch_of_jobs(tmp_path, monkeypatch):
    """A list of edit jobs runs as one padded batch (B = 2: one mask per job, different lengths -> key mask on), against the same batch on
    the oracle chain (fp32 mode)."""
    from eraxvif5tts_amd.infer.speech_edit import edit_speech
    _no_python_driver(monkeypatch)
    tts, arch, W, VW, mel_fn = _tiny_tts(tmp_path, "fp32")
    calls = []
    native = tts.model.transformer.native_sample

    def spy(*a, **k):
        calls.append((a[0].shape[0], k.get("use_mask"), k.get("cond_mask") is not None))
        return native(*a, **k)
    monkeypatch.setattr(tts.model.transformer, "native_sample", spy)
    waves = [_tone(2.0, 190), _tone(1.5, 240)]
    texts = ["a quiet tone, edited.", "another one."]
    parts = [[[0.3, 0.7], [1.2, 1.5]], [[0.5, 0.9]]]
    fixes = [[0.5, 0.3], None]
    got_w, got_m = edit_speech(tts.model, tts.vocoder, [w.cuda() for w in waves], 24000, texts, parts, fix_duration=fixes, nfe_step=4, seed=3)
    assert calls == [(2, True, True)]
    ref_w, ref_m, keeps = _oracle_edit(arch, W, VW, tts.vocab_char_map, waves, texts, parts, fixes, 3, 4, mel_fn)
    for i in range(2):
        assert got_m[i].shape == ref_m[i].shape and got_w[i].shape == ref_w[i].shape
        _check_edit_mel(got_m[i], ref_m[i], keeps[i], TOL["fp32"])
        assert rel_l2(got_w[i].cpu(), ref_w[i]) < 2e-3
