"""Model widths other than the 128 / 256 / 512 / 1024 the rest of the suite builds: the two shipped Small configs (configs/F5TTS_Small.yaml:
DiT, dim 768, 12 heads, text_dim 512, 4 text blocks, ff_mult 2; configs/E2TTS_Small.yaml: UNetT, dim 768, 12 heads, ff_mult 4) and the other
widths f5_model_create() accepts (dim % 128 == 0 up to 2048, any head count, mel_dim % 4 == 0 up to 128, text_dim % 4 == 0 -- % 32 with text
blocks --, ff_inner % 32 == 0), through CFM.sample(): the forward entry passes per-sample time rows, which turns the in-place residual stream and
the LayerNorm fold off, so the production path of a width is only reached through the sampler.

What depends on the width: the grouped position conv's weight image (csrc/model.hip: dim / 16 channels per group; at 768 / 384 / 640 / 1152 /
1280 a 64-channel output tile straddles groups), the LayerNorm fold's partial planes (dim / 64 of them; the in-kernel statistics need K = 1024,
every other width takes stats_finalize), the tile counts of every block GEMM (N = 3 * heads * 64, ff_inner, dim), split_v of csrc/dit_eval.hip
and the row-wise time MLP / AdaLN kernel (K = dim: 8 vectors per lane above 1024).

Reference: the CPU oracle (oracle/cpu_ref.py, fp32; it differs from its own fp64 evaluation by rel-L2 5e-7 .. 7e-7 at these widths, two orders
of magnitude below the tightest tolerance) on seeded weights.  Tolerances: the project's own -- tests/test_gpu_model.py (fp32 2e-4, bf16 2e-2;
stages 1e-4 / 1.5e-2) and tests/test_gpu_fp16_model.py (fp16 5e-3; stages 3.75e-3), imported from there.  Every test prints its figures."""
import glob
import os

import pytest
import torch
import yaml

from conftest import ROOT, rel_l2
from oracle import cpu_ref
from test_gpu_fp16_model import STAGE_TOL as STAGE_TOL_FP16
from test_gpu_fp16_model import TOL as TOL_FP16
from test_gpu_model import STAGE_TOL as STAGE_TOL_MODEL
from test_gpu_model import TOL as TOL_MODEL
from test_gpu_model import _gen_rows, _make_mmdit, _make_unett

pytestmark = pytest.mark.gpu
TOL = dict(TOL_MODEL, fp16=TOL_FP16)
STAGE_TOL = dict(STAGE_TOL_MODEL, fp16=STAGE_TOL_FP16)
V = 200
CONFIG_DIR = os.path.join(ROOT, "eraxvif5tts_amd", "configs")
SMALL_DIT = dict(dim=768, depth=2, heads=12, ff_mult=2, text_dim=512, text_mask_padding=False, conv_layers=4, pe_attn_head=1)  # F5TTS_Small.yaml, depth 2
SMALL_UNETT = dict(dim=768, heads=12, ff_mult=4, text_mask_padding=False, pe_attn_head=1, skip_connect_type="concat")  # E2TTS_Small.yaml (+ depth)
SAMPLE_KW = dict(steps=2, cfg_strength=2.0, sway_sampling_coef=-1.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@pytest.fixture(autouse=True)
def _launcher_defaults(monkeypatch):
    """the kernels the launcher picks by itself (by token rows): that is what the regimes below are worked out for"""
    for k in ("F5HIP_GEMM_KERNEL", "F5HIP_ATTN_KERNEL", "F5HIP_PRECISION", "F5HIP_ROPE_LAYOUT"):
        monkeypatch.delenv(k, raising=False)


def _problem(B, N, seed, mel=100):
    """A sampler batch of B utterances, the longest N frames: unequal durations, prompt lengths and text lengths whenever B > 1 (live key mask,
    row mask and text padding), y0 zeroed past each duration."""
    g = torch.Generator().manual_seed(seed)
    nc, nt = min(120, N // 3), min(60, N // 4)
    cond = torch.randn(B, nc, mel, generator=g) * 2 - 3
    text = torch.randint(0, V, (B, nt), generator=g)
    dur = torch.tensor([N - (0, 131, 247, 24)[b] for b in range(B)])
    lens = torch.tensor([nc - (0, 23, 56, 9)[b] for b in range(B)])
    for b in range(1, B):
        text[b, nt - (0, 7, 19, 3)[b]:] = -1
    assert bool((dur > torch.maximum((text != -1).sum(-1), lens)).all())  # (CFM.sample keeps these durations)
    y0 = torch.randn(B, N, mel, generator=g)
    for b in range(B):
        y0[b, int(dur[b]):] = 0
    return dict(cond=cond, text=text, dur=dur, lens=lens, y0=y0)


_ORACLE = {}  # computed once per (model, batch), shared by the precisions and never written to


def _oracle_sample(key, W, cfg, pr):
    if key not in _ORACLE:
        _ORACLE[key] = cpu_ref.sample(W, cfg, pr["cond"], pr["text"], pr["dur"], lens=pr["lens"], y0=pr["y0"], **SAMPLE_KW)
    return _ORACLE[key]


def _sample(cfm, pr, **kw):
    return cfm.sample(cond=pr["cond"].cuda(), text=pr["text"].cuda(), duration=pr["dur"].cuda(), lens=pr["lens"].cuda(), y0=pr["y0"], **SAMPLE_KW, **kw)


def _check_sample(tag, cfm, pr, ref, prec, graph_and_repeat=False):
    """CFM.sample against the oracle's (out, trajectory) on the generated rows, as tests/test_gpu_model.py compares them; prompt frames verbatim."""
    ref_out, ref_traj = ref
    out, traj = _sample(cfm, pr, use_graph=False)
    dur = pr["dur"]
    assert out.shape == ref_out.shape and traj.shape == ref_traj.shape
    e_out, e_traj = rel_l2(_gen_rows(out.cpu(), dur), _gen_rows(ref_out, dur)), rel_l2(_gen_rows(traj.cpu(), dur), _gen_rows(ref_traj, dur))
    print(f"WIDTH {tag} {prec}: sample out {e_out:.3e} traj {e_traj:.3e} (tolerance {TOL[prec]:g})")
    assert e_out < TOL[prec] and e_traj < TOL[prec], (tag, prec, e_out, e_traj)
    for b in range(out.shape[0]):
        assert torch.equal(out[b, : int(pr["lens"][b])].cpu(), pr["cond"][b, : int(pr["lens"][b])])
    if graph_and_repeat:
        again, _ = _sample(cfm, pr, use_graph=False)
        assert torch.equal(again, out), "a second eager run differs"
        for _ in range(2):  # capture + first replay, cached replay
            assert torch.equal(_sample(cfm, pr, use_graph=True)[0], out), "graph replay differs from eager"
    if prec != "fp32":
        assert cfm.transformer.residual_fallbacks() == 0
    return e_out, e_traj


_TRACES = {}


def _check_stage_taps(tag, arch, W, prec, B, N, seed, mel=100):
    """DiT.forward's stage taps (t_emb, input_embed, blk{i}.n1 / .attn / .out, final_norm) and its output against the trace= dict of
    cpu_ref.dit_forward, both CFG branches, per-sample times, key mask -- what tests/test_gpu_model.py::test_forward_stage_taps does against
    the reference's own vectors.  .attn on valid rows only (the module zero-fills padded query rows, the fused kernel skips them)."""
    import gpu_helpers as G
    pr = _problem(B, N, seed, mel)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, N, mel, generator=g)
    cond = torch.nn.functional.pad(pr["cond"], (0, 0, 0, N - pr["cond"].shape[1]))
    t = torch.tensor([0.3, 0.7, 0.05, 0.95][:B])
    mask = cpu_ref.lens_to_mask(pr["dur"], N)
    D = arch["dim"]
    m = G.make_dit(arch, V, W, prec, mel_dim=mel)
    worst = {}
    for drop in (False, True):
        key = (tag, B, N, seed, drop)
        if key not in _TRACES:
            tr = {}
            cpu_ref.dit_forward(W, arch, x, cond, pr["text"], t, drop, drop, mask=mask, trace=tr)
            _TRACES[key] = tr
        tr = _TRACES[key]
        plan = m.plan(B, N, 1)
        taps = {"t_emb": torch.zeros(B, D), "input_embed": torch.zeros(B, N, D), "final_norm": torch.zeros(B, N, D)}
        for i in range(arch["depth"]):
            for s in ("n1", "attn", "out"):
                taps[f"blk{i}.{s}"] = torch.zeros(B, N, D)
        taps = {k: v.cuda() for k, v in taps.items()}
        for k, v in taps.items():
            m.set_tap(plan, k, v)
        out = m(x=x.cuda(), cond=cond.cuda(), text=pr["text"].cuda(), time=t.cuda(), mask=mask.cuda(), drop_audio_cond=drop, drop_text=drop, cache=False)
        torch.cuda.synchronize()
        m.set_tap(plan, None, None)
        errs = {}
        for k, v in taps.items():
            got, ref = v.cpu(), tr[k]
            if k.endswith(".attn"):
                got, ref = got[mask], ref[mask]
            errs[k] = rel_l2(got, ref)
        errs["out"] = rel_l2(out.cpu(), tr["out"])
        wk = max(errs, key=errs.get)
        worst[drop] = (wk, errs[wk])
        print(f"WIDTH {tag} {prec} {B}x{N} stage taps (drop={drop}): worst {wk} {errs[wk]:.3e} (tolerance {STAGE_TOL[prec]:g}); t_emb {errs['t_emb']:.3e} "
              f"input_embed {errs['input_embed']:.3e}")
        for k, e in errs.items():
            assert e < STAGE_TOL[prec], (tag, prec, drop, k, e)
    del m
    torch.cuda.empty_cache()
    return worst


# ----------------------------------------------------------------------------- 1a. F5TTS_Small's width through the sampler
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B,N", [(1, 200), (1, 1024), (2, 1001), (4, 1024)])
def test_small_dit_sampler_matches_oracle(B, N, prec):
    """DiT 768 / 12 heads (inner 768, ff 1536, QKV N = 2304 = 9 tiles of 256, out-projection / FF2 N = 768 = 3 tiles, FF1 N = 1536 = 6 tiles; 12
    partial planes), depth 2, 2 Euler steps, CFG 2, sway -1, against cpu_ref.sample on the generated rows of out and of the trajectory.
    Token rows = 2 B N with CFG; persistent grid 256 workgroups:

      1 x 200   400 rows   below 512: reference tile kernels, no LayerNorm fold.
      1 x 1024  2048 rows  fold on.  QKV: 8 x 9 = 72 tiles of 256 rows are under three quarters of the grid, 16 x 9 = 144 tiles of 128 rows are
                           at least half of it -> one-wave-per-SIMD kernel, 128-row tiles.  FF1 (16 x 6 = 96) and the out-projection
                           (16 x 3 = 48) stay on the 8-wave kernel.  K = 768, so no consumer finishes the statistics itself: every fold site
                           takes stats_finalize over 12 partial planes.
      2 x 1001  4004 rows  at least 3584 and no multiple of 256: the four block GEMMs run over 4096 padded rows (16 x 9 = 144 / 32 x 9 = 288
                           QKV tiles).
      4 x 1024  8192 rows  QKV (32 x 9 = 288) and FF1 (32 x 6 = 192) on 256-row tiles of the one-wave-per-SIMD kernel; out-projection and FF2
                           (32 x 3 = 96 tall tiles, 64 x 3 = 192 short ones) on 128-row tiles.

    bf16 also: a second run and hipGraph replay bit-identical to the first eager run, no fp16 range-guard fallback."""
    import gpu_helpers as G
    W = cpu_ref.random_dit_weights(SMALL_DIT, V, seed=768)
    pr = _problem(B, N, seed=1000 * B + N)
    ref = _oracle_sample(("small_dit", B, N), W, SMALL_DIT, pr)
    cfm = G.make_cfm(SMALL_DIT, V, W, prec)
    _check_sample(f"dit768/12 {B}x{N}", cfm, pr, ref, prec, graph_and_repeat=prec == "bf16")
    if prec != "fp32" and 2 * B * N >= 512:
        assert G.plan_option(cfm.transformer, "ln_fold_active") == 1
    del cfm
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 1b. stage taps
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [300, 1001])
def test_small_dit_stage_taps(N, prec):
    """What pins the position-conv image of 48 channels per group (input_embed) and the K = 768 time MLP (t_emb) on their own."""
    W = cpu_ref.random_dit_weights(SMALL_DIT, V, seed=768)
    _check_stage_taps("dit768/12", SMALL_DIT, W, prec, 2, N, seed=40 + N)


# ----------------------------------------------------------------------------- 1c. knob equalities
@pytest.mark.parametrize("B,N", [(4, 1024), (2, 1001)])
def test_small_dit_knob_equalities(B, N):
    """bf16, dim 768: (1) gemm_w4 = 0 (8-wave kernel everywhere) equals the default bit for bit -- at 4 x 1024 this is the run that takes split_v
    of csrc/dit_eval.hip at inner = 768 (32 x 6 = 192 q|k tiles fit one round of the 256 CUs, 32 x 9 = 288 do not), whose separate v launch
    reads the folded c1 / c2 / W' rows at offset 2 * inner; (2) at 2 x 1001 (4004 -> 4096 padded rows) gemm_pad_rows = 0 equals the default bit
    for bit, the relation tests/test_gpu_padded_rows.py asserts at dim 1024; (3) ln_fold = 0 (two LayerNorm passes per block) and the fold are
    both within TOL of the fp32 mode and e_fold < 1.25 e_pass, the rule of tests/test_gpu_fullsize.py::
    test_layernorm_fold_against_the_unfolded_path_and_fp32_mode."""
    import gpu_helpers as G
    W = cpu_ref.random_dit_weights(SMALL_DIT, V, seed=768)
    pr = _problem(B, N, seed=1000 * B + N)
    dur = pr["dur"]
    run = lambda c: _sample(c, pr, use_graph=False, return_trajectory=False)[0].cpu()
    cfm = G.make_cfm(SMALL_DIT, V, W, "bf16")
    fold = run(cfm)
    assert torch.isfinite(fold).all() and G.plan_option(cfm.transformer, "ln_fold_active") == 1
    with G.knobs(gemm_w4=0):
        out = run(cfm)
    assert torch.equal(out, fold), ("gemm_w4 = 0", float((out - fold).abs().max()))
    if (2 * B * N) % 256:
        with G.knobs(gemm_pad_rows=0):
            out = run(cfm)
        assert torch.equal(out, fold), ("gemm_pad_rows = 0", float((out - fold).abs().max()))
    assert cfm.transformer.residual_fallbacks() == 0
    del cfm
    torch.cuda.empty_cache()
    with G.knobs(ln_fold=0):
        cfm = G.make_cfm(SMALL_DIT, V, W, "bf16")
        passes = run(cfm)
        assert cfm.transformer.residual_fallbacks() == 0 and G.plan_option(cfm.transformer, "ln_fold_active") == 0  # (the leg really ran the passes)
        del cfm
    cfm = G.make_cfm(SMALL_DIT, V, W, "fp32")
    want = run(cfm)
    del cfm
    torch.cuda.empty_cache()
    e_fold, e_pass = rel_l2(_gen_rows(fold, dur), _gen_rows(want, dur)), rel_l2(_gen_rows(passes, dur), _gen_rows(want, dur))
    print(f"WIDTH dit768/12 {B}x{N} bf16 vs fp32 mode: LayerNorm fold {e_fold:.3e}, LayerNorm passes {e_pass:.3e}; fold vs passes "
          f"{rel_l2(_gen_rows(fold, dur), _gen_rows(passes, dur)):.3e}")
    assert e_fold < TOL["bf16"] and e_pass < TOL["bf16"] and e_fold < 1.25 * e_pass


# ----------------------------------------------------------------------------- 1d. ragged sampling
@pytest.mark.parametrize("kernels", ["reference-kernels", "tuned-kernels", "by-row-count"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_small_dit_ragged_sample_equals_batch1_samples(prec, kernels, monkeypatch):
    """f5_sample_ragged at dim 768 through CFM.sample_ragged, the entry tests/test_gpu_model.py::test_ragged_sample_equals_batch1_samples uses,
    against batch-1 samples of the same utterances (130, 517 and 1001 frames): torch.equal per utterance, under the two kernel settings that
    test runs with (its `kernels` fixture: reference tile kernels only / tuned kernels forced), which is where include/f5hip.h promises equal
    bits -- "whenever both calls take the tuned kernels ... or both the fp32 mode's".  Third setting, the launcher's own choice by token rows:
    the batch-1 call of the 130-frame utterance (260 rows with CFG) stays on the reference tile kernels while the ragged batch (3360 rows)
    takes the tuned ones, so in bf16 that one utterance is held to TOL against its batch-1 sample instead; every other comparison stays
    torch.equal.  One utterance also against the CPU oracle."""
    import gpu_helpers as G
    if kernels != "by-row-count":
        v = "0" if kernels == "reference-kernels" else "1"
        monkeypatch.setenv("F5HIP_GEMM_KERNEL", v)
        monkeypatch.setenv("F5HIP_ATTN_KERNEL", v)
    W = cpu_ref.random_dit_weights(SMALL_DIT, V, seed=768)
    cfm = G.make_cfm(SMALL_DIT, V, W, prec)
    g = torch.Generator().manual_seed(77)
    nc = 90
    cond = (torch.randn(1, nc, 100, generator=g) * 2 - 3).cuda()
    durs = [130, 517, 1001]
    texts = [torch.randint(0, V, (1, n), generator=g).cuda() for n in (31, 12, 45)]
    y0s = [torch.randn(1, d, 100, generator=g).cuda() for d in durs]
    ref = [cfm.sample(cond=cond, text=t, duration=d, y0=y, return_trajectory=False, use_graph=False, **SAMPLE_KW)[0] for t, d, y in zip(texts, durs, y0s)]
    got = cfm.sample_ragged(cond, texts, durs, y0s=y0s, **SAMPLE_KW)
    for a, b, d in zip(got, ref, durs):
        assert a.shape == (1, d, 100) and torch.isfinite(a).all()
        print(f"WIDTH dit768/12 ragged {prec} [{kernels}] {d} frames: max |ragged - batch-1| {float((a - b).abs().max()):.3e}, "
              f"rel-L2 {rel_l2(a.cpu()[:, nc:], b.cpu()[:, nc:]):.3e}")
    for a, b, d in zip(got, ref, durs):
        if kernels == "by-row-count" and prec == "bf16" and 2 * d < 512:
            assert rel_l2(a.cpu()[:, nc:], b.cpu()[:, nc:]) < TOL[prec], d
        else:
            assert torch.equal(a, b), (d, float((a - b).abs().max()))
    key = ("ragged", 517)
    if key not in _ORACLE:
        _ORACLE[key] = cpu_ref.sample(W, SMALL_DIT, cond.cpu(), texts[1].cpu(), durs[1], y0=y0s[1].cpu(), return_trajectory=False, **SAMPLE_KW)
    err = rel_l2(got[1].cpu()[:, nc:], _ORACLE[key][0][:, nc:])
    print(f"WIDTH dit768/12 ragged {prec} [{kernels}] 517 frames vs oracle: {err:.3e}")
    assert err < TOL[prec]
    del cfm
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 1e. E2TTS_Small's width
_UNETT_REF = {}


def _check_unett(tag, arch, prec, B, N, seed):
    """UNetT forward (both CFG branches, key mask, per-sample times) at STAGE_TOL and CFM.sample (eager, capture, replay) at TOL against
    cpu_ref.unett_forward / cpu_ref.sample, as tests/test_gpu_model.py::test_unett_forward_and_sample_match_reference and
    ::test_unett_other_skip_types_match_oracle compare them."""
    W = cpu_ref.random_unett_weights(arch, V, seed=seed)
    m, cfm = _make_unett(arch, V, W, prec)
    pr = _problem(B, N, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, N, 100, generator=g)
    cond = torch.nn.functional.pad(pr["cond"], (0, 0, 0, N - pr["cond"].shape[1]))
    t = torch.tensor([0.3, 0.7])
    mask = cpu_ref.lens_to_mask(pr["dur"], N)
    key = (tag, B, N, seed)
    if key not in _UNETT_REF:
        fw = {drop: cpu_ref.unett_forward(W, arch, x, cond, pr["text"], t, drop, drop, mask=mask) for drop in (False, True)}
        _UNETT_REF[key] = (fw, cpu_ref.sample(W, dict(arch, backbone="UNetT"), pr["cond"], pr["text"], pr["dur"], lens=pr["lens"], y0=pr["y0"], **SAMPLE_KW))
    fw, ref = _UNETT_REF[key]
    for drop in (False, True):
        out = m(x=x.cuda(), cond=cond.cuda(), text=pr["text"].cuda(), time=t.cuda(), mask=mask.cuda(), drop_audio_cond=drop, drop_text=drop)
        err = rel_l2(out.cpu(), fw[drop])
        print(f"WIDTH {tag} {B}x{N} {prec}: forward (drop={drop}) {err:.3e} (tolerance {STAGE_TOL[prec]:g})")
        assert err < STAGE_TOL[prec], (tag, drop, err)
    _check_sample(f"{tag} {B}x{N}", cfm, pr, ref, prec, graph_and_repeat=True)
    del m, cfm
    torch.cuda.empty_cache()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [255, 1000])
@pytest.mark.parametrize("depth", [2, 4])
def test_small_unett_forward_and_sample_match_oracle(depth, N, prec):
    """UNetT 768 / 12 heads, ff_mult 4 (ff 3072), concat skips (Linear(1536 -> 768) in the second half), depth 2 and 4; B = 2.  The time token makes
    the rows of an utterance N + 1 = 256 / 1001."""
    _check_unett(f"unett768/12 depth {depth}", dict(SMALL_UNETT, depth=depth), prec, 2, N, seed=500 + depth)


# ----------------------------------------------------------------------------- 1f. the shipped yamls
def _yaml_backbone(path, precision):
    from eraxvif5tts_amd.model import DiT, MMDiT, UNetT
    with open(path) as f:
        model = yaml.safe_load(f)["model"]
    arch = dict(model["arch"])
    if model["backbone"] != "DiT":
        arch.pop("checkpoint_activations", None)
    torch.manual_seed(1234)  # the default init draws from the global generator
    cls = {"DiT": DiT, "UNetT": UNetT, "MMDiT": MMDiT}[model["backbone"]]
    return cls(**arch, text_num_embeds=V, mel_dim=model["mel_spec"]["n_mel_channels"], precision=precision).cuda()


def _yamls():
    return sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(CONFIG_DIR, "*.yaml")))


def test_the_shipped_yamls_are_the_seven_this_file_covers():
    names = _yamls()
    assert len(names) == 7 and sorted(n for n in names if "Small" in n) == ["E2TTS_Small", "F5TTS_Small"], names


@pytest.mark.parametrize("name", ["F5TTS_Small", "E2TTS_Small"])
def test_small_yaml_at_full_depth(name):
    """The backbone exactly as the yaml describes it (18 / 20 layers), default init, bf16: one sample() of 1 x 256 frames, 2 steps -- finite,
    prompt frames returned verbatim, hipGraph replay equal to eager."""
    from eraxvif5tts_amd.model import CFM
    m = _yaml_backbone(os.path.join(CONFIG_DIR, name + ".yaml"), "bf16")
    assert m.dim == 768 and m.heads == 12
    cfm = CFM(transformer=m, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()
    g = torch.Generator().manual_seed(3)
    nc = 80
    cond = (torch.randn(1, nc, 100, generator=g) * 2 - 3).cuda()
    kw = dict(cond=cond, text=torch.randint(0, V, (1, 30), generator=g).cuda(), duration=256, y0=torch.randn(1, 256, 100, generator=g), **SAMPLE_KW)
    out, _ = cfm.sample(use_graph=False, **kw)
    assert out.shape == (1, 256, 100) and torch.isfinite(out).all()
    assert torch.equal(out[:, :nc], cond)
    for _ in range(2):
        assert torch.equal(cfm.sample(use_graph=True, **kw)[0], out)
    assert m.residual_fallbacks() == 0
    del cfm, m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["E2TTS_Base", "F5TTS_Base", "F5TTS_v1_Base", "F5TTS_v1_Pruned_12", "F5TTS_v1_Pruned_14"])
def test_other_yaml_archs_pass_create_and_finalize(name):
    m = _yaml_backbone(os.path.join(CONFIG_DIR, name + ".yaml"), "bf16")
    assert m.native() is not None  # f5_model_create + f5_model_set_tensor + f5_model_finalize
    del m
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 2. the other widths create() accepts
_BASE = dict(depth=2, ff_mult=2, text_dim=128, conv_layers=2, pe_attn_head=1, text_mask_padding=False)
WIDTHS = {  # id -> (arch, mel_dim)
    "384x6": (dict(_BASE, dim=384, heads=6), 100),                                      # 24 channels per conv group
    "640x10_ff4": (dict(_BASE, dim=640, heads=10, ff_mult=4), 100),                     # 40 channels per group
    "1152x18": (dict(_BASE, dim=1152, heads=18), 100),                                  # 72 channels per group: wider than an output tile
    "1280x20": (dict(_BASE, dim=1280, heads=20), 100),                                  # 80 per group; row-wise linear with 8 vectors per lane
    "2048x32": (dict(_BASE, dim=2048, heads=32, depth=1, conv_layers=1), 100),          # the cap; row-wise linear at K = 2048
    "256x2": (dict(_BASE, dim=256, heads=2), 100),                                      # inner 128 < dim
    "128x4": (dict(_BASE, dim=128, heads=4), 100),                                      # inner 256 > dim
    "768x16": (dict(_BASE, dim=768, heads=16), 100),                                    # inner 1024 at dim 768
    "256x4_mel80": (dict(_BASE, dim=256, heads=4), 80),                                 # mel_dim below the default
    "256x4_mel128": (dict(_BASE, dim=256, heads=4), 128),                               # mel_dim = the padded mel width
    "256x4_td100": (dict(_BASE, dim=256, heads=4, text_dim=100, conv_layers=0), 100),   # text columns padded to 128
    "256x4_td96": (dict(_BASE, dim=256, heads=4, text_dim=96, conv_layers=2), 100),     # text width no power of two, with text blocks
    "128x2_ff3": (dict(_BASE, dim=128, heads=2, ff_mult=3), 100),                       # ff_mult above the default
    "384x6_rope_all": (dict(_BASE, dim=384, heads=6, pe_attn_head=None, text_mask_padding=True), 100),  # RoPE on every head, text mask padding
}


def _check_width(wid, prec, taps):
    import gpu_helpers as G
    arch, mel = WIDTHS[wid]
    seed = 3000 + sorted(WIDTHS).index(wid)
    W = cpu_ref.random_dit_weights(arch, V, seed=seed, mel_dim=mel)
    pr = _problem(2, 300, seed, mel)
    ref = _oracle_sample(("width", wid), W, arch, pr)
    cfm = G.make_cfm(arch, V, W, prec, mel_dim=mel)
    _check_sample(f"dit{wid} 2x300", cfm, pr, ref, prec, graph_and_repeat=prec != "fp32")
    if prec != "fp32":
        assert G.plan_option(cfm.transformer, "ln_fold_active") == 1
    del cfm
    torch.cuda.empty_cache()
    if taps:
        _check_stage_taps(f"dit{wid}", arch, W, prec, 2, 300, seed, mel)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("wid", list(WIDTHS))
def test_other_widths_match_oracle(wid, prec):
    """One DiT per line of WIDTHS, B = 2, N = 300 (1200 token rows with CFG: the LayerNorm fold is on in the 16-bit modes), 2 Euler steps, CFG 2:
    sample() against cpu_ref.sample at TOL; in fp32 also the stage taps of test_small_dit_stage_taps."""
    _check_width(wid, prec, taps=prec == "fp32")


def test_other_width_fp16_mode():
    _check_width("640x10_ff4", "fp16", taps=False)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mmdit_384_forward_and_sample_match_oracle(prec):
    """MMDiT at dim 384, 6 heads, depth 2 (the only other MMDiT width in the suite is 512): forward of both CFG branches and sample()."""
    arch = dict(dim=384, depth=2, heads=6, ff_mult=2, text_mask_padding=True)
    W = cpu_ref.random_mmdit_weights(arch, V, seed=61)
    m, cfm = _make_mmdit(arch, V, W, prec)
    B, N = 2, 300
    pr = _problem(B, N, 62)
    g = torch.Generator().manual_seed(63)
    x = torch.randn(B, N, 100, generator=g)
    cond = torch.nn.functional.pad(pr["cond"], (0, 0, 0, N - pr["cond"].shape[1]))
    t = torch.tensor([0.3, 0.7])
    mask = cpu_ref.lens_to_mask(pr["dur"], N)
    for drop in (False, True):
        ref = cpu_ref.mmdit_forward(W, arch, x, cond, pr["text"], t, drop, drop, mask=mask)
        out = m(x=x.cuda(), cond=cond.cuda(), text=pr["text"].cuda(), time=t.cuda(), mask=mask.cuda(), drop_audio_cond=drop, drop_text=drop)
        err = rel_l2(out.cpu(), ref)
        print(f"WIDTH mmdit384/6 {B}x{N} {prec}: forward (drop={drop}) {err:.3e} (tolerance {STAGE_TOL[prec]:g})")
        assert err < STAGE_TOL[prec], (drop, err)
    ref = _oracle_sample(("mmdit384",), W, dict(arch, backbone="MMDiT"), pr)
    _check_sample(f"mmdit384/6 {B}x{N}", cfm, pr, ref, prec, graph_and_repeat=True)
    del m, cfm
    torch.cuda.empty_cache()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_unett_384_forward_and_sample_match_oracle(prec):
    _check_unett("unett384/6", dict(dim=384, depth=2, heads=6, ff_mult=2, text_mask_padding=False, pe_attn_head=1, skip_connect_type="concat"), prec, 2, 300,
                 seed=71)


REFUSED = {
    "dim_192": dict(dim=192, heads=3),
    "dim_2176": dict(dim=2176, heads=34),
    "mel_dim_132": dict(dim=256, heads=4, mel_dim=132),
    "mel_dim_98": dict(dim=256, heads=4, mel_dim=98),
    "text_dim_100_with_a_text_block": dict(dim=256, heads=4, text_dim=100, conv_layers=1),
    "ff_inner_268": dict(dim=128, heads=2, ff_mult=2.1),
    "dim_head_32": dict(dim=256, heads=4, dim_head=32),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_widths_are_refused_at_construction(case):
    """What f5_model_create() does not implement raises F5HipError when the native model is built -- before any plan, forward or sample."""
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.model import DiT
    kw = dict(dict(_BASE, mel_dim=100), **REFUSED[case])
    m = DiT(**kw, text_num_embeds=V, precision="bf16").cuda()
    if case == "ff_inner_268":
        assert m.ff_inner == 268 and m.ff_inner % 32 != 0
    with pytest.raises(_lib.F5HipError):
        m.native()
