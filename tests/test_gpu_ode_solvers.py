"""The Runge-Kutta solvers (rk4, heun2, heun3) on the fused sampler: one rk_stage_kernel launch after every network evaluation, slopes kept
in the tail of the plan's trajectory buffer.  Against the Python driver over DiT.forward (fp32 mode, 1e-5: the tolerance of
test_native_edit_matches_the_python_driver_in_fp32_mode) and against the oracle restatement of tests/test_ode_solvers_host.py (2e-4 / 2e-2:
the tolerances of the golden tests); hipGraph replay, the ragged sampler, speech editing, UNetT / MMDiT, the full-size model and the
refusals of the C ABI."""
import ast
import ctypes as C

import pytest
import torch

from conftest import golden_arch, golden_weights, load_golden, rel_l2
from oracle import cpu_ref
from test_ode_solvers_host import RK_METHODS, oracle_sample

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
        raise AssertionError("the call took the Python driver")
    monkeypatch.setattr(CFM, "_sample_python", boom)


def _base_problem(B):
    z = load_golden("tiny_base")
    g = lambda k: torch.from_numpy(z[k])[:B]
    dur = g("duration")
    N = int(dur.max())
    y0 = torch.randn(B, N, 100, generator=torch.Generator().manual_seed(5))
    for b in range(B):
        y0[b, int(dur[b]):] = 0
    return z, dict(cond=g("cond"), text=g("text"), duration=dur, lens=g("lens"), steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0)


def _cuda(kw):
    return {k: v.cuda() if isinstance(v, torch.Tensor) and k != "y0" else v for k, v in kw.items()}


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("method", RK_METHODS)
def test_native_rk_matches_the_python_driver_in_fp32_mode(B, method):
    """f5_sample with the new method against CFM._sample_python over DiT.forward (edit_native=False with an all-true edit mask: the same
    cond_mask as the lens prefix), rel-L2 <= 1e-5 on output and trajectory."""
    import gpu_helpers as G
    z, kw = _base_problem(B)
    c = G.make_cfm(golden_arch(z), int(z["vocab"]), golden_weights(z), "fp32", method=method)
    kw = _cuda(kw)
    nat, ntraj = c.sample(**kw)
    py, ptraj = c.sample(edit_mask=torch.ones(B, kw["cond"].shape[1], dtype=torch.bool, device="cuda"), edit_native=False, **kw)
    d = kw["duration"].cpu()
    assert ntraj.shape == (4, B, int(d.max()), 100)
    assert rel_l2(_gen_rows(nat.cpu(), d), _gen_rows(py.cpu(), d)) <= 1e-5
    assert rel_l2(_gen_rows(ntraj.cpu(), d), _gen_rows(ptraj.cpu(), d)) <= 1e-5


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("method", RK_METHODS)
def test_native_rk_matches_the_oracle_restatement(method, prec, monkeypatch):
    """tiny_base, B = 2 with a key mask, CFG 2, sway -1: the fused sampler (eager, capture, replay) against the host restatement."""
    import gpu_helpers as G
    _no_python_driver(monkeypatch)
    z, kw = _base_problem(2)
    W, arch = golden_weights(z), golden_arch(z)
    ref, ref_traj = oracle_sample(W, arch, kw["cond"], kw["text"], kw["duration"], kw["lens"], kw["steps"], 2.0, -1.0, kw["y0"], method)
    c = G.make_cfm(arch, int(z["vocab"]), W, prec, method=method)
    d = kw["duration"]
    for use_graph in (False, True, True):
        out, traj = c.sample(use_graph=use_graph, **_cuda(kw))
        assert rel_l2(_gen_rows(out.cpu(), d), _gen_rows(ref, d)) < TOL[prec]
        assert rel_l2(_gen_rows(traj.cpu(), d), _gen_rows(ref_traj, d)) < TOL[prec]


def test_rk4_graph_replay_is_bit_identical_and_reads_the_current_y0():
    """bf16, tuned kernels forced, N = 256: a capture equals the eager run bit for bit, and a replay of that capture with another y0 equals
    the eager run with that y0."""
    import gpu_helpers as G
    V, B, N = 60, 2, 256
    W = cpu_ref.random_dit_weights(SMALL, V, seed=61)
    m = G.make_dit(SMALL, V, W, "bf16")
    m.set_kernels(gemm=1, attn=1)
    g = torch.Generator().manual_seed(62)
    cond = (torch.randn(B, N, 100, generator=g) * 2 - 3).cuda()
    text = torch.randint(0, V, (B, 24), generator=g).cuda()
    lens, dur = torch.tensor([128, 97]).cuda(), torch.tensor([N, N]).cuda()
    ya, yb = torch.randn(B, N, 100, generator=g), torch.randn(B, N, 100, generator=g)
    tg = cpu_ref.time_grid(3, -1.0)
    kw = dict(method="rk4", use_mask=False, return_trajectory=True)
    ea, ta = m.native_sample(cond, text, lens, dur, ya, tg, 3, 2.0, use_graph=False, **kw)
    eb, tb = m.native_sample(cond, text, lens, dur, yb, tg, 3, 2.0, use_graph=False, **kw)
    ga, gta = m.native_sample(cond, text, lens, dur, ya, tg, 3, 2.0, use_graph=True, **kw)  # capture
    gb, gtb = m.native_sample(cond, text, lens, dur, yb, tg, 3, 2.0, use_graph=True, **kw)  # replay
    torch.cuda.synchronize()
    assert not torch.equal(ea, eb)
    assert torch.equal(ga, ea) and torch.equal(gta, ta)
    assert torch.equal(gb, eb) and torch.equal(gtb, tb)


def test_rk4_ragged_sample_equals_batch1_samples():
    """f5_sample_ragged with rk4 against batch-1 CFM.sample calls of the same utterances, bf16 with the tuned kernels forced, every utterance
    at least 256 frames: torch.equal per utterance (as test_ragged_sample_equals_batch1_samples for euler / midpoint)."""
    import gpu_helpers as G
    z = load_golden("tiny_base")
    arch, V, W = golden_arch(z), int(z["vocab"]), golden_weights(z)
    cfm = G.make_cfm(arch, V, W, "bf16", method="rk4")
    cfm.transformer.set_kernels(gemm=1, attn=1)
    g = torch.Generator().manual_seed(78)
    nc = 90
    cond = (torch.randn(1, nc, 100, generator=g) * 2 - 3).cuda()
    durs = [300, 257, 411]
    texts = [torch.randint(0, V, (1, n), generator=g).cuda() for n in (31, 12, 45)]
    y0s = [torch.randn(1, d, 100, generator=g).cuda() for d in durs]
    kw = dict(steps=2, cfg_strength=2.0, sway_sampling_coef=-1.0)
    ref = [cfm.sample(cond=cond, text=t, duration=d, y0=y, return_trajectory=False, use_graph=False, **kw)[0] for t, d, y in zip(texts, durs, y0s)]
    got = cfm.sample_ragged(cond, texts, durs, y0s=y0s, **kw)
    for a, b, d in zip(got, ref, durs):
        assert a.shape == (1, d, 100) and torch.isfinite(a).all()
        assert torch.equal(a, b), (d, float((a - b).abs().max()))


def test_rk4_with_an_edit_mask_matches_the_python_driver_in_fp32_mode():
    """f5_sample_masked with rk4 against the Python driver (fp32 mode, 1e-5), B = 2 with different masks and durations; kept frames equal
    cond exactly."""
    import gpu_helpers as G
    z, kw = _base_problem(2)
    c = G.make_cfm(golden_arch(z), int(z["vocab"]), golden_weights(z), "fp32", method="rk4")
    kw = _cuda(kw)
    nc = kw["cond"].shape[1]
    edit = torch.ones(2, nc, dtype=torch.bool)
    edit[0, 3:9] = edit[0, 15:18] = edit[1, 0:2] = edit[1, 10:20] = False
    edit = edit.cuda()
    nat, ntraj = c.sample(edit_mask=edit, **kw)
    py, ptraj = c.sample(edit_mask=edit, edit_native=False, **kw)
    d = kw["duration"].cpu()
    N = int(d.max())
    assert rel_l2(_gen_rows(nat.cpu(), d), _gen_rows(py.cpu(), d)) <= 1e-5
    assert rel_l2(_gen_rows(ntraj.cpu(), d), _gen_rows(ptraj.cpu(), d)) <= 1e-5
    keep = torch.nn.functional.pad(edit.cpu() & cpu_ref.lens_to_mask(kw["lens"].cpu()), (0, N - nc))
    assert torch.equal(nat.cpu()[keep], torch.nn.functional.pad(kw["cond"].cpu(), (0, 0, 0, N - nc))[keep])


@pytest.mark.parametrize("backbone,method", [("UNetT", "heun3"), ("MMDiT", "rk4")])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_other_backbones_match_the_oracle_restatement(backbone, method, prec, monkeypatch):
    """The tiny UNetT / MMDiT goldens' architectures (both inherit native_sample), B = 2 with a key mask, on the native sampler."""
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
    cfm = CFM(transformer=m.cuda(), mel_spec_kwargs={"mel_spec_type": "vocos"}, odeint_kwargs={"method": method}).cuda()
    g = lambda k: torch.from_numpy(z[f"a.{k}"])
    cond, text, lens, dur = g("cond")[:, :16], g("text"), g("lens"), g("duration")
    y0 = g("sample_traj")[0]
    ref, ref_traj = oracle_sample(W, {**arch, "backbone": backbone}, cond, text, dur, lens, 2, 2.0, -1.0, y0, method)
    for use_graph in (False, True, True):
        out, traj = cfm.sample(cond=cond.cuda(), text=text.cuda(), duration=dur.cuda(), lens=lens.cuda(), steps=2, cfg_strength=2.0,
                               sway_sampling_coef=-1.0, y0=y0, use_graph=use_graph)
        assert rel_l2(_gen_rows(out.cpu(), dur), _gen_rows(ref, dur)) < TOL[prec]
        assert rel_l2(_gen_rows(traj.cpu(), dur), _gen_rows(ref_traj, dur)) < TOL[prec]


def test_full_size_rk4_bf16_against_fp32_mode():
    """F5TTS_Base, B = 2, N = 1024 (durations 1024 / 900: key mask on), rk4 with 8 steps (32 evaluation times: LayerNorm-fold table),
    gemm_w4 + ln_fold forced: bf16 against the fp32 parity mode, rel-L2 < 2e-2 on the generated frames, no fp32 fallback."""
    import bench
    import gpu_helpers as G
    from eraxvif5tts_amd.model import CFM, DiT
    B, N = 2, 1024
    cond, text, lens, dur = bench.synth_batch(B, N, "cuda", seed=71)
    dur[1] = 900
    y0 = torch.randn(B, N, 100, generator=torch.Generator().manual_seed(72))
    y0[1, 900:] = 0
    kw = dict(cond=cond, text=text, duration=dur, lens=lens, steps=8, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, return_trajectory=False)
    outs = {}
    with G.knobs(gemm_w4=1, ln_fold=1):
        for prec in ("fp32", "bf16"):
            torch.manual_seed(1234)
            model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision=prec), seed=0)
            if prec == "bf16":
                model.set_kernels(gemm=1, attn=1)
            cfm = CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}, odeint_kwargs={"method": "rk4"}).cuda()
            outs[prec] = cfm.sample(use_graph=False, **kw)[0].cpu()
            if prec == "bf16":
                assert torch.equal(cfm.sample(use_graph=True, **kw)[0].cpu(), outs[prec])
                assert model.residual_fallbacks() == 0
            del cfm, model
            torch.cuda.empty_cache()
    gen = ~cpu_ref.lens_to_mask(lens.cpu(), N) & cpu_ref.lens_to_mask(dur.cpu(), N)
    err = rel_l2(outs["bf16"][gen], outs["fp32"][gen])
    print(f"rk4, 22 blocks x 8 steps: bf16 vs fp32 mode rel-L2 {err:.3e}")
    assert torch.isfinite(outs["bf16"]).all() and err < 2e-2


def test_c_abi_refuses_a_short_plan_and_an_unknown_method_before_any_work():
    """A plan whose max_evals is below 4 x steps refuses an rk4 call with F5_EINVAL (3 steps of heun3 fit the same plan), and an unknown
    ode_method code is refused the same way; the output buffer is left untouched."""
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    z, kw = _base_problem(1)
    m = G.make_dit(golden_arch(z), int(z["vocab"]), golden_weights(z), "fp32")
    B, N, steps = 1, int(kw["duration"][0]), 3
    plan = m.plan(B, N, 4 * steps - 1)
    cond = torch.nn.functional.pad(kw["cond"], (0, 0, 0, N - kw["cond"].shape[1])).cuda().contiguous()
    ids = kw["text"].cuda().to(torch.int32).contiguous()
    lens = kw["lens"].cuda().to(torch.int32).contiguous()
    y0 = kw["y0"].cuda().contiguous()
    tg = cpu_ref.time_grid(steps, -1.0).contiguous()

    def call(meth):
        out = torch.full_like(cond, float("nan"))
        rc = lib.f5_sample(plan, B, N, _lib.ptr(cond), _lib.ptr(ids), ids.shape[1], _lib.ptr(lens), None, _lib.ptr(y0), C.c_void_p(tg.data_ptr()),
                           steps, 2.0, meth, _lib.ptr(out), None, 0, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    rc, out = call(_lib.F5_ODE_RK4)
    assert rc == -1 and "max_evals" in _lib.last_error() and torch.isnan(out).all()
    rc, out = call(7)
    assert rc == -1 and "ode_method" in _lib.last_error() and torch.isnan(out).all()
    rc, out = call(_lib.F5_ODE_HEUN3)
    assert rc == 0 and torch.isfinite(out).all()
