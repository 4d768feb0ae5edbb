"""The production-mode DiT evaluation, stage by stage against fp64 (include/f5hip.h: f5_plan_set_probe).

The benchmarked evaluation runs with the fp16 residual stream, in-place residual epilogues, the LayerNorm fold, pre-scaled q (bf16) and padded
block-GEMM rows all on, and a stage tap switches every one of them off.  A probe enters no mode decision: it copies a buffer the evaluation holds
anyway.  Here every probed stage of one evaluation of a sample() loop is compared with an fp64 restatement of THAT ONE stage, computed on the CPU
from the device's own probe of the stage before it and the model's own weights in fp64 (gpu_helpers.stage_ref), on a row sample
(gpu_helpers.stage_sample_rows: tile edges, sequence boundaries, the last row, 64 seeded rows), every column of a sampled row.  A row passes when
its error is within STAGE_MARGIN x the worst row error of the CPU restatement with the kernel's roundings (gpu_helpers.stage_emulate) of the same
stage and case; tests/test_production_stage_bound_host.py shows that this bound rejects the wiring defects it is there for.  So an assert here
is the rounding of one launch, not the 2e-2 of a whole sample().

Model: F5TTS_Base width (dim 1024, 16 heads, ff 2048), bench.synth_weights, depth 3 -- block 0 with its unfolded first LayerNorm and the
pre-scaled weight copy, a fully folded middle block, a last block whose FF2 writes no statistics in front of the final AdaLN pass.  CFG 2, Euler,
3 steps.  The cases are the smallest shape of each path, and each asserts its path (gpu_helpers.eval_modes, site_gemm)."""
import ctypes as C
import math

import pytest
import torch

import gpu_helpers as G
from gpu_helpers import P_BF16, P_FP16

pytestmark = pytest.mark.gpu

ARCH = dict(dim=1024, depth=3, heads=16, ff_mult=2, text_dim=512, text_mask_padding=False, conv_layers=4, pe_attn_head=1)
D, DEPTH, HEADS, INNER, FF, MEL, STEPS = 1024, 3, 16, 1024, 2048, 100, 3
F5_EINVAL, F5_ESTATE = -1, -4  # include/f5hip.h


def _tgrid():
    t = torch.linspace(0, 1, STEPS + 1)
    return t - (torch.cos(torch.pi / 2 * t) - 1 + t)  # sway_sampling_coef = -1


@pytest.fixture(scope="module")
def models():
    """get(precision name) -> the model of that mode with its one plan and its weights on the host; built on first use, shared by the module"""
    import bench
    from eraxvif5tts_amd import _lib
    from eraxvif5tts_amd.model import DiT
    _lib.require_gpu()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus & ~7 == 256, f"the shapes are worked out for a 256-CU device, this one has {cus} CUs"
    cache = {}

    def get(pname):
        if pname not in cache:
            torch.manual_seed(1234)
            model = bench.synth_weights(DiT(**ARCH, text_num_embeds=bench.VOCAB, mel_dim=MEL, precision=pname), seed=0).cuda()
            plan = model.plan(8, 1088, STEPS)  # one plan holds every case (the ragged one needs 2 x 1952 rows and a text row more)
            cache[pname] = dict(model=model, plan=plan, prec=P_BF16 if pname == "bf16" else P_FP16, W=G.stage_weights(model.state_dict(), DEPTH))
        return cache[pname]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _inputs(B, N, seed, frames=None):
    import bench
    g = torch.Generator().manual_seed(seed)
    rows = (B, N) if frames is None else (sum(frames),)
    cond = (torch.randn(*rows, MEL, generator=g) * 2 - 3).clamp(math.log(1e-5), 3.0)
    y0 = torch.randn(*rows, MEL, generator=g)
    text = torch.randint(0, bench.VOCAB, (B, max(12, N // 6)), generator=g)
    lens = torch.full((B,), N // 3) if frames is None else torch.tensor([f // 3 for f in frames])
    return cond.cuda(), text, lens, y0.cuda()


def _sample(model, inp, B, N, durations=None, frames=None, use_graph=False, traj=False):
    cond, text, lens, y0 = inp
    if frames is not None:
        out, tr = model.native_sample_ragged(cond, text, lens, frames, y0, _tgrid(), STEPS, 2.0, use_graph=use_graph), None
    else:
        dur = torch.full((B,), N) if durations is None else torch.tensor(durations)
        out, tr = model.native_sample(cond, text, lens, dur, y0, _tgrid(), STEPS, 2.0, method="euler", use_mask=durations is not None,
                                      return_trajectory=traj, use_graph=use_graph)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out, tr


def _probe_names(lnf):
    names = ["adaln", "base", "input_embed", "blk0.x_in", "blk0.n1", "final_norm", "vout"]
    for j in range(DEPTH):
        names += [f"blk{j}.{s}" for s in ("qkv", "ctx", "x_attn", "ff1", "x_ff")]
        if lnf:
            names += [f"blk{j}.stats2"] + ([f"blk{j}.stats1"] if j > 0 else [])
        elif j > 0:
            names.append(f"blk{j}.n1")
    return names


def _cols(name):
    s = name.split(".")[-1]
    return {"adaln": DEPTH * 6 * D + 2 * D, "qkv": 3 * INNER, "ctx": INNER, "ff1": FF, "stats1": 2, "stats2": 2, "vout": MEL}.get(s, D)


GUARD = 8  # rows past the evaluation's own in every probe buffer: NaN before, NaN after


class probing:
    """with probing(made, rows, names, probe_eval) as bufs: ...  -- the probes set on the plan, cleared on the way out (an exception included)"""

    def __init__(self, made, rows, names, probe_eval=0):
        self.made, self.rows, self.names, self.ev = made, rows, names, probe_eval

    def __enter__(self):
        from eraxvif5tts_amd import _lib
        lib = _lib.load()
        self.bufs = {n: torch.full((1 if n == "adaln" else self.rows + GUARD, _cols(n)), float("nan"), device="cuda") for n in self.names}
        try:
            _lib.check(lib.f5_plan_set_option(self.made["plan"], b"probe_eval", self.ev), "probe_eval")
            for n, t in self.bufs.items():
                _lib.check(lib.f5_plan_set_probe(self.made["plan"], n.encode(), _lib.ptr(t)), n)
        except BaseException:
            self.__exit__()
            raise
        return self.bufs

    def __exit__(self, *exc):
        from eraxvif5tts_amd import _lib
        lib = _lib.load()
        _lib.check(lib.f5_plan_set_probe(self.made["plan"], None, None))
        _lib.check(lib.f5_plan_set_option(self.made["plan"], b"probe_eval", 0))
        return False


def _site_counts():
    return [G.site_gemm(s)[1] for s in (1, 2, 3, 4)]


# id -> B, N, precisions, probe_evals, knobs, durations, frames, expected modes, expected (family, bm) per site (None: not asserted), equality runs
FAST, W4 = G.FAM_FAST, G.FAM_W4
CASES = {
    # 8-wave kernel, statistics launches
    "2x300": dict(B=2, N=300, precs=("bf16", "fp16"), evs=(0, 2), modes=dict(rows=1200, rows_g=1200, lnf=1, ink_qkv=0, ink_ff1=0, split_v=0),
                  sites={1: (FAST, None), 2: (FAST, None), 3: (FAST, None), 4: (FAST, None)}, equal=True, embed=True),
    # padding rows; FF1 finishes the statistics in its kernel on the one-wave-per-SIMD kernel's 128-row tiles
    "2x900": dict(B=2, N=900, precs=("bf16", "fp16"), evs=(0,), modes=dict(rows=3600, rows_g=3840, lnf=1, ink_ff1=1, split_v=0),
                  sites={3: (W4, 128)}, equal=True),
    # q|k and v launched apart
    "3x1024_split_v": dict(B=3, N=1024, precs=("bf16",), evs=(0,), knobs=dict(gemm_w4=0), modes=dict(rows=6144, rows_g=6144, lnf=1, split_v=1),
                           sites={1: (FAST, None), 2: (FAST, None), 3: (FAST, None), 4: (FAST, None)}, qkv_launches=2),
    # 256-row tiles of the one-wave-per-SIMD kernel at all four sites, whole-line resid epilogue
    "8x1024": dict(B=8, N=1024, precs=("bf16",), evs=(0,), modes=dict(rows=16384, rows_g=16384, lnf=1, split_v=0),
                   sites={1: (W4, 256), 2: (W4, 256), 3: (W4, 256), 4: (W4, 256)}),
    # a key mask: rowbits on the out-projection
    "2x300_mask": dict(B=2, N=300, precs=("bf16",), evs=(0,), durations=[300, 211], modes=dict(rows=1200, lnf=1)),
    # rope_exp, gap rows, ragged attention
    "ragged_900_1000": dict(B=2, N=1952, precs=("bf16",), evs=(0,), frames=[900, 1000], modes=dict(rows=3904, rows_g=4096, lnf=1)),
}
PARAMS = [(cid, pn, ev) for cid, c in CASES.items() for pn in c["precs"] for ev in c["evs"]]


@pytest.mark.parametrize("cid,pname,ev", PARAMS, ids=[f"{c}-{p}-eval{e}" for c, p, e in PARAMS])
def test_every_stage_of_a_production_evaluation(models, cid, pname, ev):
    c = CASES[cid]
    made = models(pname)
    model, prec, B, N = made["model"], made["prec"], c["B"], c["N"]
    frames, durations = c.get("frames"), c.get("durations")
    nb = 2 * B if frames is None else 2
    rows = nb * N
    inp = _inputs(B, N, seed=B * 10000 + N + (7 if durations else 0), frames=frames)
    run = lambda **kw: _sample(model, inp, B, N, durations=durations, frames=frames, **kw)
    with G.knobs(**c.get("knobs", {})):
        out_plain, _ = run()
        md = G.eval_modes(made["plan"], nb, N)
        want = dict(c["modes"], r16=1, rmw=1, qs=int(prec == P_BF16))
        path = [] if {k: md[k] for k in want} == want else [f"modes {md}, intended {want}"]  # (asserted below, behind the printed figures)
        before = _site_counts()
        with probing(made, rows, _probe_names(lnf=True), ev) as bufs:
            out_probed, traj = run(traj=frames is None)
            md_probed = G.eval_modes(made["plan"], nb, N)
            launches = [a - b for a, b in zip(_site_counts(), before)]
            recs = {s: G.site_gemm(s)[0] for s in (1, 2, 3, 4)}
        assert md_probed == md, (md_probed, md)  # a probe enters no mode decision
        assert torch.equal(out_probed, out_plain)
    print(f"{cid} {pname} eval {ev}: {md}; site records {recs}; launches of one sample() per site {launches}")
    per_site = STEPS * DEPTH
    if launches != [per_site * c.get("qkv_launches", 1), per_site, per_site, per_site]:
        path.append(f"launches per site {launches}")
    for s, (fam, bm) in c.get("sites", {}).items():
        if not (recs[s][0] == fam and (bm is None or recs[s][1] == bm)):
            path.append(f"site {s} launched {recs[s]}, intended family {fam} with {bm or 'any'} token rows per tile")
    assert model.residual_fallbacks() == 0
    for n, t in bufs.items():  # the token rows, all of them, and nothing behind them
        assert torch.isfinite(t[:1 if n == "adaln" else rows]).all(), n
        assert n == "adaln" or t[rows:].isnan().all(), f"{n}: rows past the evaluation's own were written"

    lay = G.stage_layout(nb, N, durations=None if durations is None else durations * 2, frames=frames)
    valid, padded = G.stage_sample_rows(lay, seed=rows)
    shares = G.stage_shares(bufs, made["W"], lay, valid, prec, prec == P_BF16, DEPTH, 1, HEADS)
    if len(padded):  # a padded query row keeps its bits through the out-projection (rowbits)
        assert durations is not None
        for j in range(DEPTH):
            x_prev = bufs["blk0.x_in"] if j == 0 else bufs[f"blk{j - 1}.x_ff"]
            assert torch.equal(bufs[f"blk{j}.x_attn"][padded.cuda()], x_prev[padded.cuda()]), j
    if c.get("embed") and prec == P_BF16 and ev == 0:  # the input embedding and the position-conv branch, at the smallest case only
        x = traj[ev].reshape(B * N, MEL)[valid % (B * N)].cpu()  # (Euler: evaluation e reads traj[e]; both CFG halves read the same rows)
        kw = dict(x=x, w=made["W"]["x_w"], base=G._take(bufs["base"], valid))
        ie = G._take(bufs["input_embed"], valid)
        e_emu = G.stage_row_errors(G.stage_emulate(prec, "input_embed", **kw), G.stage_ref("input_embed", **kw))
        e_dev = G.stage_row_errors(ie, G.stage_ref("input_embed", **kw))
        shares["input_embed"] = (float(e_dev.max()) / (G.STAGE_MARGIN * float(e_emu.max())), float(e_emu.max()), float(e_dev.max()))
        kw = dict(ie=bufs["input_embed"][:rows].float().cpu().reshape(nb, N, D), conv=made["W"]["conv"])
        R = G.stage_ref("x_in", **kw).reshape(rows, D)[valid]
        E = G.stage_emulate(prec, "x_in", **kw).reshape(rows, D)[valid]
        e_emu, e_dev = G.stage_row_errors(E, R), G.stage_row_errors(G._take(bufs["blk0.x_in"], valid), R)
        shares["blk0.x_in"] = (float(e_dev.max()) / (G.STAGE_MARGIN * float(e_emu.max())), float(e_emu.max()), float(e_dev.max()))
        for n in ("input_embed", "blk0.x_in"):
            print(f"  {n}: restatement's worst row {shares[n][1]:.3e}, worst row {shares[n][2]:.3e} = {shares[n][0]:.3f} of the bound")
    print(f"  worst stage of {cid} {pname} eval {ev}: {max(v[0] for v in shares.values()):.3f} of the bound "
          f"= {G.STAGE_MARGIN * max(v[0] for v in shares.values()):.2f} x the restatement's worst row")
    G.stage_check(f"{cid} {pname} eval {ev}", shares)
    assert not path, f"{cid} {pname}: the case no longer takes the path it is there for: {path}"

    if c.get("equal"):  # replayed: the probed call runs eagerly, gives the replay's bits and touches no cached capture
        with G.knobs(**c.get("knobs", {})):
            run(use_graph=True)
            out_replay, _ = run(use_graph=True)
            counters = (G.plan_option(model, "graph_captures"), G.plan_option(model, "graph_replays"))
            with probing(made, rows, ["blk1.qkv", "vout"], ev):
                out_probed, _ = run(use_graph=True)
            assert (G.plan_option(model, "graph_captures"), G.plan_option(model, "graph_replays")) == counters
            assert torch.equal(out_probed, out_replay)
            out_again, _ = run(use_graph=True)
            assert G.plan_option(model, "graph_replays") == counters[1] + 1 and torch.equal(out_again, out_replay)


@pytest.mark.parametrize("pname", ["bf16", "fp16"])
def test_probe_names_are_checked_before_any_work(models, pname):
    """An unknown name is F5_EINVAL from the setter; a name whose buffer the running mode does not hold is F5_ESTATE from the call, and the call
    has then written nothing."""
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    made = models(pname)
    model, plan = made["model"], made["plan"]
    buf = torch.zeros(1200 + GUARD, 3 * INNER, device="cuda")
    for name in ("blk3.qkv", "blk0.stats1", "blk1.x_in", "blk1.out", "n1", "blk.qkv", "blk1.", "blk1.qkv "):
        assert lib.f5_plan_set_probe(plan, name.encode(), _lib.ptr(buf)) == F5_EINVAL, name
    assert lib.f5_plan_set_option(plan, b"probe_eval", -1) == F5_EINVAL
    inp = _inputs(2, 300, seed=5)
    cond, text, lens, y0 = inp
    tg = _tgrid().contiguous()
    ids, l32 = text.to("cuda", torch.int32).contiguous(), lens.to("cuda", torch.int32).contiguous()
    out = torch.full_like(cond, 7.0)
    call = lambda: lib.f5_sample(plan, 2, 300, _lib.ptr(cond), _lib.ptr(ids), ids.shape[1], _lib.ptr(l32), None, _lib.ptr(y0), C.c_void_p(tg.data_ptr()), STEPS,
                                 2.0, 0, _lib.ptr(out), None, 0, _lib.stream_ptr())
    try:
        _lib.check(lib.f5_plan_set_probe(plan, b"blk1.n1", _lib.ptr(buf)))  # the fold runs no first pass in block 1
        assert call() == F5_ESTATE
        _lib.check(lib.f5_plan_set_probe(plan, None, None))
        _lib.check(lib.f5_plan_set_probe(plan, b"blk1.qkv", _lib.ptr(buf)))
        _lib.check(lib.f5_plan_set_option(plan, b"probe_eval", STEPS))  # past the loop's evaluations
        assert call() == F5_EINVAL
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (buf == 0).all()
        with G.knobs(ln_fold=0):  # unfolded: block 1 has its first pass, and no statistics
            _lib.check(lib.f5_plan_set_option(plan, b"probe_eval", 0))
            _lib.check(lib.f5_plan_set_probe(plan, b"blk1.n1", _lib.ptr(buf)))
            assert call() == 0
            _lib.check(lib.f5_plan_set_probe(plan, b"blk1.stats2", _lib.ptr(buf)))
            assert call() == F5_ESTATE
    finally:
        _lib.check(lib.f5_plan_set_probe(plan, None, None))
        _lib.check(lib.f5_plan_set_option(plan, b"probe_eval", 0))
    torch.cuda.synchronize()
    assert model.residual_fallbacks() == 0
