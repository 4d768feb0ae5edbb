"""hipGraph replay and plan reuse on inputs UNLIKE the captured call's.

The sampler's design rests on one invariant ("Graph capture: the replay invariant"): every per-call VALUE is staged into plan buffers
outside the captured region, and every node inside it reads those buffers when the graph is launched.  A test that replays the inputs it
captured cannot see a node that is skipped or that replays stale bytes -- its destination still holds the right bytes from the capture.  Here
every replay runs on other values than its capture: all inputs at once, one input at a time, another time grid of the same length, and after
other entry points have used the same plan.

Reference, everywhere: the EAGER call (use_graph=False) on the same inputs, made on a SECOND model object built from the same weights -- it
shares no plan, graph or staging buffer with the object under test.  Comparison: torch.equal on the output and on the trajectory; no
tolerance.  Whether a call captured or replayed is read from the plan's counters (include/f5hip.h: "graph_captures", "graph_replays"; a
capture's own launch is no replay), so a test that quietly captured again fails.

Shapes: B = 2, N = 300 (no multiple of 128: with CFG the second half starts at row 600 and the row-mask bytes of a tile mix both halves),
24 text columns, 2 steps, CFG 2; the smallest models (the hazards sit in graph nodes, not in tile shapes).  One plan of 3 x 384, 8 evaluation
times per model object holds every call of a test, the ragged ones included."""
import ast

import pytest
import torch

from conftest import golden_arch, golden_weights, load_golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
B, N, NT, MEL, V, STEPS, CFG = 2, 300, 24, 100, 40, 2, 2.0
PLAN = (3, 384, 8)  # max_batch, max_seq, max_evals: 2 x 300, the ragged frames below (768 rows with gaps), rk4's 8 evaluation times
FRAMES = (300, 129, 257)
MODES = {"bf16-tuned": ("bf16", True), "bf16": ("bf16", False), "fp16": ("fp16", False), "fp32": ("fp32", False)}  # tuned: set_kernels(gemm=1, attn=1)
DIT_KINDS = ("tiny_base", "tiny_v1", "long_skip")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@pytest.fixture(autouse=True)
def _launcher_defaults(monkeypatch):
    for k in ("F5HIP_GEMM_KERNEL", "F5HIP_ATTN_KERNEL", "F5HIP_PRECISION", "F5HIP_ROPE_LAYOUT"):
        monkeypatch.delenv(k, raising=False)


# ----------------------------------------------------------------------------- models, inputs, the eager twin
_SPECS, _INPUTS, _TWINS, _EAGER = {}, {}, {}, {}


def _spec(kind):
    """(backbone, arch, vocab, weights) -- the tiny golden architectures; long_skip: tiny_base + long_skip_connection on seeded weights"""
    if kind not in _SPECS:
        if kind in ("tiny_base", "tiny_v1"):
            z = load_golden(kind)
            _SPECS[kind] = ("DiT", golden_arch(z), int(z["vocab"]), golden_weights(z))
        elif kind == "long_skip":
            arch = {**golden_arch(load_golden("tiny_base")), "long_skip_connection": True}
            _SPECS[kind] = ("DiT", arch, 60, cpu_ref.random_dit_weights(arch, 60, seed=216))
        else:
            z = load_golden({"unett": "tiny_unett", "mmdit": "tiny_mmdit"}[kind])
            arch, vocab = ast.literal_eval(str(z["a.arch"])), int(z["a.vocab"])
            rand = {"unett": cpu_ref.random_unett_weights, "mmdit": cpu_ref.random_mmdit_weights}[kind]
            _SPECS[kind] = ({"unett": "UNetT", "mmdit": "MMDiT"}[kind], arch, vocab, rand(arch, vocab, seed=int(z["a.seed"])))
        assert _SPECS[kind][2] >= V
    return _SPECS[kind]


def _build(kind, mode):
    """A model object of its own (weights uploaded again, a plan of its own) with the one plan PLAN and the mode's kernel choice."""
    from eraxvif5tts_amd import model as M
    backbone, arch, vocab, W = _spec(kind)
    prec, tuned = MODES[mode]
    m = getattr(M, backbone)(**arch, text_num_embeds=vocab, mel_dim=MEL, precision=prec)
    sd = m.state_dict()
    missing = [k for k in sd if k not in W and k != "rotary_embed.inv_freq"]
    assert not missing, missing
    m.load_state_dict({k: v for k, v in W.items() if k in sd}, strict=False)
    m = m.cuda()
    m.plan(*PLAN)
    if tuned:
        m.set_kernels(gemm=1, attn=1)  # (acts on the plans that exist)
    return m


def _inputs(n=N, seed=300):
    import gpu_helpers as G
    if (n, seed) not in _INPUTS:
        _INPUTS[n, seed] = G.replay_inputs(B, n, NT, MEL, V, seed)
    return _INPUTS[n, seed]


def _sample(m, d, graph, method="euler", masked=False, sway=-1.0, cfg=CFG, use_mask=True, text=None):
    import gpu_helpers as G
    out, traj = m.native_sample(d["cond"], G.replay_text(d) if text is None else text, d["lens"], d["durations"], d["y0"], cpu_ref.time_grid(STEPS, sway),
                                STEPS, cfg, method=method, use_mask=use_mask, return_trajectory=True, use_graph=graph,
                                cond_mask=d["cond_mask"] if masked else None)
    torch.cuda.synchronize()
    return out.cpu(), traj.cpu()


def _ragged_of(d):
    """The ragged call's inputs from a 3-row input set: utterance u = the first FRAMES[u] frames of row u, and a guidance value of its own"""
    cat = lambda k: torch.cat([d[k][u, :f] for u, f in enumerate(FRAMES)])
    return dict(cond=cat("cond"), y0=cat("y0"), cond_mask=cat("cond_mask"), lens=d["lens"], text_ids=d["text_ids"], text_len=d["text_len"], cfg=d["cfg"])


def _ragged_inputs():
    import gpu_helpers as G
    if "ragged" not in _INPUTS:
        a, b = G.replay_inputs(len(FRAMES), max(FRAMES), NT, MEL, V, 129)
        a["cfg"], b["cfg"] = [2.0, 0.5, 3.5], [0.7, 3.0, 1.5]
        assert all(int(s["lens"][u]) < f for s in (a, b) for u, f in enumerate(FRAMES))
        _INPUTS["ragged"] = _ragged_of(a), _ragged_of(b)
    return _INPUTS["ragged"]


def _sample_ragged(m, r, graph, method="euler"):
    import gpu_helpers as G
    out = m.native_sample_ragged(r["cond"], G.replay_text(r), r["lens"], list(FRAMES), r["y0"], cpu_ref.time_grid(STEPS, -1.0), STEPS, r["cfg"],
                                 method=method, use_graph=graph, cond_mask=r["cond_mask"])
    torch.cuda.synchronize()
    return out.cpu()


class Case:
    """The model under test (graph calls, one plan) and its eager twin (a second object from the same weights, shared by the tests of a
    (kind, mode); its results are computed once per (inputs, arguments), shared and never written to)."""

    def __init__(self, kind, mode):
        self.key = (kind, mode)
        self.m = _build(kind, mode)
        if self.key not in _TWINS:
            _TWINS[self.key] = _build(kind, mode)
        self.twin = _TWINS[self.key]
        self.captures = self.replays = 0  # what the plan's counters must read

    def eager(self, label, d, **kw):
        k = (self.key, label, tuple(sorted((a, str(b.tolist()) if torch.is_tensor(b) else b) for a, b in kw.items())))
        if k not in _EAGER:
            _EAGER[k] = (_sample_ragged if "cfg" in d else _sample)(self.twin, d, False, **kw)
        return _EAGER[k]

    def graph(self, label, d, expect, **kw):
        """A graph call on the model under test: it equals the twin's eager call bit for bit, and it did what `expect` says ("capture" or
        "replay") -- and nothing else -- to the counters.  -> the eager result"""
        import gpu_helpers as G
        got = (_sample_ragged if "cfg" in d else _sample)(self.m, d, True, **kw)
        want = self.eager(label, d, **kw)
        self.captures += expect == "capture"
        self.replays += expect == "replay"
        have = (G.plan_option(self.m, "graph_captures"), G.plan_option(self.m, "graph_replays"))
        assert have == (self.captures, self.replays), (self.key, label, kw, expect, "captures, replays", have, "expected", (self.captures, self.replays))
        pairs = [("out", got, want)] if "cfg" in d else [("out", got[0], want[0]), ("trajectory", got[1], want[1])]
        for name, a, b in pairs:
            assert torch.isfinite(b).all(), (self.key, label, name)
            assert torch.equal(a, b), (self.key, label, kw, expect, name, f"{int((a != b).sum())} elements differ, max {float((a - b).abs().max()):.3e}")
        if MODES[self.key[1]][0] != "fp32":
            assert self.m.residual_fallbacks() == 0  # (a range-guard rerun would capture a second time)
        return want

    def differ(self, x, y):
        return not torch.equal(x if torch.is_tensor(x) else x[0], y if torch.is_tensor(y) else y[0])


# ----------------------------------------------------------------------------- (a) + (e): all inputs at once, every backbone and mode
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", DIT_KINDS + ("unett", "mmdit"))
def test_all_inputs_change_between_capture_and_replays(kind, mode):
    """Capture on A; replay on B, on A, on B -- cond, text ids, text lengths, lens, durations (in both directions under one N) and y0 all
    differ.  Then the same with an edit mask (f5_sample_masked: a capture of its own).  Each result equals its eager twin; 2 captures and 6
    replays in all.  long_skip captures the long-skip save of the stream, unett the skip saves, mmdit the restart of the text stream."""
    a, b = _inputs()
    c = Case(kind, mode)
    for masked in (False, True):
        kw = dict(masked=True) if masked else {}
        ea = c.graph("A", a, "capture", **kw)
        eb = c.graph("B", b, "replay", **kw)
        assert c.differ(ea, eb), "A and B give the same result: the replays prove nothing"
        c.graph("A", a, "replay", **kw)
        c.graph("B", b, "replay", **kw)
    assert (c.captures, c.replays) == (2, 6)


# ----------------------------------------------------------------------------- (b): one input at a time
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("field", ["cond", "text_ids", "text_len", "lens", "durations", "y0", "cond_mask"])
def test_one_changed_input_reaches_the_replay(field, mode):
    """Capture on A, replay on A with exactly `field` taken from B (DiT, CFG on: the durations case drives the captured copy of the key mask
    into the CFG half; cond_mask goes through f5_sample_masked in both calls).  The field changes the eager result, so a replay that read the
    capture's value would differ."""
    import gpu_helpers as G
    a, b = _inputs()
    kw = dict(masked=True) if field == "cond_mask" else {}
    c = Case("tiny_base", mode)
    mixed = G.replay_swap(a, b, field)
    assert [k for k in G.REPLAY_FIELDS if mixed[k] is not a[k]] == [field]
    assert c.differ(c.eager("A", a, **kw), c.eager("A+" + field, mixed, **kw)), f"{field} does not change the eager result"
    c.graph("A", a, "capture", **kw)
    c.graph("A+" + field, mixed, "replay", **kw)
    c.graph("A", a, "replay", **kw)


# ----------------------------------------------------------------------------- (c): another time grid of the same length
@pytest.mark.parametrize("mode", list(MODES))
def test_a_time_grid_of_the_same_length_with_other_values(mode):
    """sway_sampling_coef -1 against None at the same step count: other evaluation times, other step widths.  Without a LayerNorm-fold table
    (fp32 mode; 16-bit modes where ln_fold_active reads 0) the key does not change: the one capture is replayed and reads the restaged
    coefficient words and AdaLN rows.  With a table, the table's id is part of the key: the second grid captures once, and going back to the
    first grid replays the first capture (both tables are alive: the model keeps two)."""
    import gpu_helpers as G
    a, b = _inputs()
    c = Case("tiny_base", mode)
    e1 = c.graph("A", a, "capture", sway=-1.0)
    fold = G.plan_option(c.m, "ln_fold_active")
    print(f"{mode}: ln_fold_active = {fold}")
    assert fold == 0 or mode != "fp32"
    assert c.differ(e1, c.eager("A", a, sway=None)), "the grid does not change the eager result"
    c.graph("B", b, "capture" if fold else "replay", sway=None)
    assert G.plan_option(c.m, "ln_fold_active") == fold
    c.graph("A", a, "replay", sway=None)
    c.graph("B", b, "replay", sway=-1.0)
    again = c.graph("A", a, "replay", sway=-1.0)
    assert torch.equal(again[0], e1[0]) and torch.equal(again[1], e1[1])
    assert c.captures == (2 if fold else 1)


# ----------------------------------------------------------------------------- (d): what is part of the key
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_a_changed_key_captures_anew_and_the_old_capture_survives(mode):
    """durations=None against given, a text with more columns, CFG 0 against 2, another method: each is a capture of its own that equals its
    eager twin; going back to the first call replays the first capture, on other values (B) and then with the first call's bits (A)."""
    a, b = _inputs()
    c = Case("tiny_base", mode)
    first = c.graph("A", a, "capture")
    g = torch.Generator().manual_seed(40)
    wide = torch.randint(0, V, (B, 40), generator=g)
    wide[1, 33:] = -1
    for label, kw in (("nomask", dict(use_mask=False)), ("wide", dict(text=wide)), ("cfg0", dict(cfg=0.0)), ("midpoint", dict(method="midpoint")),
                      ("rk4", dict(method="rk4"))):
        other = c.graph("B " + label, b, "capture", **kw)
        assert c.differ(other, c.eager("B", b)), label
        c.graph("A " + label, a, "replay", **kw)
        c.graph("B", b, "replay")
        again = c.graph("A", a, "replay")
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    assert c.captures == 6


# ----------------------------------------------------------------------------- (e): UNetT and MMDiT, one input at a time; rk4
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("field", ["y0", "text_ids"])
@pytest.mark.parametrize("kind", ["unett", "mmdit"])
def test_other_backbones_one_changed_input(kind, field, mode):
    """y0 only and text only between a capture and its replay: UNetT's captured skip saves copy a stream that depends on both, MMDiT's captured
    restart of the text stream copies the text embeddings of the call."""
    import gpu_helpers as G
    a, b = _inputs()
    c = Case(kind, mode)
    mixed = G.replay_swap(a, b, field)
    assert c.differ(c.eager("A", a), c.eager("A+" + field, mixed)), f"{field} does not change the eager result"
    c.graph("A", a, "capture")
    c.graph("A+" + field, mixed, "replay")
    c.graph("A", a, "replay")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_unett_rk4_all_inputs(mode):
    """(a) with four evaluations per step: 2 x depth / 2 skip saves per evaluation, 8 evaluations per replay."""
    a, b = _inputs()
    c = Case("unett", mode)
    ea = c.graph("A", a, "capture", method="rk4")
    eb = c.graph("B", b, "replay", method="rk4")
    assert c.differ(ea, eb)
    c.graph("A", a, "replay", method="rk4")


# ----------------------------------------------------------------------------- (f): ragged
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_ragged_replay_on_other_inputs(mode):
    """f5_sample_ragged_ex with plan option ragged_graph = 1, frames (300, 129, 257): capture on A; replay on B (other cond, text ids, text
    lengths within the same 24 columns, lens, y0, edit masks, guidance vector); replay on A.  Then text only: the captured 2D copies move
    each utterance's text row to the scratch row the text embedding reads."""
    ra, rb = _ragged_inputs()
    c = Case("tiny_base", mode)
    ea = c.graph("rA", ra, "capture")
    eb = c.graph("rB", rb, "replay")
    assert c.differ(ea, eb)
    assert torch.equal(c.graph("rA", ra, "replay"), ea)
    mixed = {**ra, "text_ids": rb["text_ids"], "text_len": rb["text_len"]}
    off = 0
    for u, f in enumerate(FRAMES):  # (every utterance's text changes its rows)
        assert c.differ(ea[off:off + f], c.eager("rA+text", mixed)[off:off + f]), u
        off += f
    c.graph("rA+text", mixed, "replay")
    assert (c.captures, c.replays) == (1, 3)


# ----------------------------------------------------------------------------- (g): other uses of the plan between capture and replay
def _interlopers(c, kind):
    """Calls on the model under test -- the same plan, the same stream -- that overwrite what a replay must rebuild or find restaged (text
    embeddings, hoisted input embedding, key mask, row-mask bytes, AdaLN rows, staged text and cond).  -> [(name, call)]"""
    g = torch.Generator().manual_seed(7)
    x, cond = torch.randn(B, N, MEL, generator=g).cuda(), (torch.randn(B, N, MEL, generator=g) * 2 - 3).cuda()
    text = torch.randint(0, V, (B, 31), generator=g).cuda()
    keys = (torch.arange(N)[None, :] < torch.tensor([N - 70, N])[:, None]).cuda()
    (_, plan), = c.m._plans

    def forward():  # (per-sample times, a caller's key mask; text embedding + forward entry on the plan)
        out = c.m(x=x, cond=cond, text=text, time=torch.tensor([0.37, 0.81]).cuda(), mask=keys, drop_audio_cond=False, drop_text=False, cache=False)
        assert torch.isfinite(out).all()

    def text_embed():
        assert torch.isfinite(c.m._text_embed(plan, text, N, True)).all()

    def smaller():  # (an eager uniform call, 1 x 100)
        sa, _ = _inputs(100, 100)
        one = {k: v[:1] for k, v in sa.items()}
        assert int(one["durations"][0]) == 100
        assert torch.isfinite(_sample(c.m, one, False)[0]).all()

    def ragged():  # (a ragged call with a capture of its own)
        c.captures += 1
        assert torch.isfinite(_sample_ragged(c.m, _ragged_inputs()[1], True)).all()

    calls = [("forward", forward), ("text_embed", text_embed), ("smaller", smaller)]
    return calls + [("ragged", ragged)] if kind != "mmdit" else calls


@pytest.mark.parametrize("kind,mode", [("tiny_base", "bf16"), ("tiny_base", "fp32"), ("mmdit", "bf16")])
def test_other_uses_of_the_plan_between_capture_and_replay(kind, mode):
    """After the capture on A: a forward with per-sample times and a caller's mask, a text embedding, an eager 1 x 100 sample and a ragged
    sample (DiT) run on the same plan; a replay follows each of them (B, A, B, A) and one follows all four.  Every replay equals its eager
    twin, the model still holds ONE plan, and the counters moved only by what the calls did themselves (the ragged call's own capture)."""
    a, b = _inputs()
    c = Case(kind, mode)
    c.graph("A", a, "capture")
    calls = _interlopers(c, kind)
    for i, (name, call) in enumerate(calls):
        call()
        torch.cuda.synchronize()
        assert len(c.m._plans) == 1, name
        c.graph("BA"[i % 2], (b, a)[i % 2], "replay")
    for name, call in calls:
        call() if name != "ragged" else _sample_ragged(c.m, _ragged_inputs()[0], True)  # (the ragged capture exists by now: a replay of it)
    c.replays += kind != "mmdit"
    c.graph("B", b, "replay")
    assert c.captures == (1 if kind == "mmdit" else 2)


# ----------------------------------------------------------------------------- the counters themselves
def test_the_counters_are_read_only_and_an_eager_call_moves_neither():
    import gpu_helpers as G
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    a, _ = _inputs()
    m = _build("tiny_base", "fp32")
    (_, plan), = m._plans
    for key in ("graph_captures", "graph_replays"):
        assert G.plan_option(m, key) == 0
        assert lib.f5_plan_set_option(plan, key.encode(), 0) == -1 and "unknown option" in _lib.last_error()
    _sample(m, a, False)
    assert (G.plan_option(m, "graph_captures"), G.plan_option(m, "graph_replays")) == (0, 0)
    _sample(m, a, True)
    assert (G.plan_option(m, "graph_captures"), G.plan_option(m, "graph_replays")) == (1, 0)
    _sample(m, a, True)
    assert (G.plan_option(m, "graph_captures"), G.plan_option(m, "graph_replays")) == (1, 1)
