"""Block subsets of a DiT plan (include/f5hip.h: f5_plan_set_blocks; DiT.set_active_blocks): a plan with subset S computes, bit for bit, what
DiT.pruned(S) -- the model whose blocks are S renumbered -- computes, in forward() with a time per utterance (every precision mode), in sample()
(fp32 mode; bf16 against the pruned model without the LayerNorm fold, which a subset switches off) and in the ragged sampler; each result is also
within the stage tolerance of the CPU oracle on the renumbered weights.  A full list [0 .. depth) is a subset like any other (fold off); clearing
the subset gives back the bits of a run made before any subset was set, fold table, captured graphs and caches included.

Model: tiny_base widths (dim 128, 2 heads, conv text blocks) at depth 6, random weights.  B = 2, N = 56, lengths 56 and 44, 18 text ids: small
enough for the reference kernels of the small-batch path, with a key mask and padded rows; one case at 512 token rows runs the LayerNorm fold."""
import ctypes as C

import pytest
import torch

from conftest import golden_arch, load_golden, rel_l2
from eraxvif5tts_amd import _lib
from eraxvif5tts_amd.eval import prune_state_dict
from oracle import cpu_ref
from test_gpu_fp16_model import STAGE_TOL as STAGE_TOL_FP16
from test_gpu_model import STAGE_TOL

pytestmark = pytest.mark.gpu
TOL = {**STAGE_TOL, "fp16": STAGE_TOL_FP16}  # (fp16 mode: the bound tests/test_gpu_fp16_model.py holds the same stages to)
V, DEPTH = 60, 6
SUBSETS = [[0, 1, 4, 5], [1, 3], [5], [0, 1, 2, 3, 4, 5]]
IDS = ["0145", "13", "5", "all"]
B, N, DUR, LENS, NT = 2, 56, [56, 44], [20, 16], 18


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _arch():
    return {**golden_arch(load_golden("tiny_base")), "depth": DEPTH}


@pytest.fixture(scope="module")
def weights():
    return cpu_ref.random_dit_weights(_arch(), V, seed=606)


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(56)
    x = torch.randn(B, N, 100, generator=g)
    cond = torch.randn(B, N, 100, generator=g) * 2 - 3
    text = torch.randint(0, V, (B, NT), generator=g)
    text[1, 13:] = -1
    time = torch.tensor([0.3125, 0.82])
    for b in range(B):
        x[b, DUR[b]:] = 0
        cond[b, LENS[b]:] = 0
    mask = cpu_ref.lens_to_mask(torch.tensor(DUR))
    return x, cond, text, time, mask


@pytest.fixture(scope="module")
def oracle_forward(weights, inputs):
    """cpu_ref.dit_forward on the renumbered weights, computed once per subset and kept unchanged"""
    x, cond, text, time, mask = inputs
    cache = {}

    def get(S, trace=None):
        key = tuple(S)
        if key not in cache or trace is not None:
            out = cpu_ref.dit_forward(prune_state_dict(weights, S), {**_arch(), "depth": len(S)}, x, cond, text, time, False, False, mask=mask, trace=trace)
            cache[key] = out
        return cache[key]
    return get


def _models(weights, prec, method="euler"):
    import gpu_helpers as G
    return G.make_cfm(_arch(), V, weights, prec, method=method)


def _pruned_cfm(cfm, S):
    from eraxvif5tts_amd.model import CFM
    return CFM(transformer=cfm.transformer.pruned(S).cuda(), num_channels=100, mel_spec_kwargs={"mel_spec_type": "vocos"},
               odeint_kwargs=dict(cfm.odeint_kwargs)).cuda()


def _forward(dit, inputs):
    x, cond, text, time, mask = [t.cuda() for t in inputs]
    out = dit(x=x, cond=cond, text=text, time=time, mask=mask, drop_audio_cond=False, drop_text=False, cache=False)
    return out.cpu()


def _sample_kw(inputs):
    _, cond, text, _, _ = inputs
    g = torch.Generator().manual_seed(7)
    y0 = torch.randn(B, N, 100, generator=g)
    y0[1, DUR[1]:] = 0
    return dict(cond=cond[:, :max(LENS)].cuda(), text=text.cuda(), duration=torch.tensor(DUR).cuda(), lens=torch.tensor(LENS).cuda(), steps=3,
                cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, use_graph=False)


def _valid(t):
    return torch.cat([t[b, :DUR[b]] for b in range(B)])


@pytest.mark.parametrize("S", SUBSETS, ids=IDS)
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_forward_equals_the_pruned_model_bit_for_bit(weights, inputs, oracle_forward, prec, S):
    import gpu_helpers as G
    cfm = _models(weights, prec)
    dit = cfm.transformer
    dit.set_active_blocks(S)
    got = _forward(dit, inputs)
    assert dit.active_blocks == tuple(S)
    want = _forward(dit.pruned(S), inputs)
    assert torch.equal(got, want), float((got - want).abs().max())
    err = rel_l2(_valid(got), _valid(oracle_forward(S)))
    print(f"  {prec} {S}: {err:.3e} of the oracle")
    assert err < TOL[prec]
    if len(S) == DEPTH:  # the full list is a subset: equal to the call with none under ln_fold = 0 (here: nothing folds a per-utterance time)
        dit.set_active_blocks(None)
        with G.knobs(ln_fold=0):
            assert torch.equal(_forward(dit, inputs), got)
    else:
        dit.set_active_blocks(None)
        assert not torch.equal(_forward(dit, inputs), got)  # (the removed blocks do something)


@pytest.mark.parametrize("S", SUBSETS, ids=IDS)
def test_sample_fp32_equals_the_pruned_model_bit_for_bit(weights, inputs, S):
    cfm = _models(weights, "fp32")
    kw = _sample_kw(inputs)
    before, _ = cfm.sample(**kw)
    cfm.transformer.set_active_blocks(S)
    got, traj = cfm.sample(**kw)
    want, wtraj = _pruned_cfm(cfm, S).sample(**kw)
    assert torch.equal(got, want) and torch.equal(traj, wtraj)
    replay = [cfm.sample(**{**kw, "use_graph": True})[0] for _ in range(2)]  # capture + replay under the subset
    assert torch.equal(replay[0], got) and torch.equal(replay[1], got)
    cfm.transformer.set_active_blocks(None)
    after, _ = cfm.sample(**{**kw, "use_graph": True})
    assert torch.equal(after, before)


def test_sample_midpoint_fp32_equals_the_pruned_model(weights, inputs):
    S = SUBSETS[0]
    cfm = _models(weights, "fp32", method="midpoint")
    kw = _sample_kw(inputs)
    cfm.transformer.set_active_blocks(S)
    got, _ = cfm.sample(**kw)
    want, _ = _pruned_cfm(cfm, S).sample(**kw)
    assert torch.equal(got, want)


@pytest.mark.parametrize("S", SUBSETS, ids=IDS)
def test_sample_bf16_equals_the_unfolded_pruned_model(weights, inputs, S):
    import gpu_helpers as G
    cfm = _models(weights, "bf16")
    kw = _sample_kw(inputs)
    cfm.transformer.set_active_blocks(S)
    got, _ = cfm.sample(**kw)
    with G.knobs(ln_fold=0):
        want, _ = _pruned_cfm(cfm, S).sample(**kw)
        if len(S) == DEPTH:
            cfm.transformer.set_active_blocks(None)
            none, _ = cfm.sample(**kw)
            assert torch.equal(none, got)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.isfinite(got).all()


def test_clearing_the_subset_restores_the_folded_sampler(weights):
    """512 token rows (one utterance of 256 frames, both CFG halves): the bf16 sampler runs the LayerNorm fold.  Under a subset no table is held
    and the result is the unfolded pruned model's; cleared, the table is back and the bits are those of the first call, eager and replayed."""
    import gpu_helpers as G
    cfm = _models(weights, "bf16")
    dit = cfm.transformer
    g = torch.Generator().manual_seed(256)
    n = 256
    kw = dict(cond=(torch.randn(1, 40, 100, generator=g) * 2 - 3).cuda(), text=torch.randint(0, V, (1, 30), generator=g).cuda(), duration=n, steps=3,
              cfg_strength=2.0, sway_sampling_coef=-1.0, y0=torch.randn(1, n, 100, generator=g))
    before = [cfm.sample(**kw, use_graph=ug)[0] for ug in (False, True, True)]
    assert torch.equal(before[0], before[1]) and torch.equal(before[0], before[2])
    folded = G.plan_option(dit, "ln_fold_active")
    S = [0, 1, 4, 5]
    dit.set_active_blocks(S)
    got = [cfm.sample(**kw, use_graph=ug)[0] for ug in (False, True, True)]
    assert G.plan_option(dit, "ln_fold_active") == 0
    with G.knobs(ln_fold=0):
        want, _ = _pruned_cfm(cfm, S).sample(**kw, use_graph=False)
    for t in got:
        assert torch.equal(t, want)
    dit.set_active_blocks(None)
    after = [cfm.sample(**kw, use_graph=ug)[0] for ug in (True, False)]
    assert G.plan_option(dit, "ln_fold_active") == folded
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[0])


def test_ragged_sample_under_a_subset_equals_its_batch_1_calls(weights):
    cfm = _models(weights, "fp32")
    cfm.transformer.set_active_blocks([0, 1, 4, 5])
    g = torch.Generator().manual_seed(44)
    cond = (torch.randn(1, 16, 100, generator=g) * 2 - 3).cuda()
    durs = [56, 44]
    texts = [torch.randint(0, V, (1, k), generator=g).cuda() for k in (18, 13)]
    y0s = [torch.randn(1, d, 100, generator=g).cuda() for d in durs]
    kw = dict(steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0)
    ref = [cfm.sample(cond=cond, text=t, duration=d, y0=y, return_trajectory=False, use_graph=False, **kw)[0] for t, d, y in zip(texts, durs, y0s)]
    got = cfm.sample_ragged(cond, texts, durs, y0s=y0s, **kw)
    for a, b, d in zip(got, ref, durs):
        assert a.shape == (1, d, 100) and torch.isfinite(a).all()
        assert torch.equal(a, b), (d, float((a - b).abs().max()))
    pruned = _pruned_cfm(cfm, [0, 1, 4, 5]).sample_ragged(cond, texts, durs, y0s=y0s, **kw)
    for a, b in zip(got, pruned):
        assert torch.equal(a, b)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_taps_are_named_by_position(weights, inputs, prec):
    """Under [0, 1, 4, 5] the stream after position j is "blk<j>.out", j = 0 .. 3, and equals the renumbered oracle's; "blk4.out" is no stage of
    that model and is never written."""
    S = SUBSETS[0]
    dit = _models(weights, prec).transformer
    dit.set_active_blocks(S)
    x, cond, text, time, mask = inputs
    trace = {}
    cpu_ref.dit_forward(prune_state_dict(weights, S), {**_arch(), "depth": len(S)}, x, cond, text, time, False, False, mask=mask, trace=trace)
    plan = dit.plan(B, N, 1)
    taps = {f"blk{j}.out": torch.full((B, N, 128), float("nan")).cuda() for j in range(5)}
    taps["input_embed"] = torch.full((B, N, 128), float("nan")).cuda()
    for k, v in taps.items():
        dit.set_tap(plan, k, v)
    _forward(dit, inputs)
    torch.cuda.synchronize()
    dit.set_tap(plan, None, None)
    for k in ["input_embed"] + [f"blk{j}.out" for j in range(4)]:
        assert rel_l2(taps[k].cpu(), trace[k]) < TOL[prec], k
    assert bool(torch.isnan(taps["blk4.out"]).all())


def test_refusals(weights):
    from eraxvif5tts_amd.model import MMDiT, UNetT
    lib = _lib.load()
    dit = _models(weights, "fp32").transformer
    plan = dit.plan(B, N, 1)

    def set_blocks(h, blocks):
        arr = (C.c_int32 * max(len(blocks), 1))(*blocks)
        return lib.f5_plan_set_blocks(h, arr, len(blocks))

    def get_blocks(h):
        arr = (C.c_int32 * 16)()
        n = lib.f5_plan_get_blocks(h, arr, 16)
        return list(arr[:n])

    assert set_blocks(plan, [1, 3]) == 0 and get_blocks(plan) == [1, 3]
    for bad in ([], [2, 1], [0, 0], [6], [-1], [0, 1, 2, 3, 4, 5, 6]):
        assert set_blocks(plan, bad) == -1 and "f5_plan_set_blocks" in _lib.last_error(), bad  # F5_EINVAL
        assert get_blocks(plan) == [1, 3]  # refused before anything changes
    assert lib.f5_plan_set_blocks(plan, None, 3) == -1 and get_blocks(plan) == [1, 3]
    assert lib.f5_plan_set_blocks(plan, None, 0) == 0 and get_blocks(plan) == []
    for bad in ([], [2, 1], [0, 0], [6]):
        with pytest.raises(ValueError):
            dit.set_active_blocks(bad)
        assert dit.active_blocks is None
    for cls, extra in ((UNetT, {}), (MMDiT, {})):
        m = cls(dim=128, depth=4, heads=2, ff_mult=2, text_num_embeds=V, mel_dim=100, precision="fp32", **extra).cuda()
        with pytest.raises(NotImplementedError) as e:
            m.set_active_blocks([0, 1])
        h = m.plan(1, 64, 1)
        assert set_blocks(h, [0, 1]) == _lib.F5_ENOTSUP
        assert _lib.last_error() == str(e.value)  # the library's message
        assert lib.f5_plan_set_blocks(h, None, 0) == 0
