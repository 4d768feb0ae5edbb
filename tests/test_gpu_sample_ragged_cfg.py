"""`f5_sample_ragged_ex` through `CFM.sample_ragged`: a guidance strength and a per-frame condition mask of its own for every utterance of a
ragged batch -- what `F5TTSWrapper.generate_batch` needs to put independent requests into one set of launches.  Acceptance is exactness:
every utterance's rows are `torch.equal` to its own batch-1 `CFM.sample` call at its own guidance strength / edit mask (the scalar kernels and
the per-row ones run the same operations).  The one toleranced check is the oracle comparison, at `TOL` of tests/test_gpu_model.py.
Set-up of test_ragged_sample_equals_batch1_samples: tiny_base, frames [300, 257, 411] over a 90-frame prompt, texts of 31 / 12 / 45 tokens,
explicit noise; in bf16 all utterances take the tuned kernels (>= 256 rows)."""
import ctypes as C

import pytest
import torch

from conftest import golden_arch, golden_weights, load_golden, rel_l2
from oracle import cpu_ref
from test_gpu_model import TOL

pytestmark = pytest.mark.gpu
DURS = [300, 257, 411]
NC = 90
CFGS = [2.0, 0.5, 3.5]
STEPS = {"euler": 3, "midpoint": 3, "rk4": 2, "heun3": 2}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


@pytest.fixture(scope="module")
def data():
    z = load_golden("tiny_base")
    arch, V, W = golden_arch(z), int(z["vocab"]), golden_weights(z)
    g = torch.Generator().manual_seed(77)
    cond = (torch.randn(1, NC, 100, generator=g) * 2 - 3).cuda()
    texts = [torch.randint(0, V, (1, n), generator=g).cuda() for n in (31, 12, 45)]
    y0s = [torch.randn(1, d, 100, generator=g).cuda() for d in DURS]
    return dict(arch=arch, V=V, W=W, cond=cond, texts=texts, y0s=y0s, cfms={}, refs={})


def _cfm(data, prec, method):
    import gpu_helpers as G
    if (prec, method) not in data["cfms"]:
        data["cfms"][prec, method] = G.make_cfm(data["arch"], data["V"], data["W"], prec, method=method)
    return data["cfms"][prec, method]


def _single(data, prec, method, u, cfg, edit=None):
    """the batch-1 call of utterance u at guidance `cfg` (computed once per case and shared)"""
    key = (prec, method, u, float(cfg), None if edit is None else tuple(edit))
    if key not in data["refs"]:
        em = None if edit is None else _edit(*edit)
        data["refs"][key] = _cfm(data, prec, method).sample(
            cond=data["cond"], text=data["texts"][u], duration=DURS[u], y0=data["y0s"][u], return_trajectory=False, use_graph=False,
            steps=STEPS[method], cfg_strength=cfg, sway_sampling_coef=-1.0, edit_mask=em)[0]
    return data["refs"][key]


def _edit(a, b):
    """edit_mask of sample(): True = keep the prompt frame, False over the edited span [a, b)"""
    m = torch.ones(1, NC, dtype=torch.bool)
    m[0, a:b] = False
    return m.cuda()


def _ragged(data, prec, method, cfg, **kw):
    return _cfm(data, prec, method).sample_ragged(data["cond"], data["texts"], DURS, y0s=data["y0s"], steps=STEPS[method], cfg_strength=cfg,
                                                  sway_sampling_coef=-1.0, **kw)


def _assert_equal(got, want, what):
    for u, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == (1, DURS[u], 100) and torch.isfinite(a).all(), (what, u)
        assert torch.equal(a, b), (what, u, float((a - b).abs().max()))


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4", "heun3"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_guidance_vector_equals_the_scalar_batch1_calls(data, prec, method):
    """(a)  and the vector is not ignored: utterance 1 at 0.5 differs from its call at utterance 0's 2.0"""
    got = _ragged(data, prec, method, CFGS, use_graph=False)
    _assert_equal(got, [_single(data, prec, method, u, c) for u, c in enumerate(CFGS)], (prec, method))
    assert not torch.equal(got[1], _single(data, prec, method, 1, CFGS[0]))


@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_equal_entries_give_the_bits_of_the_scalar_ragged_call(data, prec, method):
    """(b)"""
    _assert_equal(_ragged(data, prec, method, [2.0, 2.0, 2.0], use_graph=False), _ragged(data, prec, method, 2.0, use_graph=False), (prec, method))


@pytest.mark.parametrize("method", ["euler", "heun3"])
def test_a_replayed_graph_honours_the_current_vector(data, method):
    """(c)  two calls with the same shapes and different vectors, the second on the first one's capture"""
    other = [0.7, 3.0, 1.5]
    first = _ragged(data, "bf16", method, CFGS, use_graph=True)
    second = _ragged(data, "bf16", method, other, use_graph=True)
    _assert_equal(first, [_single(data, "bf16", method, u, c) for u, c in enumerate(CFGS)], "capture")
    _assert_equal(second, [_single(data, "bf16", method, u, c) for u, c in enumerate(other)], "replay")


def test_a_vector_on_both_sides_of_the_single_pass_branch_is_refused(data):
    """(d)  ValueError from Python before any library call; F5_EINVAL from the C entry, which writes nothing"""
    from eraxvif5tts_amd import _lib
    with pytest.raises(ValueError, match="1e-5"):
        _ragged(data, "fp32", "euler", [2.0, 0.0, 2.0])
    cfm = _cfm(data, "fp32", "euler")
    with pytest.raises(ValueError, match="1e-5"):
        cfm.transformer.native_sample_ragged(torch.zeros(sum(DURS), 100), torch.zeros(3, 4, dtype=torch.long), torch.tensor([NC] * 3), DURS,
                                             torch.zeros(sum(DURS), 100), torch.linspace(0, 1, 3), 2, [2.0, 0.0, 2.0])
    with pytest.raises(ValueError):
        _ragged(data, "fp32", "euler", [2.0, 2.0])  # one value per utterance
    lib = _lib.load()
    _ragged(data, "fp32", "euler", CFGS, use_graph=False)  # (the plan of these shapes exists)
    plan = cfm.transformer.plan(3, 448, 2)
    total = sum(DURS)
    buf = torch.randn(total, 100, device="cuda")
    out = torch.full((total, 100), 7.0, device="cuda")
    ids = torch.zeros(3, 4, dtype=torch.int32, device="cuda")
    lens = torch.full((3,), NC, dtype=torch.int32, device="cuda")
    fr, tg = torch.tensor(DURS, dtype=torch.int32), torch.linspace(0, 1, 3)

    def call(vec):
        cv = torch.tensor(vec, dtype=torch.float32)
        return lib.f5_sample_ragged_ex(plan, 3, C.c_void_p(fr.data_ptr()), _lib.ptr(buf), _lib.ptr(ids), 4, _lib.ptr(lens), None, _lib.ptr(buf),
                                       C.c_void_p(tg.data_ptr()), 2, 2.0, C.c_void_p(cv.data_ptr()), 0, _lib.ptr(out), _lib.stream_ptr())

    for vec in ([2.0, 0.0, 2.0], [0.0, 0.0, 1e-5], [2.0, float("nan"), 2.0]):
        assert call(vec) == -1, vec  # F5_EINVAL
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), vec
    assert b"1e-5" in lib.f5_last_error() or b"NaN" in lib.f5_last_error()
    assert call([2.0, 1.0, 0.5]) == 0 and bool((out != 7.0).any())


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_an_all_zero_vector_is_the_scalar_zero_call(data, prec):
    """(e)  the single-pass branch (cfm.py:167): no combine runs, the vector has nothing to say"""
    got = _ragged(data, prec, "euler", [0.0, 0.0, 0.0], use_graph=False)
    _assert_equal(got, _ragged(data, prec, "euler", 0.0, use_graph=False), prec)
    assert not torch.equal(got[0], _ragged(data, prec, "euler", 2.0, use_graph=False)[0])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_edit_masks_equal_the_masked_batch1_calls(data, prec):
    """(f)  an interior span of utterance 0's prompt is edited, the others keep theirs; (g) the same with a guidance vector"""
    span = (20, 55)
    got = _ragged(data, prec, "euler", 2.0, use_graph=False, edit_masks=[_edit(*span), None, None])
    _assert_equal(got, [_single(data, prec, "euler", 0, 2.0, span), _single(data, prec, "euler", 1, 2.0), _single(data, prec, "euler", 2, 2.0)], prec)
    assert not torch.equal(got[0], _single(data, prec, "euler", 0, 2.0))  # the mask is not ignored
    span2 = (60, NC)
    got = _ragged(data, prec, "midpoint", CFGS, use_graph=False, edit_masks=[_edit(*span), None, _edit(*span2)])
    _assert_equal(got, [_single(data, prec, "midpoint", 0, CFGS[0], span), _single(data, prec, "midpoint", 1, CFGS[1]),
                        _single(data, prec, "midpoint", 2, CFGS[2], span2)], prec)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_the_vector_path_matches_the_oracle(data, prec):
    """(h)  utterance 2 of (a) against cpu_ref.sample at its own guidance strength: the ragged path is not only self-consistent"""
    got = _ragged(data, prec, "euler", CFGS, use_graph=False)
    o, _ = cpu_ref.sample(data["W"], data["arch"], data["cond"].cpu(), data["texts"][2].cpu(), DURS[2], steps=STEPS["euler"], cfg_strength=CFGS[2],
                          sway_sampling_coef=-1.0, y0=data["y0s"][2].cpu(), method="euler", return_trajectory=False)
    err = rel_l2(got[2].cpu()[:, NC:], o[:, NC:])
    print(f"sample_ragged with a guidance vector vs oracle [{prec}]: rel-L2 {err:.2e} (bound {TOL[prec]:g})")
    assert err < TOL[prec]
