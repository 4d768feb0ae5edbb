"""eval.distill on the device: distillation_loss of a depth-6 teacher and its pruned student against the fp64 formulas of the reference's
distillation script (src/f5_tts/train/distil_reload.py:1070-1097) on the kernels' own inputs, both predictions against the CPU oracle, and the
block ablation scan: a block whose gates are zero adds exact zeros to the stream, so removing it must cost exactly nothing."""
import math
import random

import numpy as np
import pytest
import torch

from conftest import golden_arch, load_golden, rel_l2
from eraxvif5tts_amd import _lib
from eraxvif5tts_amd.eval import block_ablation, distillation_loss, prune_state_dict, subset_losses
from oracle import cpu_ref
from test_gpu_model import STAGE_TOL

pytestmark = pytest.mark.gpu
V, DEPTH, KEEP, DEAD = 60, 6, [0, 1, 4, 5], 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _arch():
    return {**golden_arch(load_golden("tiny_base")), "depth": DEPTH}


@pytest.fixture(scope="module")
def weights():
    return cpu_ref.random_dit_weights(_arch(), V, seed=607)


def _batches():
    g = torch.Generator().manual_seed(31)
    out = []
    for n, lens, nt in ((56, [56, 44], 18), (37, [30, 37, 21], 11)):
        mel = torch.randn(len(lens), n, 100, generator=g) * 2 - 3
        for b, l in enumerate(lens):
            mel[b, l:] = 0
        out.append((mel, torch.randint(0, V, (len(lens), nt), generator=g), torch.tensor(lens)))
    return out


def _pair(weights, prec):
    import gpu_helpers as G
    from eraxvif5tts_amd.model import CFM
    teacher = G.make_cfm(_arch(), V, weights, prec)
    student = CFM(transformer=teacher.transformer.pruned(KEEP).cuda(), num_channels=100, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()
    return teacher, student


class _Recorder:
    """wraps module.forward: keeps the keyword arguments and the result of every call"""

    def __init__(self, module):
        self.module, self.inner, self.calls = module, module.forward, []
        module.forward = self

    def __call__(self, **kw):
        out = self.inner(**kw)
        self.calls.append((kw, out))
        return out

    def close(self):
        del self.module.forward


def _ulps_apart(a, b):
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))


@pytest.mark.parametrize("kw", [dict(), dict(alpha=0.3, loss_type="l1"), dict(spec_l1_weight=0.25)], ids=["default", "alpha-l1", "spec_l1"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_distillation_loss_matches_the_script_formulas(weights, prec, kw):
    teacher, student = _pair(weights, prec)
    batches = _batches()
    rec_t, rec_s = _Recorder(teacher.transformer), _Recorder(student.transformer)
    try:
        r = distillation_loss(teacher, student, batches, seed=9, **kw)
    finally:
        rec_t.close(), rec_s.close()
    assert len(rec_t.calls) == len(batches) == len(rec_s.calls)
    alpha, w, col = kw.get("alpha", 0.5), kw.get("spec_l1_weight", 0.0), 3 if kw.get("loss_type") == "l1" else 2
    W_small = prune_state_dict(weights, KEEP)
    at = 0
    for i, (mel, text, lens) in enumerate(batches):
        (tk, t_pred), (sk, s_pred) = rec_t.calls[i], rec_s.calls[i]
        assert set(tk) == {"x", "cond", "text", "time", "drop_audio_cond", "drop_text"}  # no mask, no cache
        assert torch.equal(tk["x"], sk["x"]) and torch.equal(tk["cond"], sk["cond"]) and tk["drop_audio_cond"] is False and tk["drop_text"] is False
        phi, cond, time = tk["x"].cpu(), tk["cond"].cpu(), tk["time"].cpu()
        # the draws are the script's (device generator): seeded again, its statements give the kernel's inputs back
        torch.manual_seed(9 + i)
        random.seed(9 + i)
        Bn, n = mel.shape[0], mel.shape[1]
        frac = torch.zeros((Bn,), device="cuda").float().uniform_(0.7, 1.0)
        from eraxvif5tts_amd.model.utils import lens_to_mask, mask_from_frac_lengths
        span = (mask_from_frac_lengths(lens.cuda(), frac) & lens_to_mask(lens.cuda(), length=n))
        x1 = mel.cuda()
        x0 = torch.randn_like(x1)
        tt = torch.rand((Bn,), dtype=x1.dtype, device="cuda")
        t3 = tt.unsqueeze(-1).unsqueeze(-1)
        assert torch.equal(tk["time"], tt) and torch.equal(tk["x"], (1 - t3) * x0 + t3 * x1)
        assert torch.equal(tk["cond"], torch.where(span[..., None], torch.zeros_like(x1), x1))
        # both predictions against the oracle on the kernel's phi and cond
        for pred, Wm, depth in ((t_pred, weights, DEPTH), (s_pred, W_small, len(KEEP))):
            ref = cpu_ref.dit_forward(Wm, {**_arch(), "depth": depth}, phi, cond, text, time, False, False)
            assert rel_l2(pred.cpu(), ref) < STAGE_TOL[prec]
        # distil_reload.py:1070-1097 in fp64 on the returned predictions (the fp32 elementwise values, summed in fp64)
        s, t, flow, sp = s_pred, t_pred, x1 - x0, span.cpu()
        elems = [e.cpu() for e in ((s - flow) ** 2, (t - flow) ** 2, (s - t) ** 2, (s - t).abs())]
        want = torch.stack([torch.stack([e[b][sp[b]].double().sum() for e in elems]) for b in range(Bn)])
        got = r.sums[at:at + Bn]
        assert torch.equal(r.frames[at:at + Bn], sp.sum(dim=1))
        assert bool(((got - want).abs() <= 1e-12 * want).all()), (got, want)
        frames = max(int(sp.sum()), 1)
        student_loss, distill_loss, spec = [float(want[:, k].sum()) / frames for k in (0, col, 3)]
        logged = r.batch_losses[i]
        assert _ulps_apart(logged[0], student_loss) <= 1 and _ulps_apart(logged[1], distill_loss) <= 1
        total = (1.0 - alpha) * np.float32(student_loss) + alpha * np.float32(distill_loss) + np.float32(spec) * w
        assert abs(logged[2] - float(total)) <= 4 * 2.0 ** -23 * abs(float(total))  # three fp32 roundings of the script's sum, one ulp each input
        at += Bn
    n = int(r.frames.sum())
    tot = [math.fsum(r.sums[:, k].tolist()) for k in range(4)]
    assert r.student == tot[0] / n and r.distill == tot[col] / n and r.spec_l1 == tot[3] / n
    assert r.total == (1.0 - alpha) * r.student + alpha * r.distill + w * r.spec_l1
    assert r.student_flow == tot[0] / (n * 100) and r.teacher_flow == tot[1] / (n * 100) and r.distill > 0
    again = distillation_loss(teacher, student, batches, seed=9, **kw)
    assert np.array_equal(again.sums.numpy().view(np.int64), r.sums.numpy().view(np.int64)) and again.batch_losses == r.batch_losses
    assert again.total == r.total


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_model_against_itself_has_no_distillation_loss(weights, prec):
    teacher, _ = _pair(weights, prec)
    r = distillation_loss(teacher, teacher, _batches(), seed=2)
    assert r.distill == 0.0 and r.spec_l1 == 0.0 and r.student > 0 and r.student_flow == r.teacher_flow
    assert all(b[1] == 0.0 for b in r.batch_losses)


def _kill_block(weights, block):
    """gate_msa and gate_mlp of `block` identically zero (rows 2D..3D and 5D..6D of attn_norm.linear): both branches are multiplied by 0"""
    W = dict(weights)
    D = _arch()["dim"]
    w, b = W[f"transformer_blocks.{block}.attn_norm.linear.weight"].clone(), W[f"transformer_blocks.{block}.attn_norm.linear.bias"].clone()
    for lo in (2 * D, 5 * D):
        w[lo:lo + D] = 0
        b[lo:lo + D] = 0
    W[f"transformer_blocks.{block}.attn_norm.linear.weight"], W[f"transformer_blocks.{block}.attn_norm.linear.bias"] = w, b
    return W


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_block_ablation_finds_the_block_that_does_nothing(weights, prec):
    import gpu_helpers as G
    cfm = G.make_cfm(_arch(), V, _kill_block(weights, DEAD), prec)
    batches = _batches()
    cfm.transformer.set_active_blocks([0, 1, 2, 3, 4])  # a subset in force before the scan: the teacher is still the full model, and it comes back
    rec = _Recorder(cfm.transformer)
    try:
        scan = block_ablation(cfm, batches, seed=4)
    finally:
        rec.close()
    assert cfm.transformer.active_blocks == (0, 1, 2, 3, 4)
    assert len(rec.calls) == len(batches) * (1 + DEPTH)  # the teacher ran once per batch, not once per candidate
    assert [b for b, _ in scan] == list(range(DEPTH))
    for b, r in scan:
        print(f"  {prec} block {b}: distill {r.distill:.6e} student {r.student:.6e}")
        if b == DEAD:
            assert r.distill == 0.0 and r.spec_l1 == 0.0 and r.student_flow == r.teacher_flow
        else:
            assert r.distill > 0
    from eraxvif5tts_amd.eval import select_blocks
    assert DEAD not in select_blocks([(b, r.distill) for b, r in scan], 5, range(DEPTH))
    some = block_ablation(cfm, batches[:1], blocks=[DEAD, 5], seed=4, loss_type="l1")
    assert [b for b, _ in some] == [DEAD, 5] and some[0][1].distill == 0.0 and some[1][1].distill > 0

    def broken():
        yield batches[0]
        raise RuntimeError("the loader failed")
    with pytest.raises(RuntimeError, match="the loader failed"):
        block_ablation(cfm, broken(), seed=4)
    assert cfm.transformer.active_blocks == (0, 1, 2, 3, 4)  # restored on error too


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_the_subset_route_equals_a_separately_built_pruned_student(weights, prec):
    teacher, student = _pair(weights, prec)
    batches = _batches()
    a, full = subset_losses(teacher, batches, [KEEP, None], seed=6)
    b = distillation_loss(teacher, student, batches, seed=6)
    assert np.array_equal(a.sums.numpy().view(np.int64), b.sums.numpy().view(np.int64)) and torch.equal(a.frames, b.frames)
    assert a.batch_losses == b.batch_losses and a.total == b.total
    assert full.distill == 0.0 and teacher.transformer.active_blocks is None
    with pytest.raises(ValueError):
        subset_losses(teacher, batches, [[2, 1]])
