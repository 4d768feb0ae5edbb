"""CPU tests of the pruning workbench's host side: eval.prune.select_blocks against hand-worked cases of the reference pruner's rule
(src/model_pruning/excellent_definitive-f5tts-pruner.py:662-700), the key renumbering of prune_state_dict / prune_checkpoint (:731-784) with a
round trip through infer.utils_infer.load_checkpoint, and eval.distill.distillation_loss over oracle backbones against the lines of the
reference's distillation script (src/f5_tts/train/distil_reload.py:1044-1097) restated here, the order of its random draws included."""
import math
import random

import pytest
import torch
import torch.nn.functional as F

from conftest import golden_arch, load_golden

MOD22 = [(b, float(b * 7 % 22)) for b in range(22)]  # 22 distinct scores: 0:0 1:7 2:14 3:21 4:6 5:13 6:20 7:5 8:12 9:19 10:4 11:11 12:18 13:3 14:10
#                                                      15:17 16:2 17:9 18:16 19:1 20:8 21:15


def test_select_blocks_keeps_first_two_last_two_and_the_best_of_the_middle():
    """Base, 22 blocks.  Blocks 0, 1, 20, 21 are kept whatever they score; the middle by descending score reads 3 6 9 12 15 18 2 5 8 11 14 17 4 7
    10 13 16 19: ten of them for a target of 14, eight for 12."""
    from eraxvif5tts_amd.eval import select_blocks
    assert select_blocks(MOD22, 14, range(22)) == [0, 1, 2, 3, 5, 6, 8, 9, 11, 12, 15, 18, 20, 21]
    assert select_blocks(MOD22, 12, range(22)) == [0, 1, 2, 3, 5, 6, 9, 12, 15, 18, 20, 21]
    assert select_blocks(list(reversed(MOD22)), 14, range(22)) == [0, 1, 2, 3, 5, 6, 8, 9, 11, 12, 15, 18, 20, 21]  # the order of distinct scores is nothing
    # the ends score worst and stay; a middle block that scores best of all goes first
    scores = [(0, -5.0), (1, -4.0), (2, 9.0), (3, 0.5), (4, -3.0), (5, -9.0)]
    assert select_blocks(scores, 5, range(6)) == [0, 1, 2, 4, 5]
    # block indices that are not 0 .. n - 1 (a listing of an already pruned model): the rule speaks of positions in `blocks`
    assert select_blocks([(5, 1.0), (7, 2.0), (1, 0.0), (3, 0.0), (9, 0.0), (11, 0.0)], 5, [1, 3, 5, 7, 9, 11]) == [1, 3, 7, 9, 11]


def test_select_blocks_small_targets_and_limits():
    """target >= depth keeps all, target <= 0 none, target <= 4 the FIRST target blocks whatever the scores say.  (The rule's remaining case,
    "fewer than 4 blocks: the best by score", needs 4 < target < len(blocks) < 4 and can never run, here or in the reference.)"""
    from eraxvif5tts_amd.eval import select_blocks
    worst_first = [(b, float(b)) for b in range(6)]  # the first blocks score worst
    assert select_blocks(worst_first, 6, range(6)) == [0, 1, 2, 3, 4, 5]
    assert select_blocks(worst_first, 9, range(6)) == [0, 1, 2, 3, 4, 5]
    assert select_blocks(worst_first, 0, range(6)) == [] and select_blocks(worst_first, -2, range(6)) == []
    for target in (1, 2, 3, 4):
        assert select_blocks(worst_first, target, range(6)) == list(range(target))
    assert select_blocks(MOD22, 4, range(22)) == [0, 1, 2, 3]
    assert select_blocks(MOD22, 22, range(22)) == list(range(22))


def test_select_blocks_ties_keep_list_order():
    """Equal scores: the ranking is a stable sort, so the middle blocks are taken in the order the score list names them."""
    from eraxvif5tts_amd.eval import select_blocks
    order = [5, 0, 3, 2, 4, 1, 6, 7]
    assert select_blocks([(b, 1.0) for b in order], 6, range(8)) == [0, 1, 3, 5, 6, 7]        # middle in list order: 5 3 2 4
    assert select_blocks([(b, 1.0) for b in reversed(order)], 6, range(8)) == [0, 1, 2, 4, 6, 7]  # 4 2 3 5
    assert select_blocks([(2, 1.0), (3, 2.0), (4, 1.0), (5, 2.0)], 7, range(8)) == [0, 1, 2, 3, 5, 6, 7]  # 3 5 2 4: the tie between 2 and 4


# ----------------------------------------------------------------------------- prune_state_dict / prune_checkpoint
TINY = dict(dim=128, depth=4, heads=2, ff_mult=2, text_dim=64, conv_layers=2, pe_attn_head=1, text_mask_padding=False)
KEEP = [0, 2, 3]


def _cfm(depth, seed=0):
    from eraxvif5tts_amd.model import CFM, DiT
    torch.manual_seed(seed)
    dit = DiT(**{**TINY, "depth": depth}, text_num_embeds=60, mel_dim=100, precision="fp32")
    for p in dit.parameters():  # the zero-initialised tensors too: every kept tensor must be told from every other
        p.data.normal_()
    return CFM(transformer=dit, mel_spec_kwargs={"mel_spec_type": "vocos"})


def _block_keys(sd, prefix=""):
    return sorted({int(k[len(prefix):].split(".")[1]) for k in sd if k.startswith(prefix + "transformer_blocks.")})


@pytest.mark.parametrize("prefix", ["", "transformer.", "ema_model.transformer."])
def test_prune_state_dict_renumbers_kept_blocks_and_shares_storage(prefix):
    from eraxvif5tts_amd.eval import prune_state_dict
    from eraxvif5tts_amd.model import DiT
    big = _cfm(4).transformer.state_dict()
    sd = {prefix + k: v for k, v in big.items()}
    if prefix.startswith("ema_model."):
        sd.update({"initted": torch.tensor(True), "step": torch.tensor(7)})
    out = prune_state_dict(sd, KEEP)
    assert _block_keys(out, prefix) == [0, 1, 2]
    small = DiT(**{**TINY, "depth": 3}, text_num_embeds=60, mel_dim=100, precision="fp32").state_dict()
    extra = {"initted", "step"} if prefix.startswith("ema_model.") else set()
    assert set(out) == {prefix + k for k in small} | extra
    for k, v in out.items():
        if k in extra:
            assert v is sd[k]
            continue
        name = k[len(prefix):]
        if name.startswith("transformer_blocks."):
            parts = name.split(".")
            parts[1] = str(KEEP[int(parts[1])])
            name = ".".join(parts)
        assert v is sd[prefix + name], k  # the same tensor object: nothing is copied
    for k in sd:  # text blocks and everything outside the blocks pass through under their own names
        if "transformer_blocks." not in k:
            assert out[k] is sd[k]
    assert any("text_embed.text_blocks.1." in k for k in out)


def test_prune_state_dict_refuses_bad_lists():
    from eraxvif5tts_amd.eval import prune_state_dict
    for bad in ([], [2, 1], [0, 0], [-1, 2]):
        with pytest.raises(ValueError):
            prune_state_dict({}, bad)


@pytest.mark.parametrize("kind", ["pt", "safetensors"])
def test_prune_checkpoint_round_trip(tmp_path, kind):
    """An EMA .pt checkpoint (ema_model.* keys with initted / step beside them, as the reference's trainer writes) and a flat .safetensors: the
    pruned file loads through utils_infer.load_checkpoint into a CFM of the smaller depth whose parameters are the kept blocks'."""
    from eraxvif5tts_amd.eval import prune_checkpoint
    from eraxvif5tts_amd.infer.utils_infer import load_checkpoint
    big = _cfm(4, seed=1)
    ema = {"ema_model." + k: v.clone() for k, v in big.state_dict().items()}
    ema.update({"initted": torch.tensor(True), "step": torch.tensor(1200)})
    src, dst = str(tmp_path / f"model.{kind}"), str(tmp_path / f"pruned.{kind}")
    if kind == "pt":
        torch.save({"ema_model_state_dict": ema, "model_state_dict": {k: v.clone() for k, v in big.state_dict().items()}, "step": 1200}, src)
    else:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in ema.items() if k not in ("initted", "step")}, src)
    pruned = prune_checkpoint(src, dst, KEEP)
    assert pruned == (["ema_model_state_dict", "model_state_dict"] if kind == "pt" else ["<flat>"])
    if kind == "pt":
        back = torch.load(dst, map_location="cpu", weights_only=True)
        assert back["step"] == 1200 and int(back["ema_model_state_dict"]["step"]) == 1200 and bool(back["ema_model_state_dict"]["initted"])
        assert _block_keys(back["model_state_dict"], "transformer.") == [0, 1, 2]
    small = load_checkpoint(_cfm(3, seed=2), dst, "cpu")
    want, got = big.transformer.state_dict(), small.transformer.state_dict()
    checked = 0
    for k, v in got.items():
        name = k
        if k.startswith("transformer_blocks."):
            parts = k.split(".")
            parts[1] = str(KEEP[int(parts[1])])
            name = ".".join(parts)
        assert torch.equal(v, want[name]), k
        checked += 1
    assert checked == len(got) and _block_keys(got) == [0, 1, 2]
    with pytest.raises(ValueError):
        prune_checkpoint(src, str(tmp_path / ("x.safetensors" if kind == "pt" else "x.pt")), KEEP)


def test_dit_pruned_copies_the_kept_blocks():
    dit = _cfm(4, seed=3).transformer
    small = dit.pruned(KEEP)
    assert small.depth == 3 and small.ff_inner == dit.ff_inner and small.precision == dit.precision and type(small) is type(dit)
    big_sd = dit.state_dict()
    for k, v in small.state_dict().items():
        parts = k.split(".")
        if parts[0] == "transformer_blocks":
            parts[1] = str(KEEP[int(parts[1])])
        src = big_sd[".".join(parts)]
        assert torch.equal(v, src) and v.data_ptr() != src.data_ptr(), k  # equal values, storage of its own
    with pytest.raises(ValueError):
        dit.pruned([3, 1])
    with pytest.raises(ValueError):
        dit.set_active_blocks([4])
    assert dit.active_blocks is None
    dit.set_active_blocks(KEEP)  # (no plan exists on the host: the setting waits for the first one)
    assert dit.active_blocks == tuple(KEEP)
    dit.load_state_dict(dit.state_dict())
    dit.refresh_native()
    assert dit.active_blocks == tuple(KEEP)
    dit.set_active_blocks(None)
    assert dit.active_blocks is None


def test_unett_and_mmdit_refuse_block_subsets():
    from eraxvif5tts_amd.model import MMDiT, UNetT
    for m in (UNetT(dim=128, depth=4, heads=2, ff_mult=2, text_num_embeds=60, mel_dim=100), MMDiT(dim=128, depth=4, heads=2, ff_mult=2, text_num_embeds=60, mel_dim=100)):
        with pytest.raises(NotImplementedError, match="f5_plan_set_blocks"):
            m.set_active_blocks([0, 1])
        with pytest.raises(NotImplementedError, match="f5_plan_set_blocks"):
            m.pruned([0, 1])
        m.set_active_blocks(None)


# ----------------------------------------------------------------------------- distillation_loss on CPU tensors
class _Backbone(torch.nn.Module):
    """plug point A over the CPU oracle; keeps the keyword arguments and the result of every call."""

    def __init__(self, W, cfg):
        super().__init__()
        from oracle import cpu_ref
        self.W, self.cfg, self.ref, self.dim = W, cfg, cpu_ref, cfg["dim"]
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls, self.outs = [], []

    def forward(self, **kw):
        assert set(kw) == {"x", "cond", "text", "time", "drop_audio_cond", "drop_text"}, sorted(kw)  # distil_reload.py:1056,1065: no mask, no cache
        self.calls.append(kw)
        self.outs.append(self.ref.dit_forward(self.W, self.cfg, kw["x"], kw["cond"], kw["text"], kw["time"], kw["drop_audio_cond"], kw["drop_text"]))
        return self.outs[-1]


@pytest.fixture(scope="module")
def pair():
    from eraxvif5tts_amd.eval import prune_state_dict
    from eraxvif5tts_amd.model import CFM
    from oracle import cpu_ref
    arch = {**golden_arch(load_golden("tiny_base")), "depth": 4}
    W = cpu_ref.random_dit_weights(arch, 60, seed=11)
    teacher = CFM(transformer=_Backbone(W, arch), mel_spec_kwargs={"mel_spec_type": "vocos"})
    student = CFM(transformer=_Backbone(prune_state_dict(W, KEEP), {**arch, "depth": 3}), mel_spec_kwargs={"mel_spec_type": "vocos"})
    return teacher, student


def _batches():
    z = load_golden("cfm_forward")
    mel, text, lens = torch.from_numpy(z["mel"]), torch.from_numpy(z["text"]), torch.from_numpy(z["lens"])
    return [(mel, text, lens), (mel[:2, :22], text[:2], torch.tensor([22, 15]))]


def _script_lines(mel_input, mel_lengths, seed):
    """distil_reload.py:1044-1051 after the seeding of distillation_loss, on the CPU"""
    from eraxvif5tts_amd.model.utils import lens_to_mask, mask_from_frac_lengths  # (both tested against the reference's in test_cfm_forward_host.py)
    torch.manual_seed(seed)
    random.seed(seed)
    batch_size, seq_len, _ = mel_input.shape
    mask = lens_to_mask(mel_lengths, length=seq_len)
    frac_lengths = torch.zeros((batch_size,)).float().uniform_(0.7, 1.0)
    rand_span_mask = mask_from_frac_lengths(mel_lengths, frac_lengths)
    rand_span_mask &= mask
    x1 = mel_input
    x0 = torch.randn_like(x1)
    time = torch.rand((batch_size,), dtype=x1.dtype)
    t = time.unsqueeze(-1).unsqueeze(-1)
    xt = (1 - t) * x0 + t * x1
    return rand_span_mask, x0, time, xt, x1 - x0, torch.where(rand_span_mask[..., None], torch.zeros_like(x1), x1)


@pytest.mark.parametrize("kw", [dict(), dict(alpha=0.3), dict(loss_type="l1"), dict(spec_l1_weight=0.25, alpha=0.8), dict(drop_audio_cond=True, drop_text=True)],
                         ids=["default", "alpha", "l1", "spec_l1", "dropped"])
def test_distillation_loss_restates_the_script(pair, kw):
    from eraxvif5tts_amd.eval import distillation_loss
    teacher, student = pair
    batches = _batches()
    n0 = len(teacher.transformer.calls)
    r = distillation_loss(teacher, student, batches, seed=5, **kw)
    assert len(teacher.transformer.calls) == n0 + len(batches) and len(student.transformer.calls) == n0 + len(batches)  # one forward each per batch
    alpha, w, l1 = kw.get("alpha", 0.5), kw.get("spec_l1_weight", 0.0), kw.get("loss_type", "mse") == "l1"
    sums, frames = [], []
    for i, (mel, text, lens) in enumerate(batches):
        span, x0, time, xt, target_flow, cond = _script_lines(mel, lens, 5 + i)
        tk, sk = teacher.transformer.calls[n0 + i], student.transformer.calls[n0 + i]
        for got in (tk, sk):  # the draw order: span, x0 and time are the script's
            assert torch.equal(got["x"], xt) and torch.equal(got["cond"], cond) and torch.equal(got["time"], time) and torch.equal(got["text"], text)
        assert (tk["drop_audio_cond"], tk["drop_text"]) == (False, False)
        assert (sk["drop_audio_cond"], sk["drop_text"]) == (kw.get("drop_audio_cond", False), kw.get("drop_text", False))
        s_pred, t_pred = student.transformer.outs[n0 + i], teacher.transformer.outs[n0 + i]
        # :1070-1097
        student_loss = (F.mse_loss(s_pred, target_flow, reduction="none") * span.unsqueeze(-1)).sum() / span.sum().clamp(min=1)
        full = F.l1_loss(s_pred, t_pred, reduction="none") if l1 else F.mse_loss(s_pred, t_pred, reduction="none")
        distill_loss = (full * span.unsqueeze(-1)).sum() / span.sum().clamp(min=1)
        spec_l1 = (F.l1_loss(s_pred, t_pred, reduction="none") * span.unsqueeze(-1)).sum() / span.sum().clamp(min=1)
        total = (1.0 - alpha) * student_loss + alpha * distill_loss + spec_l1 * w
        got = r.batch_losses[i]
        assert got[0] == float(student_loss) and got[1] == float(distill_loss)
        assert abs(got[2] - float(total)) <= 2.0 ** -22 * abs(float(total))
        sel = span[..., None]
        elems = (F.mse_loss(s_pred, target_flow, reduction="none"), F.mse_loss(t_pred, target_flow, reduction="none"),
                 F.mse_loss(s_pred, t_pred, reduction="none"), F.l1_loss(s_pred, t_pred, reduction="none"))
        sums.append(torch.stack([torch.where(sel, e.double(), torch.zeros((), dtype=torch.float64)).sum(dim=(1, 2)) for e in elems], dim=1))
        frames.append(span.sum(dim=1))
    sums, frames = torch.cat(sums), torch.cat(frames)
    assert torch.equal(r.frames, frames) and r.sums.shape == (5, 4)
    assert torch.allclose(r.sums, sums, rtol=1e-12, atol=0.0)
    n = int(frames.sum())
    col = 3 if l1 else 2
    tot = [math.fsum(r.sums[:, k].tolist()) for k in range(4)]
    assert r.student == tot[0] / n and r.distill == tot[col] / n and r.spec_l1 == tot[3] / n
    assert r.total == (1.0 - alpha) * r.student + alpha * r.distill + w * r.spec_l1
    assert r.student_flow == tot[0] / (n * 100) and r.teacher_flow == tot[1] / (n * 100)
    assert r.distill > 0 and len(r.utterance_losses) == 5
    again = distillation_loss(teacher, student, batches, seed=5, **kw)
    assert torch.equal(again.sums, r.sums) and again.total == r.total and again.batch_losses == r.batch_losses


def test_distillation_loss_of_a_model_against_itself_and_refusals(pair):
    from eraxvif5tts_amd.eval import distillation_loss
    from eraxvif5tts_amd.model import CFM
    teacher, student = pair
    r = distillation_loss(teacher, teacher, _batches(), seed=1)
    assert r.distill == 0.0 and r.spec_l1 == 0.0 and r.student == r.sums[:, 1].sum().item() / int(r.frames.sum()) and r.student_flow == r.teacher_flow
    with pytest.raises(ValueError, match="Unsupported distill_loss_type: huber"):
        distillation_loss(teacher, student, _batches(), loss_type="huber")
    with pytest.raises(ValueError, match="no batches"):
        distillation_loss(teacher, student, [])
    narrow = CFM(transformer=student.transformer, mel_spec_kwargs={"mel_spec_type": "vocos", "n_mel_channels": 80})
    with pytest.raises(ValueError, match="mel width"):
        distillation_loss(teacher, narrow, _batches())
    other = CFM(transformer=student.transformer, mel_spec_kwargs={"mel_spec_type": "vocos"}, vocab_char_map={"a": 0})
    with pytest.raises(ValueError, match="vocabulary"):
        distillation_loss(teacher, other, _batches())
    # an empty span: the script's clamp(min=1) gives zeros, not NaN (the flow-matching means have no frame to speak of)
    empty = distillation_loss(teacher, student, [(torch.zeros(1, 1, 100), torch.zeros(1, 1, dtype=torch.long), torch.tensor([1]))], seed=0)
    assert int(empty.frames.sum()) == 0  # one frame times a fraction below 1, truncated
    assert empty.student == 0.0 and empty.distill == 0.0 and empty.batch_losses[0] == (0.0, 0.0, 0.0) and math.isnan(empty.student_flow)
