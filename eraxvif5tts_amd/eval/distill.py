"""Pruning workbench: the losses of the reference's teacher-to-student distillation step, forward only, and the block ablation scan built on them.

``distillation_loss`` evaluates a (teacher, student) pair of ``CFM`` s over a list of batches and returns the numbers the reference's
distillation script logs per update (src/f5_tts/train/distil_reload.py:1044-1097: ``loss/student``, ``loss/distill``, ``loss/total``), from one
kernel pass per batch (``f5_distill_loss``, csrc/distill_loss.hip).  ``block_ablation`` removes each block of a DiT in turn -- through
``DiT.set_active_blocks`` on the SAME module, on the weights already in HBM -- and measures the loss against the full model, whose prediction of a
batch is computed once for all candidates; ``subset_losses`` does the same for arbitrary candidate subsets.  ``eval.prune.select_blocks`` turns the
scores into the list of blocks to keep.  Nothing here can be differentiated: no gradient, optimiser or training loop exists in this package.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from ..model.utils import lens_to_mask, list_str_to_idx, list_str_to_tensor, mask_from_frac_lengths

TERMS = ("student_flow", "teacher_flow", "mse", "l1")  # columns of DistillLoss.sums (include/f5hip.h: f5_distill_loss)
_KEEP = object()  # "leave the module's block subset as it is"


@dataclass
class DistillLoss:
    student: float       # sum (student - flow)^2 / frames: the script's student_loss (:1070-1072) -- mel times a mean, it divides by FRAMES
    distill: float       # sum (student - teacher)^2 or |student - teacher| / frames, by loss_type (:1074-1093)
    spec_l1: float       # sum |student - teacher| / frames (:1083-1087), whatever its weight
    total: float         # (1 - alpha) * student + alpha * distill + spec_l1_weight * spec_l1 (:1097)
    student_flow: float  # sum (student - flow)^2 / (frames x mel): what validation_loss reports for the student on the same draws (NaN: no frame)
    teacher_flow: float  # the same for the teacher
    batch_losses: List[Tuple[float, float, float]]  # per batch the fp32 (student, distill, total) the script would log
    sums: torch.Tensor   # f64 [utterances, 4] on the host: the four sums (TERMS) over the utterance's selected elements
    frames: torch.Tensor  # i64 [utterances] on the host: selected frames
    utterance_losses: List[Tuple[float, float]]  # per utterance (student, distill): its own sums / max(frames, 1)


def _native_distill(student, teacher, x1, x0, span8):
    """f5_distill_loss: (sums f64 [b, 4], frames i64 [b], batch f32 [4]) on the device."""
    from .. import _lib
    lib = _lib.load()
    b, n, mel = x1.shape
    nbytes = lib.f5_distill_loss_workspace(b, n, mel)
    if nbytes < 0:
        _lib.check(int(nbytes), "distill_loss_workspace")
    work = torch.empty(nbytes, device=x1.device, dtype=torch.uint8)
    sums = torch.empty(b, 4, device=x1.device, dtype=torch.float64)
    frames = torch.empty(b, device=x1.device, dtype=torch.int64)
    batch = torch.empty(4, device=x1.device, dtype=torch.float32)
    _lib.check(lib.f5_distill_loss(b, n, mel, _lib.ptr(student), _lib.ptr(teacher), _lib.ptr(x1), _lib.ptr(x0), _lib.ptr(span8), _lib.ptr(sums),
                                   _lib.ptr(frames), _lib.ptr(batch), _lib.ptr(work), _lib.stream_ptr()), "distill_loss")
    return sums, frames, batch


def _host_distill(student, teacher, x1, x0, span):
    """The script's torch expressions (:1070-1093) on CPU tensors (an oracle backbone), in the layout of _native_distill."""
    flow = x1 - x0
    elems = (F.mse_loss(student, flow, reduction="none"), F.mse_loss(teacher, flow, reduction="none"),
             F.mse_loss(student, teacher, reduction="none"), F.l1_loss(student, teacher, reduction="none"))
    sel = span[..., None]
    sums = torch.stack([torch.where(sel, e.double(), torch.zeros((), dtype=torch.float64)).sum(dim=(1, 2)) for e in elems], dim=1)
    frames = span.sum(dim=1).to(torch.int64)
    denom = span.sum().clamp(min=1)
    batch = torch.stack([(e * sel).sum() / denom for e in elems]).float()
    return sums, frames, batch


class _Batch:
    """The draws and the noised inputs of one batch (distil_reload.py:1044-1051), in the script's order and on its devices."""

    def __init__(self, cfm, mel, texts, lens):
        device = cfm.device
        x1 = mel.to(device)
        lens = torch.as_tensor(lens, dtype=torch.long).to(device)
        if isinstance(texts, list):
            texts = (list_str_to_idx(texts, cfm.vocab_char_map) if cfm.vocab_char_map is not None else list_str_to_tensor(texts)).to(device)
        batch, seq_len, dtype = x1.shape[0], x1.shape[1], x1.dtype
        mask = lens_to_mask(lens, length=seq_len)
        frac_lengths = torch.zeros((batch,), device=device).float().uniform_(0.7, 1.0)  # (the script's constants, not frac_lengths_mask)
        span = mask_from_frac_lengths(lens, frac_lengths).to(device) & mask
        x0 = torch.randn_like(x1)
        time = torch.rand((batch,), dtype=dtype, device=device)
        self.native = x1.is_cuda
        if self.native:
            if dtype != torch.float32:
                raise TypeError(f"distillation_loss on the device takes fp32 mels, not {dtype}")
            from ..model.cfm import _native_noise
            x1, x0 = x1.contiguous(), x0.contiguous()
            self.span8 = span.to(torch.uint8).contiguous()
            phi, cond = _native_noise(x1, x0, time.contiguous(), self.span8)
        else:
            t = time.unsqueeze(-1).unsqueeze(-1)
            phi = (1 - t) * x0 + t * x1
            cond = torch.where(span[..., None], torch.zeros_like(x1), x1)
        self.x1, self.x0, self.time, self.span, self.text, self.phi, self.cond = x1, x0, time, span, texts, phi, cond

    def predict(self, cfm, drop_audio_cond, drop_text):
        pred = cfm.transformer(x=self.phi, cond=self.cond, text=self.text, time=self.time, drop_audio_cond=drop_audio_cond, drop_text=drop_text)
        return pred.to(device=self.x1.device, dtype=torch.float32).contiguous() if self.native else pred

    def losses(self, student, teacher):
        """one f64 row [4 b + b + 4]: sums, frames, the batch's fp32 values (counts and fp32 values are exact in fp64: one copy at the end)"""
        sums, frames, batch = (_native_distill(student, teacher, self.x1, self.x0, self.span8) if self.native
                               else _host_distill(student, teacher, self.x1, self.x0, self.span))
        return torch.cat([sums.reshape(-1), frames.double(), batch.double()])


def _check_options(alpha, loss_type, spec_l1_weight):
    if loss_type not in ("mse", "l1"):
        raise ValueError(f"Unsupported distill_loss_type: {loss_type}")  # distil_reload.py:1079
    return float(alpha), float(spec_l1_weight)


def _check_pair(teacher, student):
    if teacher.num_channels != student.num_channels:
        raise ValueError(f"teacher and student differ in mel width: {teacher.num_channels} vs {student.num_channels}")
    vocab = [getattr(c.transformer, "text_num_embeds", None) for c in (teacher, student)]
    if vocab[0] != vocab[1] or teacher.vocab_char_map != student.vocab_char_map:
        raise ValueError(f"teacher and student differ in vocabulary ({vocab[0]} vs {vocab[1]} embeddings): the same ids would name other tokens")


def _assemble(host, sizes, mel_dim, alpha, loss_type, spec_l1_weight) -> DistillLoss:
    """`host`: the f64 rows of _Batch.losses of every batch, one after the other, on the host"""
    sums, frames, logged, at = [], [], [], 0
    col = 2 if loss_type == "mse" else 3
    for b in sizes:
        sums.append(host[at:at + 4 * b].reshape(b, 4))
        frames.append(host[at + 4 * b:at + 5 * b].to(torch.int64))
        v = host[at + 5 * b:at + 5 * b + 4].float()  # the script's fp32 scalars; its total (:1097) in fp32 tensor arithmetic
        total = (1.0 - alpha) * v[0] + alpha * v[col] + (v[3] * spec_l1_weight if spec_l1_weight > 0.0 else 0.0)
        logged.append((float(v[0]), float(v[col]), float(total)))
        at += 5 * b + 4
    sums, frames = torch.cat(sums), torch.cat(frames)
    n = int(frames.sum())
    tot = [math.fsum(sums[:, k].tolist()) for k in range(4)]  # (the correctly rounded fp64 sums: no order to speak of)
    student, distill, spec = tot[0] / max(n, 1), tot[col] / max(n, 1), tot[3] / max(n, 1)
    return DistillLoss(student=student, distill=distill, spec_l1=spec,
                       total=(1.0 - alpha) * student + alpha * distill + spec_l1_weight * spec,
                       student_flow=tot[0] / (n * mel_dim) if n else float("nan"), teacher_flow=tot[1] / (n * mel_dim) if n else float("nan"),
                       batch_losses=logged, sums=sums, frames=frames,
                       utterance_losses=[(float(s[0]) / max(int(f), 1), float(s[col]) / max(int(f), 1)) for s, f in zip(sums, frames)])


def _set_blocks(cfm, blocks):
    if blocks is not _KEEP:
        cfm.transformer.set_active_blocks(blocks)


@torch.no_grad()
def _evaluate(teacher, teacher_blocks, students, batches, seed, alpha, loss_type, spec_l1_weight, drop_audio_cond, drop_text):
    """One DistillLoss per (cfm, blocks) of `students`.  Per batch: the draws, ONE teacher forward, one forward per student, one loss pass each;
    the results stay on the device until the end."""
    alpha, spec_l1_weight = _check_options(alpha, loss_type, spec_l1_weight)
    for s, _ in students:
        _check_pair(teacher, s)
    rows = [[] for _ in students]
    sizes, mel_dim = [], None
    # Both models run with fp32 residual-stream storage (DiT.set_residual_f16; arithmetic and branch dtypes as in production): the fp16 stream
    # of the 16-bit modes is rounded once per block, so a block that adds exact zeros still moves the bits of what follows it -- noise of the
    # size of a weak block's score (1.7e-4 against 0.5 for a live block of the depth-6 test model).  With fp32 storage it scores exactly 0.
    backbones = {id(c.transformer): c.transformer for c in [teacher] + [s for s, _ in students] if hasattr(c.transformer, "set_residual_f16")}
    storage = {k: m.residual_f16 for k, m in backbones.items()}
    try:
        for m in backbones.values():
            m.set_residual_f16(False)
        for i, (mel, texts, lens) in enumerate(batches):
            torch.manual_seed(seed + i)
            random.seed(seed + i)
            b = _Batch(teacher, mel, texts, lens)
            _set_blocks(teacher, teacher_blocks)
            t_pred = b.predict(teacher, False, False)  # distil_reload.py:1056: the teacher always fully conditioned
            for k, (s, blocks) in enumerate(students):
                _set_blocks(s, blocks)
                rows[k].append(b.losses(b.predict(s, drop_audio_cond, drop_text), t_pred))
            sizes.append(b.x1.shape[0])
            mel_dim = b.x1.shape[-1]
    finally:
        for k, m in backbones.items():
            m.set_residual_f16(storage[k])
    if not sizes:
        raise ValueError("distillation_loss: no batches")
    host = torch.stack([torch.cat(r) for r in rows]).cpu()  # the call's one synchronisation
    return [_assemble(host[k], sizes, mel_dim, alpha, loss_type, spec_l1_weight) for k in range(len(students))]


def distillation_loss(teacher, student, batches: Iterable, *, alpha=0.5, loss_type="mse", spec_l1_weight=0.0, seed=0, drop_audio_cond=False,
                      drop_text=False) -> DistillLoss:
    """The distillation losses of the reference's recipe (distil_reload.py:1044-1097) for a (teacher, student) pair of ``CFM`` s, forward only.

    ``batches`` yields ``(mel [B, N, mel] zero-padded, texts, lens)`` with N = max(lens), as ``validation_loss`` takes them.  Before batch ``i``
    torch and Python's ``random`` are seeded with ``seed + i``; the draws are the script's, in its order and on the model's device: the span
    fractions ``uniform_(0.7, 1.0)`` (its constants), the ``rand`` inside ``mask_from_frac_lengths``, ``randn_like(x1)``, ``rand((B,))``.  phi and cond
    come from ``f5_cfm_noise``; each model's backbone is called once, with no mask and no cache -- the teacher fully conditioned (:1056), the
    student with the two FIXED flags given here (the script draws them; ``validation_loss`` fixes them too) -- and ``f5_distill_loss`` forms the
    four sums in one pass.  Everything stays on the device until the end: one synchronisation per call; the same arguments give the same bits.
    CPU tensors (oracle backbones) take the script's torch expressions.  For the duration of the call HIP backbones keep their residual stream
    in fp32 (``DiT.set_residual_f16(False)``, put back on exit; captured sample() graphs of their plans are dropped): a block that adds exact
    zeros then costs exactly nothing, where the fp16 stream's one rounding per block would show as noise.  In the 16-bit modes
    ``student_flow`` / ``teacher_flow`` therefore differ from ``validation_loss`` in the last bits.

    ``loss_type``: "mse" or "l1" (anything else: the script's ValueError).  A vocabulary or mel-width mismatch between the models is refused."""
    return _evaluate(teacher, _KEEP, [(student, _KEEP)], batches, seed, alpha, loss_type, spec_l1_weight, drop_audio_cond, drop_text)[0]


def subset_losses(cfm, batches: Iterable, subsets: Sequence[Optional[Sequence[int]]], *, alpha=0.5, loss_type="mse", spec_l1_weight=0.0, seed=0,
                  drop_audio_cond=False, drop_text=False) -> List[DistillLoss]:
    """``distillation_loss`` of ``cfm`` run with each block subset of ``subsets`` (``DiT.set_active_blocks`` on the same module; None = all blocks)
    against ``cfm`` run with all blocks.  The teacher's prediction of a batch is computed once and kept on the device for every candidate:
    1 + len(subsets) forwards per batch.  The subset in force before the call is restored on exit, also on error."""
    from .prune import check_blocks
    dit = cfm.transformer
    if not hasattr(dit, "set_active_blocks"):
        raise NotImplementedError("the backbone has no block subsets (DiT.set_active_blocks)")
    cands = [None if s is None else tuple(check_blocks(s, dit.depth)) for s in subsets]
    before = dit.active_blocks
    try:
        return _evaluate(cfm, None, [(cfm, s) for s in cands], batches, seed, alpha, loss_type, spec_l1_weight, drop_audio_cond, drop_text)
    finally:
        dit.set_active_blocks(before)


def block_ablation(cfm, batches: Iterable, *, blocks=None, seed=0, **loss_kw) -> List[Tuple[int, DistillLoss]]:
    """For each block of the DiT (or each of ``blocks``): the model WITHOUT that block as the student, the full model as the teacher --
    ``(block, DistillLoss)`` in block order, 1 + len(blocks) forwards per batch.  ``[(b, r.distill) for b, r in ...]`` serves ``select_blocks``
    directly: a block whose removal hurts most scores highest."""
    depth = cfm.transformer.depth
    blocks = list(range(depth)) if blocks is None else [int(b) for b in blocks]
    for b in blocks:
        if not 0 <= b < depth:
            raise ValueError(f"block {b} is outside [0, {depth})")
    if depth < 2:
        raise ValueError("block_ablation needs a model of at least two blocks")
    subsets = [[k for k in range(depth) if k != b] for b in blocks]
    return list(zip(blocks, subset_losses(cfm, batches, subsets, seed=seed, **loss_kw)))
