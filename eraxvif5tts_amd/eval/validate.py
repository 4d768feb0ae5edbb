"""Validation loss of a checkpoint: the flow-matching loss of ``CFM.forward`` (reference cfm.py:210-283) over a list of batches, forward only.

The number a checkpoint was trained on, for picking one after fine-tuning with the reference or judging a pruned model.  Nothing here can be
differentiated; there is no gradient, optimiser or trainer in this package.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import Iterable, List

import torch


@dataclass
class ValidationLoss:
    loss: float                # over all selected elements of all batches: sum(sums) / sum(counts), in fp64 (NaN when nothing was selected)
    utterance_losses: List[float]  # per utterance, in batch order: its own sums / counts
    sums: torch.Tensor         # f64 [utterances] on the host
    counts: torch.Tensor       # i64 [utterances] on the host: selected frames x mel
    frames: int                # selected frames over all batches


def validation_loss(cfm, batches: Iterable, *, seed=0, drop_audio_cond=False, drop_text=False) -> ValidationLoss:
    """``batches`` yields ``(mel [B, N, mel] zero-padded, texts, lens)`` with N = max(lens), as ``CFM.forward`` takes them -- of a padded bucket
    ``p`` of ``eval/prompts.get_inference_prompt`` that is ``(p[2], p[5], p[3])``.  Before batch ``i`` torch and Python's ``random`` are seeded
    with ``seed + i``, so the span, noise and time draws depend on (seed, position, shape) alone; the two drop flags are FIXED (default: the
    fully conditioned branch), not drawn.  The per-utterance sums stay on the device until the end: one synchronisation per call.  The same
    arguments give the same bits (the loss kernel adds in a fixed order)."""
    sums, counts = [], []
    for i, (mel, texts, lens) in enumerate(batches):
        torch.manual_seed(seed + i)
        random.seed(seed + i)
        mel = mel.to(cfm.device)
        lens = torch.as_tensor(lens, dtype=torch.long).to(mel.device)
        r = cfm.flow_loss(mel, texts, lens=lens, drop_audio_cond=drop_audio_cond, drop_text=drop_text)
        sums.append(r.sums)
        counts.append(r.counts)
        mel_dim = mel.shape[-1]
    if not sums:
        raise ValueError("validation_loss: no batches")
    s, c = torch.cat(sums).cpu(), torch.cat(counts).cpu()
    total_s, total_c = math.fsum(s.tolist()), int(c.sum())  # (the correctly rounded fp64 sum: no order to speak of)
    return ValidationLoss(loss=total_s / total_c if total_c else float("nan"),
                          utterance_losses=[float(a) / int(b) if int(b) else float("nan") for a, b in zip(s, c)],
                          sums=s, counts=c, frames=total_c // mel_dim)
