"""Validation loss of a checkpoint: the flow-matching loss of ``CFM.forward`` (reference cfm.py:210-283) over a list of batches, forward only,
and the duration loss and MAE of a duration predictor as the reference's trainer logs them (trainer.py:829-1068).

The number a checkpoint was trained on, for picking one after fine-tuning with the reference or judging a pruned model.  Nothing here can be
differentiated; there is no gradient, optimiser or trainer in this package.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import Iterable, List, Tuple

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


@dataclass
class DurationLoss:
    loss: float                # over all phonemes of all batches: sum(sq_sums) / sum(counts), in fp64 (NaN when there is no phoneme)
    mae: float                 # likewise sum(abs_sums) / sum(counts): mean absolute duration error in frames
    batch_losses: List[Tuple[float, float]]  # per batch, the (duration loss, duration MAE) pair the trainer would log for it (fp32)
    sq_sums: torch.Tensor      # f64 [utterances] on the host: sum of (logw - log(duration + 1e-6))^2 over the utterance's phonemes
    abs_sums: torch.Tensor     # f64 [utterances] on the host: sum of |exp(clamp(logw, -10, 10)) - duration|
    counts: torch.Tensor       # i64 [utterances] on the host: phonemes


def duration_validation_loss(predictor, batches: Iterable, *, algorithm="viterbi", mel_proj_matrix=None, seed=0) -> DurationLoss:
    """How good a duration predictor checkpoint is, by the numbers ``Trainer.calculate_duration_loss`` logs (reference trainer.py:925-1025).

    ``batches`` yields host tensors ``(mel [B, T, mel] zero-padded, mel_lens [B], phoneme_ids [B, nt] zero-padded, phoneme_lens [B])``.  Per
    batch, on the device: the phoneme x mel similarity (``alignment_similarity``: ids raw), the monotonic alignment search ``algorithm``
    ("viterbi" or "window"), the durations of the alignment, ``predictor(phoneme_ids, mask)`` -- ``forward``, which shifts the ids by one, as
    the trainer calls it (:1013) -- and the masked loss (``f5_duration_loss``).  Ids below 0 or above ``num_embeddings - 2`` are refused
    before any launch.  ``mel_proj_matrix`` [mel, embed_dim] is the fixed random projection of the mel frames; None draws
    ``randn(mel, embed_dim) / sqrt(mel)`` from a CPU generator seeded with ``seed`` (the trainer draws its own once per run, :934-937, so its
    logged numbers depend on that draw).  One synchronisation per call; the same arguments give the same bits.

    The searches align the PADDED batch as the reference does: an utterance with fewer phonemes than the batch maximum gives its whole length
    to the last padded row under "viterbi" (model/alignment_utils.py), so its real phonemes all get the 0.1-frame floor as their target."""
    from .. import _lib
    from ..model.alignment_utils import ALGORITHMS, alignment_durations, alignment_similarity
    if algorithm not in ALGORITHMS:
        raise ValueError(f"alignment algorithm {algorithm!r} is not built: choose one of {', '.join(repr(a) for a in ALGORITHMS)}")
    batches = list(batches)
    if not batches:
        raise ValueError("duration_validation_loss: no batches")
    rows = predictor.text_embed.num_embeddings
    for i, (_, _, ids, _) in enumerate(batches):
        ids = torch.as_tensor(ids)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) > rows - 2):
            raise ValueError(f"duration_validation_loss: batch {i} has phoneme ids outside [0, {rows - 2}] "
                             f"(forward() shifts them by one into an embedding of {rows} rows)")
    lib = _lib.load()
    dev = predictor.text_embed.weight.device
    K = predictor.text_embed.embedding_dim
    results, sizes = [], []
    for mel, mel_lens, ids, p_lens in batches:
        mel = torch.as_tensor(mel).to(device=dev, dtype=torch.float32)
        ids = torch.as_tensor(ids).to(dev)
        p_lens = torch.as_tensor(p_lens).to(device=dev, dtype=torch.int32).contiguous()
        B, nt = ids.shape
        if mel_proj_matrix is None:
            gen = torch.Generator().manual_seed(seed)
            mel_proj_matrix = torch.randn(mel.shape[-1], K, generator=gen) / math.sqrt(mel.shape[-1])
        sim = alignment_similarity(predictor, ids, p_lens, mel, mel_lens, mel_proj_matrix)
        durations = alignment_durations(sim, algorithm)
        mask = torch.arange(nt, device=dev)[None, :] < p_lens[:, None]
        logw = predictor(ids, mask).reshape(B, nt).contiguous()
        sq = torch.empty(B, dtype=torch.float64, device=dev)
        ab = torch.empty(B, dtype=torch.float64, device=dev)
        cnt = torch.empty(B, dtype=torch.int64, device=dev)
        pair = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(lib.f5_duration_loss(B, nt, _lib.ptr(logw), _lib.ptr(durations), _lib.ptr(p_lens), _lib.ptr(sq), _lib.ptr(ab), _lib.ptr(cnt),
                                        _lib.ptr(pair), _lib.stream_ptr()), "f5_duration_loss")
        results.append(torch.cat([sq, ab, cnt.double(), pair.double()]))  # (counts and fp32 values are exact in fp64: one copy at the end)
        sizes.append(B)
    host = torch.cat(results).cpu()
    sq_all, ab_all, cnt_all, pairs, at = [], [], [], [], 0
    for B in sizes:
        sq_all.append(host[at:at + B])
        ab_all.append(host[at + B:at + 2 * B])
        cnt_all.append(host[at + 2 * B:at + 3 * B].to(torch.int64))
        pairs.append((float(host[at + 3 * B]), float(host[at + 3 * B + 1])))
        at += 3 * B + 2
    sq_t, ab_t, cnt_t = torch.cat(sq_all), torch.cat(ab_all), torch.cat(cnt_all)
    total = int(cnt_t.sum())
    return DurationLoss(loss=math.fsum(sq_t.tolist()) / total if total else float("nan"),
                        mae=math.fsum(ab_t.tolist()) / total if total else float("nan"),
                        batch_losses=pairs, sq_sums=sq_t, abs_sums=ab_t, counts=cnt_t)
