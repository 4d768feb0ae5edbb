"""Monotonic alignment search: drop-in for the arithmetic of ``f5_tts/model/alignment_utils.py`` (reference :118-128, :154-258, :337-355)
and the alignment-method schedule of its trainer (:361-472).

The searches run in libf5hip (``f5_align_viterbi`` / ``f5_align_window``, csrc/align.hip) and return the reference's matrices bit for bit;
there is no eager fallback.  ``"progressive"`` is not built: the schedule below never selects it, and its result depends on the order of
``torch.sum`` over whole matrices.  The phonemizer front-ends of the reference file (viphoneme, phonemizer) are out of scope: every function
here takes phoneme index tensors.

The searches see the PADDED batch, exactly as in the reference: ``nt`` and ``T`` are the batch maxima.  An utterance with fewer phonemes than
``nt`` carries -inf in its last rows, and the viterbi backtrack then gives the utterance's whole length to the last padded row (durations
``[0, ..., 0, T]``).  This is the reference's behaviour and is kept, not repaired: align one utterance at a time, or batches of equal phoneme
count, if that is not what you want.
"""
from __future__ import annotations

import math

import torch

from .. import _lib

ALGORITHMS = ("viterbi", "window")
_ENTRY = {"viterbi": "f5_align_viterbi", "window": "f5_align_window"}


def _search(similarity, algorithm, want_alignment):
    if algorithm not in _ENTRY:
        raise ValueError(f"alignment algorithm {algorithm!r} is not built: choose one of {', '.join(repr(a) for a in ALGORITHMS)} "
                         "('progressive' of the reference is never selected by its trainer and is left out)")
    if similarity.ndim != 3:
        raise ValueError(f"similarity must be [b, nt, mel_len], got {tuple(similarity.shape)}")
    _lib.require_gpu()
    lib = _lib.load()
    sim = similarity.detach().to(device="cuda", dtype=torch.float32).contiguous()
    B, nt, T = sim.shape
    nbytes = lib.f5_align_workspace(B, nt, T)
    if nbytes < 0:
        raise _lib.F5HipError(f"libf5hip f5_align_workspace failed (code {nbytes}): {_lib.last_error()}")
    work = torch.empty(nbytes // 4, dtype=torch.int32, device=sim.device) if algorithm == "viterbi" else None
    durations = torch.empty(B, nt, dtype=torch.float32, device=sim.device)
    alignment = torch.empty(B, nt, T, dtype=torch.float32, device=sim.device) if want_alignment else None
    _lib.check(getattr(lib, _ENTRY[algorithm])(B, nt, T, _lib.ptr(sim), _lib.ptr(durations), _lib.ptr(alignment), _lib.ptr(work),
                                               _lib.stream_ptr()), _ENTRY[algorithm])
    return alignment, durations


def monotonic_alignment_search(similarity_matrix, algorithm="viterbi"):
    """similarity [b, nt, mel_len] -> hard alignment [b, nt, mel_len] of 0 / 1 on the device (reference :337-355)."""
    return _search(similarity_matrix, algorithm, True)[0]


def alignment_durations(similarity_matrix, algorithm="viterbi"):
    """Frames per phoneme [b, nt] of the same search, without materialising the alignment matrix."""
    return _search(similarity_matrix, algorithm, False)[1]


def get_durations_from_alignment(alignment):
    """alignment [b, nt, mel_len] -> durations [b, nt] (reference :118-128)."""
    return alignment.sum(dim=2)


def alignment_similarity(predictor, phoneme_ids, phoneme_lens, mel, mel_lens, mel_proj_matrix):
    """The phoneme x mel similarity the trainer aligns on (reference trainer.py:925-970): cosine similarity of ``predictor.text_embed`` rows
    (ids used raw, no +1) and the projected mel frames, + 3.0 around the diagonal, -inf on the padding.  phoneme_ids [b, nt], phoneme_lens [b],
    mel [b, T, mel_dim], mel_lens [b], mel_proj_matrix [mel_dim, embed_dim] -> [b, nt, T] fp32 on the device."""
    _lib.require_gpu()
    lib = _lib.load()
    table = predictor.text_embed.weight.detach()
    dev = table.device
    if dev.type != "cuda":
        raise _lib.F5HipError("alignment_similarity: the predictor must live on the GPU (no CPU path)")
    table = table.to(torch.float32).contiguous()
    ids = torch.as_tensor(phoneme_ids).to(device=dev, dtype=torch.int32).contiguous()
    melspec = torch.as_tensor(mel).detach().to(device=dev, dtype=torch.float32).contiguous()
    proj = torch.as_tensor(mel_proj_matrix).detach().to(device=dev, dtype=torch.float32).contiguous()
    p_lens = torch.as_tensor(phoneme_lens).to(device=dev, dtype=torch.int32).contiguous()
    m_lens = torch.as_tensor(mel_lens).to(device=dev, dtype=torch.int32).contiguous()
    if ids.ndim != 2 or melspec.ndim != 3 or melspec.shape[0] != ids.shape[0]:
        raise ValueError(f"phoneme_ids must be [b, nt] and mel [b, T, mel_dim], got {tuple(ids.shape)} and {tuple(melspec.shape)}")
    B, nt = ids.shape
    T, mel_dim = int(melspec.shape[1]), int(melspec.shape[2])
    rows, K = table.shape
    if tuple(proj.shape) != (mel_dim, K):
        raise ValueError(f"mel_proj_matrix must be [{mel_dim}, {K}], got {tuple(proj.shape)}")
    if p_lens.shape != (B,) or m_lens.shape != (B,):
        raise ValueError(f"phoneme_lens and mel_lens must be [{B}]")
    sim = torch.empty(B, nt, T, dtype=torch.float32, device=dev)
    _lib.check(lib.f5_align_similarity(B, nt, T, mel_dim, K, rows, _lib.ptr(table), _lib.ptr(ids), _lib.ptr(p_lens), _lib.ptr(melspec),
                                       _lib.ptr(m_lens), _lib.ptr(proj), _lib.ptr(sim), _lib.stream_ptr()), "f5_align_similarity")
    return sim


class AlignmentMethodManager:
    """Which search a training run uses when, and the weight of the duration loss (reference :361-435; host arithmetic only).

    Phase 1 trains the duration predictor alone on "window" alignments with weight 0.5.  Phase 2 (the full model) starts once
    ``duration_focus_updates`` updates are done, stays on "window" until epoch 3 and uses "viterbi" from then on; its weight falls from 0.5
    to 0.1 along half a cosine over ``decay_epochs`` epochs' worth of updates."""

    def __init__(self):
        self.current_method = "window"
        self.phase = 1
        self.initial_dur_weight = 0.5
        self.target_dur_weight = 0.1
        self.decay_epochs = 10
        self.max_decay_steps = None
        self.viterbi_start_epoch = 3

    def set_steps_per_epoch(self, steps_per_epoch):
        self.max_decay_steps = steps_per_epoch * self.decay_epochs
        return self.max_decay_steps

    def should_transition_to_phase2(self, global_update, duration_focus_updates):
        if global_update >= duration_focus_updates:
            return True, f"update {global_update} completes the {duration_focus_updates} duration-only updates"
        return False, "phase 1 goes on"

    def transition_to_phase2(self):
        self.phase, self.current_method = 2, "window"
        return "phase 2 begins, on the window search"

    def should_switch_to_viterbi(self, current_epoch):
        if self.phase != 2 or self.current_method == "viterbi":
            return False, "no switch outside phase 2 or once on viterbi"
        if current_epoch >= self.viterbi_start_epoch:
            return True, f"epoch {current_epoch} is at or past epoch {self.viterbi_start_epoch}, where viterbi starts"
        return False, f"epoch {current_epoch} is before epoch {self.viterbi_start_epoch}, where viterbi starts"

    def switch_to_viterbi(self):
        self.current_method = "viterbi"
        return "now on the viterbi search"

    def calculate_duration_weight(self, steps_in_phase2, current_epoch=None):
        if self.phase == 1:
            return self.initial_dur_weight
        steps = min(steps_in_phase2, self.max_decay_steps)
        falloff = 0.5 * (1 + math.cos(math.pi * steps / self.max_decay_steps))
        return self.target_dur_weight + (self.initial_dur_weight - self.target_dur_weight) * falloff


def get_alignment_method(manager, global_update, duration_focus_updates=12000, phase2_start_update=None, current_epoch=None):
    """One scheduling step (reference :438-472): advances ``manager`` and returns ``(method, logs)`` with the phase and method the call
    STARTED in, the transitions it made and the duration-loss weight."""
    logs = {"phase": manager.phase, "method": manager.current_method}
    if manager.phase == 1:
        go, reason = manager.should_transition_to_phase2(global_update, duration_focus_updates)
        if go:
            manager.transition_to_phase2()
            logs["phase_transition"], logs["transition_reason"] = True, reason
    if manager.phase == 2 and current_epoch is not None:
        go, reason = manager.should_switch_to_viterbi(current_epoch)
        if go:
            manager.switch_to_viterbi()
            logs["method_switch"], logs["switch_reason"] = True, reason
    if manager.phase == 2 and phase2_start_update is not None:
        logs["duration_weight"] = manager.calculate_duration_weight(global_update - phase2_start_update, current_epoch=current_epoch)
    else:
        logs["duration_weight"] = manager.initial_dur_weight
    return manager.current_method, logs
