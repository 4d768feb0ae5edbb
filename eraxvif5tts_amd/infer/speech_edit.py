"""Speech editing: regenerate chosen time spans of a recording and keep the rest -- the reference's ``infer/speech_edit.py`` as a library.

``build_edit_mask`` is the script's mask arithmetic (reference speech_edit.py:136-156, ``round()`` calls, the ``+ 1`` frame and the True
padding included); ``edit_speech`` runs the rest of the script (channel mean, rms boost, resampling, ``CFM.sample(edit_mask=...)``, vocoder,
rms restore, :126-189) on the HIP front end, the masked native sampler (``f5_sample_masked``) and the HIP vocoder.

As in the reference, the prompt is the ORIGINAL recording: the script builds a spliced waveform with silence in the edited spans but leaves
the line that would use it commented out (:153), so only the mask marks what is regenerated.  With ``fix_duration`` different from a span's
length the mask is laid out on the edited timeline and then cut or True-padded to the recording's frame count, exactly as there.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pad_sequence

from ..model.utils import convert_char_to_pinyin, list_str_to_idx, list_str_to_tensor
from . import audio as _audio


def build_edit_mask(num_samples, parts_to_edit, fix_duration=None, sample_rate=24000, hop_length=256):
    """bool [num_samples // hop_length + 1]: True = keep the prompt frame, False = regenerate it.  num_samples counts the waveform at
    ``sample_rate`` (after resampling); parts_to_edit = [[start_s, end_s], ...]; fix_duration = None (each span keeps its length) or one
    duration in seconds per span."""
    fix = None if fix_duration is None else list(fix_duration)
    if fix is not None and len(fix) != len(parts_to_edit):
        raise ValueError(f"fix_duration has {len(fix)} entries for {len(parts_to_edit)} parts to edit")
    offset = 0
    edit_mask = torch.zeros(1, 0, dtype=torch.bool)
    for start, end in parts_to_edit:
        part_dur = end - start if fix is None else fix.pop(0)
        part_dur = part_dur * sample_rate
        start = start * sample_rate
        edit_mask = torch.cat((edit_mask, torch.ones(1, round((start - offset) / hop_length), dtype=torch.bool),
                               torch.zeros(1, round(part_dur / hop_length), dtype=torch.bool)), dim=-1)
        offset = end * sample_rate
    # (a negative pad cuts the mask to the recording's frames)
    edit_mask = F.pad(edit_mask, (0, num_samples // hop_length - edit_mask.shape[-1] + 1), value=True)
    return edit_mask[0]


def _prepare(audio, sr, target_rms, target_sample_rate, device):
    """reference :126-134: channel mean, rms boost of a quiet recording, resampling.  -> (wave [n] at target_sample_rate, rms)"""
    audio = torch.as_tensor(audio, dtype=torch.float32)
    if audio.ndim == 1:
        audio = audio[None]
    if audio.shape[0] > 1:
        audio = torch.mean(audio, dim=0, keepdim=True)
    audio = audio.to(device)
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    if rms < target_rms:
        audio = audio * target_rms / rms
    if sr != target_sample_rate:
        audio = _audio.resample(audio, sr, target_sample_rate)  # on the device (f5_frontend_resample)
    return audio[0], rms


@torch.no_grad()
def edit_speech(model, vocoder, audio, sr, target_text, parts_to_edit, *, fix_duration=None, nfe_step=32, cfg_strength=2.0,
                sway_sampling_coef=-1.0, seed=None, target_rms=0.1):
    """Regenerate ``parts_to_edit`` of ``audio`` so that the whole recording says ``target_text``.

    model: a ``CFM`` over a HIP backbone (its ``odeint_kwargs`` choose the fixed-grid solver: euler, midpoint, rk4, heun2 or heun3); vocoder: plug point B (``.decode(mel)`` as Vocos, or
    called as BigVGAN); audio: waveform [n] or [channels, n] at ``sr`` Hz (tensor or array).  Returns ``(wave [1, samples], mel [1, n_mels,
    frames])`` on the model's device, the wave scaled back to the recording's loudness when it was boosted.

    A batch of edit jobs runs as ONE padded sample() (one mask per job, the key-padding mask on): pass lists of equal length for ``audio``,
    ``target_text`` and ``parts_to_edit`` (``sr`` an int or a list, ``fix_duration`` None or a list of per-job lists / None); the result is
    then ``([wave [1, samples_i]], [mel [1, n_mels, frames_i]])``."""
    batched = isinstance(target_text, (list, tuple))
    if not batched:
        audio, sr, target_text, parts_to_edit, fix_duration = [audio], [sr], [target_text], [parts_to_edit], [fix_duration]
    else:
        njobs = len(target_text)
        if not (len(audio) == len(parts_to_edit) == njobs):
            raise ValueError("audio, target_text and parts_to_edit need one entry per edit job")
        sr = list(sr) if isinstance(sr, (list, tuple)) else [sr] * njobs
        fix_duration = [None] * njobs if fix_duration is None else list(fix_duration)
        if len(sr) != njobs or len(fix_duration) != njobs:
            raise ValueError("sr and fix_duration need one entry per edit job")
    device = model.device
    ms = model.mel_spec
    hop, tsr = ms.hop_length, ms.target_sample_rate

    conds, masks, rmss, durations = [], [], [], []
    for a, s, parts, fix in zip(audio, sr, parts_to_edit, fix_duration):
        wave, rms = _prepare(a, s, target_rms, tsr, device)
        mask = build_edit_mask(wave.shape[-1], parts, fix, sample_rate=tsr, hop_length=hop)
        cond = ms(wave[None]).permute(0, 2, 1)[0]  # [frames, n_mels], frames = n // hop + 1 = len(mask)
        assert cond.shape[0] == mask.shape[0], (cond.shape, mask.shape)
        conds.append(cond)
        masks.append(mask)
        rmss.append(rms)
        durations.append(wave.shape[-1] // hop)  # reference :174 (ref_audio_len = 0)

    lens = torch.tensor([c.shape[0] for c in conds], device=device, dtype=torch.long)
    cond = pad_sequence(conds, batch_first=True)
    edit_mask = pad_sequence(masks, batch_first=True, padding_value=True).to(device)  # (frames past a job's lens are dropped by lens_to_mask)
    final_text = convert_char_to_pinyin(list(target_text))  # reference :163-166 (tokenizer "pinyin", every shipped config)
    text = (list_str_to_idx(final_text, model.vocab_char_map) if model.vocab_char_map is not None else list_str_to_tensor(final_text)).to(device)
    duration = torch.tensor(durations, device=device, dtype=torch.long)

    generated, _ = model.sample(cond=cond, text=text, duration=duration, lens=lens, steps=nfe_step, cfg_strength=cfg_strength,
                                sway_sampling_coef=sway_sampling_coef, seed=seed, edit_mask=edit_mask, return_trajectory=False)
    # the frames of each job: its own resolved duration (cfm.py:127-131), as a batch-1 call would return
    frames = torch.maximum(torch.maximum((text != -1).sum(dim=-1), lens) + 1, duration).clamp(max=4096).tolist()
    waves, mels = [], []
    for i, n in enumerate(frames):
        gen_mel = generated[i : i + 1, :n].to(torch.float32).permute(0, 2, 1)
        w = vocoder.decode(gen_mel) if hasattr(vocoder, "decode") else vocoder(gen_mel)
        w = w.reshape(1, -1)
        if rmss[i] < target_rms:
            w = w * rmss[i] / target_rms
        waves.append(w)
        mels.append(gen_mel)
    if batched:
        return waves, mels
    return waves[0], mels[0]
