"""Shared inference helpers: drop-in for the hot-path functions of ``f5_tts/infer/utils_infer.py``.

``chunk_text`` (:70-97), ``load_vocoder`` (:101-139), ``load_checkpoint`` (:184-226), ``load_model`` (:232-266),
``preprocess_ref_audio_text`` (:292-360, without the ASR branch), ``infer_process`` (:366-414) and ``infer_batch_process``
(:417-563) keep the reference's names, arguments, defaults and return values.  Out of scope here: the Whisper
ASR pipeline (``transcribe``: a by-name hub download), BigVGAN, the Gradio/CLI shells.
"""
from __future__ import annotations

import hashlib
import os
import re
import tempfile

import numpy as np
import torch

from ..model import CFM
from ..model.utils import convert_char_to_pinyin, get_tokenizer
from . import audio as _audio

device = "cuda" if torch.cuda.is_available() else "cpu"

# -----------------------------------------
target_sample_rate = 24000
n_mel_channels = 100
hop_length = 256
win_length = 1024
n_fft = 1024
mel_spec_type = "vocos"
target_rms = 0.1
cross_fade_duration = 0.15
ode_method = "euler"  # torchdiffeq fixed-grid solver: euler, midpoint, rk4, heun2 or heun3 (model.cfm.ODE_METHODS)
nfe_step = 32  # 16, 32
cfg_strength = 2.0
sway_sampling_coef = -1.0
speed = 1.0
fix_duration = None
# -----------------------------------------

_ref_audio_cache = {}
DEFAULT_VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "examples", "vocab.txt")


def chunk_text(text, max_chars=135):
    """Split `text` into chunks of at most `max_chars` utf-8 BYTES at sentence punctuation (reference :70-97)."""
    chunks, current = [], ""
    sentences = re.split(r"(?<=[;:,.!?])\s+|(?<=[；：，。！？])", text)
    for sentence in sentences:
        piece = sentence + " " if sentence and len(sentence[-1].encode("utf-8")) == 1 else sentence
        if len(current.encode("utf-8")) + len(sentence.encode("utf-8")) <= max_chars:
            current += piece
        else:
            if current:
                chunks.append(current.strip())
            current = piece
    if current:
        chunks.append(current.strip())
    return chunks


def load_vocoder(vocoder_name="vocos", is_local=False, local_path="", device=device, hf_cache_dir=None):
    """Plug point B.  Only local weights can be loaded (there is no network): BigVGAN from ``{local_path}/config.json`` + ``bigvgan_generator.pt``; Vocos from ``{local_path}/config.yaml`` +
    ``{local_path}/pytorch_model.bin`` as the reference's is_local branch reads them (:104-107,113-124)."""
    if vocoder_name == "bigvgan":  # reference :125-138 (parity unpinned: the BigVGAN checkout is absent from the reference tree, see eraxvif5tts_amd/bigvgan.py)
        from ..bigvgan import BigVGAN
        if not is_local:
            raise RuntimeError("snapshot_download of nvidia/bigvgan_v2_24khz_100band_256x is not possible offline: pass is_local=True with a local directory "
                               "(config.json + bigvgan_generator.pt)")
        vocoder = BigVGAN.from_pretrained(local_path, use_cuda_kernel=False)
        vocoder.remove_weight_norm()
        return vocoder.eval().to(device)
    if vocoder_name != "vocos":
        raise NotImplementedError(f"vocoder {vocoder_name}: vocos and bigvgan are the reference's two")
    from ..vocos import Vocos
    if not is_local:
        raise RuntimeError("Download Vocos from huggingface charactr/vocos-mel-24khz is not possible offline: pass "
                           "use_local_vocoder=True / is_local=True with a local vocos-mel-24khz directory")
    print(f"Load vocos from local path {local_path}")
    config_path, model_path = f"{local_path}/config.yaml", f"{local_path}/pytorch_model.bin"
    vocoder = Vocos.from_hparams(config_path)
    state_dict = torch.load(model_path, map_location="cpu", weights_only=True)
    own = vocoder.state_dict()
    vocoder.load_state_dict({k: v for k, v in state_dict.items() if k in own}, strict=False)  # feature_extractor.* buffers are not used by decode()
    return vocoder.eval().to(device)


def load_checkpoint(model, ckpt_path, device: str, dtype=None, use_ema=True):
    """Reference :184-226.  The reference casts the model to fp16 on CUDA here; the HIP backbone keeps fp32 master weights in the module and
    converts them once to the kernel layouts of its precision mode: bf16 (default), fp32, or fp16 -- the reference's own GPU dtype -- as
    chosen by ``precision=`` / ``F5HIP_PRECISION``.  ``dtype`` is accepted for the reference's signature."""
    ckpt_type = ckpt_path.split(".")[-1]
    if ckpt_type == "safetensors":
        from safetensors.torch import load_file
        checkpoint = load_file(ckpt_path, device="cpu")
    else:
        checkpoint = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    if use_ema:
        if ckpt_type == "safetensors":
            checkpoint = {"ema_model_state_dict": checkpoint}
        checkpoint["model_state_dict"] = {k.replace("ema_model.", ""): v for k, v in checkpoint["ema_model_state_dict"].items()
                                          if k not in ["initted", "step"]}
        for key in ["mel_spec.mel_stft.mel_scale.fb", "mel_spec.mel_stft.spectrogram.window"]:  # backward compatibility, as the reference
            checkpoint["model_state_dict"].pop(key, None)
    elif ckpt_type == "safetensors":
        checkpoint = {"model_state_dict": checkpoint}
    model.load_state_dict(checkpoint["model_state_dict"], strict=False)
    del checkpoint
    return model.to(device)


def load_model(model_cls, model_cfg, ckpt_path, mel_spec_type=mel_spec_type, vocab_file="", ode_method=ode_method, use_ema=True,
               device=device):
    if vocab_file == "":
        vocab_file = DEFAULT_VOCAB
    tokenizer = "custom"
    print("\nvocab : ", vocab_file)
    print("token : ", tokenizer)
    print("model : ", ckpt_path, "\n")
    vocab_char_map, vocab_size = get_tokenizer(vocab_file, tokenizer)
    model = CFM(
        transformer=model_cls(**model_cfg, text_num_embeds=vocab_size, mel_dim=n_mel_channels),
        mel_spec_kwargs=dict(n_fft=n_fft, hop_length=hop_length, win_length=win_length, n_mel_channels=n_mel_channels,
                             target_sample_rate=target_sample_rate, mel_spec_type=mel_spec_type),
        odeint_kwargs=dict(method=ode_method),
        vocab_char_map=vocab_char_map,
    ).to(device)
    return load_checkpoint(model, ckpt_path, device, use_ema=use_ema)


def remove_silence_edges(audio, silence_threshold=-42):
    return _audio.remove_silence_edges(audio, silence_threshold)


def preprocess_ref_audio_text(ref_audio_orig, ref_text, clip_short=True, show_info=print):
    show_info("Converting audio...")
    aseg = _audio.Segment.from_file(ref_audio_orig)
    if clip_short:
        aseg = _audio.clip_reference(aseg, show_info)
    aseg = remove_silence_edges(aseg)
    aseg = aseg + aseg.silent_like(50)
    with tempfile.NamedTemporaryFile(delete=False, suffix=".wav") as f:
        ref_audio = f.name
    _audio.write_wav(ref_audio, _audio.segment_to_float(aseg).mean(dim=0).numpy(), aseg.frame_rate)
    with open(ref_audio, "rb") as fh:
        audio_hash = hashlib.md5(fh.read()).hexdigest()
    if not ref_text.strip():
        if audio_hash in _ref_audio_cache:
            show_info("Using cached reference text...")
            ref_text = _ref_audio_cache[audio_hash]
        else:
            raise RuntimeError("No reference text provided and the ASR model (openai/whisper-large-v3-turbo, a network download) "
                               "is not part of this build: pass ref_text")
    else:
        show_info("Using custom reference text...")
    if not ref_text.endswith(". ") and not ref_text.endswith("。"):
        ref_text += " " if ref_text.endswith(".") else ". "
    print("\nref_text  ", ref_text)
    return ref_audio, ref_text


def _load_audio(path):
    seg = _audio.Segment.from_file(path)
    return _audio.segment_to_float(seg), seg.frame_rate


def cross_fade_concat(waves, cross_fade_duration, sample_rate=target_sample_rate):
    """Linear cross-fade of consecutive chunks (reference :519-555 / f5tts_wrapper.py:541-575)."""
    if cross_fade_duration <= 0:
        return np.concatenate(waves)
    final = waves[0]
    for nxt in waves[1:]:
        n = min(int(cross_fade_duration * sample_rate), len(final), len(nxt))
        if n <= 0:
            final = np.concatenate([final, nxt])
            continue
        mixed = final[-n:] * np.linspace(1, 0, n) + nxt[:n] * np.linspace(0, 1, n)
        final = np.concatenate([final[:-n], mixed, nxt[n:]])
    return final


# ---------------------------------------------------------------------------- the tail behind the sampler, on the device
# Per utterance the reference runs one batch-1 vocoder call, the rms rule with a device -> host comparison, a device -> host copy, and then
# cross_fade_concat / pcm16_bytes in numpy.  With the HIP vocoders the same arithmetic runs as ONE ragged decode (Vocos.decode_ragged /
# BigVGAN.decode_ragged), ONE f5_wave_finish and ONE copy, byte-identical (tests/test_gpu_wave_tail.py), so no switch selects it:
# `waves_of_mels` (F5TTSWrapper, infer_batch_process) and eval.prompts.infer_prompts take it whenever the objects at hand allow it, and the
# per-utterance host loop otherwise.

def plan_wave_tail(lengths, cross_fade_duration, sample_rate=target_sample_rate):
    """What `cross_fade_concat` does to waves of these lengths, from the lengths alone: ``joints`` (the n of every joint, by the reference's
    sequential rule ``min(int(d * rate), len(final), len(next))``), ``out_offsets`` (where each wave's first sample lands in the result),
    ``total`` samples, ``mixed`` (a joint with n > 0 exists: that piece is float64 and np.concatenate promotes the WHOLE result, so
    `pcm16_bytes` multiplies in float64; otherwise everything stays float32), ``dtype``, the uniform ``n`` the device kernel takes, and
    ``device_ok``: no joint reaches into a region an earlier joint mixed (first and last wave >= n samples, every other >= 2 n) --
    the rule of ``f5_wave_finish``, which answers F5_ENOTSUP otherwise."""
    lengths = [int(x) for x in lengths]
    nx = max(int(cross_fade_duration * sample_rate), 0) if cross_fade_duration > 0 else 0
    joints, offsets, final_len = [], [0], lengths[0]
    for length in lengths[1:]:
        n = max(min(nx, final_len, length), 0)
        joints.append(n)
        offsets.append(final_len - n)
        final_len += length - n
    mixed = any(n > 0 for n in joints)
    n_dev = nx if len(lengths) >= 2 else 0
    device_ok = all(length >= (n_dev if i in (0, len(lengths) - 1) else 2 * n_dev) for i, length in enumerate(lengths))
    return dict(joints=joints, out_offsets=offsets, total=final_len, mixed=mixed, dtype=np.float64 if mixed else np.float32, n=n_dev,
                device_ok=device_ok)


def plan_wave_tail_segments(lengths, seg_sizes, cross_fade_duration, sample_rate=target_sample_rate):
    """`plan_wave_tail` for ``np.concatenate([cross_fade_concat(seg) for seg in segments])`` -- a script in several voices: cross-fades inside
    a segment, plain concatenation between segments -- from the lengths alone.  ``seg_sizes`` lists the utterances per segment, in order
    (they sum to ``len(lengths)``).  ``joints`` holds the n of every joint of the flat list (0 between segments), ``out_offsets`` / ``total`` /
    ``mixed`` / ``dtype`` describe the concatenated result (float64 throughout once ANY joint mixed: np.concatenate promotes the segments
    that mixed nothing too), ``n`` is the cross-fade length the device kernel takes at in-segment joints, ``seg_start`` the 0/1 array
    ``f5_wave_finish_segments`` takes, and ``device_ok`` its chaining rule per segment: in a segment of two or more utterances the first and
    the last hold at least n samples, every inner one 2 n; a one-utterance segment has no constraint."""
    lengths, seg_sizes = [int(x) for x in lengths], [int(x) for x in seg_sizes]
    assert sum(seg_sizes) == len(lengths) and all(g >= 1 for g in seg_sizes)
    joints, offsets, seg_start, total, mixed, device_ok, k = [], [], [], 0, False, True, 0
    for g in seg_sizes:
        plan = plan_wave_tail(lengths[k: k + g], cross_fade_duration, sample_rate)
        if k:
            joints.append(0)
        joints += plan["joints"]
        offsets += [total + o for o in plan["out_offsets"]]
        seg_start += [1] + [0] * (g - 1)
        total += plan["total"]
        mixed = mixed or plan["mixed"]
        device_ok = device_ok and plan["device_ok"]
        k += g
    nx = max(int(cross_fade_duration * sample_rate), 0) if cross_fade_duration > 0 else 0
    return dict(joints=joints, out_offsets=offsets, total=total, mixed=mixed, dtype=np.float64 if mixed else np.float32,
                n=nx if max(seg_sizes) >= 2 else 0, device_ok=device_ok, seg_start=seg_start)


def split_voice_script(text, voices, show_info=print):
    """A script with ``[name]`` tags -> ``[(voice, text)]``, by the reference's rule (infer_cli.py:306-324): the text is cut in front of every
    ``[word]`` tag, blank pieces are skipped, a piece's voice is the tag it starts with -- "main" when it starts with none or the name is not in
    ``voices`` (with the reference's two messages) -- and every tag is removed from the piece's text, which is stripped.  One deviation: a piece
    whose text is empty after that is dropped (the reference hands "" on and fails inside infer_batch_process)."""
    tag = r"\[(\w+)\]"
    pieces = []
    for chunk in re.split(r"(?=\[\w+\])", text):
        if not chunk.strip():
            continue
        match = re.match(tag, chunk)
        if match:
            voice = match[1]
        else:
            show_info("No voice tag found, using main.")
            voice = "main"
        if voice not in voices:
            show_info(f"Voice {voice} not found, using main.")
            voice = "main"
        piece = re.sub(tag, "", chunk).strip()
        if piece:
            pieces.append((voice, piece))
    return pieces


_xfade_tables = {}


def _xfade_weights(n, dev):
    """numpy's own linspace(1, 0, n) / linspace(0, 1, n) on the device (uploaded once per n): the kernel multiplies by exactly these doubles"""
    key = (int(n), str(dev))
    if key not in _xfade_tables:
        _xfade_tables[key] = (torch.from_numpy(np.linspace(1, 0, n)).to(dev), torch.from_numpy(np.linspace(0, 1, n)).to(dev))
    return _xfade_tables[key]


def _rms_forms(rms, B, target_rms, rms_index=None):
    """The rms rule in the forms the library takes (`finish_waves` documents ``rms``): ``(gain_host, apply_host, rms_dev)``, ctypes arrays of B
    host gains with the decision ``rms_i < target_rms`` taken here exactly as the host loop takes it, or the device scalar -- with ``rms_index``
    (one entry per utterance) the device vector of one value per voice; all None: no gain."""
    import ctypes as C
    gain_host = apply_host = rms_dev = None
    if torch.is_tensor(rms) and rms.is_cuda:
        assert rms.dtype == torch.float32 and (rms.numel() == 1 if rms_index is None else rms.ndim == 1 and rms.numel() >= 1)
        assert rms_index is None or (len(rms_index) == B and all(0 <= int(i) < rms.numel() for i in rms_index))
        rms_dev = rms.reshape(-1).contiguous()
    elif rms is not None:
        assert rms_index is None, "rms_index goes with a device vector of rms values"
        per_utt = list(rms) if isinstance(rms, (list, tuple)) else [rms] * B
        assert len(per_utt) == B
        on_dev = [i for i, r in enumerate(per_utt) if torch.is_tensor(r) and r.is_cuda]
        vals = [None if i in on_dev else float(r) for i, r in enumerate(per_utt)]
        if on_dev:  # rms values that live on the device come over in ONE copy (the host loop reads each of them back for its comparison)
            for i, v in zip(on_dev, torch.stack([per_utt[i].reshape(()).to(torch.float64) for i in on_dev]).cpu().tolist()):
                vals[i] = v

        def below_target(r, v):  # `r < target_rms` as torch / Python evaluate it: an fp32 tensor compares in fp32, a number in double
            if torch.is_tensor(r):
                return bool(np.float32(v) < np.float32(target_rms)) if r.dtype == torch.float32 else bool(r.cpu() < target_rms)
            return bool(r < target_rms)
        gain_host = (C.c_float * B)(*vals)
        apply_host = (C.c_uint8 * B)(*[1 if below_target(r, v) else 0 for r, v in zip(per_utt, vals)])
    return gain_host, apply_host, rms_dev


class _TailList:
    """One utterance list as the library takes it, for `finish_waves` and `WaveStream` alike (both call the ``_segments`` entry points: a list
    without segments is one segment with rms index 0): the plan, ``n`` / ``mixed``, the rms rule in its forms (`_rms_forms`) and the ctypes
    arrays ``seg_start`` / ``rms_index`` / ``pcm_f32`` over the whole list (None where the library takes NULL)."""

    def __init__(self, samples, cross_fade_duration, sample_rate, rms, target_rms, gain_divide, segments, rms_index, pcm_f32):
        import ctypes as C
        self.samples = [int(x) for x in samples]
        B = len(self.samples)
        self.plan = plan_wave_tail_segments(self.samples, [B] if segments is None else segments, cross_fade_duration, sample_rate)
        self.n, self.mixed = self.plan["n"], self.plan["n"] > 0
        self.gain_host, self.apply_host, self.rms_dev = _rms_forms(rms, B, target_rms, rms_index)
        self.n_rms = int(self.rms_dev.numel()) if self.rms_dev is not None else 0
        self.seg_start = (C.c_uint8 * B)(*self.plan["seg_start"])
        self.rms_index = (C.c_int32 * B)(*[int(i) for i in rms_index]) if rms_index is not None and self.rms_dev is not None else None
        self.pcm_f32 = (C.c_uint8 * B)(*[1 if f else 0 for f in pcm_f32]) if pcm_f32 is not None else None
        self.target_rms, self.gain_div = float(target_rms), 1 if gain_divide else 0

    def weights(self, dev):
        """the cross-fade tables on ``dev`` (None, None when nothing mixes)"""
        return _xfade_weights(self.n, dev) if self.mixed else (None, None)


def finish_waves(wave, samples, cross_fade_duration=0.0, sample_rate=target_sample_rate, rms=None, target_rms=target_rms, want_float=True,
                 want_pcm16=False, gain_divide=False, segments=None, rms_index=None, pcm_f32=None):
    """``f5_wave_finish`` over the utterances held back to back in ``wave`` (fp32, on the GPU; ``samples[i]`` each): the rms rule, the linear
    cross-fade of `cross_fade_concat` and the int16 PCM of ``streaming.wire.pcm16_bytes`` in one kernel.  Returns ``(signal, pcm16)`` as device
    tensors (None where not asked for) -- ``signal`` float64 when a joint mixed, float32 otherwise, as numpy's promotion gives -- or ``None`` when
    the library answers F5_ENOTSUP (utterances shorter than their cross-fades: take the host functions for that call).
    ``rms``: None (no gain); a 0-dim fp32 tensor on the GPU (the gain applies when ``rms < target_rms``, decided on the device: no host wait);
    or host values -- one number / 0-dim CPU tensor for all utterances, or one per utterance -- with the decision ``rms_i < target_rms`` taken
    here exactly as the host loop takes it.  The gain is ``w * rms / target_rms`` as torch evaluates it on a GPU tensor (fp32 product, then the
    fp32 reciprocal of the host scalar), or with a true fp32 divide (``gain_divide``: torch on CPU tensors).
    ``segments`` (utterances per segment, in order; ``f5_wave_finish_segments``): the cross-fade runs inside each segment and the segments are
    joined without one -- ``np.concatenate([cross_fade_concat(seg) for seg in segments])``, see `plan_wave_tail_segments`.  ``rms_index`` (one
    entry per utterance): ``rms`` is then a 1-D fp32 GPU tensor with one value per voice and utterance k takes ``rms[rms_index[k]]``.
    ``pcm_f32`` (one flag per utterance, only for one-utterance segments): that utterance's int16 is the one a call over it alone gives -- the
    product in fp32 -- although the whole result is float64; without it ``pcm16`` is ``pcm16_bytes`` of the returned signal."""
    import ctypes as C

    from .. import _lib
    B = len(samples)
    assert wave.is_cuda and wave.dtype == torch.float32 and wave.is_contiguous() and wave.numel() == sum(samples) and B >= 1
    t = _TailList(samples, cross_fade_duration, sample_rate, rms, target_rms, gain_divide, segments, rms_index, pcm_f32)
    n, mixed = t.n, t.mixed
    total = sum(samples) - n * (B - sum(t.plan["seg_start"]))
    w_down, w_up = t.weights(wave.device)
    if total <= 0 or not t.plan["device_ok"]:
        out = pcm = None  # the library decides (and says why); nothing is allocated for a call it will refuse
    else:
        out = torch.empty(total, device=wave.device, dtype=torch.float64 if mixed else torch.float32) if want_float else None
        pcm = torch.empty(total, device=wave.device, dtype=torch.int16) if want_pcm16 else None
    got = C.c_int64(0)
    rc = _lib.load().f5_wave_finish_segments(B, _lib.ptr(wave), (C.c_int32 * B)(*t.samples), t.seg_start, t.gain_host, t.apply_host,
                                             _lib.ptr(t.rms_dev), t.n_rms, t.rms_index, t.target_rms, t.gain_div, int(n), _lib.ptr(w_down),
                                             _lib.ptr(w_up), t.pcm_f32, _lib.ptr(out) if not mixed else None, _lib.ptr(out) if mixed else None,
                                             _lib.ptr(pcm), C.byref(got), _lib.stream_ptr())
    if rc == _lib.F5_ENOTSUP:
        return None
    _lib.check(rc, "wave_finish")
    assert got.value == total
    return out, pcm


# ---------------------------------------------------------------------------- the same tail, group by group (generate_stream)
def chunk_groups(durations, first=0, group_max=8, max_rows=16384):
    """Cut chunks of these frame counts, in order, into groups of consecutive indices: the first ``first`` chunks form group 0 (``first`` <= 0: no
    such group), the rest goes into groups of at most ``group_max`` chunks and ``max_rows`` frames (a chunk longer than that stands alone) --
    with ``first = 0`` the groups one ragged sampler call each takes in `F5TTSWrapper.generate`.  A pure function of the durations."""
    durations = [int(d) for d in durations]
    group_max = max(1, int(group_max))
    head = min(max(int(first), 0), len(durations))
    groups = [list(range(head))] if head else []
    group, rows = [], 0
    for i in range(head, len(durations)):
        if group and (len(group) >= group_max or rows + durations[i] > max_rows):
            groups.append(group)
            group, rows = [], 0
        group.append(i)
        rows += durations[i]
    if group:
        groups.append(group)
    return groups


def plan_request_groups(keys, durations, group_max=8, max_rows=16384):
    """The sampler calls of `F5TTSWrapper.generate_batch`: jobs ``0 .. len(keys) - 1`` (the chunks of all requests, in flat order) cut into groups
    of indices.  ``keys[i]`` is job i's ``(nfe_step, sway_sampling_coef, cfg_strength >= 1e-5)`` -- what one sampler call must share: the step
    count, the time grid and the branch of cfm.py:167 -- and ``durations[i]`` its frame count.  Jobs of one key keep their flat order and go
    through `chunk_groups` (at most ``group_max`` jobs and ``max_rows`` frames per group); the keys are visited in order of first appearance,
    so a request mix that recurs meets the same time grids in the same order.  A pure function of its arguments."""
    assert len(keys) == len(durations)
    by_key = {}
    for i, key in enumerate(keys):
        by_key.setdefault(key, []).append(i)
    groups = []
    for members in by_key.values():
        groups += [[members[j] for j in g] for g in chunk_groups([durations[i] for i in members], 0, group_max, max_rows)]
    return groups


def stream_emitted_counts(lengths, group_sizes, cross_fade_duration, sample_rate=target_sample_rate, segments=None):
    """Output samples each push of a `WaveStream` over waves of these ``lengths`` emits when the list is pushed in consecutive groups of
    ``group_sizes`` utterances: a push that ends before the last utterance emits up to where the next utterance's first sample lands
    (`plan_wave_tail`'s ``out_offsets``), the last push the rest.  Returns ``(counts, dtype)``; the counts sum to the plan's ``total`` and the
    dtype is the whole result's -- float64 when any joint mixes, for EVERY piece, float32 otherwise.  ``segments``: the utterances per segment
    of a segmented stream (`plan_wave_tail_segments`); a push that ends a segment emits all of it."""
    plan = (plan_wave_tail(lengths, cross_fade_duration, sample_rate) if segments is None
            else plan_wave_tail_segments(lengths, segments, cross_fade_duration, sample_rate))
    assert sum(group_sizes) == len(lengths) and all(g >= 1 for g in group_sizes)
    bounds = plan["out_offsets"] + [plan["total"]]
    counts, k = [], 0
    for g in group_sizes:
        counts.append(bounds[k + g] - bounds[k])
        k += g
    return counts, plan["dtype"]


class WaveStream:
    """`finish_waves` in consecutive pushes (``f5_wave_stream_*``): ``samples`` lists the sample counts of ALL utterances up front -- they follow
    from the frame counts, before any sampling -- and ``push(wave, samples)`` hands over the next few, back to back in one fp32 GPU buffer.  The
    pieces, concatenated, are byte-identical to ``finish_waves`` over the whole list; every piece has the whole result's dtype.  ``rms``: None, a
    0-dim fp32 GPU tensor, one host value, or one host value per utterance of the whole list.  ``ok`` is False when the library would refuse
    the list (`plan_wave_tail`'s ``device_ok``): then nothing is created and the caller keeps its one-shot route.  ``close()`` frees the session.
    ``segments`` / ``rms_index`` / ``pcm_f32`` as for `finish_waves`, over the whole list (``f5_wave_stream_create_segments``)."""

    def __init__(self, samples, cross_fade_duration=0.0, sample_rate=target_sample_rate, rms=None, target_rms=target_rms, want_float=True,
                 want_pcm16=False, gain_divide=False, segments=None, rms_index=None, pcm_f32=None):
        import ctypes as C

        from .. import _lib
        assert want_float or want_pcm16
        t = _TailList(samples, cross_fade_duration, sample_rate, rms, target_rms, gain_divide, segments, rms_index, pcm_f32)
        self.samples, self.plan, self.n, self.mixed = t.samples, t.plan, t.n, t.mixed
        self.ok = bool(self.plan["device_ok"]) and min(self.samples) > 0
        self.want_float, self.want_pcm16, self.done, self._handle = want_float, want_pcm16, 0, None
        self._gain_host, self._apply_host, self._rms_dev = t.gain_host, t.apply_host, t.rms_dev
        if not self.ok:
            return
        self._tables = t.weights(torch.device("cuda", torch.cuda.current_device()))  # (kept alive with the session, which reads them in every push)
        handle = C.c_void_p()
        rc = _lib.load().f5_wave_stream_create_segments(len(self.samples), t.seg_start, int(self.n), _lib.ptr(self._tables[0]),
                                                        _lib.ptr(self._tables[1]), _lib.ptr(self._rms_dev), t.n_rms, t.rms_index, t.target_rms,
                                                        t.gain_div, t.pcm_f32, C.byref(handle))
        _lib.check(rc, "wave_stream_create")
        self._handle = handle

    def push(self, wave, samples):
        """The next ``len(samples)`` utterances -> ``(signal_or_None, pcm_or_None)`` device tensors holding what has become final."""
        import ctypes as C

        from .. import _lib
        lib = _lib.load()
        B, k = len(samples), self.done
        samples = [int(x) for x in samples]
        assert self._handle is not None, "the stream is closed, or its utterances chain (ok is False)"
        assert B >= 1 and samples == self.samples[k: k + B], "a push takes the next utterances of the list given at construction"
        assert wave.is_cuda and wave.dtype == torch.float32 and wave.is_contiguous() and wave.numel() == sum(samples)
        arr = (C.c_int32 * B)(*samples)
        gains = (C.c_float * B)(*self._gain_host[k: k + B]) if self._gain_host is not None else None
        applies = (C.c_uint8 * B)(*self._apply_host[k: k + B]) if self._apply_host is not None else None
        got = C.c_int64(0)
        _lib.check(lib.f5_wave_stream_push(self._handle, B, None, arr, gains, applies, None, None, None, C.byref(got), None), "wave_stream_push")
        count = got.value
        # (a zero-sized tensor has no address, and a push without outputs is the question above: one element at least, cut off below)
        out = torch.empty(max(count, 1), device=wave.device, dtype=torch.float64 if self.mixed else torch.float32) if self.want_float else None
        pcm = torch.empty(max(count, 1), device=wave.device, dtype=torch.int16) if self.want_pcm16 else None
        _lib.check(lib.f5_wave_stream_push(self._handle, B, _lib.ptr(wave), arr, gains, applies, _lib.ptr(out) if not self.mixed else None,
                                           _lib.ptr(out) if self.mixed else None, _lib.ptr(pcm), C.byref(got), _lib.stream_ptr()), "wave_stream_push")
        assert got.value == count
        self.done += B
        return (out[:count] if out is not None else None), (pcm[:count] if pcm is not None else None)

    def close(self):
        if self._handle is not None:
            from .. import _lib
            _lib.load().f5_wave_stream_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


# ---------------------------------------------------------------------------- remove silence (reference :569-578)
# The reference runs pydub's split_on_silence(min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10) on the exported 16-bit file
# and rewrites the file from the kept parts.  The rule here is `audio.split_on_silence`, this package's stand-in for pydub; the PCM that is judged
# is the one `audio.write_wav` puts into the file (rounded, never the truncating streaming PCM).  On the device (csrc/silence.hip) the same
# integer arithmetic gives the same parts, so only the kept samples cross to the host.
SILENCE_DEFAULTS = dict(min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10)


def remove_silence_for_generated_wav(filename):
    """The reference's name, at file level: the 16-bit file is read, split at the reference's four values and rewritten from the kept parts."""
    aseg = _audio.Segment.from_file(filename)
    kept = aseg.silent_like(0)
    for part in _audio.split_on_silence(aseg, **SILENCE_DEFAULTS):
        kept = kept + part
    _audio.write_wav_pcm16(filename, kept.samples[:, 0], aseg.frame_rate)


def rounded_pcm16(wave):
    """the int16 samples `audio.write_wav` stores for this float wave (product in float64, round half to even, clipped)"""
    x = np.asarray(wave, dtype=np.float64).reshape(-1)
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def _silence_windows(n_samples, sample_rate, min_silence_len, seek_step):
    """(n_ms, window starts, table entries) the library derives from the same four numbers (f5hip.h)"""
    n_ms = int(round(1000.0 * n_samples / sample_rate))
    windows = 0
    if n_ms >= min_silence_len:
        last = n_ms - min_silence_len
        windows = last // seek_step + 1 + (1 if last % seek_step else 0)
    return n_ms, windows, n_ms // max(min_silence_len, 1) + 2


def silence_ranges(wave, sample_rate=target_sample_rate, *, min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10):
    """``f5_op_silence_ranges``: the decision alone for a 1-D fp32 / fp64 wave on the GPU -> ``(flags, table, kept, parts)``: one byte per window
    start (1 = silent), the parts as rows ``(first sample, end sample, position in the output)``, the kept samples and the number of parts
    (host numbers: this copies)."""
    from .. import _lib
    lib = _lib.load()
    assert wave.is_cuda and wave.dim() == 1 and wave.is_contiguous() and wave.dtype in (torch.float32, torch.float64)
    n = wave.numel()
    n_ms, windows, cap = _silence_windows(n, sample_rate, min_silence_len, seek_step)
    need = lib.f5_wave_remove_silence_workspace(n, int(sample_rate), int(min_silence_len), int(seek_step))
    ws = torch.empty(max(int(need), 16), device=wave.device, dtype=torch.uint8)
    flags = torch.zeros(max(windows, 1), device=wave.device, dtype=torch.uint8)
    table = torch.zeros(cap, 3, device=wave.device, dtype=torch.int32)
    counts = torch.zeros(2, device=wave.device, dtype=torch.int64)
    rc = lib.f5_op_silence_ranges(_lib.ptr(wave) if n else None, int(wave.dtype == torch.float64), n, int(sample_rate), n_ms, int(min_silence_len),
                                  _audio.silence_threshold_floor(silence_thresh), int(keep_silence), int(seek_step), _lib.ptr(ws), ws.numel(),
                                  _lib.ptr(flags), _lib.ptr(table), _lib.ptr(counts), _lib.stream_ptr())
    _lib.check(rc, "op_silence_ranges")
    kept, parts = (int(v) for v in counts.cpu().tolist())
    return flags[:windows].cpu().numpy(), table[:parts].cpu().numpy(), kept, parts


def remove_silence_device(wave, sample_rate=target_sample_rate, *, min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10,
                          pcm16=None, want_wave=True, want_rounded=False):
    """``f5_wave_remove_silence`` on a 1-D fp32 / fp64 wave on the GPU -> ``(kept wave, kept rounded PCM, kept pcm16, parts)`` as device tensors
    (None where not asked for).  One small copy (the two counts) comes to the host to size the results; the samples stay on the device."""
    from .. import _lib
    lib = _lib.load()
    assert wave.is_cuda and wave.dim() == 1 and wave.is_contiguous() and wave.dtype in (torch.float32, torch.float64)
    n, dev = wave.numel(), wave.device
    if pcm16 is not None:
        assert pcm16.is_cuda and pcm16.dtype == torch.int16 and pcm16.is_contiguous() and pcm16.numel() == n
    assert want_wave or want_rounded or pcm16 is not None
    if n == 0:  # (nothing to judge: the host functions answer one empty part)
        empty = lambda dtype: torch.empty(0, device=dev, dtype=dtype)  # noqa: E731
        return (empty(wave.dtype) if want_wave else None, empty(torch.int16) if want_rounded else None,
                empty(torch.int16) if pcm16 is not None else None, 1)
    n_ms, _, _ = _silence_windows(n, sample_rate, min_silence_len, seek_step)
    need = lib.f5_wave_remove_silence_workspace(n, int(sample_rate), int(min_silence_len), int(seek_step))
    ws = torch.empty(max(int(need), 16), device=dev, dtype=torch.uint8)
    out = torch.empty(max(n, 1), device=dev, dtype=wave.dtype) if want_wave else None
    rounded = torch.empty(max(n, 1), device=dev, dtype=torch.int16) if want_rounded else None
    kept_pcm = torch.empty(max(n, 1), device=dev, dtype=torch.int16) if pcm16 is not None else None
    counts = torch.zeros(2, device=dev, dtype=torch.int64)
    rc = lib.f5_wave_remove_silence(_lib.ptr(wave) if n else None, int(wave.dtype == torch.float64), n, int(sample_rate), n_ms, int(min_silence_len),
                                    _audio.silence_threshold_floor(silence_thresh), int(keep_silence), int(seek_step),
                                    _lib.ptr(pcm16) if n else None, _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.ptr(rounded),
                                    _lib.ptr(kept_pcm) if n else None, _lib.ptr(counts), _lib.stream_ptr())
    _lib.check(rc, "wave_remove_silence")
    kept, parts = (int(v) for v in counts.cpu().tolist())
    cut = lambda t: t[:kept] if t is not None else None  # noqa: E731
    return cut(out), cut(rounded), cut(kept_pcm), parts


def remove_silence(wave, sample_rate=target_sample_rate, *, min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10, pcm16=None):
    """The kept samples of a finished mono wave: what `remove_silence_for_generated_wav` leaves of the file `audio.write_wav` makes of it, taken
    from the float wave itself (and, with ``pcm16``, from a second array of the same length: the truncating PCM of `finish_waves`).  A tensor on
    the GPU (fp32 / fp64) takes the device route and device tensors come back; a numpy array or CPU tensor takes the host functions, with the same
    result byte for byte.  Returns the kept wave, or ``(kept wave, kept pcm16)`` when ``pcm16`` is given.  NaN samples count as 0."""
    rule = dict(min_silence_len=min_silence_len, silence_thresh=silence_thresh, keep_silence=keep_silence, seek_step=seek_step)
    if torch.is_tensor(wave) and wave.is_cuda:
        flat = wave.reshape(-1).contiguous()
        kept, _, kept_pcm, _ = remove_silence_device(flat, sample_rate, pcm16=pcm16.reshape(-1).contiguous() if pcm16 is not None else None, **rule)
        return kept if pcm16 is None else (kept, kept_pcm)
    as_tensor = torch.is_tensor(wave)
    x = (wave.numpy() if as_tensor else np.asarray(wave)).reshape(-1)
    ranges = _audio.split_sample_ranges(_audio.Segment(rounded_pcm16(x), sample_rate, 2), **rule)
    kept = np.concatenate([x[a:b] for a, b in ranges]) if ranges else x[:0]
    if pcm16 is None:
        return torch.from_numpy(kept) if as_tensor else kept
    p = (pcm16.numpy() if torch.is_tensor(pcm16) else np.asarray(pcm16)).reshape(-1)
    assert len(p) == len(x)
    kept_pcm = np.concatenate([p[a:b] for a, b in ranges]) if ranges else p[:0]
    return (torch.from_numpy(kept), torch.from_numpy(kept_pcm)) if as_tensor else (kept, kept_pcm)


def device_tail_kind(vocoder, *tensors):
    """Which device tail applies to this vocoder object and these mels: "bigvgan" (the HIP BigVGAN: ``T * up`` samples per utterance), "vocos"
    (the HIP Vocos, or an object with its ``decode_ragged_buffer``: ``(T - 1) * hop`` samples) or None (a foreign object at plug point B, or
    tensors that are not on the GPU: the per-utterance host loop).  Both of ours have ``decode_ragged_buffer``: the class tells them apart."""
    if not tensors or not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        return None
    from ..bigvgan import BigVGAN
    if isinstance(vocoder, BigVGAN):
        return "bigvgan"
    return "vocos" if hasattr(vocoder, "decode_ragged_buffer") else None


def mel_rows_of(mels, skip):
    """[1, N_i, mel] sampler outputs -> (rows [R, mel] fp32 contiguous, row_start, frames) with the first ``skip`` frames of each left out by the
    offset (``skip``: one int, or one per utterance -- prompts of several voices).  The ragged sampler hands back views of ONE buffer: that buffer
    is taken as it is (no copy); anything else is concatenated once."""
    mel = mels[0].shape[-1]
    skips = [int(x) for x in skip] if isinstance(skip, (list, tuple)) else [int(skip)] * len(mels)
    assert len(skips) == len(mels)
    frames = [int(m.shape[1]) - k for m, k in zip(mels, skips)]
    st = mels[0].untyped_storage()
    if all(m.dtype == torch.float32 and m.is_contiguous() and m.untyped_storage().data_ptr() == st.data_ptr() and m.storage_offset() % mel == 0
           for m in mels):
        rows = torch.empty(0, dtype=torch.float32, device=mels[0].device).set_(st, 0, (st.nbytes() // (4 * mel), mel), (mel, 1))
        return rows, [m.storage_offset() // mel + k for m, k in zip(mels, skips)], frames
    rows = torch.cat([m[0, k:].to(torch.float32) for m, k in zip(mels, skips)])
    starts, r = [], 0
    for t in frames:
        starts.append(r)
        r += t
    return rows, starts, frames


def decode_utterances(vocoder, kind, rows, row_start, frames):
    """One wave buffer for all utterances (and the sample count of each) from ONE ragged call of either HIP vocoder (``kind`` is
    `device_tail_kind`'s answer: both classes take the same arguments, the sample counts differ)."""
    assert kind in ("vocos", "bigvgan")
    return vocoder.decode_ragged_buffer(rows, row_start, frames)


def waves_of_mels(vocoder, mel_spec_type, mels, skip, cross_fade_duration, sample_rate=target_sample_rate, rms=None, target_rms=target_rms,
                  rms_index=None, want_spec=True, **tail):
    """The mel -> wave stage behind the sampler (`F5TTSWrapper` and `infer_batch_process`): ``(done, waves, spectrograms)``.  With one of the
    HIP vocoders and at least 2 generated frames per utterance, ONE ragged decode of all ``mels`` (the first ``skip`` frames of each left
    out, see `mel_rows_of`) and ONE `finish_waves` (``rms`` / ``rms_index`` in its forms, ``tail``: its other arguments): ``done`` is its
    ``(signal, pcm16)`` on the device and ``waves`` is empty.  Where the library answers F5_ENOTSUP (utterances shorter than their
    cross-fades), and for a foreign vocoder object (per utterance a batch-1 call on the permuted slice), ``done`` is None and ``waves`` holds
    every utterance's wave on the host, the rms rule applied, for `cross_fade_concat`.  ``spectrograms``: [mel, T_i] host arrays (none
    unless ``want_spec``).  Byte-identical results either way (tests/test_gpu_wave_tail.py)."""
    skips = [int(x) for x in skip] if isinstance(skip, (list, tuple)) else [int(skip)] * len(mels)

    def gained(wave, i):  # the rms rule of the reference's loop (:491-492), for utterance i
        r = None if rms is None else rms[rms_index[i]] if rms_index is not None else rms[i] if isinstance(rms, (list, tuple)) else rms
        return wave * r / target_rms if r is not None and r < target_rms else wave

    waves, spectrograms = [], []
    kind = device_tail_kind(vocoder, *mels)
    if kind is not None and (kind == "vocos") == (mel_spec_type == "vocos") and min(int(m.shape[1]) - k for m, k in zip(mels, skips)) >= 2:
        rows, row_start, frames = mel_rows_of(mels, skips)
        wave_buf, samples = decode_utterances(vocoder, kind, rows, row_start, frames)
        done = finish_waves(wave_buf, samples, cross_fade_duration, sample_rate, rms=rms, target_rms=target_rms, rms_index=rms_index, **tail)
        if want_spec:
            spectrograms = [rows[r: r + t].t().cpu().numpy() for r, t in zip(row_start, frames)]
        if done is None:
            waves = [gained(w, i).cpu().numpy() for i, w in enumerate(torch.split(wave_buf, samples))]
        return done, waves, spectrograms
    for i, (generated, k) in enumerate(zip(mels, skips)):
        generated = generated.to(torch.float32)[:, k:, :].permute(0, 2, 1)
        generated_wave = vocoder.decode(generated) if mel_spec_type == "vocos" else vocoder(generated)  # reference :485-488
        waves.append(gained(generated_wave, i).squeeze().cpu().numpy())
        if want_spec:
            spectrograms.append(generated[0].cpu().numpy())
    return None, waves, spectrograms


def infer_process(ref_audio, ref_text, gen_text, model_obj, vocoder, mel_spec_type=mel_spec_type, show_info=print, progress=None,
                  target_rms=target_rms, cross_fade_duration=cross_fade_duration, nfe_step=nfe_step, cfg_strength=cfg_strength,
                  sway_sampling_coef=sway_sampling_coef, speed=speed, fix_duration=fix_duration, device=device):
    audio, sr = _load_audio(ref_audio)
    max_chars = int(len(ref_text.encode("utf-8")) / (audio.shape[-1] / sr) * (22 - audio.shape[-1] / sr))
    gen_text_batches = chunk_text(gen_text, max_chars=max_chars)
    for i, t in enumerate(gen_text_batches):
        print(f"gen_text {i}", t)
    print("\n")
    show_info(f"Generating audio in {len(gen_text_batches)} batches...")
    return next(infer_batch_process((audio, sr), ref_text, gen_text_batches, model_obj, vocoder, mel_spec_type=mel_spec_type,
                                    progress=progress, target_rms=target_rms, cross_fade_duration=cross_fade_duration,
                                    nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, speed=speed,
                                    fix_duration=fix_duration, device=device))


def infer_batch_process(ref_audio, ref_text, gen_text_batches, model_obj, vocoder, mel_spec_type="vocos", progress=None, target_rms=0.1,
                        cross_fade_duration=0.15, nfe_step=32, cfg_strength=2.0, sway_sampling_coef=-1, speed=1, fix_duration=None,
                        device=None, streaming=False, chunk_size=2048):
    audio, sr = ref_audio
    if audio.shape[0] > 1:
        audio = torch.mean(audio, dim=0, keepdim=True)
    rms = torch.sqrt(torch.mean(torch.square(audio)))  # the ORIGINAL (pre-boost) rms scales the output back (reference :440-442,491-492)
    if rms < target_rms:
        audio = audio * target_rms / rms
    audio = audio.to(device)
    if sr != target_sample_rate:
        audio = _audio.resample(audio, sr, target_sample_rate)  # on the device (f5_frontend_resample)
    if len(ref_text[-1].encode("utf-8")) == 1:
        ref_text = ref_text + " "

    ref_audio_len = audio.shape[-1] // hop_length

    def plan_batch(gen_text):  # host side of one text batch: tokens and the frame budget (reference :455-470)
        local_speed = 0.3 if len(gen_text.encode("utf-8")) < 10 else speed
        final_text_list = convert_char_to_pinyin([ref_text + gen_text])
        if fix_duration is not None:
            duration = int(fix_duration * target_sample_rate / hop_length)
        else:
            ref_text_len, gen_text_len = len(ref_text.encode("utf-8")), len(gen_text.encode("utf-8"))
            duration = ref_audio_len + int(ref_audio_len / ref_text_len * gen_text_len / local_speed)
        return final_text_list, duration

    def finish_batch(generated):  # mel -> wave (reference :481-497)
        generated = generated.to(torch.float32)[:, ref_audio_len:, :].permute(0, 2, 1)
        generated_wave = vocoder.decode(generated) if mel_spec_type == "vocos" else vocoder(generated)  # reference :485-488
        if rms < target_rms:
            generated_wave = generated_wave * rms / target_rms
        return generated_wave.squeeze().cpu().numpy(), generated[0].cpu().numpy()

    def process_batch(gen_text):
        final_text_list, duration = plan_batch(gen_text)
        with torch.inference_mode():
            generated, _ = model_obj.sample(cond=audio, text=final_text_list, duration=duration, steps=nfe_step, cfg_strength=cfg_strength,
                                            sway_sampling_coef=sway_sampling_coef, return_trajectory=False)
            generated_wave, mel = finish_batch(generated)
            if streaming:
                for j in range(0, len(generated_wave), chunk_size):
                    yield generated_wave[j: j + chunk_size], target_sample_rate
            else:
                yield generated_wave, mel

    batches = progress.tqdm(gen_text_batches) if progress is not None else gen_text_batches
    if streaming:
        for gen_text in batches:
            for chunk in process_batch(gen_text):
                yield chunk
        return
    mels = []
    # Several text batches, each long enough for the tuned kernels: ONE ragged batch per group (F5TTSWrapper.generate does the same; every
    # utterance keeps the arithmetic -- and the noise draw order -- of its own batch-1 sample() call, so the audio is bit-identical).
    transformer = getattr(model_obj, "transformer", None)
    jobs = [plan_batch(t) for t in gen_text_batches]
    group_max = int(os.environ.get("F5HIP_RAGGED_CHUNKS", "8"))
    if (group_max >= 2 and len(jobs) >= 2 and hasattr(model_obj, "sample_ragged") and hasattr(transformer, "native_sample_ragged")
            and getattr(transformer, "BACKBONE", None) == 0 and min(d for _, d in jobs) >= 256 and max(d for _, d in jobs) <= 4096):
        with torch.inference_mode():
            for idx in chunk_groups([d for _, d in jobs], 0, group_max):
                mels += model_obj.sample_ragged(audio, [jobs[i][0][0] for i in idx], [jobs[i][1] for i in idx], steps=nfe_step,
                                                cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef)
        batches = []
    for gen_text in batches:  # the reference's thread pool resolves to serial generators on the caller thread
        final_text_list, duration = plan_batch(gen_text)
        with torch.inference_mode():
            generated, _ = model_obj.sample(cond=audio, text=final_text_list, duration=duration, steps=nfe_step, cfg_strength=cfg_strength,
                                            sway_sampling_coef=sway_sampling_coef, return_trajectory=False)
        mels.append(generated)
    with torch.inference_mode():  # (the host-side pre-boost rms: the decision `rms < target_rms` is taken as the reference's loop takes it)
        done, generated_waves, spectrograms = waves_of_mels(vocoder, mel_spec_type, mels, ref_audio_len, cross_fade_duration, rms=rms,
                                                            target_rms=target_rms)
    if done is not None:
        yield done[0].cpu().numpy(), target_sample_rate, np.concatenate(spectrograms, axis=1)
    elif generated_waves:
        yield cross_fade_concat(generated_waves, cross_fade_duration), target_sample_rate, np.concatenate(spectrograms, axis=1)
    else:
        yield None, target_sample_rate, None
