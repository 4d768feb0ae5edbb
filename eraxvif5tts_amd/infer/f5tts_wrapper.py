"""F5TTSWrapper: preprocess one reference voice once, synthesize many texts -- the reference's inference facade
(``f5_tts/infer/f5tts_wrapper.py:28-621``) over the MI355X HIP backbone, sampler and vocoder.

Same constructor kwargs/defaults (:34-52), ``preprocess_reference(ref_audio_path, ref_text, clip_short)`` (:256-354),
``generate(text, output_path, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration,
use_duration_predictor, return_numpy, return_spectrogram)`` (:408-607), ``get_current_audio_length`` (:618-621), the same
stored fields, error types and the three return shapes.

Provenance of this file: the host-side control flow of ``generate()`` / ``preprocess_reference()`` is a condensed restatement of the
reference's, statement for statement where its behaviour is observable (local names, the duration rule, the progress prints, the rms and
cross-fade arithmetic) -- the north star asks for an identical API and identical host behaviour, and these lines have one spelling.  Nothing
the reference computes on the model path is reused: the backbone, sampler, vocoder, mel and resampling all run in libf5hip.

Differences forced by the offline, ROCm-only image (each raises instead of silently approximating):
  * no Whisper ASR is initialised (reference :100 downloads openai/whisper-large-v3-turbo): ``ref_text`` must be given;
  * checkpoints and the Vocos weights must be local files (reference :125 / utils_infer.py:110-112 fetch from the hub);
  * ``device`` must be a ROCm GPU: the backbone has no CPU path.
The optional conv duration predictor (:381-406) runs on the HIP path (``model/duration_predictor.py`` over ``f5_duration_predict``)
when the loaded model carries one; otherwise the reference's own fallback branch is taken (:166-168).
"""
from __future__ import annotations

import contextlib
import os
import re
import types
from typing import Optional

import numpy as np
import torch
import yaml

from ..model import CFM
from ..model import backbones as _backbones
from ..model.utils import convert_char_to_pinyin, get_tokenizer, list_str_to_idx
from . import audio as _audio
from .utils_infer import (DEFAULT_VOCAB, WaveStream, chunk_groups, chunk_text, cross_fade_concat, decode_utterances, device_tail_kind, finish_waves,
                          load_checkpoint, load_vocoder, mel_rows_of, split_voice_script)

_CONFIG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")


class F5TTSWrapper:
    """A wrapper class for F5-TTS that preprocesses reference audio once and allows for repeated TTS generation.

    ``ode_method`` is the fixed-grid solver of the sampler: "euler", "midpoint", "rk4", "heun2" or "heun3" (1 / 2 / 4 / 2 / 3 network
    evaluations per step of ``nfe_step``)."""

    def __init__(self, model_name: str = "F5TTS_v1_Base", ckpt_path: Optional[str] = None, vocab_file: Optional[str] = None,
                 vocoder_name: str = "vocos", use_local_vocoder: bool = False, vocoder_path: Optional[str] = None,
                 device: Optional[str] = None, hf_cache_dir: Optional[str] = None, target_sample_rate: int = 24000,
                 n_mel_channels: int = 100, hop_length: int = 256, win_length: int = 1024, n_fft: int = 1024,
                 ode_method: str = "euler", use_ema: bool = True, use_duration_predictor: bool = False,
                 vocoder=None, precision: Optional[str] = None, attn_dropout: Optional[float] = None):
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = device
        self.target_sample_rate, self.n_mel_channels = target_sample_rate, n_mel_channels
        self.hop_length, self.win_length, self.n_fft = hop_length, win_length, n_fft
        self.mel_spec_type = vocoder_name
        self.ode_method = ode_method
        self.use_duration_predictor = use_duration_predictor

        # model configuration: a bundled config name, or (reference :128-131) a YAML path when "custom" is in the name
        config_path = os.path.join(_CONFIG_DIR, f"{model_name}.yaml") if "custom" not in model_name.lower() else model_name
        with open(config_path, "r") as f:
            model_cfg = yaml.safe_load(f)
        model_cls = getattr(_backbones, model_cfg["model"]["backbone"], None)  # plug point A (reference :134)
        if model_cls is None:
            raise NotImplementedError(f"backbone {model_cfg['model']['backbone']} is not on the MI355X path (DiT, UNetT and MMDiT are)")
        model_arc = dict(model_cfg["model"]["arch"])
        if precision is not None:
            model_arc["precision"] = precision

        if vocab_file is None:
            vocab_file = DEFAULT_VOCAB
        self.vocab_char_map, vocab_size = get_tokenizer(vocab_file, "custom")

        self.model = CFM(
            transformer=model_cls(**model_arc, text_num_embeds=vocab_size, mel_dim=n_mel_channels),
            mel_spec_kwargs=dict(n_fft=n_fft, hop_length=hop_length, win_length=win_length, n_mel_channels=n_mel_channels,
                                 target_sample_rate=target_sample_rate, mel_spec_type=vocoder_name),
            odeint_kwargs=dict(method=ode_method),
            vocab_char_map=self.vocab_char_map,
        ).to(self.device)

        if ckpt_path is None:
            raise FileNotFoundError("ckpt_path is required: the reference's default (hf://SWivid/F5-TTS/...) is a network download")
        self._load_checkpoint(self.model, ckpt_path, use_ema=use_ema)

        self.has_duration_predictor = hasattr(self.model, "duration_predictor") and self.model.duration_predictor is not None
        if self.use_duration_predictor and not self.has_duration_predictor:
            print("Warning: Duration predictor requested but not found in model. Using fallback duration calculation.")
            self.use_duration_predictor = False
        elif self.has_duration_predictor:
            print("Duration predictor found in model.")

        if vocoder is not None:  # plug point B: any object with .decode(mel[b, 100, T])
            self.vocoder = vocoder
        else:
            if vocoder_path is None:
                vocoder_path = "../checkpoints/vocos-mel-24khz"
            self.vocoder = load_vocoder(vocoder_name=vocoder_name, is_local=use_local_vocoder, local_path=vocoder_path,
                                        device=self.device, hf_cache_dir=hf_cache_dir)

        self.ref_audio_processed = None
        self.ref_text = None
        self.ref_audio_len = None
        self._voices = {}  # add_voice(): name -> the fields of one more reference voice ("main" is the three fields above)
        self.target_rms = 0.1
        self.cross_fade_duration = 0.15
        # text chunks of one generate() call sampled concurrently (HIP streams); 1 = one after the other as the reference does.  Not a
        # constructor argument (the reference's signature is kept); set the attribute or F5HIP_CHUNK_STREAMS
        self.chunk_streams = int(os.environ.get("F5HIP_CHUNK_STREAMS", "4"))
        # text chunks of one generate() call sampled as ONE ragged batch (libf5hip f5_sample_ragged): up to this many utterances per launch set
        # (0 = off: chunks run one per stream as above).  Applies when every chunk has at least 256 frames (the row count from which a batch-1
        # call takes the tuned kernels too, so both paths compute bit-identical mels).
        self.ragged_chunks = int(os.environ.get("F5HIP_RAGGED_CHUNKS", "8"))
        # generate_stream(): the first `stream_first_chunks` text chunks form the first piece (1: the first audio waits for one utterance only);
        # the rest follows in groups of up to `ragged_chunks`.  Not a constructor argument either; set the attribute or F5HIP_STREAM_FIRST
        self.stream_first_chunks = int(os.environ.get("F5HIP_STREAM_FIRST", "1"))
        # "cpu": draw every chunk's initial noise from torch's CPU generator, in chunk order -- the numbers the reference's CPU path draws after
        # the same torch.manual_seed (reference model/cfm.py:178-183 with device = cpu); None = on the GPU, as the reference's GPU path does
        self.model.noise_device = os.environ.get("F5HIP_NOISE_DEVICE") or None
        # attention dropout, opt-in (DiT.set_attn_dropout): the reference's attention keeps dropout_p = 0.1 live at inference (modules.py:490);
        # attn_dropout=0.1 / F5HIP_ATTN_DROPOUT=0.1 runs this side the same way (own mask stream: equal in distribution, not bit for bit)
        if attn_dropout is None and os.environ.get("F5HIP_ATTN_DROPOUT"):
            attn_dropout = float(os.environ["F5HIP_ATTN_DROPOUT"])
        if attn_dropout:
            self.model.transformer.set_attn_dropout(attn_dropout)
        self.nfe_step = 32
        self.cfg_strength = 2.0
        self.sway_sampling_coef = -1.0
        self.speed = 1.0
        self.fix_duration = None

    def _load_checkpoint(self, model, ckpt_path, dtype=None, use_ema=True):
        return load_checkpoint(model, ckpt_path, self.device, dtype=dtype, use_ema=use_ema)

    # ------------------------------------------------------------------ reference voice
    def preprocess_reference(self, ref_audio_path: str, ref_text: str = "", clip_short: bool = True):
        audio, ref_text = self._preprocess_voice(ref_audio_path, ref_text, clip_short)
        self.ref_audio_processed = audio
        self.ref_text = ref_text
        self.ref_audio_len = audio.shape[-1] // self.hop_length
        return audio, ref_text

    def _preprocess_voice(self, ref_audio_path, ref_text, clip_short):
        """The steps of preprocess_reference() / add_voice(): ``(audio on the device, ref_text as it is used)``."""
        print("Converting audio...")
        aseg = _audio.Segment.from_file(ref_audio_path)
        if clip_short:
            aseg = _audio.clip_reference(aseg)
        aseg = self._remove_silence_edges(aseg)
        aseg = aseg + aseg.silent_like(50)
        if not ref_text.strip():
            raise RuntimeError("No reference text provided: automatic transcription (Whisper) needs a network model download; pass ref_text")
        print("Using custom reference text...")
        if not ref_text.endswith(". ") and not ref_text.endswith("。"):
            ref_text += " " if ref_text.endswith(".") else ". "
        print("\nReference text:", ref_text)

        audio, sr = _audio.segment_to_float(aseg), aseg.frame_rate
        if audio.shape[0] > 1:
            audio = torch.mean(audio, dim=0, keepdim=True)
        rms = torch.sqrt(torch.mean(torch.square(audio)))
        if rms < self.target_rms:  # boosted only when quieter than the target (reference :334-336)
            audio = audio * self.target_rms / rms
        audio = audio.to(self.device)
        if sr != self.target_sample_rate:
            audio = _audio.resample(audio, sr, self.target_sample_rate)  # on the device (f5_frontend_resample)
        return audio, ref_text

    # ------------------------------------------------------------------ further voices (generate_multi)
    def add_voice(self, name: str, ref_audio_path: str, ref_text: str = "", clip_short: bool = True):
        """One more reference voice for `generate_multi`, under ``name`` (a ``\\w+`` word other than "main", which is the voice
        `preprocess_reference` stored): exactly the steps of `preprocess_reference`, with the prompt's mel and its rms computed once.  The main
        fields are not touched.  Returns ``(audio, ref_text)`` as `preprocess_reference` does."""
        if not isinstance(name, str) or not re.fullmatch(r"\w+", name) or name == "main":
            raise ValueError(f"voice name {name!r}: a name is one \\w+ word (what a [name] tag can hold) and \"main\" is the voice of preprocess_reference()")
        audio, ref_text = self._preprocess_voice(ref_audio_path, ref_text, clip_short)
        self._voices[name] = self._voice_fields(audio, ref_text)
        return audio, ref_text

    def remove_voice(self, name: str):
        if name == "main":
            raise ValueError("\"main\" is the voice of preprocess_reference(): store another one with it")
        del self._voices[name]

    def _voice_fields(self, audio, ref_text):
        with torch.inference_mode():
            mel = self.model.mel_spec(audio).permute(0, 2, 1)  # what sample() makes of the raw prompt, once
            rms = torch.sqrt(torch.mean(torch.square(audio))).to(torch.float32)  # of the stored, already boosted prompt (:529-531)
        return dict(audio=audio, ref_text=ref_text, ref_audio_len=audio.shape[-1] // self.hop_length, mel=mel, rms=rms)

    def _main_voice(self):
        if self.ref_audio_processed is None or self.ref_text is None:
            return None
        cached = getattr(self, "_main_voice_cache", None)
        if (cached is None or cached["audio"] is not self.ref_audio_processed or cached["ref_text"] != self.ref_text
                or cached["ref_audio_len"] != self.ref_audio_len):  # (the main fields are public: a caller may have installed another prompt)
            cached = self._voice_fields(self.ref_audio_processed, self.ref_text)
            cached["ref_audio_len"] = self.ref_audio_len
            self._main_voice_cache = cached
        return cached

    @property
    def voices(self):
        """Read-only view: name -> fields (``audio``, ``ref_text``, ``ref_audio_len``, ``mel``, ``rms``) of every stored voice, "main" included
        once `preprocess_reference` has run."""
        main = self._main_voice()
        return types.MappingProxyType({**({"main": main} if main is not None else {}), **self._voices})

    @contextlib.contextmanager
    def _voice_installed(self, voice):
        """The main fields hold ``voice``'s inside the block (the planning of generate() reads them) and are put back behind it."""
        kept = self.ref_audio_processed, self.ref_text, self.ref_audio_len
        self.ref_audio_processed, self.ref_text, self.ref_audio_len = voice["audio"], voice["ref_text"], voice["ref_audio_len"]
        try:
            yield
        finally:
            self.ref_audio_processed, self.ref_text, self.ref_audio_len = kept

    def _remove_silence_edges(self, audio, silence_threshold=-42):
        return _audio.remove_silence_edges(audio, silence_threshold)

    def calculate_duration_with_predictor(self, text_tokens, text_lengths, local_speed=1.0):
        """Reference :381-406, op for op: token mask from the lengths, ``model.duration_predictor(tokens, mask)`` -> [b, 1, nt]
        log-durations, ``exp(...).squeeze(-1).sum(dim=1)`` and ``durations[0].item()``.  (As in the reference the reduction runs
        over the singleton channel axis, so ``.item()`` only succeeds for a one-token text; the quirk is kept, not repaired.)"""
        b, nt = text_tokens.shape
        range_tensor = torch.arange(nt, device=self.device).unsqueeze(0)
        text_tokens_mask = (range_tensor < text_lengths.unsqueeze(1)).int()
        with torch.inference_mode():
            log_durations = self.model.duration_predictor(text_tokens, text_tokens_mask)
            durations = torch.exp(log_durations).squeeze(-1).sum(dim=1)
        return self.ref_audio_len + int(durations[0].item() / local_speed)

    # ------------------------------------------------------------------ synthesis
    def generate(self, text: str, output_path: Optional[str] = None, nfe_step: Optional[int] = None, cfg_strength: Optional[float] = None,
                 sway_sampling_coef: Optional[float] = None, speed: Optional[float] = None, fix_duration: Optional[float] = None,
                 cross_fade_duration: Optional[float] = None, use_duration_predictor: Optional[bool] = None,
                 return_numpy: bool = False, return_spectrogram: bool = False, return_pcm16: bool = False, remove_silence: bool = False):
        """``return_pcm16``: the wave comes back as the int16 PCM the streaming server sends (``streaming.wire.pcm16_bytes`` of the float
        result, bit for bit), converted on the device where the device tail runs -- one int16 copy instead of a float copy and a host pass.
        ``remove_silence``: the reference's option (infer_cli --remove_silence, api.py) -- the written file is byte for byte the file without
        the option after `utils_infer.remove_silence_for_generated_wav`; the returned wave (float, or the truncating PCM with
        ``return_pcm16``) holds the same kept samples, and the spectrogram is untouched.  Where the device tail runs the decision is taken
        there (`utils_infer.remove_silence`) and only the kept samples are copied; an all-silent result is empty."""
        (nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration), jobs = self._plan_jobs(
            text, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor)
        return self._generate_jobs(jobs, output_path, nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration, return_numpy,
                                   return_spectrogram, return_pcm16, remove_silence)

    def _plan_jobs(self, text, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor):
        """The host work of generate() / generate_stream() before any sampling: the arguments' defaults, the text cut into chunks, and per chunk
        the token list and the frames asked for (duration rule or predictor) -- the ``jobs`` list."""
        if self.ref_audio_processed is None or self.ref_text is None:
            raise ValueError("Reference audio not preprocessed. Call preprocess_reference() first.")
        nfe_step = nfe_step if nfe_step is not None else self.nfe_step
        cfg_strength = cfg_strength if cfg_strength is not None else self.cfg_strength
        sway_sampling_coef = sway_sampling_coef if sway_sampling_coef is not None else self.sway_sampling_coef
        speed = speed if speed is not None else self.speed
        fix_duration = fix_duration if fix_duration is not None else self.fix_duration
        cross_fade_duration = cross_fade_duration if cross_fade_duration is not None else self.cross_fade_duration
        use_predictor = use_duration_predictor if use_duration_predictor is not None else self.use_duration_predictor
        can_use_predictor = use_predictor and self.has_duration_predictor

        audio_len = self.ref_audio_processed.shape[-1] / self.target_sample_rate
        max_chars = int(len(self.ref_text.encode("utf-8")) / audio_len * (22 - audio_len))
        text_batches = chunk_text(text, max_chars=max_chars)
        for i, text_batch in enumerate(text_batches):
            print(f"Text batch {i}: {text_batch}")
        print("\n")

        jobs = []  # (token list, frames asked for) per chunk -- host work of the reference's loop (:476-510), before any sampling
        for i, text_batch in enumerate(text_batches):
            local_speed = 0.3 if len(text_batch.encode("utf-8")) < 10 else speed
            final_text_list = convert_char_to_pinyin([self.ref_text + text_batch])
            if fix_duration is not None:
                duration = int(fix_duration * self.target_sample_rate / self.hop_length)
                print(f"Using fixed duration: {fix_duration}s ({duration} frames)")
            elif can_use_predictor:
                if isinstance(final_text_list[0], str):
                    text_tokens = list_str_to_idx(final_text_list, self.vocab_char_map).to(self.device)
                else:
                    text_tokens = torch.tensor(final_text_list, device=self.device)
                text_lengths = torch.tensor([len(t) for t in final_text_list], device=self.device)
                duration = self.calculate_duration_with_predictor(text_tokens, text_lengths, local_speed)
                print(f"Duration predictor output: {duration} frames")
            else:
                ref_text_len, gen_text_len = len(self.ref_text.encode("utf-8")), len(text_batch.encode("utf-8"))
                duration = self.ref_audio_len + int(self.ref_audio_len / ref_text_len * gen_text_len / local_speed)
                print(f"Calculated duration based on text ratio: {duration} frames")
            jobs.append((final_text_list, int(duration)))
        return (nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration), jobs

    def _sample_jobs(self, jobs, nfe_step, cfg_strength, sway_sampling_coef, voices=None):
        """The mels of these jobs, in order, by the sampler their list calls for: ragged when the backbone is the DiT and there are at least 2 jobs,
        all of at least 256 and at most 4096 frames; otherwise sample() per job, up to `chunk_streams` of them in flight.  ``voices`` (one field
        dict per job, generate_multi): every job takes its own voice's prompt mel -- in a ragged call one prompt per utterance, zero-padded
        to the longest, with ``lens``; None: the main prompt for all."""
        transformer = getattr(self.model, "transformer", None)
        # The text chunks of one call are independent (the reference samples them one after the other, :476-533).  Here up to `chunk_streams`
        # of them are in flight at once, each on a HIP stream (and a libf5hip plan) of its own: a single-utterance sample() fills a fraction
        # of the 256 CUs, so the streams overlap.  Every chunk runs exactly the launches of the serial path -- same shapes, same kernels --
        # so its mel is bit-identical to the serial result; noise is drawn in chunk order either way.
        # Several chunks, each long enough for the tuned kernels: ONE ragged batch per group of chunks -- the utterances concatenated along the
        # token axis, no padding to a common length, every chunk with the arithmetic of its own batch-1 call (bit-identical mels, same noise
        # order).  A single-utterance sample() fills a fraction of the 256 CUs; the concatenation fills them.
        ragged = (int(self.ragged_chunks) >= 2 and len(jobs) >= 2 and torch.cuda.is_available() and hasattr(transformer, "native_sample_ragged")
                  and getattr(transformer, "BACKBONE", None) == 0 and min(d for _, d in jobs) >= 256 and max(d for _, d in jobs) <= 4096)
        n_streams = 1
        if not ragged and torch.cuda.is_available() and hasattr(transformer, "finish_pending"):
            n_streams = max(1, min(len(jobs), int(self.chunk_streams)))
        main = torch.cuda.current_stream() if n_streams > 1 else None
        streams = self._chunk_stream_pool(n_streams) if n_streams > 1 else []
        for st in streams:
            st.wait_stream(main)  # the preprocessed prompt was produced on the caller's stream
        mels = []
        if ragged:
            with torch.inference_mode():
                for idx in chunk_groups([d for _, d in jobs], 0, int(self.ragged_chunks)):
                    group = [jobs[i] for i in idx]
                    cond, lens = self.ref_audio_processed, None
                    if voices is not None:
                        prompts = [voices[i]["mel"][0] for i in idx]
                        lens = torch.tensor([int(m.shape[0]) for m in prompts], device=prompts[0].device, dtype=torch.long)
                        cond = torch.nn.utils.rnn.pad_sequence(prompts, batch_first=True, padding_value=0.0)
                    mels += self.model.sample_ragged(cond, [j[0][0] for j in group], [j[1] for j in group], lens=lens, steps=nfe_step,
                                                     cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef)
        for i, (final_text_list, duration) in enumerate(jobs if not ragged else []):
            prompt = self.ref_audio_processed if voices is None else voices[i]["mel"]
            with torch.inference_mode():
                if n_streams > 1:
                    with torch.cuda.stream(streams[i % n_streams]):
                        generated, _ = self.model.sample(cond=prompt, text=final_text_list, duration=duration, steps=nfe_step,
                                                         cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, return_trajectory=False,
                                                         defer_guard=True)
                else:
                    generated, _ = self.model.sample(cond=prompt, text=final_text_list, duration=duration, steps=nfe_step,
                                                     cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, return_trajectory=False)
                mels.append(generated)
        if n_streams > 1:
            transformer.finish_pending()  # reads every chunk's fp16 range-guard flag (and lets the library redo a chunk whose guard fired)
            # finish_pending() synchronises a stream only when its plan has a guard to read (bf16 mode with fp16 storage); the vocoder below runs
            # on the caller's stream, so that stream must be ordered behind EVERY chunk stream whatever the precision (round 4: the fp32 mode
            # decoded mels that were still being written -- found by test_generate_end_to_end_matches_the_oracle_chain[fp32-False])
            for st in streams:
                main.wait_stream(st)
            with torch.inference_mode():
                for generated in mels:
                    generated.record_stream(main)
        return mels

    def _silence_step(self, signal, pcm16=None):
        """The step behind the tail when ``remove_silence`` is on: ``(kept signal, kept pcm16 or None)`` at the reference's four values
        (`utils_infer.SILENCE_DEFAULTS`), on the device for device tensors (the `finish_waves` outputs), by the host functions for arrays."""
        from .utils_infer import SILENCE_DEFAULTS, remove_silence
        kept = remove_silence(signal, self.target_sample_rate, pcm16=pcm16, **SILENCE_DEFAULTS)
        return kept if pcm16 is not None else (kept, None)

    def _generate_jobs(self, jobs, output_path, nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration, return_numpy, return_spectrogram,
                       return_pcm16, remove_silence=False):
        generated_waves, spectrograms = [], []
        mels = self._sample_jobs(jobs, nfe_step, cfg_strength, sway_sampling_coef)
        want_spec = return_spectrogram or output_path is not None
        want_float = not return_pcm16 or output_path is not None
        final_wave = final_pcm = None
        with torch.inference_mode():
            # The tail on the device where the vocoder is one of ours: the mels of all chunks go to ONE ragged vocoder call (the prompt frames
            # skipped by a row offset, no permute copy), then one wave_finish (rms rule decided on the device from the device-resident prompt,
            # cross-fade, PCM) and one copy to the host.  Byte-identical to the per-chunk loop below, which foreign vocoder objects keep.
            kind = device_tail_kind(self.vocoder, self.ref_audio_processed, *mels)
            if kind is not None and (kind == self.mel_spec_type) and mels and min(int(m.shape[1]) for m in mels) - self.ref_audio_len >= 2:
                rows, row_start, frames = mel_rows_of(mels, self.ref_audio_len)
                wave_buf, samples = decode_utterances(self.vocoder, kind, rows, row_start, frames)
                rms = torch.sqrt(torch.mean(torch.square(self.ref_audio_processed)))  # of the stored, already boosted prompt (:529-531)
                done = finish_waves(wave_buf, samples, cross_fade_duration, self.target_sample_rate, rms=rms.to(torch.float32), target_rms=self.target_rms,
                                    want_float=want_float or remove_silence, want_pcm16=return_pcm16)  # (the float wave is what is judged)
                if want_spec:
                    spectrograms = [rows[r: r + t].t().cpu().numpy() for r, t in zip(row_start, frames)]
                if done is not None:
                    if remove_silence:
                        done, remove_silence = self._silence_step(*done), False
                    final_wave = done[0].cpu().numpy() if want_float else None
                    final_pcm = done[1].cpu().numpy() if return_pcm16 else None
                else:  # utterances shorter than their cross-fades (F5_ENOTSUP): the decoded waves take the host functions
                    apply_gain = bool(rms < self.target_rms)
                    for w in torch.split(wave_buf, samples):
                        generated_waves.append((w * rms / self.target_rms if apply_gain else w).cpu().numpy())
            else:
                for generated in mels:
                    generated = generated.to(torch.float32)[:, self.ref_audio_len:, :].permute(0, 2, 1)
                    if self.mel_spec_type == "vocos":
                        generated_wave = self.vocoder.decode(generated)
                    elif self.mel_spec_type == "bigvgan":
                        generated_wave = self.vocoder(generated)
                    rms = torch.sqrt(torch.mean(torch.square(self.ref_audio_processed)))  # of the stored, already boosted prompt (:529-531)
                    if rms < self.target_rms:
                        generated_wave = generated_wave * rms / self.target_rms
                    generated_waves.append(generated_wave.squeeze().cpu().numpy())
                    if want_spec:
                        spectrograms.append(generated.squeeze().cpu().numpy())

        if final_wave is None and final_pcm is None:
            if not generated_waves:
                raise RuntimeError("No audio generated")
            final_wave = cross_fade_concat(generated_waves, cross_fade_duration, self.target_sample_rate)
        if return_pcm16 and final_pcm is None:
            from ..streaming.wire import pcm16_bytes
            final_pcm = np.frombuffer(pcm16_bytes(final_wave), dtype=np.int16)
        if remove_silence:  # the host tails (a foreign vocoder, or joints that chain): the same rule by the host functions
            final_wave, final_pcm = self._silence_step(final_wave, final_pcm)
        combined_spectrogram = np.concatenate(spectrograms, axis=1) if spectrograms else None
        if output_path is not None:
            output_dir = os.path.dirname(output_path)
            if output_dir and not os.path.exists(output_dir):
                os.makedirs(output_dir)
            _audio.write_wav(output_path, final_wave, self.target_sample_rate)
            if return_spectrogram:
                np.save(os.path.splitext(output_path)[0] + "_spec.npy", combined_spectrogram)  # matplotlib is not in the image
            if not return_numpy:
                return output_path
        if return_pcm16:
            final_wave = final_pcm
        if return_spectrogram:
            return final_wave, self.target_sample_rate, combined_spectrogram
        return final_wave, self.target_sample_rate

    def generate_stream(self, text: str, nfe_step: Optional[int] = None, cfg_strength: Optional[float] = None,
                        sway_sampling_coef: Optional[float] = None, speed: Optional[float] = None, fix_duration: Optional[float] = None,
                        cross_fade_duration: Optional[float] = None, use_duration_predictor: Optional[bool] = None,
                        return_numpy: bool = True, return_spectrogram: bool = False, return_pcm16: bool = False):
        """generate() as a generator of ``(piece, sample_rate)``: the audio of each group of text chunks as soon as it is final, cross-fades
        included.  The pieces, concatenated, are byte for byte what ``generate()`` returns for the same arguments after the same
        ``torch.manual_seed`` (float of the same dtype -- float64 in EVERY piece when chunks are cross-faded -- or int16 with ``return_pcm16``).
        The first ``stream_first_chunks`` chunks form the first piece, the rest follows in groups of up to ``ragged_chunks`` chunks and 16384
        frames (`utils_infer.chunk_groups`); per group one sampler call, one ragged vocoder call, one push into the wave tail's stream session
        (``f5_wave_stream_push``: the joint's left side is carried from the previous group) and one copy to the host.  Nothing of group g + 1
        starts before group g has been handed out.

        The streamed tail applies when the vocoder is one of the HIP vocoders, the prompt is on the GPU, every chunk has at least 2 generated
        frames and no cross-fade reaches into another (`plan_wave_tail`'s ``device_ok``); this is decided before any sampling, and otherwise
        the generator yields exactly once, with what ``generate()`` returns.  With attention dropout on, a ragged sampler call does not promise
        the bits of its batch-1 calls, so the byte-equality with ``generate()`` holds for dropout off only.  ``return_numpy`` and
        ``return_spectrogram`` are accepted for the signature's sake: a piece is always an array, and no spectrogram is streamed.  Closing the
        generator early frees the session and leaves the wrapper as it was."""
        (nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration), jobs = self._plan_jobs(
            text, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor)
        frames = self._generated_frames(jobs)
        kind = device_tail_kind(self.vocoder, self.ref_audio_processed)
        session = None
        if kind is not None and kind == self.mel_spec_type and frames and min(frames) >= 2:
            samples = [(t - 1) * self.hop_length for t in frames] if kind == "vocos" else [t * self.vocoder._total_up() for t in frames]
            with torch.inference_mode():
                rms = torch.sqrt(torch.mean(torch.square(self.ref_audio_processed)))  # of the stored, already boosted prompt (:529-531)
                session = WaveStream(samples, cross_fade_duration, self.target_sample_rate, rms=rms.to(torch.float32), target_rms=self.target_rms,
                                     want_float=not return_pcm16, want_pcm16=return_pcm16)
        if session is None or not session.ok:
            wave, rate = self._generate_jobs(jobs, None, nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration, True, False, return_pcm16)
            yield wave, rate
            return
        try:
            first = 0
            for group in chunk_groups([d for _, d in jobs], int(self.stream_first_chunks), int(self.ragged_chunks)):
                mels = self._sample_jobs([jobs[i] for i in group], nfe_step, cfg_strength, sway_sampling_coef)
                with torch.inference_mode():
                    rows, row_start, got = mel_rows_of(mels, self.ref_audio_len)
                    if got != frames[first: first + len(group)]:
                        raise RuntimeError(f"the sampler returned {got} generated frames where {frames[first: first + len(group)]} were planned")
                    wave_buf, counts = decode_utterances(self.vocoder, kind, rows, row_start, got)
                    signal, pcm = session.push(wave_buf, counts)
                    piece = (pcm if return_pcm16 else signal).cpu().numpy()
                first += len(group)
                yield piece, self.target_sample_rate
        finally:
            session.close()

    # ------------------------------------------------------------------ one script in several voices
    def _plan_multi(self, text, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor):
        """`_plan_jobs` per piece of the script, each with its voice's fields: the arguments' defaults, the flat job list, the voice (field
        dict) of every job and the jobs per segment (one segment per piece, in order)."""
        voices = self.voices
        if "main" not in voices:
            raise ValueError("Reference audio not preprocessed. Call preprocess_reference() first.")
        settings, jobs, job_voices, seg_sizes = None, [], [], []
        for name, piece in split_voice_script(text, voices):
            print(f"Voice: {name}")
            with self._voice_installed(voices[name]):
                settings, piece_jobs = self._plan_jobs(piece, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration,
                                                       use_duration_predictor)
            if piece_jobs:
                jobs += piece_jobs
                job_voices += [voices[name]] * len(piece_jobs)
                seg_sizes.append(len(piece_jobs))
        if not jobs:
            raise RuntimeError("No audio generated")
        return settings, jobs, job_voices, seg_sizes

    @staticmethod
    def _voice_rms_table(job_voices):
        """``(rms vector on the device: one value per distinct voice, index of every job's voice in it)``"""
        distinct, index = [], []
        for v in job_voices:
            at = next((i for i, d in enumerate(distinct) if d is v), None)
            if at is None:
                at = len(distinct)
                distinct.append(v)
            index.append(at)
        return torch.stack([v["rms"].reshape(()) for v in distinct]), index

    @staticmethod
    def _own_pcm_flags(seg_sizes):
        """per job: it is a segment of its own, whose generate() call forms its int16 from the fp32 product (`finish_waves`'s ``pcm_f32``)"""
        return [g == 1 for g in seg_sizes for _ in range(g)]

    def generate_multi(self, text: str, output_path: Optional[str] = None, nfe_step: Optional[int] = None, cfg_strength: Optional[float] = None,
                       sway_sampling_coef: Optional[float] = None, speed: Optional[float] = None, fix_duration: Optional[float] = None,
                       cross_fade_duration: Optional[float] = None, use_duration_predictor: Optional[bool] = None,
                       return_numpy: bool = False, return_spectrogram: bool = False, return_pcm16: bool = False, remove_silence: bool = False):
        """One script in several voices (the reference's infer_cli.py:290-354): ``text`` is cut at its ``[name]`` tags
        (`utils_infer.split_voice_script`; voices come from `preprocess_reference` -- "main" -- and `add_voice`), every piece is planned as
        ``generate()`` plans it with that voice's prompt, and ALL chunks of ALL pieces are sampled as ragged batches with one prompt per
        utterance, decoded by one ragged vocoder call and finished by one segmented wave tail: cross-fades inside a piece, plain
        concatenation between pieces, each utterance's gain by its own voice's prompt rms.  After one ``torch.manual_seed`` and with
        attention dropout off the result is byte for byte ``np.concatenate([generate(piece, ...) with that voice installed for voice, piece
        in split_voice_script(text, voices)])`` -- float (float64 as soon as one piece cross-faded), ``return_pcm16`` and the written file;
        ``remove_silence`` applies to the whole result (infer_cli.py:360-363).  Same arguments and return shapes as ``generate()``."""
        (nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration), jobs, job_voices, seg_sizes = self._plan_multi(
            text, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor)
        return self._generate_multi_jobs(jobs, job_voices, seg_sizes, output_path, nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration,
                                         return_numpy, return_spectrogram, return_pcm16, remove_silence)

    def _generate_multi_jobs(self, jobs, job_voices, seg_sizes, output_path, nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration,
                             return_numpy, return_spectrogram, return_pcm16, remove_silence=False):
        """`_generate_jobs` for a flat job list over several voices: ``job_voices[i]`` is job i's voice, ``seg_sizes`` the jobs per piece."""
        mels = self._sample_jobs(jobs, nfe_step, cfg_strength, sway_sampling_coef, voices=job_voices)
        want_spec = return_spectrogram or output_path is not None
        want_float = not return_pcm16 or output_path is not None
        final_wave = final_pcm = None
        generated_waves, spectrograms = [], []
        skips = [v["ref_audio_len"] for v in job_voices]
        with torch.inference_mode():
            kind = device_tail_kind(self.vocoder, *[v["audio"] for v in job_voices], *mels)
            if kind is not None and kind == self.mel_spec_type and min(int(m.shape[1]) - k for m, k in zip(mels, skips)) >= 2:
                rows, row_start, frames = mel_rows_of(mels, skips)
                wave_buf, samples = decode_utterances(self.vocoder, kind, rows, row_start, frames)
                rms, rms_index = self._voice_rms_table(job_voices)
                done = finish_waves(wave_buf, samples, cross_fade_duration, self.target_sample_rate, rms=rms, target_rms=self.target_rms,
                                    want_float=want_float or remove_silence, want_pcm16=return_pcm16, segments=seg_sizes, rms_index=rms_index,
                                    pcm_f32=self._own_pcm_flags(seg_sizes))
                if want_spec:
                    spectrograms = [rows[r: r + t].t().cpu().numpy() for r, t in zip(row_start, frames)]
                if done is not None:
                    if remove_silence:
                        done, remove_silence = self._silence_step(*done), False
                    final_wave = done[0].cpu().numpy() if want_float else None
                    final_pcm = done[1].cpu().numpy() if return_pcm16 else None
                else:  # utterances shorter than their cross-fades (F5_ENOTSUP): the decoded waves take the host functions
                    for w, v in zip(torch.split(wave_buf, samples), job_voices):
                        generated_waves.append((w * v["rms"] / self.target_rms if bool(v["rms"] < self.target_rms) else w).cpu().numpy())
            else:
                for generated, v in zip(mels, job_voices):
                    generated = generated.to(torch.float32)[:, v["ref_audio_len"]:, :].permute(0, 2, 1)
                    if self.mel_spec_type == "vocos":
                        generated_wave = self.vocoder.decode(generated)
                    elif self.mel_spec_type == "bigvgan":
                        generated_wave = self.vocoder(generated)
                    rms = torch.sqrt(torch.mean(torch.square(v["audio"])))  # of the stored, already boosted prompt (:529-531)
                    if rms < self.target_rms:
                        generated_wave = generated_wave * rms / self.target_rms
                    generated_waves.append(generated_wave.squeeze().cpu().numpy())
                    if want_spec:
                        spectrograms.append(generated.squeeze().cpu().numpy())

        if final_wave is None and final_pcm is None:  # the host tail: cross_fade_concat per piece, np.concatenate of the pieces
            from ..streaming.wire import pcm16_bytes
            pieces, k = [], 0
            for g in seg_sizes:
                pieces.append(cross_fade_concat(generated_waves[k: k + g], cross_fade_duration, self.target_sample_rate))
                k += g
            final_wave = np.concatenate(pieces)
            if return_pcm16:  # (each piece's int16 from its own dtype, as its generate() call forms it)
                final_pcm = np.concatenate([np.frombuffer(pcm16_bytes(p), dtype=np.int16) for p in pieces])
        if remove_silence:  # the host tails (a foreign vocoder, or joints that chain): the same rule by the host functions
            final_wave, final_pcm = self._silence_step(final_wave, final_pcm)
        combined_spectrogram = np.concatenate(spectrograms, axis=1) if spectrograms else None
        if output_path is not None:
            output_dir = os.path.dirname(output_path)
            if output_dir and not os.path.exists(output_dir):
                os.makedirs(output_dir)
            _audio.write_wav(output_path, final_wave, self.target_sample_rate)
            if return_spectrogram:
                np.save(os.path.splitext(output_path)[0] + "_spec.npy", combined_spectrogram)
            if not return_numpy:
                return output_path
        if return_pcm16:
            final_wave = final_pcm
        if return_spectrogram:
            return final_wave, self.target_sample_rate, combined_spectrogram
        return final_wave, self.target_sample_rate

    def generate_multi_stream(self, text: str, nfe_step: Optional[int] = None, cfg_strength: Optional[float] = None,
                              sway_sampling_coef: Optional[float] = None, speed: Optional[float] = None, fix_duration: Optional[float] = None,
                              cross_fade_duration: Optional[float] = None, use_duration_predictor: Optional[bool] = None,
                              return_numpy: bool = True, return_spectrogram: bool = False, return_pcm16: bool = False):
        """`generate_multi` as a generator of ``(piece, sample_rate)``, as `generate_stream` is to `generate`: groups of consecutive chunks of
        the flat list (`utils_infer.chunk_groups`, the first ``stream_first_chunks`` on their own), per group one sampler call, one ragged
        decode and one push into a segmented `WaveStream`; a group that ends a voice's piece emits all of it.  The pieces, concatenated,
        are byte for byte what ``generate_multi()`` returns (attention dropout off).  When the streamed tail does not apply -- decided
        before any sampling, by `generate_stream`'s conditions -- the generator yields exactly once, with ``generate_multi()``'s result."""
        (nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration), jobs, job_voices, seg_sizes = self._plan_multi(
            text, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor)
        skips = [v["ref_audio_len"] for v in job_voices]
        frames = [min(max(max(len(tokens[0]), int(v["mel"].shape[1])) + 1, duration), 4096) - v["ref_audio_len"]
                  for (tokens, duration), v in zip(jobs, job_voices)]  # (`_generated_frames` with each job's own prompt)
        kind = device_tail_kind(self.vocoder, *[v["audio"] for v in job_voices])
        session = None
        if kind is not None and kind == self.mel_spec_type and min(frames) >= 2:
            samples = [(t - 1) * self.hop_length for t in frames] if kind == "vocos" else [t * self.vocoder._total_up() for t in frames]
            with torch.inference_mode():
                rms, rms_index = self._voice_rms_table(job_voices)
                session = WaveStream(samples, cross_fade_duration, self.target_sample_rate, rms=rms, target_rms=self.target_rms,
                                     want_float=not return_pcm16, want_pcm16=return_pcm16, segments=seg_sizes, rms_index=rms_index,
                                     pcm_f32=self._own_pcm_flags(seg_sizes))
        if session is None or not session.ok:
            wave, rate = self._generate_multi_jobs(jobs, job_voices, seg_sizes, None, nfe_step, cfg_strength, sway_sampling_coef, cross_fade_duration,
                                                   True, False, return_pcm16)
            yield wave, rate
            return
        try:
            first = 0
            for group in chunk_groups([d for _, d in jobs], int(self.stream_first_chunks), int(self.ragged_chunks)):
                mels = self._sample_jobs([jobs[i] for i in group], nfe_step, cfg_strength, sway_sampling_coef, voices=[job_voices[i] for i in group])
                with torch.inference_mode():
                    rows, row_start, got = mel_rows_of(mels, [skips[i] for i in group])
                    if got != frames[first: first + len(group)]:
                        raise RuntimeError(f"the sampler returned {got} generated frames where {frames[first: first + len(group)]} were planned")
                    wave_buf, counts = decode_utterances(self.vocoder, kind, rows, row_start, got)
                    signal, pcm = session.push(wave_buf, counts)
                    piece = (pcm if return_pcm16 else signal).cpu().numpy()
                first += len(group)
                yield piece, self.target_sample_rate
        finally:
            session.close()

    def _generated_frames(self, jobs):
        """Frames each job's sample() call generates behind the prompt, from the host values alone: the sampler raises the frames asked for to
        one more than the longer of the text and the prompt's mel, and caps them at 4096 (model/cfm.py)."""
        cond_frames = self.model.mel_spec.frame_count(self.ref_audio_processed.shape[-1])
        return [min(max(max(len(tokens[0]), cond_frames) + 1, duration), 4096) - self.ref_audio_len for tokens, duration in jobs]

    def _chunk_stream_pool(self, n):
        pool = getattr(self, "_chunk_streams_pool", None) or []
        while len(pool) < n:
            pool.append(torch.cuda.Stream())
        self._chunk_streams_pool = pool
        return pool[:n]

    def get_current_audio_length(self):
        if self.ref_audio_processed is None:
            return 0
        return self.ref_audio_processed.shape[-1] / self.target_sample_rate
