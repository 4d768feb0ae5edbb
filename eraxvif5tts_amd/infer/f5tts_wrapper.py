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
import dataclasses
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
                          load_checkpoint, load_vocoder, mel_rows_of, plan_request_groups, plan_wave_tail_segments, split_voice_script,
                          waves_of_mels)

_CONFIG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")


@dataclasses.dataclass
class TTSJob:
    """One request of `F5TTSWrapper.generate_batch`: the text, the stored voice that speaks it, and `generate()`'s settings for this request
    alone (None: the wrapper's attribute of the same name -- for ``speed`` the voice's own speed first, see `add_voice`).  ``seed``: the
    request's noise comes from a generator of its own seeded with it, so its audio does not depend on the requests around it."""
    text: str
    voice: str = "main"
    nfe_step: Optional[int] = None
    cfg_strength: Optional[float] = None
    sway_sampling_coef: Optional[float] = None
    speed: Optional[float] = None
    fix_duration: Optional[float] = None
    cross_fade_duration: Optional[float] = None
    use_duration_predictor: Optional[bool] = None
    remove_silence: bool = False
    seed: Optional[int] = None


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
        # the clip / trim / boost steps of preprocess_reference() and add_voice() on the GPU (infer/reference.py) when a call does not say
        # (on_device=None); off by default: the host steps, as before.  `last_reference_route` is "device" or "host" after each voice
        self.reference_on_device = os.environ.get("F5HIP_REFERENCE_DEVICE", "0").strip().lower() in ("1", "true", "yes", "on")
        self.last_reference_route = None
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
        self._output_format = None  # set_output_format(): None, or (output rate, "pcm16" | "mulaw" | "alaw")

    # ------------------------------------------------------------------ output format
    def set_output_format(self, sample_rate: Optional[int] = None, encoding: Optional[str] = None):
        """The format every synthesis entry point delivers in -- a setting of the wrapper, not a per-call argument.  ``sample_rate``: None (the
        native ``target_sample_rate``; passing that rate means the same) or a positive int; ``encoding``: None / "pcm16" (the same), "mulaw" or
        "alaw" (G.711).  Anything else raises ValueError and changes nothing.  With both unset every entry point behaves as it always has.
        With a format set the conversion is the last step behind the wave tail (and behind silence removal), on the device
        (`infer.deliver.convert_wave`: torchaudio's sinc_interp_hann resampler, its sums in ordered fp64): the returned sample rate is the output
        rate; a float return is float32 at that rate; ``return_pcm16=True`` returns int16 -- ``trunc(float32 * 32767)``, saturating -- or the
        uint8 G.711 codes of that int16; ``output_path`` is written at the output rate, as a mu-law / A-law WAV file under a G.711 encoding
        (`audio.write_wav_g711`).  At the native rate nothing is resampled: the float is the tail's, the int16 the tail's own, the codes
        `infer.deliver.g711_encode` of it.  Spectrograms are untouched.  The streamed entry points push each group's tail output into a
        `infer.deliver.ConvertStream`: their pieces, concatenated, are byte for byte the one-shot result under the same format and seed."""
        from .deliver import check_output_format
        self._output_format = check_output_format(sample_rate, encoding, self.target_sample_rate)

    @property
    def output_format(self):
        """None while no format is set, else ``(sample_rate, encoding)`` with the output rate and "pcm16", "mulaw" or "alaw"."""
        return getattr(self, "_output_format", None)

    def _format_step(self, signal, pcm16, want_float, want_codes):
        """The last step of delivery under `output_format`: ``(signal, codes)`` of a finished signal and its truncating PCM (device tensors from
        the device tail, arrays from the host tails; None where there is none).  At another rate both come from `convert_wave` of the signal
        (a host array is uploaded once: there is no CPU resampler); at the native rate the PCM is encoded where the encoding is G.711."""
        fmt = self.output_format
        if fmt is None:
            return signal, pcm16
        from .deliver import LAWS, convert_wave, g711_encode, g711_encode_device
        rate, encoding = fmt
        if rate != self.target_sample_rate:
            return convert_wave(signal, self.target_sample_rate, rate, encoding, want_float=want_float, want_codes=want_codes)
        if encoding in LAWS and pcm16 is not None:
            pcm16 = g711_encode_device(pcm16, encoding) if torch.is_tensor(pcm16) and pcm16.is_cuda else g711_encode(np.asarray(pcm16), encoding)
        return signal, pcm16

    def _load_checkpoint(self, model, ckpt_path, dtype=None, use_ema=True):
        return load_checkpoint(model, ckpt_path, self.device, dtype=dtype, use_ema=use_ema)

    def set_active_blocks(self, blocks=None):
        """Speak with a subset of the backbone's blocks (``DiT.set_active_blocks``): generate(), generate_stream(), generate_multi() and
        generate_batch() then run the pruned model on the weights already loaded -- a pruning choice can be listened to before any checkpoint
        is written (``eval.prune.prune_checkpoint``).  None restores all blocks."""
        self.model.transformer.set_active_blocks(blocks)

    # ------------------------------------------------------------------ reference voice
    def preprocess_reference(self, ref_audio_path: str, ref_text: str = "", clip_short: bool = True, on_device: Optional[bool] = None):
        """``on_device``: True runs the clip / trim / pad / mono / boost steps on the GPU (`infer.reference.prepare_reference_device`: the same
        samples; the boost divides by the exact rms, see there), False on the host, None as ``self.reference_on_device`` says.  A file the device
        route does not take (a sample width other than 16 bits, more than two channels) goes the host's way; ``self.last_reference_route`` tells
        which ran."""
        audio, ref_text = self._preprocess_voice(ref_audio_path, ref_text, clip_short, on_device)
        self.ref_audio_processed = audio
        self.ref_text = ref_text
        self.ref_audio_len = audio.shape[-1] // self.hop_length
        return audio, ref_text

    def _preprocess_voice(self, ref_audio_path, ref_text, clip_short, on_device=None):
        """The steps of preprocess_reference() / add_voice(): ``(audio on the device, ref_text as it is used)``."""
        from . import reference as _reference
        print("Converting audio...")
        aseg = _audio.Segment.from_file(ref_audio_path)
        on_device = getattr(self, "reference_on_device", False) if on_device is None else on_device
        on_device = bool(on_device) and _reference.device_route_takes(aseg)
        self.last_reference_route = "device" if on_device else "host"
        if on_device:
            audio, sr, _ = _reference.prepare_reference_device(aseg, clip_short, self.target_rms, device=self.device)
        else:
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

        if not on_device:
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
    def add_voice(self, name: str, ref_audio_path: str, ref_text: str = "", clip_short: bool = True, speed: Optional[float] = None,
                  on_device: Optional[bool] = None):
        """One more reference voice for `generate_multi`, under ``name`` (a ``\\w+`` word other than "main", which is the voice
        `preprocess_reference` stored): exactly the steps of `preprocess_reference`, with the prompt's mel and its rms computed once.  The main
        fields are not touched.  Returns ``(audio, ref_text)`` as `preprocess_reference` does.
        ``speed`` (the reference's per-voice ``speed`` of infer_cli's voice table): kept in the voice's fields and used for this voice's pieces
        where a call (`generate_multi`, `generate_multi_stream`) or a request (`generate_batch`) gives no ``speed`` of its own; None: the
        wrapper's ``speed``, as before.  ``on_device``: as in `preprocess_reference`."""
        if speed is not None and not float(speed) > 0:
            raise ValueError(f"voice {name!r}: speed {speed!r} is not a positive number")
        if not isinstance(name, str) or not re.fullmatch(r"\w+", name) or name == "main":
            raise ValueError(f"voice name {name!r}: a name is one \\w+ word (what a [name] tag can hold) and \"main\" is the voice of preprocess_reference()")
        audio, ref_text = self._preprocess_voice(ref_audio_path, ref_text, clip_short, on_device)
        self._voices[name] = self._voice_fields(audio, ref_text)
        if speed is not None:
            self._voices[name]["speed"] = float(speed)
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
    # A single-voice call is a multi-voice call with one voice and one segment (include/f5hip.h: f5_wave_finish IS f5_wave_finish_segments with
    # one segment and rms index 0, the same bytes): the four entry points differ in how the script is planned and share everything behind that.
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
        plan = self._plan_jobs(text, False, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor)
        return self._synthesize(*plan, output_path, return_numpy, return_spectrogram, return_pcm16, remove_silence)

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
        plan = self._plan_jobs(text, False, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor)
        yield from self._synthesize_stream(*plan, return_pcm16)

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
        plan = self._plan_jobs(text, True, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor)
        return self._synthesize(*plan, output_path, return_numpy, return_spectrogram, return_pcm16, remove_silence)

    def generate_multi_stream(self, text: str, nfe_step: Optional[int] = None, cfg_strength: Optional[float] = None,
                              sway_sampling_coef: Optional[float] = None, speed: Optional[float] = None, fix_duration: Optional[float] = None,
                              cross_fade_duration: Optional[float] = None, use_duration_predictor: Optional[bool] = None,
                              return_numpy: bool = True, return_spectrogram: bool = False, return_pcm16: bool = False):
        """`generate_multi` as a generator of ``(piece, sample_rate)``, as `generate_stream` is to `generate`: groups of consecutive chunks of
        the flat list (`utils_infer.chunk_groups`, the first ``stream_first_chunks`` on their own), per group one sampler call, one ragged
        decode and one push into a segmented `WaveStream`; a group that ends a voice's piece emits all of it.  The pieces, concatenated,
        are byte for byte what ``generate_multi()`` returns (attention dropout off).  When the streamed tail does not apply -- decided
        before any sampling, by `generate_stream`'s conditions -- the generator yields exactly once, with ``generate_multi()``'s result."""
        plan = self._plan_jobs(text, True, nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, cross_fade_duration, use_duration_predictor)
        yield from self._synthesize_stream(*plan, return_pcm16)

    def generate_batch(self, requests, return_pcm16: bool = False, return_spectrogram: bool = False):
        """Several INDEPENDENT requests -- what a server has in flight -- through one set of ragged batches: ``requests`` is a list of `TTSJob`
        objects (or dicts with its fields), each with its own voice (`preprocess_reference`: "main", `add_voice`), step count, guidance
        strength, sway coefficient, speed, duration, cross-fade and ``remove_silence``.  Returns a list in request order; entry i is what
        ``generate(text_i, <request i's settings>, return_numpy=True, return_pcm16=, return_spectrogram=)`` returns with voice i's fields
        installed: ``(wave, sample_rate)`` or ``(wave, sample_rate, spectrogram)``.

        Every request is planned as generate() plans it; all chunks of all requests form one flat list.  The initial noise of every chunk is
        drawn BEFORE any sampling, in flat order and with the shapes sample() draws: requests without ``seed`` from torch's global generator
        (the CPU generator under ``noise_device = "cpu"``), a request with ``seed`` from a ``torch.Generator`` of its own seeded with it.  So
          * after one ``torch.manual_seed(s)`` the results are byte for byte (dtype included) those of the generate() calls made one after the
            other after the same seed -- float, ``return_pcm16`` and the spectrogram;
          * a seeded request's result does not depend on its place in the list or on the other requests, and the unseeded requests around
            it equal the serial route over the unseeded requests alone.
        The sampler calls are formed by `utils_infer.plan_request_groups`: jobs of one ``(nfe_step, sway_sampling_coef, cfg_strength >= 1e-5)``
        share a time grid and run as ragged batches of up to ``ragged_chunks`` utterances / 16384 frames with one prompt and one guidance
        strength per utterance (libf5hip ``f5_sample_ragged_ex``) where generate()'s ragged rule holds for the group (DiT, at least 2 jobs, all
        of 256 .. 4096 frames); the jobs of every other group take sample() on the chunk streams.  Unguided requests (``cfg_strength`` below
        1e-5, the reference's single pass) share no call with other requests: their batch is not doubled, so below 512 frames the kernels a
        job meets -- and with them its bits in the 16-bit modes -- depend on the rows around it, and only generate()'s own groups keep them.  One ragged vocoder call decodes all jobs,
        one segmented wave tail per distinct cross-fade length finishes them (a segment per request), each request gets its slice, and
        ``remove_silence`` runs per request on its slice, on the device.  A foreign vocoder object, or a request whose joints chain (the tail
        answers F5_ENOTSUP), is finished per request by the host functions under the same contracts.  The ODE method is the wrapper's.
        With attention dropout on, a ragged call does not promise the bits of its batch-1 calls: the contracts then hold in distribution
        only, as for `generate_multi`.
        Raises ``ValueError`` naming the request's index -- before any sampling -- for an unknown voice, an empty text, ``nfe_step < 1`` or an
        unknown field, and for an empty list."""
        voices = self.voices
        if "main" not in voices and not self._voices:
            raise ValueError("Reference audio not preprocessed. Call preprocess_reference() first.")
        reqs = list(requests) if requests is not None else []
        if not reqs:
            raise ValueError("generate_batch: no requests")
        fields = [f.name for f in dataclasses.fields(TTSJob)]
        plans = []  # per request: (settings, voice, jobs)
        for r, req in enumerate(reqs):
            if isinstance(req, dict):
                unknown = sorted(set(req) - set(fields))
                if unknown or "text" not in req:
                    raise ValueError(f"request {r}: " + (f"unknown fields {unknown}" if unknown else "no text"))
                req = TTSJob(**req)
            elif not isinstance(req, TTSJob):
                raise ValueError(f"request {r}: a TTSJob or a dict with its fields is expected, not {type(req).__name__}")
            reqs[r] = req
            if req.voice not in voices:
                raise ValueError(f"request {r}: unknown voice {req.voice!r} (stored: {sorted(voices)})")
            if not isinstance(req.text, str) or not req.text.strip():
                raise ValueError(f"request {r}: empty text")
            voice = voices[req.voice]
            given = {k: getattr(req, k) for k in ("nfe_step", "cfg_strength", "sway_sampling_coef", "speed", "fix_duration", "cross_fade_duration",
                                                  "use_duration_predictor")}
            if given["speed"] is None:
                given["speed"] = voice.get("speed")  # add_voice(speed=)
            settings = types.SimpleNamespace(**{k: v if v is not None else getattr(self, k) for k, v in given.items()})
            if int(settings.nfe_step) < 1:
                raise ValueError(f"request {r}: nfe_step {settings.nfe_step} < 1")
            plans.append((settings, voice))
        jobs, job_voices, job_req, job_kw, seg_sizes = [], [], [], [], []
        for r, (settings, voice) in enumerate(plans):
            piece_jobs = self._plan_piece(voice, reqs[r].text, settings, settings.speed)
            if not piece_jobs:
                raise ValueError(f"request {r}: the text gives no chunk to speak")
            jobs += piece_jobs
            job_voices += [voice] * len(piece_jobs)
            job_req += [r] * len(piece_jobs)
            job_kw += [dict(steps=settings.nfe_step, cfg_strength=settings.cfg_strength, sway_sampling_coef=settings.sway_sampling_coef)] * len(piece_jobs)
            seg_sizes.append(len(piece_jobs))

        # the noise of every job, in flat order, with the shapes sample() draws (model/cfm.py): nothing below can change what a request hears
        frames = self._generated_frames(jobs, job_voices)
        mel_dim, dtype = self.model.num_channels, next(self.model.parameters()).dtype
        ndev = self.model.noise_device or self.model.device
        own, y0s = {}, []
        for k, (n, v) in enumerate(zip(frames, job_voices)):
            r = job_req[k]
            kw = {}
            if reqs[r].seed is not None:
                if r not in own:
                    own[r] = torch.Generator(device=ndev).manual_seed(int(reqs[r].seed))
                kw["generator"] = own[r]
            y0s.append(torch.randn(n + v["ref_audio_len"], mel_dim, device=ndev, dtype=dtype, **kw).to(self.model.device))

        keys = [(int(kw["steps"]), None if kw["sway_sampling_coef"] is None else float(kw["sway_sampling_coef"]), float(kw["cfg_strength"]) >= 1e-5)
                for kw in job_kw]
        keys = [key if key[2] else key + (r,) for key, r in zip(keys, job_req)]  # (an unguided request keeps generate()'s own groups)
        groups = plan_request_groups(keys, [d for _, d in jobs], int(self.ragged_chunks))
        mels = self._sample_jobs(jobs, job_voices, None, groups=groups, job_kw=job_kw, y0s=y0s)

        first = [0]
        for g in seg_sizes:
            first.append(first[-1] + g)
        results = [None] * len(reqs)
        skips = [v["ref_audio_len"] for v in job_voices]
        fmt = self.output_format  # (each request's finished wave is converted, behind its silence removal)
        rate = fmt[0] if fmt else self.target_sample_rate
        want_float = not return_pcm16 or any(q.remove_silence for q in reqs) or rate != self.target_sample_rate
        with torch.inference_mode():
            kind = device_tail_kind(self.vocoder, *mels)
            on_device = (kind is not None and (kind == "vocos") == (self.mel_spec_type == "vocos")
                         and min(int(m.shape[1]) - k for m, k in zip(mels, skips)) >= 2)
            by_fade = {}  # distinct cross-fade lengths in order of first appearance -> their requests
            for r, (settings, _) in enumerate(plans):
                by_fade.setdefault(float(settings.cross_fade_duration), []).append(r)
            if on_device:
                rows, row_start, got = mel_rows_of(mels, skips)
                wave_buf, samples = decode_utterances(self.vocoder, kind, rows, row_start, got)
                waves = torch.split(wave_buf, samples)
            for fade, members in by_fade.items() if on_device else ():
                idx = [k for r in members for k in range(first[r], first[r + 1])]
                sizes = [seg_sizes[r] for r in members]
                buf = wave_buf if len(idx) == len(jobs) else torch.cat([waves[k] for k in idx])
                lengths = [samples[k] for k in idx]
                done = finish_waves(buf, lengths, want_float=want_float, want_pcm16=return_pcm16,
                                    **self._tail_kw(types.SimpleNamespace(cross_fade_duration=fade), [job_voices[k] for k in idx], sizes))
                if done is None:
                    continue  # (joints that chain: these requests take the host functions below)
                plan = plan_wave_tail_segments(lengths, sizes, fade, self.target_sample_rate)
                starts, at = [], 0
                for g in sizes:
                    starts.append(plan["out_offsets"][at])
                    at += g
                starts.append(plan["total"])
                signal, pcm = done
                for j, r in enumerate(members):
                    wave = signal[starts[j]: starts[j + 1]] if signal is not None else None
                    if wave is not None and sizes[j] == 1 and wave.dtype == torch.float64:
                        wave = wave.to(torch.float32)  # (its fp32 values widened by the buffer's promotion: the cast back is exact)
                    part = pcm[starts[j]: starts[j + 1]] if pcm is not None else None
                    if reqs[r].remove_silence:
                        wave, part = self._silence_step(wave, part)
                    if fmt is not None:
                        wave, part = self._format_step(wave, part, not return_pcm16, return_pcm16)
                    out = (part if return_pcm16 else wave).cpu().numpy()
                    if return_spectrogram:
                        spec = np.concatenate([rows[row_start[k]: row_start[k] + got[k]].t().cpu().numpy() for k in range(first[r], first[r + 1])], axis=1)
                        results[r] = (out, rate, spec)
                    else:
                        results[r] = (out, rate)
        for r, (settings, _) in enumerate(plans):  # the host tails, per request: exactly what its generate() call does behind the sampler
            if results[r] is None:
                span = slice(first[r], first[r + 1])
                results[r] = self._deliver(mels[span], settings, job_voices[span], [seg_sizes[r]], None, True, return_spectrogram, return_pcm16,
                                           reqs[r].remove_silence)
        return results

    def _plan_jobs(self, text, tagged=False, nfe_step=None, cfg_strength=None, sway_sampling_coef=None, speed=None, fix_duration=None,
                   cross_fade_duration=None, use_duration_predictor=None):
        """The host work before any sampling: ``(settings, jobs, voices, seg_sizes)`` -- the arguments every entry point takes as one value,
        each with the wrapper's attribute of the same name where it is None; per text chunk the token list and the frames asked for (duration
        rule or predictor); the voice (field dict) of every job; and the jobs per segment.  ``tagged``: the text is a script whose ``[name]``
        tags pick the voices, one segment per piece; otherwise all of it is the main voice's, one segment, and no tag is looked for."""
        voices = self.voices
        if "main" not in voices:
            raise ValueError("Reference audio not preprocessed. Call preprocess_reference() first.")
        given = dict(nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, speed=speed, fix_duration=fix_duration,
                     cross_fade_duration=cross_fade_duration, use_duration_predictor=use_duration_predictor)
        settings = types.SimpleNamespace(**{k: v if v is not None else getattr(self, k) for k, v in given.items()})
        jobs, job_voices, seg_sizes = [], [], []
        for name, piece in split_voice_script(text, voices) if tagged else [("main", text)]:
            if tagged:
                print(f"Voice: {name}")
            voice = voices[name]
            own_speed = voice.get("speed") if speed is None else None  # add_voice(speed=): used where the call names none
            piece_jobs = self._plan_piece(voice, piece, settings, settings.speed if own_speed is None else own_speed)
            jobs += piece_jobs
            job_voices += [voice] * len(piece_jobs)
            if piece_jobs:
                seg_sizes.append(len(piece_jobs))
        if not jobs:
            raise RuntimeError("No audio generated")
        return settings, jobs, job_voices, seg_sizes

    def _plan_piece(self, voice, piece, settings, speed):
        """The jobs ``(token list, frames asked for)`` of one piece of text in one voice, as generate() plans them with that voice's prompt in the
        main fields: the chunks of `chunk_text` under the prompt's byte budget, each with the duration rule (or the predictor) at ``speed``."""
        can_use_predictor = settings.use_duration_predictor and self.has_duration_predictor
        ref_text, ref_audio_len = voice["ref_text"], voice["ref_audio_len"]
        audio_len = voice["audio"].shape[-1] / self.target_sample_rate
        max_chars = int(len(ref_text.encode("utf-8")) / audio_len * (22 - audio_len))
        text_batches = chunk_text(piece, max_chars=max_chars)
        for i, text_batch in enumerate(text_batches):
            print(f"Text batch {i}: {text_batch}")
        print("\n")

        jobs = []
        for text_batch in text_batches:  # host work of the reference's loop (:476-510)
            local_speed = 0.3 if len(text_batch.encode("utf-8")) < 10 else speed
            final_text_list = convert_char_to_pinyin([ref_text + text_batch])
            if settings.fix_duration is not None:
                duration = int(settings.fix_duration * self.target_sample_rate / self.hop_length)
                print(f"Using fixed duration: {settings.fix_duration}s ({duration} frames)")
            elif can_use_predictor:
                if isinstance(final_text_list[0], str):
                    text_tokens = list_str_to_idx(final_text_list, self.vocab_char_map).to(self.device)
                else:
                    text_tokens = torch.tensor(final_text_list, device=self.device)
                text_lengths = torch.tensor([len(t) for t in final_text_list], device=self.device)
                with self._voice_installed(voice):  # (the reference's public method reads self.ref_audio_len)
                    duration = self.calculate_duration_with_predictor(text_tokens, text_lengths, local_speed)
                print(f"Duration predictor output: {duration} frames")
            else:
                ref_text_len, gen_text_len = len(ref_text.encode("utf-8")), len(text_batch.encode("utf-8"))
                duration = ref_audio_len + int(ref_audio_len / ref_text_len * gen_text_len / local_speed)
                print(f"Calculated duration based on text ratio: {duration} frames")
            jobs.append((final_text_list, int(duration)))
        return jobs

    def _generated_frames(self, jobs, voices):
        """Frames each job's sample() call generates behind its voice's prompt, from the host values alone: the sampler raises the frames asked
        for to one more than the longer of the text and the prompt's mel, and caps them at 4096 (model/cfm.py)."""
        return [min(max(max(len(tokens[0]), int(v["mel"].shape[1])) + 1, duration), 4096) - v["ref_audio_len"]
                for (tokens, duration), v in zip(jobs, voices)]

    def _sample_jobs(self, jobs, voices, settings, *, groups=None, job_kw=None, y0s=None):
        """The mels of these jobs, in order, each over its own voice's prompt mel (``voices``: one field dict per job).  The text chunks of one
        call are independent (the reference samples them one after the other, :476-533), and a single-utterance sample() fills a fraction
        of the 256 CUs, so they run together, either way with the arithmetic of their own batch-1 calls and the noise drawn in chunk order
        (bit-identical mels):
          * ragged -- the backbone is the DiT and there are at least 2 jobs, all of at least 256 frames (the row count from which a batch-1
            call takes the tuned kernels too) and at most 4096: ONE ragged batch per group of chunks (`chunk_groups`), the utterances
            concatenated along the token axis without padding, one prompt per utterance zero-padded to the longest, with ``lens``;
          * otherwise sample() per job, up to `chunk_streams` of them in flight, each on a HIP stream (and a libf5hip plan) of its own.
        `generate_batch` hands over jobs of independent requests: ``groups`` (`utils_infer.plan_request_groups`: index lists, every group of
        one step count and time grid) replaces the rule's one list -- each group that meets the rule above is ONE ragged call with its jobs'
        guidance strengths as a vector, the jobs of every other group take sample(); ``job_kw`` holds each job's ``steps`` / ``cfg_strength`` /
        ``sway_sampling_coef`` and ``y0s`` its initial noise ([n, mel], drawn by the caller), so the grouping cannot change a bit."""
        transformer = getattr(self.model, "transformer", None)
        sample_kw = dict(steps=settings.nfe_step, cfg_strength=settings.cfg_strength, sway_sampling_coef=settings.sway_sampling_coef) if settings else None
        can_ragged = (int(self.ragged_chunks) >= 2 and torch.cuda.is_available() and hasattr(transformer, "native_sample_ragged")
                      and getattr(transformer, "BACKBONE", None) == 0)

        def fits(idx):  # the ragged rule over these jobs
            return can_ragged and len(idx) >= 2 and min(jobs[i][1] for i in idx) >= 256 and max(jobs[i][1] for i in idx) <= 4096

        if groups is None:
            ragged_groups = chunk_groups([d for _, d in jobs], 0, int(self.ragged_chunks)) if fits(range(len(jobs))) else []
            singles = [] if ragged_groups else list(range(len(jobs)))
        else:
            ragged_groups = [list(g) for g in groups if fits(g)]
            singles = [i for g in groups if not fits(g) for i in g]
        mels = [None] * len(jobs)
        with torch.inference_mode():
            for idx in ragged_groups:
                prompts = [voices[i]["mel"][0] for i in idx]
                lens = torch.tensor([int(m.shape[0]) for m in prompts], device=prompts[0].device, dtype=torch.long)
                cond = torch.nn.utils.rnn.pad_sequence(prompts, batch_first=True, padding_value=0.0)
                kw = sample_kw
                if job_kw is not None:  # one step count and time grid per group (the planner's key), a guidance strength per utterance
                    kw = dict(job_kw[idx[0]], cfg_strength=[float(job_kw[i]["cfg_strength"]) for i in idx])
                if y0s is not None:
                    kw = dict(kw, y0s=[y0s[i] for i in idx])
                for i, mel in zip(idx, self.model.sample_ragged(cond, [jobs[i][0][0] for i in idx], [jobs[i][1] for i in idx], lens=lens, **kw)):
                    mels[i] = mel
        if not singles:
            return mels
        n_streams = 1
        if torch.cuda.is_available() and hasattr(transformer, "finish_pending"):
            n_streams = max(1, min(len(singles), int(self.chunk_streams)))
        main, streams = (torch.cuda.current_stream(), self._chunk_stream_pool(n_streams)) if n_streams > 1 else (None, [])
        for st in streams:
            st.wait_stream(main)  # the prompts' mels were produced on the caller's stream
        for k, i in enumerate(singles):
            (tokens, duration), v = jobs[i], voices[i]
            kw = sample_kw if job_kw is None else job_kw[i]
            if y0s is not None:
                kw = dict(kw, y0=y0s[i].unsqueeze(0))
            with torch.inference_mode(), torch.cuda.stream(streams[k % n_streams]) if streams else contextlib.nullcontext():
                mels[i] = self.model.sample(cond=v["mel"], text=tokens, duration=duration, return_trajectory=False, **kw,
                                            **({"defer_guard": True} if streams else {}))[0]
        if not streams:
            return mels
        transformer.finish_pending()  # reads every chunk's fp16 range-guard flag (and lets the library redo a chunk whose guard fired)
        # finish_pending() synchronises a stream only when its plan has a guard to read (bf16 mode with fp16 storage); the vocoder runs on the
        # caller's stream, so that stream must be ordered behind EVERY chunk stream whatever the precision (round 4: the fp32 mode decoded
        # mels that were still being written -- found by test_generate_end_to_end_matches_the_oracle_chain[fp32-False])
        for st in streams:
            main.wait_stream(st)
        with torch.inference_mode():
            for i in singles:
                mels[i].record_stream(main)
        return mels

    def _silence_step(self, signal, pcm16=None):
        """The step behind the tail when ``remove_silence`` is on: ``(kept signal, kept pcm16 or None)`` at the reference's four values
        (`utils_infer.SILENCE_DEFAULTS`), on the device for device tensors (the `finish_waves` outputs), by the host functions for arrays."""
        from .utils_infer import SILENCE_DEFAULTS, remove_silence
        kept = remove_silence(signal, self.target_sample_rate, pcm16=pcm16, **SILENCE_DEFAULTS)
        return kept if pcm16 is not None else (kept, None)

    def _tail_kw(self, settings, voices, seg_sizes):
        """What `finish_waves` and `WaveStream` take alike for these jobs: the cross-fade, the rms rule as a device vector with one value per
        distinct voice and every job's index into it, the segments, and per job whether it is a segment of its own, whose int16 a call over
        it alone forms from the fp32 product (``pcm_f32``)."""
        distinct, index = [], []
        for v in voices:
            at = next((i for i, d in enumerate(distinct) if d is v), None)
            if at is None:
                at = len(distinct)
                distinct.append(v)
            index.append(at)
        return dict(cross_fade_duration=settings.cross_fade_duration, sample_rate=self.target_sample_rate, target_rms=self.target_rms,
                    rms=torch.stack([v["rms"].reshape(()) for v in distinct]), rms_index=index, segments=seg_sizes,
                    pcm_f32=[g == 1 for g in seg_sizes for _ in range(g)])

    def _synthesize(self, settings, jobs, voices, seg_sizes, output_path=None, return_numpy=False, return_spectrogram=False, return_pcm16=False,
                    remove_silence=False):
        """Sampler, mel -> wave (`utils_infer.waves_of_mels`: on the device where the vocoder is one of ours), and delivery in the three return
        shapes of generate()."""
        return self._deliver(self._sample_jobs(jobs, voices, settings), settings, voices, seg_sizes, output_path, return_numpy, return_spectrogram,
                             return_pcm16, remove_silence)

    def _deliver(self, mels, settings, voices, seg_sizes, output_path=None, return_numpy=False, return_spectrogram=False, return_pcm16=False,
                 remove_silence=False):
        """`_synthesize` behind the sampler: these mels -> what generate() returns, in the wrapper's `output_format` where one is set."""
        fmt = self.output_format
        rate = fmt[0] if fmt else self.target_sample_rate
        resamples = rate != self.target_sample_rate  # (then float and codes both come from the converted signal: the tail's PCM is not asked for)
        g711 = fmt is not None and fmt[1] != "pcm16"
        want_codes = return_pcm16 or (output_path is not None and g711)  # (a G.711 file holds the codes, a PCM file the rounded float)
        want_float = not return_pcm16 or (output_path is not None and not g711)
        want_spec = return_spectrogram or output_path is not None
        tail_pcm = want_codes and not resamples
        with torch.inference_mode():
            done, generated_waves, spectrograms = waves_of_mels(
                self.vocoder, self.mel_spec_type, mels, [v["ref_audio_len"] for v in voices], want_spec=want_spec, want_pcm16=tail_pcm,
                want_float=want_float or remove_silence or resamples, **self._tail_kw(settings, voices, seg_sizes))  # (the float wave is what is judged)
            if done is not None and remove_silence:
                done, remove_silence = self._silence_step(*done), False
            if done is not None and fmt is not None:
                done = self._format_step(*done, want_float, want_codes)
        if done is not None:
            final_wave = done[0].cpu().numpy() if want_float else None
            final_pcm = done[1].cpu().numpy() if want_codes else None
        else:  # the host tail: cross_fade_concat per segment, np.concatenate of the segments
            pieces, k = [], 0
            for g in seg_sizes:
                pieces.append(cross_fade_concat(generated_waves[k: k + g], settings.cross_fade_duration, self.target_sample_rate))
                k += g
            final_wave, final_pcm = np.concatenate(pieces), None
            if tail_pcm:  # (each segment's int16 from its own dtype, as its generate() call forms it)
                from ..streaming.wire import pcm16_bytes
                final_pcm = np.concatenate([np.frombuffer(pcm16_bytes(p), dtype=np.int16) for p in pieces])
        if remove_silence:  # the host tails (a foreign vocoder, or joints that chain): the same rule by the host functions
            final_wave, final_pcm = self._silence_step(final_wave, final_pcm)
        if done is None and fmt is not None:  # the host tails under a format: the signal is uploaded once and converted on the device
            with torch.inference_mode():
                final_wave, final_pcm = (None if x is None else x.cpu().numpy() if torch.is_tensor(x) else x
                                         for x in self._format_step(final_wave, final_pcm, want_float, want_codes))
        combined_spectrogram = np.concatenate(spectrograms, axis=1) if spectrograms else None
        if output_path is not None:
            output_dir = os.path.dirname(output_path)
            if output_dir and not os.path.exists(output_dir):
                os.makedirs(output_dir)
            if g711:
                _audio.write_wav_g711(output_path, final_pcm, rate, fmt[1])
            else:
                _audio.write_wav(output_path, final_wave, rate)
            if return_spectrogram:
                np.save(os.path.splitext(output_path)[0] + "_spec.npy", combined_spectrogram)  # matplotlib is not in the image
            if not return_numpy:
                return output_path
        if return_pcm16:
            final_wave = final_pcm
        if return_spectrogram:
            return final_wave, rate, combined_spectrogram
        return final_wave, rate

    def _synthesize_stream(self, settings, jobs, voices, seg_sizes, return_pcm16):
        """`_synthesize` group by group, as a generator of ``(piece, sample_rate)``; where the streamed tail does not apply, its result once."""
        frames = self._generated_frames(jobs, voices)
        kind = device_tail_kind(self.vocoder, *[v["audio"] for v in voices])
        fmt = self.output_format
        rate = fmt[0] if fmt else self.target_sample_rate
        resamples = rate != self.target_sample_rate  # (the tail then hands its float signal to a ConvertStream, which forms float and codes)
        session = converter = None
        if kind is not None and kind == self.mel_spec_type and min(frames) >= 2:
            samples = [(t - 1) * self.hop_length for t in frames] if kind == "vocos" else [t * self.vocoder._total_up() for t in frames]
            with torch.inference_mode():
                session = WaveStream(samples, want_float=not return_pcm16 or resamples, want_pcm16=return_pcm16 and not resamples,
                                     **self._tail_kw(settings, voices, seg_sizes))
        if session is None or not session.ok:
            yield self._synthesize(settings, jobs, voices, seg_sizes, return_numpy=True, return_pcm16=return_pcm16)
            return
        try:
            first = 0
            groups = chunk_groups([d for _, d in jobs], int(self.stream_first_chunks), int(self.ragged_chunks))
            for g, group in enumerate(groups):
                mels = self._sample_jobs([jobs[i] for i in group], [voices[i] for i in group], settings)
                with torch.inference_mode():
                    rows, row_start, got = mel_rows_of(mels, [voices[i]["ref_audio_len"] for i in group])
                    if got != frames[first: first + len(group)]:
                        raise RuntimeError(f"the sampler returned {got} generated frames where {frames[first: first + len(group)]} were planned")
                    wave_buf, counts = decode_utterances(self.vocoder, kind, rows, row_start, got)
                    signal, pcm = session.push(wave_buf, counts)
                    if resamples:
                        if converter is None:
                            from .deliver import ConvertStream
                            converter = ConvertStream(self.target_sample_rate, rate, fmt[1], is_f64=session.mixed, want_float=not return_pcm16,
                                                      want_codes=return_pcm16, device=wave_buf.device)
                        signal, pcm = converter.push(signal, last=g == len(groups) - 1)
                    elif fmt is not None:
                        signal, pcm = self._format_step(signal, pcm, not return_pcm16, return_pcm16)
                    piece = (pcm if return_pcm16 else signal).cpu().numpy()
                first += len(group)
                yield piece, rate
        finally:
            session.close()
            if converter is not None:
                converter.close()

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
