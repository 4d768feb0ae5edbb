"""Speaker similarity ("SIM") on MI355X: the ECAPA-TDNN speaker-verification head of the reference's ``eval/ecapa_tdnn.py`` behind
``utils_eval.run_sim`` -- the figure ``eval_seedtts_testset.py`` / ``eval_librispeech_test_clean.py`` report next to WER, and the number the
pruning workbench (``block_ablation``, ``select_blocks``, ``F5TTSWrapper.set_active_blocks``) needs to say whether a pruned model still speaks
with the prompt's voice.

What runs here (``csrc/speaker.hip``, fp32, forward only): everything of ``ECAPA_TDNN.get_feat`` / ``forward`` behind the feature extractor --
layer mix, instance norm, layer1, the three SE-Res2 blocks, the wide convolution, the attentive statistics pool, BatchNorm and the embedding
linear -- plus run_sim's resample (``f5_frontend_resample``) and cosine around it.  The published checkpoint ``wavlm_large_finetune.pth`` loads
by its own key names (``torch.load(...)["model"]``).

The feature extractor in front of it is a plug point.  ``eval/wavlm.py``'s ``WavLMExtractor`` fills it on the device (``csrc/wavlm.hip``;
``WavLMExtractor.from_speaker_checkpoint`` reads its tensors from the same ``wavlm_large_finetune.pth``): an object with ``extract`` gets all
2 n waves in ONE ragged call and its packed hidden states go to the head as they are.  Any other callable
``feature_extractor(list_of_16kHz_waves)`` that returns the hidden states, as s3prl's ``{"hidden_states": [L tensors [B, T, F]]}`` or one
stacked tensor, is called one wave at a time as before.  Nothing here fetches anything.
``global_context_att=True`` checkpoints are refused (another function, not approximated)."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from .. import _lib

SIM_SAMPLE_RATE = 16000  # run_sim resamples both waves to 16 kHz before the extractor
_SKIP_PREFIX = "feature_extract."
_NO_EXTRACTOR = ("speaker_similarity needs feature_extractor: a callable taking a list of 16 kHz waves (1-D device tensors) and returning the "
                 "WavLM hidden states, as s3prl's {'hidden_states': [L tensors [B, T, F]]} or one stacked tensor [L, B, T, F].  WavLM itself is not "
                 "provided (the reference loads it from s3prl over torch.hub; nothing here downloads it): load it yourself and pass it in.")


def _spec(cfg):
    Fd, ch, W, w = cfg["feat_dim"], cfg["channels"], cfg["cat_channels"], cfg["channels"] // cfg["scale"]
    spec = {"feature_weight": (cfg["layers"],)}

    def bn(p, n):
        for f in ("weight", "bias", "running_mean", "running_var"):
            spec[f"{p}.{f}"] = (n,)

    spec["layer1.conv.weight"], spec["layer1.conv.bias"] = (ch, Fd, 5), (ch,)
    bn("layer1.bn", ch)
    for b in (2, 3, 4):
        for cb in ("Conv1dReluBn1", "Conv1dReluBn2"):
            spec[f"layer{b}.{cb}.conv.weight"], spec[f"layer{b}.{cb}.conv.bias"] = (ch, ch, 1), (ch,)
            bn(f"layer{b}.{cb}.bn", ch)
        for i in range(cfg["scale"] - 1):
            spec[f"layer{b}.Res2Conv1dReluBn.convs.{i}.weight"], spec[f"layer{b}.Res2Conv1dReluBn.convs.{i}.bias"] = (w, w, 3), (w,)
            bn(f"layer{b}.Res2Conv1dReluBn.bns.{i}", w)
        spec[f"layer{b}.SE_Connect.linear1.weight"], spec[f"layer{b}.SE_Connect.linear1.bias"] = (cfg["se_bottleneck"], ch), (cfg["se_bottleneck"],)
        spec[f"layer{b}.SE_Connect.linear2.weight"], spec[f"layer{b}.SE_Connect.linear2.bias"] = (ch, cfg["se_bottleneck"]), (ch,)
    spec["conv.weight"], spec["conv.bias"] = (W, 3 * ch, 1), (W,)
    spec["pooling.linear1.weight"], spec["pooling.linear1.bias"] = (cfg["attention_channels"], W, 1), (cfg["attention_channels"],)
    spec["pooling.linear2.weight"], spec["pooling.linear2.bias"] = (W, cfg["attention_channels"], 1), (W,)
    bn("bn", 2 * W)
    spec["linear.weight"], spec["linear.bias"] = (cfg["emb_dim"], 2 * W), (cfg["emb_dim"],)
    return spec


class SpeakerEncoder:
    """``ECAPA_TDNN_SMALL(feat_dim=1024, feat_type="wavlm_large")`` without its feature extractor.  Not an ``nn.Module``: it holds no trainable
    state, only the host copy of the checkpoint's tensors and the native handle built from them on first use."""

    def __init__(self, feat_dim=1024, channels=512, emb_dim=256, layers=25, cat_channels=1536, se_bottleneck=128, attention_channels=128, scale=8):
        self.cfg = dict(feat_dim=int(feat_dim), channels=int(channels), emb_dim=int(emb_dim), layers=int(layers), cat_channels=int(cat_channels),
                        se_bottleneck=int(se_bottleneck), attention_channels=int(attention_channels), scale=int(scale))
        self.emb_dim = self.cfg["emb_dim"]
        self._spec = _spec(self.cfg)
        self._state = None
        self._native = None

    # ------------------------------------------------------------------ checkpoint
    def load_state_dict(self, state_dict):
        """The reference's ``state_dict()`` names.  ``feature_extract.*`` and ``num_batches_tracked`` are ignored; any other unknown name, a
        missing tensor or a wrong shape raises, naming it.  A ``global_context_att=True`` pooling is refused."""
        kept, unknown = {}, []
        for k, v in state_dict.items():
            if k.startswith(_SKIP_PREFIX) or k.endswith("num_batches_tracked"):
                continue
            if k not in self._spec:
                unknown.append(k)
                continue
            kept[k] = v
        w = kept.get("pooling.linear1.weight")
        if w is not None and w.ndim >= 2 and w.shape[1] == 3 * self.cfg["cat_channels"]:
            raise ValueError(f"pooling.linear1.weight has {w.shape[1]} = 3 x {self.cfg['cat_channels']} input channels: a global_context_att=True "
                             "checkpoint.  The device head implements global_context_att=False (ECAPA_TDNN_SMALL / run_sim) and does not approximate the other.")
        if unknown:
            raise KeyError(f"unexpected key(s) in the speaker checkpoint: {unknown[:4]}{' ...' if len(unknown) > 4 else ''}")
        for name, shape in self._spec.items():
            if name not in kept:
                raise KeyError(f"missing key in the speaker checkpoint: {name}")
            if tuple(kept[name].shape) != tuple(shape):
                raise ValueError(f"{name}: shape {tuple(kept[name].shape)}, expected {tuple(shape)}")
        self._drop_native()
        self._state = {k: kept[k].detach().to("cpu", torch.float32).contiguous() for k in self._spec}
        return self

    @classmethod
    def from_checkpoint(cls, path, **config):
        """``wavlm_large_finetune.pth`` as run_sim loads it: ``torch.load(path)["model"]``, strict except for ``feature_extract.*``."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        state = ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt else ckpt
        return cls(**config).load_state_dict(state)

    # ------------------------------------------------------------------ native handle
    def _drop_native(self):
        if self._native is not None:
            _lib.load().f5_speaker_destroy(self._native)
            self._native = None

    def __del__(self):
        try:
            self._drop_native()
        except Exception:  # noqa: BLE001
            pass

    def native(self):
        if self._native is not None:
            return self._native
        if self._state is None:
            raise RuntimeError("SpeakerEncoder has no weights: call load_state_dict() or build it with from_checkpoint()")
        _lib.require_gpu()
        lib = _lib.load()
        cfg = _lib.SpeakerConfig(**self.cfg)
        hd = C.c_void_p()
        _lib.check(lib.f5_speaker_create(C.byref(cfg), C.byref(hd)), "speaker_create")
        try:
            _lib.set_tensors(hd, "f5_speaker_set_tensor", "f5_speaker_has_tensor", self._state)
            _lib.check(lib.f5_speaker_finalize(hd), "speaker_finalize")
        except Exception:
            lib.f5_speaker_destroy(hd)
            raise
        self._native = hd
        return hd

    # ------------------------------------------------------------------ embedding
    @staticmethod
    def _frames_of(features):
        """-> (list of frame counts, how to get the packed [L, rows, F] tensor)"""
        if isinstance(features, torch.Tensor):
            if features.ndim != 4:
                raise ValueError(f"features: one tensor must be [L, B, T, F], got {tuple(features.shape)}")
            return [int(features.shape[2])] * int(features.shape[1])
        if not isinstance(features, (list, tuple)) or not features:
            raise ValueError("features: a non-empty list of [L, T, F] tensors or one [L, B, T, F] tensor")
        for f in features:
            if not isinstance(f, torch.Tensor) or f.ndim != 3:
                raise ValueError("features: every list entry must be a tensor [L, T, F]")
        return [int(f.shape[1]) for f in features]

    def check_features(self, features):
        """Shape checks without touching the device (also what ``embed`` runs first); returns the frame counts."""
        frames = self._frames_of(features)
        first = features if isinstance(features, torch.Tensor) else features[0]
        L, Fd = int(first.shape[0]), int(first.shape[-1])
        if L != self.cfg["layers"] or Fd != self.cfg["feat_dim"]:
            raise ValueError(f"features have {L} layers of {Fd} features; the encoder was built for {self.cfg['layers']} x {self.cfg['feat_dim']}")
        if not isinstance(features, torch.Tensor):
            for f in features:
                if int(f.shape[0]) != L or int(f.shape[2]) != Fd:
                    raise ValueError("features: utterances differ in layers or feature width")
        for u, t in enumerate(frames):
            if t < 2:
                raise ValueError(f"utterance {u} has {t} frame(s): the speaker head needs at least 2 (InstanceNorm1d over one frame raises in the reference too)")
        return frames

    @torch.no_grad()
    def embed(self, features):
        """``features``: a list of device tensors ``[L, T_u, F]`` (utterances of different lengths) or one ``[L, B, T, F]`` tensor.  Returns
        ``[B, emb_dim]`` fp32 on the device.  One call is one ragged launch set (per 64 utterances) and nothing synchronises with the host; an
        utterance's embedding has the same bits whatever shares the call with it."""
        frames = self.check_features(features)
        self.native()
        if isinstance(features, torch.Tensor):
            L, B, T, Fd = features.shape
            hs = features.to(device="cuda", dtype=torch.float32).reshape(L, B * T, Fd).contiguous()
        else:
            hs = torch.cat([f.to(device="cuda", dtype=torch.float32) for f in features], dim=1).contiguous()
        return self._embed_rows(hs, frames)

    def _embed_rows(self, hs, frames):
        lib = _lib.load()
        hd = self.native()
        B = len(frames)
        emb = torch.empty(B, self.emb_dim, device=hs.device, dtype=torch.float32)
        with torch.cuda.device(hs.device):
            _lib.check(lib.f5_speaker_embed_ragged(hd, B, (C.c_int32 * B)(*frames), _lib.ptr(hs), _lib.ptr(emb), _lib.stream_ptr()), "speaker_embed_ragged")
        return emb

    @torch.no_grad()
    def embed_packed(self, hs, frames):
        """``hs``: one contiguous fp32 device tensor ``[L, sum(frames), F]``, the utterances back to back along the row axis -- what
        ``WavLMExtractor.extract`` returns, taken as it is (no concatenation).  The same launches, and so the same bits, as ``embed`` on the list of
        its slices."""
        frames = [int(t) for t in frames]
        if not isinstance(hs, torch.Tensor) or hs.ndim != 3 or not hs.is_cuda or hs.dtype != torch.float32 or not hs.is_contiguous():
            raise ValueError("embed_packed: hs must be a contiguous fp32 device tensor [L, rows, F]")
        if int(hs.shape[0]) != self.cfg["layers"] or int(hs.shape[2]) != self.cfg["feat_dim"]:
            raise ValueError(f"features have {int(hs.shape[0])} layers of {int(hs.shape[2])} features; the encoder was built for "
                             f"{self.cfg['layers']} x {self.cfg['feat_dim']}")
        if not frames or sum(frames) != int(hs.shape[1]):
            raise ValueError(f"embed_packed: frames sum to {sum(frames)}, hs has {int(hs.shape[1])} rows")
        for u, t in enumerate(frames):
            if t < 2:
                raise ValueError(f"utterance {u} has {t} frame(s): the speaker head needs at least 2 (InstanceNorm1d over one frame raises in the reference too)")
        return self._embed_rows(hs, frames)


def _hidden_states(out, n):
    """What an extractor returned for n waves -> list of n tensors [L, T, F] (its own, equal, T: the batch is padded by the extractor)."""
    if isinstance(out, dict):
        if "hidden_states" not in out:
            raise ValueError("feature_extractor returned a dict without 'hidden_states'")
        out = out["hidden_states"]
    if isinstance(out, (list, tuple)):
        out = torch.stack(list(out), dim=0)
    if not isinstance(out, torch.Tensor):
        raise ValueError("feature_extractor must return {'hidden_states': [...]}, a list of [B, T, F] tensors or one stacked tensor")
    if out.ndim == 3 and n == 1:
        out = out.unsqueeze(1)
    if out.ndim != 4 or out.shape[1] != n:
        raise ValueError(f"feature_extractor returned hidden states of shape {tuple(out.shape)} for {n} wave(s); expected [L, {n}, T, F]")
    return [out[:, b] for b in range(n)]


@torch.no_grad()
def speaker_similarity(encoder, pairs, feature_extractor=None, sample_rate=24000):
    """``run_sim`` without the files.  ``pairs``: a list of ``(generated, prompt)`` waves (1-D tensors, or ``[1, n]``), at ``sample_rate``
    (an int, or one ``(rate_generated, rate_prompt)`` tuple).  Each wave is resampled to 16 kHz on the device (``f5_frontend_resample``, the
    ``torchaudio.transforms.Resample`` both sides agree on) and handed to ``feature_extractor`` ONE AT A TIME, as run_sim does (batch 1: no
    padding frames enter the statistics); all 2 n utterances are then embedded in ragged launches and compared with ``F.cosine_similarity``.
    A ``feature_extractor`` with an ``extract`` method (``WavLMExtractor``) gets all 2 n waves in one ragged call instead, which keeps batch-1
    semantics per utterance and gives the same bits as the one-at-a-time route.
    Returns ``(similarities [n] on the device, their mean as a float)``; the ``float`` is the call's one synchronisation."""
    if not isinstance(encoder, SpeakerEncoder):
        raise TypeError("speaker_similarity: encoder must be a SpeakerEncoder")
    if feature_extractor is None or not callable(feature_extractor):
        raise ValueError(_NO_EXTRACTOR)
    if not isinstance(pairs, (list, tuple)) or not pairs:
        raise ValueError("speaker_similarity: pairs must be a non-empty list of (generated, prompt) waves")
    rates = tuple(sample_rate) if isinstance(sample_rate, (list, tuple)) else (sample_rate, sample_rate)
    if len(rates) != 2 or any(int(r) <= 0 for r in rates):
        raise ValueError("speaker_similarity: sample_rate is a positive int or a (generated, prompt) pair of them")
    from .. import frontend
    ragged = hasattr(feature_extractor, "extract")
    feats, waves = [], []
    for i, pair in enumerate(pairs):
        if not isinstance(pair, (list, tuple)) or len(pair) != 2:
            raise ValueError(f"speaker_similarity: pair {i} is not a (generated, prompt) pair")
        for wave, rate in zip(pair, rates):
            w = torch.as_tensor(wave)
            if w.ndim == 2 and w.shape[0] == 1:
                w = w[0]
            if w.ndim != 1 or w.numel() == 0:
                raise ValueError(f"speaker_similarity: pair {i} holds a wave of shape {tuple(w.shape)}; expected [n] or [1, n]")
            w = w.to(device="cuda", dtype=torch.float32)
            if int(rate) != SIM_SAMPLE_RATE:
                w = frontend.resample(w, int(rate), SIM_SAMPLE_RATE)
            if ragged:
                waves.append(w)
            else:
                feats.extend(_hidden_states(feature_extractor([w]), 1))
    emb = encoder.embed_packed(*feature_extractor.extract(waves)) if ragged else encoder.embed(feats)
    sim = F.cosine_similarity(emb[0::2], emb[1::2])
    return sim, float(sim.mean())


def wrapper_similarity(wrapper, wave, encoder, feature_extractor=None, voice="main", sample_rate=None):
    """Score a wave an ``F5TTSWrapper`` returned against the voice prompt it was cloned from: ``wrapper.voices[voice]["audio"]`` (at the
    wrapper's ``target_sample_rate``) versus ``wave`` (at ``sample_rate``, default the same).  What someone holds after
    ``set_active_blocks``: did the pruned model keep the voice?  Returns the similarity as a float."""
    voices = wrapper.voices
    if voice not in voices:
        raise KeyError(f"no voice {voice!r}: run preprocess_reference (or add_voice) first")
    native = int(wrapper.target_sample_rate)
    prompt = voices[voice]["audio"]
    wave = torch.as_tensor(wave)
    if wave.dtype in (torch.int16, torch.int32):
        wave = wave.to(torch.float32) / 32768.0
    _, mean = speaker_similarity(encoder, [(wave.reshape(-1), torch.as_tensor(prompt).reshape(-1))], feature_extractor,
                                 sample_rate=(int(sample_rate) if sample_rate else native, native))
    return mean
