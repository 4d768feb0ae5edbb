"""The WavLM feature extractor in front of the speaker head (``speaker.py``) on MI355X: the network ``utils_eval.run_sim`` takes from s3prl as
``wavlm_large``, here as ``csrc/wavlm.hip`` (fp32, forward only).  With it ``speaker_similarity`` needs nothing from outside this package but
the checkpoint: ``wavlm_large_finetune.pth`` carries the extractor's tensors under ``feature_extract.model.*`` next to the head's.

PINNED: the arithmetic is transformers' ``WavLMModel`` at ``feat_extract_norm="layer"``, ``do_stable_layer_norm=True`` (microsoft/wavlm-large),
state dict names included (``naming="hf"``); ``final_norm="hf"`` returns exactly ``WavLMModel(output_hidden_states=True).hidden_states``.  Tested
against a seeded tiny model's fp64 hidden states (tests/golden/wavlm_tiny.npz, tools/make_wavlm_golden.py).

UNPINNED (written from recollection; neither s3prl's nor fairseq's source was at hand): (1) ``final_norm="s3prl"`` -- the last hidden state
WITHOUT the encoder's final LayerNorm, which is what s3prl's ``layer_results`` are believed to hold, and the default because run_sim is the
purpose; (2) the fairseq key map of ``naming="fairseq"`` / ``from_speaker_checkpoint`` (``_FAIRSEQ_RULES`` below).  Both are one-line changes
if a comparison with s3prl says otherwise.

The relative position buckets use a float ``log``; they are evaluated here with torch, exactly as ``_relative_positions_bucket`` does, and handed
to the library as a table -- the device never computes a bucket."""
from __future__ import annotations

import ctypes as C
import math
import re

import torch

from .. import _lib

_LARGE = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_bias=False, hidden_size=1024,
              num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
              num_buckets=320, max_bucket_distance=800, layer_norm_eps=1e-5, feat_extract_norm="layer", do_stable_layer_norm=True, add_adapter=False)
_HEAD_DIMS = (16, 64)  # the attention kernel's builds (csrc/wavlm.hip)
_MIN_TABLE = 4096      # frames the first bucket table covers (82 s); a longer utterance rebuilds it once
_POS = "encoder.pos_conv_embed.conv."
_IGNORED = ("masked_spec_embed", "mask_emb")
_FINAL_NORM = {"s3prl": 0, "hf": 1}

# fairseq (the names inside wavlm_large_finetune.pth behind "feature_extract.model.") -> transformers.  UNPINNED, see the module docstring.
_FAIRSEQ_RULES = (
    (r"^feature_extractor\.conv_layers\.(\d+)\.0\.(weight|bias)$", r"feature_extractor.conv_layers.\1.conv.\2"),
    (r"^feature_extractor\.conv_layers\.(\d+)\.2\.1\.(weight|bias)$", r"feature_extractor.conv_layers.\1.layer_norm.\2"),
    (r"^layer_norm\.(weight|bias)$", r"feature_projection.layer_norm.\1"),
    (r"^post_extract_proj\.(weight|bias)$", r"feature_projection.projection.\1"),
    (r"^encoder\.pos_conv\.0\.(weight_g|weight_v|bias)$", r"encoder.pos_conv_embed.conv.\1"),
    (r"^encoder\.layers\.(\d+)\.self_attn\.(q_proj|k_proj|v_proj|out_proj)\.(weight|bias)$", r"encoder.layers.\1.attention.\2.\3"),
    (r"^encoder\.layers\.(\d+)\.self_attn\.grep_linear\.(weight|bias)$", r"encoder.layers.\1.attention.gru_rel_pos_linear.\2"),
    (r"^encoder\.layers\.(\d+)\.self_attn\.grep_a$", r"encoder.layers.\1.attention.gru_rel_pos_const"),
    (r"^encoder\.layers\.(\d+)\.self_attn\.relative_attention_bias\.weight$", r"encoder.layers.\1.attention.rel_attn_embed.weight"),
    (r"^encoder\.layers\.(\d+)\.self_attn_layer_norm\.(weight|bias)$", r"encoder.layers.\1.layer_norm.\2"),
    (r"^encoder\.layers\.(\d+)\.fc1\.(weight|bias)$", r"encoder.layers.\1.feed_forward.intermediate_dense.\2"),
    (r"^encoder\.layers\.(\d+)\.fc2\.(weight|bias)$", r"encoder.layers.\1.feed_forward.output_dense.\2"),
    (r"^encoder\.layers\.(\d+)\.final_layer_norm\.(weight|bias)$", r"encoder.layers.\1.final_layer_norm.\2"),
    (r"^encoder\.layer_norm\.(weight|bias)$", r"encoder.layer_norm.\1"),
)
SPEAKER_CHECKPOINT_PREFIX = "feature_extract.model."


def fairseq_to_hf(name):
    """one fairseq WavLM tensor name -> its transformers name, or None when no rule matches"""
    for pat, rep in _FAIRSEQ_RULES:
        if re.match(pat, name):
            return re.sub(pat, rep, name)
    return None


def _spec(cfg):
    """name -> shape of the tensors the native handle takes (the positional convolution folded)"""
    Fd, H, I, cd = cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"], cfg["conv_dim"]
    spec = {}
    for i, c in enumerate(cd):
        p = f"feature_extractor.conv_layers.{i}"
        spec[f"{p}.conv.weight"] = (c, 1 if i == 0 else cd[i - 1], cfg["conv_kernel"][i])
        if cfg["conv_bias"]:
            spec[f"{p}.conv.bias"] = (c,)
        spec[f"{p}.layer_norm.weight"] = spec[f"{p}.layer_norm.bias"] = (c,)
    spec["feature_projection.layer_norm.weight"] = spec["feature_projection.layer_norm.bias"] = (cd[-1],)
    spec["feature_projection.projection.weight"], spec["feature_projection.projection.bias"] = (Fd, cd[-1]), (Fd,)
    spec[_POS + "weight"] = (Fd, Fd // cfg["num_conv_pos_embedding_groups"], cfg["num_conv_pos_embeddings"])
    spec[_POS + "bias"] = (Fd,)
    spec["encoder.layer_norm.weight"] = spec["encoder.layer_norm.bias"] = (Fd,)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            spec[f"{p}.attention.{n}.weight"], spec[f"{p}.attention.{n}.bias"] = (Fd, Fd), (Fd,)
        spec[f"{p}.attention.gru_rel_pos_const"] = (1, H, 1, 1)
        spec[f"{p}.attention.gru_rel_pos_linear.weight"], spec[f"{p}.attention.gru_rel_pos_linear.bias"] = (8, Fd // H), (8,)
        if i == 0:
            spec[f"{p}.attention.rel_attn_embed.weight"] = (cfg["num_buckets"], H)
        for n in ("layer_norm", "final_layer_norm"):
            spec[f"{p}.{n}.weight"] = spec[f"{p}.{n}.bias"] = (Fd,)
        spec[f"{p}.feed_forward.intermediate_dense.weight"], spec[f"{p}.feed_forward.intermediate_dense.bias"] = (I, Fd), (I,)
        spec[f"{p}.feed_forward.output_dense.weight"], spec[f"{p}.feed_forward.output_dense.bias"] = (Fd, I), (Fd,)
    return spec


def relative_buckets(num_buckets, max_distance, n):
    """The model's bucket of the distances d = key - query = -(n - 1) .. n - 1, int32 [2 n - 1]: torch on the host, float log, the operations
    of ``WavLMAttention._relative_positions_bucket`` in its order."""
    d = torch.arange(-(n - 1), n, dtype=torch.long)
    nb = num_buckets // 2
    out = (d > 0).to(torch.long) * nb
    a = torch.abs(d)
    max_exact = nb // 2
    large = torch.log(a.float() / max_exact)
    large = large / math.log(max_distance / max_exact)
    large = large * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return (out + torch.where(a < max_exact, a, large)).to(torch.int32)


class WavLMExtractor:
    """WavLM (large form) on the device.  Not an ``nn.Module``: host copies of the tensors and a native handle built from them on first use.
    Config names are transformers' ``WavLMConfig``'s; the defaults are microsoft/wavlm-large.

    ``normalize_input`` (default True): ``F.layer_norm(wave, wave.shape)`` in front, as s3prl's expert does for the large model.
    ``final_norm``: ``"s3prl"`` (default, UNPINNED: the last state as the last layer left it) or ``"hf"`` (pinned: the encoder's LayerNorm applied
    to it, ``WavLMModel``'s hidden_states)."""

    def __init__(self, normalize_input=True, final_norm="s3prl", **config):
        unknown = sorted(set(config) - set(_LARGE))
        if unknown:
            raise ValueError(f"WavLMExtractor: unknown config field(s) {unknown}")
        cfg = dict(_LARGE, **config)
        for k in ("conv_dim", "conv_kernel", "conv_stride"):
            cfg[k] = tuple(int(v) for v in cfg[k])
        if cfg["feat_extract_norm"] != "layer":
            raise ValueError(f"feat_extract_norm={cfg['feat_extract_norm']!r}: only \"layer\" is implemented (\"group\" is WavLM base, another network)")
        if not cfg["do_stable_layer_norm"]:
            raise ValueError("do_stable_layer_norm=False: only the stable-LayerNorm (pre-LN) encoder is implemented")
        if cfg["add_adapter"]:
            raise ValueError("add_adapter=True: adapters are not implemented")
        if not (len(cfg["conv_dim"]) == len(cfg["conv_kernel"]) == len(cfg["conv_stride"])) or not 1 <= len(cfg["conv_dim"]) <= 8:
            raise ValueError("conv_dim, conv_kernel and conv_stride must have the same length, 1 .. 8")
        if any(c <= 0 or c % 32 for c in cfg["conv_dim"]):
            raise ValueError(f"conv_dim={cfg['conv_dim']}: positive multiples of 32")
        Fd, H = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
        if H <= 0 or Fd <= 0 or Fd % H:
            raise ValueError(f"hidden_size={Fd} is not divisible by num_attention_heads={H}")
        if Fd // H not in _HEAD_DIMS:
            raise ValueError(f"num_attention_heads={H}: head dimension {Fd // H} is not built by the attention kernel {_HEAD_DIMS}")
        if Fd % 32 or int(cfg["intermediate_size"]) % 32:
            raise ValueError("hidden_size and intermediate_size must be multiples of 32")
        g = int(cfg["num_conv_pos_embedding_groups"])
        if g <= 0 or Fd % g or (Fd // g) % 16:
            raise ValueError(f"num_conv_pos_embedding_groups={g}: hidden_size / groups must be a multiple of 16")
        if final_norm not in _FINAL_NORM:
            raise ValueError(f"final_norm={final_norm!r}: 'hf' or 's3prl'")
        self.cfg = cfg
        self.normalize_input = bool(normalize_input)
        self.final_norm = final_norm
        self.layers = int(cfg["num_hidden_layers"]) + 1
        self.feat_dim = Fd
        self._spec = _spec(cfg)
        self._state = None
        self._native = None
        self._table_n = 0

    # ------------------------------------------------------------------ checkpoint
    def load_state_dict(self, state_dict, naming="hf"):
        """Strict: a missing, unknown or mis-shaped name raises and names it (``masked_spec_embed`` / ``mask_emb`` are ignored).  ``naming``:
        ``"hf"`` (``WavLMModel.state_dict()``) or ``"fairseq"`` (UNPINNED map).  The positional convolution comes as
        ``parametrizations.weight.original0/1`` or ``weight_g/weight_v`` and is folded here (W = g v / ||v||, the norm over dims (0, 1) per tap),
        or already folded as ``weight``."""
        if naming not in ("hf", "fairseq"):
            raise ValueError(f"naming={naming!r}: 'hf' or 'fairseq'")
        sd, unknown = {}, []
        for k, v in state_dict.items():
            if k in _IGNORED:
                continue
            name = fairseq_to_hf(k) if naming == "fairseq" else k
            if name is None:
                unknown.append(k)
                continue
            sd[name] = v
        for g, v in (("parametrizations.weight.original0", "parametrizations.weight.original1"), ("weight_g", "weight_v")):
            if _POS + g in sd or _POS + v in sd:
                if _POS + g not in sd or _POS + v not in sd:
                    raise KeyError(f"missing key in the WavLM checkpoint: {_POS + (g if _POS + g not in sd else v)}")
                if _POS + "weight" in sd:
                    raise KeyError(f"the WavLM checkpoint holds both {_POS}weight and its weight-norm parts")
                wg, wv = sd.pop(_POS + g).detach().to("cpu", torch.float64), sd.pop(_POS + v).detach().to("cpu", torch.float64)
                if wg.numel() != wv.shape[-1]:
                    raise ValueError(f"{_POS + g}: shape {tuple(wg.shape)} does not hold one gain per tap of {tuple(wv.shape)}")
                sd[_POS + "weight"] = (wg.reshape(1, 1, -1) * wv / wv.norm(p=2, dim=(0, 1), keepdim=True)).to(torch.float32)
        unknown += [k for k in sd if k not in self._spec]
        if unknown:
            raise KeyError(f"unexpected key(s) in the WavLM checkpoint: {unknown[:4]}{' ...' if len(unknown) > 4 else ''}")
        for name, shape in self._spec.items():
            if name not in sd:
                raise KeyError(f"missing key in the WavLM checkpoint: {name}")
            if tuple(sd[name].shape) != tuple(shape):
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)}, expected {tuple(shape)}")
        self._drop_native()
        self._state = {k: sd[k].detach().to("cpu", torch.float32).contiguous() for k in self._spec}
        return self

    @classmethod
    def from_speaker_checkpoint(cls, path, **config):
        """The extractor inside ``wavlm_large_finetune.pth``: the ``feature_extract.model.*`` tensors of ``torch.load(path)["model"]``, the
        keys ``SpeakerEncoder`` skips, under fairseq's names (UNPINNED map)."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        state = ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt else ckpt
        n = len(SPEAKER_CHECKPOINT_PREFIX)
        own = {k[n:]: v for k, v in state.items() if k.startswith(SPEAKER_CHECKPOINT_PREFIX)}
        if not own:
            raise KeyError(f"{path} holds no {SPEAKER_CHECKPOINT_PREFIX}* tensors")
        return cls(**config).load_state_dict(own, naming="fairseq")

    # ------------------------------------------------------------------ native handle
    def _drop_native(self):
        if self._native is not None:
            _lib.load().f5_wavlm_destroy(self._native)
            self._native = None
            self._table_n = 0

    def __del__(self):
        try:
            self._drop_native()
        except Exception:  # noqa: BLE001
            pass

    def _native_config(self):
        c = self.cfg
        n = len(c["conv_dim"])
        pad = lambda t: (C.c_int32 * 8)(*(tuple(t) + (0,) * (8 - n)))  # noqa: E731
        return _lib.WavLMConfig(num_conv_layers=n, conv_dim=pad(c["conv_dim"]), conv_kernel=pad(c["conv_kernel"]), conv_stride=pad(c["conv_stride"]),
                                conv_bias=int(bool(c["conv_bias"])), hidden_size=int(c["hidden_size"]), num_hidden_layers=int(c["num_hidden_layers"]),
                                num_attention_heads=int(c["num_attention_heads"]), intermediate_size=int(c["intermediate_size"]),
                                num_conv_pos_embeddings=int(c["num_conv_pos_embeddings"]),
                                num_conv_pos_embedding_groups=int(c["num_conv_pos_embedding_groups"]), num_buckets=int(c["num_buckets"]),
                                max_bucket_distance=int(c["max_bucket_distance"]), feat_extract_norm=0, do_stable_layer_norm=1, add_adapter=0,
                                normalize_input=int(self.normalize_input), layer_norm_eps=float(c["layer_norm_eps"]))

    def native(self):
        if self._native is not None:
            return self._native
        if self._state is None:
            raise RuntimeError("WavLMExtractor has no weights: call load_state_dict() or build it with from_speaker_checkpoint()")
        _lib.require_gpu()
        lib = _lib.load()
        cfg = self._native_config()
        hd = C.c_void_p()
        _lib.check(lib.f5_wavlm_create(C.byref(cfg), C.byref(hd)), "wavlm_create")
        try:
            _lib.set_tensors(hd, "f5_wavlm_set_tensor", "f5_wavlm_has_tensor", self._state)
            _lib.check(lib.f5_wavlm_finalize(hd), "wavlm_finalize")
        except Exception:
            lib.f5_wavlm_destroy(hd)
            raise
        self._native = hd
        self._table_n = 0
        return hd

    def _ensure_buckets(self, hd, max_frames):
        if max_frames <= self._table_n:
            return
        n = _MIN_TABLE
        while n < max_frames:
            n *= 2
        b = relative_buckets(self.cfg["num_buckets"], self.cfg["max_bucket_distance"], n).contiguous()
        _lib.check(_lib.load().f5_wavlm_set_buckets(hd, n, C.cast(b.data_ptr(), C.POINTER(C.c_int32))), "wavlm_set_buckets")
        self._table_n = n

    # ------------------------------------------------------------------ extraction
    def frames(self, n_samples):
        """frames an utterance of ``n_samples`` gives (``_get_feat_extract_output_lengths``' rule); below 1 when it is too short for one"""
        n = int(n_samples)
        for k, s in zip(self.cfg["conv_kernel"], self.cfg["conv_stride"]):
            if n < k:
                return -1
            n = (n - k) // s + 1
        return n

    def conv_frames(self, n_samples):
        """frames behind every conv layer"""
        out, n = [], int(n_samples)
        for k, s in zip(self.cfg["conv_kernel"], self.cfg["conv_stride"]):
            n = (n - k) // s + 1
            out.append(n)
        return out

    def tap_shape(self, name, samples):
        """[rows, width] of a tap of a call over utterances of ``samples`` samples"""
        m = re.match(r"^conv(\d+)$", name)
        if m and int(m.group(1)) < len(self.cfg["conv_dim"]):
            i = int(m.group(1))
            return sum(self.conv_frames(n)[i] for n in samples), self.cfg["conv_dim"][i]
        return sum(self.frames(n) for n in samples), self.feat_dim

    @torch.no_grad()
    def extract(self, waves, final_norm=None, taps=None):
        """``waves``: a list of 1-D 16 kHz device waves of any lengths.  One ragged call; returns ``(hs, frames)``: ``hs`` fp32
        ``[L, sum(frames), F]`` on the device, the utterances back to back along the row axis (what ``SpeakerEncoder.embed_packed`` takes), and the
        list of frame counts.  An utterance's rows have the same bits whatever shares the call.  Nothing synchronises with the host in the steady
        state.  ``taps``: a dict whose keys name intermediate tensors (``conv{i}``, ``proj``, ``posconv``, ``layer{i}.attn``, ``layer{i}.out``);
        it is filled with them (test hook)."""
        fn = self.final_norm if final_norm is None else final_norm
        if fn not in _FINAL_NORM:
            raise ValueError(f"final_norm={fn!r}: 'hf' or 's3prl'")
        if not isinstance(waves, (list, tuple)) or not waves:
            raise ValueError("extract: waves must be a non-empty list of 1-D tensors")
        samples = []
        for u, w in enumerate(waves):
            if not isinstance(w, torch.Tensor) or w.ndim != 1:
                raise ValueError(f"extract: wave {u} is not a 1-D tensor")
            samples.append(int(w.numel()))
        frames = [self.frames(n) for n in samples]
        for u, t in enumerate(frames):
            if t < 1:
                raise ValueError(f"extract: utterance {u} has {samples[u]} sample(s), too short for one frame")
        lib = _lib.load()
        hd = self.native()
        self._ensure_buckets(hd, max(frames))
        cat = torch.cat([w.to(device="cuda", dtype=torch.float32) for w in waves]).contiguous()
        B = len(waves)
        hs = torch.empty(self.layers, sum(frames), self.feat_dim, device=cat.device, dtype=torch.float32)
        with torch.cuda.device(cat.device):
            if taps:
                for name in taps:
                    taps[name] = torch.full(self.tap_shape(name, samples), float("nan"), device=cat.device, dtype=torch.float32)
                    _lib.check(lib.f5_wavlm_set_tap(hd, name.encode(), _lib.ptr(taps[name])), f"wavlm_set_tap({name})")
            try:
                _lib.check(lib.f5_wavlm_extract_ragged(hd, B, (C.c_int32 * B)(*samples), _lib.ptr(cat), _FINAL_NORM[fn], _lib.ptr(hs), _lib.stream_ptr()),
                           "wavlm_extract_ragged")
            finally:
                if taps:
                    for name in taps:
                        lib.f5_wavlm_set_tap(hd, name.encode(), None)
        return hs, frames

    def __call__(self, waves):
        """s3prl's form for waves of EQUAL length: ``{"hidden_states": [L tensors [B, T, F]]}``, so the object fits any plug point that takes a
        callable extractor.  (Waves of different lengths: ``extract``.)"""
        if isinstance(waves, torch.Tensor):
            waves = [waves] if waves.ndim == 1 else list(waves)
        hs, frames = self.extract(list(waves))
        if len(set(frames)) != 1:
            raise ValueError("WavLMExtractor(waves): the waves give different frame counts; use extract() for a ragged batch")
        hs = hs.view(self.layers, len(frames), frames[0], self.feat_dim)
        return {"hidden_states": [hs[l] for l in range(self.layers)]}
