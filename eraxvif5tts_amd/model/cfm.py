"""Conditional-flow-matching sampler: drop-in for ``f5_tts.model.cfm.CFM`` on the inference path.

``sample()`` follows reference cfm.py:82-208 step by step on the host (mel of a raw-wave prompt, text -> ids, duration
rule, masks, per-sample seeded noise, sway-sampled time grid) and hands the whole ODE loop -- ``steps`` x (cond + uncond
DiT evaluations, CFG combine, fixed-grid update) and the final ``where(cond_mask, cond, y)`` -- to ONE native call
(``f5_sample`` in include/f5hip.h, hipGraph-replayed; ``f5_sample_masked`` for speech editing's ``edit_mask``) when the backbone is the
HIP ``DiT``.  For any other backbone object (plug point A accepts arbitrary modules) the same loop is driven from Python over
``transformer(...)`` calls.
The solver is ``odeint_kwargs["method"]``, one of torchdiffeq's fixed-grid methods (``ODE_METHODS``): euler, midpoint, rk4 (torchdiffeq's
``rk4_alt_step_func``, the 3/8 rule), heun2, heun3 -- 1 / 2 / 4 / 2 / 3 network evaluations per step.  Adaptive solvers, the Adams family and
other odeint options raise ``ValueError`` before any work.
``forward()`` (cfm.py:210-283) returns the flow-matching loss of a batch, FORWARD ONLY, for validation runs: ``flow_loss()`` restates the
reference's host logic with its random draws in the reference's order, calls the backbone once, and on the device wraps it in two HIP kernels
(``f5_cfm_noise``, ``f5_cfm_loss``: csrc/cfm_loss.hip).  It runs under ``no_grad``; gradients, the optimiser and the trainer are not provided.
"""
from __future__ import annotations

from dataclasses import dataclass
from random import random

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pad_sequence

from .modules import MelSpec
from .utils import default, exists, lens_to_mask, list_str_to_idx, list_str_to_tensor, mask_from_frac_lengths


@dataclass
class FlowLoss:
    """What ``CFM.flow_loss`` returns: the loss, its per-utterance parts, the backbone's tensors, and the random draws it used."""
    loss: torch.Tensor            # 0-dim: sum(sums) / sum(counts)
    sums: torch.Tensor            # f64 [b]: sum of the selected squared differences
    counts: torch.Tensor          # i64 [b]: selected rows x mel
    cond: torch.Tensor            # [b, n, mel]: where(rand_span_mask, 0, x1)
    pred: torch.Tensor            # [b, n, mel]: the backbone's output
    x0: torch.Tensor              # [b, n, mel]: the noise
    time: torch.Tensor            # [b]
    rand_span_mask: torch.Tensor  # bool [b, n], after the length mask
    drop_audio_cond: bool
    drop_text: bool


def _native_noise(x1, x0, time, span8):
    """f5_cfm_noise: (phi, cond) of device fp32 [b, n, mel] tensors; span8 u8 [b, n], time f32 [b]."""
    from .. import _lib
    lib = _lib.load()
    b, n, mel = x1.shape
    phi, cond = torch.empty_like(x1), torch.empty_like(x1)
    _lib.check(lib.f5_cfm_noise(b, n, mel, _lib.ptr(x1), _lib.ptr(x0), _lib.ptr(time), _lib.ptr(span8), _lib.ptr(phi), _lib.ptr(cond),
                                _lib.stream_ptr()), "cfm_noise")
    return phi, cond


def _native_loss(pred, x1, x0, span8):
    """f5_cfm_loss: (loss f32 0-dim, sums f64 [b], counts i64 [b]) on the device."""
    from .. import _lib
    lib = _lib.load()
    b, n, mel = x1.shape
    nbytes = lib.f5_cfm_loss_workspace(b, n, mel)
    if nbytes < 0:
        _lib.check(int(nbytes), "cfm_loss_workspace")
    work = torch.empty(nbytes, device=x1.device, dtype=torch.uint8)
    sums = torch.empty(b, device=x1.device, dtype=torch.float64)
    counts = torch.empty(b, device=x1.device, dtype=torch.int64)
    loss = torch.empty(1, device=x1.device, dtype=torch.float32)
    _lib.check(lib.f5_cfm_loss(b, n, mel, _lib.ptr(pred), _lib.ptr(x1), _lib.ptr(x0), _lib.ptr(span8), _lib.ptr(sums), _lib.ptr(counts),
                               _lib.ptr(loss), _lib.ptr(work), _lib.stream_ptr()), "cfm_loss")
    return loss.reshape(()), sums, counts


def _euler(fn, t0, t1, y):
    return (t1 - t0) * fn(t0, y)


def _midpoint(fn, t0, t1, y):
    dt = t1 - t0
    half = 0.5 * dt
    return dt * fn(t0 + half, y + fn(t0, y) * half)


def _rk4(fn, t0, t1, y):  # torchdiffeq rk4_alt_step_func (the 3/8 rule): what method="rk4" runs
    dt = t1 - t0
    k1 = fn(t0, y)
    k2 = fn(t0 + dt * (1 / 3), y + dt * k1 * (1 / 3))
    k3 = fn(t0 + dt * (2 / 3), y + dt * (k2 - k1 * (1 / 3)))
    k4 = fn(t1, y + dt * (k1 - k2 + k3))
    return (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def _heun2(fn, t0, t1, y):  # tableau c = [0, 1], a21 = 1, b = [1/2, 1/2]
    dt = t1 - t0
    k1 = fn(t0, y)
    k2 = fn(t0 + dt, y + dt * k1)
    return dt * (k1 * 0.5 + k2 * 0.5)


def _heun3(fn, t0, t1, y):  # tableau c = [0, 1/3, 2/3], a21 = 1/3, a32 = 2/3, b = [1/4, 0, 3/4]
    dt = t1 - t0
    k1 = fn(t0, y)
    k2 = fn(t0 + dt * (1 / 3), y + dt * k1 * (1 / 3))
    k3 = fn(t0 + dt * (2 / 3), y + dt * k2 * (2 / 3))
    return dt * (k1 * 0.25 + k3 * 0.75)


# torchdiffeq's fixed-grid solvers, fp32 operation order kept: method -> step(fn, t0, t1, y) = dy, with y1 = y + dy.  The native sampler runs
# the same methods (include/f5hip.h: F5_ODE_*).
ODE_METHODS = {"euler": _euler, "midpoint": _midpoint, "rk4": _rk4, "heun2": _heun2, "heun3": _heun3}


def ode_method(odeint_kwargs):
    """The fixed-grid method named by ``odeint_kwargs``; ValueError for anything this package does not run."""
    extra = sorted(set(odeint_kwargs) - {"method"})
    if extra:
        raise ValueError(f"unsupported odeint_kwargs {extra}: only 'method' is taken (one of {sorted(ODE_METHODS)})")
    method = odeint_kwargs.get("method", "euler")
    if method not in ODE_METHODS:
        raise ValueError(f"unsupported ODE method {method!r}: the fixed-grid solvers are {sorted(ODE_METHODS)}")
    return method


class CFM(nn.Module):
    def __init__(self, transformer, sigma=0.0, odeint_kwargs=dict(method="euler"), audio_drop_prob=0.35, cond_drop_prob=0.25,
                 num_channels=None, mel_spec_module=None, mel_spec_kwargs=dict(), frac_lengths_mask=(0.7, 1.0), vocab_char_map=None):
        super().__init__()
        self.frac_lengths_mask = frac_lengths_mask
        self.mel_spec = default(mel_spec_module, MelSpec(**mel_spec_kwargs))
        self.num_channels = default(num_channels, self.mel_spec.n_mel_channels)
        self.audio_drop_prob, self.cond_drop_prob = audio_drop_prob, cond_drop_prob
        self.transformer = transformer
        self.dim = transformer.dim
        self.sigma = sigma
        self.odeint_kwargs = odeint_kwargs
        self.vocab_char_map = vocab_char_map
        # where sample() draws its initial noise when none is given: None = on the model's device, as the reference does (cfm.py:182: a GPU
        # run uses the device generator); "cpu" = from torch's CPU generator and then moved, i.e. the numbers the reference's CPU path draws
        # for the same torch.manual_seed / seed= (end-to-end parity runs against the CPU oracle)
        self.noise_device = None

    @property
    def device(self):
        return next(self.parameters()).device

    def forward(self, inp, text, *, lens=None, noise_scheduler=None):
        """The reference's ``CFM.forward`` (cfm.py:210-283): same arguments, same ``(loss, cond, pred)``, the VALUE only -- it runs under
        ``torch.no_grad()`` through kernels that have no backward, so nothing returned here can be differentiated.  See ``flow_loss``."""
        r = self.flow_loss(inp, text, lens=lens)
        return r.loss, r.cond, r.pred

    @torch.no_grad()
    def flow_loss(self, inp, text, *, lens=None, x0=None, time=None, rand_span_mask=None, drop_audio_cond=None, drop_text=None):
        """The flow-matching loss of one batch, forward only (validation runs: picking a checkpoint, judging a pruned model).  NOTHING HERE
        CAN BE DIFFERENTIATED: no gradient, optimiser or trainer exists in this package, and the result carries no graph.

        Follows reference cfm.py:210-283 line by line -- raw wave -> mel, text -> ids, ``lens`` default, length mask, random span, noise, time,
        the two drop flags, ONE backbone call ``transformer(x=phi, cond=cond, text=text, time=time, drop_audio_cond=, drop_text=)`` (no mask, no
        cache: any module at plug point A works), masked MSE against ``x1 - x0`` -- and makes the random draws in the reference's order and on
        its devices: ``uniform_`` for the span fractions and the ``rand_like`` inside ``mask_from_frac_lengths`` (both on the model's device),
        ``randn_like(x1)``, ``torch.rand((batch,))`` on the model's device, then Python's ``random()`` twice.  After the same
        ``torch.manual_seed(s); random.seed(s)`` a CPU run draws what the reference draws.

        A draw given by keyword is NOT drawn; the draws after it keep their order.  ``rand_span_mask`` (bool [b, n]) stands for the two span
        draws and is still and-ed with the length mask; ``x0`` [b, n, mel]; ``time`` [b]; a given ``drop_audio_cond`` / ``drop_text`` is final and
        its ``random()`` call is skipped, a drawn ``drop_text`` follows the reference's rule (it also sets a DRAWN ``drop_audio_cond``).

        CUDA tensors (fp32) take the two HIP kernels: ``f5_cfm_noise`` (phi and cond: torch's bits) and ``f5_cfm_loss`` (the selected squared
        differences summed in fp64 in a fixed order: the same input gives the same bits; the flow and the elementwise loss never reach
        memory).  CPU tensors (an oracle backbone) take the torch expressions of the reference.

        Returns ``FlowLoss``: ``loss`` (0-dim; NaN when the span is empty, as ``mean()`` of an empty tensor), ``sums`` f64 [b] and ``counts`` i64
        [b] (per utterance: selected rows x mel; loss = sum(sums) / sum(counts)), ``cond``, ``pred``, and the draws used: ``x0``, ``time``,
        ``rand_span_mask`` (after the length mask), ``drop_audio_cond``, ``drop_text``."""
        if inp.ndim == 2:  # raw wave
            inp = self.mel_spec(inp)
            inp = inp.permute(0, 2, 1)
            assert inp.shape[-1] == self.num_channels
        batch, seq_len, dtype, device = *inp.shape[:2], inp.dtype, self.device

        if isinstance(text, list):
            if exists(self.vocab_char_map):
                text = list_str_to_idx(text, self.vocab_char_map).to(device)
            else:
                text = list_str_to_tensor(text).to(device)
            assert text.shape[0] == batch

        if not exists(lens):
            lens = torch.full((batch,), seq_len, device=device)
        mask = lens_to_mask(lens, length=seq_len)

        if not exists(rand_span_mask):
            frac_lengths = torch.zeros((batch,), device=self.device).float().uniform_(*self.frac_lengths_mask)
            rand_span_mask = mask_from_frac_lengths(lens, frac_lengths)
        rand_span_mask = rand_span_mask.to(mask.device) & mask

        x1 = inp
        x0 = torch.randn_like(x1) if not exists(x0) else x0.to(device=x1.device, dtype=dtype)
        time = torch.rand((batch,), dtype=dtype, device=self.device) if not exists(time) else time.to(device=self.device, dtype=dtype)

        native = x1.is_cuda
        if native:
            if dtype != torch.float32:
                raise TypeError(f"flow_loss on the device takes fp32 mels, not {dtype}")
            x1, x0 = x1.contiguous(), x0.contiguous()
            span8 = rand_span_mask.to(device=x1.device, dtype=torch.uint8).contiguous()
            phi, cond = _native_noise(x1, x0, time.to(x1.device).contiguous(), span8)
        else:
            t = time.unsqueeze(-1).unsqueeze(-1)
            phi = (1 - t) * x0 + t * x1
            cond = torch.where(rand_span_mask[..., None], torch.zeros_like(x1), x1)

        # cfg training with a drop rate (cfm.py:266-271): p_drop, then p_uncond
        audio_given = exists(drop_audio_cond)
        if not audio_given:
            drop_audio_cond = random() < self.audio_drop_prob
        if not exists(drop_text):
            drop_text = random() < self.cond_drop_prob
            if drop_text and not audio_given:
                drop_audio_cond = True
        drop_audio_cond, drop_text = bool(drop_audio_cond), bool(drop_text)

        pred = self.transformer(x=phi, cond=cond, text=text, time=time, drop_audio_cond=drop_audio_cond, drop_text=drop_text)

        if native:
            loss, sums, counts = _native_loss(pred.to(device=x1.device, dtype=torch.float32).contiguous(), x1, x0, span8)
        else:
            flow = x1 - x0
            elem = F.mse_loss(pred, flow, reduction="none")
            loss = elem[rand_span_mask].mean()
            sums = torch.where(rand_span_mask[..., None], elem.double(), torch.zeros((), dtype=torch.float64)).sum(dim=(1, 2))
            counts = rand_span_mask.sum(dim=1) * x1.shape[-1]
        return FlowLoss(loss=loss, sums=sums, counts=counts, cond=cond, pred=pred, x0=x0, time=time, rand_span_mask=rand_span_mask,
                        drop_audio_cond=drop_audio_cond, drop_text=drop_text)

    @torch.no_grad()
    def sample(self, cond, text, duration, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None, seed=None,
               max_duration=4096, vocoder=None, no_ref_audio=False, duplicate_test=False, t_inter=0.1, edit_mask=None,
               y0=None, return_trajectory=True, use_graph="auto", defer_guard=False, noise_device=None, edit_native=True):
        """Same arguments and return value ``(out, trajectory)`` as the reference.  Extra keyword-only knobs:
        ``y0`` (explicit initial noise, zero-padded [b, N, mel]: parity tests), ``noise_device`` ("cpu": draw the noise as the reference's
        CPU path does, cfm.py:178-183 with self.device = cpu; default ``self.noise_device``, None = the model's device), ``return_trajectory=False`` skips
        materialising the [steps+1, b, N, mel] trajectory (returned as None), ``use_graph`` = True / False / "auto" (default: replay a hipGraph from the second call with the same shape on),
        ``defer_guard=True`` returns without the call's one stream synchronisation (several sample() calls can then be in flight on several
        streams); ``transformer.finish_pending()`` completes them.  ``edit_mask`` calls run on the native sampler too (f5_sample_masked: the
        per-frame cond_mask replaces the lens prefix); ``edit_native=False`` sends them to the Python driver instead (parity tests).
        ``odeint_kwargs["method"]`` picks the fixed-grid solver (``ODE_METHODS``: euler, midpoint, rk4, heun2, heun3); any other method or
        odeint option raises ``ValueError`` before any work."""
        method = ode_method(self.odeint_kwargs)
        self.eval()
        if cond.ndim == 2:  # raw wave
            cond = self.mel_spec(cond)
            cond = cond.permute(0, 2, 1)
            assert cond.shape[-1] == self.num_channels
        cond = cond.to(next(self.parameters()).dtype)
        batch, cond_seq_len, device = *cond.shape[:2], cond.device
        if not exists(lens):
            lens = torch.full((batch,), cond_seq_len, device=device, dtype=torch.long)

        if isinstance(text, list):
            if exists(self.vocab_char_map):
                text = list_str_to_idx(text, self.vocab_char_map).to(device)
            else:
                text = list_str_to_tensor(text).to(device)
            assert text.shape[0] == batch

        cond_mask = lens_to_mask(lens)
        if edit_mask is not None:
            cond_mask = cond_mask & edit_mask
        if isinstance(duration, int):
            duration = torch.full((batch,), duration, device=device, dtype=torch.long)
        duration = torch.maximum(torch.maximum((text != -1).sum(dim=-1), lens) + 1, duration)  # at least one generated frame
        duration = duration.clamp(max=max_duration)
        max_dur = int(duration.amax())

        if duplicate_test:
            test_cond = F.pad(cond, (0, 0, cond_seq_len, max_dur - 2 * cond_seq_len), value=0.0)
        cond = F.pad(cond, (0, 0, 0, max_dur - cond_seq_len), value=0.0)
        if no_ref_audio:
            cond = torch.zeros_like(cond)
        cond_mask = F.pad(cond_mask, (0, max_dur - cond_mask.shape[-1]), value=False).unsqueeze(-1)
        step_cond = torch.where(cond_mask, cond, torch.zeros_like(cond))
        mask = lens_to_mask(duration) if batch > 1 else None  # single inference needs no mask (cfm.py:152-155)

        if y0 is None:
            ndev = default(default(noise_device, self.noise_device), self.device)
            rows = []
            for dur in duration:
                if exists(seed):
                    torch.manual_seed(seed)
                rows.append(torch.randn(int(dur), self.num_channels, device=ndev, dtype=step_cond.dtype))
            y0 = pad_sequence(rows, padding_value=0, batch_first=True).to(device)
        else:
            y0 = y0.to(device=device, dtype=step_cond.dtype)

        t_start = 0
        if duplicate_test:
            t_start = t_inter
            y0 = (1 - t_start) * y0 + t_start * test_cond
            steps = int(steps * (1 - t_start))
        t = torch.linspace(t_start, 1, steps + 1, device=self.device, dtype=step_cond.dtype)
        if sway_sampling_coef is not None:
            t = t + sway_sampling_coef * (torch.cos(torch.pi / 2 * t) - 1 + t)

        native = getattr(self.transformer, "native_sample", None)
        if native is not None and (edit_mask is None or edit_native):
            # lens-prefix cond_mask and duration-prefix key mask are rebuilt on the device by the kernels; an edit_mask call hands the
            # [b, N] cond_mask (lens_to_mask(lens) & edit_mask, False-padded) over as it is
            # a batch whose durations are all equal has an all-true key mask (cfm.py:152-155 builds it anyway): the kernels' unmasked
            # forms compute the same thing
            use_mask = mask is not None and bool((duration != max_dur).any())
            out, trajectory = native(cond, text, lens, duration, y0, t, steps, cfg_strength, method=method, use_mask=use_mask,
                                     return_trajectory=return_trajectory, use_graph=use_graph, defer_guard=defer_guard,
                                     cond_mask=None if edit_mask is None else cond_mask.squeeze(-1))
            out = out.to(step_cond.dtype)
        else:
            out, trajectory = self._sample_python(step_cond, cond, cond_mask, text, mask, y0, t, cfg_strength, method, return_trajectory)
        self.transformer.clear_cache()

        if exists(vocoder):
            out = out.permute(0, 2, 1)
            out = vocoder(out)
        return out, trajectory

    @torch.no_grad()
    def sample_ragged(self, cond, texts, durations, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None, seed=None,
                      max_duration=4096, y0s=None, noise_device=None, use_graph="auto", edit_masks=None):
        """``sample()`` for several texts over ONE prompt, each with its own duration, in one set of kernel launches without padding the
        utterances to a common length (libf5hip ``f5_sample_ragged``).  Equivalent to ``[sample(cond, [t], d)[0] for t, d in zip(texts,
        durations)]`` -- the reference's batch-1 arithmetic per utterance (cfm.py:82-208 with batch = 1: no key mask), noise drawn in the
        same order -- and returns that list ([1, N_i, mel] each).  cond: mel [1, nc, mel] or raw wave [1, nw] (one prompt for every text), or
        [B, nc, mel] with ``lens`` (a prompt per utterance, zero-padded to a common nc as for ``sample()``); texts: list of str / list of token
        lists / id tensor; durations: list of ints.
        Independent requests in one batch (libf5hip ``f5_sample_ragged_ex``): ``cfg_strength`` may be a sequence with one float per utterance
        -- utterance i then equals ``sample(..., cfg_strength=cfg_strength[i])``; a sequence that mixes values below 1e-5 (the reference's
        single-pass branch, cfm.py:167) with guided ones raises ``ValueError`` before any library call.  ``edit_masks``: one bool tensor
        ([n] or [1, n]) or None per utterance, combined with the prompt prefix as ``sample(edit_mask=...)`` does.  ``y0s``: explicit noise
        per utterance; an entry that is None is drawn here, in order."""
        method = ode_method(self.odeint_kwargs)
        self.eval()
        native = getattr(self.transformer, "native_sample_ragged", None)
        if native is None:
            raise NotImplementedError("the backbone has no ragged sampler")
        if not isinstance(cfg_strength, (int, float)):
            cfg_strength = [float(c) for c in (cfg_strength.tolist() if torch.is_tensor(cfg_strength) else cfg_strength)]
            if len(cfg_strength) != len(texts):
                raise ValueError(f"cfg_strength holds {len(cfg_strength)} values for {len(texts)} utterances")
            if len({c >= 1e-5 for c in cfg_strength}) > 1:
                raise ValueError("cfg_strength mixes values below 1e-5 (single pass, cfm.py:167) with guided ones: sample them in separate calls")
        if edit_masks is not None and len(edit_masks) != len(texts):
            raise ValueError(f"edit_masks holds {len(edit_masks)} entries for {len(texts)} utterances")
        if cond.ndim == 2:  # raw wave
            cond = self.mel_spec(cond).permute(0, 2, 1)
        cond = cond.to(next(self.parameters()).dtype)
        nutt = len(texts)
        assert cond.shape[0] in (1, nutt) and cond.shape[-1] == self.num_channels
        cond_seq_len, device = cond.shape[1], cond.device
        if not exists(lens):
            lens = torch.full((nutt,), cond_seq_len, device=device, dtype=torch.long)
        if isinstance(texts, torch.Tensor):  # token ids [B, nt], -1 padded
            text = texts.to(device)
        elif len(texts) and isinstance(texts[0], torch.Tensor):  # one id row per utterance
            text = pad_sequence([x.reshape(-1) for x in texts], padding_value=-1, batch_first=True).to(device)
        elif exists(self.vocab_char_map):
            text = list_str_to_idx(list(texts), self.vocab_char_map).to(device)
        else:
            text = list_str_to_tensor(list(texts)).to(device)
        duration = torch.tensor([int(d) for d in durations], device=device, dtype=torch.long)
        duration = torch.maximum(torch.maximum((text != -1).sum(dim=-1), lens) + 1, duration).clamp(max=max_duration)  # cfm.py:127-131
        frames = [int(d) for d in duration]
        conds, noises = [], []
        ndev = default(default(noise_device, self.noise_device), self.device)
        for i, n in enumerate(frames):
            conds.append(F.pad(cond[i if cond.shape[0] > 1 else 0], (0, 0, 0, n - cond_seq_len), value=0.0))
            if y0s is not None and y0s[i] is not None:
                noises.append(y0s[i].reshape(n, self.num_channels).to(device=device, dtype=cond.dtype))
            else:
                if exists(seed):
                    torch.manual_seed(seed)
                noises.append(torch.randn(n, self.num_channels, device=ndev, dtype=cond.dtype).to(device))
        t = torch.linspace(0, 1, steps + 1, device=self.device, dtype=cond.dtype)
        if sway_sampling_coef is not None:
            t = t + sway_sampling_coef * (torch.cos(torch.pi / 2 * t) - 1 + t)
        extra = {}
        if edit_masks is not None and any(m is not None for m in edit_masks):
            # cond_mask of sample(): lens_to_mask(lens) & edit_mask, False-padded to the utterance's frames -- per utterance, back to back
            rows = []
            for i, n in enumerate(frames):
                prefix = torch.arange(n, device=device) < lens[i]
                if edit_masks[i] is not None:
                    em = edit_masks[i].reshape(-1).to(device=device, dtype=torch.bool)
                    prefix = prefix & F.pad(em[:n], (0, max(0, n - em.numel())), value=False)
                rows.append(prefix)
            extra["cond_mask"] = torch.cat(rows)
        out = native(torch.cat(conds), text, lens, frames, torch.cat(noises), t, steps, cfg_strength, method=method,
                     use_graph=use_graph, **extra)
        self.transformer.clear_cache()
        return [o.unsqueeze(0).to(cond.dtype) for o in torch.split(out, frames)]

    def _sample_python(self, step_cond, cond, cond_mask, text, mask, y0, t, cfg_strength, method, return_trajectory):
        """Generic driver over ``transformer(...)`` calls (non-native backbones, edit_native=False): the fixed-grid steps of ODE_METHODS."""
        def fn(tt, x):
            pred = self.transformer(x=x, cond=step_cond, text=text, time=tt, mask=mask, drop_audio_cond=False, drop_text=False, cache=True)
            if cfg_strength < 1e-5:
                return pred
            null_pred = self.transformer(x=x, cond=step_cond, text=text, time=tt, mask=mask, drop_audio_cond=True, drop_text=True, cache=True)
            return pred + (pred - null_pred) * cfg_strength

        if method not in ODE_METHODS:
            raise ValueError(f"unsupported ODE method {method!r}: the fixed-grid solvers are {sorted(ODE_METHODS)}")
        step = ODE_METHODS[method]
        y, traj = y0, [y0]
        for t0, t1 in zip(t[:-1], t[1:]):
            y = y + step(fn, t0, t1, y)
            if return_trajectory:
                traj.append(y)
        out = torch.where(cond_mask, cond, y)
        return out, (torch.stack(traj) if return_trajectory else None)
