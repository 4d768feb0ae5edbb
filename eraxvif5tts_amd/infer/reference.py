"""The reference-voice front-end on the device (csrc/reference.hip): clip, trim, pad, mono mix and rms boost of `F5TTSWrapper._preprocess_voice`
without the host's Python window loops.  The rule is `audio.clip_reference` / `audio.remove_silence_edges` / `Segment.silent_like` /
`audio.segment_to_float`, sample for sample; the one stated difference is the rms the boost divides by (`prepare_reference_device`)."""
from __future__ import annotations

import numpy as np
import torch

from . import audio as _audio

# what f5tts_wrapper.py:256-379 passes to pydub
REFERENCE_RULE = dict(passes=((1000, -50), (100, -40)), keep_silence=1000, seek_step=10, soft_limit_ms=6000, hard_limit_ms=12000,
                      silence_threshold=-42, lead_chunk_ms=10, pad_ms=50)
CLIP_MESSAGES = ("Audio is over 12s, clipping short. (1)", "Audio is over 12s, clipping short. (2)", "Audio is over 12s, clipping short. (3)")


def device_route_takes(seg):
    """16-bit samples (IEEE-float files arrive as such), one or two channels, a millisecond that holds a frame, fewer than 2^31 samples"""
    n, ch = seg.samples.shape
    return seg.sample_width == 2 and ch in (1, 2) and seg.frame_rate >= 1000 and n * ch < 2 ** 31


def make_rule(clip_short=True, target_rms=0.1, *, passes=REFERENCE_RULE["passes"], keep_silence=1000, seek_step=10, soft_limit_ms=6000,
              hard_limit_ms=12000, silence_threshold=-42, lead_chunk_ms=10, pad_ms=50, edge_integers=None):
    """struct f5_reference_rule: the thresholds go in as the integers `audio.silence_threshold_floor` / `audio.edge_threshold_integers` give
    (``edge_integers``: the pair itself, for tests)"""
    from .. import _lib
    (len1, db1), (len2, db2) = passes
    r_lead, r_trail = edge_integers if edge_integers is not None else _audio.edge_threshold_integers(silence_threshold)
    return _lib.ReferenceRule(int(bool(clip_short)), int(len1), _audio.silence_threshold_floor(db1), int(len2), _audio.silence_threshold_floor(db2),
                              int(keep_silence), int(seek_step), int(soft_limit_ms), int(hard_limit_ms), int(r_lead), int(r_trail),
                              int(lead_chunk_ms), int(pad_ms), float(target_rms))


class _Call:
    """the buffers of one clip: the uploaded PCM, workspace, table and counts"""

    def __init__(self, pcm, sample_rate, rule):
        from .. import _lib
        import ctypes as C
        self.lib, self._lib = _lib.load(), _lib
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 2 and pcm.is_contiguous()
        self.pcm, self.rate, self.rule = pcm, int(sample_rate), rule
        self.n, self.ch = pcm.shape
        self.rule_p = C.byref(rule)
        need = self.lib.f5_reference_prepare_workspace(self.n, self.ch, self.rate, self.rule_p)
        if need < 0:
            _lib.check(int(need), "reference_prepare_workspace")
        rows = int(self.lib.f5_reference_table_rows(self.n, self.ch, self.rate, self.rule_p))
        dev = pcm.device
        self.ws = torch.empty(max(int(need), 16), device=dev, dtype=torch.uint8)
        self.table = torch.zeros(rows, 3, device=dev, dtype=torch.int32)
        self.counts = torch.zeros(_lib.F5_REF_WORDS, device=dev, dtype=torch.int64)
        self.pad_frames = int(rule.pad_ms * (self.rate / 1000.0))

    def _head(self):
        return (self._lib.ptr(self.pcm) if self.n else None, self.n, self.ch, self.rate, self.rule_p)

    def plan(self):
        rc = self.lib.f5_op_reference_plan(*self._head(), self._lib.ptr(self.ws), self.ws.numel(), self._lib.ptr(self.table),
                                           self._lib.ptr(self.counts), self._lib.stream_ptr())
        self._lib.check(rc, "op_reference_plan")

    def read(self):
        """counts and table in ONE device -> host copy: ``(dict of the counts, table rows [parts, 3] as numpy)``"""
        both = torch.cat([self.counts, self.table.reshape(-1).to(torch.int64)]).cpu().numpy()
        rec = {k: int(v) for k, v in zip(self._lib.REF_WORDS, both)}
        return rec, both[self._lib.F5_REF_WORDS:].reshape(-1, 3)[:rec["parts"]]

    def out_frames(self, rec, cut_ms):
        """frames of slice_ms(0, cut_ms) of the edge segment, and with the pad"""
        n2 = rec["edge_ms"]
        end = cut_ms if cut_ms >= 0 else n2 + cut_ms
        kept = min(int(min(max(end, 0), n2) * (self.rate / 1000.0)), rec["edge_frames"])
        return kept, kept + self.pad_frames

    def prepare(self, cut_ms, out_frames, planned=True, want_pcm=False):
        dev = self.pcm.device
        wave = torch.empty(max(out_frames, 1), device=dev, dtype=torch.float32)
        ints = torch.empty(max(out_frames, 1), self.ch, device=dev, dtype=torch.int16) if want_pcm else None
        rc = self.lib.f5_reference_prepare(*self._head(), int(bool(planned)), int(cut_ms), self._lib.ptr(self.ws), self.ws.numel(),
                                           self._lib.ptr(self.table), self._lib.ptr(self.counts), int(out_frames), self._lib.ptr(wave),
                                           self._lib.ptr(ints), self._lib.stream_ptr())
        self._lib.check(rc, "reference_prepare")
        return wave[:out_frames], (ints[:out_frames] if want_pcm else None)


def reference_plan(pcm, sample_rate, rule):
    """``f5_op_reference_plan``: the decision alone for int16 PCM ``[n, ch]`` on the GPU -> ``(record, table)`` as host numbers (this copies):
    the counts by name (`_lib.REF_WORDS`) and the rows ``(first frame, end frame, position)`` of the gathered parts, before the edges."""
    call = _Call(pcm, sample_rate, rule)
    call.plan()
    return call.read()


def prepare_reference_device(seg_or_path, clip_short=True, target_rms=0.1, show_info=print, *, device="cuda", rule=None, want_pcm=False,
                             unboosted=False):
    """The host steps of `F5TTSWrapper._preprocess_voice` on the device -> ``(audio fp32 [1, n] on the device, sample_rate, record)``: one upload
    of the clip's int16 PCM, `f5_op_reference_plan`, a small device -> host read (the counts and the part table, O(parts) bytes; it carries
    the silent trailing milliseconds the host's `end -= 0.001` loop needs, the clip flags for the messages, and the output's size), then
    `f5_reference_prepare` on the plan's workspace, and a second read of the same block behind it for the record (the sum of squares, rms32,
    whether the boost applied).  TWO reads per voice, neither of samples.

    ``record``: ``ranges`` (the ``(first, end)`` sample ranges of the clip whose concatenation is the result before the pad -- equal to
    `audio.reference_sample_ranges`), ``messages``, ``lead_ms``, ``trail_ms``, ``kept``, ``out_frames``, ``sumsq``, ``rms32`` (numpy float32),
    ``boost`` and the other counts of f5hip.h.  With ``want_pcm`` also ``pcm`` (int16 ``[n, ch]`` on the device: the integers before the float
    conversion); with ``unboosted`` the target is 0, so nothing is boosted (the wave as converted).

    The rms: the host route divides by torch's fp32 ``sqrt(mean(square(audio)))``, whose summation order is torch's own.  Here it is
    ``rms32 = float32(sqrt(S / (ch^2 * 32768^2 * n)))`` from the exact integer sum of squares S of the mono wave (pad included), fp64 inside;
    the boost, when ``rms32 < float32(target_rms)``, is ``(x * float32(target_rms)) / rms32`` per sample, the host's two fp32 operations."""
    seg = seg_or_path if isinstance(seg_or_path, _audio.Segment) else _audio.Segment.from_file(seg_or_path)
    if not device_route_takes(seg):
        raise ValueError(f"the device route takes 16-bit samples in 1 or 2 channels at 1000 Hz or more (width {seg.sample_width}, "
                         f"{seg.samples.shape[1]} channels, {seg.frame_rate} Hz given)")
    if rule is None:
        rule = make_rule(clip_short, 0.0 if unboosted else target_rms)
    pcm = torch.from_numpy(np.ascontiguousarray(seg.samples, dtype=np.int16)).to(device)
    call = _Call(pcm, seg.frame_rate, rule)
    call.plan()
    rec, table = call.read()
    messages = [m for bit, m in enumerate(CLIP_MESSAGES) if rec["clip"] >> bit & 1]
    for m in messages:
        show_info(m)
    cut_ms = _audio.trailing_cut_ms(rec["edge_frames"], seg.frame_rate, rec["trail_ms"])
    kept, total = call.out_frames(rec, cut_ms)
    wave, ints = call.prepare(cut_ms, total, planned=True, want_pcm=want_pcm)
    late, _ = call.read()
    assert late["kept"] == kept and late["out_frames"] == total, (late, kept, total)
    rec.update({k: late[k] for k in ("kept", "out_frames", "sumsq", "boost", "rms_bits")})
    rec["rms32"] = np.array([rec["rms_bits"]], np.uint32).view(np.float32)[0]
    rec["cut_ms"], rec["messages"] = cut_ms, messages
    rec["ranges"] = _audio.cut_sample_ranges([(int(a), int(b)) for a, b, _ in table], rec["lead_frame"], kept)
    if want_pcm:
        rec["pcm"] = ints
    return wave.reshape(1, -1), seg.frame_rate, rec
