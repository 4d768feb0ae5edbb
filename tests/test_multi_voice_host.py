"""Host logic of multi-voice synthesis (no GPU): `utils_infer.split_voice_script` -- the reference's `[name]` tag rule -- on the scripts whose
cuts were worked out from the reference's two regular expressions; `plan_wave_tail_segments` against what
``np.concatenate([cross_fade_concat(seg) for seg in segments])`` does to numpy arrays of those lengths; `stream_emitted_counts` with segments;
`mel_rows_of` with one skip per utterance; and the C ABI's two new names in the header and the binding table."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

from eraxvif5tts_amd.infer.utils_infer import (cross_fade_concat, mel_rows_of, plan_wave_tail, plan_wave_tail_segments, split_voice_script,
                                               stream_emitted_counts)
from eraxvif5tts_amd.streaming.wire import pcm16_bytes

SR = 24000
N = 16
D = N / SR + 1e-9  # int(D * SR) == 16
VOICES = {"main": None, "town": None, "giọng_2": None}

SCRIPTS = [
    ("Hello there. [main] hi. [town] yo [ghost] boo", [("main", "Hello there."), ("main", "hi."), ("town", "yo"), ("main", "boo")]),
    ("[town][main] x", [("main", "x")]),
    ("  [town]   ", []),
    ("a [a-b] c [town]d", [("main", "a [a-b] c"), ("town", "d")]),
    ("[town] one [town] two", [("town", "one"), ("town", "two")]),
    ("x [Town] y", [("main", "x"), ("main", "y")]),
    (" [main]a[giọng_2]b", [("main", "a"), ("giọng_2", "b")]),
]


@pytest.mark.parametrize("script,want", SCRIPTS)
def test_split_voice_script(script, want):
    said = []
    assert split_voice_script(script, VOICES, show_info=said.append) == want
    assert all(m in ("No voice tag found, using main.",) or re.fullmatch(r"Voice \w+ not found, using main\.", m) for m in said)


def test_split_voice_script_says_what_the_reference_says():
    said = []
    split_voice_script("Hello there. [main] hi. [town] yo [ghost] boo", VOICES, show_info=said.append)
    assert said == ["No voice tag found, using main.", "Voice ghost not found, using main."]
    said.clear()
    split_voice_script("x [Town] y", VOICES, show_info=said.append)  # names are case-sensitive, as dict keys are
    assert said == ["No voice tag found, using main.", "Voice Town not found, using main."]


# ---------------------------------------------------------------------------------------------------------------- plan_wave_tail_segments
SEG_SIZES = [[1], [2], [1, 1, 1], [3, 1, 2], [1, 4]]
CHOICES = [N, 2 * N, 2 * N + 1, 3 * N + 7]


def _length_lists(B):
    """every list for B <= 3, and for longer lists 60 drawn ones plus the four constant ones"""
    if B <= 3:
        return [list(c) for c in itertools.product(CHOICES, repeat=B)]
    g = np.random.default_rng(B)
    return [[c] * B for c in CHOICES] + [[int(x) for x in g.choice(CHOICES, B)] for _ in range(60)]


def _segments(items, seg_sizes):
    out, k = [], 0
    for g in seg_sizes:
        out.append(items[k: k + g])
        k += g
    return out


def _rule(lengths, seg_sizes, n):
    """the chaining rule, restated: in a segment of two or more, end utterances hold n and inner ones 2 n; a segment of one holds anything"""
    for seg in _segments(lengths, seg_sizes):
        for i, length in enumerate(seg):
            if len(seg) >= 2 and length < (n if i in (0, len(seg) - 1) else 2 * n):
                return False
    return True


@pytest.mark.parametrize("seg_sizes", SEG_SIZES, ids=str)
def test_plan_segments_matches_numpy(seg_sizes):
    B = sum(seg_sizes)
    seen = set()
    for lengths in _length_lists(B):
        g = np.random.default_rng(sum(lengths))
        waves = [g.uniform(-0.99, 0.99, x).astype(np.float32) for x in lengths]
        parts = [cross_fade_concat(seg, D, SR) for seg in _segments(waves, seg_sizes)]
        ref = np.concatenate(parts)
        plan = plan_wave_tail_segments(lengths, seg_sizes, D, SR)
        assert plan["total"] == len(ref) and plan["dtype"] == ref.dtype
        assert (ref.dtype == np.float32) == (max(seg_sizes) == 1) and plan["mixed"] == (ref.dtype == np.float64)
        assert plan["seg_start"] == [1 if i == 0 else 0 for g_ in seg_sizes for i in range(g_)]
        assert plan["n"] == (N if max(seg_sizes) >= 2 else 0)
        # offsets and joints: each segment's own plan, moved behind the segments before it
        offsets, joints, base = [], [], 0
        for seg, part in zip(_segments(lengths, seg_sizes), parts):
            own = plan_wave_tail(seg, D, SR)
            offsets += [base + o for o in own["out_offsets"]]
            joints += ([0] if base else []) + own["joints"]
            base += len(part)
        assert plan["out_offsets"] == offsets and plan["joints"] == joints
        ok = _rule(lengths, seg_sizes, N)
        assert plan["device_ok"] == ok, (lengths, seg_sizes)
        seen.add(ok)
        if not ok:
            continue
        # what the device kernel does: every output sample written once, from at most two waves, a joint only inside a segment
        out = np.zeros(plan["total"], dtype=plan["dtype"])
        for k, w in enumerate(waves):
            n_in = 0 if plan["seg_start"][k] else N
            n_out = N if k + 1 < B and not plan["seg_start"][k + 1] else 0
            pos = plan["out_offsets"][k]
            if n_in:
                out[pos: pos + N] = waves[k - 1][-N:] * np.linspace(1, 0, N) + w[:N] * np.linspace(0, 1, N)
            out[pos + n_in: pos + len(w) - n_out] = w[n_in: len(w) - n_out]
        assert np.array_equal(out, ref) and pcm16_bytes(out) == pcm16_bytes(ref)
    assert True in seen and (False in seen) == (max(seg_sizes) >= 3)  # only an inner utterance can break the rule with these lengths


def test_plan_segments_with_one_segment_is_plan_wave_tail():
    for lengths, d in [([10000, 8000, 9000], 0.15), ([10000], 0.15), ([100, 8000], 0.15), ([3600, 7199, 3600], 0.15), ([5, 6], 0.0)]:
        a, b = plan_wave_tail(lengths, d, SR), plan_wave_tail_segments(lengths, [len(lengths)], d, SR)
        assert all(a[key] == b[key] for key in a)


@pytest.mark.parametrize("seg_sizes", [[3, 1, 2], [6], [1] * 6, [2, 2, 2], [1, 4, 1]], ids=str)
def test_stream_emitted_counts_with_segments(seg_sizes):
    lengths = [3 * N + 7, 2 * N, N, 5, 2 * N + 1, N]
    if seg_sizes not in ([3, 1, 2], [1] * 6):  # (the 5-sample utterance is a segment of its own only in those two)
        lengths = [3 * N + 7, 2 * N, 2 * N + 1, 2 * N, 2 * N + 1, N]
    plan = plan_wave_tail_segments(lengths, seg_sizes, D, SR)
    assert plan["device_ok"]
    for cut in itertools.product([0, 1], repeat=5):  # a 1 at position i: a new push begins with utterance i + 1
        groups, size = [], 1
        for c in cut:
            if c:
                groups.append(size)
                size = 0
            size += 1
        groups.append(size)
        counts, dtype = stream_emitted_counts(lengths, groups, D, SR, segments=seg_sizes)
        assert sum(counts) == plan["total"] and dtype == plan["dtype"] and len(counts) == len(groups) and min(counts) >= 0
        k = 0
        for g, c in zip(groups, counts):  # a push that ends a segment (or the list) emits everything it was given
            k += g
            if k == len(lengths) or plan["seg_start"][k]:  # (the joint with the carry lands on samples this push emits)
                assert c == sum(lengths[k - g: k]) - N * sum(1 for i in range(k - g + 1, k) if not plan["seg_start"][i])
    assert stream_emitted_counts(lengths, [6], D, SR, segments=seg_sizes)[0] == [plan["total"]]


def test_mel_rows_of_takes_one_skip_per_utterance():
    mel, frames, skips = 100, [20, 9, 33], [7, 2, 11]
    buf = torch.randn(sum(frames) + 4, mel)
    views = [v.unsqueeze(0) for v in torch.split(buf[2: 2 + sum(frames)], frames)]
    rows, start, T = mel_rows_of(views, skips)
    assert rows.data_ptr() == buf.data_ptr() and T == [f - s for f, s in zip(frames, skips)]
    for v, s, t, k in zip(views, start, T, skips):
        assert torch.equal(rows[s: s + t], v[0, k:])
    rows, start, T = mel_rows_of([v.clone() for v in views], skips)
    assert rows.shape == (sum(T), mel) and start == [0, 13, 20]
    same, start1, T1 = mel_rows_of(views, 7)
    assert (start1, T1) == mel_rows_of(views, [7, 7, 7])[1:]
    with pytest.raises(AssertionError):
        mel_rows_of(views, [1, 2])


def test_segment_entry_points_are_declared_and_bound():
    from eraxvif5tts_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "f5hip.h")) as fh:
        header = fh.read()
    for name in ("f5_wave_finish_segments", "f5_wave_stream_create_segments"):
        assert re.search(r"F5_API\s+int\s+" + name + r"\s*\(", header) and name in _lib.EXPORTS
    assert re.search(r"#define F5HIP_VERSION 400\b", header)  # detected by symbol: the number stays
