"""Host logic of the device wave tail (no GPU): `utils_infer.plan_wave_tail` -- the extents planning behind `f5_wave_finish` -- against what
`cross_fade_concat` and `pcm16_bytes` actually do to numpy arrays of those lengths: where every wave lands, the n of each joint (the reference's
sequential rule), the total length, and the rule that picks float32 or float64 for the result and for the PCM product.  Also the row planning
of `mel_rows_of` and the duck-typing of the streaming front-end."""
import numpy as np
import pytest
import torch

from eraxvif5tts_amd.infer.utils_infer import cross_fade_concat, mel_rows_of, plan_wave_tail
from eraxvif5tts_amd.streaming.wire import pcm16_bytes, process_chunk

SR = 24000
CASES = [
    ([10000, 8000], 0.15),                 # the usual joint: n = 3600
    ([10000, 8000, 9000, 7300, 20000], 0.15),
    ([10000], 0.15),                       # one wave: nothing to join, float32
    ([10000, 8000, 9000], 0.0),            # cross-fade off: plain concatenation, float32
    ([10000, 8000, 9000], -1.0),
    ([10000, 8000], 1 / 24000),            # n = 1
    ([10000, 8000, 5], 1e-6),              # int(d * rate) = 0: joints of n = 0, float32
    ([100, 8000], 0.15),                   # first wave shorter than n: n = 100 at that joint
    ([10000, 2000, 9000], 0.15),           # middle wave shorter than n: n = 2000, then min(3600, len(final)) again
    ([10000, 5000, 9000], 0.15),           # middle wave between n and 2 n: both joints take 3600 but the second reaches the first's mix
    ([300, 200, 100, 50, 4000], 0.15),     # a chain of short waves
    ([3600, 7200, 3600], 0.15),            # exactly at the device rule's limit
    ([3600, 7199, 3600], 0.15),            # one sample below it
]


def _waves(lengths, seed=0):
    g = np.random.default_rng(seed)
    return [g.uniform(-0.99, 0.99, n).astype(np.float32) for n in lengths]


@pytest.mark.parametrize("lengths,d", CASES)
def test_plan_matches_cross_fade_concat(lengths, d):
    waves = _waves(lengths)
    ref = cross_fade_concat(waves, d)
    plan = plan_wave_tail(lengths, d, SR)
    assert plan["total"] == len(ref)
    assert plan["dtype"] == ref.dtype and plan["mixed"] == (ref.dtype == np.float64)
    # the n of every joint, restated from the reference's loop on the arrays themselves
    final, joints = waves[0], []
    for nxt in waves[1:]:
        n = min(int(d * SR), len(final), len(nxt)) if d > 0 else 0
        joints.append(max(n, 0))
        final = cross_fade_concat([final, nxt], d)
    assert plan["joints"] == joints and len(final) == plan["total"]
    # where each wave lands: its first sample past its own fade-in is the wave's own value, unless a later joint mixed it again
    for k, (off, w) in enumerate(zip(plan["out_offsets"], waves)):
        n_in = joints[k - 1] if k else 0
        n_out = joints[k] if k < len(joints) else 0
        if n_in + n_out < len(w) and plan["device_ok"]:
            assert ref[off + n_in] == w[n_in]
            assert np.array_equal(ref[off + n_in: off + len(w) - n_out], w[n_in: len(w) - n_out].astype(ref.dtype))


@pytest.mark.parametrize("lengths,d", CASES)
def test_device_rule_is_the_no_chaining_rule(lengths, d):
    """device_ok exactly when every joint takes the full n = int(d * rate) from untouched samples on both sides, i.e. when a kernel that
    mixes each joint independently reproduces the sequential host loop; restated here as that independent mix on numpy arrays."""
    plan = plan_wave_tail(lengths, d, SR)
    n, B = plan["n"], len(lengths)
    expect_ok = all(length >= (n if i in (0, B - 1) else 2 * n) for i, length in enumerate(lengths))
    assert plan["device_ok"] == expect_ok
    if not plan["device_ok"]:
        return
    assert all(j == n for j in plan["joints"])
    waves = _waves(lengths, seed=1)
    ref = cross_fade_concat(waves, d)
    out = np.zeros(plan["total"], dtype=plan["dtype"])
    pos = 0
    for k, w in enumerate(waves):  # one pass, every output sample written once from the two waves it depends on
        assert pos == plan["out_offsets"][k]
        body_end = len(w) - (n if k < B - 1 else 0)
        if k and n:
            out[pos: pos + n] = waves[k - 1][-n:] * np.linspace(1, 0, n) + w[:n] * np.linspace(0, 1, n)
        start = n if k else 0
        out[pos + start: pos + body_end] = w[start: body_end]
        pos += body_end
    assert np.array_equal(out, ref) and out.dtype == ref.dtype
    assert pcm16_bytes(out) == pcm16_bytes(ref)


def test_pcm_precision_follows_the_promotion():
    """pcm16_bytes multiplies in the array's own precision: float64 after a mixed joint, float32 otherwise -- and the two differ on some
    samples, so the device kernel has to pick the one the host path would have used (plan['mixed'])."""
    g = np.random.default_rng(5)
    w = g.uniform(-0.99, 0.99, 200000).astype(np.float32)
    p32 = np.frombuffer(pcm16_bytes(w), np.int16)
    p64 = np.frombuffer(pcm16_bytes(w.astype(np.float64)), np.int16)
    assert (w * 32767).dtype == np.float32 and (p32 != p64).any() and np.abs(p32.astype(int) - p64.astype(int)).max() == 1
    assert not plan_wave_tail([len(w)], 0.15)["mixed"] and plan_wave_tail([len(w), 5000], 0.15)["mixed"]
    assert not plan_wave_tail([len(w), 5000], 0.0)["mixed"]
    joined = cross_fade_concat([w, w[:5000]], 0.15)
    assert joined.dtype == np.float64 and np.array_equal(np.frombuffer(pcm16_bytes(joined), np.int16)[:1000], p64[:1000])


def test_mel_rows_of_views_and_copies():
    mel, skip = 100, 7
    frames = [20, 9, 33]
    buf = torch.randn(sum(frames) + 4, mel)
    views = [v.unsqueeze(0) for v in torch.split(buf[2: 2 + sum(frames)], frames)]  # views of one buffer, as the ragged sampler returns them
    rows, start, T = mel_rows_of(views, skip)
    assert rows.data_ptr() == buf.data_ptr() and T == [f - skip for f in frames]  # taken as it is: no copy
    for v, s, t in zip(views, start, T):
        assert torch.equal(rows[s: s + t], v[0, skip:])
    separate = [v.clone() for v in views]  # tensors of their own: concatenated once, prompt frames dropped
    rows, start, T = mel_rows_of(separate, skip)
    assert rows.shape == (sum(frames) - 3 * skip, mel) and start == [0, 13, 15]
    for v, s, t in zip(separate, start, T):
        assert torch.equal(rows[s: s + t], v[0, skip:])
    rows, _, _ = mel_rows_of([v.to(torch.bfloat16) for v in views], skip)
    assert rows.dtype == torch.float32


def test_process_chunk_asks_for_pcm16_only_where_offered():
    class Old:  # any object with the reference's generate(): floats, converted on the host
        def generate(self, text, return_numpy=False):
            return np.array([0.5, -0.25, 0.99997], np.float32), SR

    class New:  # an object that offers int16 itself
        asked = None

        def generate(self, text, return_numpy=False, return_pcm16=False):
            self.asked = return_pcm16
            return np.array([16383, -8191, 32766], np.int16), SR

    assert process_chunk("hi.", Old()) == pcm16_bytes(np.array([0.5, -0.25, 0.99997], np.float32))
    new = New()
    assert process_chunk("hi.", new) == np.array([16383, -8191, 32766], np.int16).tobytes() and new.asked is True
    assert process_chunk("   ", new) is None
