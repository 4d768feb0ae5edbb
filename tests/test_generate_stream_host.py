"""Host logic of the streamed synthesis (no GPU): `utils_infer.chunk_groups` (which chunks form which piece), `utils_infer.stream_emitted_counts`
(how many samples each push of a wave stream emits, and in which dtype) against `plan_wave_tail`, and `streaming.wire.stream_audio` with
``stream_groups`` over a duck-typed model."""
import itertools

import numpy as np
import pytest

from eraxvif5tts_amd.infer.utils_infer import chunk_groups, plan_wave_tail, stream_emitted_counts
from test_gpu_wave_tail import LENGTHS, SR


def compositions(total):
    """every way to cut `total` utterances into consecutive groups: 2^(total-1) lists of group sizes"""
    out = []
    for cuts in itertools.product([0, 1], repeat=total - 1):
        sizes, run = [], 1
        for c in cuts:
            if c:
                sizes.append(run)
                run = 1
            else:
                run += 1
        out.append(sizes + [run])
    return out


# ---------------------------------------------------------------------------------------------------------------- grouping
def test_first_group_then_groups_of_ragged_chunks():
    d = [300] * 11
    assert chunk_groups(d, first=1, group_max=8) == [[0], list(range(1, 9)), [9, 10]]
    assert chunk_groups(d, first=3, group_max=4) == [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9, 10]]
    assert chunk_groups(d[:4], first=1, group_max=2) == [[0], [1, 2], [3]]
    # first = 0: the groups of generate()'s ragged sampler calls
    assert chunk_groups(d, first=0, group_max=8) == [list(range(8)), [8, 9, 10]]


def test_row_cap_and_order():
    d = [4000, 4000, 4000, 4000, 4000, 500, 4096, 4096, 4096, 4096, 300]
    groups = chunk_groups(d, first=1, group_max=8)
    assert groups == [[0], [1, 2, 3, 4], [5, 6, 7, 8], [9, 10]]
    assert [i for g in groups for i in g] == list(range(len(d)))  # order kept, nothing lost
    for g in groups[1:]:
        assert len(g) <= 8 and sum(d[i] for i in g) <= 16384
    assert sum(d[i] for i in groups[1]) + d[5] > 16384  # the cap is what closed group 1, not the count
    assert chunk_groups([20000, 100], first=0, group_max=8) == [[0], [1]]  # a chunk above the cap stands alone


def test_grouping_edge_cases():
    assert chunk_groups([300], first=1, group_max=8) == [[0]]
    assert chunk_groups([300], first=0, group_max=8) == [[0]]
    assert chunk_groups([300, 400, 500], first=3, group_max=8) == [[0, 1, 2]]
    assert chunk_groups([300, 400, 500], first=7, group_max=8) == [[0, 1, 2]]
    assert chunk_groups([], first=1, group_max=8) == []
    assert chunk_groups([300, 400, 500], first=1, group_max=0) == [[0], [1], [2]]  # ragged sampling off: one chunk per piece
    assert chunk_groups([300, 400], first=-2, group_max=8) == [[0, 1]]


def _loop_of_infer_batch_process(durations, group_max):
    """the grouping `infer_batch_process` carried as a loop of its own before it called `chunk_groups`, restated"""
    groups, i = [], 0
    while i < len(durations):
        group, rows = [], 0
        while i < len(durations) and len(group) < group_max and (not group or rows + durations[i] <= 16384):
            group.append(i)
            rows += durations[i]
            i += 1
        groups.append(group)
    return groups


def test_chunk_groups_is_the_loop_infer_batch_process_had():
    rng = np.random.default_rng(1234)
    lists = [[], [300], [16384], [16385], [20000, 100], [100, 20000, 100], [8192, 8192, 1], [8192, 8193], [4096] * 9]
    for _ in range(400):
        n = int(rng.integers(1, 25))
        d = [int(x) for x in rng.integers(256, 4097, n)]
        if rng.random() < 0.3:  # chunks above the row cap, which stand alone
            for k in rng.integers(0, n, int(rng.integers(1, 3))):
                d[int(k)] = int(rng.integers(16385, 40000))
        lists.append(d)
    assert sum(1 for d in lists if d and max(d) > 16384) >= 50
    for d in lists:
        for g in range(2, 10):
            assert chunk_groups(d, 0, g) == _loop_of_infer_batch_process(d, g), (d, g)


# ---------------------------------------------------------------------------------------------------------------- emitted counts
@pytest.mark.parametrize("d", [0.0, 0.15, 1 / 24000])
def test_emitted_counts_follow_the_plan(d):
    plan = plan_wave_tail(LENGTHS, d, SR)
    assert plan["device_ok"]
    bounds = plan["out_offsets"] + [plan["total"]]
    cuts = compositions(len(LENGTHS))
    assert len(cuts) == 16 and len({tuple(c) for c in cuts}) == 16
    for sizes in cuts:
        counts, dtype = stream_emitted_counts(LENGTHS, sizes, d, SR)
        assert len(counts) == len(sizes) and sum(counts) == plan["total"] and dtype == plan["dtype"]
        k = 0
        for size, count in zip(sizes, counts):
            # a push ending at utterance k + size - 1 emits up to where utterance k + size begins; the last push up to the end
            assert count == bounds[k + size] - bounds[k]
            k += size
    n = plan["n"]
    counts, _ = stream_emitted_counts(LENGTHS, [1, 1, 1, 1, 1], d, SR)
    assert counts == [LENGTHS[0] - n, LENGTHS[1] - n, LENGTHS[2] - n, LENGTHS[3] - n, LENGTHS[4]]


def test_dtype_is_the_streams_not_the_pushs():
    assert stream_emitted_counts([9000, 8000], [1, 1], 0.15, SR) == ([9000 - 3600, 8000], np.float64)  # the first push mixes nothing: float64 still
    assert stream_emitted_counts([9000, 8000], [1, 1], 0.0, SR) == ([9000, 8000], np.float32)
    assert stream_emitted_counts([9000], [1], 0.15, SR) == ([9000], np.float32)  # one utterance: no joint, float32, all of it
    assert stream_emitted_counts([3600, 7200, 3600], [1, 1, 1], 0.15, SR) == ([0, 3600, 3600], np.float64)  # a first push may emit nothing
    with pytest.raises(AssertionError):
        stream_emitted_counts([9000, 8000], [1], 0.15, SR)


# ---------------------------------------------------------------------------------------------------------------- stream_audio
class FakeStreamingModel:
    """duck-typed wrapper: generate() one block per text, generate_stream() the same samples in pieces of 3"""
    target_sample_rate = SR
    device = "cpu"

    def __init__(self):
        self.ref_audio_processed = self.ref_text = self.ref_audio_len = None
        self.calls, self.closed = [], 0

    def _pcm(self, text):
        assert self.ref_text == "a voice. "
        return (np.arange(len(text), dtype=np.int16) + ord(text[0])) * 3

    def generate(self, text, return_numpy=False, return_pcm16=False, **kw):
        self.calls.append(("generate", text, kw))
        assert return_pcm16
        return self._pcm(text), SR

    def generate_stream(self, text, return_pcm16=False, **kw):
        self.calls.append(("generate_stream", text, kw))
        assert return_pcm16
        pcm = self._pcm(text)
        try:
            for i in range(0, len(pcm), 3):
                yield pcm[i: i + 3], SR
        finally:
            self.closed += 1


class FakeBlockModel(FakeStreamingModel):
    generate_stream = None  # (no such method: attribute lookups give None, not a callable)


def _cache():
    from eraxvif5tts_amd.streaming.wire import ReferenceCache
    cache = ReferenceCache()
    cache.entries["spk"] = {"loaded": True, "processed_mel": np.zeros(4), "processed_text": "a voice. ", "processed_mel_len": 7}
    return cache


def test_stream_audio_yields_header_and_every_piece():
    from eraxvif5tts_amd.streaming.wire import create_wave_header, stream_audio
    chunks = ["hello..", "   ", "and more"]
    model = FakeStreamingModel()
    blocks = list(stream_audio(model, _cache(), "spk", chunks, nfe_step=3))
    assert [c[0] for c in model.calls] == ["generate", "generate"] and len(blocks) == 3  # the default: one block per text chunk
    model = FakeStreamingModel()
    parts = list(stream_audio(model, _cache(), "spk", chunks, stream_groups=True, nfe_step=3))
    assert parts[0] == create_wave_header(SR) == blocks[0]
    assert model.calls == [("generate_stream", "hello.", {"nfe_step": 3}), ("generate_stream", "and more", {"nfe_step": 3})]
    assert len(parts) == 1 + 2 + 3 and all(len(p) <= 6 for p in parts[1:])  # 6 and 8 samples in pieces of 3
    assert b"".join(parts) == b"".join(blocks)
    assert model.closed == 2 and model.ref_audio_processed is None and model.ref_text is None


def test_stream_audio_without_generate_stream_keeps_the_default():
    from eraxvif5tts_amd.streaming.wire import stream_audio
    a, b = FakeBlockModel(), FakeBlockModel()
    plain = list(stream_audio(a, _cache(), "spk", ["hello.", "and more"]))
    asked = list(stream_audio(b, _cache(), "spk", ["hello.", "and more"], stream_groups=True))
    assert asked == plain and len(asked) == 3 and [c[0] for c in b.calls] == ["generate", "generate"]


def test_stream_audio_closed_early_clears_the_reference_state():
    from eraxvif5tts_amd.streaming.wire import stream_audio
    model = FakeStreamingModel()
    stream = stream_audio(model, _cache(), "spk", ["hello there", "never reached"], stream_groups=True)
    next(stream)  # header
    next(stream)  # first piece of the first text
    assert model.ref_text == "a voice. " and model.closed == 0
    stream.close()
    assert model.ref_audio_processed is None and model.ref_text is None and model.ref_audio_len is None
    assert model.closed == 1 and len(model.calls) == 1  # the model's generator was closed too; the second text never started
