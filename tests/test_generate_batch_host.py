"""Host side of `F5TTSWrapper.generate_batch` (no GPU): the sampler-group planner as a pure function, the C ABI entry it rests on, the
signature and `TTSJob`'s defaults, and the validation errors, which name the request's index."""
import dataclasses
import inspect
import os
import random
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_request_groups_over_random_lists():
    from eraxvif5tts_amd.infer.utils_infer import chunk_groups, plan_request_groups
    rng = random.Random(5)
    for trial in range(300):
        n = rng.randint(1, 40)
        keys = [(rng.choice([2, 3, 32]), rng.choice([-1.0, None, 0.5]), rng.random() < 0.7) for _ in range(n)]
        durations = [rng.choice([120, 256, 300, 1100, 2047, 4096, 9000, 17000]) for _ in range(n)]
        group_max, max_rows = rng.choice([1, 2, 3, 8]), rng.choice([4096, 16384])
        groups = plan_request_groups(keys, durations, group_max, max_rows)
        assert sorted(i for g in groups for i in g) == list(range(n))          # every job in exactly one group
        seen = []
        for g in groups:
            assert len({keys[i] for i in g}) == 1                               # one key per group (so on / off guidance is never mixed)
            assert len({keys[i][2] for i in g}) == 1
            assert g == sorted(g)                                               # flat order inside a group
            assert len(g) <= group_max                                          # the caps; a job longer than the row cap stands alone
            assert sum(durations[i] for i in g) <= max_rows or len(g) == 1
            if keys[g[0]] not in seen:
                seen.append(keys[g[0]])
            assert keys[g[0]] == seen[-1]                                       # a key's groups are consecutive ...
        first = []
        for k in keys:
            if k not in first:
                first.append(k)
        assert seen == first                                                    # ... and the keys come in order of first appearance
        for k in first:                                                         # inside a key: chunk_groups over its jobs, in flat order
            members = [i for i in range(n) if keys[i] == k]
            want = [[members[j] for j in g] for g in chunk_groups([durations[i] for i in members], 0, group_max, max_rows)]
            assert [g for g in groups if keys[g[0]] == k] == want
    assert plan_request_groups([], []) == []
    same = [(3, -1.0, True)] * 5
    assert plan_request_groups(same, [300] * 5) == chunk_groups([300] * 5) == [[0, 1, 2, 3, 4]]  # one key: generate()'s own groups


def test_the_new_entry_is_declared_and_exported():
    from eraxvif5tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    decl = re.search(r"F5_API\s+int\s+f5_sample_ragged_ex\s*\(([^;]*)\);", header)
    assert decl and "f5_sample_ragged_ex" in _lib.EXPORTS
    args = [a.strip() for a in decl[1].replace("\n", " ").split(",")]
    assert len(args) == 16 and len(_lib._PROTOS["f5_sample_ragged_ex"][1]) == 16
    assert args[7].startswith("const uint8_t* cond_mask") and args[12].startswith("const float* cfg_host")
    assert re.search(r"#define F5HIP_VERSION 400\b", header)  # detected by symbol: the number stays
    lib = _lib.load(build_if_missing=True)
    assert hasattr(lib, "f5_sample_ragged_ex") and lib.f5_version() == 400


def test_signature_and_ttsjob_defaults():
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper, TTSJob
    params = inspect.signature(F5TTSWrapper.generate_batch).parameters
    assert list(params) == ["self", "requests", "return_pcm16", "return_spectrogram"]
    assert params["return_pcm16"].default is False and params["return_spectrogram"].default is False
    fields = {f.name: f.default for f in dataclasses.fields(TTSJob)}
    assert list(fields) == ["text", "voice", "nfe_step", "cfg_strength", "sway_sampling_coef", "speed", "fix_duration", "cross_fade_duration",
                            "use_duration_predictor", "remove_silence", "seed"]
    assert fields["text"] is dataclasses.MISSING and fields["voice"] == "main" and fields["remove_silence"] is False
    assert all(fields[k] is None for k in fields if k not in ("text", "voice", "remove_silence"))
    assert inspect.signature(F5TTSWrapper.add_voice).parameters["speed"].default is None
    # the sampler's new parameters are keyword-only with defaults (existing callers pass today's arguments)
    from eraxvif5tts_amd.model import CFM, DiT
    assert inspect.signature(CFM.sample_ragged).parameters["edit_masks"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(CFM.sample_ragged).parameters["edit_masks"].default is None
    cm = inspect.signature(DiT.native_sample_ragged).parameters["cond_mask"]
    assert cm.kind is inspect.Parameter.KEYWORD_ONLY and cm.default is None


def _bare_wrapper():
    """a wrapper with one stored voice and nothing else: validation runs before anything that needs a model"""
    from eraxvif5tts_amd.infer.f5tts_wrapper import F5TTSWrapper
    w = F5TTSWrapper.__new__(F5TTSWrapper)
    w.ref_audio_processed = w.ref_text = w.ref_audio_len = None
    w._voices = {"town": dict(audio=torch.zeros(1, 48000), ref_text="a quiet horn. ", ref_audio_len=187, mel=torch.zeros(1, 188, 100),
                              rms=torch.tensor(0.1))}
    w.nfe_step, w.cfg_strength, w.sway_sampling_coef, w.speed, w.fix_duration = 32, 2.0, -1.0, 1.0, None
    w.cross_fade_duration, w.use_duration_predictor = 0.15, False
    w.model = types.SimpleNamespace(sample=lambda *a, **k: pytest.fail("sampled"), sample_ragged=lambda *a, **k: pytest.fail("sampled"))
    return w


def test_validation_errors_name_the_request():
    from eraxvif5tts_amd.infer.f5tts_wrapper import TTSJob
    w = _bare_wrapper()
    good = TTSJob("hello there.", voice="town")
    with pytest.raises(ValueError, match=r"request 1\b.*'main'"):
        w.generate_batch([good, TTSJob("hello there.")])  # "main" was never preprocessed
    with pytest.raises(ValueError, match=r"request 2\b.*empty text"):
        w.generate_batch([good, good, TTSJob("", voice="town")])
    with pytest.raises(ValueError, match=r"request 0\b.*nfe_step"):
        w.generate_batch([TTSJob("hello there.", voice="town", nfe_step=0), good])
    with pytest.raises(ValueError, match=r"request 1\b.*unknown fields \['tempo'\]"):
        w.generate_batch([good, dict(text="hello there.", voice="town", tempo=1.0)])
    with pytest.raises(ValueError, match=r"request 0\b"):
        w.generate_batch(["hello there."])
    with pytest.raises(ValueError, match="no requests"):
        w.generate_batch([])


def test_a_mixed_guidance_vector_is_refused_before_any_library_call():
    from eraxvif5tts_amd.model import CFM

    class Backbone(torch.nn.Module):
        dim = 8

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def native_sample_ragged(self, *a, **k):
            pytest.fail("the backbone was called")

    cfm = CFM(transformer=Backbone(), num_channels=100, mel_spec_kwargs={"mel_spec_type": "vocos"})
    cond, texts = torch.zeros(1, 10, 100), [torch.zeros(1, 4, dtype=torch.long)] * 3
    for bad in ([2.0, 0.0, 2.0], [0.0, 1e-5, 0.0], torch.tensor([1.0, 1.0, 1e-6])):
        with pytest.raises(ValueError, match="1e-5"):
            cfm.sample_ragged(cond, texts, [20, 20, 20], cfg_strength=bad)
    with pytest.raises(ValueError, match="2 values for 3"):
        cfm.sample_ragged(cond, texts, [20, 20, 20], cfg_strength=[2.0, 2.0])
    with pytest.raises(ValueError, match="edit_masks"):
        cfm.sample_ragged(cond, texts, [20, 20, 20], edit_masks=[None])
