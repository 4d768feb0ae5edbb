"""Host side of the duration-validation path: the numpy restatement of the two alignment searches (tests/alignment_ref.py) against the
matrices captured from the reference (tests/golden/alignment.npz, tools/capture_alignment_golden.py), the C ABI's new names, and the
alignment-method schedule against transitions worked out by hand.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import alignment_ref as R
from conftest import ROOT, load_golden

NEW_SYMBOLS = ("f5_align_similarity", "f5_align_workspace", "f5_align_viterbi", "f5_align_window", "f5_duration_loss")


@pytest.fixture(scope="module")
def cases():
    return R.golden_cases(load_golden("alignment"))


def test_fixture_covers_the_generated_cases(cases):
    gen = R.generate_cases()
    assert list(cases) == list(gen)
    for name, (sim, _) in cases.items():
        assert sim.dtype == np.float32 and np.array_equal(sim.view(np.int32), gen[name].view(np.int32)), name
    shapes = {name: sim.shape for name, (sim, _) in cases.items()}
    assert any(s[1] == 1 for s in shapes.values()) and any(s[2] == 1 for s in shapes.values())
    assert any(s[1] > s[2] for s in shapes.values()) and any(s[1] > 256 for s in shapes.values()) and (1, 200, 1500) in shapes.values()


def test_restatement_equals_the_reference_exactly(cases):
    compared = 0
    for name, (sim, want) in cases.items():
        for alg in R.ALGORITHMS:
            if want[alg] is None:  # the reference raised: only its window search does, and only on an empty search window
                assert alg == "window" and R.window_has_empty_search(sim) and sim.shape[1] > sim.shape[2], (name, alg)
                continue
            assert not (alg == "window" and R.window_has_empty_search(sim)), name
            got = R.SEARCH[alg](sim)
            assert got.dtype == np.float32 and np.array_equal(got, want[alg]), (name, alg)
            compared += 1
    assert compared > len(cases)  # every viterbi case and every window case the reference could run


def test_every_column_has_one_owner(cases):
    for name, (sim, _) in cases.items():
        for alg in R.ALGORITHMS:
            a = R.SEARCH[alg](sim)
            assert np.array_equal(a.sum(axis=1), np.ones((sim.shape[0], sim.shape[2]), np.float32)), (name, alg)


def test_kept_quirk_padded_rows_take_the_utterance(cases):
    """An utterance with fewer phonemes than the padded batch gives its whole length to the last, all -inf row (viterbi)."""
    sim, want = cases["ragged"]
    d = R.viterbi(sim).sum(axis=2)
    assert d[1].tolist() == [0] * 6 + [33] and d[2].tolist() == [0] * 6 + [33]
    assert np.array_equal(d, want["viterbi"].sum(axis=2))
    assert R.viterbi(np.zeros((1, 5, 12), np.float32)).sum(axis=2).tolist() == [[0, 0, 0, 0, 12]]  # constant 0: no positive gradient


def test_header_and_bindings_name_the_new_entry_points():
    from eraxvif5tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"F5_API\s+\w+\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name


def test_unbuilt_algorithms_raise_value_error():
    from eraxvif5tts_amd.model.alignment_utils import ALGORITHMS, alignment_durations, monotonic_alignment_search
    assert ALGORITHMS == ("viterbi", "window")
    for alg in ("progressive", "dtw", ""):
        with pytest.raises(ValueError, match="'viterbi', 'window'"):
            monotonic_alignment_search(torch.zeros(1, 2, 3), algorithm=alg)
        with pytest.raises(ValueError, match="'viterbi', 'window'"):
            alignment_durations(torch.zeros(1, 2, 3), alg)


def test_get_durations_from_alignment_is_the_row_sum():
    from eraxvif5tts_amd.model.alignment_utils import get_durations_from_alignment
    a = torch.tensor([[[1., 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]])
    assert get_durations_from_alignment(a).tolist() == [[2.0, 1.0, 1.0]]


def test_schedule_matches_hand_computed_transitions():
    from eraxvif5tts_amd.model.alignment_utils import AlignmentMethodManager, get_alignment_method
    m = AlignmentMethodManager()
    assert (m.phase, m.current_method) == (1, "window") and m.set_steps_per_epoch(100) == 1000
    # phase 1: window, weight 0.5, whatever the epoch says
    method, logs = get_alignment_method(m, 10, duration_focus_updates=50, current_epoch=7)
    assert method == "window" and logs == {"phase": 1, "method": "window", "duration_weight": 0.5}
    # update 50 reaches the threshold: phase 2 in the same call, still window at epoch 2; no phase2_start_update yet -> 0.5
    method, logs = get_alignment_method(m, 50, duration_focus_updates=50, current_epoch=2)
    assert method == "window" and m.phase == 2 and logs["phase"] == 1 and logs["phase_transition"] is True
    assert "method_switch" not in logs and logs["duration_weight"] == 0.5
    # epoch 2, 250 steps into phase 2: 0.1 + 0.4 * 0.5 * (1 + cos(pi / 4))
    method, logs = get_alignment_method(m, 300, duration_focus_updates=50, phase2_start_update=50, current_epoch=2)
    assert method == "window" and "phase_transition" not in logs
    assert logs["duration_weight"] == pytest.approx(0.1 + 0.2 * (1 + math.sqrt(0.5)), rel=1e-12)
    # no epoch given: no switch
    assert get_alignment_method(m, 400, 50, phase2_start_update=50)[0] == "window"
    # epoch 3: viterbi from this call on; 500 steps in = half way: 0.1 + 0.4 * 0.5 = 0.3
    method, logs = get_alignment_method(m, 550, duration_focus_updates=50, phase2_start_update=50, current_epoch=3)
    assert method == "viterbi" and logs["method"] == "window" and logs["method_switch"] is True
    assert logs["duration_weight"] == pytest.approx(0.3, rel=1e-12)
    # it stays; past the decay the weight rests at 0.1
    method, logs = get_alignment_method(m, 5000, duration_focus_updates=50, phase2_start_update=50, current_epoch=1)
    assert method == "viterbi" and "method_switch" not in logs and logs["duration_weight"] == pytest.approx(0.1, rel=1e-12)
    # a fresh manager that meets the update threshold and epoch 3 at once goes to viterbi in one call
    m2 = AlignmentMethodManager()
    assert get_alignment_method(m2, 12000, current_epoch=3)[0] == "viterbi" and get_alignment_method(AlignmentMethodManager(), 11999, current_epoch=3)[0] == "window"
