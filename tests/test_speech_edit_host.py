"""Speech editing on the host: the edit-mask arithmetic of the reference script (infer/speech_edit.py:136-156) and the C ABI declaration of
the masked sampler.  No GPU needed."""
import os
import re
import shutil
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _runs(mask):
    """[(value, length), ...] of a 1-D bool tensor"""
    out = []
    for v in mask.tolist():
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [tuple(r) for r in out]


def test_edit_mask_of_the_reference_example_with_fix_duration():
    from eraxvif5tts_amd.infer.speech_edit import build_edit_mask
    # 1.42 s * 24000 / 256 = 133.125 -> 133 kept; 1.2 s -> 112.5 -> 112 regenerated (round half to even); (4.04 - 2.44) s -> 150 kept;
    # 1 s -> 93.75 -> 94 regenerated; 130000 // 256 + 1 = 508 frames -> 19 True frames of padding
    m = build_edit_mask(130000, [[1.42, 2.44], [4.04, 4.9]], fix_duration=[1.2, 1])
    assert m.dtype == torch.bool and m.shape == (508,)
    assert _runs(m) == [(True, 133), (False, 112), (True, 150), (False, 94), (True, 19)]


def test_edit_mask_without_fix_duration():
    from eraxvif5tts_amd.infer.speech_edit import build_edit_mask
    # spans keep their own length: (2.44 - 1.42) s -> 95.6 -> 96, (4.9 - 4.04) s -> 80.6 -> 81
    m = build_edit_mask(130000, [[1.42, 2.44], [4.04, 4.9]])
    assert _runs(m) == [(True, 133), (False, 96), (True, 150), (False, 81), (True, 48)]
    fix = [1.2, 1]
    build_edit_mask(130000, [[1.42, 2.44], [4.04, 4.9]], fix_duration=fix)
    assert fix == [1.2, 1]  # the caller's list is not consumed (the script pops its own)


def test_edit_mask_touching_the_end_of_the_clip():
    from eraxvif5tts_amd.infer.speech_edit import build_edit_mask
    # 3.0 s clip, the last second edited: 187.5 -> 188 kept, 93.75 -> 94 regenerated = 72000 // 256 + 1 frames, no padding
    m = build_edit_mask(72000, [[2.0, 3.0]])
    assert _runs(m) == [(True, 188), (False, 94)]
    # a fixed duration past the end: the mask is cut to the clip's frames (negative pad), as in the script
    m = build_edit_mask(72000, [[2.0, 3.0]], fix_duration=[1.5])
    assert m.shape == (282,) and _runs(m) == [(True, 188), (False, 94)]
    # other rates / hops follow the same arithmetic: 16 kHz, hop 160 -> 0.5 s = 50 frames kept, 0.25 s = 25 regenerated, 16000 // 160 + 1 = 101
    m = build_edit_mask(16000, [[0.5, 0.75]], sample_rate=16000, hop_length=160)
    assert _runs(m) == [(True, 50), (False, 25), (True, 26)]


def test_masked_sampler_is_declared_and_exported():
    from eraxvif5tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    decl = re.search(r"F5_API int f5_sample_masked\(([^;]*)\);", header)
    assert decl, "f5_sample_masked is not declared in include/f5hip.h"
    assert "const uint8_t* cond_mask" in decl.group(1)
    assert "f5_sample_masked" in _lib.EXPORTS
    lib = _lib.load(build_if_missing=True)
    assert hasattr(lib, "f5_sample_masked")
    nm = shutil.which("nm")
    if nm:  # exported from the shared object itself (the library is built with -fvisibility=hidden)
        syms = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT f5_sample_masked$", syms, re.M)
