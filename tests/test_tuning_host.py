"""CPU tests of the tuning-knob table (csrc/tuning.h): the key list and defaults of a freshly loaded library, set / get of every knob, the
refusals, and that gpu_helpers.knobs puts back what it found.  DEFAULTS below is the one copy of the defaults the tests keep; everything else
reads a knob (f5_tuning_get) before it sets it."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import gpu_helpers as G
from eraxvif5tts_amd import _lib

F5_EINVAL = -1  # include/f5hip.h

DEFAULTS = {
    "attn_variant": 0, "attn_prescale": 1, "conv31": 1, "conv31_tok": 0, "op_conv_kernel": 0, "vocos_fft": 1, "bigvgan_group_frames": 2048,
    "gemm_variant": 1, "gemm_group": 0, "gemm_group_sites": 0, "gemm_reverse_sites": 8, "gemm_persist": 1, "gemm_persist_grid": 0, "gemm_tile": 0,
    "gemm_bm128": 1, "gemm_lean": 1, "gemm_pad_rows": 1, "gemm_w4": 1, "gemm_w4_ink": 1, "gemm_w4_bm": 0, "ln_rows": 2, "ln_rows_min": 16384,
    "ln_wide": 1, "ln_defer": 1, "ln_fold": 1, "ln_fold_inkernel": 0, "resid_rmw": 1, "residual_f16": 1, "w_prefetch": 16384, "sync_evals": 0,
    "bench_pad_a": 0, "bench_pad_w": 0,
}
BOOL_KNOBS = {"resid_rmw", "sync_evals", "ln_wide", "residual_f16", "vocos_fft", "attn_prescale", "op_conv_kernel", "conv31", "ln_defer", "gemm_lean",
              "gemm_pad_rows", "ln_fold_inkernel", "ln_fold", "gemm_w4", "gemm_persist"}

# what a process that has only just loaded the library sees: plain ctypes, no F5HIP_TUNING (which eraxvif5tts_amd._lib alone applies)
_FRESH = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.f5_tuning_key.restype = ctypes.c_char_p
out, i = {}, 0
while True:
    key = lib.f5_tuning_key(i)
    if key is None:
        break
    v = ctypes.c_int(-12345)
    assert lib.f5_tuning_get(key, ctypes.byref(v)) == 0, key
    assert key.decode() not in out, key
    out[key.decode()] = v.value
    i += 1
assert lib.f5_tuning_key(-1) is None and lib.f5_tuning_key(i + 1) is None
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=True)


def _keys(lib):
    keys, i = [], 0
    while (key := lib.f5_tuning_key(i)) is not None:
        keys.append(key.decode())
        i += 1
    return keys


def test_keys_and_defaults_of_a_fresh_library(lib):
    env = {k: v for k, v in os.environ.items() if k != "F5HIP_TUNING"}
    r = subprocess.run([sys.executable, "-c", _FRESH, _lib.LIB_PATH], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == DEFAULTS
    assert len(DEFAULTS) == 32 and BOOL_KNOBS <= set(DEFAULTS) and len(BOOL_KNOBS) == 15
    assert sorted(_keys(lib)) == sorted(DEFAULTS)


def test_set_get_round_trip_of_every_key(lib):
    for key in _keys(lib):
        with G.knobs(**{key: G.knob_get(key)}):  # puts back what is in force now
            if key in BOOL_KNOBS:
                assert lib.f5_tuning_set(key.encode(), 7) == 0 and G.knob_get(key) == 1, key
                assert lib.f5_tuning_set(key.encode(), 0) == 0 and G.knob_get(key) == 0, key
            else:
                # values every validator accepts; 9 is one that bool storage would turn into 1
                for value in (256, 9, 0) if key != "bigvgan_group_frames" else (256, 9):
                    assert lib.f5_tuning_set(key.encode(), value) == 0 and G.knob_get(key) == value, (key, value)


@pytest.mark.parametrize("key,value", [("bigvgan_group_frames", 0), ("gemm_persist_grid", 7), ("gemm_persist_grid", 4097), ("attn_variant", 6)])
def test_refused_values_leave_the_knob_alone(lib, key, value):
    was = G.knob_get(key)
    assert lib.f5_tuning_set(key.encode(), value) == F5_EINVAL
    assert key in _lib.last_error()
    assert G.knob_get(key) == was


def test_unknown_and_null_arguments(lib):
    v = C.c_int(77)
    assert lib.f5_tuning_set(b"no_such_knob", 1) == F5_EINVAL
    assert "unknown tuning key 'no_such_knob'" in _lib.last_error()
    assert lib.f5_tuning_get(b"no_such_knob", C.byref(v)) == F5_EINVAL and v.value == 77
    assert lib.f5_tuning_set(None, 1) == F5_EINVAL
    assert lib.f5_tuning_get(None, C.byref(v)) == F5_EINVAL and lib.f5_tuning_get(b"ln_rows", None) == F5_EINVAL
    with pytest.raises(_lib.F5HipError):
        G.knob_get("no_such_knob")


def test_knobs_restores_what_it_found(lib):
    class Boom(Exception):
        pass

    found = {k: G.knob_get(k) for k in ("ln_rows", "gemm_lean")}
    try:
        assert lib.f5_tuning_set(b"ln_rows", 4) == 0 and lib.f5_tuning_set(b"gemm_lean", 1) == 0  # by hand: the state the blocks below find
        with pytest.raises(Boom):
            with G.knobs(ln_rows=1, gemm_lean=0):
                assert (G.knob_get("ln_rows"), G.knob_get("gemm_lean")) == (1, 0)
                with G.knobs(ln_rows=3):
                    assert G.knob_get("ln_rows") == 3
                    raise Boom
        assert (G.knob_get("ln_rows"), G.knob_get("gemm_lean")) == (4, 1)
        with pytest.raises(_lib.F5HipError):  # a value refused in the middle of one call: what that call had set already is put back
            with G.knobs(ln_rows=1, gemm_persist_grid=7):
                pass
        assert G.knob_get("ln_rows") == 4
    finally:
        for k, v in found.items():
            assert lib.f5_tuning_set(k.encode(), v) == 0
