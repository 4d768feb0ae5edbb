"""Host side of the attention-dropout mode: the C ABI declares and binds its two entry points, and the mask generator
the kernels compile (eraxvif5tts_amd/csrc/philox.h, plain C++) is Philox4x32-10 as published -- the numpy restatement the GPU tests take their
expected masks from reproduces the Random123 known-answer vectors, and the header, compiled with g++, reproduces the numpy version."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dropout_ref as R
from conftest import ROOT

NEW = ("f5_plan_set_attn_dropout", "f5_op_attention_dropout")


def test_abi_declares_lists_and_binds_the_entry_points():
    from eraxvif5tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    for name in NEW:
        assert re.search(r"F5_API\s+int\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name
    m = re.search(r"int f5_plan_set_attn_dropout\(f5_plan_t p, float prob, uint64_t seed\);", header)
    assert m, "f5_plan_set_attn_dropout's signature"
    assert re.search(r"int f5_op_attention_dropout\(int precision, int kernel, int B, int N, int H, const float\* qkv, const uint8_t\* mask, float prob,\s*"
                     r"uint64_t seed, uint32_t stream_word, uint32_t batch0, float\* out, f5_stream_t stream\);", header)
    lib = _lib.load()  # (binds every entry of EXPORTS: a missing symbol raises)
    for name in NEW:
        assert getattr(lib, name).argtypes is not None
    assert lib.f5_version() == 400


def test_numpy_philox_reproduces_the_random123_vectors():
    for ctr, key, want in R.KAT:
        got = R.philox4x32_10(*ctr, *key)
        assert tuple(int(w) for w in got) == want, (ctr, key, [hex(int(w)) for w in got])


_PROGRAM = r"""
#include <stdio.h>
#include "philox.h"
int main() {
    const uint32_t kat[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                                {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
    for (int i = 0; i < 3; ++i) {
        const Philox4 o = philox4x32_10(kat[i][0], kat[i][1], kat[i][2], kat[i][3], kat[i][4], kat[i][5]);
        printf("%08x %08x %08x %08x\n", o.v[0], o.v[1], o.v[2], o.v[3]);
    }
    uint64_t s = 0x9E3779B97F4A7C15ull;  /* splitmix64: the (counter, key) pairs the Python side regenerates */
    for (int i = 0; i < 1000; ++i) {
        uint32_t w[6];
        for (int j = 0; j < 6; ++j) {
            s += 0x9E3779B97F4A7C15ull;
            uint64_t z = s;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            w[j] = (uint32_t)(z >> 32);
        }
        const Philox4 o = philox4x32_10(w[0], w[1], w[2], w[3], w[4], w[5]);
        printf("%08x %08x %08x %08x\n", o.v[0], o.v[1], o.v[2], o.v[3]);
    }
    /* the mask wrapper and the threshold */
    const Philox4 d = attn_dropout_draws(7u, 11u, 13u, 0x10003u, 0x123456789ABCDEF0ull);
    printf("%08x %08x %08x %08x\n", d.v[0], d.v[1], d.v[2], d.v[3]);
    printf("%u\n", attn_dropout_threshold(0.1));
    return 0;
}
"""


def _splitmix_words(n):
    M = (1 << 64) - 1
    s, out = 0x9E3779B97F4A7C15, []
    for _ in range(n):
        s = (s + 0x9E3779B97F4A7C15) & M
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        out.append(z >> 32)
    return out


def test_header_compiled_with_gxx_equals_the_numpy_version(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed: philox.h must compile as plain host C++"
    src = tmp_path / "philox_check.cpp"
    src.write_text(_PROGRAM)
    exe = tmp_path / "philox_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "eraxvif5tts_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    words = np.array(_splitmix_words(6000), dtype=np.uint64).reshape(1000, 6)
    cols = [np.concatenate([np.array([k[0][i] if i < 4 else k[1][i - 4] for k in R.KAT], dtype=np.uint64), words[:, i]]) for i in range(6)]
    o = R.philox4x32_10(*cols)
    want = ["%08x %08x %08x %08x" % tuple(int(o[j][i]) for j in range(4)) for i in range(1003)]
    assert lines[:1003] == want
    assert lines[:3] == ["%08x %08x %08x %08x" % k[2] for k in R.KAT]
    d = R.philox4x32_10(7, 11, 13, 0x10003, 0x9ABCDEF0, 0x12345678)
    assert lines[1003] == "%08x %08x %08x %08x" % tuple(int(w) for w in d)
    assert lines[1004] == str(R.threshold(0.1)) == "429496730"


def test_keep_mask_layout_and_threshold():
    """keep_mask against the scalar definition at a few points: word k & 3 of call k >> 2, batch word batch0 + b, bw * H + head."""
    B, H, N, seed, stream, b0 = 2, 3, 41, R.SEED_HI, 0x10003, 5
    km = R.keep_mask(seed, stream, b0, B, H, N, 0.1)
    assert km.shape == (B, H, N, N) and km.dtype == bool
    for b, h, q, k in [(0, 0, 0, 0), (1, 2, 40, 40), (0, 1, 17, 6), (1, 0, 3, 39)]:
        o = R.philox4x32_10(k >> 2, q, (b0 + b) * H + h, stream, seed & 0xFFFFFFFF, seed >> 32)
        assert km[b, h, q, k] == (int(o[k & 3]) >= 429496730)
    assert R.keep_mask(seed, stream, b0, 1, 1, 8, 0.0).all()


def test_keep_fraction_of_every_gpu_test_mask():
    seen = set()
    for seed, stream, b0, (B, H, N) in R.MASK_CASES:
        if (seed, stream, b0, B, H, N) in seen:
            continue
        seen.add((seed, stream, b0, B, H, N))
        km = R.keep_mask(seed, stream, b0, B, H, N, R.P)
        dev = (km.mean() - (1.0 - R.P)) / R.sigma_of(km.size)
        assert abs(dev) < 5.0, (hex(seed), stream, b0, (B, H, N), dev)
