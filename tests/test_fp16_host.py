"""Host side of the fp16 precision mode (include/f5hip.h: F5_PREC_FP16): the constant, the precision names the backbones accept, the
F5HIP_PRECISION environment variable, and the attention-dropout refusal, which comes before any library call."""
import os
import re

import pytest

from conftest import ROOT

ARCH = dict(dim=128, depth=1, heads=2, ff_mult=2, text_dim=64, conv_layers=0, pe_attn_head=1, text_mask_padding=False)


def _dit(**kw):
    from eraxvif5tts_amd.model import DiT
    return DiT(**ARCH, text_num_embeds=20, mel_dim=100, **kw)


def test_constant_and_header_agree():
    from eraxvif5tts_amd import _lib
    assert _lib.F5_PREC_FP16 == 2 and (_lib.F5_PREC_BF16, _lib.F5_PREC_FP32) == (0, 1)
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    assert re.search(r"#define\s+F5_PREC_FP16\s+2\b", header)
    for name in ("f5_op_linear_fused_p", "f5_op_ln_fold_p"):
        assert re.search(r"F5_API\s+int\s+" + name + r"\s*\(int precision,", header), name
        assert name in _lib.EXPORTS, name


def test_precision_names():
    from eraxvif5tts_amd import _lib
    assert _dit(precision="fp16").precision == _lib.F5_PREC_FP16
    assert _dit(precision="bf16").precision == _lib.F5_PREC_BF16
    assert _dit(precision="fp32").precision == _lib.F5_PREC_FP32
    with pytest.raises(KeyError):
        _dit(precision="fp8")
    from eraxvif5tts_amd.model import MMDiT, UNetT
    assert UNetT(dim=128, depth=2, heads=2, ff_mult=2, text_num_embeds=20, mel_dim=100, precision="fp16").precision == _lib.F5_PREC_FP16
    assert MMDiT(dim=128, depth=2, heads=2, ff_mult=2, text_num_embeds=20, mel_dim=100, precision="fp16").precision == _lib.F5_PREC_FP16


def test_environment_variable_is_honoured_at_construction(monkeypatch):
    from eraxvif5tts_amd import _lib
    monkeypatch.setenv("F5HIP_PRECISION", "fp16")
    assert _dit().precision == _lib.F5_PREC_FP16
    assert _dit(precision="bf16").precision == _lib.F5_PREC_BF16  # the argument wins
    monkeypatch.delenv("F5HIP_PRECISION")
    assert _dit().precision == _lib.F5_PREC_BF16                  # the default stays bf16


def test_attention_dropout_is_refused_before_the_library_is_loaded(monkeypatch):
    from eraxvif5tts_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("set_attn_dropout reached the library")
    monkeypatch.setattr(_lib, "load", no_library)
    m = _dit(precision="fp16")
    with pytest.raises(NotImplementedError, match="fp16"):
        m.set_attn_dropout(0.1)
    assert m._attn_dropout is None
    m.set_attn_dropout(None)  # turning the mode off is always allowed (no plan yet: nothing to call)
    m.set_attn_dropout(0.0)
