"""Host side of the ragged BigVGAN decode (no GPU): the header declares `f5_bigvgan_decode_ragged` and `_lib` binds it, argument for argument like
`f5_vocoder_decode_ragged`."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_ragged_bigvgan_entry_point():
    from eraxvif5tts_amd import _lib
    with open(os.path.join(ROOT, "include", "f5hip.h")) as f:
        header = f.read()
    m = re.search(r"F5_API\s+int\s+f5_bigvgan_decode_ragged\s*\(([^)]*)\)\s*;", header)
    assert m, "include/f5hip.h does not declare f5_bigvgan_decode_ragged"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 9
    assert params[0].startswith("f5_bigvgan_t") and params[-1].startswith("f5_stream_t") and params[7].startswith("int64_t*")
    assert "#define F5HIP_VERSION 400" in header  # the entry point is detected by symbol, not by version
    restype, argtypes = _lib._PROTOS["f5_bigvgan_decode_ragged"]
    assert restype is C.c_int and len(argtypes) == 9
    assert argtypes == _lib._PROTOS["f5_vocoder_decode_ragged"][1]


def test_bigvgan_class_has_the_ragged_methods_and_keeps_its_tail_kind():
    from eraxvif5tts_amd.bigvgan import BigVGAN
    from eraxvif5tts_amd.infer import utils_infer as U
    assert callable(getattr(BigVGAN, "decode_ragged", None)) and callable(getattr(BigVGAN, "decode_ragged_buffer", None))
    assert U.device_tail_kind(object()) is None  # (no tensors: the host loop)
