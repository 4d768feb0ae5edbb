"""The WavLM feature extractor on the device (include/f5hip.h: f5_wavlm_*, f5_op_wavlm_*; csrc/wavlm.hip) and its Python surface
(eraxvif5tts_amd/eval/wavlm.py) against tests/wavlm_ref.py in fp64, which tests/test_wavlm_host.py pins to transformers' WavLMModel.

Bound of every comparison, per tensor (tap, hidden state or op output), no element exempted:
    max|gpu - ref64| / max|ref64|  <=  4 x  max|ref32 - ref64| / max|ref64|
with ref64 the restatement in fp64 and ref32 the SAME torch graph in fp32 on the CPU, both on the same fp32 inputs and parameters: the
yardstick is what fp32 arithmetic costs on this very tensor, and the factor 4 is for the different summation orders (the device adds K in
chunks of 512 on the MFMA's fma chain, torch in its BLAS's blocks).  The yardstick is computed here, never taken from the device.  Every
figure is printed before it is asserted; with F5HIP_WAVLM_ERRORS=<path> they are also appended to that file (profiles/wavlm_errors.txt).
Ragged calls are compared bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import speaker_ref as SR
import wavlm_ref as R
from conftest import load_golden
from eraxvif5tts_amd import _lib
from eraxvif5tts_amd.eval import SpeakerEncoder, WavLMExtractor, speaker_similarity

pytestmark = pytest.mark.gpu
FACTOR = 4.0
F5_EINVAL = -1
TINY = R.TINY_CONFIG
WIDE = dict(R.LARGE_CONFIG, num_hidden_layers=2)  # hidden 1024, 16 heads, FFN 4096, the full conv stack


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


_REPORTED = []


def _report(what, dev, r32, r64):
    """print, record and assert one tensor's bound"""
    r64 = r64.double().cpu()
    scale = float(r64.abs().max())
    err = float((dev.double().cpu() - r64).abs().max()) / scale
    yard = float((r32.double().cpu() - r64).abs().max()) / scale
    line = f"{what:44s} device {err:.3e}   fp32 torch (yardstick) {yard:.3e}   ratio {err / yard if yard else float('inf'):.2f}"
    print(line)
    path = os.environ.get("F5HIP_WAVLM_ERRORS")
    if path:
        with open(path, "a" if _REPORTED else "w") as fh:  # a run starts the file afresh: reruns give the same file, not a longer one
            fh.write(line + "\n")
        _REPORTED.append(what)
    return what, err, yard


def _assert_all(rows):
    bad = [f"{w}: {e:.3e} > {FACTOR:g} x {y:.3e}" for w, e, y in rows if not e <= FACTOR * y]
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------- shared references (computed once, never modified)
@functools.lru_cache(maxsize=None)
def golden():
    z = load_golden("wavlm_tiny")
    P = {k[6:]: torch.from_numpy(z[k]) for k in z if k.startswith("state.")}
    waves = [torch.from_numpy(z[f"wave{i}"]) for i in range(len(R.GOLDEN_SAMPLES))]
    hs64 = [torch.from_numpy(z[f"hs{i}"]) for i in range(len(R.GOLDEN_SAMPLES))]
    return P, R.to_dtype(P, torch.float64), waves, hs64


@functools.lru_cache(maxsize=None)
def tiny_reference(final_norm, normalize):
    """per dtype: (packed hidden states [L, rows, F], packed taps) of the three golden waves"""
    P32, P64, waves, _ = golden()
    out = []
    for P in (P32, P64):
        hs, taps = [], []
        for w in waves:
            t = {}
            hs.append(R.forward(P, TINY, w, final_norm=final_norm, normalize_input=normalize, taps=t))
            taps.append(t)
        out.append((torch.cat(hs, dim=1), {k: torch.cat([t[k] for t in taps]) for k in taps[0]}))
    return out


@functools.lru_cache(maxsize=None)
def tiny_extractor(normalize=False, final_norm="hf"):
    return WavLMExtractor(normalize_input=normalize, final_norm=final_norm, **TINY).load_state_dict(golden()[0])


def tap_names(cfg):
    return [f"conv{i}" for i in range(len(cfg["conv_dim"]))] + ["proj", "posconv"] + \
           [f"layer{i}.{s}" for i in range(cfg["num_hidden_layers"]) for s in ("attn", "out")]


# ----------------------------------------------------------------------------- the tiny model
@pytest.mark.parametrize("final_norm", ["hf", "s3prl"])
def test_tiny_model_every_tap_and_hidden_state(final_norm):
    P32, P64, waves, hs64 = golden()
    (h32, t32), (h64, t64) = tiny_reference(final_norm, False)
    if final_norm == "hf":  # the restatement IS the golden (test_wavlm_host.py); say so on this side too
        assert float((h64 - torch.cat(hs64, dim=1)).abs().max()) <= 1e-12 * float(h64.abs().max())
    taps = dict.fromkeys(tap_names(TINY))
    hs, frames = tiny_extractor().extract([w.cuda() for w in waves], final_norm=final_norm, taps=taps)
    torch.cuda.synchronize()
    assert frames == [2, 37, 130] and hs.shape == h64.shape
    assert set(taps) == set(t64)
    rows = [_report(f"tiny/{final_norm}/tap {k}", taps[k], t32[k], t64[k]) for k in taps]
    rows += [_report(f"tiny/{final_norm}/hidden_states[{l}]", hs[l], h32[l], h64[l]) for l in range(hs.shape[0])]
    _assert_all(rows)
    assert torch.equal(taps["posconv"], hs[0]) and torch.equal(taps["layer0.out"], hs[1])
    if final_norm == "s3prl":
        assert torch.equal(taps[f"layer{TINY['num_hidden_layers'] - 1}.out"], hs[-1])


def test_tiny_model_with_input_normalisation():
    _, _, waves, _ = golden()
    (h32, _), (h64, _) = tiny_reference("s3prl", True)
    hs, _ = tiny_extractor(True, "s3prl").extract([w.cuda() for w in waves])
    _assert_all([_report(f"tiny/normalize_input/hidden_states[{l}]", hs[l], h32[l], h64[l]) for l in range(hs.shape[0])])


def test_ragged_call_is_bit_equal_to_single_calls_at_any_position():
    _, _, waves, _ = golden()
    ex = tiny_extractor(True, "s3prl")
    dev = [w.cuda() for w in waves]
    together, frames = ex.extract(dev)
    rev, rframes = ex.extract(dev[::-1])
    assert rframes == frames[::-1]
    off, roff = np.cumsum([0] + frames), np.cumsum([0] + rframes)
    for u in range(len(dev)):
        alone, f = ex.extract([dev[u]])
        assert f == [frames[u]]
        assert torch.equal(alone, together[:, off[u]:off[u + 1]]), u
        v = len(dev) - 1 - u
        assert torch.equal(alone, rev[:, roff[v]:roff[v + 1]]), u
    # the callable form (equal lengths) is the same computation
    out = ex([dev[1], dev[1]])["hidden_states"]
    assert len(out) == ex.layers and out[0].shape == (2, frames[1], TINY["hidden_size"])
    single = together[:, off[1]:off[2]]
    assert all(torch.equal(out[l][0], single[l]) and torch.equal(out[l][1], single[l]) for l in range(ex.layers))


def test_call_cut_into_several_launch_sets_changes_no_bit():
    """125 utterances: the first launch set closes at 64 utterances, the second at 2048 frames (5 x 2 + 55 x 37 = 2045), the third takes the
    rest -- each with its own offsets into the waves, the output and the taps, on one reused workspace.  No bit may change."""
    _, _, waves, _ = golden()
    ex = tiny_extractor(True, "s3prl")
    dev = [w.cuda() for w in waves]
    order = [1, 0, 2] + [0] * 66 + [1] * 56
    assert len(order) == 125
    single = [ex.extract([d])[0] for d in dev]
    taps = dict.fromkeys(["conv1", "conv2", "proj", "layer1.attn"])
    single_taps = []
    for d in dev:
        t = dict.fromkeys(taps)
        ex.extract([d], taps=t)
        single_taps.append(t)
    hs, frames = ex.extract([dev[i] for i in order], taps=taps)
    assert frames == [[2, 37, 130][i] for i in order]
    off = np.cumsum([0] + frames)
    for u, i in enumerate(order):
        assert torch.equal(hs[:, off[u]:off[u + 1]], single[i]), u
    for name in taps:
        rows = [single_taps[i][name].shape[0] for i in order]
        toff = np.cumsum([0] + rows)
        assert taps[name].shape[0] == toff[-1]
        for u, i in enumerate(order):
            assert torch.equal(taps[name][toff[u]:toff[u + 1]], single_taps[i][name]), (name, u)


# ----------------------------------------------------------------------------- the new kernels one by one, production widths
def _host(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return a, a.ctypes.data


@functools.lru_cache(maxsize=None)
def attention_case(T, H, dh):
    g = torch.Generator().manual_seed(1000 * T + H)
    qkv = torch.randn(T, 3 * H * dh, generator=g)
    gate = 1.0 + torch.rand(T, H, generator=g)  # the gate's range is (1, 2) for const = 1
    rel = torch.randn(H, 2 * T - 1, generator=g)

    def ref(dt):
        q, k, v = (t.to(dt).view(T, H, dh) for t in qkv.chunk(3, dim=1))
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + (T - 1)
        return R.attention_core(q, k, v, gate.to(dt), rel.to(dt)[:, idx])
    return qkv, gate, rel, ref(torch.float32), ref(torch.float64)


@pytest.mark.parametrize("T, H, dh", [(1, 16, 64), (2, 16, 64), (63, 16, 64), (64, 16, 64), (65, 16, 64), (130, 16, 64), (257, 4, 16)])
def test_op_attention(T, H, dh):
    qkv, gate, rel, r32, r64 = attention_case(T, H, dh)
    out = torch.full((T, H * dh), float("nan"), device="cuda")
    dq, dg, dr = qkv.cuda(), gate.cuda(), rel.cuda()
    _lib.check(_lib.load().f5_op_wavlm_attention(T, H, dh, _lib.ptr(dq), _lib.ptr(dg), _lib.ptr(dr), _lib.ptr(out), _lib.stream_ptr()),
               "op_wavlm_attention")
    torch.cuda.synchronize()
    _assert_all([_report(f"op/attention T={T} H={H} dh={dh}", out, r32, r64)])


@functools.lru_cache(maxsize=None)
def pos_conv_case(T, C_, k, groups):
    g = torch.Generator().manual_seed(31 * T + k)
    x = torch.randn(T, C_, generator=g)
    w = torch.randn(C_, C_ // groups, k, generator=g) / (C_ // groups * k) ** 0.5
    b = 0.1 * torch.randn(C_, generator=g)
    return x, w, b, R.pos_conv(x, w, b, groups), R.pos_conv(x.double(), w.double(), b.double(), groups)


@pytest.mark.parametrize("T, k", [(1, 128), (64, 128), (130, 128), (64, 5), (33, 5)])
def test_op_pos_conv(T, k):
    C_, groups = 1024, 16
    x, w, b, r32, r64 = pos_conv_case(T, C_, k, groups)
    (wa, wp), (ba, bp) = _host(w), _host(b)
    out = torch.full((T, C_), float("nan"), device="cuda")
    dx = x.cuda()
    _lib.check(_lib.load().f5_op_wavlm_pos_conv(T, C_, k, groups, _lib.ptr(dx), wp, bp, _lib.ptr(out), _lib.stream_ptr()), "op_wavlm_pos_conv")
    _assert_all([_report(f"op/pos_conv T={T} C={C_} k={k} groups={groups}", out, r32, r64)])


@functools.lru_cache(maxsize=None)
def conv_case(T_in, cin, cout, k, stride, bias):
    g = torch.Generator().manual_seed(7 * T_in + k + cin)
    x = torch.randn(T_in, cin, generator=g)
    P = {"feature_extractor.conv_layers.0.conv.weight": torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5,
         "feature_extractor.conv_layers.0.layer_norm.weight": 1.0 + 0.2 * torch.randn(cout, generator=g),
         "feature_extractor.conv_layers.0.layer_norm.bias": 0.1 * torch.randn(cout, generator=g)}
    if bias:
        P["feature_extractor.conv_layers.0.conv.bias"] = 0.1 * torch.randn(cout, generator=g)
    cfg = dict(conv_stride=(stride,), layer_norm_eps=1e-5)
    ref = lambda P, x: R.conv_layer(P, cfg, 0, x.t().unsqueeze(0))[0].t()  # noqa: E731
    with torch.no_grad():
        return x, P, ref(P, x), ref(R.to_dtype(P, torch.float64), x.double())


@pytest.mark.parametrize("T_in, cin, cout, k, stride, bias", [(65, 512, 512, 3, 2, False), (64, 512, 512, 3, 2, True), (65, 512, 512, 2, 2, True),
                                                             (130, 512, 512, 2, 2, False), (1003, 1, 512, 10, 5, False), (1000, 1, 512, 10, 5, True)])
def test_op_conv_ln_gelu(T_in, cin, cout, k, stride, bias):
    x, P, r32, r64 = conv_case(T_in, cin, cout, k, stride, bias)
    p = "feature_extractor.conv_layers.0."
    (wa, wp), (la, lp), (ma, mp) = _host(P[p + "conv.weight"]), _host(P[p + "layer_norm.weight"]), _host(P[p + "layer_norm.bias"])
    ba, bp = _host(P[p + "conv.bias"]) if bias else (None, None)
    T_out = (T_in - k) // stride + 1
    assert r64.shape == (T_out, cout)
    out = torch.full((T_out, cout), float("nan"), device="cuda")
    dx = x.cuda()
    _lib.check(_lib.load().f5_op_wavlm_conv_ln_gelu(T_in, cin, cout, k, stride, _lib.ptr(dx), wp, bp, lp, mp, _lib.ptr(out), _lib.stream_ptr()),
               "op_wavlm_conv_ln_gelu")
    _assert_all([_report(f"op/conv_ln_gelu T_in={T_in} {cin}->{cout} k={k} s={stride} bias={int(bias)}", out, r32, r64)])


# ----------------------------------------------------------------------------- two layers at wavlm-large's widths
def test_two_layer_model_at_hidden_1024():
    P32 = R.random_state(WIDE, seed=11)
    wave = 0.3 * torch.randn(8000, generator=torch.Generator().manual_seed(12))
    t32, t64 = {}, {}
    h32 = R.forward(P32, WIDE, wave, final_norm="s3prl", normalize_input=True, taps=t32)
    h64 = R.forward(R.to_dtype(P32, torch.float64), WIDE, wave, final_norm="s3prl", normalize_input=True, taps=t64)
    ex = WavLMExtractor(**WIDE).load_state_dict(P32)  # the defaults: normalize_input, final_norm="s3prl"
    taps = dict.fromkeys(tap_names(WIDE))
    hs, frames = ex.extract([wave.cuda()], taps=taps)
    assert frames == [24] and hs.shape == (3, 24, 1024)
    rows = [_report(f"wide/tap {k}", taps[k], t32[k], t64[k]) for k in taps]
    rows += [_report(f"wide/hidden_states[{l}]", hs[l], h32[l], h64[l]) for l in range(3)]
    _assert_all(rows)
    # the same utterance behind another one (a non-zero first row for the dh = 64 attention, the k = 128 positional conv and the conv GEMMs)
    short = 0.3 * torch.randn(1300, generator=torch.Generator().manual_seed(13))
    both, bframes = ex.extract([short.cuda(), wave.cuda()])
    alone_short, _ = ex.extract([short.cuda()])
    assert bframes == [ex.frames(1300), 24] and bframes[0] == 3
    assert torch.equal(both[:, 3:], hs) and torch.equal(both[:, :3], alone_short)


# ----------------------------------------------------------------------------- speaker_similarity through the extractor
def test_speaker_similarity_ragged_route():
    """The ragged route (one extract call, packed hidden states straight into the head) is bit-equal to the plug point's old route (the same
    extractor wrapped in a plain callable: one wave at a time, re-concatenated), and both agree with speaker_ref fed by wavlm_ref in fp64.
    Bound: with e the embeddings, a cosine moves by at most the sum of the relative errors of its two vectors (first order), so
    |sim - sim64| <= 8 x 2 x max_u |e32_u - e64_u| / |e64_u| -- the fp32 restatement chain's own embedding error as the yardstick, 8 x as
    tests/test_gpu_speaker.py allows the head."""
    P32, P64, waves, _ = golden()
    scfg = dict(feat_dim=TINY["hidden_size"], channels=64, emb_dim=16, layers=TINY["num_hidden_layers"] + 1, cat_channels=1536, se_bottleneck=128,
                attention_channels=128, scale=8)
    S32 = SR.filled_state(scfg)
    enc = SpeakerEncoder(**scfg).load_state_dict(S32)
    ex = tiny_extractor(True, "s3prl")
    g = torch.Generator().manual_seed(3)
    pairs = [(waves[1], waves[2]), (0.3 * torch.randn(1500, generator=g), waves[1][:400])]
    sim, mean = speaker_similarity(enc, pairs, feature_extractor=ex, sample_rate=16000)
    calls = []

    def plain(ws):
        calls.append(len(ws))
        return ex(ws)
    sim_old, mean_old = speaker_similarity(enc, pairs, feature_extractor=plain, sample_rate=16000)
    assert calls == [1, 1, 1, 1]
    assert torch.equal(sim, sim_old) and mean == mean_old
    with torch.no_grad():
        e = {dt: [SR.forward(SR.to_dtype(S32, dt), R.forward(P, TINY, w, final_norm="s3prl", normalize_input=True), scfg)[0]
                  for pair in pairs for w in pair] for dt, P in ((torch.float32, P32), (torch.float64, P64))}
    e32, e64 = e[torch.float32], e[torch.float64]
    sim64 = torch.stack([torch.nn.functional.cosine_similarity(e64[2 * i], e64[2 * i + 1], dim=0) for i in range(len(pairs))])
    yard = max(float((a.double() - b).norm() / b.norm()) for a, b in zip(e32, e64))
    err = float((sim.double().cpu() - sim64).abs().max())
    print(f"speaker_similarity: |sim - sim64| {err:.3e}   embedding yardstick {yard:.3e}   sims {sim64.tolist()}")
    assert err <= 16 * yard
    assert abs(mean - float(sim64.mean())) <= 16 * yard


# ----------------------------------------------------------------------------- refusals launch nothing
def test_refusals_answer_an_error_and_launch_nothing():
    lib = _lib.load()
    ex = tiny_extractor()
    hd = ex.native()
    ex._ensure_buckets(hd, 1)
    samples = [760, 29]  # 29 samples: conv layer 1 leaves one frame, shorter than conv layer 2's kernel
    assert ex.frames(29) < 1 and lib.f5_wavlm_frames(hd, 29) < 0 and lib.f5_wavlm_frames(hd, 30) == 1 and lib.f5_wavlm_frames(hd, 760) == 37
    wave = torch.zeros(sum(samples), device="cuda")
    hs = torch.full((ex.layers, 64, 64), float("nan"), device="cuda")
    rc = lib.f5_wavlm_extract_ragged(hd, 2, (C.c_int32 * 2)(*samples), _lib.ptr(wave), 1, _lib.ptr(hs), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == F5_EINVAL and "utterance 1" in _lib.last_error() and bool(torch.isnan(hs).all())
    with pytest.raises(ValueError, match="too short"):
        ex.extract([wave[:760], wave[760:]])
    for field, value, word in (("feat_extract_norm", 1, "feat_extract_norm"), ("do_stable_layer_norm", 0, "do_stable_layer_norm"),
                               ("add_adapter", 1, "add_adapter"), ("num_attention_heads", 2, "head dimension 32"),
                               ("num_attention_heads", 5, "not divisible")):
        cfg = ex._native_config()
        setattr(cfg, field, value)
        out = C.c_void_p()
        assert lib.f5_wavlm_create(C.byref(cfg), C.byref(out)) == F5_EINVAL and not out.value
        assert word in _lib.last_error(), _lib.last_error()
    assert lib.f5_op_wavlm_attention(8, 4, 32, _lib.ptr(wave), _lib.ptr(wave), _lib.ptr(wave), _lib.ptr(hs), _lib.stream_ptr()) == F5_EINVAL
    with pytest.raises(ValueError, match="feat_extract_norm"):
        WavLMExtractor(**dict(TINY, feat_extract_norm="group"))
