"""The speaker-similarity head on the device (include/f5hip.h: f5_speaker_*, f5_op_speaker_*; csrc/speaker.hip) and its Python surface
(eraxvif5tts_amd/eval/speaker.py) against tests/speaker_ref.py and the tensors captured from the reference (tests/golden/speaker.npz).

Bound of every comparison with a reference (the form tests/test_gpu_bigvgan_widths.py uses for fp32 kernels), measured against the reference
side, never the code under test -- with ref64 the restatement in fp64 and ref32 the same torch graph in fp32 on the CPU, both on the same fp32
inputs:
    rel-L2(gpu, ref64) <= 8 x rel-L2(ref32, ref64)   and   <= 1e-4
    max|gpu - ref64|   <= 8 x max|ref32 - ref64| + 2^-23 max|ref64|
(for the golden parity ref32 is the fixture itself: the reference module's own fp32 output).  The restatement's fp32 error is 1e-7 .. 4e-7
relative at both widths, so the margin is not tight; tools/speaker_ab.py writes the measured figures to profiles/speaker_ab.txt.
Shapes: T in {2, 3, 5, 9, 37, 150} -- shorter than every dilation (2, 3, 4) and than the k = 5 kernel, odd, not a multiple of the 64-row GEMM
tile or the 4-way time split of the statistics -- at the golden width (C = 64: Res2 width 8, the GEMM's padded-K and narrow-N paths) and the
production width (F 1024, C 512, L 25, emb 256) at T = 37 and 150.
Ragged calls are compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import speaker_ref as R
from conftest import load_golden
from eraxvif5tts_amd import _lib
from eraxvif5tts_amd.eval import SpeakerEncoder, speaker_similarity

pytestmark = pytest.mark.gpu
CONFIGS = {"golden": R.GOLDEN_CONFIG, "production": R.PRODUCTION_CONFIG}
SHAPES = [("golden", T) for T in (2, 3, 5, 9, 37, 150)] + [("production", 37), ("production", 150)]
OPS = ("featnorm", "layer1", "conv1x1", "res2.layer2", "res2.layer3", "res2.layer4", "se", "pool", "embed")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


# ----------------------------------------------------------------------------- shared references (computed once, never modified)
@functools.lru_cache(maxsize=None)
def _params(name):
    P32 = R.filled_state(CONFIGS[name])
    return P32, R.to_dtype(P32, torch.float64)


@functools.lru_cache(maxsize=None)
def _encoder(name):
    return SpeakerEncoder(**CONFIGS[name]).load_state_dict(_params(name)[0])


def _both(fn, P32, P64, *xs):
    with torch.no_grad():
        return fn(P32, *xs), fn(P64, *[x.double() for x in xs])


@functools.lru_cache(maxsize=None)
def reference(name, T):
    """op -> (fp32 inputs, ref32, ref64): every op's input is the fp32 restatement's own tensor at that point of one forward pass."""
    cfg = CONFIGS[name]
    P32, P64 = _params(name)
    sc = cfg["scale"]
    hs = R.hidden_states(T, cfg)
    ref = {}
    ref["featnorm"] = ((hs,),) + _both(lambda P, h: R.featnorm(h, P["feature_weight"]), P32, P64, hs)
    x0 = ref["featnorm"][1]
    ref["layer1"] = ((x0,),) + _both(lambda P, x: R.conv_relu_bn(x, P, "layer1.conv", "layer1.bn"), P32, P64, x0)
    out1 = ref["layer1"][1]
    ref["conv1x1"] = ((out1,),) + _both(lambda P, x: R.conv_relu_bn(x, P, "layer2.Conv1dReluBn1.conv", "layer2.Conv1dReluBn1.bn"), P32, P64, out1)
    y1 = ref["conv1x1"][1]
    for b in (2, 3, 4):
        ref[f"res2.layer{b}"] = ((y1,),) + _both(lambda P, x, b=b: R.res2(x, P, f"layer{b}.Res2Conv1dReluBn", sc, R.DILATIONS[b]), P32, P64, y1)
    with torch.no_grad():
        y3 = R.conv_relu_bn(ref["res2.layer2"][1], P32, "layer2.Conv1dReluBn2.conv", "layer2.Conv1dReluBn2.bn")
    ref["se"] = ((y3, out1),) + _both(lambda P, x, r: R.se(x, P, "layer2.SE_Connect") + r, P32, P64, y3, out1)
    t32 = {}
    with torch.no_grad():
        e32 = R.forward(P32, hs, cfg, t32)
        e64 = R.forward(P64, hs.double(), cfg)
    ref["pool"] = ((t32["conv"],),) + _both(lambda P, x: R.pool(x, P), P32, P64, t32["conv"])
    ref["embed"] = ((hs,), e32, e64)
    return ref


# ----------------------------------------------------------------------------- the device side
def _frames(frames):
    return (C.c_int32 * len(frames))(*frames)


def _host(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return a, a.ctypes.data


def _tm(x):
    """reference layout [1, C, T] -> time-major [T, C] on the device"""
    return x[0].t().contiguous().cuda()


def _cm(y):
    """time-major [T, C] device -> [1, C, T] on the host"""
    return y.t().contiguous().unsqueeze(0).cpu()


def _bn_host(P, prefix):
    return _host(torch.stack([P[prefix + ".weight"], P[prefix + ".bias"], P[prefix + ".running_mean"], P[prefix + ".running_var"]]))


def op_conv(P, conv, bn, dil, xs, frames):
    """xs: time-major [rows, cin] on the device"""
    lib = _lib.load()
    w = P[conv + ".weight"]
    cout, cin, k = w.shape
    (wa, wp), (ba, bp), (na, np_) = _host(w), _host(P[conv + ".bias"]), _bn_host(P, bn)
    out = torch.full((xs.shape[0], cout), float("nan"), device="cuda")
    _lib.check(lib.f5_op_speaker_conv_relu_bn(len(frames), _frames(frames), cin, cout, k, dil, _lib.ptr(xs), wp, bp, np_, R.BN_EPS, _lib.ptr(out),
                                              _lib.stream_ptr()), "op_speaker_conv_relu_bn")
    return out


def op_res2(P, prefix, scale, dil, xs, frames):
    lib = _lib.load()
    Cc = xs.shape[1]
    (wa, wp) = _host(torch.stack([P[f"{prefix}.convs.{i}.weight"] for i in range(scale - 1)]))
    (ba, bp) = _host(torch.stack([P[f"{prefix}.convs.{i}.bias"] for i in range(scale - 1)]))
    (na, np_) = _host(torch.stack([torch.stack([P[f"{prefix}.bns.{i}.{f}"] for f in ("weight", "bias", "running_mean", "running_var")])
                                   for i in range(scale - 1)]))
    out = torch.full_like(xs, float("nan"))
    _lib.check(lib.f5_op_speaker_res2(len(frames), _frames(frames), Cc, scale, dil, _lib.ptr(xs), wp, bp, np_, R.BN_EPS, _lib.ptr(out), _lib.stream_ptr()),
               "op_speaker_res2")
    return out


def op_se(P, prefix, xs, resid, frames):
    lib = _lib.load()
    Cc = xs.shape[1]
    (a1, p1), (a2, p2) = _host(P[prefix + ".linear1.weight"]), _host(P[prefix + ".linear1.bias"])
    (a3, p3), (a4, p4) = _host(P[prefix + ".linear2.weight"]), _host(P[prefix + ".linear2.bias"])
    out = torch.full_like(xs, float("nan"))
    _lib.check(lib.f5_op_speaker_se(len(frames), _frames(frames), Cc, a1.shape[0], _lib.ptr(xs), _lib.ptr(resid), p1, p2, p3, p4, _lib.ptr(out),
                                    _lib.stream_ptr()), "op_speaker_se")
    return out


def op_pool(P, xs, frames, prefix="pooling"):
    lib = _lib.load()
    Cc = xs.shape[1]
    (a1, p1), (a2, p2) = _host(P[prefix + ".linear1.weight"]), _host(P[prefix + ".linear1.bias"])
    (a3, p3), (a4, p4) = _host(P[prefix + ".linear2.weight"]), _host(P[prefix + ".linear2.bias"])
    out = torch.full((len(frames), 2 * Cc), float("nan"), device="cuda")
    _lib.check(lib.f5_op_speaker_pool(len(frames), _frames(frames), Cc, a1.shape[0], _lib.ptr(xs), p1, p2, p3, p4, _lib.ptr(out), _lib.stream_ptr()),
               "op_speaker_pool")
    return out


def op_featnorm(P, hs, frames):
    """hs [L, rows, F] on the device"""
    lib = _lib.load()
    L, rows, Fd = hs.shape
    (fa, fp) = _host(P["feature_weight"])
    out = torch.full((rows, Fd), float("nan"), device="cuda")
    _lib.check(lib.f5_op_speaker_featnorm(len(frames), _frames(frames), L, Fd, _lib.ptr(hs), fp, _lib.ptr(out), _lib.stream_ptr()), "op_speaker_featnorm")
    return out


def run_op(name, op, inputs):
    """One utterance through the device form of `op`; the result in the reference's layout, on the host."""
    cfg, P = CONFIGS[name], _params(name)[0]
    T = inputs[0].shape[1] if op in ("featnorm", "embed") else inputs[0].shape[2]
    if op == "featnorm":
        return _cm(op_featnorm(P, inputs[0].cuda().contiguous(), [T]))
    if op == "layer1":
        return _cm(op_conv(P, "layer1.conv", "layer1.bn", 1, _tm(inputs[0]), [T]))
    if op == "conv1x1":
        return _cm(op_conv(P, "layer2.Conv1dReluBn1.conv", "layer2.Conv1dReluBn1.bn", 1, _tm(inputs[0]), [T]))
    if op.startswith("res2."):
        b = int(op[-1])
        return _cm(op_res2(P, f"layer{b}.Res2Conv1dReluBn", cfg["scale"], R.DILATIONS[b], _tm(inputs[0]), [T]))
    if op == "se":
        return _cm(op_se(P, "layer2.SE_Connect", _tm(inputs[0]), _tm(inputs[1]), [T]))
    if op == "pool":
        return op_pool(P, _tm(inputs[0]), [T]).cpu()
    if op == "embed":
        return _encoder(name).embed([inputs[0].cuda()]).cpu()
    raise KeyError(op)


def figures(gpu, ref32, ref64):
    gpu, ref32, ref64 = gpu.double(), ref32.double(), ref64.double()
    return dict(rel_gpu=R.rel_l2(gpu, ref64), rel_ref=R.rel_l2(ref32, ref64), max_gpu=float((gpu - ref64).abs().max()),
                max_ref=float((ref32 - ref64).abs().max()), scale=float(ref64.abs().max()))


def assert_bound(f, what):
    print(f"{what}: rel-L2 gpu {f['rel_gpu']:.3e} ref32 {f['rel_ref']:.3e} (x{f['rel_gpu'] / max(f['rel_ref'], 1e-300):.2f}); "
          f"max-abs gpu {f['max_gpu']:.3e} ref32 {f['max_ref']:.3e}; max|ref64| {f['scale']:.3e}")
    assert f["rel_gpu"] <= 8 * f["rel_ref"] and f["rel_gpu"] <= 1e-4, (what, f)
    assert f["max_gpu"] <= 8 * f["max_ref"] + 2.0 ** -23 * f["scale"], (what, f)


def measure(name, T, op):
    inputs, ref32, ref64 = reference(name, T)[op]
    gpu = run_op(name, op, inputs)
    assert gpu.shape == ref64.shape, (op, gpu.shape, ref64.shape)
    assert torch.isfinite(gpu).all(), op
    return figures(gpu, ref32, ref64)


# ----------------------------------------------------------------------------- 1. golden parity
@functools.lru_cache(maxsize=None)
def _golden():
    z = load_golden("speaker")
    for v in z.values():
        v.setflags(write=False)
    return z


@pytest.mark.parametrize("T", (2, 3, 9, 23))
def test_golden_parity(T):
    z, cfg = _golden(), R.GOLDEN_CONFIG
    enc, lib = _encoder("golden"), _lib.load()
    P64 = _params("golden")[1]
    hs = torch.from_numpy(z[f"T{T}.hs"].copy())
    widths = {"instance_norm": cfg["feat_dim"], "layer1": cfg["channels"], "layer2": cfg["channels"], "layer3": cfg["channels"], "layer4": cfg["channels"],
              "conv": cfg["cat_channels"]}
    bufs = {n: torch.full((T, w), float("nan"), device="cuda") for n, w in widths.items()}
    bufs["pooling"] = torch.full((1, 2 * cfg["cat_channels"]), float("nan"), device="cuda")
    hd = enc.native()
    try:
        for n, b in bufs.items():
            _lib.check(lib.f5_speaker_set_tap(hd, n.encode(), _lib.ptr(b)), "speaker_set_tap")
        emb = enc.embed([hs.cuda()])
        torch.cuda.synchronize()
    finally:
        for n in bufs:
            lib.f5_speaker_set_tap(hd, n.encode(), None)
    t64 = {}
    with torch.no_grad():
        t64["emb"] = R.forward(P64, hs.double(), cfg, t64)
    got = {n: (_cm(b) if n != "pooling" else b.cpu()) for n, b in bufs.items()}
    got["emb"] = emb.cpu()
    for n in R.TAPS + ("emb",):
        gold = torch.from_numpy(z[f"T{T}.{n}"].copy())
        assert got[n].shape == gold.shape, n
        assert torch.isfinite(got[n]).all(), n
        assert_bound(figures(got[n], gold, t64[n]), f"golden T={T} {n}")


# ----------------------------------------------------------------------------- 2. per op against the fp64 restatement
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name,T", SHAPES)
def test_op_against_fp64(name, T, op):
    assert_bound(measure(name, T, op), f"{name} T={T} {op}")


# ----------------------------------------------------------------------------- 3. hazard cells: a condition on the reference alone
def hazard_cells(name, T):
    """pooling cells of the fp64 reference with a residual strictly between 0 and 1e-6, in the full forward pass and in the pool op's own input"""
    P64 = _params(name)[1]
    ref = reference(name, T)
    with torch.no_grad():
        t64 = {}
        R.forward(P64, ref["embed"][0][0].double(), CONFIGS[name], t64)
        _, full = R.pool_residuals(t64["conv"], P64)
        _, own = R.pool_residuals(ref["pool"][0][0].double(), P64)
    return [int(((r > 0) & (r < 1e-6)).sum()) for r in (full, own)], int((full == 0).sum())


@pytest.mark.parametrize("name,T", SHAPES + [("golden", 23)])
def test_no_hazard_cells_in_the_reference(name, T):
    hazards, zeros = hazard_cells(name, T)
    print(f"{name} T={T}: hazard cells {hazards}, exactly-zero cells {zeros}")
    assert hazards == [0, 0], "change the seed in speaker_ref.SEEDS, not the bound"
    assert zeros > 0  # the all-zero channels behind the ReLU occur for real: both sides give sqrt(1e-9) there


def test_constant_channels_pool_to_the_clamp():
    """A channel that is zero in every frame, and one that holds a constant (a power of two: every product is exact), have residual exactly 0:
    the pooled std is sqrt(float32(1e-9)) to the bit, the mean the constant."""
    cfg, P = R.GOLDEN_CONFIG, _params("golden")[0]
    Cc, frames = cfg["cat_channels"], [2, 9, 37]
    rs = np.random.RandomState(5)
    x = torch.from_numpy(np.maximum(rs.standard_normal((sum(frames), Cc)), 0).astype(np.float32))
    x[:, 3] = 0.0
    x[:, 70] = 0.03125
    out = op_pool(P, x.cuda(), frames).cpu()
    want = torch.sqrt(torch.tensor(1e-9, dtype=torch.float32))
    for u in range(len(frames)):
        assert out[u, Cc + 3] == want and out[u, Cc + 70] == want, (u, out[u, Cc + 3].item(), out[u, Cc + 70].item())
        assert out[u, 3] == 0.0 and out[u, 70] == 0.03125
    assert torch.isfinite(out).all() and (out[:, Cc:] >= want).all()


# ----------------------------------------------------------------------------- 4. ragged = batch-1, bit for bit
def _utts(frames, seed=100):
    cfg = R.GOLDEN_CONFIG
    return [R.hidden_states(t, cfg, seed=seed + i).cuda() for i, t in enumerate(frames)]


def test_ragged_call_equals_single_calls():
    enc = _encoder("golden")
    utts = _utts((2, 150, 3, 37, 9))
    together = enc.embed(utts)
    alone = torch.cat([enc.embed([u]) for u in utts])
    assert torch.isfinite(together).all()
    assert torch.equal(together, alone)
    assert torch.equal(together, enc.embed(utts))  # the same call twice
    stacked = torch.stack([utts[4], utts[4], utts[4]], dim=1)  # the [L, B, T, F] form
    assert torch.equal(enc.embed(stacked), together[4:5].expand(3, -1))


def test_seventy_utterances_cross_the_table_boundary():
    enc = _encoder("golden")
    frames = [2 + (i * 5) % 8 for i in range(70)]
    utts = _utts(frames, seed=300)
    together = enc.embed(utts)
    assert together.shape == (70, R.GOLDEN_CONFIG["emb_dim"]) and torch.isfinite(together).all()
    for i in (0, 1, 61, 62, 63, 64, 65, 66, 68, 69):
        assert torch.equal(together[i: i + 1], enc.embed([utts[i]])), i
    assert torch.equal(together, enc.embed(utts))


@pytest.mark.parametrize("junk", (1e30, float("nan")))
def test_neighbours_do_not_change_an_utterance(junk):
    """A convolution tap, a statistic or a softmax that read past the utterance's edge would meet 1e30 or NaN there."""
    enc, cfg = _encoder("golden"), R.GOLDEN_CONFIG
    for T in (2, 9, 37):
        (u,) = _utts((T,), seed=500 + T)
        alone = enc.embed([u])
        for tj in (2, 5):
            j = torch.full((cfg["layers"], tj, cfg["feat_dim"]), junk, device="cuda")
            got = enc.embed([j, u, j])
            assert torch.equal(got[1:2], alone), (T, tj)
    # the same at op level, where the junk sits in the activations themselves (the head's instance norm would launder a constant)
    P = _params("golden")[0]
    frames = [4, 9, 3]
    rs = np.random.RandomState(9)
    for Cc, run in ((cfg["channels"], lambda x, f: op_res2(P, "layer4.Res2Conv1dReluBn", cfg["scale"], 4, x, f)),
                    (cfg["feat_dim"], lambda x, f: op_conv(P, "layer1.conv", "layer1.bn", 1, x, f)),
                    (cfg["channels"], lambda x, f: op_se(P, "layer3.SE_Connect", x, x, f)),
                    (cfg["cat_channels"], lambda x, f: op_pool(P, x, f))):
        mid = torch.from_numpy(rs.standard_normal((frames[1], Cc)).astype(np.float32)).cuda()
        x = torch.cat([torch.full((frames[0], Cc), junk, device="cuda"), mid, torch.full((frames[2], Cc), junk, device="cuda")])
        got, alone = run(x, frames), run(mid, [frames[1]])
        if got.shape[0] == len(frames):  # the pool: one row per utterance
            assert torch.equal(got[1:2], alone)
        else:
            assert torch.equal(got[frames[0]: frames[0] + frames[1]], alone)


# ----------------------------------------------------------------------------- 5. end to end with a stand-in extractor
class StandInExtractor:
    """Not WavLM: frames of 400 samples every 320 (25 ms / 20 ms at 16 kHz), a fixed random projection per layer and a tanh.  Records what it
    returned, so that the restatement embeds the very same hidden states."""

    def __init__(self, cfg, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.proj = (torch.randn(cfg["layers"], 400, cfg["feat_dim"], generator=g) / 4.0).cuda()
        self.bias = torch.randn(cfg["layers"], 1, cfg["feat_dim"], generator=g).cuda()
        self.seen = []

    def __call__(self, waves):
        assert len(waves) == 1 and waves[0].ndim == 1 and waves[0].is_cuda
        fr = waves[0].unfold(0, 400, 320)  # [T, 400]
        hs = torch.tanh(torch.einsum("tk,lkf->ltf", fr, self.proj) + self.bias)
        self.seen.append(hs.cpu())
        return {"hidden_states": [hs[l].unsqueeze(0) for l in range(hs.shape[0])]}


def test_similarity_end_to_end():
    cfg, enc = R.GOLDEN_CONFIG, _encoder("golden")
    P32, P64 = _params("golden")
    g = torch.Generator().manual_seed(11)
    n = 8
    waves = [0.1 * torch.randn(2400 + 480 * i, generator=g) for i in range(2 * n)]  # 24 kHz: 0.1 .. 0.4 s
    pairs = [(waves[2 * i], waves[2 * i + 1]) for i in range(n - 1)] + [(waves[0], waves[0])]
    ext = StandInExtractor(cfg)
    sim, mean = speaker_similarity(enc, pairs, ext, sample_rate=24000)
    assert sim.shape == (n,) and sim.is_cuda and len(ext.seen) == 2 * n
    sim = sim.cpu()
    assert abs(mean - float(sim.mean())) <= 2.0 ** -22
    with torch.no_grad():
        e32 = R.embed_ragged(P32, ext.seen, cfg)
        e64 = R.embed_ragged(P64, [h.double() for h in ext.seen], cfg)
    cos = lambda e: torch.nn.functional.cosine_similarity(e[0::2], e[1::2])  # noqa: E731
    assert_bound(figures(sim, cos(e32), cos(e64)), "similarity end to end")
    assert abs(float(sim[n - 1]) - 1.0) <= 2.0 ** -22  # a wave paired with itself
    with pytest.raises(ValueError, match="feature_extractor"):
        speaker_similarity(enc, pairs, None)


# ----------------------------------------------------------------------------- 6. production key names
def test_production_checkpoint_names_load_and_run():
    cfg = R.PRODUCTION_CONFIG
    sd = dict(_params("production")[0])
    for bn in [k[: -len(".running_var")] for k in sd if k.endswith(".running_var")]:
        sd[bn + ".num_batches_tracked"] = torch.tensor(1234)
    sd["feature_extract.foo"] = torch.zeros(4)
    sd["feature_extract.model.encoder.layers.23.self_attn.k_proj.weight"] = torch.zeros(2, 2)
    enc = SpeakerEncoder().load_state_dict(sd)  # the defaults are the production head
    hs = R.hidden_states(37, cfg).cuda()
    emb = enc.embed([hs])
    assert emb.shape == (1, 256) and torch.isfinite(emb).all()
    assert torch.equal(emb, _encoder("production").embed([hs]))
    lib = _lib.load()
    for skipped in ("feature_extract.foo", "bn.num_batches_tracked"):
        assert lib.f5_speaker_has_tensor(enc.native(), skipped.encode(), None) == 0
    # a global_context_att pooling is refused by the library itself, with a message
    shape = (C.c_int64 * 3)(cfg["attention_channels"], 3 * cfg["cat_channels"], 1)
    w = np.zeros((cfg["attention_channels"], 3 * cfg["cat_channels"], 1), np.float32)
    hd = C.c_void_p()
    _lib.check(lib.f5_speaker_create(C.byref(_lib.SpeakerConfig(**cfg)), C.byref(hd)), "speaker_create")
    try:
        assert lib.f5_speaker_set_tensor(hd, b"pooling.linear1.weight", w.ctypes.data, shape, 3) == _lib.F5_ENOTSUP
        assert "global_context_att" in _lib.last_error()
        assert lib.f5_speaker_finalize(hd) != 0 and "was never set" in _lib.last_error()
        one = (C.c_int32 * 2)(5, 1)
        assert lib.f5_speaker_embed_ragged(hd, 2, one, None, None, None) != 0
    finally:
        lib.f5_speaker_destroy(hd)
    # frames < 2 is refused by the library before any launch
    hs2 = torch.zeros(cfg["layers"], 6, cfg["feat_dim"], device="cuda")
    out = torch.zeros(2, 256, device="cuda")
    assert lib.f5_speaker_embed_ragged(enc.native(), 2, one, _lib.ptr(hs2), _lib.ptr(out), _lib.stream_ptr()) == -1
    assert "at least 2" in _lib.last_error()
