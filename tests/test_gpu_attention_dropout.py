"""Attention dropout at op level (include/f5hip.h: f5_op_attention_dropout): the three kernels that realise the mask -- the
reference kernel's dropout build in fp32 and bf16, and the bf16 MFMA flash kernel of attention_dropout.hip -- against the host mask of
tests/dropout_ref.py.  The mask is read back bit for bit through one-hot values, the outputs are held against fp64 math on the same mask, and
the mode's statistics (keep fraction, unbiasedness) and its determinism are checked.  p = 0.1 throughout."""
import functools

import pytest
import torch

import dropout_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
P_BF16, P_FP32 = 0, 1
KERNELS = [(P_FP32, 0), (P_BF16, 0), (P_BF16, 1)]
KERNEL_IDS = ["fp32_reference", "bf16_reference", "bf16_mfma"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from eraxvif5tts_amd import _lib
    _lib.require_gpu()


def op_attention_dropout(precision, kernel, qkv, mask=None, p=R.P, seed=R.SEED, stream=R.STREAM, batch0=R.BATCH0):
    from eraxvif5tts_amd import _lib
    lib = _lib.load()
    B, N, three, H, dh = qkv.shape
    assert three == 3 and dh == 64
    q = qkv.cuda().float().contiguous()
    mk = None if mask is None else mask.cuda().to(torch.uint8).contiguous()
    out = torch.empty(B, N, H * 64, device="cuda")
    _lib.check(lib.f5_op_attention_dropout(precision, kernel, B, N, H, _lib.ptr(q), _lib.ptr(mk), p, seed, stream, batch0, _lib.ptr(out), _lib.stream_ptr()),
               "f5_op_attention_dropout")
    return out.cpu()


def _bf16(t):
    return t.to(torch.bfloat16).float()


def _host_mask(seed, stream, batch0, B, H, N):
    return torch.from_numpy(R.keep_mask(seed, stream, batch0, B, H, N, R.P))


def _attn_fp64(qkv, mask, keep=None, p=R.P):
    """softmax over the valid keys in fp64; with `keep` [B, H, N, N]: the kept probabilities, divided by 1 - p"""
    q, k, v = [qkv[:, :, i].transpose(1, 2).double() for i in range(3)]  # [B, H, N, 64]
    s = q @ k.transpose(-1, -2) / 8.0
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.double() / (1.0 - p)
    return (pr @ v).transpose(1, 2).reshape(qkv.shape[0], qkv.shape[1], -1)


# ----------------------------------------------------------------------------- 1. the mask, read back
@pytest.mark.parametrize("prec,kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("B,H,N", R.READBACK_SHAPES)
def test_mask_read_back_equals_the_host_mask(prec, kernel, B, H, N):
    """v[k] = e_(k - k0) inside a 64-key window and 0 elsewhere: out[q, j] is P[q, k0 + j] / 0.9 where the key was kept and exactly 0 where it
    was dropped (P > 0 on every valid key: scores of 0.5 randn stay far from underflow)."""
    g = torch.Generator().manual_seed(B * 1000 + N)
    lens = {200: [200, 187]}.get(N)
    windows = {64: [0], 41: [0], 200: [0, 64, 136], 320: [0, 256]}[N]
    mask = None if lens is None else torch.arange(N)[None, :] < torch.tensor(lens)[:, None]
    qkv = _bf16(0.5 * torch.randn(B, N, 3, H, 64, generator=g))
    want = _host_mask(R.SEED, R.STREAM, R.BATCH0, B, H, N)
    got = torch.zeros(B, H, N, N, dtype=torch.bool)
    seen = torch.zeros(N, dtype=torch.bool)
    for k0 in windows:
        w = min(64, N - k0)
        qkv[:, :, 2] = 0.0
        for j in range(w):
            qkv[:, k0 + j, 2, :, j] = 1.0
        out = op_attention_dropout(prec, kernel, qkv, mask).view(B, N, H, 64).permute(0, 2, 1, 3)  # [B, H, q, j]
        got[:, :, :, k0:k0 + w] = out[..., :w] != 0
        seen[k0:k0 + w] = True
    valid = torch.ones(B, 1, 1, N, dtype=torch.bool) if mask is None else mask[:, None, None, :]
    valid = (valid & seen[None, None, None, :]).expand(B, H, N, N)  # (the windows need not cover every key)
    assert not (got & ~valid).any(), "a masked key contributed"
    assert torch.equal(got[valid], want[valid]), f"{int((got[valid] != want[valid]).sum())} mask bits differ"
    n = int(valid.sum())
    dev = (float(got[valid].double().mean()) - (1.0 - R.P)) / R.sigma_of(n)
    print(f"  keep fraction {float(got[valid].double().mean()):.5f} over {n} draws: {dev:+.2f} sigma")
    assert abs(dev) < 5.0


# ----------------------------------------------------------------------------- 2. parity with fp64 on the host mask
@functools.lru_cache(maxsize=None)
def _parity_case(B, N, H, masked):
    g = torch.Generator().manual_seed(N + H)
    qkv = _bf16(torch.randn(B, N, 3, H, 64, generator=g) * 1.5)  # the inputs of tests/test_gpu_ops.py::test_attention_tuned_kernel
    mask = None
    if masked:
        lens = torch.tensor([N, max(1, N - 13), max(1, N // 2)][:B])
        mask = torch.arange(N)[None, :] < lens[:, None]
    keep = _host_mask(R.SEED_HI, R.STREAM, R.BATCH0, B, H, N)
    return qkv, mask, _attn_fp64(qkv, mask), _attn_fp64(qkv, mask, keep)


@pytest.mark.parametrize("prec,kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("B,N,H,masked", R.PARITY_SHAPES)
def test_parity_with_fp64_on_the_host_mask(prec, kernel, B, N, H, masked):
    """fp32 reference kernel: the 3e-6 of test_attention_reference_kernel.  bf16 kernels: no more than 1.5 x the error the corresponding
    kernel WITHOUT dropout makes on the same inputs (measured here; expected ratio ~1.05: the same rounding noise over 90 % of the terms,
    scaled by 1 / 0.9 -- the factor leaves room for another valid summation order), and inside the bounds the existing tests state for them
    (4e-3 reference kernel, 6e-3 tuned kernel)."""
    import gpu_helpers as G
    qkv, mask, ref0, ref = _parity_case(B, N, H, masked)
    out = op_attention_dropout(prec, kernel, qkv, mask, seed=R.SEED_HI)
    assert torch.isfinite(out).all()
    err = rel_l2(out, ref)
    if prec == P_FP32:
        print(f"  rel-L2 {err:.3e}")
        assert err < 3e-6
        return
    err0 = rel_l2(G.op_attention(P_BF16, kernel, qkv, mask), ref0)
    print(f"  rel-L2 {err:.3e} with dropout, {err0:.3e} without: ratio {err / err0:.3f}")
    assert err <= 1.5 * err0
    assert err < (4e-3 if kernel == 0 else 6e-3)


# ----------------------------------------------------------------------------- 3. prob = 0
@pytest.mark.parametrize("prec,kernel", KERNELS, ids=KERNEL_IDS)
def test_prob_zero_gives_the_bits_of_op_attention(prec, kernel):
    import gpu_helpers as G
    B, N, H = 2, 200, 2
    g = torch.Generator().manual_seed(3)
    qkv = _bf16(torch.randn(B, N, 3, H, 64, generator=g))
    mask = torch.arange(N)[None, :] < torch.tensor([200, 187])[:, None]
    assert torch.equal(op_attention_dropout(prec, kernel, qkv, mask, p=0.0), G.op_attention(prec, kernel, qkv, mask))


# ----------------------------------------------------------------------------- 4. determinism and sensitivity
@functools.lru_cache(maxsize=None)
def _plain_case():
    g = torch.Generator().manual_seed(200)
    return _bf16(torch.randn(2, 200, 3, 2, 64, generator=g))


@pytest.mark.parametrize("prec,kernel", KERNELS, ids=KERNEL_IDS)
def test_deterministic_and_sensitive_to_every_mask_word(prec, kernel):
    """Same arguments: same bits.  Another seed (high word), call word or batch word: another mask -- two independent masks differ by 0.3 .. 0.45
    rel-L2 on randn inputs, 0.05 is far below that and far above rounding."""
    qkv = _plain_case()
    a = op_attention_dropout(prec, kernel, qkv)
    assert torch.equal(a, op_attention_dropout(prec, kernel, qkv))
    for kw in (dict(seed=R.SEED ^ (1 << 40)), dict(stream=R.STREAM + 1), dict(batch0=R.BATCH0 + 1)):
        d = rel_l2(op_attention_dropout(prec, kernel, qkv, **kw), a)
        print(f"  {kw}: rel-L2 {d:.3f}")
        assert d > 0.05, kw


def test_bf16_kernels_realise_the_same_mask():
    """reference kernel and MFMA kernel, same arguments: each lies within its own bound of the exact sum over the same kept terms (4e-3 and
    6e-3, so at most 1e-2 apart; 1.2e-2 asked); another mask would give ~0.4"""
    qkv = _plain_case()
    d = rel_l2(op_attention_dropout(P_BF16, 1, qkv), op_attention_dropout(P_BF16, 0, qkv))
    print(f"  rel-L2 {d:.3e}")
    assert d <= 1.2e-2


# ----------------------------------------------------------------------------- 5. unbiasedness
@pytest.mark.parametrize("prec,kernel", [KERNELS[0], KERNELS[2]], ids=[KERNEL_IDS[0], KERNEL_IDS[2]])
def test_mean_over_64_call_words_approaches_the_undropped_output(prec, kernel):
    """E[keep / (1 - p)] = 1: the mean over 64 independent masks is sqrt(64) = 8 times closer to the no-dropout output than one run; asked: 4."""
    import gpu_helpers as G
    qkv = _plain_case()
    plain = G.op_attention(prec, kernel, qkv, None)
    runs = [op_attention_dropout(prec, kernel, qkv, stream=st) for st in range(64)]
    one = rel_l2(runs[0], plain)
    mean = rel_l2(torch.stack(runs).double().mean(0), plain)
    print(f"  one run {one:.4f}, mean of 64 {mean:.4f}: ratio {one / mean:.2f}")
    assert mean <= one / 4
