"""Host reference of the attention-dropout mask (eraxvif5tts_amd/csrc/philox.h): a numpy Philox4x32-10 and the keep mask
of one attention call.  Plain module, no fixtures: the host and GPU tests import it."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)

# Random123 known-answer vectors of philox4x32-10 (kat_vectors): counter words, key words, output words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (broadcast against each other) of 32-bit words; returns the four output words as uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(a, dtype=np.uint64) & U32 for a in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0 = (k0 + np.uint64(W0)) & U32
        k1 = (k1 + np.uint64(W1)) & U32
    return tuple(a.astype(np.uint32) for a in (c0, c1, c2, c3))


def threshold(p):
    """T = round(p * 2^32): a probability is kept when its draw is >= T"""
    return int(round(p * 2.0 ** 32))


def keep_mask(seed, stream, batch0, B, H, N, p):
    """bool [B, H, N(query), N(key)]: keep(q, k) of batch item b (batch word batch0 + b), head h, call word `stream`:
    (o0..o3) = Philox4x32-10(counter = (k >> 2, q, bw * H + head, stream), key = (seed & 0xffffffff, seed >> 32)); keep = o[k & 3] >= T."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nk4 = (N + 3) // 4
    kq = np.arange(nk4, dtype=np.uint64)[None, None, None, :]
    q = np.arange(N, dtype=np.uint64)[None, None, :, None]
    bh = (((np.arange(B, dtype=np.uint64) + np.uint64(batch0))[:, None] * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :]) & U32)[:, :, None, None]
    o = philox4x32_10(kq, q, bh, int(stream) & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)
    draws = np.stack(o, axis=-1).reshape(B, H, N, 4 * nk4)[..., :N]  # word j of call kq decides key 4 * kq + j
    return draws >= np.uint32(threshold(p)) if threshold(p) < 2 ** 32 else np.zeros_like(draws, dtype=bool)


def sigma_of(n, p=0.1):
    """standard deviation of the keep fraction over n independent draws"""
    return float(np.sqrt(p * (1.0 - p) / n))


# ---- what the GPU op tests (tests/test_gpu_attention_dropout.py) draw masks for: (seed, stream, batch0, (B, H, N)); the host test checks
#      every one of them for its keep fraction, so the GPU-side fraction test is satisfiable by the reference alone
P = 0.1
SEED, STREAM, BATCH0 = 1234, 0x10003, 5
SEED_HI = 0x123456789ABCDEF0  # (a seed whose high word matters: the 64-bit seed crosses the ABI whole)
READBACK_SHAPES = [(2, 2, 64), (1, 3, 41), (2, 2, 200), (1, 1, 320)]                           # (B, H, N)
PARITY_SHAPES = [(2, 56, 2, True), (1, 41, 2, False), (2, 200, 3, True), (1, 320, 2, False), (3, 333, 1, True), (2, 1024, 4, True)]  # (B, N, H, masked)
MASK_CASES = ([(SEED, STREAM, BATCH0, s) for s in READBACK_SHAPES] + [(SEED_HI, STREAM, BATCH0, (B, H, N)) for B, N, H, _ in PARITY_SHAPES] +
              [(SEED, STREAM, BATCH0, (2, 2, 200)), (SEED ^ (1 << 40), STREAM, BATCH0, (2, 2, 200)), (SEED, STREAM + 1, BATCH0, (2, 2, 200)),
               (SEED, STREAM, BATCH0 + 1, (2, 2, 200))] + [(SEED, st, BATCH0, (2, 2, 200)) for st in range(64)])
