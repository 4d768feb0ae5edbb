"""Host restatement (numpy) of the duration-validation path, shared by tests/test_alignment_host.py, tests/test_gpu_alignment.py and
tools/: the two monotonic alignment searches in the reference's fp32 arithmetic (exact: compared bit for bit), the similarity block and
the loss in fp64 (compared with derived tolerances), and the seeded cases the golden fixture tests/golden/alignment.npz was captured on.

Reference: model/alignment_utils.py:154-258 (searches), model/trainer.py:925-970 (similarity), :984-1025 (loss)."""
import hashlib

import numpy as np

ALGORITHMS = ("viterbi", "window")
STORE_LIMIT = 4096  # the fixture stores a case's similarity input up to this many elements, and its SHA-256 beyond


# ----------------------------------------------------------------------------- the searches, exact
def viterbi_path_prob(sim):
    """P [B, nt, T] in fp32, every cell one fp32 add in the reference's association; cells are visited by anti-diagonals (each needs only
    its upper and left neighbour, so the visiting order changes no bit)."""
    sim = np.asarray(sim, np.float32)
    B, nt, T = sim.shape
    P = np.zeros_like(sim)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(nt + T - 1):
            n = np.arange(max(0, k - T + 1), min(nt - 1, k) + 1)
            t = k - n
            if k == 0:
                P[:, 0, 0] = sim[:, 0, 0]
                continue
            first_row, first_col = n == 0, t == 0
            inner = ~first_row & ~first_col
            if first_row.any():  # P[0,t] = P[0,t-1] + s[0,t]
                P[:, 0, k] = P[:, 0, k - 1] + sim[:, 0, k]
            if first_col.any():  # P[n,0] = P[n-1,0] + s[n,0]
                P[:, k, 0] = P[:, k - 1, 0] + sim[:, k, 0]
            ni, ti = n[inner], t[inner]
            if ni.size:
                P[:, ni, ti] = sim[:, ni, ti] + np.maximum(P[:, ni - 1, ti], P[:, ni, ti - 1])
    return P


def viterbi(sim):
    """alignment [B, nt, T] of 0 / 1 (fp32)."""
    P = viterbi_path_prob(sim)
    B, nt, T = P.shape
    out = np.zeros_like(P)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            curr = T - 1
            for n in range(nt - 1, -1, -1):
                boundary = 0
                if n > 0:
                    row = P[b, n, :curr + 1]
                    rising = np.nonzero(row[1:] - row[:-1] > 0)[0]  # fp32 differences; NaN compares false
                    if rising.size:
                        boundary = int(rising[-1])
                out[b, n, boundary:curr + 1] = 1
                curr = boundary - 1
                if curr < 0:
                    break
    return out


def window(sim, window_size=0.2):
    """alignment [B, nt, T] of 0 / 1 (fp32).  An empty search window (start > expected_end + window: only when nt > T; the reference raises on
    it) gives the row the single frame `start`, as f5_align_window documents."""
    sim = np.asarray(sim, np.float32)
    B, nt, T = sim.shape
    out = np.zeros_like(sim)
    width = max(2, int(T * window_size))
    frames_per_phone = T / nt
    for b in range(B):
        start = 0
        for n in range(nt - 1):
            expected_end = int((n + 1) * frames_per_phone)
            lo, hi = max(start, expected_end - width), min(T - 1, expected_end + width)
            best_end = lo + int(np.argmax(sim[b, n, lo:hi + 1])) if hi >= lo else lo
            out[b, n, start:best_end + 1] = 1
            start = best_end + 1
            if start >= T:
                break
        if start < T:
            out[b, nt - 1, start:] = 1
    return out


def window_has_empty_search(sim):
    """True when some row of some utterance meets an empty search window (where the reference raises)."""
    sim = np.asarray(sim, np.float32)
    B, nt, T = sim.shape
    width = max(2, int(T * 0.2))
    for b in range(B):
        start = 0
        for n in range(nt - 1):
            expected_end = int((n + 1) * (T / nt))
            lo, hi = max(start, expected_end - width), min(T - 1, expected_end + width)
            if hi < lo:
                return True
            start = lo + int(np.argmax(sim[b, n, lo:hi + 1])) + 1
            if start >= T:
                break
    return False


SEARCH = {"viterbi": viterbi, "window": window}


# ----------------------------------------------------------------------------- similarity and loss, fp64
def similarity64(embed, ids, p_lens, mel, m_lens, proj):
    """trainer.py:925-970 in fp64 from the fp32 inputs: [B, nt, T] with -inf on the padding."""
    embed, mel, proj = (np.asarray(a, np.float64) for a in (embed, mel, proj))
    ids = np.asarray(ids)
    B, nt = ids.shape
    T = mel.shape[1]
    e = embed[ids]
    e = e / (np.linalg.norm(e, axis=2, keepdims=True) + 1e-8)
    m = mel @ proj
    m = m / (np.linalg.norm(m, axis=2, keepdims=True) + 1e-8)
    sim = e @ m.transpose(0, 2, 1)
    for b in range(B):
        p_len, m_len = int(p_lens[b]), int(m_lens[b])
        if p_len > 0 and m_len > 0:
            for p in range(p_len):
                center = (p * m_len) // p_len
                width = max(3, m_len // 10)
                sim[b, p, max(0, center - width):min(m_len, center + width)] += 3.0
        sim[b, p_len:, :] = -np.inf
        sim[b, :, m_len:] = -np.inf
    return sim


def duration_loss64(logw, durations, p_lens):
    """trainer.py:984-1025 per utterance, in fp64 from the fp32 inputs: (sum of squared log error, sum of absolute duration error, count),
    math.fsum-exact, and the batch's (loss, mae) with the reference's + 1e-8 denominator."""
    import math
    logw, durations = np.asarray(logw, np.float32), np.asarray(durations, np.float32)
    B, nt = logw.shape
    sq, ab, cnt = [], [], []
    for b in range(B):
        n = max(0, min(nt, int(p_lens[b])))
        lw = logw[b, :n].astype(np.float64)
        d = np.maximum(durations[b, :n].astype(np.float64), 0.1)
        sq.append(math.fsum(((lw - np.log(d + 1e-6)) ** 2).tolist()))
        ab.append(math.fsum(np.abs(np.exp(np.clip(lw, -10.0, 10.0)) - d).tolist()))
        cnt.append(n)
    den = sum(cnt) + 1e-8
    return np.array(sq), np.array(ab), np.array(cnt, np.int64), math.fsum(sq) / den, math.fsum(ab) / den


# ----------------------------------------------------------------------------- the cases
def _hashed(B, nt, T, salt):
    """fp32 values in [-2, 2) from an integer hash of the cell: 24 significant bits, the same on every platform and numpy."""
    b = np.arange(B, dtype=np.int64)[:, None, None]
    n = np.arange(nt, dtype=np.int64)[None, :, None]
    t = np.arange(T, dtype=np.int64)[None, None, :]
    h = ((n * 73856093) ^ (t * 19349663) ^ ((b + salt) * 83492791)) & 0xFFFFFF
    return (h.astype(np.float64) / 2.0 ** 22 - 2.0).astype(np.float32)


def _ragged(seed):
    """B = 3 with unequal phoneme and mel lengths: -inf rows and columns, one utterance without phonemes."""
    rng = np.random.default_rng(seed)
    sim = rng.standard_normal((3, 7, 33)).astype(np.float32)
    for b, (p_len, m_len) in enumerate(RAGGED_LENS):
        sim[b, p_len:, :] = -np.inf
        sim[b, :, m_len:] = -np.inf
    return sim


RAGGED_LENS = ((7, 33), (4, 20), (0, 27))


def generate_cases():
    """name -> similarity fp32 [B, nt, T]: the smallest shapes at which the searches can go wrong (one row, one frame, more rows than frames,
    rows across a wave and across 256 lanes, frame counts off every tile, -inf padding, no positive entry, exact ties, and one production-size
    matrix for the window rule's float arithmetic)."""
    rng = np.random.default_rng(20240607)
    randn = lambda *s: rng.standard_normal(s).astype(np.float32)
    return {
        "nt1": randn(1, 1, 9),
        "T1": randn(2, 5, 1),
        "nt_gt_T": randn(2, 12, 5),
        "nt_gt_T_b": _hashed(3, 12, 5, 5),
        "nt70_T33": randn(1, 70, 33),
        "nt300_T257": _hashed(1, 300, 257, 1),
        "nt70_T257": _hashed(2, 70, 257, 3),  # (the reference's window search raises on the nt > T cases above: these two give it a golden
        "nt300_T333": _hashed(1, 300, 333, 4),  # at the same row counts)
        "nt1024_T64": _hashed(1, 1024, 64, 6),  # the largest row count: sixteen waves hand their last row on
        "ragged": _ragged(7),
        "all_negative": -np.abs(randn(1, 6, 20)) - np.float32(0.1),
        "const0": np.zeros((1, 5, 12), np.float32),
        "const1p5": np.full((1, 5, 12), 1.5, np.float32),
        "integer": rng.integers(-2, 3, (2, 8, 21)).astype(np.float32),
        "nt200_T1500": _hashed(1, 200, 1500, 2),
    }


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def golden_cases(z):
    """The fixture's cases: name -> (sim, {algorithm: alignment or None}).  A stored input is used as stored; a large one is regenerated and
    held against its stored SHA-256.  None: the reference raised on that case (window search, empty window)."""
    gen = generate_cases()
    out = {}
    for name in [str(s) for s in z["names"]]:
        if name + ".sim" in z:
            sim = z[name + ".sim"]
        else:
            sim = gen[name]
            assert np.array_equal(digest(sim), z[name + ".sim_sha256"]), f"{name}: the generated input is not the one the fixture was captured on"
        shape = tuple(int(v) for v in z[name + ".shape"])
        want = {}
        for alg in ALGORITHMS:
            key = f"{name}.{alg}"
            want[alg] = np.unpackbits(z[key])[:int(np.prod(shape))].reshape(shape).astype(np.float32) if key in z else None
        out[name] = (sim, want)
    return out
