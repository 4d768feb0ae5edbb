"""The comparisons of test_gpu_gemm_tiles.py can fail (CPU only): five corruptions a subtly wrong kernel would produce, applied to the correct
output of one exact GEMM case (293 x 192 x 192: a ragged last 256-row tile of 37 rows) and one exact convolution case (3 utterances of 513
tokens, dim 1024), in both stored types.

Each corruption is rejected by both assertions the GPU tests use -- bit equality with the rounded fp64 result, and the shared element-wise bound
(gpu_helpers.check_elementwise) -- while the whole-matrix rel-L2 of test_gpu_ops.py at its thresholds (3e-3 for the fused GEMM epilogues,
6e-3 for the tuned convolution) accepts the first and the third.  rel-L2 of each corrupted output against fp64 (bf16 / fp16 storage):

    1  one lane's four consecutive outputs short of one product            GEMM   1.01e-03 / 1.01e-03   accepted by the old 3e-3
    2  one 16-row fragment of the last ragged tile left unwritten (zeros)  GEMM   6.49e-02 / 6.49e-02
    3  one tap dropped on the first row of the second token tile           conv   4.83e-03 / 4.83e-03   accepted by the old 6e-3
    4  row 0 of utterance 1 computed with the tail of utterance 0          conv   1.73e-02 / 1.73e-02
    5  one K-step of 32 skipped for one 64-column tile                     GEMM   2.23e-01 / 2.23e-01

The correct outputs themselves sit at 0 (GEMM: small integers, exact in both types) and 1.55e-05 / 0 (conv): the rounding of the stored type.
The bound rejects the mildest corruption (1) at 32 times its size in bf16 and 251 times in fp16."""
import pytest
import torch

import gpu_helpers as G
from conftest import rel_l2

OLD_GEMM_THRESHOLD, OLD_CONV_THRESHOLD = 3e-3, 6e-3  # tests/test_gpu_ops.py: test_linear_fused_epilogues, test_conv_pos_embed_tuned_kernels
M, N, K = 256 + 37, 192, 192
B, L, DIM = 3, 513, 1024


@pytest.fixture(scope="module")
def gemm_case():
    (A, W, b), _ = G.exact_case("store", M, N, K, M, 1, False, seed=5)
    ref, scale = G.fused_ref("store", A, W, b)
    return A.double(), W.double(), ref, scale


@pytest.fixture(scope="module")
def conv_case():
    g = torch.Generator().manual_seed(6)
    x, w, b = G.ints(g, (B, L, DIM), -2, 2), G.ints(g, (DIM, DIM // 16, 31), -1, 1), G.ints(g, (DIM,), -8, 8)
    return x, w, b, G.conv31_ref(x, w, b), G.conv31_ref(x.abs(), w.abs(), b.abs())


def _lane(A, W, ref):
    """row 270 (the partial fragment's neighbour), columns 100 .. 103: the last product of the K sum is missing"""
    out = ref.clone()
    k = int(((A[270] != 0) & ((W[100:104] != 0).sum(dim=0) >= 3)).nonzero()[-1])  # (the last k whose products are not zero anyway)
    out[270, 100:104] -= A[270, k] * W[100:104, k]
    return out


def _fragment(A, W, ref):
    """rows 272 .. 287 of the ragged tile, columns 64 .. 79, never written"""
    out = ref.clone()
    out[272:288, 64:80] = 0.0
    return out


def _kstep(A, W, ref):
    """columns 64 .. 127 summed without k = 32 .. 63"""
    out = ref.clone()
    out[:, 64:128] -= A[:, 32:64] @ W[64:128, 32:64].t()
    return out


def _tap(x, w, b, ref):
    """token 128 of utterance 0 (first row of the second 128-token tile): tap 7 of every channel dropped"""
    out = ref.clone()
    cg = DIM // 16
    xin = x[0, 128 + 7 - 15].double().reshape(16, cg)  # the token tap 7 reads
    out[0, 128] -= torch.einsum("gi,goi->go", xin, w[:, :, 7].double().reshape(16, cg, cg)).reshape(DIM)
    return out


def _neighbour(x, w, b, ref):
    """token 0 of utterance 1: taps 0 .. 14 read the last 15 tokens of utterance 0 where Conv1d pads with zeros"""
    out = ref.clone()
    cg = DIM // 16
    for tap in range(15):
        xin = x[0, L - 15 + tap].double().reshape(16, cg)
        out[1, 0] += torch.einsum("gi,goi->go", xin, w[:, :, tap].double().reshape(16, cg, cg)).reshape(DIM)
    return out


def _rejected(name, out, ref, scale, precision):
    """both assertions of the GPU tests refuse `out`"""
    stored = G.round_to(precision, out)
    assert not torch.equal(stored, G.round_to(precision, ref)), name
    with pytest.raises(AssertionError, match="out of bound"):
        G.check_elementwise(name, stored, ref, scale, precision)
    return rel_l2(stored, ref)


@pytest.mark.parametrize("precision", [G.P_BF16, G.P_FP16], ids=["bf16", "fp16"])
def test_gemm_corruptions_are_rejected(gemm_case, precision):
    A, W, ref, scale = gemm_case
    good = G.round_to(precision, ref)
    G.check_elementwise("correct output", good, ref, scale, precision)
    print(f"  correct output: rel-L2 {rel_l2(good, ref):.2e}")
    errs = {}
    for name, fn in (("lane", _lane), ("fragment", _fragment), ("kstep", _kstep)):
        bad = fn(A, W, ref)
        assert int((bad != ref).sum()) >= (3 if name == "lane" else 200), name  # the corruption really changes the output
        errs[name] = _rejected(name, bad, ref, scale, precision)
        print(f"  {name}: rel-L2 {errs[name]:.2e}")
    assert errs["lane"] < OLD_GEMM_THRESHOLD, "the old whole-matrix comparison accepts one wrong lane"
    assert errs["kstep"] > OLD_GEMM_THRESHOLD  # (a whole skipped K-step is the size of error it can see)


@pytest.mark.parametrize("precision", [G.P_BF16, G.P_FP16], ids=["bf16", "fp16"])
def test_conv_corruptions_are_rejected(conv_case, precision):
    x, w, b, ref, scale = conv_case
    good = G.round_to(precision, ref)
    G.check_elementwise("correct output", good, ref, scale, precision)
    print(f"  correct output: rel-L2 {rel_l2(good, ref):.2e}")
    errs = {}
    for name, fn in (("tap", _tap), ("neighbour", _neighbour)):
        bad = fn(x, w, b, ref)
        assert int((bad != ref).sum()) >= 500, name
        errs[name] = _rejected(name, bad, ref, scale, precision)
        print(f"  {name}: rel-L2 {errs[name]:.2e}")
    assert errs["tap"] < OLD_CONV_THRESHOLD, "the old whole-matrix comparison accepts a dropped tap on a tile-boundary row"
