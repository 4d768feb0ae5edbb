"""Shared helpers of the GPU parity tests (everything goes through the C ABI of libf5hip.so)."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

from eraxvif5tts_amd import _lib
from eraxvif5tts_amd.model import CFM, DiT


def make_dit(arch, vocab, weights, precision, mel_dim=100):
    m = DiT(**arch, text_num_embeds=vocab, mel_dim=mel_dim, precision=precision)
    sd = m.state_dict()
    missing = [k for k in sd if k not in weights and k != "rotary_embed.inv_freq"]
    assert not missing, missing
    m.load_state_dict({k: v for k, v in weights.items() if k in sd}, strict=False)
    return m.cuda()


def make_cfm(arch, vocab, weights, precision, method="euler", mel_dim=100):
    m = make_dit(arch, vocab, weights, precision, mel_dim=mel_dim)
    return CFM(transformer=m, num_channels=mel_dim, mel_spec_kwargs={"mel_spec_type": "vocos"}, odeint_kwargs={"method": method}).cuda()


def op_linear(precision, kernel, A, W, bias=None, act="none"):
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[0]
    A = A.cuda().float().contiguous()
    W = W.cuda().float().contiguous()
    b = None if bias is None else bias.cuda().float().contiguous()
    out = torch.empty(M, N, device="cuda")
    _lib.check(lib.f5_op_linear(precision, kernel, M, N, K, _lib.ptr(A), _lib.ptr(W), _lib.ptr(b), _lib.ACT[act], _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu()


EPI_STORE_T, EPI_RESID, EPI_ROPE_T, EPI_GATE_T = 0, 2, 4, 5


def op_linear_fused(kernel, epi, A, W, bias, act="none", gate=None, rowmask=None, rope=None, rope_heads=0, seq=0, stream_in=None):
    """One DiT block linear with its fused epilogue (include/f5hip.h: f5_op_linear_fused).  epi 2 updates `stream_in` (the fp16 residual
    stream, given as f32) in place and returns it."""
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[0]
    dev = [None if t is None else t.cuda().float().contiguous() for t in (A, W, bias, gate, rope)]
    mk = None if rowmask is None else rowmask.cuda().to(torch.uint8).contiguous()
    out = torch.empty(M, N, device="cuda") if stream_in is None else stream_in.cuda().float().contiguous().clone()
    _lib.check(lib.f5_op_linear_fused(kernel, epi, M, N, K, _lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ACT[act],
                                      _lib.ptr(dev[3]), _lib.ptr(mk), _lib.ptr(dev[4]), rope_heads, seq, _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu()


def op_attention(precision, kernel, qkv, mask=None):
    lib = _lib.load()
    B, N, three, H, dh = qkv.shape
    assert three == 3 and dh == 64
    q = qkv.cuda().float().contiguous()
    mk = None if mask is None else mask.cuda().to(torch.uint8).contiguous()
    out = torch.empty(B, N, H * 64, device="cuda")
    _lib.check(lib.f5_op_attention(precision, kernel, B, N, H, _lib.ptr(q), _lib.ptr(mk), _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu()


def op_attention_ragged_rc(precision, attn_kernel, nbr, off, n, H, rows, qkv, out, ldq_extra=0, ldo_extra=0):
    """include/f5hip.h: f5_op_attention_ragged.  qkv [nbr * rows, 3 * H * 64 + ldq_extra], out [nbr * rows, H * 64 + ldo_extra] (pre-filled by
    the caller: what no launch writes comes back unchanged).  Returns (return code, out on the host)."""
    lib = _lib.load()
    cnt = len(n)
    assert len(off) == cnt and qkv.shape == (nbr * rows, 3 * H * 64 + ldq_extra) and out.shape == (nbr * rows, H * 64 + ldo_extra)
    q = qkv.cuda().float().contiguous()
    o = out.cuda().float().contiguous().clone()
    rc = lib.f5_op_attention_ragged(precision, attn_kernel, nbr, cnt, (C.c_int * cnt)(*off), (C.c_int * cnt)(*n), H, rows, ldq_extra, ldo_extra,
                                    _lib.ptr(q), _lib.ptr(o), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, o.cpu()


def op_attention_ragged(precision, attn_kernel, nbr, off, n, H, rows, qkv, out, ldq_extra=0, ldo_extra=0):
    rc, o = op_attention_ragged_rc(precision, attn_kernel, nbr, off, n, H, rows, qkv, out, ldq_extra, ldo_extra)
    _lib.check(rc, "f5_op_attention_ragged")
    return o


def op_conv_pos(precision, x, w0, b0, w1, b1):
    lib = _lib.load()
    B, N, D = x.shape
    xs = [t.cuda().float().contiguous() for t in (x, w0, b0, w1, b1)]
    out = torch.empty(B, N, D, device="cuda")
    _lib.check(lib.f5_op_conv_pos_embed(precision, B, N, D, *[_lib.ptr(t) for t in xs], _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu()


def op_ln_mod(x, scale, shift):
    lib = _lib.load()
    rows, dim = x.shape
    xs = [t.cuda().float().contiguous() for t in (x, scale, shift)]
    out = torch.empty(rows, dim, device="cuda")
    _lib.check(lib.f5_op_layernorm_modulate(rows, dim, *[_lib.ptr(t) for t in xs], _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def op_ln_fold(epi, x, A, Wo, bo, gate, W, bias, scale, shift, pivot=None, act="none", rope=None, rope_heads=0, seq=0):
    """include/f5hip.h: f5_op_ln_fold.  Returns (updated fp16 stream as f32 [M, D], stats [M, 2] = (mean, rstd), out [M, N])."""
    lib = _lib.load()
    M, D = x.shape
    N, Kb = W.shape[0], A.shape[1]
    dev = [None if t is None else t.cuda().float().contiguous() for t in (A, Wo, bo, gate, pivot, W, bias, scale, shift, rope)]
    xs = x.cuda().float().contiguous().clone()
    stats = torch.empty(M, 2, device="cuda")
    out = torch.empty(M, N, device="cuda")
    _lib.check(lib.f5_op_ln_fold(epi, M, D, N, Kb, _lib.ptr(xs), *[_lib.ptr(t) for t in dev[:9]], _lib.ACT[act], _lib.ptr(dev[9]), rope_heads, seq,
                                 _lib.ptr(stats), _lib.ptr(out), _lib.stream_ptr()))
    return xs.cpu(), stats.cpu(), out.cpu()


def op_linear_fused_p(precision, kernel, epi, A, W, bias, act="none", gate=None, rowmask=None, rope=None, rope_heads=0, seq=0, stream_in=None):
    """include/f5hip.h: f5_op_linear_fused_p -- op_linear_fused in the 16-bit mode `precision` (0 bf16, 2 fp16)."""
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[0]
    dev = [None if t is None else t.cuda().float().contiguous() for t in (A, W, bias, gate, rope)]
    mk = None if rowmask is None else rowmask.cuda().to(torch.uint8).contiguous()
    out = torch.empty(M, N, device="cuda") if stream_in is None else stream_in.cuda().float().contiguous().clone()
    _lib.check(lib.f5_op_linear_fused_p(precision, kernel, epi, M, N, K, _lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ACT[act],
                                        _lib.ptr(dev[3]), _lib.ptr(mk), _lib.ptr(dev[4]), rope_heads, seq, _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu()


def op_ln_fold_p(precision, epi, x, A, Wo, bo, gate, W, bias, scale, shift, pivot=None, act="none", rope=None, rope_heads=0, seq=0):
    """include/f5hip.h: f5_op_ln_fold_p.  Returns (updated fp16 stream as f32 [M, D], stats [M, 2] = (mean, rstd), out [M, N])."""
    lib = _lib.load()
    M, D = x.shape
    N, Kb = W.shape[0], A.shape[1]
    dev = [None if t is None else t.cuda().float().contiguous() for t in (A, Wo, bo, gate, pivot, W, bias, scale, shift, rope)]
    xs = x.cuda().float().contiguous().clone()
    stats = torch.empty(M, 2, device="cuda")
    out = torch.empty(M, N, device="cuda")
    _lib.check(lib.f5_op_ln_fold_p(precision, epi, M, D, N, Kb, _lib.ptr(xs), *[_lib.ptr(t) for t in dev[:9]], _lib.ACT[act], _lib.ptr(dev[9]), rope_heads,
                                   seq, _lib.ptr(stats), _lib.ptr(out), _lib.stream_ptr()))
    return xs.cpu(), stats.cpu(), out.cpu()


def op_conv31(precision, kernel, x, w, b, act="none"):
    """include/f5hip.h: f5_op_conv31 -- one grouped Conv1d(k = 31, groups = 16, padding 15) + bias (+ Mish): x [B, N, dim], w [dim, dim/16, 31]."""
    lib = _lib.load()
    B, N, D = x.shape
    xs = [t.cuda().float().contiguous() for t in (x, w, b)]
    out = torch.empty(B, N, D, device="cuda")
    _lib.check(lib.f5_op_conv31(precision, kernel, B, N, D, *[_lib.ptr(t) for t in xs], _lib.ACT[act], _lib.ptr(out), _lib.stream_ptr()), "f5_op_conv31")
    return out.cpu()


# f5_debug_last_gemm (include/f5hip.h): kernel families, schedules and flag bits of the launch record
FAM_TILE, FAM_FAST, FAM_W4, FAM_CONV31 = 0, 1, 2, 3
SCHED_PLAIN, SCHED_STAGGERED, SCHED_PERSISTENT = 0, 1, 2
FLAG_F16, FLAG_LNF, FLAG_F32, FLAG_CONV = 1, 2, 4, 8


def last_gemm():
    """(family, bm, bn, schedule, flags) of the last GEMM / conv31 launch of this process."""
    v = [C.c_int(0) for _ in range(5)]
    _lib.check(_lib.load().f5_debug_last_gemm(*[C.byref(t) for t in v]))
    return tuple(t.value for t in v)


# f5_debug_eval_modes (include/f5hip.h): the fields of csrc/model_internal.h's DitEvalModes, in its order
EVAL_MODE_FIELDS = ("rows", "rows_g", "defer", "r16", "rmw", "lnf", "qs", "wpf", "ink_qkv", "ink_ff1", "split_v", "frow0")


def eval_modes(plan, nb, N, per_batch_rows=False):
    """The launch forms one DiT evaluation of nb x N token rows takes in the plan's present state (nb counts the CFG-doubled batch), as a dict."""
    v = (C.c_int32 * len(EVAL_MODE_FIELDS))()
    _lib.check(_lib.load().f5_debug_eval_modes(plan, nb, N, int(bool(per_batch_rows)), v), "f5_debug_eval_modes")
    return dict(zip(EVAL_MODE_FIELDS, v))


# ----------------------------------------------------------------------------- element-wise comparison of the 16-bit GEMM / conv kernels
P_BF16, P_FP32, P_FP16 = 0, 1, 2
PREC_NAMES = {P_BF16: "bf16", P_FP32: "fp32", P_FP16: "fp16"}
F32_ULPS = 8 * 2.0 ** -23


def round_to(precision, t):
    """`t` rounded once (to nearest even) to the stored type of the mode `precision` (bf16 0, fp32 1, fp16 2), as f32."""
    if precision == P_FP32:
        return t.float()
    return (t.float().half() if precision == P_FP16 else t.float().to(torch.bfloat16)).float()


def stored_ulp(precision, ref):
    """Spacing of the stored type of the mode `precision` at |ref| (fp64)."""
    return fp32_ulp(ref) if precision == P_FP32 else fp16_ulp(ref) if precision == P_FP16 else bf16_ulp(ref)


def check_elementwise(name, out, ref, scale, precision=P_FP16, extra=None):
    """|out - ref| <= 1 ulp(ref) of the stored type (fp16 / bf16 / fp32) + 8 fp32 ulps of `scale` (+ extra), element-wise; prints the worst
    share of the bound before it asserts.  Pure tensor arithmetic: runs on the CPU."""
    ref = ref.double()
    err = (out.double() - ref).abs()
    ulp = stored_ulp(precision, ref)
    tname = PREC_NAMES[precision]
    bound = ulp + F32_ULPS * scale.double().abs()
    if extra is not None:
        bound = bound + extra.double()
    ratio = err / bound
    worst = float(ratio.max())
    print(f"  {name}: worst {worst:.3f} of the bound, {float((err / ulp).max()):.3f} {tname} ulp")
    assert torch.isfinite(out).all(), name
    bad = ratio > 1
    assert not bad.any(), f"{name}: {int(bad.sum())} elements out of bound (worst {worst:.3f} of it), first at {bad.nonzero()[0].tolist()}"
    return worst


# ----------------------------------------------------------------------------- attention: the fp64 reference with the terms of the element-wise
# bound, the CPU restatement of the bf16 kernels' arithmetic, and the adversarial inputs the bf16 tests share
LN2, LOG2E = 0.6931471805599453, 1.4426950408889634
QSCALE = 0.125 * LOG2E  # what a pre-scaled q carries: 1 / sqrt(64) * log2(e)


def attn_ref_terms(qkv, mask, precision, base2=False, keep=None, p=0.0):
    """fp64 softmax attention of qkv [B, N, 3, H, 64] over the keys `mask` [B, N] allows, and the terms of the element-wise bound
    (check_elementwise): (ref, mag, extra), each [B, N, H * 64] in fp64.
        ref    sum_k p_k v_k
        mag    pv (1 + 2 max_k sum_d |q_d k_d| scale), pv = sum_k p_k |v_k|: what the fp32 arithmetic works on -- the PV sum and, through the
               exponential, the score sum (an error ds of a score is a relative error ds of its numerator, once in the numerator, once in l)
        extra  one rounding (to nearest even) of each un-normalised numerator to the stored type:
               fp16  2^-11 pv + N 2^-25 max |v|   (half an ulp of 10 stored bits; numerators in the subnormal range, spacing 2^-24, against
                                                   l >= 1: the exponent reference is a score of the row)
               bf16  2^-8 pv                      (half an ulp of 7 stored bits; no subnormal term: bf16 has fp32's exponent range and the
                                                   kernels keep row sums below 2^64)
               fp32  0                            (the numerators stay in fp32: the reference kernel of the fp32 mode)
    base2: q is pre-scaled (QSCALE is in it): scores q . k ln 2, and the score magnitude sum_d |q_d k_d| as it stands.  keep [B, H, N, N] bool
    and p: the dropout mask and the factor 1 / (1 - p) on p_k, in ref and in pv."""
    B, N = qkv.shape[0], qkv.shape[1]
    outs = ([], [], [])
    for b in range(B):  # one batch item at a time: the [H, N, N] fp64 temporaries of a long sequence are large
        q, k, v = [qkv[b, :, i].transpose(0, 1).double() for i in range(3)]  # [H, N, 64]
        s = q @ k.transpose(-1, -2) * (LN2 if base2 else 0.125)
        sabs = q.abs() @ k.abs().transpose(-1, -2) * (1.0 if base2 else 0.125)
        if mask is not None:
            s = s.masked_fill(~mask[b][None, None, :], float("-inf"))
            sabs = sabs.masked_fill(~mask[b][None, None, :], 0.0)
        pr = torch.softmax(s, dim=-1)
        if keep is not None:
            pr = pr * keep[b].double() / (1.0 - p)
        o = pr @ v
        pv = pr @ v.abs()  # sum_k p_k |v_k| / l
        mag = pv * (1.0 + 2.0 * sabs.amax(dim=-1, keepdim=True))
        if precision == P_FP16:
            extra = 2.0 ** -11 * pv + N * 2.0 ** -25 * v.abs().amax(dim=(-1, -2), keepdim=True)
        elif precision == P_FP32:
            extra = torch.zeros_like(pv)
        else:
            extra = 2.0 ** -8 * pv
        for dst, t in zip(outs, (o, mag, extra.expand_as(o))):
            dst.append(t.transpose(0, 1).reshape(N, -1))
    return tuple(torch.stack(t) for t in outs)


def bf16_trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero), as f32"""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


EMULATE_VARIANTS = ("rne", "trunc_p", "trunc_out", "drop_last_valid_key", "leak_first_masked_key")


def attn_emulate_bf16(qkv, mask, variant="rne", base2=False):
    """CPU restatement of the bf16 flash kernels' arithmetic (attention_fast.hip, attention_pipe.hip): fp32 scores, numerators exp2(s c - m) in
    fp32 against a reference m (the row maximum here; softmax does not depend on it), the row sum from the UNROUNDED numerators, the numerators
    rounded once to bf16 (to nearest even) for the PV product, fp32 accumulation, one bf16 rounding of o / l.  -> [B, N, H * 64] f32.
    Variants other than `rne` are the defects the element-wise bound and the bias statistic must catch:
        trunc_p / trunc_out     the numerators / the outputs truncated to bf16 instead of rounded
        drop_last_valid_key     the last valid key of every batch item is left out
        leak_first_masked_key   the first masked key of a batch item counts; where its mask hides none, the ragged last tile's first padding
                                row does: it holds the last key again (the kernels re-read key N - 1 there); a whole last tile: nothing"""
    assert variant in EMULATE_VARIANTS
    B, N, _, H, _ = qkv.shape
    valid = torch.ones(B, N, dtype=torch.bool) if mask is None else mask.clone()
    twice = torch.zeros(B, dtype=torch.bool)  # the last key counted twice
    for b in range(B):
        if variant == "drop_last_valid_key":
            valid[b, int(valid[b].nonzero()[-1])] = False
        elif variant == "leak_first_masked_key":
            hidden = (~valid[b]).nonzero()
            if len(hidden):
                valid[b, int(hidden[0])] = True
            else:
                twice[b] = N % 64 != 0
    q, k, v = [qkv[:, :, i].transpose(1, 2).float() for i in range(3)]  # [B, H, N, 64]
    c = torch.tensor(1.0 if base2 else QSCALE, dtype=torch.float32)  # base2: q is pre-scaled, as f5_op_attention_prescaled takes it
    s = (q @ k.transpose(-1, -2)).masked_fill(~valid[:, None, None, :], float("-inf"))
    m = (s * c).amax(dim=-1, keepdim=True)
    num = torch.exp2(torch.addcmul(-m, s, c))
    dup = twice[:, None, None].float() * num[..., N - 1]  # [B, H, N]
    l = num.sum(dim=-1) + dup
    rnd = bf16_trunc if variant == "trunc_p" else bf16_round
    o = rnd(num) @ v + (rnd(dup)[..., None] * v[:, :, N - 1:N, :])
    o = o / l[..., None]
    o = bf16_trunc(o) if variant == "trunc_out" else bf16_round(o)
    return o.transpose(1, 2).reshape(B, N, H * 64)


def attn_randn_case(B, N, H, masked, seed=None, positive_v=False):
    """bf16(randn * 1.5) inputs [B, N, 3, H, 64] and the ragged-lengths key mask (N, N - 13, ...) of the attention tests; positive_v: V replaced
    by bf16(|V| + 0.5), so that every output is at least 0.5 and sum_k p_k |v_k| is the output itself (the rounding-bias statistic)."""
    g = torch.Generator().manual_seed(N + H if seed is None else seed)
    qkv = bf16_round(torch.randn(B, N, 3, H, 64, generator=g) * 1.5)
    if positive_v:
        qkv[:, :, 2] = bf16_round(qkv[:, :, 2].abs() + 0.5)
    mask = None
    if masked:
        lens = torch.tensor([N, max(1, N - 13)][:B])
        mask = torch.arange(N)[None, :] < lens[:, None]
    return qkv, mask


def mean_signed_error(out, ref, valid=None):
    """m = mean over the valid rows of (out - ref) / ref: the rounding-bias statistic (inputs of attn_randn_case(positive_v=True))"""
    out, ref = (out, ref) if valid is None else (out[valid], ref[valid])
    return float(((out.double() - ref.double()) / ref.double()).mean())


def attn_case_deferred_rescale():
    """Inputs of test_attention_deferred_rescale_thresholds (tests/test_gpu_ops.py): score jumps just below and far above the pipelined
    kernel's 2^16 threshold, early and late, and a row whose maximum creeps up tile by tile.  -> (qkv, planted query rows)"""
    g = torch.Generator().manual_seed(9)
    B, N, H = 1, 1024, 2
    qkv = torch.randn(B, N, 3, H, 64, generator=g) * 0.5
    qn = qkv[0, :, 0] / qkv[0, :, 0].norm(dim=-1, keepdim=True)      # unit queries
    for q, (key, nat) in {5: (700, 10.0), 37: (130, 12.5), 90: (1000, 40.0), 200: (3, 60.0)}.items():
        qkv[0, q, 0] = qn[q] * 8.0                                   # |q| = 8: q.k / 8 = |k| cos
        qkv[0, key, 1] = qn[q] * nat                                 # score of (q, key) = nat nats (16 log2 units = 11.1 nats)
    qkv[0, 300, 0] = qn[300] * 8.0
    for i, key in enumerate(range(10, 1024, 64)):                    # one key per tile, each 1.5 nats above the previous
        qkv[0, key, 1] = qn[300] * (1.5 * (i + 1))
    return bf16_round(qkv), (5, 37, 90, 200, 300)


def attn_case_range_guard(masked):
    """Inputs of test_attention_wide_kernel_range_guard (tests/test_gpu_ops.py): score jumps around the wide kernel's 2^64 guard, a creeping
    maximum and -- masked -- an utterance whose whole first tile is masked out.  -> (qkv, mask or None, planted query rows)"""
    g = torch.Generator().manual_seed(21)
    B, N, H = 2, 1024, 2
    qkv = torch.randn(B, N, 3, H, 64, generator=g) * 0.5
    jumps = {5: (700, 62.0 / LOG2E), 37: (130, 65.5 / LOG2E), 90: (1000, 144.0 / LOG2E), 200: (3, 430.0 / LOG2E), 411: (200, 90.0 / LOG2E),
             600: (90, 63.5 / LOG2E), 777: (960, 64.5 / LOG2E)}
    for bb in range(B):
        qn = qkv[bb, :, 0] / qkv[bb, :, 0].norm(dim=-1, keepdim=True)
        for q, (key, nat) in jumps.items():
            qkv[bb, q, 0] = qn[q] * 8.0          # |q| = 8: q.k / 8 = |k| cos
            qkv[bb, key, 1] = qn[q] * nat        # score of (q, key) = nat nats
        qkv[bb, 300, 0] = qn[300] * 8.0
        for i, key in enumerate(range(74, 1024, 64)):   # one key per tile, each 6 nats above the previous
            qkv[bb, key, 1] = qn[300] * (6.0 * (i + 1))
    qkv = bf16_round(qkv)
    mask = None
    if masked:
        mask = torch.ones(B, N, dtype=torch.bool)
        mask[1, :70] = False      # the first tile (and 6 keys of the second) of utterance 1
        mask[1, 1000:] = False
        mask[0, 990:] = False
    return qkv, mask, list(jumps) + [300]


def attn_case_spiked_512():
    """Inputs of test_attention_tuned_kernel_spiked_scores (tests/test_gpu_ops.py): one key dominates late in the sequence."""
    g = torch.Generator().manual_seed(5)
    B, N, H = 1, 512, 2
    qkv = bf16_round(torch.randn(B, N, 3, H, 64, generator=g))
    qkv[0, 400, 1] = qkv[0, 7, 0] * 8.0  # key 400 aligned with query 7
    return bf16_round(qkv)


def op_attention_prescaled(kernel, qkv, mask=None):
    """include/f5hip.h: f5_op_attention_prescaled (bf16; the q part of qkv carries QSCALE)"""
    lib = _lib.load()
    B, N, three, H, dh = qkv.shape
    assert three == 3 and dh == 64
    q = qkv.cuda().float().contiguous()
    mk = None if mask is None else mask.cuda().to(torch.uint8).contiguous()
    out = torch.empty(B, N, H * 64, device="cuda")
    _lib.check(lib.f5_op_attention_prescaled(kernel, B, N, H, _lib.ptr(q), _lib.ptr(mk), _lib.ptr(out), _lib.stream_ptr()), "f5_op_attention_prescaled")
    return out.cpu()


def linear_ref(A, W, b, act):
    """fp64 result and the magnitude the fp32 arithmetic works on (GELU's derivative is below 1.13: the accumulation error passes through it)."""
    ref = A.double() @ W.double().t() + b.double()
    scale = A.double().abs() @ W.double().abs().t() + b.double().abs()
    if act == "gelu_tanh":
        ref, scale = F.gelu(ref, approximate="tanh"), 1.13 * scale
    elif act == "gelu_erf":  # (the Vocos feed-forward; its derivative stays below 1.13 as well)
        ref, scale = F.gelu(ref), 1.13 * scale
    elif act == "mish":      # (derivative below 1.1)
        ref, scale = F.mish(ref), 1.1 * scale
    return ref, scale


def rope_ref(lin, ls, rope, seq, rope_heads=1):
    """x_transformers' rotation of adjacent feature pairs on the q | k columns of the first rope_heads heads of a fused QKV output [M, 3 * inner]
    (fp64) and of its magnitude; rope [seq, 32, 2] = (cos, sin), position = row % seq."""
    M, inner = lin.shape[0], lin.shape[1] // 3
    ref, scale = lin.clone(), ls.clone()
    cs = rope.double().reshape(seq, 32, 2)[torch.arange(M) % seq]
    cos, sin = cs[..., 0], cs[..., 1]
    for part in range(2):
        for h in range(rope_heads):
            c0 = part * inner + h * 64
            v, s = lin[:, c0:c0 + 64].reshape(M, 32, 2), ls[:, c0:c0 + 64].reshape(M, 32, 2)
            ref[:, c0:c0 + 64] = torch.stack([v[..., 0] * cos - v[..., 1] * sin, v[..., 1] * cos + v[..., 0] * sin], dim=-1).reshape(M, 64)
            scale[:, c0:c0 + 64] = torch.stack([s[..., 0] * cos.abs() + s[..., 1] * sin.abs(), s[..., 1] * cos.abs() + s[..., 0] * sin.abs()], dim=-1).reshape(M, 64)
    return ref, scale


def fused_ref(epi_name, A, W, b, act="none", gate=None, rowmask=None, x=None, rope=None, rope_heads=1, seq=0, addend=None, lin=None):
    """fp64 reference and fp32 magnitude of one fused epilogue (oracle/cpu_ref.py: dit_block's linears, apply_rope): store | gate | rope | resid
    | add2 (lin + addend, both outputs).  gate [N], or one row per token row [M, N] (a per-batch gate, expanded by the caller).  lin: (fp64
    result, magnitude) of the contraction where it is not A W^T + b (a convolution)."""
    lin, ls = linear_ref(A, W, b, act) if lin is None else lin
    keep = None if rowmask is None else rowmask.double()[:, None]
    if epi_name == "add2":
        return lin + addend.double(), ls + addend.double().abs()
    if epi_name == "resid":
        upd = gate.double() * lin if keep is None else gate.double() * lin * keep  # masked rows are left as they are
        return x.double() + upd, x.double().abs() + gate.double().abs() * ls
    if epi_name == "gate":
        return (gate.double() * lin if keep is None else gate.double() * lin * keep), gate.double().abs() * ls  # masked rows are zeros
    if epi_name == "store":
        return lin, ls
    return rope_ref(lin, ls, rope, seq, rope_heads)


def run_fused(precision, kernel, epi_name, A, W, b, act="none", gate=None, rowmask=None, x=None, rope=None, rope_heads=1, seq=0):
    if epi_name == "resid":
        return op_linear_fused_p(precision, kernel, EPI_RESID, A, W, b, "none", gate, rowmask, stream_in=x)
    if epi_name == "gate":
        return op_linear_fused_p(precision, kernel, EPI_GATE_T, A, W, b, act, gate, rowmask)
    if epi_name == "store":
        return op_linear_fused_p(precision, kernel, EPI_STORE_T, A, W, b, act)
    return op_linear_fused_p(precision, kernel, EPI_ROPE_T, A, W, b, "none", None, None, rope, rope_heads, seq)


def linear_problem(precision, M, N, K, seed):
    """randn operands rounded to the mode's 16-bit type on the host (so the kernel's own input conversion is exact), fp32 bias"""
    g = torch.Generator().manual_seed(seed)
    A, W, b = round_to(precision, torch.randn(M, K, generator=g)), round_to(precision, torch.randn(N, K, generator=g) / math.sqrt(K)), torch.randn(N, generator=g)
    return g, A, W, b


def fused_case(precision, epi_name, M, N, K, seq, seed):
    """Random real-valued inputs, the launch and the fp64 reference + fp32 magnitude of one fused epilogue in the 16-bit mode `precision`:
    resid (in place on the fp16 stream, gate), gate (+ row mask), store (GELU tanh), rope (one head)."""
    g, A, W, b = linear_problem(precision, M, N, K, seed)
    kw = {}
    if epi_name == "resid":
        kw = dict(gate=torch.randn(N, generator=g), x=(torch.randn(M, N, generator=g) * 3).half().float())
    elif epi_name == "gate":
        kw = dict(gate=torch.randn(N, generator=g), rowmask=torch.rand(M, generator=g) > 0.2)
    elif epi_name == "store":
        kw = dict(act="gelu_tanh")
    else:
        ang = torch.rand(seq, 32, generator=g) * 6.28
        kw = dict(rope=torch.stack([ang.cos(), ang.sin()], dim=-1), rope_heads=1, seq=seq)
    ref, scale = fused_ref(epi_name, A, W, b, **kw)
    run = lambda kernel=1: run_fused(precision, kernel, epi_name, A, W, b, **kw)
    return run, ref, scale


def ln_fold_inputs(M, D, N, Kb, epi, offset=40.0):
    """One LayerNorm-fold site at offset 40 (f5_op_ln_fold_p): the positional arguments (x, A, Wo, bo, gate, W, bias, scale, shift) and the keyword
    arguments (pivots; FF1 + GELU for epi 0, fused QKV + RoPE on one head with seq = M / 2 for epi 4).  A and Wo are exact in bf16 and in fp16."""
    g = torch.Generator().manual_seed(M + N + int(offset))
    both = lambda t: torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t.to(torch.bfloat16).float())  # exact in bf16 and in fp16
    x = torch.randn(M, D, generator=g) * 1.7 + offset + torch.randn(M, 1, generator=g) * 0.5
    A = both(torch.randn(M, Kb, generator=g))
    Wo = both(torch.randn(D, Kb, generator=g) / Kb ** 0.5)
    bo = torch.randn(D, generator=g) * 0.1
    gate = torch.randn(D, generator=g) * 0.3
    W = torch.randn(N, D, generator=g) / D ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    scale, shift = torch.randn(D, generator=g) * 0.2, torch.randn(D, generator=g) * 0.3
    seq = M // 2 if epi == 4 else M
    rope = None
    if epi == 4:
        ang = torch.arange(seq)[:, None] * (1.0 / 10000.0 ** (torch.arange(0, 64, 2) / 64.0))[None, :]
        rope = torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(seq, 64).float()
    xh = x.half().float()
    pivot = torch.stack([xh.mean(dim=1) + 0.01, torch.ones(M)], dim=1)
    kw = dict(pivot=pivot, act="gelu_tanh" if epi == 0 else "none", rope=rope, rope_heads=1, seq=seq)
    return (x, A, Wo, bo, gate, W, bias, scale, shift), kw


def ln_fold_ref(args, kw, epi, xs, stats):
    """fp64 reference and fp32 magnitude of the folded projection rstd (x . W'^T - mean c1) + c2 from the kernel's own stream `xs`, statistics
    and fold table (f5_op_fold_weights), through GELU (epi 0) or RoPE (epi 4)."""
    lib = _lib.load()
    _, _, _, _, _, W, bias, scale, shift = args
    N, D = W.shape
    M = xs.shape[0]
    dev = [t.cuda().float().contiguous() for t in (W, bias, scale, shift, scale, shift)]
    Wt, c1, c2 = torch.empty(N, D, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    _lib.check(lib.f5_op_fold_weights(N, N, 0, D, 0, *[_lib.ptr(t) for t in dev], _lib.ptr(Wt), _lib.ptr(c1), _lib.ptr(c2), _lib.stream_ptr()))
    torch.cuda.synchronize()
    Wt, c1, c2 = Wt.cpu().double(), c1.cpu().double(), c2.cpu().double()
    mean, rstd = stats[:, 0].double()[:, None], stats[:, 1].double()[:, None]
    ref = rstd * (xs.double() @ Wt.t() - mean * c1) + c2
    mag = rstd * (xs.double().abs() @ Wt.abs().t() + mean.abs() * Wt.abs().sum(dim=1)) + bias.double().abs() + W.double().abs() @ shift.double().abs()
    if epi == 0:
        return F.gelu(ref, approximate="tanh"), 1.13 * mag
    return rope_ref(ref, mag, kw["rope"], kw["seq"], 1)


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_case(epi, M, N, K, seq, rope_heads, masked, seed, gate_batches=0, a_rows=None):
    """Exact inputs of one epilogue (test_gpu_gemm_tiles.py: integers and halves whose every product, partial sum and epilogue value is exact
    in fp32): (positional A, W, b), keyword arguments of G.run_fused / G.fused_ref.  gate_batches > 0: one gate row per batch item
    [gate_batches, N]; a_rows: A holds that many rows (a_row_mod); epi "add2": an addend of multiples of 1/2 in +-64."""
    g = torch.Generator().manual_seed(seed)
    A, W, b = ints(g, (a_rows or M, K), -2, 2), ints(g, (N, K), -1, 1), ints(g, (N,), -8, 8)
    kw = {}
    if epi == "add2":
        kw["addend"] = ints(g, (M, N), -128, 128) * 0.5
    if epi in ("gate", "resid"):
        kw["gate"] = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[torch.randint(0, 6, (gate_batches, N) if gate_batches else (N,), generator=g)]
        if masked:
            kw["rowmask"] = torch.rand(M, generator=g) > 0.2
    if epi == "resid":
        kw["x"] = ints(g, (M, N), -128, 128) * 0.5
    if epi == "rope":
        table = torch.tensor([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [0.5, 0.5]])
        kw.update(rope=table[torch.randint(0, 5, (seq, 32), generator=g)], rope_heads=rope_heads, seq=seq)
    return (A, W, b), kw


def conv31_ref(x, w, b):
    """Grouped Conv1d(k = 31, groups = 16, padding 15) of x [B, L, dim] in fp64, zero padding inside each utterance; one matmul per group."""
    B, L, dim = x.shape
    cg = dim // 16
    xp = F.pad(x.double(), (0, 0, 15, 15))
    win = xp.unfold(1, 31, 1)  # [B, L, dim, 31]
    out = torch.empty(B, L, dim, dtype=torch.float64)
    for gi in range(16):
        a = win[:, :, gi * cg:(gi + 1) * cg, :].reshape(B * L, cg * 31)
        out[:, :, gi * cg:(gi + 1) * cg] = (a @ w[gi * cg:(gi + 1) * cg].double().reshape(cg, cg * 31).t()).reshape(B, L, cg)
    return out + b.double()


# ----------------------------------------------------------------------------- row-wise kernels (include/f5hip.h: test and diagnostic entry points)
def knob_get(key):
    """The value tuning knob `key` holds now (include/f5hip.h: f5_tuning_get)."""
    v = C.c_int()
    _lib.check(_lib.load().f5_tuning_get(key.encode(), C.byref(v)), f"f5_tuning_get({key})")
    return v.value


class knobs:
    """with knobs(ln_rows=4, ln_rows_min=1): ... -- tuning knobs set through f5_tuning_set.  On the way out, an exception included, each gets back
    the value that f5_tuning_get read before it was set, last set first: nested uses unwind, and a value F5HIP_TUNING put in force survives."""

    def __init__(self, **kv):
        self.kv = kv
        self.found = []

    def __enter__(self):
        lib = _lib.load()
        try:
            for k, v in self.kv.items():
                was = knob_get(k)
                _lib.check(lib.f5_tuning_set(k.encode(), int(v)), f"f5_tuning_set({k}, {v})")
                self.found.append((k, was))
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        lib = _lib.load()
        while self.found:
            k, was = self.found.pop()
            _lib.check(lib.f5_tuning_set(k.encode(), was))
        return False


def _pad_cols(t, ld, fill):
    """[rows, n] -> [rows, ld], the columns past n filled with `fill` (a kernel that reads them shows it)."""
    out = torch.full((t.shape[0], ld), fill, dtype=torch.float32)
    out[:, :t.shape[1]] = t
    return out


def op_layernorm_res(precision, x, y=None, y2=None, ymode=0, mul=None, add=None, mod_bstride=0, rows_per_batch=0, add_one=1, inplace=1,
                     xin_f16=1, xout_f16=1, ldx=None, ldy=None, ldo=None, sat_tag=0):
    """include/f5hip.h: f5_op_layernorm_res.  x [rows, dim] (the stream), y / y2 [rows, dim]; mul / add [dim] or [batches, mod_bstride].
    Returns (out [rows, dim], written-back stream [rows, dim], guard words: 6 Python ints).  Padding columns of x / y / y2 hold NaN; the
    helper asserts that the kernels leave the padding of `out` and of the stream buffer untouched."""
    lib = _lib.load()
    rows, dim = x.shape
    ldx, ldy, ldo = ldx or dim, ldy or dim, ldo or dim
    nan = float("nan")
    xs = _pad_cols(x.float(), ldx, nan).cuda()
    ys = None if y is None else _pad_cols(y.float(), ldy, nan).cuda()
    y2s = None if y2 is None else _pad_cols(y2.float(), ldy, nan).cuda()
    nb = -(-rows // (rows_per_batch or rows)) if mod_bstride else 1
    need = (nb - 1) * mod_bstride + dim
    m, a = [t.float().reshape(-1).contiguous().cuda() for t in (mul, add)]
    assert m.numel() >= need and a.numel() >= need
    out = torch.full((rows, ldo), 7.0, device="cuda")
    xback = torch.full((rows, ldx), 7.0, device="cuda")
    guard = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    rc = lib.f5_op_layernorm_res(precision, xin_f16, xout_f16, rows, dim, ldx, ldy, ldo, _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(y2s), ymode, _lib.ptr(m),
                                 _lib.ptr(a), mod_bstride, rows_per_batch, add_one, inplace, sat_tag, _lib.ptr(out), _lib.ptr(xback), _lib.ptr(guard),
                                 _lib.stream_ptr())
    _lib.check(rc, "f5_op_layernorm_res")
    out, xback = out.cpu(), xback.cpu()
    assert (out[:, dim:] == 0).all(), "a LayerNorm kernel wrote past dim"
    pad = xback[:, dim:]
    assert (pad.isnan().all() if inplace else (pad == 0).all()), "a LayerNorm kernel wrote the stream past dim"
    return out[:, :dim], xback[:, :dim], [int(v) & 0xffffffff for v in guard.cpu().tolist()]


def op_layernorm_res_rc(precision, xin_f16, xout_f16, rows, dim, ymode=0, inplace=1, ldx=None):
    """The return code of f5_op_layernorm_res for an argument set the launcher should refuse (no data checked)."""
    lib = _lib.load()
    ldx = ldx or dim
    x = torch.zeros(rows, ldx, device="cuda")
    y = torch.zeros(rows, ldx, device="cuda")
    md = torch.zeros(ldx, device="cuda")
    out = torch.zeros(rows, ldx, device="cuda")
    xb = torch.zeros(rows, ldx, device="cuda")
    return lib.f5_op_layernorm_res(precision, xin_f16, xout_f16, rows, dim, ldx, ldx, ldx, _lib.ptr(x), _lib.ptr(y), _lib.ptr(y), ymode, _lib.ptr(md),
                                   _lib.ptr(md), 0, 0, 1, inplace, 0, _lib.ptr(out), _lib.ptr(xb), None, _lib.stream_ptr())


def op_f32_to_f16(src):
    """include/f5hip.h: f5_op_f32_to_f16.  Returns (the fp16 values as f32, guard words)."""
    lib = _lib.load()
    s = src.float().contiguous().cuda()
    dst = torch.empty_like(s)
    guard = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.f5_op_f32_to_f16(s.numel(), _lib.ptr(s), _lib.ptr(dst), _lib.ptr(guard), _lib.stream_ptr()), "f5_op_f32_to_f16")
    return dst.cpu(), [int(v) & 0xffffffff for v in guard.cpu().tolist()]


def op_qknorm_rope(precision, qkv, heads, rope_heads, rows_per_batch, wq, wk, rope):
    lib = _lib.load()
    rows = qkv.shape[0]
    ts = [None if t is None else t.float().contiguous().cuda() for t in (qkv, wq, wk, rope)]
    out = torch.empty_like(ts[0])
    _lib.check(lib.f5_op_qknorm_rope(precision, rows, heads, rope_heads, rows_per_batch, *[_lib.ptr(t) for t in ts], _lib.ptr(out), _lib.stream_ptr()),
               "f5_op_qknorm_rope")
    return out.cpu()


def op_dwconv7_ln(precision, x, wt, cbias, ln_w, ln_b):
    lib = _lib.load()
    B, N, C = x.shape
    ts = [t.float().contiguous().cuda() for t in (x, wt, cbias, ln_w, ln_b)]
    out = torch.empty(B, N, C, device="cuda")
    _lib.check(lib.f5_op_dwconv7_ln(precision, B, N, C, *[_lib.ptr(t) for t in ts], _lib.ptr(out), _lib.stream_ptr()), "f5_op_dwconv7_ln")
    return out.cpu()


def op_grn(precision, h, gamma, beta):
    lib = _lib.load()
    B, N, C = h.shape
    ts = [t.float().contiguous().cuda() for t in (h, gamma, beta)]
    out = torch.empty(B, N, C, device="cuda")
    _lib.check(lib.f5_op_grn(precision, B, N, C, *[_lib.ptr(t) for t in ts], _lib.ptr(out), _lib.stream_ptr()), "f5_op_grn")
    return out.cpu()


def op_rmsnorm(precision, x, g):
    lib = _lib.load()
    rows, dim = x.shape
    ts = [t.float().contiguous().cuda() for t in (x, g)]
    out = torch.empty(rows, dim, device="cuda")
    _lib.check(lib.f5_op_rmsnorm(precision, rows, dim, *[_lib.ptr(t) for t in ts], _lib.ptr(out), _lib.stream_ptr()), "f5_op_rmsnorm")
    return out.cpu()


def plan_guard_words(model):
    """The fp16 range guard's record in the one plan `model` (a DiT) sampled with: residual_fallbacks and the five diagnostics
    f5_plan_get_option reports (residual_guard_amax_bits, _nan, _pass, _blocks, _row), as unsigned values."""
    lib = _lib.load()
    (_, h), = model._plans
    out = {}
    for k in ("residual_fallbacks", "residual_guard_amax_bits", "residual_guard_nan", "residual_guard_pass", "residual_guard_blocks", "residual_guard_row"):
        v = C.c_int(0)
        _lib.check(lib.f5_plan_get_option(h, k.encode(), C.byref(v)))
        out[k] = v.value & 0xffffffff
    return out


def bf16_ulp(ref):
    """Spacing of bf16 at |ref| (fp64): 2^(floor(log2 |ref|) - 7), at least that of the smallest normal."""
    _, e = torch.frexp(ref.abs().double())
    return torch.pow(2.0, (e - 8).clamp(min=-133).double())


def fp32_ulp(ref):
    """Spacing of fp32 at |ref| (fp64): 2^(floor(log2 |ref|) - 23), at least the subnormal spacing 2^-149."""
    _, e = torch.frexp(ref.abs().double())
    return torch.pow(2.0, (e - 24).clamp(min=-149).double())


def fp16_ulp(ref):
    """Spacing of fp16 at |ref| (fp64): 2^(floor(log2 |ref|) - 10), at least the subnormal spacing 2^-24."""
    _, e = torch.frexp(ref.abs().double())
    return torch.pow(2.0, (e - 11).clamp(min=-24).double())


def check_rounded(name, out, ref, scale, precision):
    """Element-wise bound of a kernel output against its fp64 reference.  `scale` [same shape]: the magnitude of the largest term the kernel
    evaluates in fp32 for that element; the slack is 8 fp32 ulps of it.  bf16 / fp16 outputs (precision 0 / 2): |out - ref| <= 1 ulp of ref in
    the stored type + slack per element; fp32 outputs: <= 1e-5 |ref| + slack.  Returns (worst error in the bound's units, (signed error sum in
    ulps of the stored type, count)) for the bias check: the sum runs over the elements whose slack is below 0.05 ulp."""
    ref = ref.double()
    err = out.double() - ref
    slack = 8 * 2.0 ** -23 * scale.double().abs()
    if precision in (0, 2):
        ulp = bf16_ulp(ref) if precision == 0 else fp16_ulp(ref)
        bound = ulp + slack
        keep = slack < 0.05 * ulp  # the rounding bias is read where fp32 evaluation error is negligible next to an ulp of the stored type
        signed = (err * torch.sign(ref) / ulp)[keep]
        sums = (float(signed.sum()), int(signed.numel()))
    else:
        bound = 1e-5 * ref.abs() + slack
        sums = (0.0, 0)
    ratio = (err.abs() / bound)
    worst = float(ratio.max())
    bad = ratio > 1
    if precision in (0, 2):  # (in ulps where the fp32 slack is negligible; the bound's share everywhere)
        in_ulp = float((err.abs() / ulp)[keep].max()) if keep.any() else float("nan")
        print(f"  {name}: worst {in_ulp:.3f} {'bf16' if precision == 0 else 'fp16'} ulp, {worst:.3f} of the bound")
    else:
        print(f"  {name}: worst {float((err.abs() / ref.abs().clamp(min=1e-30)).max()):.3e} relative, {worst:.3f} of the bound")
    assert not bad.any(), (f"{name}: {int(bad.sum())} elements out of bound, first at {bad.nonzero()[0].tolist()}: "
                           f"out {float(out.reshape(-1)[bad.reshape(-1).nonzero()[0]])} ref {float(ref.reshape(-1)[bad.reshape(-1).nonzero()[0]])}")
    return worst, sums


# ----------------------------------------------------------------------------- the reference tile kernel (f5_op_tile_gemm) and the CPU
# restatements of its arithmetic and of the reference attention kernel's (tests/test_tile_kernel_bound_host.py)
EPI_STORE_F32, EPI_ADD2 = 1, 3
TILE_EPI = {"store": EPI_STORE_T, "store_f32": EPI_STORE_F32, "resid": EPI_RESID, "add2": EPI_ADD2, "rope": EPI_ROPE_T, "gate": EPI_GATE_T}


def op_tile_gemm(precision, epi_name, A, W, b, act="none", gate=None, gate_bstride=0, rows_per_batch=0, rowmask=None, x=None, rope=None, rope_heads=0,
                 seq=0, addend=None, a_row_mod=0, f16_stream=False, pad=0, guard=2, conv=False):
    """include/f5hip.h: f5_op_tile_gemm -- gemm_tile_kernel in the mode `precision` with the epilogue `epi_name` (TILE_EPI).  Dense: A [M or
    a_row_mod, K], W [N, K], M = the rows of x / addend, else of A.  conv: A = x [B, L, dim], W [dim, dim / 16, 31].  The output buffers are
    [M + guard, N + pad] filled with NaN (the residual stream x in its [M, N] corner); the helper asserts that padding columns and guard rows
    come back as NaN.  f16_stream: the stream / addend and out_f hold fp16 (add2_f16).  seq is a synonym of rows_per_batch (RoPE).
    Returns (out_t [M, N] or None, out_f [M, N] or None)."""
    lib = _lib.load()
    epi = TILE_EPI[epi_name]
    if conv:
        Bc, L, N = A.shape
        M, K, rows_per_batch = Bc * L, 0, L
        A = A.reshape(M, N)
    else:
        N, K = W.shape
        M = x.shape[0] if x is not None else addend.shape[0] if addend is not None else A.shape[0]
        assert A.shape == ((a_row_mod or M), K)
    rpb = rows_per_batch or seq or M
    nb = -(-M // rpb)
    ld = N + pad
    nan = float("nan")
    dev = lambda t: None if t is None else t.float().contiguous().cuda()

    def buf(init):
        t = torch.full((M + guard, ld), nan)
        if init is not None:
            t[:M, :N] = init
        return t.cuda()

    needs_t, needs_f = epi_name in ("store", "rope", "gate", "add2"), epi_name in ("store_f32", "resid", "add2")
    ot, of = buf(None) if needs_t else None, buf(x) if needs_f else None
    keepalive = [dev(A), dev(W), dev(b), dev(gate), dev(rope), None if addend is None else _pad_cols(addend.float(), ld, nan).cuda(),
                 None if rowmask is None else rowmask.to(torch.uint8).contiguous().cuda()]
    if gate is not None:
        assert gate.numel() >= (nb - 1) * gate_bstride + N
    if rowmask is not None:
        assert rowmask.numel() == M
    if rope is not None:
        assert rope.numel() == rpb * 64
    a = _lib.TileGemm()
    for name, t in zip(("A", "W", "bias", "gate", "rope", "addend", "rowmask"), keepalive):
        setattr(a, name, None if t is None else t.data_ptr())
    a.out_t, a.out_f = (None if ot is None else ot.data_ptr()), (None if of is None else of.data_ptr())
    a.precision, a.mode, a.epi, a.M, a.N, a.K, a.a_row_mod, a.act = precision, int(conv), epi, M, N, K, a_row_mod, _lib.ACT[act]
    a.gate_bstride, a.rows_per_batch, a.rope_heads, a.ldadd, a.add2_f16 = gate_bstride, rpb, rope_heads, ld, int(f16_stream)
    a.ldo, a.ldof, a.out_rows = ld, ld, M + guard
    _lib.check(lib.f5_op_tile_gemm(C.byref(a), _lib.stream_ptr()), "f5_op_tile_gemm")
    torch.cuda.synchronize()
    res = []
    for name, t in (("out_t", ot), ("out_f", of)):
        if t is None:
            res.append(None)
            continue
        t = t.cpu()
        assert t[:, N:].isnan().all(), f"{name}: the tile kernel wrote a padding column (ld = N + {pad})"
        assert t[M:].isnan().all(), f"{name}: the tile kernel wrote a guard row"
        res.append(t[:M, :N].contiguous())
    return tuple(res)


def expect_tile_launch(what, precision, conv=False):
    """the launch record names the 64 x 64 tile family with the element type and conv flags of the case"""
    want = (FAM_TILE, 64, 64, SCHED_PLAIN, {P_BF16: 0, P_FP16: FLAG_F16, P_FP32: FLAG_F32}[precision] | (FLAG_CONV if conv else 0))
    rec = last_gemm()
    assert rec == want, f"{what}: launched (family, bm, bn, schedule, flags) = {rec}, intended {want}"


def expand_gate(gate, M, rows_per_batch):
    """a per-batch gate [nb, N] as one row per token row [M, N]"""
    return gate[torch.arange(M) // rows_per_batch]


def tile_stored(precision, epi_name, f16_stream, ref):
    """what the tile kernel stores of the fp64 result `ref`: (out_t, out_f), rounded once to the mode's type / to the stream's (fp32 or fp16)"""
    t = round_to(precision, ref) if epi_name in ("store", "rope", "gate", "add2") else None
    f = round_to(P_FP16 if f16_stream else P_FP32, ref) if epi_name in ("store_f32", "resid", "add2") else None
    return t, f


TILE_DEFECTS = ("none", "drop_last_k_chunk", "tail_column_neighbour_bias", "gate_of_previous_batch", "rope_pair_swapped", "a_row_mod_ignored")


def _act_f32(v, act):
    if act == "gelu_tanh":
        return F.gelu(v, approximate="tanh")
    if act == "gelu_erf":
        return F.gelu(v)
    if act == "mish":
        return F.mish(v)
    return v


def tile_emulate(precision, epi_name, A, W, b, act="none", gate=None, rows_per_batch=0, rowmask=None, x=None, rope=None, rope_heads=0, seq=0,
                 addend=None, a_row_mod=0, f16_stream=False, defect="none"):
    """CPU restatement of gemm_tile_kernel + gemm_epilogue4 in float32 (csrc/gemm.hip, csrc/gemm_epilogue.h): operands in the mode's type, one
    fp32 accumulator per output that takes the products k = 0, 1, ... as fused multiply-adds (v_mfma_f32_16x16x4_f32 is an fp32 FMA chain;
    the products of two 16-bit operands are exact in fp32), then bias, activation, gate / RoPE / addend in separate fp32 operations (the
    build has FMA contraction off), one rounding to the stored type.  gate [N] or [batches, N] (batch = m // rows_per_batch).
    -> (out_t, out_f) as tile_stored.  `defect` (TILE_DEFECTS) plants what the device test is there to catch:
        drop_last_k_chunk            the last 32-wide K chunk is left out
        tail_column_neighbour_bias   the last column of a partial 4-lane group (N % 4 != 0) takes the bias of the column before it
        gate_of_previous_batch       every row of a 64-row tile takes the gate of the batch item the tile's first row lies in
        rope_pair_swapped            the two (cos, sin) pairs of a 4-lane group change places
        a_row_mod_ignored            row m reads A[m]: past the a_row_mod rows of A, zeros"""
    assert defect in TILE_DEFECTS
    N, K = W.shape
    M = x.shape[0] if x is not None else addend.shape[0] if addend is not None else A.shape[0]
    A, W = round_to(precision, A), round_to(precision, W)
    if a_row_mod:
        if defect == "a_row_mod_ignored":
            A = torch.cat([A, torch.zeros(M - a_row_mod, K)])
        else:
            A = A[torch.arange(M) % a_row_mod]
    acc = torch.zeros(M, N, dtype=torch.float32)
    for k in range(K - 32 if defect == "drop_last_k_chunk" else K):
        acc = (acc.double() + A[:, k, None].double() * W[None, :, k].double()).float()  # one rounding: an FMA
    bias = b.float().clone()
    if defect == "tail_column_neighbour_bias" and N % 4 != 0 and N > 1:
        bias[N - 1] = bias[N - 2]
    v = acc + bias
    rpb = rows_per_batch or seq or M
    g = None
    if gate is not None:
        rows = torch.arange(M)
        batch = (rows // 64 * 64 if defect == "gate_of_previous_batch" else rows) // rpb
        g = gate.float()[batch] if gate.dim() == 2 else gate.float()[None, :]
    keep = torch.ones(M, dtype=torch.bool) if rowmask is None else rowmask.bool()
    if epi_name in ("store", "store_f32"):
        res = _act_f32(v, act)
    elif epi_name == "gate":
        res = _act_f32(v, act)
        res = torch.where(keep[:, None], res if g is None else res * g, torch.zeros_like(res))
    elif epi_name == "resid":
        t = _act_f32(v, act)
        t = t if g is None else t * g
        cur = round_to(P_FP16 if f16_stream else P_FP32, x)
        res = torch.where(keep[:, None], cur + t, cur)
    elif epi_name == "add2":
        res = v + round_to(P_FP16 if f16_stream else P_FP32, addend)
    else:
        inner = N // 3
        cs = rope.float().reshape(rpb, 32, 2)[torch.arange(M) % rpb]
        if defect == "rope_pair_swapped":
            cs = cs.reshape(M, 16, 2, 2).flip(2).reshape(M, 32, 2)
        cos, sin = cs[..., 0], cs[..., 1]
        res = v.clone()
        for part in range(2):
            for h in range(rope_heads):
                c0 = part * inner + h * 64
                p = v[:, c0:c0 + 64].reshape(M, 32, 2)
                res[:, c0:c0 + 64] = torch.stack([p[..., 0] * cos - p[..., 1] * sin, p[..., 1] * cos + p[..., 0] * sin], dim=-1).reshape(M, 64)
    return tile_stored(precision, epi_name, f16_stream, res)


def attn_emulate_ref(qkv, mask, precision, base2=False, leak_padding_key=False):
    """CPU restatement of attn_ref_kernel (csrc/attention.hip) in float32: 64-key tiles, fp32 scores times the scale, the running maximum and
    row sum rescaled by expf(m_old - m_new), numerators expf(s - m_new) kept in fp32, fp32 PV sums, o * (1 / l) rounded once to the stored type.
    leak_padding_key: the defect the device test is there to catch -- the first padding row of the ragged last tile (zeros: the kernel
    zero-fills it) counts as a key: score 0, value 0.  -> [B, N, H * 64] f32."""
    B, N, _, H, _ = qkv.shape
    valid = torch.ones(B, N, dtype=torch.bool) if mask is None else mask
    x = round_to(precision, qkv)
    q, k, v = [x[:, :, i].transpose(1, 2).float() for i in range(3)]  # [B, H, N, 64]
    scale = torch.tensor(LN2 if base2 else 0.125, dtype=torch.float32)
    m_i = torch.full((B, H, N), float("-inf"))
    l_i, o = torch.zeros(B, H, N), torch.zeros(B, H, N, 64)
    for k0 in range(0, N, 64):
        k1 = min(N, k0 + 64)
        s = (q @ k[:, :, k0:k1].transpose(-1, -2)) * scale
        ok = valid[:, None, None, k0:k1].expand_as(s)
        vt = v[:, :, k0:k1]
        if leak_padding_key and k1 == N and N % 64 != 0:
            s = torch.cat([s, torch.zeros(B, H, N, 1)], dim=-1)
            ok = torch.cat([ok, torch.ones(B, H, N, 1, dtype=torch.bool)], dim=-1)
            vt = torch.cat([vt, torch.zeros(B, H, 1, 64)], dim=2)
        s = s.masked_fill(~ok, float("-inf"))
        m_new = torch.maximum(m_i, s.amax(dim=-1))
        alpha = torch.where(m_i == float("-inf"), torch.zeros_like(m_i), torch.exp(m_i - m_new))
        p = torch.where(s == float("-inf"), torch.zeros_like(s), torch.exp(s - m_new[..., None]))
        l_i = l_i * alpha + p.sum(dim=-1)
        o = o * alpha[..., None] + p @ vt
        m_i = m_new
    inv = torch.where(l_i > 0, 1.0 / l_i, torch.zeros_like(l_i))
    return round_to(precision, (o * inv[..., None]).transpose(1, 2).reshape(B, N, H * 64))


# ----------------------------------------------------------------------------- the text path (compute_text_embed, csrc/eval_common.hip): fp64
# reference, the CPU restatement of the kernel chain with its planted defects, and the per-row bound (tests/test_text_embed_bound_host.py,
# tests/test_gpu_text_embed.py)
TEXT_MARGIN = 4.0  # a result passes when its worst row error is within TEXT_MARGIN x the restatement's worst row error of the same case
TEXT_DEFECTS = ("none", "last_token_gathers_filler", "position_off_by_one", "mask_after_drop_text", "conv_across_batch", "grn_over_flattened_batch",
                "no_mask_after_last_block", "position_wraps")


def text_clamp_ids(text, vocab):
    """What text_gather_kernel makes of an id outside [-1, vocab): the nearer end of that range (-1 is the filler)."""
    return text.clamp(min=-1, max=vocab - 1)


def text_pos_table_f32(td, rows):
    """The position table as f5_model_finalize fills it (csrc/model.hip), in float32 on the host: inv_j = 1 / powf(10000, 2j / td) with the C
    library's powf (through ctypes, numpy's power where no libm is found), ang = p * inv_j, [cos | sin] -> [rows, td]."""
    import ctypes.util

    import numpy as np
    half = td // 2
    expo = (np.arange(half, dtype=np.float32) * np.float32(2)) / np.float32(td)
    name = ctypes.util.find_library("m")
    if name:
        powf = C.CDLL(name).powf
        powf.restype, powf.argtypes = C.c_float, [C.c_float, C.c_float]
        pw = np.array([powf(10000.0, float(e)) for e in expo], dtype=np.float32)
    else:
        pw = np.power(np.float32(10000), expo)
    inv = (np.float32(1) / pw).astype(np.float32)
    ang = (np.arange(rows, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return torch.from_numpy(np.concatenate([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32))


def text_reference(W, cfg, text, N, drop_text, mmdit=False):
    """R: oracle/cpu_ref's text embedding evaluated in float64 on the weights cast to double -> [B, N, td] (MMDiT: [B, nt, dim])."""
    from oracle import cpu_ref
    Wd = {k: v.double() for k, v in W.items() if k.startswith("text_embed.")}
    if mmdit:
        return cpu_ref.mmdit_text_embedding(Wd, cfg, text, drop_text=drop_text)
    return cpu_ref.text_embedding(Wd, cfg, text, N, drop_text=drop_text)


def text_emulate(precision, W, cfg, text, N, drop_text, mmdit=False, defect="none"):
    """CPU restatement of compute_text_embed in float32: text_gather_kernel (ids clamped into the table, filler flags before drop_text, the
    position index clamped at the table's last row), mask_rows_kernel, then per ConvNeXt-V2 block dwconv7_ln -> the mode's type, pwconv1 + GELU
    (weights and output in the mode's type), GRN in place in the mode's type, pwconv2 (weights in the mode's type) added to the fp32 output, and
    the mask again.  `defect` (TEXT_DEFECTS) plants what tests/test_gpu_text_embed.py is there to catch:
        last_token_gathers_filler    the last real token row of every batch item reads table row 0
        position_off_by_one          row p takes position p + 1
        mask_after_drop_text         the filler flags are taken from the ids drop_text has zeroed
        conv_across_batch            the depthwise conv's taps run over the flattened B * N rows (zero padding only at the two ends)
        grn_over_flattened_batch     GRN's sequence norm runs over all B * N rows
        no_mask_after_last_block     the filler rows are not zeroed again after the last block
        position_wraps               positions past the table wrap around instead of clamping to its last row"""
    assert defect in TEXT_DEFECTS
    table = W["text_embed.text_embed.weight"].float()
    B, nt = text.shape
    N = nt if mmdit else N
    n = min(nt, N)
    ids = torch.zeros(B, N, dtype=torch.long)
    ids[:, :n] = text_clamp_ids(text[:, :n].long(), table.shape[0] - 1) + 1
    filler = ids == 0
    if defect == "last_token_gathers_filler":
        for b in range(B):
            real = (~filler[b]).nonzero()
            if real.numel():
                ids[b, int(real[-1])] = 0
    if drop_text:
        ids = torch.zeros_like(ids)
        if defect == "mask_after_drop_text":
            filler = ids == 0
    x = table[ids]
    n_conv = 0 if mmdit else cfg.get("conv_layers", 0)
    mp = bool(cfg.get("text_mask_padding", True))
    if not (mmdit or n_conv > 0):
        return x
    pos_rows = 1024 if mmdit else 4096
    p = torch.arange(N) + (1 if defect == "position_off_by_one" else 0)
    p = p % pos_rows if defect == "position_wraps" else p.clamp(max=pos_rows - 1)
    x = x + text_pos_table_f32(x.shape[-1], min(pos_rows, N + 1))[p][None]
    if mp:
        x = x.masked_fill(filler[..., None], 0.0)
    td = x.shape[-1]
    for i in range(n_conv):
        pre = f"text_embed.text_blocks.{i}."
        w = {k: W[pre + k].float() for k in ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias", "grn.gamma",
                                            "grn.beta", "pwconv2.weight", "pwconv2.bias")}
        xin = x.reshape(1, B * N, td) if defect == "conv_across_batch" else x
        y = F.conv1d(xin.transpose(1, 2), w["dwconv.weight"], w["dwconv.bias"], padding=3, groups=td).transpose(1, 2).reshape(B, N, td)
        mean = y.mean(dim=-1, keepdim=True)
        d = y - mean
        y = round_to(precision, d * torch.rsqrt((d * d).mean(dim=-1, keepdim=True) + 1e-6) * w["norm.weight"] + w["norm.bias"])
        h = round_to(precision, F.gelu(y @ round_to(precision, w["pwconv1.weight"]).t() + w["pwconv1.bias"]))
        hs = h.reshape(1, B * N, 2 * td) if defect == "grn_over_flattened_batch" else h
        g = torch.sqrt((hs * hs).sum(dim=1, keepdim=True))
        nx = g / (g.mean(dim=-1, keepdim=True) + 1e-6)
        h = round_to(precision, w["grn.gamma"].reshape(-1) * (h * nx) + w["grn.beta"].reshape(-1) + h)
        x = x + (h @ round_to(precision, w["pwconv2.weight"]).t() + w["pwconv2.bias"])
        if mp and not (defect == "no_mask_after_last_block" and i == n_conv - 1):
            x = x.masked_fill(filler[..., None], 0.0)
    return x


def text_row_errors(X, R):
    """The row metric: e[b, p] = max_c |X - R| / max_c |R[b, p, :]| over the rows whose reference is not all zero (0 elsewhere), and the mask of
    the rows the reference zeroes (the filler rows under text_mask_padding)."""
    R = R.double()
    top = R.abs().amax(dim=-1)
    zero = top == 0
    e = (X.double() - R).abs().amax(dim=-1) / top.clamp(min=1e-300)
    return torch.where(zero, torch.zeros_like(e), e), zero


def check_text_rows(name, X, R, E, margin=TEXT_MARGIN):
    """Every row of X within margin x the restatement E's worst row error against R, and exact zeros on the rows R zeroes.  Prints the
    restatement's worst row error, the margin and X's worst row as a share of the bound; returns that share."""
    eE, _ = text_row_errors(E, R)
    eX, zero = text_row_errors(X, R)
    bound = margin * float(eE.max())
    assert torch.isfinite(X).all(), name
    nz = int((X[zero] != 0).sum())
    worst = float(eX.max())
    share = worst / bound if bound > 0 else (0.0 if worst == 0 else float("inf"))
    print(f"  {name}: restatement's worst row {float(eE.max()):.3e}, margin {margin:g}, worst row {worst:.3e} = {share:.3f} of the bound "
          f"(row {tuple(int(i) for i in (eX == eX.max()).nonzero()[0])}); rel-L2 {float((X.double() - R.double()).norm() / R.double().norm().clamp(min=1e-300)):.3e}; "
          f"{int(zero.sum())} zeroed rows")
    assert nz == 0, f"{name}: {nz} non-zero elements on rows the reference zeroes"
    bad = eX > bound
    assert not bad.any(), f"{name}: {int(bad.sum())} rows out of bound (worst {share:.3f} of it), first at {bad.nonzero()[0].tolist()}"
    return share


TEXT_V = 200  # vocabulary of the text cases: ids 0 .. 199, table of 201 rows
# id -> (backbone, text_dim, conv_layers, text_mask_padding, B, N, nt, real tokens per batch item)
TEXT_CASES = {
    "td512_c4_mask_3x77": ("dit", 512, 4, True, 3, 77, 90, (77, 40, 90)),    # no filler / -1 padded / nt = 90 > N: curtailed at N
    "td512_c4_nomask_3x77": ("dit", 512, 4, False, 3, 77, 90, (77, 40, 90)),
    "td512_c4_mask_2x5": ("dit", 512, 4, True, 2, 5, 5, (5, 3)),             # a sequence shorter than the 7-tap conv
    "td512_c4_mask_2x300": ("dit", 512, 4, True, 2, 300, 200, (200, 0)),     # 600 rows: whole and ragged GEMM tiles; one item all filler
    "td128_c2_nomask_3x77": ("dit", 128, 2, False, 3, 77, 90, (77, 40, 90)),  # the tiny goldens' width
    "td100_c0_2x77": ("unett", 100, 0, True, 2, 77, 77, (77, 40)),           # E2-TTS / UNetT form: the gather alone, no position table
    "mmdit128_mask_nt1030": ("mmdit", 128, 0, True, 2, 1030, 1030, (1030, 1000)),  # positions 1024 .. 1029 clamp to row 1023 of the table
    "mmdit128_nomask_nt1030": ("mmdit", 128, 0, False, 2, 1030, 1030, (1030, 1000)),
}
_TEXT_CASE_CACHE = {}


def text_case(cid):
    """One line of TEXT_CASES as a dict: arch (the smallest model create() accepts: dim 128), seeded weights W, text and a second text with
    the same filler pattern [B, nt] (-1 padded), B, N, backbone, mmdit.  Built once and shared; nothing writes to it."""
    if cid in _TEXT_CASE_CACHE:
        return _TEXT_CASE_CACHE[cid]
    from oracle import cpu_ref
    backbone, td, conv, mp, B, N, nt, real = TEXT_CASES[cid]
    seed = 7000 + sorted(TEXT_CASES).index(cid)
    if backbone == "mmdit":
        arch = dict(dim=128, depth=1, heads=2, ff_mult=2, text_mask_padding=mp)
        W = cpu_ref.random_mmdit_weights(arch, TEXT_V, seed=seed)
    elif backbone == "unett":
        arch = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=td, conv_layers=conv, text_mask_padding=mp, pe_attn_head=1, skip_connect_type="concat")
        W = cpu_ref.random_unett_weights(arch, TEXT_V, seed=seed)
    else:
        arch = dict(dim=128, depth=1, heads=2, ff_mult=2, text_dim=td, conv_layers=conv, text_mask_padding=mp, pe_attn_head=1)
        W = cpu_ref.random_dit_weights(arch, TEXT_V, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    texts = []
    for _ in range(2):
        t = torch.randint(0, TEXT_V, (B, nt), generator=g)
        for b, n in enumerate(real):
            t[b, n:] = -1
        texts.append(t)
    texts[0][0, 0], texts[0][0, min(real[0], nt) - 1] = TEXT_V - 1, 0  # the two ends of the table are gathered
    case = dict(arch=arch, W=W, text=texts[0], text2=texts[1], B=B, N=N, backbone=backbone, mmdit=backbone == "mmdit")
    _TEXT_CASE_CACHE[cid] = case
    return case


_TEXT_REF_CACHE = {}


def text_case_terms(cid, precision, drop_text):
    """(R, E_p) of a case: the fp64 reference and the restatement in the mode `precision`; computed once per key, shared, never written to."""
    key = (cid, drop_text)
    c = text_case(cid)
    if key not in _TEXT_REF_CACHE:
        _TEXT_REF_CACHE[key] = text_reference(c["W"], c["arch"], c["text"], c["N"], drop_text, c["mmdit"])
    ekey = (cid, precision, drop_text)
    if ekey not in _TEXT_REF_CACHE:
        _TEXT_REF_CACHE[ekey] = text_emulate(precision, c["W"], c["arch"], c["text"], c["N"], drop_text, c["mmdit"])
    return _TEXT_REF_CACHE[key], _TEXT_REF_CACHE[ekey]


# ----------------------------------------------------------------------------- plan read-backs and the input sets of the graph-replay tests
def plan_option(model, key):
    """f5_plan_get_option(key) of the ONE plan `model` (a DiT / UNetT / MMDiT) holds."""
    (_, h), = model._plans
    v = C.c_int(-1)
    _lib.check(_lib.load().f5_plan_get_option(h, key.encode(), C.byref(v)), f"f5_plan_get_option({key})")
    return v.value


REPLAY_FIELDS = ("cond", "text_ids", "text_len", "lens", "durations", "y0", "cond_mask")


def replay_inputs(B, N, nt, mel, V, seed):
    """Two input sets (A, B) of one native_sample() shape -- dicts over REPLAY_FIELDS, host tensors -- in which every value differs:
        cond, y0     f32 [B, N, mel]  other seeds (cond = randn * 2 - 3, as a log-mel prompt; y0 = randn)
        text_ids     int [B, nt]      B's id at every position is another id than A's
        text_len     int [B]          valid tokens per row, all in [nt - 9, nt]: both texts have nt columns (replay_text pads with -1)
        lens         int [B]          prompt frames, around N / 3
        durations    int [B]          A = (N, N - 43, ...), B = (..., N - 89, N): max = N in both (the same key), every row differs, row 0
                                      shrinks and the last row grows from A to B
        cond_mask    bool [B, N]      lens prefix with 1 frame in 5 edited out (f5_sample_masked), drawn per set
    Needs B >= 2 (one row cannot change its duration under a fixed N), nt >= 12 and N >= 100 (durations stay above text and prompt)."""
    assert B >= 2 and nt >= 12 and N >= 100 and V >= 3
    ga, gb = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed + 7919)
    rows = torch.arange(B)
    ids_a = torch.randint(0, V, (B, nt), generator=ga)
    sets = []
    for which, g in enumerate((ga, gb)):
        d = dict(cond=torch.randn(B, N, mel, generator=g) * 2 - 3, y0=torch.randn(B, N, mel, generator=g))
        d["text_ids"] = ids_a if which == 0 else (ids_a + 1 + torch.randint(0, V - 1, (B, nt), generator=g)) % V
        d["text_len"] = nt - (rows * 7) % 5 if which == 0 else nt - 5 - (rows * 3) % 5
        d["lens"] = N // 3 - 23 * rows % (N // 4) if which == 0 else N // 3 - 11 + (9 * rows) % 20
        dur = N - 43 * rows - 13 * (rows > 1) if which == 0 else N - 82 - 7 * (B - 1 - rows)
        dur[0 if which == 0 else B - 1] = N
        d["durations"] = dur.clamp(min=N // 2 + 1)
        d["cond_mask"] = (torch.arange(N)[None, :] < d["lens"][:, None]) & (torch.rand(B, N, generator=g) > 0.2)
        assert int(d["durations"].max()) == N and bool((d["durations"] > torch.maximum(d["text_len"], d["lens"])).all())
        sets.append(d)
    a, b = sets
    for k in REPLAY_FIELDS:
        differs = a[k] != b[k]
        assert bool(differs.any(dim=1).all() if k == "cond_mask" else differs.all()), k
    return a, b


def replay_swap(a, b, field):
    """`a` with exactly the one field of REPLAY_FIELDS taken from `b` (a new dict; the tensors are shared and never written to)."""
    assert field in REPLAY_FIELDS
    return {**a, field: b[field]}


def replay_text(d):
    """The text tensor [B, nt] of an input set: text_ids with the columns from text_len on set to the pad -1."""
    return torch.where(torch.arange(d["text_ids"].shape[1])[None, :] < d["text_len"][:, None], d["text_ids"], torch.full_like(d["text_ids"], -1))


# ----------------------------------------------------------------------------- the production-mode DiT evaluation, stage by stage (stage probes,
# include/f5hip.h: f5_plan_set_probe): per stage the fp64 restatement of THAT stage from the probe of the stage before it, the CPU restatement
# with the kernel's roundings (stage_emulate) and its planted defects, and the per-row bound (tests/test_production_stage_bound_host.py,
# tests/test_gpu_production_stages.py)
STAGE_MARGIN = 3.0  # a row passes when its error is within STAGE_MARGIN x the restatement's worst row error of the same stage and case
STAGE_EPS = 1e-6    # LayerNorm eps (modules.py:308,624)
STAGE_DEFECTS = ("none", "stats_quarter_row", "stats_of_previous_site", "v_c1_c2_shifted_by_inner", "fold_rows_of_another_time", "q_not_scaled",
                 "q_scaled_twice", "gate_mlp_for_gate_msa", "blk0_unscaled_weight_copy", "final_pair_swapped", "rope_position_is_row_index")


def site_gemm(site):
    """include/f5hip.h: f5_debug_site_gemm -- ((family, bm, bn, schedule, flags) of the last launch of block call site 1 QKV / 2 out-projection /
    3 FF1 / 4 FF2, launches of that site in this process so far)."""
    v = [C.c_int(0) for _ in range(6)]
    _lib.check(_lib.load().f5_debug_site_gemm(site, *[C.byref(t) for t in v]), "f5_debug_site_gemm")
    return tuple(t.value for t in v[:5]), v[5].value


def stage_layout(nb, N, durations=None, frames=None):
    """The rows of one evaluation: nb batch items of N rows.  durations [nb] (a key mask: item b's first durations[b] rows are keys and valid
    queries) or frames (a ragged call: N = T, nb = 2 halves, utterance u at rows [off[u], off[u] + frames[u]) of each half, the rest gaps) or
    neither.  -> dict: rows, N, seg [rows] (attention sequence of the row, -1 = gap), seg_rows {id: (first row, rows)}, key [rows] bool (the row
    is a key of its sequence and a valid query), pos [rows] (RoPE position)."""
    rows = nb * N
    seg = torch.full((rows,), -1, dtype=torch.long)
    key = torch.zeros(rows, dtype=torch.bool)
    pos = torch.zeros(rows, dtype=torch.long)
    seg_rows = {}
    if frames is None:
        for b in range(nb):
            seg_rows[b] = (b * N, N)
            seg[b * N:(b + 1) * N] = b
            key[b * N:b * N + (N if durations is None else int(durations[b]))] = True
            pos[b * N:(b + 1) * N] = torch.arange(N)
    else:
        off, T = [], 0
        for n in frames:
            off.append(T)
            T = -(-(T + n + 16) // 16) * 16
        assert T == N and nb == 2, (T, N, nb)
        for br in range(2):
            for u, n in enumerate(frames):
                r0 = br * T + off[u]
                seg_rows[br * len(frames) + u] = (r0, n)
                seg[r0:r0 + n] = br * len(frames) + u
                key[r0:r0 + n] = True
                pos[r0:r0 + n] = torch.arange(n)
    return dict(rows=rows, N=N, seg=seg, seg_rows=seg_rows, key=key, pos=pos)


def stage_sample_rows(lay, seed=0, rows_real=None):
    """The rows a stage is compared on: the first and last row of every 128-row tile (which holds those of every 256-row tile), the last real row
    (rows_real: the evaluation's token rows when the buffers hold more), the rows on both sides of every boundary between attention sequences,
    and 64 seeded rows.  -> (valid rows: keys / queries of their sequence, padded rows: inside a sequence, behind its key mask), both sorted."""
    rows = rows_real or lay["rows"]
    pick = set(range(0, rows, 128)) | set(min(r + 127, rows - 1) for r in range(0, rows, 128)) | {rows - 1}
    for r0, n in lay["seg_rows"].values():
        pick |= {r0, r0 + n - 1, max(r0 - 1, 0), min(r0 + n, rows - 1)}
        nk = int(lay["key"][r0:r0 + n].sum())
        pick |= {r0 + nk - 1, min(r0 + nk, rows - 1)}
    g = torch.Generator().manual_seed(1000 + seed)
    pick |= set(torch.randint(0, rows, (64,), generator=g).tolist())
    idx = torch.tensor(sorted(pick))
    return idx[lay["key"][idx]], idx[(~lay["key"][idx]) & (lay["seg"][idx] >= 0)]


def stage_weights(W, depth, mel=100):
    """The fp32 weights the stages use, from a DiT state dict: per block qkv_w [3 inner, D] (to_q | to_k | to_v), qkv_b, o_w, o_b, f1_w, f1_b,
    f2_w, f2_b; out_w, out_b; x_w (the noisy-mel columns of the input projection); conv (w0, b0, w1, b1)."""
    f = lambda k: W[k].detach().float().cpu()
    blocks = []
    for i in range(depth):
        p = f"transformer_blocks.{i}."
        blocks.append(dict(qkv_w=torch.cat([f(p + f"attn.{n}.weight") for n in ("to_q", "to_k", "to_v")]),
                           qkv_b=torch.cat([f(p + f"attn.{n}.bias") for n in ("to_q", "to_k", "to_v")]),
                           o_w=f(p + "attn.to_out.0.weight"), o_b=f(p + "attn.to_out.0.bias"), f1_w=f(p + "ff.ff.0.0.weight"), f1_b=f(p + "ff.ff.0.0.bias"),
                           f2_w=f(p + "ff.ff.2.weight"), f2_b=f(p + "ff.ff.2.bias")))
    return dict(blocks=blocks, out_w=f("proj_out.weight"), out_b=f("proj_out.bias"), x_w=f("input_embed.proj.weight")[:, :mel],
                conv=tuple(f(f"input_embed.conv_pos_embed.conv1d.{i}.{k}") for i in (0, 2) for k in ("weight", "bias")))


def stage_ada(ada, l, D, depth):
    """The AdaLN row's slots of block l: (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp) (modules.py:312); l = depth: the final
    pair (scale, shift) (modules.py:333)."""
    a = ada.reshape(-1)
    n = 6 if l < depth else 2
    return tuple(a[l * 6 * D + i * D:l * 6 * D + (i + 1) * D] for i in range(n))


def _ln64(x):
    x = x.double()
    d = x - x.mean(dim=-1, keepdim=True)
    return d * torch.rsqrt((d * d).mean(dim=-1, keepdim=True) + STAGE_EPS)


def _rope_table(pos, f64):
    """(cos, sin) [len(pos), 32, 2] of the positions: angle = pos * 10000^(-2j / 64); fp32 as the plan's table, or fp64"""
    dt = torch.float64 if f64 else torch.float32
    inv = 1.0 / (10000.0 ** (torch.arange(0, 64, 2, dtype=dt) / 64.0))
    ang = pos.to(dt)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1)


def _rope_apply(lin, cs, inner, rope_heads):
    out = lin.clone()
    cos, sin = cs[..., 0], cs[..., 1]
    for part in range(2):
        for h in range(rope_heads):
            c0 = part * inner + h * 64
            v = lin[:, c0:c0 + 64].reshape(-1, 32, 2)
            out[:, c0:c0 + 64] = torch.stack([v[..., 0] * cos - v[..., 1] * sin, v[..., 1] * cos + v[..., 0] * sin], dim=-1).reshape(-1, 64)
    return out


def _fp16_clamp(t):
    return t.clamp(min=-65504.0, max=65504.0)


def stage_ref(stage, **kw):
    """fp64 restatement of ONE stage from the probe of the stage before it (kw: what stage_emulate takes; the model's own weights, in fp64)."""
    d = lambda t: t.double()
    if stage in ("n1", "final_norm"):
        return _ln64(kw["x"]) * (1.0 + d(kw["scale"])) + d(kw["shift"])
    if stage == "stats":
        x = d(kw["x"])
        dd = x - x.mean(dim=-1, keepdim=True)
        return torch.stack([x.mean(dim=-1), torch.rsqrt((dd * dd).mean(dim=-1) + STAGE_EPS)], dim=-1)
    if stage in ("qkv", "qkv_folded"):
        n = d(kw["n1"]) if stage == "qkv" else _ln64(kw["x"]) * (1.0 + d(kw["scale"])) + d(kw["shift"])
        lin = n @ d(kw["w"]).t() + d(kw["b"])
        inner = lin.shape[1] // 3
        ref, _ = rope_ref(lin, lin.abs(), _rope_table(kw["pos"], True), len(kw["pos"]), kw["rope_heads"])  # (row i takes table row i)
        if kw["qs"]:
            ref[:, :inner] *= QSCALE
        return ref
    if stage == "ff1":
        n = _ln64(kw["x"]) * (1.0 + d(kw["scale"])) + d(kw["shift"])
        return F.gelu(n @ d(kw["w"]).t() + d(kw["b"]), approximate="tanh")
    if stage == "resid":  # clamp_fp16(x + gate (a W^T + b))
        return _fp16_clamp(d(kw["x"]) + d(kw["gate"]) * (d(kw["a"]) @ d(kw["w"]).t() + d(kw["b"])))
    if stage == "vout":
        return d(kw["h"]) @ d(kw["w"]).t() + d(kw["b"])
    if stage == "ctx":  # attn_ref_terms' softmax (base 2 under qs) for the sampled queries alone: q [S, H, 64], k / v [keys, H, 64] of their sequence
        q, k, v = d(kw["q"]).transpose(0, 1), d(kw["k"]).transpose(0, 1), d(kw["v"]).transpose(0, 1)
        s = q @ k.transpose(-1, -2) * (LN2 if kw["qs"] else 0.125)
        return (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(q.shape[1], -1)
    if stage == "input_embed":
        return _fp16_clamp(d(kw["x"]) @ d(kw["w"]).t() + d(kw["base"]))
    if stage == "x_in":  # ie [B, L, D]: the stream plus mish(conv(mish(conv(.)))) of it, every utterance by itself
        w0, b0, w1, b1 = kw["conv"]
        ie = d(kw["ie"])
        return _fp16_clamp(ie + F.mish(conv31_ref(F.mish(conv31_ref(ie, w0, b0)), w1, b1)))
    raise ValueError(stage)


def _stage_stats_f32(x, pivot, quarter=False):
    """(mean, rstd) as the residual epilogues and lnf_row_stats take them: fp32 sums of (h - pivot) and (h - pivot)^2 per 64-feature tile, added
    tile by tile; mean = pivot + s1 / D, var = s2 / D - (s1 / D)^2.  quarter: the defect -- the first quarter of the row alone."""
    x = x.float()
    D = x.shape[1]
    pv = torch.zeros(x.shape[0]) if pivot is None else pivot.float()
    dd = x - pv[:, None]
    if quarter:
        dd, D = dd[:, :D // 4], D // 4
    s1, s2 = torch.zeros(x.shape[0]), torch.zeros(x.shape[0])
    for c in range(0, D, 64):
        s1 = s1 + dd[:, c:c + 64].sum(dim=1)
        s2 = s2 + (dd[:, c:c + 64] * dd[:, c:c + 64]).sum(dim=1)
    md = s1 / D
    var = (s2 / D - md * md).clamp(min=0.0)
    return pv + md, 1.0 / torch.sqrt(var + STAGE_EPS)


def _stage_folded_f32(x, mean, rstd, w, b, scale, shift, q_rows, defect="none", v_rows=None):
    """rstd (x . W'^T - mean c1) + c2 with W' = fp16(W (1 + scale) qs), c1 = rowsum W', c2 = (b + W . shift) qs (lnfold.hip); q_rows > 0: the
    first q_rows rows carry QSCALE.  v_rows = (first, count): the v rows of a fused projection (the defect moves their c1 / c2)."""
    qsv = torch.ones(w.shape[0])
    if q_rows:
        qsv[:q_rows] = {"q_not_scaled": 1.0, "q_scaled_twice": QSCALE * QSCALE}.get(defect, QSCALE)
    qsv = qsv.float()
    wt = (w.float() * (1.0 + scale.float())[None, :] * qsv[:, None]).half().float()
    c1 = wt.sum(dim=1)
    c2 = (b.float() + w.float() @ shift.float()) * qsv
    if defect == "v_c1_c2_shifted_by_inner" and v_rows:
        v0, n = v_rows
        c1, c2 = c1.clone(), c2.clone()
        c1[v0:v0 + n], c2[v0:v0 + n] = c1[v0 - n:v0].clone(), c2[v0 - n:v0].clone()
    return rstd.float()[:, None] * (x.float() @ wt.t() - mean.float()[:, None] * c1[None, :]) + c2[None, :]


def stage_emulate(precision, stage, defect="none", **kw):
    """CPU restatement of ONE stage of the production-mode evaluation (csrc/dit_eval.hip) with the kernel's roundings, in float32: the fp16
    stream, 16-bit operands of the mode `precision` with fp32 accumulation, W' = fp16(W (1 + scale)) with c1 and c2 under the fold, one rounding
    to the stored type (the mode's; fp16 saturating for the stream; fp32 for the statistics and proj_out).  Stages and their inputs:
        n1, final_norm  x, scale, shift                                       LayerNorm pass of the fp16 stream
        stats           x, pivot [S] or None                                  (mean, rstd) [S, 2] of the stream rows
        qkv             n1, w, b, pos, rope_heads, qs                         block 0's unfolded projection (qs: the q rows of w, b carry QSCALE)
        qkv_folded      x, scale, shift, w, b, pos, rope_heads, qs [, xstat]  the folded projection from the stream itself
        ff1             x, scale, shift, w, b [, xstat]                       folded FF1 + GELU(tanh)
        resid           x, a, w, b, gate                                      x + gate (a W^T + b) into the stream
        ctx             q [S, H, 64], k, v [keys, H, 64], qs                  softmax attention of the sampled queries over their sequence's keys
        vout            h, w, b
        input_embed     x, w, base;  x_in: ie [B, L, D], conv
    `defect` (STAGE_DEFECTS) plants what tests/test_gpu_production_stages.py is there to catch, at the stage it belongs to; xstat: the stream
    rows whose statistics a folded projection uses when they are not its own input's (the previous site's: a defect)."""
    assert defect in STAGE_DEFECTS
    rnd = lambda t: round_to(precision, t)
    if stage in ("n1", "final_norm"):
        x = kw["x"].float()
        dd = x - x.mean(dim=-1, keepdim=True)
        scale, shift = (kw["shift"], kw["scale"]) if (defect == "final_pair_swapped" and stage == "final_norm") else (kw["scale"], kw["shift"])
        return rnd(dd * torch.rsqrt((dd * dd).mean(dim=-1, keepdim=True) + STAGE_EPS) * (1.0 + scale.float()) + shift.float())
    if stage == "stats":
        return torch.stack(_stage_stats_f32(kw["x"], kw.get("pivot"), quarter=defect == "stats_quarter_row"), dim=-1)
    if stage in ("qkv", "qkv_folded"):
        inner = kw["w"].shape[0] // 3
        if stage == "qkv":
            w, b = kw["w"].float().clone(), kw["b"].float().clone()
            if kw["qs"]:
                s = {"q_not_scaled": 1.0, "blk0_unscaled_weight_copy": 1.0, "q_scaled_twice": QSCALE * QSCALE}.get(defect, QSCALE)
                w[:inner] *= torch.tensor(s, dtype=torch.float32)
                b[:inner] *= torch.tensor(s, dtype=torch.float32)
            lin = rnd(kw["n1"]) @ rnd(w).t() + b
        else:
            mean, rstd = _stage_stats_f32(kw.get("xstat", kw["x"]), None, quarter=defect == "stats_quarter_row")
            lin = _stage_folded_f32(kw["x"], mean, rstd, kw["w"], kw["b"], kw["scale"], kw["shift"], inner if kw["qs"] else 0, defect, (2 * inner, inner))
        return rnd(_rope_apply(lin, _rope_table(kw["pos"], False), inner, kw["rope_heads"]))
    if stage == "ff1":
        mean, rstd = _stage_stats_f32(kw.get("xstat", kw["x"]), None, quarter=defect == "stats_quarter_row")
        return rnd(F.gelu(_stage_folded_f32(kw["x"], mean, rstd, kw["w"], kw["b"], kw["scale"], kw["shift"], 0), approximate="tanh"))
    if stage == "resid":
        t = (rnd(kw["a"]) @ rnd(kw["w"]).t() + kw["b"].float()) * kw["gate"].float()
        return (kw["x"].float() + t).clamp(min=-65504.0, max=65504.0).half().float()
    if stage == "vout":
        return rnd(kw["h"]) @ rnd(kw["w"]).t() + kw["b"].float()
    if stage == "ctx":  # fp32 scores, numerators exp2(s c - m) rounded once to the mode's type for the PV product, the row sum from the unrounded ones
        q, k, v = [rnd(kw[n]).transpose(0, 1) for n in ("q", "k", "v")]
        c = torch.tensor(1.0 if kw["qs"] else QSCALE, dtype=torch.float32)
        s = q @ k.transpose(-1, -2)
        m = (s * c).amax(dim=-1, keepdim=True)
        num = torch.exp2(torch.addcmul(-m, s, c))
        o = rnd(num) @ v / num.sum(dim=-1, keepdim=True)
        return rnd(o.transpose(0, 1).reshape(q.shape[1], -1))
    if stage == "input_embed":
        return (rnd(kw["x"]) @ rnd(kw["w"]).t() + kw["base"].half().float()).clamp(min=-65504.0, max=65504.0).half().float()
    if stage == "x_in":
        w0, b0, w1, b1 = [t.float() for t in kw["conv"]]
        ie = kw["ie"].float()
        conv = lambda t, w, b: F.conv1d(t.transpose(1, 2), rnd(w), b, padding=15, groups=16).transpose(1, 2)
        y = rnd(F.mish(conv(rnd(F.mish(conv(rnd(ie), w0, b0))), w1, b1)))
        return (ie + y).clamp(min=-65504.0, max=65504.0).half().float()
    raise ValueError(stage)


def stage_row_errors(X, R, parts=1, stats=False):
    """The row metric.  e[r] = max over the `parts` equal column groups of a row (q | k | v) of max_c |X - R| / max_c |R| within the group.
    stats: X, R = (mean, rstd) [S, 2]: max(|mean error| in units of the row's standard deviation, relative rstd error)."""
    X, R = X.double(), R.double()
    if stats:
        return torch.maximum((X[:, 0] - R[:, 0]).abs() * R[:, 1], (X[:, 1] - R[:, 1]).abs() / R[:, 1])
    S = R.shape[0]
    err = (X - R).abs().reshape(S, parts, -1).amax(dim=-1)
    return (err / R.abs().reshape(S, parts, -1).amax(dim=-1).clamp(min=1e-300)).amax(dim=-1)


def stage_row_bias(X, R, parts=1):
    """The second row metric: |sum_c (X - R) sign(R)| / sum_c |R| per column group, the largest group.  A rounding error changes sign from column
    to column and averages out over a row (1 / sqrt(columns) of the first metric); a wrong row factor -- a row's rstd, a gate -- or a wrong
    row offset does not."""
    X, R = X.double(), R.double()
    S = R.shape[0]
    num = ((X - R) * torch.sign(R)).reshape(S, parts, -1).sum(dim=-1).abs()
    return (num / R.abs().reshape(S, parts, -1).sum(dim=-1).clamp(min=1e-300)).amax(dim=-1)


def _take(t, idx):
    return t[idx.to(t.device)].float().cpu()


def stage_shares(probes, Wst, lay, idx, precision, qs, depth, rope_heads, heads, margin=None, only=None, say=print):
    """Every probed stage of one evaluation against the fp64 restatement R of that stage, computed from the probe of the stage before it, on the
    rows idx (valid rows: stage_sample_rows); the bound per stage is margin x the worst row error of the restatement E with the kernel's
    roundings (stage_emulate) from the same inputs.  probes: name -> tensor [rows.., cols] (host or device; rows beyond the sample are read only
    for the keys of attention).  Folded evaluations (stats probes present) and unfolded ones alike.
    -> {stage: (worst row of the probe / bound, restatement's worst row error, probe's worst row error)}; prints one line per stage."""
    margin = STAGE_MARGIN if margin is None else margin
    D = Wst["blocks"][0]["o_w"].shape[0]
    inner = Wst["blocks"][0]["o_w"].shape[1]
    ada = probes["adaln"].float().cpu()
    pos = lay["pos"][idx]
    out = {}

    def judge(name, X, R, E, **kw):
        eE, eX = stage_row_errors(E, R, **kw), stage_row_errors(X, R, **kw)
        bound = margin * float(eE.max())
        assert torch.isfinite(X).all(), name
        share = float(eX.max()) / bound if bound > 0 else (0.0 if float(eX.max()) == 0 else float("inf"))
        line = (f"  {name}: restatement's worst row {float(eE.max()):.3e}, worst row {float(eX.max()):.3e} = {share:.3f} of the bound "
                f"(row {int(idx[int(eX.argmax())])})")
        if not kw.get("stats"):  # the signed row sum, held to the restatement's in the same way
            bE, bX = stage_row_bias(E, R, kw.get("parts", 1)), stage_row_bias(X, R, kw.get("parts", 1))
            bshare = float(bX.max()) / (margin * float(bE.max())) if float(bE.max()) > 0 else (0.0 if float(bX.max()) == 0 else float("inf"))
            line += f"; row bias {float(bE.max()):.3e} / {float(bX.max()):.3e} = {bshare:.3f} (row {int(idx[int(bX.argmax())])})"
            share = max(share, bshare)
        out[name] = (share, float(eE.max()), float(eX.max()))
        say(line)

    x_prev = _take(probes["blk0.x_in"], idx)
    pivot = None  # the previous site's means (site 0 has none)
    for l in range(depth):
        Wb = Wst["blocks"][l]
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = stage_ada(ada, l, D, depth)
        t = f"blk{l}."
        folded1 = (t + "stats1") in probes
        if not folded1:
            n1 = _take(probes[t + "n1"], idx)
            kw = dict(x=x_prev, scale=sc_a, shift=sh_a)
            judge(t + "n1", n1, stage_ref("n1", **kw), stage_emulate(precision, "n1", **kw))
            kw = dict(n1=n1, w=Wb["qkv_w"], b=Wb["qkv_b"], pos=pos, rope_heads=rope_heads, qs=qs)
            stage = "qkv"
        else:
            kw = dict(x=x_prev, pivot=pivot)
            st1 = _take(probes[t + "stats1"], idx)
            judge(t + "stats1", st1, stage_ref("stats", **kw), stage_emulate(precision, "stats", **kw), stats=True)
            pivot = st1[:, 0]
            kw = dict(x=x_prev, scale=sc_a, shift=sh_a, w=Wb["qkv_w"], b=Wb["qkv_b"], pos=pos, rope_heads=rope_heads, qs=qs)
            stage = "qkv_folded"
        qkv = _take(probes[t + "qkv"], idx)
        judge(t + "qkv", qkv, stage_ref(stage, **kw), stage_emulate(precision, stage, **kw), parts=3)
        # attention: the sampled queries of a sequence over that sequence's probed keys
        ctx = _take(probes[t + "ctx"], idx)
        R, E = torch.empty(len(idx), inner, dtype=torch.float64), torch.empty(len(idx), inner)
        for sid in lay["seg"][idx].unique().tolist():
            r0, n = lay["seg_rows"][sid]
            sel = (lay["seg"][idx] == sid).nonzero().reshape(-1)
            keys = probes[t + "qkv"][r0:r0 + n].float().cpu()[lay["key"][r0:r0 + n]].reshape(-1, 3, heads, 64)
            kw = dict(q=qkv[sel].reshape(-1, 3, heads, 64)[:, 0], k=keys[:, 1], v=keys[:, 2], qs=qs)
            R[sel], E[sel] = stage_ref("ctx", **kw), stage_emulate(precision, "ctx", **kw)
        judge(t + "ctx", ctx, R, E)
        x_attn = _take(probes[t + "x_attn"], idx)
        kw = dict(x=x_prev, a=ctx, w=Wb["o_w"], b=Wb["o_b"], gate=g_a)
        judge(t + "x_attn", x_attn, stage_ref("resid", **kw), stage_emulate(precision, "resid", **kw))
        if (t + "stats2") in probes:
            kw = dict(x=x_attn, pivot=pivot)
            st2 = _take(probes[t + "stats2"], idx)
            judge(t + "stats2", st2, stage_ref("stats", **kw), stage_emulate(precision, "stats", **kw), stats=True)
            pivot = st2[:, 0]
        ff1 = _take(probes[t + "ff1"], idx)
        kw = dict(x=x_attn, scale=sc_m, shift=sh_m, w=Wb["f1_w"], b=Wb["f1_b"])
        judge(t + "ff1", ff1, stage_ref("ff1", **kw), stage_emulate(precision, "ff1", **kw))
        x_ff = _take(probes[t + "x_ff"], idx)
        kw = dict(x=x_attn, a=ff1, w=Wb["f2_w"], b=Wb["f2_b"], gate=g_m)
        judge(t + "x_ff", x_ff, stage_ref("resid", **kw), stage_emulate(precision, "resid", **kw))
        x_prev = x_ff
    scale, shift = stage_ada(ada, depth, D, depth)
    fn = _take(probes["final_norm"], idx)
    kw = dict(x=x_prev, scale=scale, shift=shift)
    judge("final_norm", fn, stage_ref("final_norm", **kw), stage_emulate(precision, "final_norm", **kw))
    kw = dict(h=fn, w=Wst["out_w"], b=Wst["out_b"])
    judge("vout", _take(probes["vout"], idx), stage_ref("vout", **kw), stage_emulate(precision, "vout", **kw))
    return out


def stage_check(name, shares):
    """asserts every stage of stage_shares within its bound; the message names the stages that are not"""
    bad = {k: round(v[0], 3) for k, v in shares.items() if not v[0] <= 1.0}
    assert not bad, f"{name}: stages out of bound (worst row / bound): {bad}"


def stage_chain(precision, Wst, ada, lay, x_in, qs, depth, rope_heads, heads, defect="none", ada_other=None):
    """A whole folded evaluation restated on the CPU with stage_emulate, every stage from the one before it over ALL rows of the layout: the
    probes a device would give (the host stand-in of tests/test_production_stage_bound_host.py).  `defect` (STAGE_DEFECTS) is planted where the
    library would carry it:
        stats_quarter_row            every statistics site sums the first quarter of the row
        stats_of_previous_site       a folded projection reads the statistics table of site k - 1
        v_c1_c2_shifted_by_inner     the v rows of a folded QKV projection take the c1 / c2 of the k rows
        fold_rows_of_another_time    W', c1, c2 come from the AdaLN row ada_other (another evaluation time's rows of the fold table)
        q_not_scaled, q_scaled_twice the q rows carry no / twice the softmax scale (qs)
        gate_mlp_for_gate_msa        the out-projection takes slot 5 of the AdaLN row
        blk0_unscaled_weight_copy    block 0 projects with the copy whose q rows carry no scale (qs)
        final_pair_swapped           the final AdaLN reads (shift, scale)
        rope_position_is_row_index   RoPE position = row % N, not the row's position in its utterance (a ragged batch)"""
    D = Wst["blocks"][0]["o_w"].shape[0]
    inner = Wst["blocks"][0]["o_w"].shape[1]
    rows = lay["rows"]
    pos = torch.arange(rows) % lay["N"] if defect == "rope_position_is_row_index" else lay["pos"]
    probes = {"adaln": ada.clone(), "blk0.x_in": x_in.clone()}
    fold_ada = ada_other if defect == "fold_rows_of_another_time" else ada
    x, x_site_before, pivot = x_in, None, None  # x_site_before: the stream as the site before the current one saw it
    emu = lambda stage, **kw: stage_emulate(precision, stage, defect=defect, **kw)
    for l in range(depth):
        Wb = Wst["blocks"][l]
        t = f"blk{l}."
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = stage_ada(ada, l, D, depth)
        fsh_a, fsc_a, _, fsh_m, fsc_m, _ = stage_ada(fold_ada, l, D, depth)
        if l == 0:
            probes[t + "n1"] = emu("n1", x=x, scale=sc_a, shift=sh_a)
            probes[t + "qkv"] = emu("qkv", n1=probes[t + "n1"], w=Wb["qkv_w"], b=Wb["qkv_b"], pos=pos, rope_heads=rope_heads, qs=qs)
        else:
            probes[t + "stats1"] = emu("stats", x=x, pivot=pivot)
            pivot = probes[t + "stats1"][:, 0]
            xstat = x_site_before if defect == "stats_of_previous_site" else x
            probes[t + "qkv"] = emu("qkv_folded", x=x, xstat=xstat, scale=fsc_a, shift=fsh_a, w=Wb["qkv_w"], b=Wb["qkv_b"], pos=pos, rope_heads=rope_heads, qs=qs)
        qkv = probes[t + "qkv"].reshape(rows, 3, heads, 64)
        ctx = torch.zeros(rows, inner)
        for sid, (r0, n) in lay["seg_rows"].items():
            kmask = lay["key"][r0:r0 + n]
            ctx[r0:r0 + n] = emu("ctx", q=qkv[r0:r0 + n, 0], k=qkv[r0:r0 + n, 1][kmask], v=qkv[r0:r0 + n, 2][kmask], qs=qs)
        probes[t + "ctx"] = ctx
        gate = g_m if defect == "gate_mlp_for_gate_msa" else g_a
        x_attn = emu("resid", x=x, a=ctx, w=Wb["o_w"], b=Wb["o_b"], gate=gate)
        pad = (~lay["key"]) & (lay["seg"] >= 0)
        x_attn[pad] = x[pad]  # rowbits: a padded query row keeps its bits
        probes[t + "x_attn"] = x_attn
        probes[t + "stats2"] = emu("stats", x=x_attn, pivot=pivot)
        pivot = probes[t + "stats2"][:, 0]
        probes[t + "ff1"] = emu("ff1", x=x_attn, xstat=x if defect == "stats_of_previous_site" else x_attn, scale=fsc_m, shift=fsh_m, w=Wb["f1_w"], b=Wb["f1_b"])
        x_ff = emu("resid", x=x_attn, a=probes[t + "ff1"], w=Wb["f2_w"], b=Wb["f2_b"], gate=g_m)
        probes[t + "x_ff"] = x_ff
        x_site_before, x = x_attn, x_ff
    scale, shift = stage_ada(ada, depth, D, depth)
    probes["final_norm"] = emu("final_norm", x=x, scale=scale, shift=shift)
    probes["vout"] = emu("vout", h=probes["final_norm"], w=Wst["out_w"], b=Wst["out_b"])
    return probes
