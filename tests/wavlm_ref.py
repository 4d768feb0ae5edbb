"""Plain-torch restatement of the WavLM feature extractor at feat_extract_norm="layer", do_stable_layer_norm=True (microsoft/wavlm-large's
form), the checker of tests/test_wavlm_host.py and tests/test_gpu_wavlm.py.  Written against transformers' ``modeling_wavlm.py`` and pinned to it:
tests/test_wavlm_host.py compares it with a fresh ``WavLMModel`` in fp64 wherever transformers is installed, and with the hidden states
tools/make_wavlm_golden.py stored (tests/golden/wavlm_tiny.npz) everywhere.

dtype-generic: every function computes in the dtype of the tensors it is given (fp64 is the exact side of the GPU bounds, fp32 on the CPU their
yardstick).  Parameters travel as a name -> tensor dict under ``WavLMModel.state_dict()``'s names, the positional convolution either as the two
weight-norm tensors or already folded (``encoder.pos_conv_embed.conv.weight``).  One utterance per call (batch 1, no padding, no mask)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

TINY_CONFIG = dict(conv_dim=(32, 32, 32), conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), conv_bias=False, hidden_size=64, num_hidden_layers=3,
                   num_attention_heads=4, intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, num_buckets=32,
                   max_bucket_distance=64, layer_norm_eps=1e-5)
LARGE_CONFIG = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_bias=False, hidden_size=1024,
                    num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                    num_buckets=320, max_bucket_distance=800, layer_norm_eps=1e-5)
GOLDEN_SAMPLES = (50, 760, 2620)  # 2, 37 and 130 frames at TINY_CONFIG: one exact-bucket, one log-bucket and one clamped-last-bucket length


def to_dtype(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


def frames_of(cfg, n):
    """frames an utterance of n samples gives; below 1 (or negative) when it is too short"""
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        if n < k:
            return -1
        n = (n - k) // s + 1
    return n


def state_spec(cfg, folded=True):
    """name -> shape of every tensor the network reads (``folded``: the positional convolution as one weight)"""
    Fd, H, I, cd = cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"], tuple(cfg["conv_dim"])
    dh, k, cg = Fd // H, cfg["num_conv_pos_embeddings"], Fd // cfg["num_conv_pos_embedding_groups"]
    spec = {}
    for i, c in enumerate(cd):
        p = f"feature_extractor.conv_layers.{i}"
        spec[f"{p}.conv.weight"] = (c, 1 if i == 0 else cd[i - 1], cfg["conv_kernel"][i])
        if cfg["conv_bias"]:
            spec[f"{p}.conv.bias"] = (c,)
        spec[f"{p}.layer_norm.weight"] = spec[f"{p}.layer_norm.bias"] = (c,)
    spec["feature_projection.layer_norm.weight"] = spec["feature_projection.layer_norm.bias"] = (cd[-1],)
    spec["feature_projection.projection.weight"], spec["feature_projection.projection.bias"] = (Fd, cd[-1]), (Fd,)
    spec["encoder.pos_conv_embed.conv.bias"] = (Fd,)
    if folded:
        spec["encoder.pos_conv_embed.conv.weight"] = (Fd, cg, k)
    else:
        spec["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (1, 1, k)
        spec["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = (Fd, cg, k)
    spec["encoder.layer_norm.weight"] = spec["encoder.layer_norm.bias"] = (Fd,)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            spec[f"{p}.attention.{n}.weight"], spec[f"{p}.attention.{n}.bias"] = (Fd, Fd), (Fd,)
        spec[f"{p}.attention.gru_rel_pos_const"] = (1, H, 1, 1)
        spec[f"{p}.attention.gru_rel_pos_linear.weight"], spec[f"{p}.attention.gru_rel_pos_linear.bias"] = (8, dh), (8,)
        if i == 0:
            spec[f"{p}.attention.rel_attn_embed.weight"] = (cfg["num_buckets"], H)
        for n in ("layer_norm", "final_layer_norm"):
            spec[f"{p}.{n}.weight"] = spec[f"{p}.{n}.bias"] = (Fd,)
        spec[f"{p}.feed_forward.intermediate_dense.weight"], spec[f"{p}.feed_forward.intermediate_dense.bias"] = (I, Fd), (I,)
        spec[f"{p}.feed_forward.output_dense.weight"], spec[f"{p}.feed_forward.output_dense.bias"] = (Fd, I), (Fd,)
    return spec


def random_state(cfg, seed, folded=True):
    """fp32 parameters of a working size: LayerNorm weights around 1, everything else N(0, fan_in^-1/2)-ish, no tensor left at a special value"""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for name, shape in state_spec(cfg, folded).items():
        if name.endswith("layer_norm.weight") or name.endswith("gru_rel_pos_const") or name.endswith("original0"):
            P[name] = 1.0 + 0.2 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            P[name] = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("rel_attn_embed.weight"):
            P[name] = torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            P[name] = torch.randn(shape, generator=g) * (1.5 / math.sqrt(fan_in))
    return P


def fold_pos_conv(g, v):
    """weight_norm(dim=2): W = g * v / ||v||, the norm over dims (0, 1) per tap"""
    return g * v / v.norm(p=2, dim=(0, 1), keepdim=True)


def pos_conv_weight(P):
    for g, v in (("parametrizations.weight.original0", "parametrizations.weight.original1"), ("weight_g", "weight_v")):
        if f"encoder.pos_conv_embed.conv.{g}" in P:
            return fold_pos_conv(P[f"encoder.pos_conv_embed.conv.{g}"], P[f"encoder.pos_conv_embed.conv.{v}"])
    return P["encoder.pos_conv_embed.conv.weight"]


def relative_buckets(cfg, n):
    """the model's bucket of the distances d = key - query = -(n - 1) .. n - 1 (int64 [2 n - 1]); float log, as the model evaluates it"""
    d = torch.arange(-(n - 1), n, dtype=torch.long)
    nb = cfg["num_buckets"] // 2
    out = (d > 0).to(torch.long) * nb
    a = torch.abs(d)
    max_exact = nb // 2
    large = torch.log(a.float() / max_exact)
    large = large / math.log(cfg["max_bucket_distance"] / max_exact)
    large = large * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(a < max_exact, a, large)


def position_bias(P, cfg, T):
    """[H, T, T]: R[h][j - i]"""
    b = relative_buckets(cfg, T)
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + (T - 1)
    return P["encoder.layers.0.attention.rel_attn_embed.weight"][b[idx]].permute(2, 0, 1)


def normalize_wave(w):
    return F.layer_norm(w, w.shape)


def conv_layer(P, cfg, i, x):
    """x [1, cin, T] -> [1, cout, T']"""
    p = f"feature_extractor.conv_layers.{i}"
    y = F.conv1d(x, P[f"{p}.conv.weight"], P.get(f"{p}.conv.bias"), stride=cfg["conv_stride"][i])
    y = F.layer_norm(y.transpose(1, 2), (y.shape[1],), P[f"{p}.layer_norm.weight"], P[f"{p}.layer_norm.bias"], cfg["layer_norm_eps"])
    return F.gelu(y.transpose(1, 2))


def projection(P, cfg, x):
    """x [T, C] -> [T, hidden]"""
    y = F.layer_norm(x, (x.shape[-1],), P["feature_projection.layer_norm.weight"], P["feature_projection.layer_norm.bias"], cfg["layer_norm_eps"])
    return F.linear(y, P["feature_projection.projection.weight"], P["feature_projection.projection.bias"])


def pos_conv(x, w, b, groups):
    """x [T, C] -> x + gelu(conv(x)) with the last frame dropped when k is even"""
    k = w.shape[-1]
    y = F.conv1d(x.t().unsqueeze(0), w, b, padding=k // 2, groups=groups)
    if k % 2 == 0:
        y = y[:, :, :-1]
    return x + F.gelu(y)[0].t()


def gate(P, cfg, i, h):
    """h [T, hidden] (the normalised input) -> g [T, H]"""
    p = f"encoder.layers.{i}.attention"
    H = cfg["num_attention_heads"]
    T = h.shape[0]
    proj = F.linear(h.view(T, H, -1), P[f"{p}.gru_rel_pos_linear.weight"], P[f"{p}.gru_rel_pos_linear.bias"])
    ab = torch.sigmoid(proj.view(T, H, 2, 4).sum(-1))
    return ab[..., 0] * (ab[..., 1] * P[f"{p}.gru_rel_pos_const"].view(1, H) - 1.0) + 2.0


def attention_core(q, k, v, g, R):
    """q, k, v [T, H, dh]; g [T, H]; R [H, T, T] -> [T, H dh]"""
    T, H, dh = q.shape
    s = torch.einsum("ihd,jhd->hij", q * dh ** -0.5, k) + g.t().unsqueeze(-1) * R
    return torch.einsum("hij,jhd->ihd", torch.softmax(s, dim=-1), v).reshape(T, H * dh)


def encoder_layer(P, cfg, i, x, R, taps=None):
    p = f"encoder.layers.{i}"
    H, eps = cfg["num_attention_heads"], cfg["layer_norm_eps"]
    T, Fd = x.shape
    h = F.layer_norm(x, (Fd,), P[f"{p}.layer_norm.weight"], P[f"{p}.layer_norm.bias"], eps)
    q, k, v = (F.linear(h, P[f"{p}.attention.{n}.weight"], P[f"{p}.attention.{n}.bias"]).view(T, H, -1) for n in ("q_proj", "k_proj", "v_proj"))
    a = attention_core(q, k, v, gate(P, cfg, i, h), R)
    x = x + F.linear(a, P[f"{p}.attention.out_proj.weight"], P[f"{p}.attention.out_proj.bias"])
    if taps is not None:
        taps[f"layer{i}.attn"] = x
    h = F.layer_norm(x, (Fd,), P[f"{p}.final_layer_norm.weight"], P[f"{p}.final_layer_norm.bias"], eps)
    h = F.gelu(F.linear(h, P[f"{p}.feed_forward.intermediate_dense.weight"], P[f"{p}.feed_forward.intermediate_dense.bias"]))
    x = x + F.linear(h, P[f"{p}.feed_forward.output_dense.weight"], P[f"{p}.feed_forward.output_dense.bias"])
    if taps is not None:
        taps[f"layer{i}.out"] = x
    return x


@torch.no_grad()
def forward(P, cfg, wave, final_norm="hf", normalize_input=False, taps=None):
    """wave [n] -> hidden states [L, T, hidden] of one utterance, L = layers + 1.  ``taps`` (a dict) receives conv{i} [T_i, C], proj, posconv,
    layer{i}.attn and layer{i}.out [T, hidden]."""
    if final_norm not in ("hf", "s3prl"):
        raise ValueError(final_norm)
    x = wave.to(next(iter(P.values())).dtype)
    if normalize_input:
        x = normalize_wave(x)
    x = x.view(1, 1, -1)
    for i in range(len(cfg["conv_dim"])):
        x = conv_layer(P, cfg, i, x)
        if taps is not None:
            taps[f"conv{i}"] = x[0].t()
    x = projection(P, cfg, x[0].t())
    if taps is not None:
        taps["proj"] = x
    x = pos_conv(x, pos_conv_weight(P), P["encoder.pos_conv_embed.conv.bias"], cfg["num_conv_pos_embedding_groups"])
    if taps is not None:
        taps["posconv"] = x
    R = position_bias(P, cfg, x.shape[0])
    hs = [x]
    for i in range(cfg["num_hidden_layers"]):
        x = encoder_layer(P, cfg, i, x, R, taps)
        hs.append(x)
    if final_norm == "hf":
        hs[-1] = F.layer_norm(x, (x.shape[-1],), P["encoder.layer_norm.weight"], P["encoder.layer_norm.bias"], cfg["layer_norm_eps"])
    return torch.stack(hs)
