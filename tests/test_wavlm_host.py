"""Host side of the WavLM feature extractor (eraxvif5tts_amd/eval/wavlm.py): the fp64 restatement tests/wavlm_ref.py against the golden
hidden states of a seeded tiny ``transformers.WavLMModel`` (tests/golden/wavlm_tiny.npz, tools/make_wavlm_golden.py) and, where transformers is
installed, against fresh models; the bucket table; key mapping, strictness and config refusals; the frame rule.  No GPU."""
import math

import numpy as np
import pytest
import torch

import wavlm_ref as R
from conftest import load_golden
from eraxvif5tts_amd.eval import SpeakerEncoder, speaker_similarity
from eraxvif5tts_amd.eval import speaker as speaker_mod
from eraxvif5tts_amd.eval import wavlm as W
from eraxvif5tts_amd.eval.wavlm import WavLMExtractor

CFG = R.TINY_CONFIG


def golden_state():
    z = load_golden("wavlm_tiny")
    return z, {k[6:]: torch.from_numpy(z[k]) for k in z if k.startswith("state.")}


def test_restatement_equals_golden_to_fp64_roundoff():
    z, P = golden_state()
    P64 = R.to_dtype(P, torch.float64)
    for i, n in enumerate(R.GOLDEN_SAMPLES):
        wave, hs = torch.from_numpy(z[f"wave{i}"]), torch.from_numpy(z[f"hs{i}"])
        assert wave.numel() == n and hs.shape == (CFG["num_hidden_layers"] + 1, R.frames_of(CFG, n), CFG["hidden_size"])
        got = R.forward(P64, CFG, wave, final_norm="hf")
        assert float((got - hs).abs().max()) <= 1e-12 * float(hs.abs().max())
        s3 = R.forward(P64, CFG, wave, final_norm="s3prl")
        assert torch.equal(s3[:-1], got[:-1]) and not torch.allclose(s3[-1], got[-1])


def test_golden_lengths_reach_log_and_clamped_buckets():
    nb = CFG["num_buckets"] // 2
    b2, b37, b130 = (set(R.relative_buckets(CFG, T).tolist()) for T in (2, 37, 130))
    exact = set(range(nb // 2)) | {nb + i for i in range(nb // 2)}
    assert b2 <= exact and not b37 <= exact
    assert nb - 1 not in b37 and {nb - 1, 2 * nb - 1} <= b130


def _hf_model(conv_bias, seed):
    transformers = pytest.importorskip("transformers")
    cfg = dict(CFG, conv_bias=conv_bias)
    torch.manual_seed(seed)
    model = transformers.WavLMModel(transformers.WavLMConfig(
        num_feat_extract_layers=len(cfg["conv_dim"]), feat_extract_norm="layer", do_stable_layer_norm=True, hidden_dropout=0.0, activation_dropout=0.0,
        attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0, mask_feature_prob=0.0, **cfg)).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    return cfg, model.double()


@pytest.mark.parametrize("conv_bias", [False, True])
def test_restatement_equals_fresh_transformers_model(conv_bias):
    cfg, model = _hf_model(conv_bias, seed=5 + conv_bias)
    P = {k: v.detach().clone() for k, v in model.state_dict().items() if k != "masked_spec_embed"}
    assert ("feature_extractor.conv_layers.1.conv.bias" in P) == conv_bias
    g = torch.Generator().manual_seed(9)
    for n in (50, 413, 2620):
        wave = torch.randn(n, generator=g, dtype=torch.float64)
        with torch.no_grad():
            hs = torch.stack([h[0] for h in model(wave[None], output_hidden_states=True).hidden_states])
        got = R.forward(P, cfg, wave, final_norm="hf")
        assert got.shape == hs.shape
        assert float((got - hs).abs().max()) <= 1e-12 * float(hs.abs().max())


def test_bucket_table_equals_compute_bias():
    transformers = pytest.importorskip("transformers")
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    for nbuckets, maxd, T in ((32, 64, 130), (320, 800, 1000)):
        att = WavLMAttention(embed_dim=64, num_heads=4, num_buckets=nbuckets, max_distance=maxd)
        bias = att.compute_bias(T, T)  # [H, T, T]
        b = W.relative_buckets(nbuckets, maxd, T)
        assert b.dtype == torch.int32 and b.shape == (2 * T - 1,)
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + (T - 1)
        assert torch.equal(att.rel_attn_embed.weight[b.long()[idx]].permute(2, 0, 1), bias)
        assert torch.equal(b.long(), R.relative_buckets(dict(num_buckets=nbuckets, max_bucket_distance=maxd), T))
    # a longer table is the shorter one extended: the bucket is a function of the distance alone
    assert torch.equal(W.relative_buckets(320, 800, 4096)[4096 - 130:4096 + 129], W.relative_buckets(320, 800, 130))


def test_frame_count_rule():
    ex = WavLMExtractor(**CFG)
    large = WavLMExtractor()
    for n in (1, 9, 10, 49, 50, 51, 760, 2620, 16000):
        assert ex.frames(n) == R.frames_of(CFG, n)
    assert [ex.frames(n) for n in R.GOLDEN_SAMPLES] == [2, 37, 130]
    assert ex.frames(29) < 1 and ex.frames(30) == 1 and ex.frames(9) < 1
    assert large.frames(8000) == 24 and large.frames(16000) == 49 and large.frames(399) < 1 and large.frames(400) == 1
    try:
        import transformers
    except ImportError:
        return
    m = transformers.WavLMModel(transformers.WavLMConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=64))
    for n in (400, 401, 8000, 16000, 123457):
        assert large.frames(n) == int(m._get_feat_extract_output_lengths(n))


def test_load_state_dict_is_strict_and_maps_keys():
    _, P = golden_state()
    ex = WavLMExtractor(**CFG).load_state_dict(P)
    folded = R.fold_pos_conv(P[W._POS + "parametrizations.weight.original0"].double(), P[W._POS + "parametrizations.weight.original1"].double()).float()
    assert torch.equal(ex._state[W._POS + "weight"], folded)
    assert set(ex._state) == set(R.state_spec(CFG, folded=True))
    # weight_g / weight_v and the folded form load the same tensors; masked_spec_embed is ignored
    old = {k: v for k, v in P.items() if "parametrizations" not in k}
    old[W._POS + "weight_g"], old[W._POS + "weight_v"] = P[W._POS + "parametrizations.weight.original0"], P[W._POS + "parametrizations.weight.original1"]
    old["masked_spec_embed"] = torch.zeros(CFG["hidden_size"])
    ex2 = WavLMExtractor(**CFG).load_state_dict(old)
    ex3 = WavLMExtractor(**CFG).load_state_dict(dict(ex._state))
    for k in ex._state:
        assert torch.equal(ex._state[k], ex2._state[k]) and torch.equal(ex._state[k], ex3._state[k])
    missing = dict(P)
    del missing["encoder.layers.1.attention.gru_rel_pos_const"]
    with pytest.raises(KeyError, match="encoder.layers.1.attention.gru_rel_pos_const"):
        WavLMExtractor(**CFG).load_state_dict(missing)
    with pytest.raises(KeyError, match="encoder.layers.1.attention.rel_attn_embed.weight"):
        WavLMExtractor(**CFG).load_state_dict(dict(P, **{"encoder.layers.1.attention.rel_attn_embed.weight": torch.zeros(32, 4)}))
    with pytest.raises(ValueError, match="feature_projection.projection.weight"):
        WavLMExtractor(**CFG).load_state_dict(dict(P, **{"feature_projection.projection.weight": torch.zeros(64, 33)}))
    with pytest.raises(KeyError, match="original1"):
        WavLMExtractor(**CFG).load_state_dict({k: v for k, v in P.items() if not k.endswith("original1")})
    with pytest.raises(KeyError, match="conv.bias"):
        WavLMExtractor(**dict(CFG, conv_bias=True)).load_state_dict(P)


def _to_fairseq(P):
    out = {}
    for k, v in P.items():
        k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        k = k.replace("encoder.pos_conv_embed.conv.", "encoder.pos_conv.0.")
        k = k.replace(".attention.gru_rel_pos_linear.", ".self_attn.grep_linear.").replace(".attention.gru_rel_pos_const", ".self_attn.grep_a")
        k = k.replace(".attention.rel_attn_embed.", ".self_attn.relative_attention_bias.").replace(".attention.", ".self_attn.")
        k = k.replace(".feed_forward.intermediate_dense.", ".fc1.").replace(".feed_forward.output_dense.", ".fc2.")
        if k.startswith("encoder.layers.") and ".layer_norm." in k:
            k = k.replace(".layer_norm.", ".self_attn_layer_norm.")
        k = k.replace("feature_projection.layer_norm.", "layer_norm.").replace("feature_projection.projection.", "post_extract_proj.")
        if k.startswith("feature_extractor."):
            k = k.replace(".conv.", ".0.").replace(".layer_norm.", ".2.1.")
        out[k] = v
    return out


def test_fairseq_names_and_speaker_checkpoint(tmp_path):
    _, P = golden_state()
    fs = _to_fairseq(P)
    assert "post_extract_proj.weight" in fs and "encoder.layers.2.self_attn.grep_a" in fs and "feature_extractor.conv_layers.1.2.1.bias" in fs
    ref = WavLMExtractor(**CFG).load_state_dict(P)
    ex = WavLMExtractor(**CFG).load_state_dict(dict(fs, mask_emb=torch.zeros(64)), naming="fairseq")
    for k in ref._state:
        assert torch.equal(ref._state[k], ex._state[k]), k
    with pytest.raises(KeyError, match="encoder.layers.0.self_attn.bogus"):
        WavLMExtractor(**CFG).load_state_dict(dict(fs, **{"encoder.layers.0.self_attn.bogus": torch.zeros(1)}), naming="fairseq")
    with pytest.raises(KeyError):
        WavLMExtractor(**CFG).load_state_dict(P, naming="fairseq")
    # the speaker checkpoint holds them behind feature_extract.model., next to the head's own tensors, which this loader leaves alone
    ckpt = {"model": dict({"feature_extract.model." + k: v for k, v in fs.items()}, **{"feature_weight": torch.zeros(4), "linear.bias": torch.zeros(3)})}
    path = tmp_path / "sv.pth"
    torch.save(ckpt, path)
    ex = WavLMExtractor.from_speaker_checkpoint(str(path), **CFG)
    for k in ref._state:
        assert torch.equal(ref._state[k], ex._state[k]), k
    torch.save({"model": {"feature_weight": torch.zeros(4)}}, path)
    with pytest.raises(KeyError, match="feature_extract.model"):
        WavLMExtractor.from_speaker_checkpoint(str(path), **CFG)


@pytest.mark.parametrize("bad, word", [
    (dict(feat_extract_norm="group"), "feat_extract_norm"),
    (dict(do_stable_layer_norm=False), "do_stable_layer_norm"),
    (dict(add_adapter=True), "add_adapter"),
    (dict(num_attention_heads=5), "num_attention_heads"),
    (dict(num_attention_heads=2), "head dimension 32"),
    (dict(num_conv_pos_embedding_groups=8), "num_conv_pos_embedding_groups"),
    (dict(conv_dim=(32, 32, 40)), "conv_dim"),
    (dict(hidden_act="relu"), "hidden_act"),
])
def test_config_refusals_name_the_field(bad, word):
    with pytest.raises(ValueError, match=word):
        WavLMExtractor(**dict(CFG, **bad))
    with pytest.raises(ValueError, match="final_norm"):
        WavLMExtractor(final_norm="fairseq", **CFG)


def test_defaults_are_wavlm_large():
    ex = WavLMExtractor()
    assert ex.cfg["conv_dim"] == (512,) * 7 and ex.layers == 25 and ex.feat_dim == 1024 and ex.final_norm == "s3prl" and ex.normalize_input
    assert {k: ex.cfg[k] for k in R.LARGE_CONFIG} == R.LARGE_CONFIG
    spec = W._spec(ex.cfg)
    assert spec["encoder.pos_conv_embed.conv.weight"] == (1024, 64, 128) and spec["encoder.layers.0.attention.rel_attn_embed.weight"] == (320, 16)
    assert sum(math.prod(s) for s in spec.values()) > 300e6


def test_extract_refuses_bad_input_before_touching_the_device():
    _, P = golden_state()
    ex = WavLMExtractor(**CFG).load_state_dict(P)
    with pytest.raises(ValueError, match="too short"):
        ex.extract([torch.zeros(760), torch.zeros(29)])
    with pytest.raises(ValueError, match="1-D"):
        ex.extract([torch.zeros(1, 760)])
    with pytest.raises(ValueError, match="non-empty"):
        ex.extract([])
    assert ex._native is None
    with pytest.raises(RuntimeError, match="no weights"):
        WavLMExtractor(**CFG).native()


def test_speaker_similarity_without_extractor_still_raises_its_message():
    enc = SpeakerEncoder(feat_dim=32, channels=64, emb_dim=16, layers=3)
    with pytest.raises(ValueError) as e:
        speaker_similarity(enc, [(torch.zeros(100), torch.zeros(100))], feature_extractor=None)
    assert str(e.value) == speaker_mod._NO_EXTRACTOR
    assert speaker_mod._NO_EXTRACTOR.startswith("speaker_similarity needs feature_extractor: a callable taking a list of 16 kHz waves")


def test_embed_packed_checks_its_input():
    enc = SpeakerEncoder(feat_dim=32, channels=64, emb_dim=16, layers=3)
    with pytest.raises(ValueError, match="contiguous fp32 device tensor"):
        enc.embed_packed(torch.zeros(3, 10, 32), [10])
    with pytest.raises(ValueError, match="contiguous fp32 device tensor"):
        enc.embed_packed([torch.zeros(3, 10, 32)], [10])
