"""Host side of the speaker-similarity head: the plain-torch restatement (tests/speaker_ref.py) against the tensors captured from the reference's
ECAPA_TDNN (tests/golden/speaker.npz, tools/speaker_golden.py), and the argument handling of eraxvif5tts_amd.eval.speaker that needs no GPU.

Bound of the restatement: the fixture was written by the reference module in fp32; the restatement is the same torch graph in fp32, so the two
can differ only by what two fp32 evaluation orders of one graph differ by (another BLAS blocking, another thread count).  That is bounded by
the reference's OWN fp32 error, measured on the fixture: rel-L2(golden, restatement in fp64), observed 0.9e-7 .. 4.1e-7 over the taps and
embeddings (2.0e-6 on the T = 2 pool, whose residuals E[x^2] - mean^2 sit closest to the clamp).  Per tensor: rel-L2(restatement fp32, golden) <= rel-L2(golden, restatement fp64).  (Where the fixture was captured the left side is
0.0 on every tensor.)"""
import functools

import numpy as np
import pytest
import torch

import speaker_ref as R
from conftest import load_golden
from eraxvif5tts_amd.eval import SpeakerEncoder, speaker_similarity
from eraxvif5tts_amd.eval import speaker as S


@functools.lru_cache(maxsize=None)
def _golden():
    z = load_golden("speaker")
    for v in z.values():
        v.setflags(write=False)
    return z


def _golden_cfg(z):
    return {str(k): int(v) for k, v in zip(z["config_keys"], z["config_values"])}


def test_fixture_matches_the_restatements_rules():
    z = _golden()
    assert int(z["fill_version"]) == R.FILL_VERSION
    assert _golden_cfg(z) == R.GOLDEN_CONFIG
    assert tuple(int(t) for t in z["frames"]) == (2, 3, 9, 23)
    for T in z["frames"]:
        np.testing.assert_array_equal(z[f"T{T}.hs"], R.hidden_states(int(T), R.GOLDEN_CONFIG).numpy())


@pytest.mark.parametrize("T", (2, 3, 9, 23))
def test_restatement_reproduces_the_reference(T):
    z, cfg = _golden(), R.GOLDEN_CONFIG
    P32 = R.filled_state(cfg)
    P64 = R.to_dtype(P32, torch.float64)
    hs = torch.from_numpy(z[f"T{T}.hs"].copy())
    t32, t64 = {}, {}
    t32["emb"] = R.forward(P32, hs, cfg, t32)
    t64["emb"] = R.forward(P64, hs.double(), cfg, t64)
    for name in R.TAPS + ("emb",):
        gold = torch.from_numpy(z[f"T{T}.{name}"].copy())
        assert gold.shape == t32[name].shape, name
        spread = R.rel_l2(gold, t64[name])
        got = R.rel_l2(t32[name], gold)
        print(f"T={T} {name}: restatement-vs-golden {got:.3e}, golden-vs-fp64 {spread:.3e}")
        assert 0 < spread < 1e-4, (name, spread)  # the fixture is an fp32 evaluation of this graph (the cap the fp32 kernels carry), not something else
        assert got <= spread, (name, got, spread)


def _synthetic_checkpoint(cfg):
    sd = R.filled_state(cfg)
    sd["feature_extract.model.encoder.layers.0.foo"] = torch.zeros(3)
    sd["feature_extract.foo"] = torch.zeros(1)
    sd["layer1.bn.num_batches_tracked"] = torch.tensor(7)
    sd["bn.num_batches_tracked"] = torch.tensor(7)
    return sd


def test_from_checkpoint_key_handling(tmp_path):
    cfg = R.GOLDEN_CONFIG
    sd = _synthetic_checkpoint(cfg)
    path = tmp_path / "speaker.pth"
    torch.save({"model": sd}, path)
    enc = SpeakerEncoder.from_checkpoint(str(path), **cfg)
    assert sorted(enc._state) == sorted(R.state_spec(cfg))  # feature_extract.* and num_batches_tracked are gone, nothing else is

    missing = dict(sd)
    del missing["layer3.Res2Conv1dReluBn.bns.4.running_var"]
    with pytest.raises(KeyError, match=r"layer3\.Res2Conv1dReluBn\.bns\.4\.running_var"):
        SpeakerEncoder(**cfg).load_state_dict(missing)

    unknown = dict(sd)
    unknown["layer5.conv.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="layer5.conv.weight"):
        SpeakerEncoder(**cfg).load_state_dict(unknown)

    gca = dict(sd)
    gca["pooling.linear1.weight"] = torch.zeros(cfg["attention_channels"], 3 * cfg["cat_channels"], 1)
    with pytest.raises(ValueError, match="global_context_att"):
        SpeakerEncoder(**cfg).load_state_dict(gca)

    shape = dict(sd)
    shape["linear.weight"] = torch.zeros(cfg["emb_dim"], 7)
    with pytest.raises(ValueError, match="linear.weight"):
        SpeakerEncoder(**cfg).load_state_dict(shape)


def test_python_spec_is_the_restatements_spec():
    for cfg in (R.GOLDEN_CONFIG, R.PRODUCTION_CONFIG):
        assert {k: tuple(v) for k, v in S._spec(cfg).items()} == {k: tuple(v) for k, v in R.state_spec(cfg).items()}
    assert SpeakerEncoder().cfg == R.PRODUCTION_CONFIG


def test_speaker_similarity_argument_errors():
    enc = SpeakerEncoder(**R.GOLDEN_CONFIG)
    wave = torch.zeros(1600)
    with pytest.raises(ValueError, match="feature_extractor"):
        speaker_similarity(enc, [(wave, wave)])
    with pytest.raises(ValueError, match="WavLM itself is not provided"):
        speaker_similarity(enc, [(wave, wave)], feature_extractor=None)
    with pytest.raises(TypeError, match="SpeakerEncoder"):
        speaker_similarity(object(), [(wave, wave)], feature_extractor=lambda w: None)
    with pytest.raises(ValueError, match="non-empty list"):
        speaker_similarity(enc, [], feature_extractor=lambda w: None)
    with pytest.raises(ValueError, match="sample_rate"):
        speaker_similarity(enc, [(wave, wave)], feature_extractor=lambda w: None, sample_rate=0)
    with pytest.raises(ValueError, match="sample_rate"):
        speaker_similarity(enc, [(wave, wave)], feature_extractor=lambda w: None, sample_rate=(16000, 16000, 16000))
    with pytest.raises(RuntimeError, match="no weights"):
        enc.native()


def test_short_and_misshapen_features_are_refused():
    cfg = R.GOLDEN_CONFIG
    enc = SpeakerEncoder(**cfg)
    L, Fd = cfg["layers"], cfg["feat_dim"]
    ok = torch.zeros(L, 5, Fd)
    assert enc.check_features([ok, torch.zeros(L, 2, Fd)]) == [5, 2]
    assert enc.check_features(torch.zeros(L, 3, 4, Fd)) == [4, 4, 4]
    with pytest.raises(ValueError, match="utterance 1 has 1 frame"):
        enc.embed([ok, torch.zeros(L, 1, Fd)])
    with pytest.raises(ValueError, match="at least 2"):
        enc.embed(torch.zeros(L, 2, 1, Fd))
    with pytest.raises(ValueError, match="layers"):
        enc.embed([torch.zeros(L + 1, 5, Fd)])
    with pytest.raises(ValueError, match="feature width"):
        enc.embed([ok, torch.zeros(L, 5, Fd * 2)])
    with pytest.raises(ValueError, match="non-empty list"):
        enc.embed([])
    with pytest.raises(ValueError, match=r"\[L, T, F\]"):
        enc.embed([torch.zeros(5, Fd)])


def test_extractor_output_forms():
    L, T, Fd = 3, 4, 8
    layers = [torch.full((1, T, Fd), float(i)) for i in range(L)]
    want = torch.stack(layers, 0)[:, 0]
    for out in ({"hidden_states": layers}, {"hidden_states": tuple(layers)}, layers, torch.stack(layers, 0), torch.stack(layers, 0)[:, 0]):
        (got,) = S._hidden_states(out, 1)
        assert torch.equal(got, want)
    with pytest.raises(ValueError, match="hidden_states"):
        S._hidden_states({"last_hidden_state": layers[0]}, 1)
    with pytest.raises(ValueError, match="expected"):
        S._hidden_states(torch.zeros(L, 2, T, Fd), 1)
