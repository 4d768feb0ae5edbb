#!/usr/bin/env python
"""Capture tests/golden/speaker.npz from the reference implementation (development machine only; no GPU, never run by a test).

    python tools/speaker_golden.py /path/to/reference/tree

Loads the reference tree's eval/ecapa_tdnn.py as it stands and builds its ECAPA_TDNN at the small golden config.  The class fetches its feature
extractor through torch.hub.load; for the duration of this script that function returns a stub module instead (one parameter, an empty
``model.encoder.layers``, and a forward that answers ``{"hidden_states": [...]}`` with preset tensors), so nothing is downloaded and the class
runs unmodified.  Every parameter and buffer is overwritten by tests/speaker_ref.fill(name, shape): the fixture stores no weights.  Recorded per
utterance length: the seeded hidden states, the reference's embedding, and (forward hooks) the tensors behind the instance norm, layer1, each
SE block, the wide convolution and the pool.  Only data goes into the fixture."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speaker_ref as R  # noqa: E402

FRAMES = (2, 3, 9, 23)


class _Stub(torch.nn.Module):
    def __init__(self, layers, feat_dim):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.model = torch.nn.Module()
        self.model.encoder = torch.nn.Module()
        self.model.encoder.layers = torch.nn.ModuleList()
        self.layers, self.feat_dim = layers, feat_dim
        self.preset = None

    def forward(self, wavs):
        hs = self.preset if self.preset is not None else torch.zeros(self.layers, 4, self.feat_dim)
        return {"hidden_states": [hs[l].unsqueeze(0) for l in range(hs.shape[0])]}


def load_reference(tree):
    hits = [os.path.join(d, "ecapa_tdnn.py") for d, _, files in os.walk(tree) if "ecapa_tdnn.py" in files and d.endswith("eval")]
    if not hits:
        raise SystemExit(f"no eval/ecapa_tdnn.py under {tree}")
    spec = importlib.util.spec_from_file_location("reference_ecapa_tdnn", hits[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_reference(mod, cfg):
    stub = _Stub(cfg["layers"], cfg["feat_dim"])
    real = torch.hub.load
    torch.hub.load = lambda *a, **k: stub
    try:
        model = mod.ECAPA_TDNN(feat_dim=cfg["feat_dim"], channels=cfg["channels"], emb_dim=cfg["emb_dim"])
    finally:
        torch.hub.load = real
    model.eval()
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.startswith("feature_extract.") or name.endswith("num_batches_tracked"):
                continue
            t.copy_(torch.from_numpy(R.fill(name, tuple(t.shape))))
    return model, stub


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    mod = load_reference(sys.argv[1])
    cfg = R.GOLDEN_CONFIG
    model, stub = build_reference(mod, cfg)
    spec = R.state_spec(cfg)
    own = {n: tuple(t.shape) for n, t in model.state_dict().items() if not n.startswith("feature_extract.") and not n.endswith("num_batches_tracked")}
    assert own == {n: tuple(s) for n, s in spec.items()}, "tests/speaker_ref.state_spec disagrees with the reference's state_dict()"
    assert model.pooling.global_context_att is False

    taps = {}
    hooks = [model.instance_norm.register_forward_hook(lambda m, i, o: taps.__setitem__("instance_norm", o)),
             model.layer1.register_forward_hook(lambda m, i, o: taps.__setitem__("layer1", o)),
             model.layer2.register_forward_hook(lambda m, i, o: taps.__setitem__("layer2", o)),
             model.layer3.register_forward_hook(lambda m, i, o: taps.__setitem__("layer3", o)),
             model.layer4.register_forward_hook(lambda m, i, o: taps.__setitem__("layer4", o)),
             model.conv.register_forward_hook(lambda m, i, o: taps.__setitem__("conv", torch.relu(o))),
             model.pooling.register_forward_hook(lambda m, i, o: taps.__setitem__("pooling", o))]
    out = {"fill_version": np.int64(R.FILL_VERSION), "frames": np.asarray(FRAMES, np.int64),
           "config_keys": np.asarray(sorted(cfg)), "config_values": np.asarray([cfg[k] for k in sorted(cfg)], np.int64)}
    with torch.no_grad():
        for T in FRAMES:
            hs = R.hidden_states(T, cfg)
            stub.preset = hs
            emb = model(torch.zeros(1, 16))
            assert torch.isfinite(emb).all()
            out[f"T{T}.hs"] = hs.numpy()
            out[f"T{T}.emb"] = emb.numpy()
            for name in R.TAPS:
                out[f"T{T}.{name}"] = taps[name].numpy().astype(np.float32)
    for h in hooks:
        h.remove()
    path = os.path.join(ROOT, "tests", "golden", "speaker.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
