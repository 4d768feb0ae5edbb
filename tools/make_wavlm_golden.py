"""Writes tests/golden/wavlm_tiny.npz: a seeded, tiny ``transformers.WavLMModel`` (about 125 k parameters) in wavlm-large's form
(feat_extract_norm="layer", do_stable_layer_norm=True), three waves and the model's own fp64 hidden states.  The pin of tests/wavlm_ref.py and,
through it, of the device extractor (eraxvif5tts_amd/eval/wavlm.py) -- the tests themselves need no transformers.

    python tools/make_wavlm_golden.py [--check]

EVERY parameter is perturbed after the model's own init: as initialised, the biases are zero and gru_rel_pos_const is one, and a mistake in
either would be invisible.  The waves give 2, 37 and 130 frames: exact buckets only, the logarithmic buckets, and the clamped last bucket
(32 buckets, max distance 64).  One thread, fixed zip timestamps: the file regenerates bit for bit (--check compares instead of writing)."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "wavlm_tiny.npz")
SAMPLES = (50, 760, 2620)
CONFIG = dict(hidden_size=64, num_hidden_layers=3, num_attention_heads=4, intermediate_size=128, conv_dim=(32, 32, 32), conv_kernel=(10, 3, 2),
              conv_stride=(5, 2, 2), num_feat_extract_layers=3, conv_bias=False, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4,
              num_buckets=32, max_bucket_distance=64, feat_extract_norm="layer", do_stable_layer_norm=True, layer_norm_eps=1e-5,
              hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0,
              mask_time_prob=0.0, mask_feature_prob=0.0)


def build():
    from transformers import WavLMConfig, WavLMModel
    torch.set_num_threads(1)
    torch.manual_seed(20240607)
    model = WavLMModel(WavLMConfig(**CONFIG)).eval()
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.05)
    out = {"state." + k: v.detach().numpy().copy() for k, v in model.state_dict().items() if k != "masked_spec_embed"}
    waves = [torch.randn(n, generator=g) * 0.3 for n in SAMPLES]
    m64 = model.double()
    for i, w in enumerate(waves):
        with torch.no_grad():
            hs = m64(w.double()[None], output_hidden_states=True).hidden_states
        out[f"wave{i}"] = w.numpy()
        out[f"hs{i}"] = torch.stack([h[0] for h in hs]).numpy()  # [L, T, hidden] fp64, the last entry behind the encoder's LayerNorm
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    arrays = build()
    if "--check" in sys.argv:
        tmp = io.BytesIO()
        write_npz(tmp, arrays)
        same = tmp.getvalue() == open(PATH, "rb").read()
        print("identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    write_npz(PATH, arrays)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes, {sum(a.size for k, a in arrays.items() if k.startswith('state.'))} parameters")


if __name__ == "__main__":
    main()
