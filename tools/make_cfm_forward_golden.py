"""Generate tests/golden/cfm_forward.npz: the REFERENCE's CFM.forward (cfm.py:210-283) on CPU over the oracle backbone.

Run by hand where the reference tree is present:  python tools/make_cfm_forward_golden.py
The reference's own cfm.py / utils.py are imported unmodified through oracle/ref_import.py; the backbone behind plug point A is the CPU oracle
(oracle/cpu_ref.dit_forward) on the tiny_base network, whose weights tests/golden/tiny_base.npz already holds (they are not stored again).
Only data is written: inputs, seeds, and per seed the reference's loss, cond, pred, span mask and drop flags; and mask_from_frac_lengths
(utils.py:58-66) on stated fractions, both ends of CFM's default (0.7, 1.0) included.
"""
from __future__ import annotations

import importlib
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import cpu_ref  # noqa: E402
import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)  # kept when they add a new (drop_audio_cond, drop_text) pair, or are the first two


class OracleBackbone(torch.nn.Module):
    """plug point A over the CPU oracle (as tests/test_host_logic.py wraps it); records the flags the reference called it with."""

    def __init__(self, W, cfg):
        super().__init__()
        self.W, self.cfg, self.dim = W, cfg, cfg["dim"]
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.flags = None

    def forward(self, x, cond, text, time, drop_audio_cond, drop_text, mask=None, cache=False):
        assert mask is None and cache is False
        self.flags = (bool(drop_audio_cond), bool(drop_text))
        return cpu_ref.dit_forward(self.W, self.cfg, x, cond, text, time, drop_audio_cond, drop_text, mask=mask)


def main():
    _, _, cfm_mod = ref_import.load_reference()
    utils = importlib.import_module("f5_tts.model.utils")
    z = np.load(os.path.join(GOLDEN, "tiny_base.npz"), allow_pickle=False)

    def conv(v):
        return None if v == "None" else (v == "True" if v in ("True", "False") else int(v))
    cfg = {str(k): conv(str(v)) for k, v in zip(z["arch_keys"], z["arch_vals"])}
    W = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("W.")}
    bb = OracleBackbone(W, cfg)
    c = cfm_mod.CFM(transformer=bb, mel_spec_kwargs={"mel_spec_type": "vocos"})

    g = torch.Generator().manual_seed(4242)
    B, N, V = 3, 29, int(z["vocab"])
    lens = torch.tensor([29, 22, 17])  # ragged; the longest fills the batch, as a padded bucket does
    mel = torch.randn(B, N, 100, generator=g) * 2 - 3
    mel = torch.where(torch.arange(N)[None, :, None] < lens[:, None, None], mel, torch.zeros(()))
    text = torch.randint(0, V, (B, 12), generator=g)
    text[1, 9:] = -1
    text[2, 7:] = -1
    d = {"mel": mel, "text": text, "lens": lens}
    kept, pairs = [], set()
    for s in SEEDS:
        torch.manual_seed(s)
        random.seed(s)
        with torch.no_grad():
            loss, cond, pred = c(mel, text, lens=lens)
        if len(kept) >= 2 and bb.flags in pairs:
            continue
        pairs.add(bb.flags)
        kept.append(s)
        span = (cond == 0).all(dim=-1) & (torch.arange(N)[None, :] < lens[:, None])  # cfm.py:263: the span rows of cond are exactly zero
        d.update({f"s{s}.loss": loss, f"s{s}.cond": cond, f"s{s}.pred": pred, f"s{s}.span": span,
                  f"s{s}.flags": np.array(bb.flags)})
        print("seed", s, "flags", bb.flags, "loss", float(loss), "span rows", span.sum(dim=1).tolist())
    assert {(False, False), (True, True)} <= pairs, pairs  # both branches of cfm.py:267-271
    d["seeds"] = np.array(kept)

    # mask_from_frac_lengths alone: truncations at both ends of (0.7, 1.0) and in between, one rand_like draw after the seed
    seq_len = torch.tensor([29, 22, 17, 10, 1, 29])
    frac = torch.tensor([0.7, 1.0, 0.7, 1.0, 0.7, 0.85])
    d["frac.seq_len"], d["frac.frac"] = seq_len, frac
    for s in (0, 1, 2):
        torch.manual_seed(s)
        d[f"frac.mask{s}"] = utils.mask_from_frac_lengths(seq_len, frac)
        d[f"frac.next{s}"] = torch.rand(4)  # the generator's position behind the call: exactly one draw of frac's shape was made
    np.savez_compressed(os.path.join(GOLDEN, "cfm_forward.npz"),
                        **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in d.items()})
    print("cfm_forward.npz seeds", kept)


if __name__ == "__main__":
    main()
