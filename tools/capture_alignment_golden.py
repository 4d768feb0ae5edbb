#!/usr/bin/env python
"""Capture tests/golden/alignment.npz from the reference implementation (development machine only; no GPU, never run by a test).

    python tools/capture_alignment_golden.py /path/to/reference/tree

Loads the reference tree's model/alignment_utils.py as it stands -- with stand-in modules for its two phonemizer imports (viphoneme,
phonemizer), which are not needed by the searches -- and records, for every case of tests/alignment_ref.generate_cases(), the similarity
input (or its SHA-256 when it is large: the cases regenerate it) and the 0 / 1 matrices its "viterbi" and "window" functions return, packed
to bits.  Where the reference raises (the window search on an empty window, nt > T) the case has no entry for that algorithm.  Only data
goes into the fixture."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alignment_ref  # noqa: E402


def load_reference(tree):
    hits = [os.path.join(d, "alignment_utils.py") for d, _, files in os.walk(tree) if "alignment_utils.py" in files and d.endswith("model")]
    if not hits:
        raise SystemExit(f"no model/alignment_utils.py under {tree}")
    for name, attr in (("viphoneme", "vi2IPA"), ("phonemizer", "phonemize")):
        stand_in = types.ModuleType(name)
        setattr(stand_in, attr, lambda *a, **k: (_ for _ in ()).throw(RuntimeError(f"{name} is a stand-in")))
        sys.modules.setdefault(name, stand_in)
    spec = importlib.util.spec_from_file_location("reference_alignment_utils", hits[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    out, names = {}, []
    for name, sim in alignment_ref.generate_cases().items():
        names.append(name)
        out[name + ".shape"] = np.array(sim.shape, np.int64)
        if sim.size <= alignment_ref.STORE_LIMIT:
            out[name + ".sim"] = sim
        else:
            out[name + ".sim_sha256"] = alignment_ref.digest(sim)
        for alg in alignment_ref.ALGORITHMS:
            try:
                a = ref.monotonic_alignment_search(torch.from_numpy(sim.copy()), algorithm=alg).numpy()
            except Exception as e:  # noqa: BLE001
                print(f"{name}: {alg} raised {type(e).__name__}: {e}")
                continue
            assert a.shape == sim.shape and np.isin(a, (0.0, 1.0)).all()
            out[f"{name}.{alg}"] = np.packbits(a.astype(np.uint8).reshape(-1))
            print(f"{name}: {alg} durations of utterance 0: {a[0].sum(axis=1)[:12].tolist()}")
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "alignment.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
