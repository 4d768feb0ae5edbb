"""Layer pruning on the host: which blocks to keep, and the checkpoint surgery that keeps them.

``select_blocks`` is the selection rule of the reference's pruner (src/model_pruning/excellent_definitive-f5tts-pruner.py:662-700) over any
scores -- a ``block_scores.json`` the reference wrote from weight histograms, or ``eval.distill.block_ablation``'s measured losses.
``prune_state_dict`` / ``prune_checkpoint`` are its key renumbering (:731-784): the kept ``transformer_blocks.<n>.`` move to their position in
the list, the others go, everything else passes through.  Nothing here runs the model; ``DiT.set_active_blocks`` auditions a choice on the
weights already in HBM before any checkpoint is written.
"""
from __future__ import annotations

import re
from typing import Dict, Iterable, List, Sequence, Tuple

import torch

_BLOCK_KEY = re.compile(r"(^|\.)transformer_blocks\.(\d+)\.")


def check_blocks(blocks, depth=None) -> List[int]:
    """The block list as ints: non-empty, strictly increasing, each in [0, depth) when the depth is known.  ValueError otherwise."""
    out = [int(b) for b in blocks]
    if not out:
        raise ValueError("the block list is empty")
    for i, b in enumerate(out):
        if b < 0 or (depth is not None and b >= depth):
            raise ValueError(f"block {b} is outside [0, {depth if depth is not None else 'depth'})")
        if i and b <= out[i - 1]:
            raise ValueError(f"the block list must be strictly increasing ({b} follows {out[i - 1]})")
    return out


def select_blocks(scores: Sequence[Tuple[int, float]], target_layers: int, blocks: Sequence[int]) -> List[int]:
    """The blocks to keep, by the reference's rule (pruner.py:662-700), case for case.  ``blocks``: the model's block indices in order;
    ``scores``: ``(block, score)`` pairs, higher = keep (ranked by descending score, ties in list order: a stable sort, as the reference's).
      target >= len(blocks)  all of them
      target <= 0            none
      target <= 4            the first ``target`` blocks
      fewer than 4 blocks    the ``target`` best by score
      otherwise              the first two and the last two, then the best of the middle until ``target`` are kept
    The result is sorted."""
    blocks = list(blocks)
    target = int(target_layers)
    ranked = sorted(((int(b), float(s)) for b, s in scores), key=lambda bs: bs[1], reverse=True)  # (stable: equal scores keep their order)
    if target >= len(blocks):
        return sorted(blocks)
    if target <= 0:
        return []
    if target <= 4:
        return sorted(blocks[:target])
    if len(blocks) < 4:  # (unreachable after the cases above, kept as the reference has it)
        return sorted(b for b, _ in ranked[:target])
    must_keep = sorted({blocks[0], blocks[1], blocks[-2], blocks[-1]})
    middle = [b for b, _ in ranked if b not in must_keep]
    count = target - len(must_keep)
    if count < 0:
        return must_keep[:target]
    return sorted(must_keep + middle[:count])


def prune_state_dict(state_dict: Dict[str, torch.Tensor], blocks: Iterable[int]) -> Dict[str, torch.Tensor]:
    """The state dict of the model that keeps ``blocks`` (pruner.py:731-784): a key with a component ``transformer_blocks.<n>.`` is dropped
    when block n is not kept and renumbered to n's position in ``blocks`` when it is -- at any prefix (``transformer.``, ``ema_model.``, none);
    ``text_embed.text_blocks.*`` and every other entry pass through.  The tensors are the same objects: nothing is copied."""
    blocks = check_blocks(blocks)
    new_index = {old: new for new, old in enumerate(blocks)}
    out = {}
    for key, value in state_dict.items():
        m = _BLOCK_KEY.search(key)
        if m is None:
            out[key] = value
            continue
        old = int(m.group(2))
        if old in new_index:
            out[key[:m.start(2)] + str(new_index[old]) + key[m.end(2):]] = value
    return out


def _is_state_dict(d) -> bool:
    return isinstance(d, dict) and any(torch.is_tensor(v) for v in d.values())


def prune_checkpoint(src: str, dst: str, blocks: Iterable[int]) -> List[str]:
    """Write the checkpoint ``src`` (``.pt`` or ``.safetensors``, read as ``infer.utils_infer.load_checkpoint`` reads them) with only
    ``blocks`` kept, into the same container at ``dst``.  ``prune_state_dict`` is applied to ``ema_model_state_dict`` and ``model_state_dict``
    where the file has them, or to the file's flat dict; ``initted``, ``step`` and every other entry stay.  Returns the names of the
    dictionaries it pruned.  The result loads into a model of depth ``len(blocks)``, here and in the reference."""
    blocks = check_blocks(blocks)
    kind_src, kind_dst = src.split(".")[-1], dst.split(".")[-1]
    if (kind_src == "safetensors") != (kind_dst == "safetensors"):
        raise ValueError(f"prune_checkpoint keeps the container: {src!r} -> {dst!r} changes it")
    if kind_src == "safetensors":
        from safetensors.torch import load_file, save_file
        save_file(prune_state_dict(load_file(src, device="cpu"), blocks), dst)
        return ["<flat>"]
    checkpoint = torch.load(src, map_location="cpu", weights_only=True)
    pruned = []
    if isinstance(checkpoint, dict) and any(_is_state_dict(checkpoint.get(k)) for k in ("ema_model_state_dict", "model_state_dict")):
        checkpoint = dict(checkpoint)
        for name in ("ema_model_state_dict", "model_state_dict"):
            if _is_state_dict(checkpoint.get(name)):
                checkpoint[name] = prune_state_dict(checkpoint[name], blocks)
                pruned.append(name)
    else:
        checkpoint = prune_state_dict(checkpoint, blocks)
        pruned.append("<flat>")
    torch.save(checkpoint, dst)
    return pruned
