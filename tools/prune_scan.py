"""The block ablation scan (eval/distill.block_ablation) on F5TTS_Base with random weights: every one of the 22 blocks removed in turn through
DiT.set_active_blocks, the loss against the full model on one batch of 8 utterances x 1024 frames.

    python tools/prune_scan.py [--precision bf16] [--target 14] [--out profiles/prune_scan.txt]

One scan is 1 + 22 backbone evaluations of the batch (the teacher's prediction is computed once) and 22 loss passes; it is timed ONCE, wall
clock, device synchronised before the start (the call ends in its one device-to-host copy), after one warm-up call on a single block so that the
plan and the workspaces exist.  Printed: the time, per block the distillation loss and the student's flow-matching loss, and the blocks
eval.prune.select_blocks keeps for --target.  Random weights: the scores say nothing about a trained model; the run shows the cost of a scan
and that it is reproducible.  Needs a GPU; nothing here falls back."""
import argparse
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--precision", default="bf16")
ap.add_argument("--target", type=int, default=14)
ap.add_argument("--out", default=None, help="write the figures to this file")
ap.add_argument("--build", default=None, help="name of the build measured (default: the short hash of HEAD, where git can tell)")
args = ap.parse_args()
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (BASE_ARCH, VOCAB, synth_weights: the random initialisation of the benchmark)
from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.eval import block_ablation, select_blocks  # noqa: E402
from eraxvif5tts_amd.model import CFM, DiT  # noqa: E402

B, N, MEL = 8, 1024, 100


def make_batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = torch.linspace(0.6 * N, N, B).long().flip(0)  # ragged; the longest fills the batch
    mel = torch.randn(B, N, MEL, generator=g) * 2 - 3
    mel = torch.where(torch.arange(N)[None, :, None] < lens[:, None, None], mel, torch.zeros(()))
    nt = N // 8
    text = torch.randint(0, bench.VOCAB, (B, nt), generator=g)
    text = torch.where(torch.arange(nt)[None, :] < (lens[:, None] // 8), text, torch.full_like(text, -1))
    return mel.cuda(), text.cuda(), lens.cuda()


def main():
    device = _lib.require_gpu()
    torch.manual_seed(0)  # DiT() draws its non-zero initial weights from the global generator
    model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=MEL, precision=args.precision))
    cfm = CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()
    batches = [make_batch()]
    block_ablation(cfm, batches, blocks=[0], seed=0)  # warm-up: weights in HBM, the plan, the workspaces
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scan = block_ablation(cfm, batches, seed=0)
    secs = time.perf_counter() - t0
    again = block_ablation(cfm, batches, blocks=[0, 21], seed=0)
    assert again[0][1].sums.equal(scan[0][1].sums) and again[1][1].sums.equal(scan[21][1].sums)  # the same bits on a second run
    keep = select_blocks([(b, r.distill) for b, r in scan], args.target, range(model.depth))
    build = args.build
    try:
        build = build or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        build = "unknown"
    lines = ["Block ablation scan, F5TTS_Base (22 blocks), random weights (bench.synth_weights, seed 0), one batch of 8 x 1024 frames.",
             f"Produced by `python tools/prune_scan.py --precision {args.precision} --target {args.target}` on one {device}; libf5hip "
             f"{_lib.load().f5_version()}, built from the working tree on top of commit {build}.",
             "Measured ONCE: a single wall-clock reading, no repeats, no spread -- a size, not a benchmark.  Nothing is asserted on it.",
             "",
             f"scan of {model.depth} blocks: {secs:.3f} s  ({1 + model.depth} backbone evaluations of the batch, {model.depth} loss passes, "
             f"{model.depth + 1} changes of the block subset)",
             "",
             "block  distill (sum (student - teacher)^2 / frames)  student flow loss  teacher flow loss"]
    for b, r in scan:
        lines.append(f"{b:5d}  {r.distill:.9e}  {r.student_flow:.9e}  {r.teacher_flow:.9e}")
    lines += ["", f"select_blocks(target = {args.target}): {keep}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
