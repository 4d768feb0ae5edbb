"""The validation-loss loop (eval/validate.validation_loss over CFM.flow_loss) on a fixed set of random-weight F5TTS_Base batches: the two HIP
kernels of csrc/cfm_loss.hip against the same loop with their torch expressions on the device.

    python tools/validate_ab.py [--repeats 5] [--precision bf16] [--out profiles/validation_loss.md]

Both routes run in the same process, alternating, after one warm-up of each (plans and workspaces exist from then on); wall clock around a
whole validation_loss() call, device synchronised before the start (the call ends in a device-to-host copy).  Reported: utterances/s of each
route (median and spread), and -- timed with device events around back-to-back launches at KERNEL_SHAPE, its own warm-up first -- the time
of f5_cfm_noise, f5_cfm_loss and of their torch expressions, with the bytes the algorithm needs (computed below from the shapes) over that
time.  KERNEL_SHAPE is far larger than a validation batch, so that the tensors do not fit the 256 MiB Infinity Cache and a call outlasts the
host's enqueue: at the loop's own batch sizes these kernels take microseconds and the loop's time is the backbone's.  Needs a GPU; nothing here
falls back."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--kernel-iters", type=int, default=50)
ap.add_argument("--precision", default="bf16")
ap.add_argument("--out", default=None, help="write the figures as markdown to this file")
args = ap.parse_args()
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402  (BASE_ARCH, VOCAB, synth_weights: the random initialisation of the benchmark)
from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.eval import validation_loss  # noqa: E402
from eraxvif5tts_amd.model import CFM, DiT  # noqa: E402
from eraxvif5tts_amd.model import cfm as cfm_mod  # noqa: E402

SHAPES = [(8, 1024), (8, 768), (16, 512), (4, 2048), (8, 1024), (16, 512)]  # (utterances, frames) per batch
MEL = 100
KERNEL_SHAPE = (64, 4096)  # the kernels alone: 105 MB per tensor, so the three inputs of the loss pass do not fit the 256 MiB Infinity Cache


def make_batches(seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for B, N in SHAPES:
        lens = torch.linspace(0.6 * N, N, B).long().flip(0)  # ragged; the longest fills the batch
        mel = torch.randn(B, N, MEL, generator=g) * 2 - 3
        mel = torch.where(torch.arange(N)[None, :, None] < lens[:, None, None], mel, torch.zeros(()))
        nt = N // 8
        text = torch.randint(0, bench.VOCAB, (B, nt), generator=g)
        text = torch.where(torch.arange(nt)[None, :] < (lens[:, None] // 8), text, torch.full_like(text, -1))
        out.append((mel.cuda(), text.cuda(), lens.cuda()))
    return out


def torch_noise(x1, x0, time, span8):
    t = time.unsqueeze(-1).unsqueeze(-1)
    return (1 - t) * x0 + t * x1, torch.where(span8.bool()[..., None], torch.zeros_like(x1), x1)


def torch_loss(pred, x1, x0, span8):
    m = span8.bool()
    elem = F.mse_loss(pred, x1 - x0, reduction="none")
    sums = torch.where(m[..., None], elem.double(), torch.zeros((), dtype=torch.float64, device=x1.device)).sum(dim=(1, 2))
    return elem[m].mean(), sums, m.sum(dim=1) * x1.shape[-1]


def event_ms(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    _lib.require_gpu()
    torch.manual_seed(0)  # DiT() draws its non-zero initial weights from the global generator
    model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=MEL, precision=args.precision))
    cfm = CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()
    batches = make_batches()
    utts = sum(b for b, _ in SHAPES)
    native = (cfm_mod._native_noise, cfm_mod._native_loss)

    def run(route):
        cfm_mod._native_noise, cfm_mod._native_loss = native if route == "hip" else (torch_noise, torch_loss)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = validation_loss(cfm, batches, seed=0)
            return time.perf_counter() - t0, r
        finally:
            cfm_mod._native_noise, cfm_mod._native_loss = native

    secs = {"hip": [], "torch": []}
    losses = {}
    for rep in range(-1, args.repeats):  # (-1: the warm-up of each route, not recorded)
        for route in ("hip", "torch"):
            s, r = run(route)
            losses.setdefault(route, r.loss)
            assert r.loss == losses[route], (route, r.loss, losses[route])  # the same bits on every repeat
            if rep >= 0:
                secs[route].append(s)

    # the kernels alone, on the largest batch: bytes the algorithm needs / device time
    B, N = KERNEL_SHAPE
    x1, x0, pred = [torch.randn(B, N, MEL, device="cuda") for _ in range(3)]
    tt = torch.rand(B, device="cuda")
    span8 = (torch.rand(B, N, device="cuda") < 0.85).to(torch.uint8)
    sel = int(span8.sum())
    noise_bytes = 4 * B * N * MEL * 4 + B * N + B * 4                  # x1, x0 in; phi, cond out; span; time
    loss_bytes = 3 * sel * MEL * 4 + 2 * B * N + (B + 1) * 16 + 4    # the selected rows of pred, x1, x0; span twice; sums, counts, loss
    lib = _lib.load()
    phi, cond = torch.empty_like(x1), torch.empty_like(x1)
    work = torch.empty(lib.f5_cfm_loss_workspace(B, N, MEL), device="cuda", dtype=torch.uint8)
    sums, counts = torch.empty(B, device="cuda", dtype=torch.float64), torch.empty(B, device="cuda", dtype=torch.int64)
    loss = torch.empty(1, device="cuda")
    P = _lib.ptr

    def hip_noise():  # the buffers exist: the host does nothing but the call (the kernels' time, not the allocator's)
        _lib.check(lib.f5_cfm_noise(B, N, MEL, P(x1), P(x0), P(tt), P(span8), P(phi), P(cond), _lib.stream_ptr()))

    def hip_loss():
        _lib.check(lib.f5_cfm_loss(B, N, MEL, P(pred), P(x1), P(x0), P(span8), P(sums), P(counts), P(loss), P(work), _lib.stream_ptr()))

    ms = {"f5_cfm_noise": event_ms(hip_noise, args.kernel_iters),
          "f5_cfm_loss": event_ms(hip_loss, args.kernel_iters),
          "torch noise expressions": event_ms(lambda: torch_noise(x1, x0, tt, span8), args.kernel_iters),
          "torch loss expressions": event_ms(lambda: torch_loss(pred, x1, x0, span8), args.kernel_iters)}
    need = {"f5_cfm_noise": noise_bytes, "f5_cfm_loss": loss_bytes, "torch noise expressions": noise_bytes, "torch loss expressions": loss_bytes}

    rate = {k: [utts / s for s in v] for k, v in secs.items()}
    rec = {"device": torch.cuda.get_device_name(0), "precision": args.precision, "shapes": SHAPES, "utterances": utts, "repeats": args.repeats,
           "utterances_per_s": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in rate.items()},
           "loss": losses, "kernel_shape": [B, N, MEL], "selected_rows": sel,
           "kernels": {k: {"ms": round(v, 5), "needed_bytes": need[k], "GB_per_s": round(need[k] / (v * 1e-3) / 1e9, 1)} for k, v in ms.items()}}
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("# Validation loss loop\n\n")
            fh.write("`tools/validate_ab.py`: `eval.validate.validation_loss` over random-weight F5TTS_Base batches, the HIP kernels of\n"
                     "`csrc/cfm_loss.hip` against the same loop with their torch expressions on the device; same process, alternating, one\n"
                     "warm-up of each route.\n\n")
            fh.write(f"- device: {rec['device']}; precision {args.precision}; batches (utterances, frames): {SHAPES}; {utts} utterances per loop; "
                     f"{args.repeats} repeats\n")
            for k, v in rec["utterances_per_s"].items():
                fh.write(f"- {k} route: {v['median']} utterances/s (median; min {v['min']}, max {v['max']})\n")
            fh.write(f"- loss (both routes draw the same spans, noise and times): hip {losses['hip']!r}, torch {losses['torch']!r}\n\n")
            fh.write(f"Kernels alone at {B} x {N} x {MEL} (105 MB per tensor: beyond the Infinity Cache), {sel} of {B * N} rows selected, device "
                     f"events around {args.kernel_iters} back-to-back calls:\n\n")
            fh.write("| | ms per call | bytes the algorithm needs | GB/s |\n|---|---|---|---|\n")
            for k, v in rec["kernels"].items():
                fh.write(f"| {k} | {v['ms']} | {v['needed_bytes']} | {v['GB_per_s']} |\n")


if __name__ == "__main__":
    main()
