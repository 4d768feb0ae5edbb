"""How often the two range guards of attn_wide_kernel's reference-free build fire over one C2 sample() (32 x 1024 frames, CFG, NFE 32).

The counters exist only in a diagnostic build of attention_fast.hip (-DF5_ATTN_GUARD_COUNT), never in the shipped kernel:
  B=eraxvif5tts_amd/build
  hipcc <build.py's FLAGS> -fno-slp-vectorize -DF5_ATTN_GUARD_COUNT -c eraxvif5tts_amd/csrc/attention_fast.hip -o $B/guardcount/attention_fast.o
  hipcc -shared -fPIC --offload-arch=gfx950 $B/[!a]*.o $B/attention.o $B/attention_pipe.o $B/guardcount/attention_fast.o \
        -o eraxvif5tts_amd/lib/libf5hip_guardcount.so        # every object of the normal build but attention_fast.o
  F5HIP_LIB=eraxvif5tts_amd/lib/libf5hip_guardcount.so python tools/attn_guard_count.py
"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from eraxvif5tts_amd import _lib  # noqa: E402
from eraxvif5tts_amd.model import CFM, DiT  # noqa: E402

lib = _lib.load()
_lib.require_gpu()
B, N = bench.WORKLOADS["C2"]
cond, text, lens, dur = bench.synth_batch(B, N, "cuda", seed=0)
torch.manual_seed(1234)
model = bench.synth_weights(DiT(**bench.BASE_ARCH, text_num_embeds=bench.VOCAB, mel_dim=100, precision="bf16"), seed=0)
cfm = CFM(transformer=model, mel_spec_kwargs={"mel_spec_type": "vocos"}).cuda()
y0 = torch.randn(B, N, 100, generator=torch.Generator().manual_seed(1))
cnt = (C.c_uint * 3)()
assert lib.f5_debug_attn_guard_counts(cnt, 1) == 0
out, _ = cfm.sample(cond=cond, text=text, duration=dur, lens=lens, steps=32, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, use_graph=False)
torch.cuda.synchronize()
assert lib.f5_debug_attn_guard_counts(cnt, 0) == 0
print(f"C2 sample(): reference-free items {cnt[0]}, high-side trips (waves) {cnt[1]}, low-side re-runs (workgroups) {cnt[2]}; "
      f"output finite: {bool(torch.isfinite(out).all())}")
