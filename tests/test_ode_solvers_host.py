"""The Runge-Kutta members of torchdiffeq's fixed-grid family (rk4 = rk4_alt_step_func, heun2, heun3) on the host: CFM.sample over a CPU
backbone against an independent restatement of the step functions, their convergence order on a linear ODE, the methods that stay refused,
the C ABI declaration, and the solver table's time grid (csrc/ode_methods.h, compiled with g++) against the per-method rules.  No GPU needed; tests/test_gpu_ode_solvers.py runs the same methods on the fused sampler."""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import golden_arch, golden_weights, load_golden, rel_l2
from oracle import cpu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_METHODS = ("rk4", "heun2", "heun3")


def restated_step(method, f, t0, t1, y):
    """y1 of one fixed-grid step, written out stage by stage in torchdiffeq's fp32 operation order (the spec of the new solvers)."""
    dt = t1 - t0
    if method == "rk4":
        k1 = f(t0, y)
        k2 = f(t0 + dt * (1 / 3), y + dt * k1 * (1 / 3))
        k3 = f(t0 + dt * (2 / 3), y + dt * (k2 - k1 * (1 / 3)))
        k4 = f(t1, y + dt * (k1 - k2 + k3))
        dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
    elif method == "heun2":
        k1 = f(t0, y)
        k2 = f(t0 + dt, y + dt * k1)
        dy = dt * (k1 * 0.5 + k2 * 0.5)
    elif method == "heun3":
        k1 = f(t0, y)
        k2 = f(t0 + dt * (1 / 3), y + dt * k1 * (1 / 3))
        k3 = f(t0 + dt * (2 / 3), y + dt * k2 * (2 / 3))
        dy = dt * (k1 * 0.25 + k3 * 0.75)
    else:
        raise AssertionError(method)
    return y + dy


def oracle_sample(W, arch, cond, text, duration, lens, steps, cfg_strength, sway, y0, method, edit_mask=None):
    """cfm.py:82-208 over the CPU oracle's forward with explicit y0 and the restated step: (out, trajectory [steps + 1, B, N, mel])."""
    cond = cond.float()
    b, nc, _ = cond.shape
    cond_mask = cpu_ref.lens_to_mask(lens)
    if edit_mask is not None:
        cond_mask = cond_mask & edit_mask
    duration = torch.maximum(torch.maximum((text != -1).sum(dim=-1), lens) + 1, duration)
    N = int(duration.max())
    cond = F.pad(cond, (0, 0, 0, N - nc))
    cond_mask = F.pad(cond_mask, (0, N - cond_mask.shape[-1]), value=False)[..., None]
    step_cond = torch.where(cond_mask, cond, torch.zeros_like(cond))
    mask = cpu_ref.lens_to_mask(duration) if b > 1 else None
    fwd = {"UNetT": cpu_ref.unett_forward, "MMDiT": cpu_ref.mmdit_forward}.get(arch.get("backbone"), cpu_ref.dit_forward)

    def f(t, x):
        pred = fwd(W, arch, x, step_cond, text, t, False, False, mask=mask)
        if cfg_strength < 1e-5:
            return pred
        null = fwd(W, arch, x, step_cond, text, t, True, True, mask=mask)
        return pred + (pred - null) * cfg_strength

    t = cpu_ref.time_grid(steps, sway)
    y, traj = y0.float(), [y0.float()]
    for t0, t1 in zip(t[:-1], t[1:]):
        y = restated_step(method, f, t0, t1, y)
        traj.append(y)
    return torch.where(cond_mask, cond, y), torch.stack(traj)


class _CpuBackbone(torch.nn.Module):
    """A non-native backbone (no native_sample): CFM.sample drives its ODE loop from Python over the oracle's DiT forward."""

    def __init__(self, W, arch):
        super().__init__()
        self.W, self.arch, self.dim = W, arch, arch["dim"]
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x, cond, text, time, drop_audio_cond, drop_text, mask=None, cache=False):
        return cpu_ref.dit_forward(self.W, self.arch, x, cond, text, time, drop_audio_cond, drop_text, mask=mask)

    def clear_cache(self):
        pass


@pytest.mark.parametrize("method", RK_METHODS)
def test_cfm_python_driver_matches_the_restated_solver(method):
    """tiny_base weights, B = 2 (key mask on: durations 56 / 44), CFG 2, sway -1, explicit y0: CFM.sample's output and trajectory against
    the restatement, rel-L2 < 2e-5."""
    from eraxvif5tts_amd.model import CFM
    z = load_golden("tiny_base")
    arch, W = golden_arch(z), golden_weights(z)
    c = CFM(transformer=_CpuBackbone(W, arch), mel_spec_kwargs={"mel_spec_type": "vocos"}, odeint_kwargs={"method": method})
    g = lambda k: torch.from_numpy(z[k])
    steps = 3
    out, traj = c.sample(cond=g("cond"), text=g("text"), duration=g("duration"), lens=g("lens"), steps=steps, cfg_strength=2.0,
                         sway_sampling_coef=-1.0, y0=g("y0"))
    ref, ref_traj = oracle_sample(W, arch, g("cond"), g("text"), g("duration"), g("lens"), steps, 2.0, -1.0, g("y0"), method)
    assert traj.shape == (steps + 1, 2, 56, 100) and torch.isfinite(out).all()
    assert rel_l2(out, ref) < 2e-5 and rel_l2(traj, ref_traj) < 2e-5
    # the solvers differ from each other (and from euler at the same grid): the method is really the one asked for
    other, _ = oracle_sample(W, arch, g("cond"), g("text"), g("duration"), g("lens"), steps, 2.0, -1.0, g("y0"), "heun2" if method != "heun2" else "rk4")
    assert rel_l2(out, other) > 1e-4


@pytest.mark.parametrize("method,order", [("rk4", 4), ("heun3", 3), ("heun2", 2)])
def test_step_functions_converge_at_their_order(method, order):
    """dy/dt = lam * y, y(0) = 1 on [0, 1] in float64 through the step function CFM._sample_python uses: halving dt divides the global error
    by 2^order (measured ratio within [0.7, 1.4] x 2^order)."""
    from eraxvif5tts_amd.model.cfm import ODE_METHODS
    lam = -1.3
    exact = math.exp(lam)

    def err(steps):
        t = torch.linspace(0, 1, steps + 1, dtype=torch.float64)
        y = torch.ones(1, dtype=torch.float64)
        for t0, t1 in zip(t[:-1], t[1:]):
            y = y + ODE_METHODS[method](lambda tt, x: lam * x, t0, t1, y)
        return abs(float(y) - exact)

    e1, e2, e3 = err(8), err(16), err(32)
    for a, b in ((e1, e2), (e2, e3)):
        assert 0.7 * 2 ** order <= a / b <= 1.4 * 2 ** order, (method, e1, e2, e3)


def test_step_functions_are_the_restated_ones():
    """On a nonlinear time-dependent field the package's step functions give the restatement bit for bit (same fp32 operation order)."""
    from eraxvif5tts_amd.model.cfm import ODE_METHODS
    g = torch.Generator().manual_seed(3)
    y = torch.randn(4, 100, generator=g)
    f = lambda t, x: torch.sin(3 * x) * (1 + t) - 0.7 * x
    t0, t1 = torch.tensor(0.125), torch.tensor(0.4375)
    for m in RK_METHODS:
        assert torch.equal(y + ODE_METHODS[m](f, t0, t1, y), restated_step(m, f, t0, t1, y)), m


@pytest.mark.parametrize("kwargs", [{"method": "dopri5"}, {"method": "explicit_adams"}, {"method": "bosh3"},
                                    {"method": "rk4", "options": {"step_size": 0.1}}, {"method": "euler", "perturb": True}])
def test_unsupported_solvers_raise_before_any_work(kwargs):
    from eraxvif5tts_amd.model import CFM
    z = load_golden("tiny_base")
    bb = _CpuBackbone(golden_weights(z), golden_arch(z))
    calls = []
    bb.forward = lambda *a, **k: calls.append(1)
    c = CFM(transformer=bb, mel_spec_kwargs={"mel_spec_type": "vocos"}, odeint_kwargs=kwargs)
    with pytest.raises(ValueError, match="heun3"):  # the message names the supported set
        c.sample(cond=torch.from_numpy(z["cond"]), text=torch.from_numpy(z["text"]), duration=torch.from_numpy(z["duration"]),
                 lens=torch.from_numpy(z["lens"]), steps=2, cfg_strength=2.0, y0=torch.from_numpy(z["y0"]))
    assert not calls


def test_unsupported_solver_raises_on_the_native_path_before_the_library():
    """DiT.native_sample / native_sample_ragged refuse an unknown method name with ValueError (not KeyError) before any library call."""
    from eraxvif5tts_amd.model import DiT
    m = DiT(dim=128, depth=1, heads=2, ff_mult=2, text_dim=64, conv_layers=1, text_num_embeds=10, mel_dim=100)
    x = torch.zeros(1, 8, 100)
    with pytest.raises(ValueError, match="rk4"):
        m.native_sample(x, torch.zeros(1, 4, dtype=torch.long), torch.tensor([4]), torch.tensor([8]), x, torch.linspace(0, 1, 3), 2, 2.0,
                        method="dopri5")
    with pytest.raises(ValueError, match="rk4"):
        m.native_sample_ragged(x[0], torch.zeros(1, 4, dtype=torch.long), torch.tensor([4]), [8], x[0], torch.linspace(0, 1, 3), 2, 2.0,
                               method="adaptive_heun")


def test_rk_solvers_are_declared_and_exported():
    from eraxvif5tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    for name, code in (("RK4", 2), ("HEUN2", 3), ("HEUN3", 4)):
        assert re.search(rf"#define F5_ODE_{name} {code}\b", header), name
    assert re.search(r"F5_API int f5_ode_evals_per_step\(int ode_method\);", header)
    assert "f5_ode_evals_per_step" in _lib.EXPORTS
    assert (_lib.F5_ODE_RK4, _lib.F5_ODE_HEUN2, _lib.F5_ODE_HEUN3) == (2, 3, 4)
    lib = _lib.load(build_if_missing=True)
    # the table is the library's (no device needed): Python sizes plans from it
    assert [lib.f5_ode_evals_per_step(_lib.ODE_METHODS[m]) for m in ("euler", "midpoint", "rk4", "heun2", "heun3")] == [1, 2, 4, 2, 3]
    assert lib.f5_ode_evals_per_step(5) == -1 and lib.f5_ode_evals_per_step(-1) == -1  # F5_EINVAL
    nm = shutil.which("nm")
    if nm:
        syms = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT f5_ode_evals_per_step$", syms, re.M)


_GRID_PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "ode_methods.h"
/* stdin: "method steps" and the steps + 1 grid words in hex, per case; stdout: the tv words, then the cf words of the case */
int main() {
    int method, steps;
    while (scanf("%d %d", &method, &steps) == 2) {
        const OdeMethod* om = ode_method_of(method);
        if (!om) return 2;
        std::vector<float> grid(steps + 1), tv(om->evals * steps), cf(om->evals * steps);
        for (float& g : grid) {
            uint32_t w;
            if (scanf("%x", &w) != 1) return 3;
            memcpy(&g, &w, 4);
        }
        ode_time_grid(*om, grid.data(), steps, tv.data(), cf.data());
        for (const std::vector<float>* v : {&tv, &cf}) {
            for (float f : *v) {
                uint32_t w;
                memcpy(&w, &f, 4);
                printf("%08x ", w);
            }
            printf("\n");
        }
    }
    return ode_method_of(5) || ode_method_of(-1);
}
"""


def _restated_grid(method, t):
    """(tv, cf) of the float32 grid `t`: the evaluation times and step coefficients of torchdiffeq's fixed-grid rules, one float32 rounding per
    operation (numpy float32 scalars), written out per method."""
    import numpy as np
    f = np.float32
    third, two_thirds, half = f(1 / 3), f(2 / 3), f(0.5)
    tv, cf = [], []
    for t0, t1 in zip(t[:-1], t[1:]):
        dt = t1 - t0
        if method == "euler":
            tv += [t0]
            cf += [dt]
        elif method == "midpoint":
            tv += [t0, t0 + dt * half]
            cf += [half * dt, dt]
        elif method == "rk4":
            tv += [t0, t0 + dt * third, t0 + dt * two_thirds, t1]
            cf += [dt] * 4
        elif method == "heun2":
            tv += [t0, t0 + dt]
            cf += [dt] * 2
        else:
            tv += [t0, t0 + dt * third, t0 + dt * two_thirds]
            cf += [dt] * 3
    assert all(type(v) is np.float32 for v in tv + cf)
    return np.array(tv, dtype=f), np.array(cf, dtype=f)


def test_time_grid_header_compiled_with_gxx_equals_the_restated_rules(tmp_path):
    """csrc/ode_methods.h is plain host C++ (g++ -Wall -Werror, contraction off) and its table-driven ode_time_grid gives, bit for bit, the
    evaluation times and coefficient words of the per-method rules: five methods x steps 1, 2, 7, 32 x the linear grid and the grid swayed with -1."""
    import numpy as np
    from eraxvif5tts_amd import _lib
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed: ode_methods.h must compile as plain host C++"
    src, exe = tmp_path / "ode_grid.cpp", tmp_path / "ode_grid"
    src.write_text(_GRID_PROGRAM)
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "eraxvif5tts_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    cases, lines = [], []
    for method in ("euler", "midpoint", "rk4", "heun2", "heun3"):
        for steps in (1, 2, 7, 32):
            for sway in (None, -1.0):
                t = cpu_ref.time_grid(steps, sway).float().numpy()
                assert t.dtype == np.float32 and t.shape == (steps + 1,)
                cases.append((method, steps, sway, t))
                lines.append(f"{_lib.ODE_METHODS[method]} {steps} " + " ".join(f"{int(w):08x}" for w in t.view(np.uint32)))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
    assert len(out) == 2 * len(cases) + 1
    words = 0
    for i, (method, steps, sway, t) in enumerate(cases):
        tv, cf = _restated_grid(method, t)
        for name, want, line in (("tv", tv, out[2 * i]), ("cf", cf, out[2 * i + 1])):
            got = np.array([int(w, 16) for w in line.split()], dtype=np.uint32)
            assert got.shape == want.shape and (got == want.view(np.uint32)).all(), (method, steps, sway, name)
            words += got.size
    assert words == 2 * 2 * (1 + 2 + 4 + 2 + 3) * (1 + 2 + 7 + 32)
