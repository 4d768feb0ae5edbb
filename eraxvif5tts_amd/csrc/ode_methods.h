// ode_methods.h -- torchdiffeq's fixed-grid solver family as one table, and the time grid of a call.  Plain host C++ (no HIP): the host test
// compiles it with g++ (tests/test_ode_solvers_host.py).
//
// The method is chosen by odeint_kwargs["method"] (cfm.py:197); ODE_METHODS is indexed by the F5_ODE_* constants of include/f5hip.h.  Evaluation
// j of step s has the evaluation index evals * s + j (its AdaLN rows, fold-table entry and coefficient word) and runs at t0 + c[j] * dt in
// fp32, as torchdiffeq computes it; rk4's last evaluation is at t1 itself.  Its coefficient word is h[j] * dt.  After every evaluation one
// update kernel runs (sampler.hip: sample_steps), writing the next evaluation's input or, after the last one, y1:
//   rk_stage false  launch_cfg_step: y0 + (h[j] dt) f                                        (Euler, midpoint)
//   rk_stage true   launch_rk_stage with stage[j]: the slopes it combines, and the slot its own slope is kept in (slot[j], -1: not needed later)
// The two kernels round differently (the stage kernel forms one FMA chain, the step kernel two operations), so a method keeps the one it has.
// The combinations restate torchdiffeq's step functions (heun2 / heun3 tableaux, rk4 = rk4_alt_step_func, the 3/8 rule):
//   rk4    x2 = y0 + dt k1 (1/3)    x3 = y0 + dt (k2 - k1 (1/3))    x4 = y0 + dt (k1 - k2 + k3)    y1 = y0 + dt (k1 + 3 k2 + 3 k3 + k4) / 8
//   heun2  x2 = y0 + dt k1                                                                        y1 = y0 + dt (k1 / 2 + k2 / 2)
//   heun3  x2 = y0 + dt k1 (1/3)    x3 = y0 + dt k2 (2/3)                                         y1 = y0 + dt (k1 / 4 + 3 k3 / 4)
// (the kernel forms each of them as one FMA chain; torchdiffeq's rk4 groups the last one as (k1 + 3 (k2 + k3) + k4) * dt * 0.125).
// Slope slots live in the tail of the trajectory buffer, past its steps + 1 states: a method with E evaluations per step keeps at most
// E - 1 slopes, and E * steps <= max_evals with steps >= 1 gives steps + 1 + (E - 1) <= max_evals + 1 states, which is what the buffer holds.
#pragma once

// One stage of an explicit Runge-Kutta step (kernels.h: launch_rk_stage):
//   out = y0 + (dt * (wk[0] k_0 + .. + wk[nk-1] k_{nk-1} + wf f)) * post
struct RkStage {
    float wk[3];
    float wf, post;
    int nk;
};

struct OdeMethod {
    int evals;       // network evaluations per step
    float c[4];      // evaluation times t0 + c[j] * dt
    float h[4];      // coefficient words h[j] * dt
    bool last_at_t1; // the last evaluation runs at t1 (rk4_alt_step_func: k4 = f(t1, ...))
    bool rk_stage;   // the update kernel behind an evaluation: launch_rk_stage (true) or launch_cfg_step (false)
    RkStage stage[4];
    int slot[4];
};
inline constexpr float ODE_THIRD = 1.0f / 3.0f, ODE_TWO_THIRDS = 2.0f / 3.0f;
inline const OdeMethod ODE_METHODS[] = {
    /* F5_ODE_EULER */ {1, {0.f}, {1.f}, false, false, {}, {-1, -1, -1, -1}},
    /* F5_ODE_MIDPOINT */ {2, {0.f, 0.5f}, {0.5f, 1.f}, false, false, {}, {-1, -1, -1, -1}},
    /* F5_ODE_RK4 */
    {4, {0.f, ODE_THIRD, ODE_TWO_THIRDS, 1.f}, {1.f, 1.f, 1.f, 1.f}, true, true,
     {{{0.f, 0.f, 0.f}, 1.f, ODE_THIRD, 0}, {{-ODE_THIRD, 0.f, 0.f}, 1.f, 1.f, 1}, {{1.f, -1.f, 0.f}, 1.f, 1.f, 2}, {{1.f, 3.f, 3.f}, 1.f, 0.125f, 3}},
     {0, 1, 2, -1}},
    /* F5_ODE_HEUN2 */
    {2, {0.f, 1.f}, {1.f, 1.f}, false, true, {{{0.f, 0.f, 0.f}, 1.f, 1.f, 0}, {{0.5f, 0.f, 0.f}, 0.5f, 1.f, 1}}, {0, -1, -1, -1}},
    /* F5_ODE_HEUN3 */
    {3, {0.f, ODE_THIRD, ODE_TWO_THIRDS}, {1.f, 1.f, 1.f}, false, true,
     {{{0.f, 0.f, 0.f}, 1.f, ODE_THIRD, 0}, {{0.f, 0.f, 0.f}, 1.f, ODE_TWO_THIRDS, 0}, {{0.25f, 0.f, 0.f}, 0.75f, 1.f, 1}},
     {0, -1, -1, -1}},
};
inline const OdeMethod* ode_method_of(int ode_method) {
    return ode_method >= 0 && ode_method < (int)(sizeof(ODE_METHODS) / sizeof(ODE_METHODS[0])) ? &ODE_METHODS[ode_method] : nullptr;
}

// evaluation times tv and coefficient words cf (om.evals * steps floats each) of the grid tgrid[0 .. steps], in the fp32 operation order of
// torchdiffeq's fixed-grid solvers: t0 + dt * c and dt * h are rounded once per operation (build with FMA contraction off)
inline void ode_time_grid(const OdeMethod& om, const float* tgrid, int steps, float* tv, float* cf) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int E = om.evals;
    for (int s = 0; s < steps; ++s) {
        const float t0 = tgrid[s], t1 = tgrid[s + 1];
        const float dt = t1 - t0;
        for (int j = 0; j < E; ++j) {
            tv[E * s + j] = j == 0 ? t0 : (om.last_at_t1 && j == E - 1) ? t1 : t0 + dt * om.c[j];
            cf[E * s + j] = dt * om.h[j];
        }
    }
}
