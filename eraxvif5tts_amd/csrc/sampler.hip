// sampler.hip -- CFM.sample on the device (reference model/cfm.py:82-208): the fixed-grid ODE loop over network evaluations with CFG doubling
// -- one step loop over the solver table of ode_methods.h, behind the prologue of a uniform or of a ragged call --, hipGraph capture / replay
// keyed by the call, the fp16 range guard and its fp32 fallback, the LayerNorm-fold tables of a time grid, and the two families of entry points.
#include <algorithm>

#include "model_internal.h"

static_assert(F5_ODE_EULER == 0 && F5_ODE_MIDPOINT == 1 && F5_ODE_RK4 == 2 && F5_ODE_HEUN2 == 3 && F5_ODE_HEUN3 == 4 &&
                  sizeof(ODE_METHODS) / sizeof(ODE_METHODS[0]) == 5,
              "ODE_METHODS (ode_methods.h) is indexed by the F5_ODE_* constants");

extern "C" int f5_ode_evals_per_step(int ode_method) {
    const OdeMethod* om = ode_method_of(ode_method);
    return om ? om->evals : f5_fail(F5_EINVAL, "bad ode_method %d", ode_method);
}
// what both entry points refuse before any work: an unknown method, a grid the plan's per-evaluation buffers do not hold
static int check_method_and_evals(const f5_plan_s* p, int ode_method, int steps) {
    const OdeMethod* om = ode_method_of(ode_method);
    if (!om) return f5_fail(F5_EINVAL, "bad ode_method %d", ode_method);
    const int nev = om->evals * steps;
    if (nev > p->maxE) return f5_fail(F5_EINVAL, "%d evaluations exceed the plan's max_evals=%d", nev, p->maxE);
    return 0;
}

// ----------------------------------------------------------------------------- the sample loop
// attention dropout: call words one sample loop consumes (evaluations x blocks)
static uint32_t sample_call_words(const f5_plan_s* p, const SampleArgs& a) {
    return (uint32_t)(ode_method_of(a.method)->evals * a.steps) * (uint32_t)plan_depth(p);
}

// Prologue of a uniform batch [B, N]: text embeddings, the hoisted half of the input embedding, the key mask of the durations, the MMDiT text
// rows.  -> the key mask of the evaluations (null: none)
static int uniform_prologue(f5_plan_s* p, const SampleArgs& a, const uint8_t** mask, hipStream_t st) {
    const int B = a.B, N = a.N, bn = B * N;
    // (the AdaLN modulation rows of all evaluation times are already in p->mod: f5_sample keeps them across calls)
    // text embeddings are constants of the whole sample() (the reference caches them per branch, dit.py:202-210)
    F5_TRY(compute_text_embed(p, p->text_in, a.nt, B, N, 0, p->te[0], st));
    const uint8_t* cmask = a.cmask_on ? p->cmask_in : nullptr;  // read from the plan buffer: a replay sees the current call's mask
    F5_TRY(compute_base(p, p->cond_in, p->lens_in, p->te[0], B, N, 0, 0, st, cmask));
    if (a.cfg_on) {
        F5_TRY(compute_text_embed(p, p->text_in, a.nt, B, N, 1, p->te[1], st));
        F5_TRY(compute_base(p, p->cond_in, p->lens_in, p->te[1], B, N, 1, (size_t)bn, st, cmask));
    }
    *mask = nullptr;
    if (a.mask_on) {
        F5_TRY(launch_len_mask(p->dur_in, B, N, p->mask, st));
        if (a.cfg_on) F5_HIP(hipMemcpyAsync(p->mask + bn, p->mask, bn, hipMemcpyDeviceToDevice, st));
        *mask = p->mask;
        F5_TRY(launch_rowbits(p->mask, (a.cfg_on ? 2 : 1) * (int)bn, p->rowbits, st));
        p->rowbits_src = p->mask;
    }
    if (p->m->cfg.backbone == F5_BACKBONE_MMDIT) {  // the text stream restarts from these rows at every evaluation (mmdit.py:163-173: the cached embeddings)
        p->c_src[0] = p->te[0];
        p->c_src[1] = a.cfg_on ? p->te[1] : nullptr;
        p->c_nt = a.nt;
        p->c_rows_each = B * a.nt;
    }
    return 0;
}

// Prologue of a ragged call (p->rg; see "public: ragged sample"): text embedding and the hoisted half of the input embedding per utterance,
// each at its row offset
static int ragged_prologue(f5_plan_s* p, const SampleArgs& a, hipStream_t st) {
    const Ragged& rg = *p->rg;
    const int B = a.B, T = rg.T, mel = p->m->cfg.mel_dim, td = p->m->cfg.text_dim;
    for (int br = 0; br < (a.cfg_on ? 2 : 1); ++br)
        for (int u = 0; u < B; ++u) {
            const int nu = rg.n[u], nt_eff = a.nt < nu ? a.nt : nu;  // tokens beyond the frame count are curtailed (dit.py:51)
            float* te = p->te[br] + (size_t)rg.off[u] * td;
            F5_HIP(hipMemcpy2DAsync(p->text_in + (size_t)B * a.nt, (size_t)nt_eff * 4, p->text_in + (size_t)u * a.nt, (size_t)a.nt * 4, (size_t)nt_eff * 4, 1,
                                    hipMemcpyDeviceToDevice, st));
            F5_TRY(compute_text_embed(p, p->text_in + (size_t)B * a.nt, nt_eff, 1, nu, br, te, st));
            // (the staged per-frame condition mask, utterance u's slice at its row offset: a replay sees the current call's mask)
            F5_TRY(compute_base(p, p->cond_in + (size_t)rg.off[u] * mel, p->lens_in + u, te, 1, nu, br, (size_t)br * T + rg.off[u], st,
                                a.cmask_on ? p->cmask_in + rg.off[u] : nullptr));
        }
    return 0;
}

// The steps of a call over `rows` token rows per CFG half (nb batch items of N rows in all, key mask `mask` or null).  Evaluation j of step
// s reads xs = traj[s] (j = 0) or p->xmid, and the method's update kernel behind it writes p->xmid, or xn = traj[s + 1] after the last one.
// sync: diagnostic knob "sync_evals" -- the stream is synchronised between steps (never while capturing).
static int sample_steps(f5_plan_s* p, const SampleArgs& a, int rows, int nb, int N, const uint8_t* mask, bool sync, hipStream_t st) {
    const OdeMethod& om = *ode_method_of(a.method);
    const int mel = p->m->cfg.mel_dim;
    const size_t state = (size_t)rows * mel;
    float* slots = p->traj + (size_t)(a.steps + 1) * state;  // (ode_methods.h: the slot invariant)
    const float* vu = a.cfg_on ? p->vout + (size_t)rows * MELP : nullptr;
    const float* cfgr = a.cfg_rows ? p->cfg_rows : nullptr;  // (read at run time: a replay honours the vector staged by the current call)
    for (int s = 0; s < a.steps; ++s) {
        if (sync && s > 0) F5_HIP(hipStreamSynchronize(st));
        const float* xs = p->traj + (size_t)s * state;
        float* xn = p->traj + (size_t)(s + 1) * state;
        for (int j = 0; j < om.evals; ++j) {
            const int ev = om.evals * s + j;
            float* xo = j == om.evals - 1 ? xn : p->xmid;
            F5_TRY(net_eval(p, j == 0 ? xs : p->xmid, rows, nb, N, ev, 0, mask, st));
            if (om.rk_stage)
                F5_TRY(launch_rk_stage(xs, p->vout, vu, MELP, rows, mel, a.cfg, p->coefs + ev, om.stage[j], slots, state,
                                       om.slot[j] >= 0 ? slots + (size_t)om.slot[j] * state : nullptr, xo, st, cfgr));
            else
                F5_TRY(launch_cfg_step(xs, p->vout, vu, MELP, rows, mel, a.cfg, p->coefs + ev, xo, st, cfgr));
        }
    }
    return 0;
}

// everything between the staged inputs and the final state traj[steps]; capturable (no syncs, no allocations)
static int sample_body(f5_plan_s* p, const SampleArgs& a, hipStream_t st) {
    // range guard of the fp16 residual stream: cleared by a KERNEL node of the graph, so every replay starts clean.  (Not hipMemsetAsync: on
    // ROCm 7.2 the 32-byte memset node captured here cleared the words on the first launch of the instantiated graph and filled them with
    // two stale host pointers on every replay -- gpurun_out/r3g: [512..519] = {0xf5dffab8, 0x78fe, 0xea66b000, 0x7909} x 2 -- which read as
    // a raised flag and sent the second sample() of every process through the fp32 fallback.)
    F5_TRY(launch_fill_f32(reinterpret_cast<float*>(p->sat_flag), 8, 0.0f, st));
    if (p->rg) {  // one batch item per CFG half: the concatenation of the utterances, T rows; no key mask
        F5_TRY(ragged_prologue(p, a, st));
        F5_TRY(sample_steps(p, a, p->rg->T, a.cfg_on ? 2 : 1, p->rg->T, nullptr, false, st));
    } else {
        const uint8_t* mask = nullptr;
        F5_TRY(uniform_prologue(p, a, &mask, st));
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (g_sync_evals) (void)hipStreamIsCapturing(st, &capturing);
        F5_TRY(sample_steps(p, a, a.B * a.N, a.cfg_on ? 2 * a.B : a.B, a.N, mask, g_sync_evals && capturing == hipStreamCaptureStatusNone, st));
    }
    return plan_attn_dropout_advance(p, sample_call_words(p, a), st);  // (the loop's last node: a replay advances the base as an eager call does)
}

// ----------------------------------------------------------------------------- the graph cache
template <typename Pred> static void drop_graphs_where(f5_plan_s* p, Pred stale) {
    p->graphs.erase(std::remove_if(p->graphs.begin(), p->graphs.end(), stale), p->graphs.end());
}

// the ODE loop of one sample() on the staged inputs: replay of the hipGraph captured for this exact problem, or eager launches
static int run_sample_loop(f5_plan_s* p, const SampleArgs& a, int use_graph, hipStream_t st) {
    if (use_graph && p->taps.empty() && p->probes.empty() && !p->timing) {  // (taps, probes, timing: eager, and no cached capture is touched)
        // a tuning knob changed since the capture: the graph baked the old kernel choice
        drop_graphs_where(p, [](const GraphEntry& g) { return g.key.epoch != g_tuning_epoch; });
        const GraphKey key{a, g_tuning_epoch, p->fold && g_ln_fold ? p->fold->id : 0, p->rg ? p->rg->n : std::vector<int>()};
        auto ge = std::find_if(p->graphs.begin(), p->graphs.end(), [&](const GraphEntry& g) { return g.key == key; });
        if (ge == p->graphs.end()) {
            GraphEntry g(key);  // (leaving early destroys what it holds by then)
            if (!p->cap_stream) F5_HIP(hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking));
            F5_HIP(hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeRelaxed));
            int rc = sample_body(p, a, p->cap_stream);
            hipError_t e = hipStreamEndCapture(p->cap_stream, &g.graph);
            F5_TRY(rc);
            if (e != hipSuccess) return f5_fail(F5_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
            e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
            if (e != hipSuccess) return f5_fail(F5_EHIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
            // small LRU-less cache: drop the oldest bucket (32: batch inference over length buckets meets a few dozen shapes)
            if (p->graphs.size() >= 32) p->graphs.erase(p->graphs.begin());
            p->graphs.push_back(std::move(g));
            ge = p->graphs.end() - 1;
            ++p->graph_captures;  // (the launch below is the capture's own: it does not count as a replay)
        } else {
            ++p->graph_replays;
        }
        F5_HIP(hipGraphLaunch(ge->exec, st));
    } else {
        F5_TRY(sample_body(p, a, st));
    }
    if (p->drop_p > 0.0) {  // the loop is issued: host mirror of the base word its last node advances on the device
        p->drop_call_base = p->drop_base_host;
        p->drop_base_host += sample_call_words(p, a);
    }
    return 0;
}

// The stream was stored as saturating fp16: one small read of the flag words the LayerNorm passes raise (a stream synchronisation).  A
// large-activation checkpoint must not clip silently: the loop is repeated with fp32 residual storage -- y0 is still traj[0], every other
// input is staged -- and the plan keeps fp32 storage from now on.
static int guard_check_and_fallback(f5_plan_s* p, const SampleArgs& a, int use_graph, hipStream_t st) {
    F5_HIP(hipMemcpyAsync(p->sat_host, p->sat_flag, 32, hipMemcpyDeviceToHost, st));
    F5_HIP(hipStreamSynchronize(st));
    if (*p->sat_host != 0u) {
        p->sat_amax_bits = p->sat_host[1];
        p->sat_nan = p->sat_host[2] != 0u;
        p->sat_pass = p->sat_host[3];
        p->sat_blocks = p->sat_host[4];
        p->sat_row = 0x7fffffffu - p->sat_host[5];
        p->res_f16 = 0;
        ++p->fallbacks;
        plan_drop_graphs(p);  // they baked the fp16 kernels
        if (p->drop_p > 0.0) {  // attention dropout: the rerun draws the masks of the call it repeats
            F5_TRY(launch_attn_dropout_set(p->drop_base, p->drop_call_base, st));
            p->drop_base_host = p->drop_call_base;
        }
        F5_TRY(run_sample_loop(p, a, use_graph, st));
    }
    return 0;
}

static int finish_outputs(f5_plan_s* p, const SampleArgs& a, float* out, float* trajectory, hipStream_t st) {
    const int mel = p->m->cfg.mel_dim;
    const size_t state = (size_t)a.B * a.N * mel;
    F5_TRY(launch_final_where(p->cond_in, p->traj + (size_t)a.steps * state, p->lens_in, a.cmask_on ? p->cmask_in : nullptr, a.B, a.N, mel, out, st));
    if (trajectory) F5_HIP(hipMemcpyAsync(trajectory, p->traj, (size_t)(a.steps + 1) * state * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

// LayerNorm fold: point the plan at the model's table for the evaluation times `tv` (p->mod holds their AdaLN rows, computed on `st`), building it
// when no plan has sampled on this grid yet.  Never an error: without a table (knob off, grid too long, allocation refused) the unfolded path runs.
static int acquire_fold(f5_plan_s* p, const std::vector<float>& tv, hipStream_t st) {
    f5_model_s* m = p->m;
    const int nev = (int)tv.size();
    FoldTable* want = nullptr;
    if (m->w_fold && g_ln_fold && p->lnf_stats && nev > 0 && nev <= F5_FOLD_MAX_EVALS && p->sub.empty() /* the table is laid out for the full depth */) {
        const bool qs = plan_attn_prescale(p);
        for (FoldTable* t : m->folds)
            if (t->tv == tv && t->qscaled == qs) want = t;
        if (!want) {
            for (size_t i = 0; i < m->folds.size() && m->folds.size() >= F5_FOLD_TABLES;) {  // oldest first, never one a plan still points to
                if (m->folds[i]->users == 0 && m->folds[i] != p->fold) {
                    (void)hipDeviceSynchronize();  // (launches of other streams may still read it)
                    delete m->folds[i];
                    m->folds.erase(m->folds.begin() + i);
                } else {
                    ++i;
                }
            }
            const f5_dit_config& c = m->cfg;
            const size_t n = (size_t)nev * c.depth * m->fold_R;
            FoldTable* t = new FoldTable();
            bool ok = t->arena.alloc(&t->Wt, n * c.dim * 2, false) == 0 && t->arena.alloc_t(&t->c1, n, false) == 0 && t->arena.alloc_t(&t->c2, n, false) == 0 &&
                      hipEventCreateWithFlags(&t->ready, hipEventDisableTiming) == hipSuccess;
            ok = ok && launch_fold_weights(m->w_fold, m->b_fold, p->mod, m->modrow, nev, c.depth, m->fold_R, 3 * m->inner, c.dim, t->Wt, t->c1, t->c2, st, qs ? m->inner : 0,
                                           qs ? F5_ATTN_QSCALE : 1.0f) == 0 &&
                 hipEventRecord(t->ready, st) == hipSuccess;
            if (!ok) {
                (void)hipGetLastError();
                delete t;
            } else {
                t->tv = tv;
                t->qscaled = qs;
                t->id = ++m->fold_seq;
                m->folds.push_back(t);
                want = t;
            }
        } else if (want != p->fold) {
            F5_HIP(hipStreamWaitEvent(st, want->ready, 0));  // built on another plan's stream
        }
    }
    if (want != p->fold) {
        if (p->fold) --p->fold->users;
        p->fold = want;
        if (want) ++want->users;
    }
    // A capture bakes its table's addresses and carries the table's id in its key (GraphKey::fold_id), so it is launched only while the plan
    // points at that very table: captures of the model's other live tables stay, and a caller that alternates between two grids replays both.
    // Captures of a table that no longer exists (evicted above, or by another plan of the model) can never be found again -- ids are not
    // reused -- and are destroyed here.
    drop_graphs_where(p, [m](const GraphEntry& g) {
        return g.key.fold_id != 0 && std::none_of(m->folds.begin(), m->folds.end(), [&](const FoldTable* t) { return t->id == g.key.fold_id; });
    });
    return 0;
}

// evaluation times / coefficient words of a fixed grid (ode_methods.h: ode_time_grid) -> p->tvals / p->coefs, and the AdaLN rows of every
// evaluation time -> p->mod (kept across calls with the same grid on the same stream)
static int stage_time_grid(f5_plan_s* p, const float* tgrid_host, int steps, int ode_method, hipStream_t st) {
    const OdeMethod& om = *ode_method_of(ode_method);
    const int nev = om.evals * steps;
    std::vector<float> tv(nev), cf(nev);
    ode_time_grid(om, tgrid_host, steps, tv.data(), cf.data());
    // The time MLP and every AdaLN row depend only on the evaluation times: a server calls sample() with the same grid every time,
    // so the 0.56 GB weight pass is done once per grid and kept (1.7 ms per call; 3 % of a single-utterance sample()).
    if (p->mod_tv != tv || p->mod_stream != st) {  // the rows are ordered only behind the stream they were computed on
        p->mod_tv.clear();
        F5_TRY(launch_set_floats(p->tvals, tv.data(), nev, st));
        F5_TRY(compute_modulation(p, p->tvals, nev, st));
        p->mod_tv = tv;
        p->mod_stream = st;
    }
    F5_TRY(acquire_fold(p, tv, st));
    return launch_set_floats(p->coefs, cf.data(), nev, st);
}

// A plan holds ONE deferred sample(): its staged inputs and the device flag words would be overwritten by the next call.  Every entry point
// that reuses the plan's buffers completes the deferred call first (on the stream it was enqueued on), so a raised range-guard flag is never
// lost when a caller round-robins more chunks than it has streams.
int finish_if_pending(f5_plan_s* p) {
    if (p && p->pending.valid) return f5_sample_finish(p, (f5_stream_t)p->pending.stream);
    return 0;
}

// f5_sample and f5_sample_masked: cond_mask (dev u8 [B, N]) or null = the lens prefix
static int sample_impl(f5_plan_t p, int B, int N, const float* cond, const int32_t* text, int nt, const int32_t* lens, const int32_t* durations,
                       const float* y0, const float* tgrid_host, int steps, float cfg_strength, int ode_method, float* out, float* trajectory,
                       int use_graph, f5_stream_t stream, const uint8_t* cond_mask) {
    F5_TRY(check_plan_shape(p, B, N));
    if (!cond || !text || !lens || !y0 || !tgrid_host || !out) return f5_fail(F5_EINVAL, "null argument");
    if (steps <= 0 || nt <= 0) return f5_fail(F5_EINVAL, "steps and nt must be positive");
    F5_TRY(check_method_and_evals(p, ode_method, steps));
    F5_TRY(finish_if_pending(p));
    hipStream_t st = (hipStream_t)stream;
    f5_model_s* m = p->m;
    const int mel = m->cfg.mel_dim, bn = B * N;
    const size_t state = (size_t)bn * mel;
    const bool mmdit = m->cfg.backbone == F5_BACKBONE_MMDIT;
    if (mmdit && nt > p->maxN) return f5_fail(F5_EINVAL, "MMDiT: text length %d exceeds the plan's max_seq %d", nt, p->maxN);
    const int nt_eff = (mmdit || nt < N) ? nt : N;  // tokens beyond the frame count are curtailed (dit.py:51; MMDiT keeps them all, mmdit.py:40)

    F5_TRY(stage_time_grid(p, tgrid_host, steps, ode_method, st));
    F5_TRY(dit_probe_check(p, cfg_strength >= 1e-5f ? 2 * B : B, N, 0, ode_method_of(ode_method)->evals * steps));  // (needs the grid's fold table)
    F5_HIP(hipMemcpyAsync(p->cond_in, cond, state * sizeof(float), hipMemcpyDeviceToDevice, st));
    F5_HIP(hipMemcpyAsync(p->traj, y0, state * sizeof(float), hipMemcpyDeviceToDevice, st));
    F5_HIP(hipMemcpy2DAsync(p->text_in, (size_t)nt_eff * 4, text, (size_t)nt * 4, (size_t)nt_eff * 4, B, hipMemcpyDeviceToDevice, st));
    F5_HIP(hipMemcpyAsync(p->lens_in, lens, B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (durations) F5_HIP(hipMemcpyAsync(p->dur_in, durations, B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (cond_mask) F5_HIP(hipMemcpyAsync(p->cmask_in, cond_mask, (size_t)bn, hipMemcpyDeviceToDevice, st));

    SampleArgs a{B, N, nt_eff, steps, ode_method, cfg_strength >= 1e-5f ? 1 : 0, durations ? 1 : 0, cfg_strength, cond_mask ? 1 : 0};  // cfm.py:167
    const bool guarded = plan_res_f16(p) && p->sat_check && !p->timing;
    F5_TRY(run_sample_loop(p, a, use_graph, st));
    p->pending = PendingSample{};
    if (guarded && p->sat_check == 2) {
        // deferred guard (plan option "residual_guard" = 2): nothing synchronises here, so several plans can be fed on several streams from
        // one host thread; f5_sample_finish reads the flag later and repeats the loop if it must (the inputs stay staged in the plan)
        p->pending = PendingSample{true, a, use_graph, out, trajectory, st};
    } else if (guarded) {
        F5_TRY(guard_check_and_fallback(p, a, use_graph, st));
    }
    return finish_outputs(p, a, out, trajectory, st);
}

extern "C" int f5_sample(f5_plan_t p, int B, int N, const float* cond, const int32_t* text, int nt, const int32_t* lens,
                         const int32_t* durations, const float* y0, const float* tgrid_host, int steps, float cfg_strength, int ode_method,
                         float* out, float* trajectory, int use_graph, f5_stream_t stream) {
    return sample_impl(p, B, N, cond, text, nt, lens, durations, y0, tgrid_host, steps, cfg_strength, ode_method, out, trajectory, use_graph,
                       stream, nullptr);
}

extern "C" int f5_sample_masked(f5_plan_t p, int B, int N, const float* cond, const int32_t* text, int nt, const int32_t* lens,
                                const int32_t* durations, const float* y0, const float* tgrid_host, int steps, float cfg_strength,
                                int ode_method, const uint8_t* cond_mask, float* out, float* trajectory, int use_graph, f5_stream_t stream) {
    if (!cond_mask) return f5_fail(F5_EINVAL, "null cond_mask");
    return sample_impl(p, B, N, cond, text, nt, lens, durations, y0, tgrid_host, steps, cfg_strength, ode_method, out, trajectory, use_graph,
                       stream, cond_mask);
}

extern "C" int f5_sample_finish(f5_plan_t p, f5_stream_t stream) {
    if (!p) return f5_fail(F5_EINVAL, "null plan");
    if (!p->pending.valid) return 0;
    const PendingSample ps = p->pending;
    p->pending = PendingSample{};
    hipStream_t st = (hipStream_t)stream;
    const int before = p->fallbacks;
    F5_TRY(guard_check_and_fallback(p, ps.a, ps.use_graph, st));
    if (p->fallbacks != before) return finish_outputs(p, ps.a, ps.out, ps.trajectory, st);  // the loop ran again: write the outputs again
    return 0;
}

// ----------------------------------------------------------------------------- public: ragged sample
// The ODE loop of f5_sample over utterances of DIFFERENT frame counts in one set of launches, with no padding to a common length and no key
// mask: what F5TTSWrapper.generate needs for the text chunks of one call (the reference runs them one after the other at batch 1,
// infer/f5tts_wrapper.py:476-533; a batch-1 sample() has mask = None, cfm.py:152-155).  Every per-row kernel (GEMMs, LayerNorm, CFG step) runs
// over the concatenation; the three places where a token sees its neighbours are handled so that each utterance gets exactly the arithmetic
// of its own batch-1 call: the position conv reads zero gap rows where it would read its zero padding, RoPE takes a per-row position table,
// attention is launched per utterance on its rows.  Text embedding and the hoisted half of the input embedding are computed per utterance
// (ragged_prologue); the steps are sample_steps over the T rows of a half.
//
// f5_sample_ragged and f5_sample_ragged_ex: cond_mask (dev u8 [sum(frames)]) or null = the lens prefix of every utterance; cfg_host (host
// f32 [B]) or null = cfg_strength for all of them
static int sample_ragged_impl(f5_plan_t p, int B, const int32_t* frames_host, const float* cond, const int32_t* text, int nt, const int32_t* lens,
                              const uint8_t* cond_mask, const float* y0, const float* tgrid_host, int steps, float cfg_strength,
                              const float* cfg_host, int ode_method, float* out, f5_stream_t stream) {
    if (!p) return f5_fail(F5_EINVAL, "null plan");
    F5_TRY(f5_check_device());
    if (!frames_host || !cond || !text || !lens || !y0 || !tgrid_host || !out) return f5_fail(F5_EINVAL, "null argument");
    f5_model_s* m = p->m;
    if (m->cfg.backbone != F5_BACKBONE_DIT) return f5_fail(F5_ENOTSUP, "f5_sample_ragged: DiT backbone only");
    if (B <= 0 || B > p->maxB || steps <= 0 || nt <= 0 || nt > p->maxN) return f5_fail(F5_EINVAL, "bad B / steps / nt for this plan");
    F5_TRY(check_method_and_evals(p, ode_method, steps));
    if (!p->taps.empty() || p->timing) return f5_fail(F5_ESTATE, "f5_sample_ragged: stage taps / in-situ timing are not available here");
    // One doubled batch cannot hold utterances of both branches of cfm.py:167 (below 1e-5 the reference makes ONE pass, and its bits are
    // those of an undoubled batch): refused before anything is staged or launched; the caller keeps such requests in different calls.
    bool cfg_on = cfg_strength >= 1e-5f;
    if (cfg_host) {
        cfg_on = cfg_host[0] >= 1e-5f;
        for (int u = 0; u < B; ++u) {
            if (!(cfg_host[u] == cfg_host[u])) return f5_fail(F5_EINVAL, "utterance %d: guidance strength is NaN", u);
            if ((cfg_host[u] >= 1e-5f) != cfg_on)
                return f5_fail(F5_EINVAL, "guidance strengths below and at or above 1e-5 in one call (utterances 0 and %d): sample them in separate calls", u);
        }
    }
    const bool cfg_vec = cfg_host && cfg_on;  // (below 1e-5 no combine runs: the vector has nothing to say)
    Ragged rg;
    for (int u = 0; u < B; ++u) {
        if (frames_host[u] <= 0 || frames_host[u] > p->maxN) return f5_fail(F5_EINVAL, "utterance %d: %d frames outside 1 .. %d", u, frames_host[u], p->maxN);
        rg.off.push_back(rg.T);
        rg.n.push_back(frames_host[u]);
        rg.T = (int)round_up((size_t)rg.T + frames_host[u] + RAGGED_GAP, 16);
    }
    const size_t bn_cap = (size_t)p->maxB * p->maxN;
    if ((size_t)rg.T > bn_cap || 2 * (size_t)rg.T > p->rows_cap || (size_t)(B + 1) * nt > bn_cap)
        return f5_fail(F5_EINVAL, "%d rows (frames + gaps) exceed the plan (max_batch x max_seq = %zu)", rg.T, bn_cap);
    F5_TRY(finish_if_pending(p));
    hipStream_t st = (hipStream_t)stream;
    const int mel = m->cfg.mel_dim, D = m->cfg.dim, td = m->cfg.text_dim, T = rg.T;
    F5_TRY(stage_time_grid(p, tgrid_host, steps, ode_method, st));
    F5_TRY(dit_probe_check(p, cfg_on ? 2 : 1, T, 0, ode_method_of(ode_method)->evals * steps));  // (needs the grid's fold table)
    // stage the inputs at their row offsets; everything between the utterances is zero
    F5_HIP(hipMemsetAsync(p->cond_in, 0, (size_t)T * mel * sizeof(float), st));
    F5_HIP(hipMemsetAsync(p->traj, 0, (size_t)T * mel * sizeof(float), st));
    F5_HIP(hipMemsetAsync(p->te[0], 0, (size_t)T * td * sizeof(float), st));
    F5_HIP(hipMemsetAsync(p->te[1], 0, (size_t)T * td * sizeof(float), st));
    F5_HIP(hipMemsetAsync(p->base, 0, (size_t)2 * T * D * sizeof(float), st));
    if (p->base16) F5_HIP(hipMemsetAsync(p->base16, 0, (size_t)2 * T * D * 2, st));
    F5_HIP(hipMemsetAsync(p->rope_exp, 0, (size_t)T * 64 * sizeof(float), st));
    F5_HIP(hipMemsetAsync(p->gapflag, 1, (size_t)2 * T, st));
    size_t src = 0;
    for (int u = 0; u < B; ++u) {
        const size_t nu = rg.n[u], off = rg.off[u];
        F5_HIP(hipMemcpyAsync(p->cond_in + off * mel, cond + src * mel, nu * mel * sizeof(float), hipMemcpyDeviceToDevice, st));
        F5_HIP(hipMemcpyAsync(p->traj + off * mel, y0 + src * mel, nu * mel * sizeof(float), hipMemcpyDeviceToDevice, st));
        F5_HIP(hipMemcpyAsync(p->rope_exp + off * 64, p->rope, nu * 64 * sizeof(float), hipMemcpyDeviceToDevice, st));
        F5_HIP(hipMemsetAsync(p->gapflag + off, 0, nu, st));
        F5_HIP(hipMemsetAsync(p->gapflag + T + off, 0, nu, st));
        src += nu;
    }
    F5_HIP(hipMemcpyAsync(p->text_in, text, (size_t)B * nt * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    F5_HIP(hipMemcpyAsync(p->lens_in, lens, B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (cond_mask) {  // the per-frame condition masks at the utterances' row offsets (compute_base and the final where read their slices)
        F5_HIP(hipMemsetAsync(p->cmask_in, 0, (size_t)T, st));
        src = 0;
        for (int u = 0; u < B; ++u) {
            F5_HIP(hipMemcpyAsync(p->cmask_in + rg.off[u], cond_mask + src, (size_t)rg.n[u], hipMemcpyDeviceToDevice, st));
            src += (size_t)rg.n[u];
        }
    }
    if (cfg_vec) {  // one value per row of a half, staged here -- outside the captured region -- so a replayed graph reads this call's values
        F5_TRY(launch_fill_f32(p->cfg_rows, (size_t)T, 0.0f, st));
        for (int u = 0; u < B; ++u) F5_TRY(launch_fill_f32(p->cfg_rows + rg.off[u], (size_t)rg.n[u], cfg_host[u], st));
    }

    SampleArgs a{B, T, nt, steps, ode_method, cfg_on ? 1 : 0, 0, cfg_vec ? 0.0f : cfg_strength, cond_mask ? 1 : 0, cfg_vec ? 1 : 0};  // cfm.py:167
    p->pending = PendingSample{};
    p->rg = &rg;
    const int use_graph = p->ragged_graph;  // a bucket shape that recurs (batch inference over fixed buckets) replays its capture
    int rc = run_sample_loop(p, a, use_graph, st);
    // (always checked inside the call; the rerun reads the same staged mask and guidance rows)
    if (rc == 0 && plan_res_f16(p) && p->sat_check) rc = guard_check_and_fallback(p, a, use_graph, st);
    p->rg = nullptr;
    F5_TRY(rc);
    const float* xf = p->traj + (size_t)steps * T * mel;
    src = 0;
    for (int u = 0; u < B; ++u) {
        const size_t off = rg.off[u];
        F5_TRY(launch_final_where(p->cond_in + off * mel, xf + off * mel, p->lens_in + u, cond_mask ? p->cmask_in + off : nullptr, 1, rg.n[u], mel,
                                  out + src * mel, st));
        src += (size_t)rg.n[u];
    }
    return 0;
}

extern "C" int f5_sample_ragged(f5_plan_t p, int B, const int32_t* frames_host, const float* cond, const int32_t* text, int nt, const int32_t* lens,
                                const float* y0, const float* tgrid_host, int steps, float cfg_strength, int ode_method, float* out,
                                f5_stream_t stream) {
    return sample_ragged_impl(p, B, frames_host, cond, text, nt, lens, nullptr, y0, tgrid_host, steps, cfg_strength, nullptr, ode_method, out, stream);
}

extern "C" int f5_sample_ragged_ex(f5_plan_t p, int B, const int32_t* frames_host, const float* cond, const int32_t* text, int nt, const int32_t* lens,
                                   const uint8_t* cond_mask, const float* y0, const float* tgrid_host, int steps, float cfg_strength,
                                   const float* cfg_host, int ode_method, float* out, f5_stream_t stream) {
    return sample_ragged_impl(p, B, frames_host, cond, text, nt, lens, cond_mask, y0, tgrid_host, steps, cfg_strength, cfg_host, ode_method, out, stream);
}
