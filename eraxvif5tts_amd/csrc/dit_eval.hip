// dit_eval.hip -- one evaluation of the DiT backbone (reference model/backbones/dit.py:185-233, model/modules.py:301-336,610-641): its modes,
// decided once (dit_eval_modes), the LayerNorm and LayerNorm-fold call sites, the two halves of a block, and the walk over the blocks.
#include "model_internal.h"

// Tile quantisation at small batches: the fused projection has 12 feature tiles per token tile; when the q|k part alone (8 tiles
// per token tile) fills the CUs a whole number of times but q|k|v does not (M = 8192, 4 utterances x 1024 frames x CFG: 256 + 128
// tiles on 256 CUs, the second round half empty), v is projected by its own launch on 256 x 128 tiles: 70 -> 62 us per block.
// (round 3, late: any token count whose q|k tiles fit one round while q|k|v would need a second -- ragged batches, odd batch sizes:
//  M = 6144: 288 tiles of 256 x 256 = two rounds, 60 us; 192 + 192 narrower ones: 53 us.  Same sums either way.)
static bool split_v_tiles(int rows, int inner, int ncu) {
    const int tiles_m = (rows + 255) / 256;
    return inner % 256 == 0 && tiles_m * (2 * inner / 256) <= ncu && tiles_m * (3 * inner / 256) > ncu && tiles_m * (2 * inner / 256) >= 160;
}

// LayerNorm fold: which of an evaluation's two folded projections (QKV, FF1) take their row statistics from the producer's partial sums inside
// their own kernel.  md.rows token rows, md.rows_g with the padding of the block GEMMs.  Otherwise one stats_finalize launch sits in front.
static void lnf_inkernel_sites(const f5_plan_s* p, DitEvalModes& md) {
    const f5_dit_config& c = p->m->cfg;
    const int D = c.dim, inner = p->m->inner, ff = c.ff_inner, rows = md.rows, rows_g = md.rows_g;
    if (!p->lnf_stats2) return;
    auto narrow_tile = [&](int M, int N) {  // the 8-wave kernel gives this projection a tile narrower than 256 (statistics held in registers)
        GemmParams t = gp_zero();
        t.M = M; t.N = N; t.K = D; t.lda = D; t.ldw = D;
        return gemm_fast_lnf_inkernel(t);
    };
    // knob "ln_fold_inkernel": the 8-wave kernel's in-kernel form wherever its tile allows (QKV as DitEval::attention launches it: q|k and v apart under
    // split_v).  md.split_v is the tile arithmetic alone.  The launch adds three conditions, so the two can disagree: where the one-wave-per-SIMD
    // kernel takes the fused projection (3 x 1024 frames on 256 CUs) this line asks about q|k and v apart and the launch is fused.  The answer is
    // the same either way: the window starts at 160 q|k tiles of 256 x 256, so by the shape rule neither q|k nor q|k|v is narrow there (gemm_fast_tile),
    // and a forced tile (knobs "gemm_tile", "gemm_bm128" = 2) is forced on q|k, v and q|k|v alike.  And a launch that carries the in-kernel form is
    // refused by the one-wave-per-SIMD kernel unless its own 128-row tiles finish the statistics (gemm_w4_ok), which leaves it split as predicted.
    if (g_ln_fold_inkernel) {
        md.ink_qkv = narrow_tile(rows, md.split_v ? 2 * inner : 3 * inner);
        if (md.split_v) md.ink_qkv = md.ink_qkv && narrow_tile(rows, inner);
        md.ink_ff1 = narrow_tile(rows, ff);
    }
    // ... and on the one-wave-per-SIMD kernel's 128-row tiles the consumer finishes the statistics by default (gemm_w4.hip: finish_stats; small
    // batches, where the two statistics launches of a block were 13 of its 102 us).  Only where the 8-wave kernel could take the launch in the
    // same form, should the other kernel refuse it.
    if (!c.qk_norm) {
        if (!md.ink_qkv && gemm_w4_lnf_inkernel(rows_g, 3 * inner, D) != 0 && narrow_tile(rows_g, 3 * inner)) md.ink_qkv = true;
        if (!md.ink_ff1 && gemm_w4_lnf_inkernel(rows_g, ff, D) != 0 && narrow_tile(rows_g, ff)) md.ink_ff1 = true;
    }
}

int dit_eval_modes(const f5_plan_s* p, int nb, int N, int mod_bstride, DitEvalModes* out) {
    const f5_model_s* m = p->m;
    const f5_dit_config& c = m->cfg;
    const int D = c.dim, inner = m->inner, ff = c.ff_inner, rows = nb * N;
    DitEvalModes& md = *out = DitEvalModes{};
    md.rows = rows;
    // Residual stream storage.  fp32 mode, stage taps or ln_defer = 0: fp32 throughout.  bf16 production mode: fp16 from here on (the
    // hoisted part of the input embedding included) -- the reference's own GPU path keeps the whole model, residual stream included, in
    // fp16 (utils_infer.py:184-193); arithmetic stays fp32 and the branches stay bf16.  Bytes per block of the two LayerNorm passes:
    // 1 408 -> 1 024 MiB at C2; of the input embedding 656 -> 400 MiB.
    md.defer = p->taps.empty() && g_ln_defer && !c.long_skip;  // (long skip: the stream after the input embedding is needed as a value)
    md.r16 = plan_res_f16(p);
    // In-place residual updates (bf16 production mode, one time per evaluation): the fp16 stream is updated by the epilogues of the attention
    // out-projection and of the second FF linear (EPI_RESID on the fp16 stream) and the LayerNorm passes only read it (block 0 first adds the
    // position-conv branch): 1 024 MiB of stream + branch traffic per block instead of 1 280, and the two passes shrink from 384 + 640 MiB to
    // 256 + 256.  Otherwise (fp32 stream, stage taps, per-sample time rows, knob "resid_rmw" = 0): store-only branches, adds fused into the passes.
    md.rmw = md.r16 && mod_bstride == 0 && g_resid_rmw;
    // LayerNorm fold (round 4; gemm.h, lnfold.hip): from the second LayerNorm of block 0 on, the two LayerNorm passes of a block are gone.  The
    // in-place residual epilogues (out-projection, FF2) also write partial row sums of the values they store, stats_finalize_kernel turns them
    // into (mean, rstd) per row -- and carries the fp16 range guard the passes carried -- and the QKV / FF1 projections read the fp16 stream
    // itself against this evaluation time's W' = fp16(W (1 + scale)), applying rstd (acc - mean c1) + c2 in their epilogues.  Block 0's first
    // pass stays (it folds the position-conv branch in), and so does the final AdaLN pass in front of proj_out.  Needs the in-place stream
    // (rmw), the time grid's table (stage_time_grid) and the tuned kernel at all four call sites.
    // Token counts that are not a multiple of the 256-row tile (8 x 1001 frames, every ragged batch): the four block GEMMs run over the rows
    // ROUNDED UP to 256 -- the workspace is padded to that anyway -- so that they stay on the persistent schedule with whole tiles only.  The rows
    // past the last token compute on whatever the padding holds (finite: zero-filled arena, saturating fp16 stores).  Their fp16 stream rows are
    // never reset: the EPI_RESID epilogues keep adding gate * (A W + b) to them, evaluation after evaluation and call after call, until they sit
    // at the saturation value.  What reads them: the four block GEMMs themselves (the out-projection and FF2 read-modify-write them, their
    // partial row sums go to lnf_partial) and a folded consumer that finishes the row statistics inside its kernel (gemm_w4.hip finish_stats, the
    // 8-wave in-kernel form), which turns them into (mean, rstd) for its own epilogue.  GemmParams::lnf_rows = rows keeps them out of every stored
    // statistics table and out of the fp16 range guard -- a padding row at +-65504 must not send the plan to fp32 storage.  Nothing else reads
    // them: every other kernel works on `rows`, attention on the utterances' own rows.
    md.rows_g = (md.rmw && g_gemm_pad_rows && rows >= 3584 /* from here on the fused projection takes the 256-wide persistent tile */ && rows % 256 != 0 && (size_t)((rows + 255) / 256 * 256) <= p->rows_cap) ? (rows + 255) / 256 * 256 : rows;
    const FoldTable* ft = p->fold;
    // (not under a block subset: the table and block 0's second weight copy are laid out for the full depth -- no fold, q as projected)
    md.lnf = md.rmw && g_ln_fold && ft && p->lnf_stats && p->fold_eval >= 0 && p->fold_eval < (int)ft->tv.size() && p->gemm_kernel != 0 &&
             (p->gemm_kernel == 1 || rows >= 512) && D % 64 == 0 && inner % 64 == 0 && ff % 64 == 0 && p->sub.empty();
    // pre-scaled q: the table's q rows and block 0's second weight copy carry the softmax scale, the attention kernels apply none
    md.qs = md.lnf && ft->qscaled && plan_attn_prescale(p);
    if (md.lnf && ft->qscaled && !md.qs) return f5_fail(F5_ESTATE, "dit_eval: the fold table holds pre-scaled q rows, the plan runs without them");
    md.frow0 = md.lnf ? ((size_t)p->fold_eval * c.depth) * (size_t)m->fold_R : 0;
    // small batches: every block's weights come from HBM again and the GEMMs are bound by operand latency, so the LayerNorm passes pull
    // the weights of the launches behind them towards the caches (one dword per line): a block's first pass the out-projection and FF1, the
    // second one FF2 and the next block's QKV projection
    md.wpf = md.r16 && g_w_prefetch && rows <= g_w_prefetch;
    md.split_v = split_v_tiles(rows, inner, f5_cu_count());
    if (md.lnf) lnf_inkernel_sites(p, md);
    return 0;
}

extern "C" int f5_debug_eval_modes(f5_plan_t p, int nb, int N, int per_batch_rows, int32_t* out) {
    if (!p || !out || nb <= 0 || N <= 0) return f5_fail(F5_EINVAL, "f5_debug_eval_modes: null plan / output or empty shape");
    if (p->m->cfg.backbone != F5_BACKBONE_DIT) return f5_fail(F5_ENOTSUP, "f5_debug_eval_modes: DiT backbone only");
    DitEvalModes md;
    F5_TRY(dit_eval_modes(p, nb, N, per_batch_rows ? p->m->modrow : 0, &md));
    const int32_t v[F5_EVAL_MODES_N] = {md.rows, md.rows_g, md.defer, md.r16, md.rmw, md.lnf, md.qs, md.wpf, md.ink_qkv, md.ink_ff1, md.split_v, (int32_t)md.frow0};
    memcpy(out, v, sizeof(v));
    return 0;
}

int dit_probe_check(f5_plan_s* p, int nb, int N, int mod_bstride, int nev) {
    if (p->probes.empty()) return 0;
    if (p->m->cfg.backbone != F5_BACKBONE_DIT) return f5_fail(F5_ENOTSUP, "stage probes: DiT backbone only");
    if (p->probe_eval >= nev) return f5_fail(F5_EINVAL, "stage probes: probe_eval %d, the call makes %d evaluation(s)", p->probe_eval, nev);
    p->fold_eval = mod_bstride ? -1 : p->probe_eval;  // (as net_eval sets it for that evaluation)
    DitEvalModes md;
    F5_TRY(dit_eval_modes(p, nb, N, mod_bstride, &md));
    for (const auto& kv : p->probes) {
        int j;
        std::string s;
        F5_TRY(probe_parse(kv.first, plan_depth(p), &j, &s));
        const char* why = nullptr;
        if ((s == "x_in" || s == "x_attn" || s == "x_ff") && !md.rmw) why = "the residual stream is not updated in place";
        if (s == "n1" && md.lnf && j > 0) why = "the LayerNorm fold runs no first pass in this block";
        if ((s == "stats1" || s == "stats2") && !md.lnf) why = "no LayerNorm fold";
        if (why) return f5_fail(F5_ESTATE, "stage probe '%s': %s in this evaluation", kv.first.c_str(), why);
    }
    return 0;
}

namespace {
// the block at position j of the walk: model block l, its weights, its AdaLN rows, its prefetch sets, its rows of the fold table
struct DitBlock {
    int l, j;
    const BlockW* b;
    const float* ml;  // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp (modules.py:312)
    PrefetchSet pf1, pf2, pf1f, pf2f;
    bool lnf1, lnf_next;
    const char* fW;  // this block's W' rows: q|k|v, then ff.0.0
    const float *fc1, *fc2;
};
// one running evaluation: its arguments, its modes, and its call sites
struct DitEval {
    f5_plan_s* const p;
    const int nb, N, mod_bstride;
    const float* const modp;
    const uint8_t* const mask;
    hipStream_t const st;
    DitEvalModes md;
    f5_model_s* const m = p->m;
    const f5_dit_config& c = m->cfg;
    const int D = c.dim, P = c.precision, inner = m->inner, ff = c.ff_inner;
    PrefetchSet pf1f_prev{{nullptr, nullptr, nullptr, nullptr}, {0u, 0u, 0u, 0u}};  // the previous block's pf1f
    unsigned* sat() const { return md.r16 ? p->sat_flag : nullptr; }
    float* lnf_table(int k) const { return k < 0 ? nullptr : (k & 1 ? p->lnf_stats2 : p->lnf_stats); }
    int layernorm(int site, int j, const float* mul, const float* add, const PrefetchSet* pf) const;
    void lnf_producer(GemmParams& g, int k, const PrefetchSet& pf, bool consumer_inkernel) const;
    int lnf_consumer(GemmParams& g, int k, bool inkernel, int site, int tag, const PrefetchSet* pf) const;
    DitBlock block(int j, int l, int l_next) const;
    int attention(const DitBlock& k) const;
    int feed_forward(const DitBlock& k) const;
    // stage probes: copies of what this evaluation holds anyway, of its token rows (md.rows, never the padding rows of the block GEMMs)
    const bool probing = plan_probing(p);
    int stream_prec() const { return md.r16 ? F5_PREC_FP16 : F5_PREC_FP32; }
    const void* stream() const { return md.r16 ? p->xres16 : (const void*)p->xres; }
    int probe(int j, const char* stage, int prec, const void* src, int cols, int ld = 0, int rows = 0) const {
        if (!probing) return 0;
        return probe_copy(p, j < 0 ? std::string(stage) : "blk" + std::to_string(j) + "." + stage, prec, src, ld ? ld : cols, rows ? rows : md.rows, cols, st);
    }
};
}  // namespace

// One of the evaluation's three LayerNorm passes over the stream, out -> p->hT: site 1 / 2 = the first / second LayerNorm of the block at position j,
// 3 = the final AdaLN.  In-place stream (rmw): the stream already holds every branch and the pass only reads it, but block 0's first, which adds the
// position-conv branch.  Otherwise the pass adds the stored branch(es).  With no stage tap set (defer), the residual stream is then written once per
// block: the first pass normalises x + y without storing it, the second LayerNorm of the block repeats the add (same operands, same order:
// bit-identical) and stores x + y + y_attn; after the last block the stream itself is not needed any more, so the last add is not written back.
int DitEval::layernorm(int site, int j, const float* mul, const float* add, const PrefetchSet* pf) const {
    void* const xs = md.r16 ? p->xres16 : (void*)p->xres;
    const void* y = md.rmw && !(site == 1 && j == 0) ? nullptr : p->yT;
    const void* y2 = !md.rmw && md.defer && site == 2 ? p->yA : nullptr;
    const int ymode = md.rmw || !md.defer ? 1 : (site == 2 ? 3 : 2);
    return launch_layernorm_res(P, xs, md.r16, xs, md.r16, D, md.rows, D, y, D, y2, ymode, mul, add, mod_bstride, N, 1, p->hT, D, st, pf, sat(),
                                site == 3 ? 3 : site | (j << 4));
}

// LayerNorm sites of the folded evaluation, in order: k = 2l is block l's second LayerNorm (statistics: its out-projection), k = 2l - 1 its
// first (statistics: FF2 of block l - 1).  Site k's (mean, rstd) go to table k & 1 (lnf_table); its pivots -- the rows' previous means -- are site
// k - 1's, in the other table (two tables: with the statistics taken inside the consumer kernel, sibling workgroups must still find the OLD means
// while feature tile 0's workgroups store the new ones).  A site's statistics are finished either inside the consumer kernel (ink: the
// one-wave-per-SIMD kernel's 128-row tiles, or the 8-wave kernel's tiles narrower than 256) or by one stats_finalize launch in front of
// it (same bits: lnf_stats_math.h).
// producer side of site k (out-projection, FF2): partial row sums of the stream it stores
void DitEval::lnf_producer(GemmParams& g, int k, const PrefetchSet& pf, bool consumer_inkernel) const {
    g.stats_out = p->lnf_partial; g.stats_ld = (int)p->rows_cap; g.stats_pivot = lnf_table(k - 1);
    g.lnf_rows = md.rows;  // (M = rows_g: the padding rows stay out of the range guard)
    if (md.rows <= g_w_prefetch && md.r16 && g_w_prefetch && consumer_inkernel) {  // no statistics launch behind this one: the GEMM itself touches the weights
        g.pf_p[0] = pf.p[0]; g.pf_n[0] = pf.n[0]; g.pf_p[1] = pf.p[1]; g.pf_n[1] = pf.n[1];
    }
}
// consumer side of site k: statistics finalized by one more launch, which also prefetches `pf`, or the in-kernel form
int DitEval::lnf_consumer(GemmParams& g, int k, bool inkernel, int site, int tag, const PrefetchSet* pf) const {
    const float* pivots = lnf_table(k - 1);
    g.lnf_rows = md.rows;  // (M = rows_g: the padding rows stay out of lnf_stats_out and the range guard)
    g.lnf_stats = lnf_table(k);  // (in-kernel form: marks the launch as folded; read only by the 256-wide tile)
    if (!inkernel)
        return timed(p, site, st, [&] {
            return launch_stats_finalize(p->lnf_partial, (int)p->rows_cap, D / 64, md.rows, D, pivots, lnf_table(k), sat(), tag, st, pf);
        });
    g.lnf_partial = p->lnf_partial; g.lnf_partial_ld = (int)p->rows_cap; g.lnf_ncols = D / 64;
    g.lnf_pivot = pivots; g.lnf_stats_out = lnf_table(k); g.lnf_sat = sat(); g.lnf_sat_tag = tag;
    return 0;
}

DitBlock DitEval::block(int j, int l, int l_next) const {
    DitBlock k{};
    k.l = l; k.j = j; k.b = &m->blocks[l];
    const BlockW& b = *k.b;
    k.ml = modp + (size_t)l * 6 * D;
    const size_t wes = f5_elem_size(P), fR = (size_t)m->fold_R, frow = md.frow0 + (size_t)l * fR;
    // (weight prefetch, DitEvalModes::wpf: the first LayerNorm pass pulls the out-projection and FF1, the second one FF2 and the next block's QKV projection)
    k.pf1 = PrefetchSet{{b.w_o, b.w_ff1, nullptr, nullptr}, {(unsigned)(D * inner * wes), (unsigned)(ff * D * wes), 0u, 0u}};
    k.pf2 = PrefetchSet{{b.w_ff2, l_next >= 0 ? m->blocks[l_next].w_qkv : nullptr, nullptr, nullptr}, {(unsigned)(D * ff * wes), (unsigned)(3 * inner * D * wes), 0u, 0u}};
    // (LayerNorm fold: the statistics kernels sit where the passes sat and prefetch what runs behind THEM -- the one behind the out-projection
    //  this block's W' rows of ff.0.0 and the FF2 weight, the one behind FF2 the next block's W' rows of q|k|v and its out-projection weight)
    if (md.lnf) {
        const FoldTable* ft = p->fold;
        k.pf2f = PrefetchSet{{(const char*)ft->Wt + (frow + 3 * inner) * D * 2, b.w_ff2, nullptr, nullptr}, {(unsigned)((size_t)ff * D * 2), (unsigned)(D * ff * wes), 0u, 0u}};
        if (l + 1 < c.depth)
            k.pf1f = PrefetchSet{{(const char*)ft->Wt + (frow + fR) * D * 2, m->blocks[l + 1].w_o, nullptr, nullptr}, {(unsigned)((size_t)3 * inner * D * 2), (unsigned)(D * inner * wes), 0u, 0u}};
        k.fW = (const char*)ft->Wt + frow * D * 2;
        k.fc1 = ft->c1 + frow; k.fc2 = ft->c2 + frow;
    }
    k.lnf1 = md.lnf && l > 0;  // this block's first LayerNorm is folded into its QKV projection (statistics: the previous block's FF2)
    k.lnf_next = md.lnf && l + 1 < c.depth;  // (the final AdaLN pass reads the stream itself)
    return k;
}

// attention half of a block: x += (conv branch | previous block's gated FF output); n1 = LN(x) * (1 + scale_msa) + shift_msa; q|k|v; attention;
// y = gate_msa * to_out(attn), 0 on padded query rows (modules.py:499-501, 635)
int DitEval::attention(const DitBlock& k) const {
    const BlockW& b = *k.b;
    const int rows = md.rows, j = k.j, l = k.l;
    const Ragged* rg = p->rg;  // ragged sample(): N = rows of one half, the utterances sit inside it between zero gaps
    const std::string tn = "blk" + std::to_string(j);
    if (j == 0) F5_TRY(probe(-1, "input_embed", stream_prec(), stream(), D));
    if (!k.lnf1) F5_TRY(timed(p, F5_SITE_LN1, st, [&] { return layernorm(1, j, k.ml + D, k.ml, md.wpf ? &k.pf1 : nullptr); }));
    if (j == 0 && md.rmw) F5_TRY(probe(0, "x_in", F5_PREC_FP16, p->xres16, D));
    if (!k.lnf1) F5_TRY(probe(j, "n1", P, p->hT, D));
    if (j == 0) F5_TRY(tap_f32(p, "input_embed", p->xres, D, rows, D, st));
    if (j == 0 && c.long_skip)  // residual = x  (dit.py:217-218)
        F5_HIP(hipMemcpyAsync(p->skips[0], p->xres, (size_t)rows * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (j > 0) F5_TRY(tap_f32(p, "blk" + std::to_string(j - 1) + ".out", p->xres, D, rows, D, st));
    F5_TRY(tap_t(p, tn + ".n1", p->hT, D, rows, D, st));
    const void* const wqkv = (md.qs && b.w_qkv_qs) ? b.w_qkv_qs : b.w_qkv;  // (block 0: the only unfolded projection of a folded evaluation)
    const float* const bqkv = (md.qs && b.w_qkv_qs) ? b.b_qkv_qs : b.b_qkv;
    const float* const rope = rg ? p->rope_exp : p->rope;  // (ragged: row r of a half -> its position in its utterance)
    GemmParams g = gp_qkv(p, wqkv, bqkv, md.rows_g, N, rope, true);
    if (k.lnf1) {
        g = gp_folded(g, p->xres16, k.fW, k.fc1, k.fc2);
        F5_TRY(lnf_consumer(g, 2 * l - 1, md.ink_qkv, F5_SITE_LN1, 1 | (l << 4), md.wpf ? &pf1f_prev : nullptr));
    }
    // v apart (split_v_tiles) -- not in fp32, not on the tile kernel, and not when the one-wave-per-SIMD kernel takes the whole fused projection: its
    // 128-row tiles give every CU a whole number of tiles there
    const bool split_v = !c.qk_norm && P != F5_PREC_FP32 && p->gemm_kernel != 0 && md.split_v && !gemm_w4_ok(g, GEMM_DENSE, EPI_ROPE_T);
    GemmParams gv = g;  // (the v launch of a split)
    if (split_v) {
        g.N = 2 * inner; gv.N = inner;
        gv.W = (const char*)wqkv + (size_t)2 * inner * D * f5_elem_size(P); gv.bias = bqkv + 2 * inner;
        if (k.lnf1) {
            gv = gp_folded(gv, p->xres16, k.fW + (size_t)2 * inner * D * 2, k.fc1 + 2 * inner, k.fc2 + 2 * inner);
            gv.lnf_stats_out = nullptr;  // (the q|k launch's feature tile 0 stores the new means)
        }
        gv.out_t = (char*)p->qkv + (size_t)2 * inner * f5_elem_size(P);
        gv.rope = nullptr; gv.rope_inner = gv.rope_heads = 0;
    }
    if (c.qk_norm) { g.rope = nullptr; g.rope_inner = g.rope_heads = 0; }  // q, k stored as projected; RMSNorm per head, then RoPE, in place (modules.py:463-475)
    F5_TRY(timed(p, F5_SITE_QKV, st, [&] {
        int rc = run_gemm(p, g, GEMM_DENSE, c.qk_norm ? EPI_STORE_T : EPI_ROPE_T, st);
        if (!rc && c.qk_norm) rc = launch_qknorm_rope(P, p->qkv, 3 * inner, rows, inner, c.heads, m->rope_heads, b.w_qn, b.w_kn, rope, N, st);
        return !rc && split_v ? run_gemm(p, gv, GEMM_DENSE, EPI_STORE_T, st) : rc;
    }));
    if (k.lnf1) F5_TRY(probe(j, "stats1", F5_PREC_FP32, lnf_table(2 * l - 1), 2));
    F5_TRY(probe(j, "qkv", P, p->qkv, 3 * inner));
    if (rg) {  // every utterance gets the computation of the launch its own batch-1 sample() makes, on its rows of both halves; the ones
               // that launch would give to the pipelined kernel share launches (grid.z = utterance x branch, 12 utterances per table)
        const AttnDropout drop = plan_attn_dropout(p, j, 0, (uint32_t)rg->n.size());  // batch word = branch * B + u
        F5_TRY(launch_attention_ragged_all(P, p->attn_kernel, nb, (int)rg->n.size(), rg->off.data(), rg->n.data(), c.heads, p->qkv, 3 * inner, p->cT, inner,
                                           st, N, md.qs, &drop));
    } else {
        const AttnDropout drop = plan_attn_dropout(p, j);  // batch word = row of the (CFG-doubled) batch
        F5_TRY(timed(p, F5_SITE_ATTN, st, [&] { return launch_attention(P, plan_attn_kind(p, N), nb, N, c.heads, p->qkv, 3 * inner, mask, p->cT, inner, st, 0, md.qs, &drop); }));
    }
    F5_TRY(probe(j, "ctx", P, p->cT, inner));
    if (float* d = tap_dst(p, tn + ".attn"))  // Attention module output before gating (extra GEMM, debug only)
        F5_TRY(run_gemm(p, gp_linear_f32(p->cT, b.w_o, b.b_o, rows, D, inner, d), GEMM_DENSE, EPI_STORE_F32, st));
    g = gp_out_proj(p, b.w_o, b.b_o, md.rows_g, N, k.ml + 2 * D, mod_bstride, mask, md.defer ? p->yA : p->yT, true);
    g.rowbits = (mask && mask == p->rowbits_src) ? p->rowbits : nullptr;
    if (md.rmw) g = gp_resid_stream(g, p->xres16, true);
    // partial row sums of the updated stream (site 2l); pivot = the row's previous mean (none yet at site 0: the tables are this evaluation's)
    if (md.lnf) lnf_producer(g, 2 * l, k.pf2f, md.ink_ff1);  // (prefetch: the weights of FF1 and FF2)
    F5_TRY(timed(p, F5_SITE_OUT, st, [&] { return run_gemm(p, g, GEMM_DENSE, md.rmw ? EPI_RESID : EPI_GATE_T, st); }));
    return md.rmw ? probe(j, "x_attn", F5_PREC_FP16, p->xres16, D) : 0;
}

// feed-forward half of a block: x += y; n2 = LN(x) * (1 + scale_mlp) + shift_mlp; y = gate_mlp * ff(n2)  (modules.py:639)
int DitEval::feed_forward(const DitBlock& k) const {
    const BlockW& b = *k.b;
    const int l = k.l;
    if (!md.lnf) F5_TRY(timed(p, F5_SITE_LN2, st, [&] { return layernorm(2, k.j, k.ml + 4 * D, k.ml + 3 * D, md.wpf ? &k.pf2 : nullptr); }));
    GemmParams g = gp_ff1(p, b.w_ff1, b.b_ff1, md.rows_g, true);
    if (md.lnf) {
        g = gp_folded(g, p->xres16, k.fW + (size_t)3 * inner * D * 2, k.fc1 + 3 * inner, k.fc2 + 3 * inner);
        F5_TRY(lnf_consumer(g, 2 * l, md.ink_ff1, F5_SITE_LN2, 2 | (l << 4), md.wpf ? &k.pf2f : nullptr));
    }
    F5_TRY(timed(p, F5_SITE_FF1, st, [&] { return run_gemm(p, g, GEMM_DENSE, EPI_STORE_T, st); }));
    if (md.lnf) F5_TRY(probe(k.j, "stats2", F5_PREC_FP32, lnf_table(2 * l), 2));
    F5_TRY(probe(k.j, "ff1", P, p->ffh, ff));
    g = gp_ff2(p, b.w_ff2, b.b_ff2, md.rows_g, N, k.ml + 5 * D, mod_bstride, p->yT, true);
    if (md.rmw) g = gp_resid_stream(g, p->xres16, true);
    if (k.lnf_next) lnf_producer(g, 2 * l + 1, k.pf1f, md.ink_qkv);  // site 2l + 1 (prefetch: the next block's q|k|v weights and its out-projection)
    F5_TRY(timed(p, F5_SITE_FF2, st, [&] { return run_gemm(p, g, GEMM_DENSE, md.rmw ? EPI_RESID : EPI_GATE_T, st); }));
    return md.rmw ? probe(k.j, "x_ff", F5_PREC_FP16, p->xres16, D) : 0;
}

// one network evaluation over `nb` batch rows (rows = nb*N) whose noisy mel rows are x[xrows, mel] (xrows divides rows);
// modulation row for batch b is modp + b * mod_bstride.  Result: p->vout [rows, MELP] f32.
int dit_eval(f5_plan_s* p, const float* x, int xrows, int nb, int N, const float* modp, int mod_bstride, const uint8_t* mask, hipStream_t st) {
    DitEval e{p, nb, N, mod_bstride, modp, mask, st};
    const f5_dit_config& c = e.c;
    const int D = c.dim, P = c.precision, rows = nb * N;
    // input embedding: h = W_x . x + base ; x_res = h + mish(conv(mish(conv(h)))), into the stream's storage (DitEvalModes::r16)
    const bool r16 = plan_res_f16(p);
    F5_TRY(input_embed(p, x, xrows, rows, N, r16 ? p->xres16 : (void*)p->xres, r16, true, st));
    F5_TRY(dit_eval_modes(p, nb, N, mod_bstride, &e.md));
    F5_TRY(e.probe(-1, "adaln", F5_PREC_FP32, modp, e.m->modrow, 0, 1));
    F5_TRY(e.probe(-1, "base", F5_PREC_FP32, p->base, D));  // (the hoisted half of the input embedding: what the x-projection adds)
    // Block subset (f5_plan_set_blocks): position j of the walk runs model block l = sub[j] -- its weights, its AdaLN rows, its prefetch sets --
    // and everything that speaks of the first, the previous or the last block (the position-conv branch, the long-skip copy, tap names, guard
    // tags, the dropout call word) keys on j: the evaluation of the model whose blocks are the subset renumbered.  No subset: l = j.
    const int nblk = plan_depth(p);
    auto block_at = [&](int j) { return p->sub.empty() ? j : p->sub[j]; };
    for (int j = 0; j < nblk; ++j) {
        const DitBlock k = e.block(j, block_at(j), j + 1 < nblk ? block_at(j + 1) : -1);
        F5_TRY(e.attention(k));
        F5_TRY(e.feed_forward(k));
        e.pf1f_prev = k.pf1f;  // (what a statistics launch in front of the next block's QKV projection prefetches)
    }
    const float* mf = modp + (size_t)c.depth * 6 * D;  // final AdaLN: (scale, shift) (modules.py:333)
    F5_TRY(e.layernorm(3, 0, mf, mf + D, nullptr));
    F5_TRY(tap_f32(p, "blk" + std::to_string(nblk - 1) + ".out", p->xres, D, rows, D, st));
    if (c.long_skip) {  // x = long_skip_connection(cat(x, residual))  (dit.py:227-228), then the final AdaLN on it
        const size_t es = f5_elem_size(P);
        F5_TRY(launch_convert_pad(P, p->xres, D, rows, D, D, p->catT, 2 * D, st));
        F5_TRY(launch_convert_pad(P, p->skips[0], D, rows, D, D, (char*)p->catT + (size_t)D * es, 2 * D, st));
        F5_TRY(run_gemm(p, gp_linear_f32(p->catT, e.m->w_lskip, nullptr, rows, D, 2 * D, p->xres), GEMM_DENSE, EPI_STORE_F32, st));
        F5_TRY(launch_layernorm(P, p->xres, D, rows, D, mf, mf + D, mod_bstride, N, 1, p->hT, D, st));
    }
    F5_TRY(tap_t(p, "final_norm", p->hT, D, rows, D, st));
    F5_TRY(e.probe(-1, "final_norm", P, p->hT, D));
    F5_TRY(run_gemm(p, gp_proj_out(p, rows, p->vout), GEMM_DENSE, EPI_STORE_F32, st));
    return e.probe(-1, "vout", F5_PREC_FP32, p->vout, c.mel_dim, MELP);
}
