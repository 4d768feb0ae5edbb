// eval_common.hip -- what every backbone evaluation shares: GEMM dispatch, stage taps, the AdaLN table (modules.py:311,332), the text
// embedding (dit.py:49-79), the hoisted half of the input embedding (dit.py:88-96), and the public single-evaluation entry points.
#include "model_internal.h"

// ----------------------------------------------------------------------------- helpers
// Pre-scaled q: bf16 production mode of the DiT backbone on the tuned attention kernels, no qk_norm, no stage taps.  The
// softmax scale then sits in the weights that project q -- the fold table's q rows and block 0's second copy -- and the attention kernels
// apply none.  It rides on the LayerNorm fold: an evaluation that runs unfolded keeps q as projected (dit_eval).
bool plan_attn_prescale(const f5_plan_s* p) {
    const f5_dit_config& c = p->m->cfg;
    const bool want = p->attn_prescale < 0 ? g_attn_prescale != 0 : p->attn_prescale != 0;
    return want && c.backbone == F5_BACKBONE_DIT && c.precision == F5_PREC_BF16 && !c.qk_norm && p->attn_kernel != 0 && p->taps.empty() &&
           p->m->blocks.size() > 0 && p->m->blocks[0].w_qkv_qs != nullptr && !(p->drop_p > 0.0) /* the dropout kernels take q as projected */;
}
AttnDropout plan_attn_dropout(const f5_plan_s* p, int l, uint32_t bw0, uint32_t bw_step) {
    AttnDropout d;
    if (!(p->drop_p > 0.0)) return d;
    d.prob = p->drop_p;
    d.seed = p->drop_seed;
    d.base = p->drop_base;
    d.offset = (uint32_t)p->drop_eval * (uint32_t)plan_depth(p) + (uint32_t)l;
    d.bw0 = bw0;
    d.bw_step = bw_step;
    return d;
}
int plan_attn_kind(const f5_plan_s* p, int S) {  // launch_attention's kernel for sequences of S tokens: 1 = the tuned kernels where they support S
    return p->attn_kernel != 0 && attention_fast_supported(p->m->cfg.precision, S, p->m->cfg.heads) ? 1 : 0;
}
int plan_attn_dropout_advance(f5_plan_s* p, uint32_t by, hipStream_t st) {
    if (!(p->drop_p > 0.0)) return 0;
    return launch_attn_dropout_advance(p->drop_base, by, st);
}
// fp16 residual storage for this plan's evaluations (bf16 mode without stage taps; the plan option overrides the process-wide knob)
bool plan_res_f16(const f5_plan_s* p) {
    const bool want = p->res_f16 < 0 ? g_res_f16 != 0 : p->res_f16 != 0;
    if (p->m->cfg.backbone != F5_BACKBONE_DIT || p->m->cfg.long_skip) return false;  // (UNetT, MMDiT and the long-skip DiT keep fp32 streams)
    return want && p->taps.empty() && g_ln_defer && p->m->cfg.precision != F5_PREC_FP32 && p->xres16 && p->base16;  // (both 16-bit modes)
}

GemmParams gp_zero() {
    GemmParams g;
    memset(&g, 0, sizeof(g));
    return g;
}
static struct { GemmLaunchRecord last{-1, 0, 0, 0, 0}; int launches = 0; } g_site_gemm[5];
int run_gemm(f5_plan_s* p, const GemmParams& g, int mode, int epi, hipStream_t st) {
    const int prec = p->m->cfg.precision;
    // 1 = tuned kernel wherever it can run; -1 (auto) = tuned kernel from 512 token rows on (narrower tiles keep the CUs busy at small M)
    int kind = 0;
    if (p->gemm_kernel != 0 && gemm_fast_supported(g, prec, mode, epi) && (p->gemm_kernel == 1 || g.M >= 512)) kind = 1;
    const int rc = launch_gemm(g, prec, mode, epi, kind, st);
    if (g.site >= 1 && g.site <= 4) {  // host-side record per block call site (f5_debug_site_gemm)
        g_site_gemm[g.site].last = g_last_gemm;
        ++g_site_gemm[g.site].launches;
    }
    return rc;
}
// diagnostic: the last launch of one of the DiT block's four call sites (GemmParams::site: 1 QKV, 2 out-projection, 3 FF1, 4 FF2) and the number of
// launches the site has made in this process (a QKV projection with v apart makes two per block)
extern "C" int f5_debug_site_gemm(int site, int* family, int* bm, int* bn, int* schedule, int* flags, int* launches) {
    if (site < 1 || site > 4 || !family || !bm || !bn || !schedule || !flags || !launches) return f5_fail(F5_EINVAL, "f5_debug_site_gemm: site 1 .. 4, no null argument");
    const GemmLaunchRecord& r = g_site_gemm[site].last;
    *family = r.family; *bm = r.bm; *bn = r.bn; *schedule = r.schedule; *flags = r.flags;
    *launches = g_site_gemm[site].launches;
    return 0;
}
// ---- call-site builders: the GemmParams of the linears every backbone shares.  `site`: the launch is one of the DiT block's four call sites of the
// per-site tile-walk knobs (GemmParams::site = 1 .. 4); the other backbones' linears carry none.
GemmParams gp_linear(const void* A, const void* W, const float* bias, int M, int N, int K) {  // A [M, K] . W [N, K]^T + bias, destination left to the caller
    GemmParams g = gp_zero();
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = bias;
    return g;
}
// input x-projection (EPI_ADD2): h = W_x . x + base -> p->hT and the stream `res`; res16: `res` and the addend (p->base16) hold fp16 elements
GemmParams gp_x_proj(const f5_plan_s* p, int xrows, int rows, void* res, bool res16) {
    GemmParams g = gp_linear(p->xin, p->m->w_x, nullptr, rows, p->m->cfg.dim, MELP);
    g.a_row_mod = xrows < rows ? xrows : 0;
    g.addend = res16 ? reinterpret_cast<const float*>(p->base16) : p->base; g.ldadd = g.N; g.out_t = p->hT; g.ldo = g.N;
    g.out_f = reinterpret_cast<float*>(res); g.ldof = g.N; g.add2_f16 = res16;
    return g;
}
GemmParams gp_pos_conv(const f5_plan_s* p, int li, int rows, int N) {  // position conv li (GEMM_CONV31): hT -> cT (EPI_STORE_T), cT -> yT (EPI_GATE_T)
    const f5_model_s* m = p->m;
    const int D = m->cfg.dim;
    GemmParams g = gp_zero();
    g.A = li == 0 ? p->hT : p->cT; g.lda = D; g.W = m->w_conv[li]; g.M = rows; g.N = D; g.K = 31 * m->conv_win;
    g.bias = m->b_conv[li]; g.act = ACT_MISH; g.rows_per_batch = N; g.conv_cg = m->conv_cg; g.conv_win = m->conv_win;
    g.out_t = li == 0 ? p->cT : p->yT; g.ldo = D;
    return g;
}
GemmParams gp_qkv(const f5_plan_s* p, const void* W, const float* bias, int M, int rpb, const float* rope, bool site) {  // hT -> q|k|v with RoPE (EPI_ROPE_T)
    GemmParams g = gp_linear(p->hT, W, bias, M, 3 * p->m->inner, p->m->cfg.dim);
    g.out_t = p->qkv; g.ldo = g.N; g.rows_per_batch = rpb; g.site = site ? 1 : 0;
    g.rope = rope; g.rope_inner = p->m->inner; g.rope_heads = p->m->rope_heads;
    return g;
}
// out-projection: gate * to_out(cT), 0 where rowmask is 0, as a stored branch `out_t` (EPI_GATE_T) -- or into a stream (gp_resid_stream)
GemmParams gp_out_proj(const f5_plan_s* p, const void* W, const float* bias, int M, int rpb, const float* gate, int gate_bstride, const uint8_t* rowmask,
                       void* out_t, bool site) {
    GemmParams g = gp_linear(p->cT, W, bias, M, p->m->cfg.dim, p->m->inner);
    g.out_t = out_t; g.ldo = out_t ? g.N : 0; g.gate = gate; g.gate_bstride = gate_bstride; g.rows_per_batch = rpb; g.rowmask = rowmask; g.site = site ? 2 : 0;
    return g;
}
GemmParams gp_ff1(const f5_plan_s* p, const void* W, const float* bias, int M, bool site) {  // hT -> gelu(ff.0.0) -> ffh (EPI_STORE_T)
    GemmParams g = gp_linear(p->hT, W, bias, M, p->m->cfg.ff_inner, p->m->cfg.dim);
    g.act = ACT_GELU_TANH; g.out_t = p->ffh; g.ldo = g.N; g.site = site ? 3 : 0;
    return g;
}
GemmParams gp_ff2(const f5_plan_s* p, const void* W, const float* bias, int M, int rpb, const float* gate, int gate_bstride, void* out_t, bool site) {  // as gp_out_proj, from ffh
    GemmParams g = gp_linear(p->ffh, W, bias, M, p->m->cfg.dim, p->m->cfg.ff_inner);
    g.out_t = out_t; g.ldo = out_t ? g.N : 0; g.gate = gate; g.gate_bstride = gate_bstride; g.rows_per_batch = rpb; g.site = site ? 4 : 0;
    return g;
}
GemmParams gp_linear_f32(const void* A, const void* W, const float* bias, int M, int N, int K, float* out) {  // ... stored as fp32 to out [M, N] (EPI_STORE_F32)
    GemmParams g = gp_linear(A, W, bias, M, N, K);
    g.out_f = out; g.ldof = N;
    return g;
}
GemmParams gp_proj_out(const f5_plan_s* p, int M, float* out) { return gp_linear_f32(p->hT, p->m->w_out, p->m->b_out, M, MELP, p->m->cfg.dim, out); }
// points an EPI_RESID site (out-projection, FF2) at the residual stream it updates in place: fp32, or the fp16 stream of the bf16 / fp16 modes
GemmParams gp_resid_stream(GemmParams g, void* stream, bool f16) {
    g.out_t = nullptr; g.out_f = reinterpret_cast<float*>(stream); g.ldof = g.N; g.add2_f16 = f16;
    return g;
}
// a QKV or FF1 site in its LayerNorm-fold form: A = the fp16 stream itself, W' = fp16(W (1 + scale)), c1 = rowsum W', c2 = b + W . shift (gemm.h)
GemmParams gp_folded(GemmParams g, const void* stream16, const void* Wf, const float* c1, const float* c2) {
    g.A = stream16; g.W = Wf; g.bias = nullptr; g.lnf_c1 = c1; g.lnf_c2 = c2;
    return g;
}

// Input embedding of every backbone (dit.py:88-96, mmdit.py:69-79, unett.py:88-98; the cond / text half of the linear is hoisted into `base`):
// h = W_x . x + base -> p->hT and the stream `res` [rows, D]; then mish(conv(mish(conv(h)))) -> p->yT.  The second conv only STORES its branch
// (activation dtype); every fp32 residual add of the network is fused into the pass that follows it (coalesced streaming RMW, store-only GEMM
// epilogues).  tm: the launches are in-situ timing sites (DiT).  Ragged sample() (DiT): the gap rows of what the convs read are zeroed.
int input_embed(f5_plan_s* p, const float* x, int xrows, int rows, int N, void* res, bool res16, bool tm, hipStream_t st) {
    const f5_dit_config& c = p->m->cfg;
    const int P = c.precision;
    const size_t row_bytes = (size_t)c.dim * f5_elem_size(P);
    auto run = [&](int site, const GemmParams& g, int mode, int epi) {
        return tm ? timed(p, site, st, [&] { return run_gemm(p, g, mode, epi, st); }) : run_gemm(p, g, mode, epi, st);
    };
    F5_TRY(launch_convert_pad(P, x, c.mel_dim, xrows, c.mel_dim, MELP, p->xin, MELP, st));
    F5_TRY(run(F5_SITE_INPUT, gp_x_proj(p, xrows, rows, res, res16), GEMM_DENSE, EPI_ADD2));
    if (p->rg) F5_TRY(launch_zero_rows(p->hT, row_bytes, rows, p->gapflag, st));
    F5_TRY(run(F5_SITE_CONV, gp_pos_conv(p, 0, rows, N), GEMM_CONV31, EPI_STORE_T));
    if (p->rg) F5_TRY(launch_zero_rows(p->cT, row_bytes, rows, p->gapflag, st));
    return run(F5_SITE_CONV, gp_pos_conv(p, 1, rows, N), GEMM_CONV31, EPI_GATE_T);
}

float* tap_dst(f5_plan_s* p, const std::string& name) {
    auto it = p->taps.find(name);
    return it == p->taps.end() ? nullptr : it->second;
}
int tap_f32(f5_plan_s* p, const std::string& name, const float* src, int ld, int rows, int cols, hipStream_t st) {
    float* d = tap_dst(p, name);
    if (!d) return 0;
    return launch_convert_back(F5_PREC_FP32, src, ld, rows, cols, d, cols, st);
}
int tap_t(f5_plan_s* p, const std::string& name, const void* src, int ld, int rows, int cols, hipStream_t st) {
    float* d = tap_dst(p, name);
    if (!d) return 0;
    return launch_convert_back(p->m->cfg.precision, src, ld, rows, cols, d, cols, st);
}

int probe_parse(const std::string& name, int depth, int* j, std::string* stage) {
    *j = -1;
    *stage = name;
    if (name == "adaln" || name == "base" || name == "input_embed" || name == "final_norm" || name == "vout") return 0;
    static const char* const kBlockStages[] = {"x_in", "n1", "stats1", "stats2", "qkv", "ctx", "x_attn", "ff1", "x_ff"};
    const size_t dot = name.find('.');
    if (name.compare(0, 3, "blk") == 0 && dot != std::string::npos && dot > 3 && dot <= 3 + 4 &&
        name.find_first_not_of("0123456789", 3) == dot) {
        *j = atoi(name.c_str() + 3);
        *stage = name.substr(dot + 1);
        for (const char* s : kBlockStages)
            if (*stage == s && *j < depth && !(*stage == "x_in" && *j != 0) && !(*stage == "stats1" && *j == 0)) return 0;
    }
    return f5_fail(F5_EINVAL, "unknown stage probe '%s'", name.c_str());
}
int probe_copy(f5_plan_s* p, const std::string& name, int precision, const void* src, int ld, int rows, int cols, hipStream_t st) {
    auto it = p->probes.find(name);
    if (it == p->probes.end()) return 0;
    return launch_convert_back(precision, src, ld, rows, cols, it->second, cols, st);
}

// time values (device, n of them) -> modulation rows [n][modrow] (AdaLN of every block + final), t_emb in p->temb
int compute_modulation(f5_plan_s* p, const float* tvals_dev, int n, hipStream_t st) {
    f5_model_s* m = p->m;
    const int D = m->cfg.dim;
    F5_TRY(launch_time_sinus(tvals_dev, n, p->tsin, st));
    F5_TRY(tap_f32(p, "t_sin", p->tsin, 256, n, 256, st));
    F5_TRY(launch_gemv_rows(p->tsin, 256, n, m->w_t0, m->b_t0, D, 256, 0, 1, p->thid, D, st));  // Linear -> SiLU
    F5_TRY(launch_gemv_rows(p->thid, D, n, m->w_t2, m->b_t2, D, D, 0, 0, p->temb, D, st));      // Linear
    F5_TRY(tap_f32(p, "t_emb", p->temb, D, n, D, st));
    // every AdaLN: Linear(SiLU(t_emb))  (modules.py:311,332); UNetT has none: its layers see the time as a token (unett.py:211-213)
    if (m->modrow > 0) F5_TRY(launch_gemv_rows(p->temb, D, n, m->w_adaln, m->b_adaln, m->modrow, D, 1, 0, p->mod, m->modrow, st));
    if (m->modrow > 0) F5_TRY(tap_f32(p, "adaln", p->mod, m->modrow, n, m->modrow, st));
    return 0;
}

// TextEmbedding.forward (dit.py:49-79) -> out f32 [B*N, td]
int compute_text_embed(f5_plan_s* p, const int32_t* text, int nt, int B, int N, int drop_text, float* out, hipStream_t st) {
    f5_model_s* m = p->m;
    const f5_dit_config& c = m->cfg;
    const int td = c.text_dim, P = c.precision;
    if (c.backbone == F5_BACKBONE_MMDIT) {  // mmdit.py:40-61: [B, nt, dim], not padded to the frame count; table of 1024 positions
        F5_TRY(launch_text_gather(text, nt, B, nt, td, m->text_table, c.text_num_embeds + 1, m->text_pos, m->text_pos_rows, drop_text, out, p->filler, st));
        if (c.text_mask_padding) F5_TRY(launch_mask_rows(out, B * nt, td, p->filler, st));
        return 0;
    }
    const int rows = B * N;
    const bool extra = c.conv_layers > 0;
    F5_TRY(launch_text_gather(text, nt, B, N, td, m->text_table, c.text_num_embeds + 1, extra ? m->text_pos : nullptr, m->text_pos_rows, drop_text, out,
                              p->filler, st));
    if (!extra) return 0;
    const bool mp = c.text_mask_padding != 0;
    if (mp) F5_TRY(launch_mask_rows(out, rows, td, p->filler, st));
    for (int i = 0; i < c.conv_layers; ++i) {
        const TextBlockW& t = m->tblocks[i];
        F5_TRY(launch_dwconv7_ln(P, out, B, N, td, t.dw_wt, t.dw_b, t.ln_w, t.ln_b, p->teT, td, st));
        GemmParams g = gp_linear(p->teT, t.w1, t.b1, rows, 2 * td, td);
        g.act = ACT_GELU_ERF; g.out_t = p->te_h; g.ldo = 2 * td;
        F5_TRY(run_gemm(p, g, GEMM_DENSE, EPI_STORE_T, st));
        F5_TRY(launch_grn(P, p->te_h, B, N, 2 * td, t.gamma, t.beta, p->grn_scratch, st));
        g = gp_linear(p->te_h, t.w2, t.b2, rows, td, 2 * td);
        g.act = ACT_NONE; g.out_f = out; g.ldof = td; g.rows_per_batch = N;
        F5_TRY(run_gemm(p, g, GEMM_DENSE, EPI_RESID, st));
        if (mp) F5_TRY(launch_mask_rows(out, rows, td, p->filler, st));
    }
    return 0;
}

// base[rows, D] = b_in + W_cond . cond + W_text . text_embed for `nb` batch rows starting at row offset row0
int compute_base(f5_plan_s* p, const float* cond, const int32_t* lens, const float* te, int nb, int N, int zero_cond, size_t row0,
                        hipStream_t st, const uint8_t* cmask) {
    f5_model_s* m = p->m;
    const f5_dit_config& c = m->cfg;
    const int D = c.dim, td = m->in_td, P = c.precision, kct = MELP + m->td_pad;  // (columns td .. td_pad stay zero: the arena zero-fills)
    const size_t es = f5_elem_size(P);
    void* ab = (char*)p->abase + row0 * kct * es;
    F5_TRY(launch_pack_base(P, cond, lens, cmask, te, nb, N, c.mel_dim, MELP, td, zero_cond, ab, kct, st));
    F5_TRY(run_gemm(p, gp_linear_f32(ab, m->w_ct, m->b_in, nb * N, D, kct, p->base + row0 * D), GEMM_DENSE, EPI_STORE_F32, st));
    if (p->base16) F5_TRY(launch_f32_to_f16(p->base + row0 * D, (char*)p->base16 + row0 * D * 2, (size_t)nb * N * D, st, plan_res_f16(p) ? p->sat_flag : nullptr));
    return 0;
}


// one network evaluation of whichever backbone the model is (plug point A)
int net_eval(f5_plan_s* p, const float* x, int xrows, int nb, int N, int time_row, int per_batch_rows, const uint8_t* mask, hipStream_t st) {
    f5_model_s* m = p->m;
    p->drop_eval = per_batch_rows ? 0 : time_row;  // (a sample loop's time_row is its evaluation index; a forward is evaluation 0)
    if (m->cfg.backbone == F5_BACKBONE_UNETT)
        return unett_eval(p, x, xrows, nb, N, p->temb + (size_t)time_row * m->cfg.dim, per_batch_rows ? m->cfg.dim : 0, mask, st);
    if (m->cfg.backbone == F5_BACKBONE_MMDIT)
        return mmdit_eval(p, x, xrows, nb, N, p->mod + (size_t)time_row * m->modrow, per_batch_rows ? m->modrow : 0, mask, st);
    p->fold_eval = per_batch_rows ? -1 : time_row;  // (the fold table holds one set of weights per evaluation TIME of the staged grid)
    return dit_eval(p, x, xrows, nb, N, p->mod + (size_t)time_row * m->modrow, per_batch_rows ? m->modrow : 0, mask, st);
}

int check_plan_shape(f5_plan_s* p, int B, int N) {
    if (!p) return f5_fail(F5_EINVAL, "null plan");
    if (B <= 0 || N <= 0 || B > p->maxB || N > p->maxN || (size_t)B * N > (size_t)p->maxB * p->maxN)
        return f5_fail(F5_EINVAL, "shape (B=%d, N=%d) exceeds the plan (B<=%d, N<=%d)", B, N, p->maxB, p->maxN);
    return f5_check_device();
}

// ----------------------------------------------------------------------------- public: text embed / forward
extern "C" int f5_text_embed(f5_plan_t p, int B, int N, const int32_t* text, int nt, int drop_text, float* out, f5_stream_t stream) {
    F5_TRY(check_plan_shape(p, B, N));
    if (!text || !out || nt <= 0) return f5_fail(F5_EINVAL, "null/empty text");
    if (p->m->cfg.backbone == F5_BACKBONE_MMDIT && nt > p->maxN)  // (its B * nt rows use the plan's per-row buffers, as f5_mmdit_forward's do)
        return f5_fail(F5_EINVAL, "text length %d outside 1 .. the plan's max_seq %d", nt, p->maxN);
    return compute_text_embed(p, text, nt, B, N, drop_text, out, (hipStream_t)stream);
}

extern "C" int f5_dit_forward(f5_plan_t p, int B, int N, const float* x, const float* cond, const float* text_embed, const float* time,
                              int drop_audio_cond, const uint8_t* mask, float* out, f5_stream_t stream) {
    F5_TRY(check_plan_shape(p, B, N));
    if (!x || !cond || !text_embed || !time || !out) return f5_fail(F5_EINVAL, "null argument");
    if (p->m->cfg.backbone == F5_BACKBONE_MMDIT) return f5_fail(F5_ENOTSUP, "MMDiT: the text stream has its own length, call f5_mmdit_forward");
    F5_TRY(finish_if_pending(p));
    hipStream_t st = (hipStream_t)stream;
    f5_model_s* m = p->m;
    F5_TRY(dit_probe_check(p, B, N, m->modrow, 1));
    p->mod_tv.clear();  // p->mod is overwritten with per-sample times
    F5_TRY(compute_modulation(p, time, B, st));
    F5_TRY(compute_base(p, cond, nullptr, text_embed, B, N, drop_audio_cond, 0, st));
    F5_TRY(net_eval(p, x, B * N, B, N, 0, 1, mask, st));
    F5_TRY(plan_attn_dropout_advance(p, (uint32_t)plan_depth(p), st));
    p->drop_base_host += p->drop_p > 0.0 ? (uint32_t)plan_depth(p) : 0u;
    return launch_convert_back(F5_PREC_FP32, p->vout, MELP, B * N, m->cfg.mel_dim, out, m->cfg.mel_dim, st);
}

extern "C" int f5_mmdit_forward(f5_plan_t p, int B, int N, int nt, const float* x, const float* cond, const float* text_embed, const float* time,
                                int drop_audio_cond, const uint8_t* mask, float* out, f5_stream_t stream) {
    F5_TRY(check_plan_shape(p, B, N));
    if (!x || !cond || !text_embed || !time || !out) return f5_fail(F5_EINVAL, "null argument");
    if (p->m->cfg.backbone != F5_BACKBONE_MMDIT) return f5_fail(F5_ENOTSUP, "f5_mmdit_forward needs an F5_BACKBONE_MMDIT model");
    if (nt <= 0 || nt > p->maxN) return f5_fail(F5_EINVAL, "text length %d outside 1 .. the plan's max_seq %d", nt, p->maxN);
    hipStream_t st = (hipStream_t)stream;
    f5_model_s* m = p->m;
    p->mod_tv.clear();  // p->mod is overwritten with per-sample times
    F5_TRY(compute_modulation(p, time, B, st));
    F5_TRY(compute_base(p, cond, nullptr, nullptr, B, N, drop_audio_cond, 0, st));
    p->c_src[0] = text_embed;
    p->c_src[1] = nullptr;
    p->c_nt = nt;
    p->c_rows_each = B * nt;
    F5_TRY(net_eval(p, x, B * N, B, N, 0, 1, mask, st));
    F5_TRY(plan_attn_dropout_advance(p, (uint32_t)m->cfg.depth, st));
    p->drop_base_host += p->drop_p > 0.0 ? (uint32_t)m->cfg.depth : 0u;
    return launch_convert_back(F5_PREC_FP32, p->vout, MELP, B * N, m->cfg.mel_dim, out, m->cfg.mel_dim, st);
}

