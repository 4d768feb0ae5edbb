// unett_eval.hip -- one evaluation of the UNetT backbone (reference model/backbones/unett.py:185-253).
#include "model_internal.h"

// one evaluation of the UNetT backbone (reference model/backbones/unett.py:185-253) over `nb` batch rows; temb = time embedding of batch row b at
// temb + b * temb_bstride (stride 0: one time for all).  Result: p->vout [nb * N, MELP] f32 (the time token's row dropped, :246).
// The stream is fp32 (`xres`, read-modify-write by the fp32 EPI_RESID epilogues); activations in the precision's dtype.
int unett_eval(f5_plan_s* p, const float* x, int xrows, int nb, int N, const float* temb, int temb_bstride, const uint8_t* mask, hipStream_t st) {
    f5_model_s* m = p->m;
    const f5_dit_config& c = m->cfg;
    const int D = c.dim, P = c.precision, inner = m->inner, S = N + 1, rows_in = nb * N, rows = nb * S;
    const size_t es = f5_elem_size(P);
    // InputEmbedding (unett.py:88-98): h = proj(cat(x, cond, text)); x = conv_pos_embed(h) + h
    F5_TRY(input_embed(p, x, xrows, rows_in, N, p->xin_res, false, false, st));
    // x = cat([t, x], dim=1); mask = pad(mask, (1, 0), 1)  (:211-214)
    F5_TRY(launch_pack_time_token(P, p->xin_res, p->yT, temb, temb_bstride, nb, N, D, p->xres, st));
    const uint8_t* mask1 = nullptr;
    if (mask) {
        F5_TRY(launch_pad_mask(mask, nb, N, p->mask1, st));
        mask1 = p->mask1;
    }
    const int half = c.depth / 2;
    for (int l = 0; l < c.depth; ++l) {
        const BlockW& b = m->blocks[l];
        if (l < half) {  // skips.append(x)  (:229-230)
            F5_HIP(hipMemcpyAsync(p->skips[l], p->xres, (size_t)rows * D * sizeof(float), hipMemcpyDeviceToDevice, st));
        } else {         // skip = skips.pop()  (:232-238)
            const float* skip = p->skips[c.depth - 1 - l];
            if (c.skip_connect == F5_SKIP_CONCAT) {
                F5_TRY(launch_convert_pad(P, p->xres, D, rows, D, D, p->catT, 2 * D, st));
                F5_TRY(launch_convert_pad(P, skip, D, rows, D, D, (char*)p->catT + (size_t)D * es, 2 * D, st));
                F5_TRY(run_gemm(p, gp_linear_f32(p->catT, b.w_skip, nullptr, rows, D, 2 * D, p->xres), GEMM_DENSE, EPI_STORE_F32, st));
            } else if (c.skip_connect == F5_SKIP_ADD) {
                F5_TRY(launch_add_f32(p->xres, skip, (size_t)rows * D, st));
            }
        }
        // x = attn(attn_norm(x), rope, mask) + x  (:241)
        F5_TRY(launch_rmsnorm(P, p->xres, D, rows, D, b.g_attn, p->hT, D, st));
        F5_TRY(run_gemm(p, gp_qkv(p, b.w_qkv, b.b_qkv, rows, S, p->rope, false), GEMM_DENSE, EPI_ROPE_T, st));
        const AttnDropout drop = plan_attn_dropout(p, l);
        F5_TRY(launch_attention(P, plan_attn_kind(p, S), nb, S, c.heads, p->qkv, 3 * inner, mask1, p->cT, inner, st, 0, 0, &drop));
        // (masked query rows: attention output is 0, modules.py:499-501)
        F5_TRY(run_gemm(p, gp_resid_stream(gp_out_proj(p, b.w_o, b.b_o, rows, S, nullptr, 0, mask1, nullptr, false), p->xres, false), GEMM_DENSE, EPI_RESID, st));
        // x = ff(ff_norm(x)) + x  (:242)
        F5_TRY(launch_rmsnorm(P, p->xres, D, rows, D, b.g_ff, p->hT, D, st));
        F5_TRY(run_gemm(p, gp_ff1(p, b.w_ff1, b.b_ff1, rows, false), GEMM_DENSE, EPI_STORE_T, st));
        F5_TRY(run_gemm(p, gp_resid_stream(gp_ff2(p, b.w_ff2, b.b_ff2, rows, S, nullptr, 0, nullptr, false), p->xres, false), GEMM_DENSE, EPI_RESID, st));
    }
    // x = norm_out(x)[:, 1:, :]; proj_out  (:246-248)
    F5_TRY(launch_rmsnorm(P, p->xres, D, rows, D, m->g_out, p->hT, D, st));
    F5_TRY(run_gemm(p, gp_proj_out(p, rows, p->vout_s), GEMM_DENSE, EPI_STORE_F32, st));
    return launch_drop_time_token(p->vout_s, nb, N, MELP, p->vout, st);
}

