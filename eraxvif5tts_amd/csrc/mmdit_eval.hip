// mmdit_eval.hip -- one evaluation of the MMDiT backbone (reference model/backbones/mmdit.py:146-190, model/modules.py:646-707).
#include "model_internal.h"

// one evaluation of the MMDiT backbone (reference model/backbones/mmdit.py:146-190, MMDiTBlock modules.py:646-707, JointAttnProcessor :509-606) over
// `nb` batch rows.  Two fp32 residual streams: frames `xres` [nb * N, D] and text `cres` [nb * nt, D] (restarted from p->c_src at every
// evaluation: unlike DiT's text embedding the text stream passes through the time-conditioned blocks).  Each block projects both streams with
// their own weights (RoPE per stream, positions from 0), gathers q|k|v into the joint [frames | text] sequence of every utterance, runs one
// attention over it, scatters the result back and applies the gated out-projection / FF updates to each stream in place (EPI_RESID).
int mmdit_eval(f5_plan_s* p, const float* x, int xrows, int nb, int N, const float* modp, int mod_bstride, const uint8_t* mask, hipStream_t st) {
    f5_model_s* m = p->m;
    const f5_dit_config& c = m->cfg;
    const int D = c.dim, P = c.precision, inner = m->inner, nt = p->c_nt, S = N + nt, rows = nb * N, rows_c = nb * nt;
    const size_t es = f5_elem_size(P);
    if (nt <= 0 || !p->c_src[0]) return f5_fail(F5_ESTATE, "MMDiT: no text stream staged");
    // c = text_embed(text)  (:163-173)
    for (int h = 0; h < 2; ++h) {
        const int r0 = h * p->c_rows_each, nr = std::min(rows_c - r0, p->c_rows_each);
        if (nr <= 0) break;
        if (!p->c_src[h]) return f5_fail(F5_ESTATE, "MMDiT: text stream of the second branch missing");
        F5_HIP(hipMemcpyAsync(p->cres + (size_t)r0 * D, p->c_src[h], (size_t)nr * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    // AudioEmbedding (:69-79): h = Linear(cat(x, cond)); x = conv_pos_embed(h) + h   (the cond half of the linear is hoisted into `base`)
    F5_TRY(input_embed(p, x, xrows, rows, N, p->xres, false, false, st));
    const uint8_t* maskJ = nullptr;
    if (mask) {  // modules.py:573: no mask over the text keys
        F5_TRY(launch_joint_mask(mask, nb, N, nt, p->maskJ, st));
        maskJ = p->maskJ;
    }
    const size_t qrow = (size_t)3 * inner * es, arow = (size_t)inner * es;
    // one stream's half block behind the attention, in place (EPI_RESID): stream += gate_msa * to_out(attn), padded query rows of the frames
    // untouched (:596-599); stream += gate_mlp * ff(norm(stream)).  (wo, bo), (w1, b1), (w2, b2): to_out, ff.0.0, ff.2 of the stream; mod: its six AdaLN rows
    auto update = [&](float* stream, int M, int rpb, const void* wo, const float* bo, const void* w1, const float* b1, const void* w2, const float* b2,
                      const float* mod, const uint8_t* rm) -> int {
        F5_TRY(run_gemm(p, gp_resid_stream(gp_out_proj(p, wo, bo, M, rpb, mod + 2 * D, mod_bstride, rm, nullptr, false), stream, false), GEMM_DENSE, EPI_RESID, st));
        F5_TRY(launch_layernorm(P, stream, D, M, D, mod + 4 * D, mod + 3 * D, mod_bstride, rpb, 1, p->hT, D, st));
        F5_TRY(run_gemm(p, gp_ff1(p, w1, b1, M, false), GEMM_DENSE, EPI_STORE_T, st));
        return run_gemm(p, gp_resid_stream(gp_ff2(p, w2, b2, M, rpb, mod + 5 * D, mod_bstride, nullptr, false), stream, false), GEMM_DENSE, EPI_RESID, st);
    };
    for (int l = 0; l < c.depth; ++l) {
        const BlockW& b = m->blocks[l];
        const bool last = l == c.depth - 1;
        const float* mx = modp + (size_t)l * 12 * D;  // attn_norm_x: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp (modules.py:312)
        const float* mc = mx + (size_t)6 * D;         // attn_norm_c: the same six, or (scale, shift) of AdaLayerNorm_Final in the last block (:333)
        // frames: norm_x -> q|k|v with RoPE over positions 0 .. N-1
        if (l == 0)  // (x += position-conv branch, written back)
            F5_TRY(launch_layernorm_add(P, p->xres, D, rows, D, p->yT, D, mx + D, mx, mod_bstride, N, 1, p->hT, D, st));
        else
            F5_TRY(launch_layernorm(P, p->xres, D, rows, D, mx + D, mx, mod_bstride, N, 1, p->hT, D, st));
        F5_TRY(run_gemm(p, gp_qkv(p, b.w_qkv, b.b_qkv, rows, N, p->rope, false), GEMM_DENSE, EPI_ROPE_T, st));
        F5_TRY(launch_copy_segments(p->qkv, (size_t)N * qrow, p->qkvJ, (size_t)S * qrow, (size_t)N * qrow, nb, st));
        // text: norm_c -> q|k|v with RoPE over positions 0 .. nt-1
        F5_TRY(launch_layernorm(P, p->cres, D, rows_c, D, last ? mc : mc + D, last ? mc + D : mc, mod_bstride, nt, 1, p->hT, D, st));
        F5_TRY(run_gemm(p, gp_qkv(p, b.w_qkv_c, b.b_qkv_c, rows_c, nt, p->rope, false), GEMM_DENSE, EPI_ROPE_T, st));
        F5_TRY(launch_copy_segments(p->qkv, (size_t)nt * qrow, (char*)p->qkvJ + (size_t)N * qrow, (size_t)S * qrow, (size_t)nt * qrow, nb, st));
        const AttnDropout drop = plan_attn_dropout(p, l);
        F5_TRY(launch_attention(P, plan_attn_kind(p, S), nb, S, c.heads, p->qkvJ, 3 * inner, maskJ, p->attJ, inner, st, 0, 0, &drop));
        // text: c += gate_msa * to_out_c(attn_c); c += gate_mlp * ff_c(norm)   (:697-706; nothing in the context_pre_only block)
        if (!last) {
            F5_TRY(launch_copy_segments((const char*)p->attJ + (size_t)N * arow, (size_t)S * arow, p->cT, (size_t)nt * arow, (size_t)nt * arow, nb, st));
            F5_TRY(update(p->cres, rows_c, nt, b.w_o_c, b.b_o_c, b.w_ff1_c, b.b_ff1_c, b.w_ff2_c, b.b_ff2_c, mc, nullptr));
        }
        // frames: x += gate_msa * to_out(attn_x) (0 on padded rows); x += gate_mlp * ff_x(norm)   (:709-713)
        F5_TRY(launch_copy_segments(p->attJ, (size_t)S * arow, p->cT, (size_t)N * arow, (size_t)N * arow, nb, st));
        F5_TRY(update(p->xres, rows, N, b.w_o, b.b_o, b.w_ff1, b.b_ff1, b.w_ff2, b.b_ff2, mx, mask));
    }
    const float* mf = modp + (size_t)m->modrow - 2 * D;  // norm_out: (scale, shift) (modules.py:333)
    F5_TRY(launch_layernorm(P, p->xres, D, rows, D, mf, mf + D, mod_bstride, N, 1, p->hT, D, st));
    return run_gemm(p, gp_proj_out(p, rows, p->vout), GEMM_DENSE, EPI_STORE_F32, st);
}
