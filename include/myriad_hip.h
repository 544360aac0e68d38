/* libmyriad_hip.so -- C ABI of the MI355X (gfx950) kernels behind the Myriad / MiniGPT-4 hot path.
 *
 * The reference (tzjtatata/Myriad) has no FFI of its own: every op below replaces a stock PyTorch op sequence
 * inside the reference's nn.Module sub-blocks (file:line cited per entry, paths relative to the reference
 * checkout).  The drop-in boundary one level up is the registered model class (myriad_amd.Myriad / MiniGPT4).
 *
 * Conventions: plain device pointers owned by the caller, explicit dims / leading
 * dimensions in ELEMENTS, explicit hipStream_t, no hidden allocation (workspaces are passed in).  Library state is what
 * the caller registers: the split-K scratch -- in an opaque mh_ctx (mh_ctx_set_workspace + mh_ctx_make_current) or in the
 * process-default record (mh_set_workspace / mh_set_stream_workspace); one scratch per stream that may split K: two streams
 * must not share one -- the launch profiler's event pool (mh_prof_*, off unless started) and the option table below
 * (mh_set_option / mh_get_option: on/off switches between equivalent code paths, each defaulting to the measured-best setting).
 * The shipped library exports nothing else: the timing probes and sweep switches of tools/ (mhdbg_*) are compiled only into
 * libmyriad_hip_dbg.so (-DMH_DEBUG_HOOKS).  Calls on different streams with their own scratch are independent.
 * Every function returns 0 on success or a negative MH_ERR_* code and never throws.
 * bf16 tensors are raw uint16 bit patterns; "f32" means IEEE float.
 */
#ifndef MYRIAD_HIP_H
#define MYRIAD_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mh_stream_t; /* == hipStream_t */

#define MH_OK 0
#define MH_ERR_ARG (-1)
#define MH_ERR_LAUNCH (-2)
#define MH_ERR_UNSUPPORTED (-3)

/* mh_gemm_bf16_nt flags */
#define MH_GEMM_OUT_F32 1  /* C is f32 (else bf16) */
#define MH_GEMM_GELU 2     /* erf-GELU after bias, before residual */
#define MH_GEMM_REGSTAGE 4 /* register-staged LDS fill instead of LDS-DMA (A/B testing) */

/* K1/K2  C[M,N] = alpha * A[M,K] . B[N,K]^T (+bias[N]) (GELU) (+residual[M,N] f32).  A,B bf16, K % 64 == 0.
 * Replaces every nn.Linear on the path: eva_vit.py:124,146,55-59; Qformer.py:127-133,281,352,367;
 * myriad.py:263 (llama_proj); modeling_llama.py:134-136,159-162,604; and their autograd dgrad/wgrad. */
int mh_gemm_bf16_nt(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                    const float* bias, const float* residual, int ldr, int flags, float alpha, mh_stream_t s);

/* Which kernel mh_gemm_bf16_nt will launch for this shape and with how many K splits (splits > 1 adds one
 * fixed-order reduce launch): *kernel = 0 weight-streaming gemv (M <= 16), 1 = 128x128x64 tile (gemm_nt_kernel),
 * 2 = 256x256x64 tile, eight waves, hand-scheduled K loop (gemm_x8_kernel; gemm_256_kernel, the 256x256x32 kernel of
 * rounds 1-3, only for operands whose byte offsets pass 2 GiB or with option gemm256_impl = 0), 3 = gemm_nt_kernel with a
 * 128x64 tile (grids that leave most CUs empty), 4 / 5 = gemm_nt_kernel with a 160x128 / 160x96 tile and a 4-deep ring
 * (128 < M <= 320: the batch-1 step's 148 / 257 rows as one / two row tiles, the weight streamed once), 6 = gemm_nt_kernel
 * with a 64x64 tile and an 8-deep ring (one-round grids with K <= 3072).
 * For profilers and benchmarks that attribute time per kernel. */
int mh_gemm_plan(int M, int N, int K, int flags, int* kernel, int* splits);

/* Launch profiler (`roofline.achieved` is per launch of the dominant kernel): between mh_prof_start and
 * mh_prof_stop every launch of gemm_x8_kernel / gemm_256_kernel / gemm_nt_kernel is bracketed by two HIP events on the stream it is launched
 * on -- the kernel alone, also when it is the partial-product launch of a split-K op.  Launches inside a stream capture are
 * skipped.  mh_prof_stop waits for the device and writes, per recorded launch i, meta[6i..6i+5] = (kernel id as
 * mh_gemm_plan numbers them, M, N, K, K splits, flags) and ms[i]; returns the number of records (<= cap).  The events
 * (2 per record) are created once and reused.  One host thread.  Both calls launch a one-wave no-op kernel
 * (mh_prof_marker_kernel) on `s`, so that a rocprofv3 kernel trace of the same run shows where the profiled region lies. */
int mh_prof_start(int capacity, mh_stream_t s);
double mh_prof_overhead_ms(void); /* median of 33 EMPTY event pairs timed by the last mh_prof_start: what a pair adds to a launch */
int mh_prof_stop(int* meta, float* ms, int cap, mh_stream_t s);

/* Linear + residual add + the RMSNorm that consumes the sum (modeling_llama.py:281-293 then :66-74 of the next block):
 * H[M,N] = A.B^T + residual (f32, the new residual stream), Y[M,N] = bf16(norm_w * H * rsqrt(mean(H^2) + eps)).
 * When the GEMM is split along K the slab reduction, the residual add and the norm run as ONE kernel; otherwise this is
 * mh_gemm_bf16_nt followed by mh_rmsnorm_fwd.  Both forms give bit-identical H and Y. */
int mh_gemm_residual_rmsnorm(const void* A, int lda, const void* B, int ldb, float* H, int ldh, const float* residual,
                             int ldr, const float* norm_w, float eps, void* Y, long ldy, int M, int N, int K,
                             mh_stream_t s);

/* Same for the pre-LN ViT blocks (eva_vit.py:173-180; ImageBind transformer.py:160-163): H = A.B^T + bias + residual,
 * Y = bf16(LayerNorm(H) * norm_w + norm_b), dense [M,N] outputs. */
int mh_gemm_residual_layernorm(const void* A, int lda, const void* B, int ldb, float* H, int ldh, const float* bias,
                               const float* residual, int ldr, const float* norm_w, const float* norm_b, float eps, void* Y,
                               int M, int N, int K, mh_stream_t s);
/* dY = A.B^T (a dgrad Linear) followed by the RMSNorm backward that consumes it: dx = d rmsnorm(x; w)(dY) + dres, written
 * as f32 (dx) and/or bf16 (dx_bf16).  dy_buf: [M, N] f32 scratch (used when K is not split).  Same bits as
 * mh_gemm_bf16_nt(..., MH_GEMM_OUT_F32) + mh_rmsnorm_bwd; one launch and one pass over dY less when K is split. */
int mh_gemm_rmsnorm_bwd(const void* A, int lda, const void* B, int ldb, float* dy_buf, const float* x, const float* w,
                        const float* dres, float* dx, void* dx_bf16, int M, int N, int K, float eps, mh_stream_t s);
/* The LayerNorm counterpart (the backward of mh_gemm_residual_layernorm): dY = A.B^T, dx = d layernorm(x; w)(dY) + dres as
 * f32 (dx) and/or bf16 (dx_bf16).  dy_buf: [M, N] f32 scratch; it holds dY on return when dgamma != NULL.  dgamma / dbeta
 * (f32 [N], both or neither, N <= 4096): the LayerNorm's parameter gradients, (+)= when accumulate, from per-block partials in
 * ws (mh_layernorm_param_grads_ws_floats(M, N) floats) reduced in block order.  Same bits as mh_gemm_bf16_nt(...,
 * MH_GEMM_OUT_F32) + mh_layernorm_bwd (+ mh_layernorm_param_grads); the split-K partials are summed inside the norm kernel. */
int mh_gemm_layernorm_bwd(const void* A, int lda, const void* B, int ldb, float* dy_buf, const float* x, const float* w,
                          const float* dres, float* dx, void* dx_bf16, float* dgamma, float* dbeta, int accumulate, float* ws,
                          long ws_floats, int M, int N, int K, float eps, mh_stream_t s);

/* Scratch for the automatic split-K path of mh_gemm_bf16_nt (used for shapes whose tile count under-fills the
 * 256 CUs).  The caller owns the buffer; pass NULL to disable.  Not needed for correctness. */
int mh_set_workspace(void* ptr, long bytes);
/* Further scratches (each >= the first one's size) for launches on other streams (up to 4), so that a frozen forward or a
 * leaf backward can run beside the main stream without sharing split-K slabs with it.  ptr = NULL unregisters. */
int mh_set_stream_workspace(mh_stream_t stream, void* ptr, long bytes);
/* split-K variant (f32 out, no epilogue) for skinny outputs with a long reduction (conv-stem wgrad):
 * ws holds mh_gemm_splitk_ws_floats(M,N,splits) floats; fixed-order reduction -> deterministic. */
long mh_gemm_splitk_ws_floats(int M, int N, int splits);
int mh_gemm_bf16_nt_splitk(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                           int splits, float* ws, mh_stream_t s);

/* K3/K4/K5 fused attention.  q/k/v/o token-major [B,S,ld] bf16, head h at columns [h*D,(h+1)*D); D in
 * {<=64, <=96 (88), <=128}; lse [B,H,Sq] f32; bias optional additive [H,Sq,Sk] f32 (eva_vit.py:131-140);
 * kv_len optional [B] valid-key counts (right padding, modeling_llama.py:43-54); causal aligns the last query
 * with the last key (KV-cache decode: Sq=1).  With Sq = 1 a row whose kv_len[b] <= 0 gets a zero o row and lse = -inf, and a
 * kv_len[b] > Sk counts as Sk.  Replaces eva_vit.py:125-145, Qformer.py:195-262, modeling_llama.py:197-222 and their autograd. */
int mh_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const float* bias,
                const int* kv_len, int B, int H, int Sq, int Sk, int D, long q_bs, int ldq, long k_bs, int ldk,
                long v_bs, int ldv, long o_bs, int ldo, float scale, int causal, mh_stream_t s);
/* Q-Former attention with attention-probability dropout (train mode): O = (P . Z) V with the LSE of the undropped P;
 * backward dV = (P . Z)^T dO, dP = (dO V^T) . Z, delta from the dropped O.  Z[b,h,i,j] = dropout_keep(seed,
 * ((b*H + h)*Sq + i)*Sk + j).  No bias / padding / causal mask.  p = 0 callers use mh_attn_fwd / mh_attn_bwd. */
int mh_attn_fwd_dropout(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Sq, int Sk, int D,
                        long q_bs, int ldq, long k_bs, int ldk, long v_bs, int ldv, long o_bs, int ldo, float scale,
                        float drop_p, unsigned long long seed, mh_stream_t s);
int mh_attn_bwd_dropout(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                        float* delta_ws, void* dq, void* dk, void* dv, int B, int H, int Sq, int Sk, int D, long q_bs, int ldq,
                        long k_bs, int ldk, long v_bs, int ldv, long o_bs, int ldo, long do_bs, int lddo, long dq_bs,
                        int lddq, long dk_bs, int lddk, long dv_bs, int lddv, float scale, float drop_p,
                        unsigned long long seed, mh_stream_t s);
int mh_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                float* delta_ws /* [B,H,Sq] f32 scratch */, void* dq, void* dk, void* dv, const float* bias,
                const int* kv_len, int B, int H, int Sq, int Sk, int D, long q_bs, int ldq, long k_bs, int ldk,
                long v_bs, int ldv, long o_bs, int ldo, long do_bs, int lddo, long dq_bs, int lddq, long dk_bs,
                int lddk, long dv_bs, int lddv, float scale, int causal, mh_stream_t s);

/* K5 + K8 fused, training path: LLaMA causal self-attention with the rotary embedding applied on load
   (modeling_llama.py:109-123 apply_rotary_pos_emb, :168-231 LlamaAttention.forward).  qkv = [q | k | v] [B, S, ld] bf16,
   PRE-rotary, head h at columns h*D..; one workgroup per (batch, head) holds the whole sequence (S <= 160, D = 128:
   mh_attn_rope_supported; otherwise MH_ERR_UNSUPPORTED and the caller uses mh_rope_inplace + mh_attn_fwd/bwd).
   pos [B*S] position ids, cos/sin [max_pos, D/2] f32, kv_len optional [B] (right padding).  bwd writes
   dqkv = [dq | dk | dv] with dq, dk already un-rotated.  mh_gemm_attn_rope_bwd = the o_proj dgrad GEMM
   dO = A[M,K].Bw[N,K]^T followed by that backward, with the split-K partial sums of dO added up inside the attention
   kernel (do_buf [M, N] bf16 is scratch for the unsplit case). */
int mh_attn_rope_supported(int S, int D);
int mh_attn_rope_fwd(const void* qkv, int ld, void* o, int ldo, float* lse, const int* pos, const float* cos_tab,
                     const float* sin_tab, const int* kv_len, int B, int H, int S, int D, float scale, mh_stream_t s);
int mh_attn_rope_bwd(const void* qkv, int ld, const void* o, int ldo, const void* dout, int ldd, const float* lse,
                     void* dqkv, const int* pos, const float* cos_tab, const float* sin_tab, const int* kv_len,
                     int B, int H, int S, int D, float scale, mh_stream_t s);
int mh_gemm_attn_rope_bwd(const void* A, int lda, const void* Bw, int ldb, void* do_buf, int K, const void* qkv,
                          int ld, const void* o, int ldo, const float* lse, void* dqkv, const int* pos,
                          const float* cos_tab, const float* sin_tab, const int* kv_len, int B, int H, int S,
                          int D, float scale, mh_stream_t s);

/* K7 RMSNorm (modeling_llama.py:66-74) f32 in -> bf16 out; bwd is dgrad-only (+ optional residual-grad add,
 * optional bf16 copy of dx for the next dgrad GEMM). */
int mh_rmsnorm_fwd(const float* x, const float* w, void* y_bf16, long ldy, int M, int D, float eps, mh_stream_t s);
int mh_rmsnorm_bwd(const float* dy, const float* x, const float* w, const float* dres, float* dx, void* dx_bf16,
                   int M, int D, float eps, mh_stream_t s);
/* K6 LayerNorm (eva_vit.py:175-176; blip2.py:119-125; Qformer.py:106,288,374) f32 in -> bf16 and/or f32 out.
 * mh_layernorm_bwd is dgrad-only (+ optional residual-grad add, optional bf16 copy of dx): one kernel, the one that
 * mh_gemm_layernorm_bwd feeds split-K slabs, here with a single slab.  It holds the row in registers, so D % 4 == 0 and
 * D <= 8192 (MH_ERR_ARG otherwise, nothing written); the forward takes any D % 4 == 0. */
int mh_layernorm_fwd(const float* x, const float* w, const float* b, void* y_bf16, float* y_f32, int M, int D,
                     float eps, mh_stream_t s);
int mh_layernorm_bwd(const float* dy, const float* x, const float* w, const float* dres, float* dx, void* dx_bf16,
                     int M, int D, float eps, mh_stream_t s);
/* K31 LayerNorm parameter gradients (trainable Q-Former): dgamma (+)= sum_m dy * xhat, dbeta (+)= sum_m dy, xhat recomputed
 * from the LayerNorm input x [M,D] f32.  ws: mh_layernorm_param_grads_ws_floats(M, D) floats of scratch (per-block partials,
 * reduced in block order: deterministic).  D % 4 == 0, D <= 4096. */
long mh_layernorm_param_grads_ws_floats(int M, int D);
int mh_layernorm_param_grads(const float* dy, const float* x, float* dgamma, float* dbeta, int M, int D, float eps,
                             int accumulate, float p_out, unsigned long long seed_out, float* ws, long ws_floats,
                             mh_stream_t s);
/* K32 Q-Former hidden dropout fused into the LayerNorm (qf_dropout.hip).  fwd: x = z * keep(seed_in) + res (res != NULL; x
 * written to x_out, the backward's LayerNorm input) or x = z; y = LN(x) * keep(seed_out).  bwd (x = the LayerNorm input):
 * g = dy * keep(seed_out); dx = LN'(g) in f32 (the residual's gradient), dz_bf16 = dx * keep(seed_in) (the GEMM's).
 * keep(seed)[m, d] = dropout_keep(seed, m * D + d): 1/(1-p) or 0, and 1 at p = 0.  mh_dropout_keep_mask writes
 * keep(seed)[i] for i < n. */
int mh_layernorm_fwd_dropout(const float* z, const float* res, const float* w, const float* b, float* x_out, void* y_bf16,
                             float* y_f32, int M, int D, float eps, float p_in, unsigned long long seed_in, float p_out,
                             unsigned long long seed_out, mh_stream_t s);
int mh_layernorm_bwd_dropout(const float* dy, const float* x, const float* w, float* dx, void* dz_bf16, int M, int D,
                             float eps, float p_in, unsigned long long seed_in, float p_out, unsigned long long seed_out,
                             mh_stream_t s);
int mh_dropout_keep_mask(float* out, long n, float p, unsigned long long seed, mh_stream_t s);
/* K33 stochastic depth in the trainable EVA ViT (drop_path.hip; eva_vit.py:162,173-176, timm drop_path with scale_by_keep).
 * A branch runs on the K kept samples of the batch only: its matrices are COMPACT, [K*N, *] (N rows a sample, batch order); the
 * residual stream stays full, [B*N, D] f32.  A map is a HOST array slot[B]: slot[b] = the compact sample index of sample b, or
 * -1 when b is not in the set.  It is checked here (every kept sample names one of 0 .. K-1, each exactly once, K = the count
 * given) and travels in the kernel arguments: B <= 64 (MH_ERR_UNSUPPORTED above), a bad map is MH_ERR_ARG and nothing is launched.
 * A NULL map with K = B means every sample in order.  D % 4 == 0, D <= 8192 (the parameter gradients: D <= 4096).
 *   residual_layernorm: h_out[r] = h[r] + scale * y[compact row] for the samples of slot_in, h[r] (same bits) for the others;
 *       then xn = LayerNorm(h_out; w, b) as bf16 for the samples of slot_out, at their compact rows.  y == NULL (K_in = 0): no
 *       branch, h_out may be NULL; xn == NULL (K_out = 0): no norm.  h_out must not be h.
 *   layernorm_bwd: dx[r] = dres[r] + LayerNorm backward of dy[compact row] at x[r] for the samples of slot_in, dres[r] (same
 *       bits) for the others; dx_bf16 (optional) = bf16(out_scale * dx) for the samples of slot_out at their compact rows.
 *   gather_scale: dst = bf16(scale * src) for the samples of slot_out at their compact rows.
 *   layernorm_param_grads: dgamma (+)= sum dy * xhat, dbeta (+)= sum dy over the compact rows (dy compact [K*N, D], x full); 16
 *       rows a block, blocks reduced in order: deterministic.  ws: mh_drop_path_param_grads_ws_floats(K, N, D) floats. */
int mh_drop_path_residual_layernorm(const float* h, const float* y, const int* slot_in, int K_in, float scale, const float* w,
                                    const float* b, const int* slot_out, int K_out, float* h_out, void* xn_bf16, int B, int N,
                                    int D, float eps, mh_stream_t s);
int mh_drop_path_layernorm_bwd(const float* dy, const float* x, const float* w, const float* dres, const int* slot_in, int K_in,
                               const int* slot_out, int K_out, float out_scale, float* dx, void* dx_bf16, int B, int N, int D,
                               float eps, mh_stream_t s);
int mh_drop_path_gather_scale(const float* src, const int* slot_out, int K_out, float scale, void* dst_bf16, int B, int N, int D,
                              mh_stream_t s);
long mh_drop_path_param_grads_ws_floats(int K, int N, int D);
int mh_drop_path_layernorm_param_grads(const float* dy, const float* x, const int* slot_in, int K_in, float* dgamma, float* dbeta,
                                       int B, int N, int D, float eps, int accumulate, float* ws, long ws_floats, mh_stream_t s);
/* K30 TN weight-gradient GEMM (trainable Q-Former): out[N,K] (+)= dy^T . x with dy [M,N] (row stride lddy) and x [M,K]
 * (row stride ldx) row-major bf16, fp32 accumulation into out (row stride ldo); accumulate = 0 overwrites.  bias != NULL: the
 * fused bias gradient bias[N] (+)= sum_m dy[m,:].  N % 64 == K % 64 == 0, lddy / ldx multiples of 8, dy / x 16-byte aligned;
 * any M.  splits: M splits (0 = mh_gemm_tn_wgrad_auto_splits); splits > 1 need mh_gemm_tn_wgrad_ws_floats(...) floats of
 * scratch in ws and reduce in split order (bit-identical run to run). */
long mh_gemm_tn_wgrad_ws_floats(int M, int N, int K, int splits);
int mh_gemm_tn_wgrad_auto_splits(int M, int N, int K);
int mh_gemm_tn_wgrad(const void* dy, long lddy, const void* x, long ldx, float* out, long ldo, float* bias, int M, int N, int K,
                     int accumulate, int splits, float* ws, long ws_floats, mh_stream_t s);

/* K8 rotary, rotate-half form gathered by position id (modeling_llama.py:109-123); in place on heads
 * [col0, col0 + n_heads*head_dim) of a [n_tok, ld] bf16 buffer; tables [max_pos, head_dim/2] f32; sign=-1 = bwd. */
int mh_rope_inplace(void* x, int ld, int col0, int n_tok, int n_heads, int head_dim, const int* pos,
                    const float* cos_tab, const float* sin_tab, float sign, mh_stream_t s);
/* K9 SiLU-gated MLP elementwise (modeling_llama.py:139-140): gu = [M, 2I] = [gate | up] bf16. */
int mh_silu_mul_fwd(const void* gu, void* h, int M, int I, mh_stream_t s);
int mh_silu_mul_bwd(const void* dh, const void* gu, void* dgu, int M, int I, mh_stream_t s);
/* the same with gate / up interleaved in blocks of `blk` columns ([g 0..blk-1 | u 0..blk-1 | g blk.. ]; blk = 0: the halves
   layout above), and the SiLU-gated MLP fused into the GEMMs around it (modeling_llama.py:139-140): gu[M, 2I] = X Wgu^T with
   Wgu's rows interleaved in blocks of 128, act[M, I] = silu(g) * u from the gate|up GEMM's epilogue; dgu = silu_mul_bwd(dH
   WdT^T, gu) from the down projection's dgrad epilogue (dact_buf [M, I] bf16: scratch when the policy does not run the fused
   kernel).  Same bits as GEMM + mh_silu_mul_*_blk. */
int mh_silu_mul_fwd_blk(const void* gu, void* h, int M, int I, int blk, mh_stream_t s);
int mh_silu_mul_bwd_blk(const void* dh, const void* gu, void* dgu, int M, int I, int blk, mh_stream_t s);
int mh_gemm_swiglu_fwd(const void* X, int ldx, const void* Wgu, int ldw, void* gu, int ldgu, void* act, int ldact, int M,
                       int I, int K, mh_stream_t s);
int mh_gemm_swiglu_bwd(const void* dH, int lddh, const void* WdT, int ldw, const void* gu, int ldgu, void* dgu, int lddgu,
                       void* dact_buf, int M, int I, int K, mh_stream_t s);
/* erf-GELU on bf16 (Qformer.py:352-356 via ACT2FN["gelu"]) */
int mh_gelu_fwd(const void* x, void* y, long n, mh_stream_t s);
int mh_gelu_bwd(const void* dy, const void* x, void* dx, long n, mh_stream_t s);
/* the erf-GELU MLP (Qformer.py:481-484: intermediate_query -> gelu -> output_query; eva_vit.py:54-61) with the elementwise half in
   the epilogue of the GEMM next to it: pre[M, N] = X W^T + bias (bf16, kept for the backward) and act = gelu(pre) in one launch;
   dpre = bf16(dY WT^T) * gelu'(pre) in one launch.  Fused when the policy runs an unsplit tile kernel, otherwise GEMM + mh_gelu_*
   (dact_buf [M, N] bf16: scratch for that case; dense rows required then).  Same bits as the separate launches. */
int mh_gemm_gelu_fwd(const void* X, int ldx, const void* W, int ldw, const float* bias, void* pre, int ldpre, void* act, int ldact,
                     int M, int N, int K, mh_stream_t s);
int mh_gemm_gelu_bwd(const void* dY, int lddy, const void* WT, int ldw, const void* pre, int ldpre, void* dpre, int lddpre,
                     void* dact_buf, int M, int N, int K, mh_stream_t s);

/* counter-based dropout for PEFT lora_dropout (myriad.py:171-178): mask = f(seed, flat index); bwd regenerates it */
int mh_dropout_bf16(const void* x, long ldx, void* y, long ldy, long rows, int cols, float p, unsigned long long seed,
                    mh_stream_t s);
int mh_dropout_add_f32(const float* dy, long lddy, float* acc, long ldacc, long rows, int cols, float p,
                       unsigned long long seed, mh_stream_t s);

/* K10 (PEFT form) LoRA on q_proj/v_proj, y = W x + (alpha/r) B (A dropout(x)) (myriad.py:170-180).  The UP projection
 * rides the qkv GEMM as a 64-column K border; these kernels do the skinny parts.  A = [R2, D] f32 (A_q rows then A_v
 * rows, R2 = 2r in {16,32}); border / dborder = columns [D, D+R2) of the bordered operand / its gradient. */
int mh_lora_down(const void* x, long ldx, const float* A, void* border, long ldo, int M, int D, int R2, float s, float p,
                 unsigned long long seed, mh_stream_t st);
int mh_lora_dx(const float* dx_ext, long ld, const float* A, float* out, int M, int D, int R2, float s, float p,
               unsigned long long seed, mh_stream_t st);
/* Head of a single-token decode step with LoRA attached (M <= 2 rows, no dropout): x_ext[:, :D] = bf16(rmsnorm(h; w, eps)) and
 * x_ext[:, D:D+64] = its LoRA border, one launch with the bits of mh_rmsnorm_fwd + mh_lora_down (LlamaRMSNorm,
 * modeling_llama.py:66-74, in front of the peft q_proj / v_proj).  MH_ERR_UNSUPPORTED for M > 2 or D > 4096. */
int mh_rmsnorm_lora_down(const float* h, long ldh, const float* norm_w, float eps, const float* A, void* x_ext, long ldx, int M,
                         int D, int R2, float s, mh_stream_t st);
/* The qkv dgrad with the LoRA border, [M, D+64] = dqkv . [W_qkv | B_ext]^T-layout operand (myriad.py:170-180 under autograd),
 * and the LoRA dx correction that reads it, in one call: when mh_gemm_plan(M, D+64, K) splits K the correction kernel sums the
 * fp32 partial slabs itself (no reduce launch, same bits) and writes the summed border d(s*t) [M, 64] to border_out; otherwise
 * the product goes through dx_ext_buf [M, D+64] (which then holds the border) and border_out is left alone. */
int mh_gemm_lora_dx(const void* A, int lda, const void* Bw, int ldb, float* dx_ext_buf, const float* loraA, float* dxn,
                    float* border_out, int M, int D, int K, int R2, float s, float p, unsigned long long seed, mh_stream_t stream);
/* mh_gemm_lora_dx followed by the backward of the RMSNorm whose output the qkv projection read (the layer's input norm,
 * modeling_llama.py:66-74, 257-259 under autograd): dx = d rmsnorm(x; w)(dxn) + dres as f32 (dx) and / or bf16 (dx_bf16).
 * With D <= 4096 and R2 = 16 the LoRA correction and the norm backward are ONE kernel that also sums the dgrad's split-K
 * slabs (the [M, D] f32 dxn never exists); otherwise, or with option lora_norm_fused = 0, mh_lora_dx and mh_rmsnorm_bwd run
 * back to back through dxn_buf [M, D] f32.  Same bits either way.  dx_ext_buf / border_out as in mh_gemm_lora_dx. */
int mh_gemm_lora_rmsnorm_bwd(const void* A, int lda, const void* Bw, int ldb, float* dx_ext_buf, const float* loraA,
                             float* dxn_buf, float* border_out, const float* x, const float* w, const float* dres, float* dx,
                             void* dx_bf16, int M, int D, int K, int R2, float s, float p, unsigned long long seed, float eps,
                             mh_stream_t stream);
long mh_lora_wgrad_ws_floats(int D, int R2);
int mh_lora_wgrad(const void* x, long ldx, const float* dx_ext, long ldg, const void* dq, const void* dv, long ldq,
                  const void* border, long ldb, float* dA, float* dBq, float* dBv, float* ws, int M, int D, int R2,
                  float s, float p, unsigned long long seed, mh_stream_t st);
int mh_lora_refresh_border(const float* Bq, const float* Bv, void* ext, long ld_ext, void* extT, long ld_extT, int W,
                           int D, int r, mh_stream_t st);
/* The same for every layer in one launch: table = device array of n_layers x {B_q, B_v, W_ext, W_ext^T or NULL} pointers
 * (4 x 8 bytes per layer), all layers sharing the two row strides. */
int mh_lora_refresh_borders(const void* table, int n_layers, long ld_ext, long ld_extT, int W, int D, int r, mh_stream_t stream);

/* K10 rank-r adaptor y = x + (x A^T) B^T (networks.py:81-93), f32, r in {1,2,4,8}. */
int mh_lowrank_fwd(const float* x, const float* A, const float* Bm, float* y, float* t, int M, int D, int R,
                   mh_stream_t s);
long mh_lowrank_bwd_ws_floats(int M, int D, int R);
int mh_lowrank_bwd(const float* dy, const float* x, const float* t, const float* A, const float* Bm, float* dA,
                   float* dB, float* dx, float* ws, int M, int D, int R, mh_stream_t s);

/* K11 clamp-CE (modeling_llama.py:718-728) per-row loss + fused d(logits) (bf16, zero-padded to ldd). */
int mh_clamp_ce(const float* logits, long ldl, const long* labels, float* row_loss, void* dlogits_bf16, long ldd,
                int R, int V, float grad_scale, mh_stream_t s);
int mh_sum_f32(const float* x, float* out, long n, float scale, mh_stream_t s);
/* greedy step (evaluation_aqa_dataset.py:289-301 top_p=0.01 == arg-max; min_length ban of EOS) */
int mh_argmax_rows(const float* logits, long ldl, long* out, float* margin, int R, int V, int ban_id, mh_stream_t s);
/* the same plus p_max[row] = softmax(logits * inv_temp)[argmax] (banned id excluded): tells whether HF's
   `do_sample=True, top_p=p` is the arg-max (p_max >= p keeps exactly one token) -- generation_kwargs of the eval script */
int mh_argmax_pmax_rows(const float* logits, long ldl, long* out, float* margin, float* pmax, int R, int V, int ban_id,
                        float inv_temp, mh_stream_t s);
/* end of a decode step on the device: rec[3][R] f32 = (ids, margins, p_max) of this step in one small record, next_ids = ids
   (the next step's input: myriad.py:433-454's feed-back of the generated token), *step += 1 -- the token step needs no host
   input and the host fetches a step with one copy */
int mh_decode_record(const long* nxt, const float* margin, const float* pmax, float* rec, long* next_ids, int* step, int R,
                     mh_stream_t s);
/* the same plus pos[r] += 1 and kvlen[r] += 1 (the decode step's device-resident rotary position and valid-key count, one int per
   row): the step's three bookkeeping launches as one */
int mh_decode_advance(const long* nxt, const float* margin, const float* pmax, float* rec, long* next_ids, int* step, int* pos,
                      int* kvlen, int R, mh_stream_t s);
/* sampled decode step (HF generate(do_sample=True), conversation.py:144-168's chat call: TopK -> TopP -> multinomial, after the
   min_length ban and TemperatureLogitsWarper), one workgroup per row, V <= 32768, ldl % 4 == 0, 16-byte aligned rows (else
   MH_ERR_UNSUPPORTED).  params[4] f32 on the device = (inv_temp, top_p, top_k, penalty): tokens below the k-th largest tempered
   logit go (ties at it all stay), then every token whose exclusive prefix mass in (logit desc, id asc) order reaches top_p (the
   largest always stays); out[r] = the smallest i of that kept set with inclusive mass > u * (kept mass).  u from Philox4x32-10,
   key = *seed (u64 on the device), counter = ((step ? *step : 0) + t_add, 0, r, 0): u = (x0 >> 8) * 2^-24, written to u_out[r]
   when u_out is given.  margin / pmax as mh_argmax_pmax_rows (same bits); kept[r] = size of the kept set, or -1 when the tied
   top-k set has more than 1024 members (out[r] is then the arg-max and the caller draws the row).
   Values that have no order of their own:
   - -0.0 and +0.0 are one value for the top-k threshold, the tie set and the (logit desc, id asc) order.
   - a NaN logit, of either sign, is -inf for the draw: never a candidate, no mass, never out[r].  margin / pmax stay what
     mh_argmax_pmax_rows computes on that row (NaN does not win the arg-max there either; p_max of such a row is NaN).
   - a row holding +inf (after the ban): out[r] = the arg-max, the lowest id holding +inf, and kept[r] = 1 whatever top_p is.  A
     finite logit that the temperature pushes to +inf counts the same way: the lowest such id, alone.
   - a row with nothing finite left after the ban (all -inf / NaN): kept[r] = -1 and out[r] = the arg-max rule's answer, id 0
     for an all -inf row. */
int mh_sample_rows(const float* logits, long ldl, long* out, float* margin, float* pmax, int* kept, float* u_out, int R, int V,
                   int ban_id, const float* params, const unsigned long long* seed, const int* step, int t_add, mh_stream_t s);
/* HF RepetitionPenaltyLogitsProcessor in place on f32 logits [R, ldl]: seen = R x ceil(V/32) u32 bitmap of the ids generated so
   far (zeroed by the caller once per generate); prev_ids[r] (when given) is added first, then every seen id's logit becomes
   x * p (x < 0) or x / p, p = *penalty (device scalar) -- each id once however often it was generated */
int mh_repetition_penalty_rows(float* logits, long ldl, unsigned* seen, const long* prev_ids, int R, int V, const float* penalty,
                               mh_stream_t s);
/* mh_decode_advance with the sampler's kept count as a fourth record row: rec[4][R] f32 = (ids, margins, p_max, kept) */
int mh_decode_advance_kept(const long* nxt, const float* margin, const float* pmax, const int* kept, float* rec, long* next_ids,
                           int* step, int* pos, int* kvlen, int R, mh_stream_t s);
/* mh_decode_advance under a row mask (the slot engine's token step, live int[R] on the device): a row with live[r] != 0 advances
   as above; an idle row records (-1, 0, 0) and keeps next_ids[r], pos[r] and kvlen[r].  *step += 1 once per launch. */
int mh_decode_advance_rows(const long* nxt, const float* margin, const float* pmax, float* rec, long* next_ids, int* step,
                           int* pos, int* kvlen, const int* live, int R, mh_stream_t s);
/* The sampled step of the decode-slot engine: mh_sample_rows with per-row state on the device.  params[6] f32 = (inv_temp, top_p,
   top_k, penalty, min_length, eos_id); seed[r] (u64) is row r's Philox key and gen[r] (the tokens its request has generated so
   far) the step of its draw, counter = (gen[r], 0, 0, 0) -- the draw of mh_sample_rows for row 0 of a one-row call with that seed
   at t = gen[r], whatever slot the request sits in.  Row r bans eos_id iff gen[r] < min_length.  A row with live[r] == 0 (live
   may be null: every row is live) writes out = -1, margin = pmax = 0, kept = 0 and nothing else.  margin and pmax are required;
   the shape limits are mh_sample_rows'. */
int mh_sample_rows_slots(const float* logits, long ldl, long* out, float* margin, float* pmax, int* kept, float* u_out, int R, int V,
                         const float* params, const unsigned long long* seed, const int* gen, const int* live, mh_stream_t s);
/* the greedy pick with the same per-row ban: arg-max, margin and p_max (at params[0] = inv_temp) as mh_argmax_pmax_rows computes
   them on the wide path, row r banning eos_id iff gen[r] < min_length; idle rows as above.  Same shape limits. */
int mh_argmax_pmax_rows_slots(const float* logits, long ldl, long* out, float* margin, float* pmax, int R, int V, const float* params,
                              const int* gen, const int* live, mh_stream_t s);
/* mh_repetition_penalty_rows under the row mask: a row with live[r] == 0 changes neither its logits nor its bitmap (the caller
   zeroes a row's bitmap words when the row takes a new request) */
int mh_repetition_penalty_rows_slots(float* logits, long ldl, unsigned* seen, const long* prev_ids, int R, int V, const float* penalty,
                                     const int* live, mh_stream_t s);
/* mh_decode_advance_kept under the row mask, with the per-row token count: a live row records (id, margin, p_max, kept) in
   rec[4][R], feeds its id back and advances pos[r], kvlen[r] and gen[r]; an idle row records (-1, 0, 0, 0) and keeps all its
   state.  kept may be null (a greedy pick): the fourth record row is then 0.  *step += 1 once per launch. */
int mh_decode_advance_kept_rows(const long* nxt, const float* margin, const float* pmax, const int* kept, float* rec, long* next_ids,
                                int* step, int* pos, int* kvlen, int* gen, const int* live, int R, mh_stream_t s);
/* token log-probabilities of a decode step: the log-softmax at temperature 1 of the f32 logits [R, ldl] a pick was made from (after
   the in-place repetition penalty when it is on; temperature, top-k, top-p and the EOS ban do not enter).  ids[r] = the pick of row
   r; watch = 8 int32 ids on the device (-1 or any id outside [0, V): unused, its entries are 0.0), read by the kernel so one
   captured graph serves every watch set.  out = 10 rows of R floats, row stride ldo >= R (rows of a step's record, say):
   out[0][r] = lse = m + log(sum_j exp(x_j - m)) with m the row maximum, f32 in a fixed order; out[1][r] = x[ids[r]] - lse;
   out[2 + w][r] = x[watch[w]] - lse.  A row with live[r] == 0 (live may be null: every row is live) or ids[r] < 0 writes 0.0 to
   its ten entries and reads no logits.  One 1024-thread workgroup per row with the row in registers when V <= 32768, ldl % 4 == 0
   and the base is 16-byte aligned; one strided workgroup per row otherwise.  A null logits / ids / watch / out, V < 1 or ldo < R
   is MH_ERR_ARG before any launch. */
int mh_token_scores_rows(const float* logits, long ldl, const long* ids, const int* watch, float* out, long ldo, int R, int V,
                         const int* live, mh_stream_t s);

/* beam search step (HF GenerationMixin._beam_search), nb <= 8 beams, K = 2*nb, 2*nb <= V <= 32768 (else MH_ERR_UNSUPPORTED):
   rows b*rpi .. b*rpi+rpi-1 of fp32 logits [B*rpi, ldl] belong to item b (rpi = nb, or 1 for the step after a prefill at B rows);
   per row score = scores[row] + ((x - max) - log(sum exp(x - max))), -inf at ban_id (< 0: none); per item the top K over its
   rpi*V candidates, best first, ties to the lower flat index row_in_item * V + token: out_s / out_i [B, K] (the step's record).
   part_s / part_i = caller scratch of B*rpi*K entries each.  pos / kvlen (both given or both null): += 1 for rows [0, n_adv). */
int mh_beam_topk(const float* logits, long ldl, const float* scores, float* part_s, int* part_i, float* out_s, int* out_i, int B,
                 int rpi, int nb, int V, int ban_id, int* pos, int* kvlen, int n_adv, mh_stream_t s);
/* in-place KV-cache reorder of every layer in one launch: caches = device table of L pointers to [B*nb, T_cap, C] bf16 caches
   (16-byte aligned, C % 8 == 0); cache[r, p] = old cache[src[r], p] for p in [*lo, *hi), src / lo / hi read from device memory
   (capturable).  src[r] must name a row of r's own item (b*nb .. b*nb+nb-1; anything else is treated as src[r] == r); rows with
   src[r] == r are not written; duplicate parents are fine (every source is read before any store of the same cell). */
int mh_beam_reorder_kv(void* const* caches, int L, int B, int nb, long T_cap, int C, const int* src, const int* lo, const int* hi,
                       mh_stream_t s);
/* the decode slots' beam groups: mh_beam_topk at rpi = nb for G items, one request each, with per-item state in device memory.
   live[G], gen[G] (tokens the item's request has generated), prm[2] = (min_length, eos_id), all int32 and read by the kernels, so
   one captured graph serves every value.  A live item (live[g] != 0) bans eos_id iff gen[g] < min_length; its K = 2*nb entries of
   out_s / out_i [G, K] are what mh_beam_topk writes for that item alone (B = 1) with that ban; then pos[r] += 1 and kvlen[r] += 1
   for its nb rows g*nb .. g*nb+nb-1 and gen[g] += 1.  An idle item's row workgroups leave before they load a logit, its record
   entries are (0.0, -1) and its pos / kvlen / gen / scratch rows are not touched.  part_s / part_i = scratch of G*nb*K entries.
   Limits as mh_beam_topk; a null pointer (pos and kvlen included), V < 1 or ldl < V is MH_ERR_ARG; both before any launch. */
int mh_beam_topk_items(const float* logits, long ldl, const float* scores, float* part_s, int* part_i, float* out_s, int* out_i, int G,
                       int nb, int V, const int* live, int* gen, const int* prm, int* pos, int* kvlen, mh_stream_t s);
/* mh_beam_reorder_kv with a window and a live flag per item: item g copies positions [lo[g], hi[g]) clamped to [0, T_cap) among its
   rows g*nb .. g*nb+nb-1; an item with live[g] == 0 and every position outside an item's window are not touched; a parent outside
   the item is ignored.  lo / hi / live int32 [G] in device memory (capturable).  With src = each group's first row, the window
   [0, S0_g) and live = the groups just refilled it broadcasts a prefilled prompt to its sibling rows. */
int mh_beam_reorder_kv_items(void* const* caches, int L, int G, int nb, long T_cap, int C, const int* src, const int* lo,
                             const int* hi, const int* live, mh_stream_t s);
/* beam-search multinomial sampling / the repetition penalty under beams: mh_beam_topk's step with HF's processor chain on the
   log-probs and Gumbel noise on the candidates.  logits [B*nb, ldl] fp32 (nb rows per item, always), scores [B*nb].  Per row, in
   fp32: lp = (x - max) - log(sum exp(x - max)) (NaN -> -inf); for every id in the row's bitmap seen[row] (W = ceil(V/32) words a
   row; null: none) lp = lp < 0 ? lp*p : lp/p; lp[ban_id] = -inf (< 0: none); then with draw != 0: w = lp * inv_temp; the
   k = max(top_k, 2) largest w stay, ties at the k-th value included; of those, in (w desc, id asc) order, candidate i stays while
   its exclusive prefix mass of softmax(w) is < top_p * total (top_p >= 1: all), the best two always; acc = w + scores[row] for
   what stays, -inf otherwise; key = acc - log(-log(u)), u = ((x0 >> 9) + 0.5) * 2^-23, x0 = the first word of Philox4x32-10 with
   key = *seed and counter (t, row_in_item * V + id, item, 1), t = (step ? *step : 0) + t_add.  With draw == 0: key = acc =
   lp + scores[row] (no temperature, cuts or noise; params only read for the penalty).  params = f32 (inv_temp, top_p, top_k,
   penalty) in device memory, mh_sample_rows' layout.  Per item the top K = 2*nb by (key desc, flat asc), flat = row_in_item * V +
   id: out_s = acc, out_i = flat, out_k = key (null: not written), each [B, K]; out_f [B] = 1 when a row of the item had more than
   1024 candidates tied into its top-k set, whose top-p cut was then not applied (the indices written are valid; the host redoes
   the item), else 0.  part_k / part_a / part_i = scratch of B*nb*K entries each, part_f of B*nb.  pos / kvlen (both or neither):
   += 1 for rows [0, n_adv), and *step += 1 with them.  4 <= V <= 32768, V % 4 == 0, 2*nb <= V, nb <= 8, else MH_ERR_UNSUPPORTED;
   a null required pointer, V < 1 or ldl < V is MH_ERR_ARG; both before any launch. */
int mh_beam_sample_topk(const float* logits, long ldl, const float* scores, const unsigned* seen, float* part_k, float* part_a,
                        int* part_i, int* part_f, float* out_s, int* out_i, int* out_f, float* out_k, int B, int nb, int V,
                        int ban_id, int draw, const float* params, const unsigned long long* seed, int* step, int t_add, int* pos,
                        int* kvlen, int n_adv, mh_stream_t s);
/* the seen-id bitmaps follow their hypotheses: seen[r] = old seen[src[r]] | bit(ids[r]) over [B*nb, ceil(V/32)] words, in place
   (every source word of an item is read before any store); src as in mh_beam_reorder_kv, ids int64 (outside [0, V): no bit). */
int mh_beam_seen_update(unsigned* seen, const int* src, const long* ids, int B, int nb, int V, mh_stream_t s);
/* the decode slots' beam groups: mh_beam_sample_topk for G items of nb rows, one request each, with per-item state in device
   memory, so one captured graph serves every run.  live[G], gen[G] (tokens the item's request has generated) and bprm[2] =
   (min_length, eos_id) are int32, seed[G] is one 64-bit Philox key per item; params (inv_temp, top_p, top_k, penalty) stays one
   vector for the launch.  A live item (live[g] != 0) bans eos_id iff gen[g] < min_length and draws Philox step t = gen[g] + t_add
   with key seed[g] and counter (t, row_in_item * V + id, 0, 1): the item field is 0 wherever the item sits, so its K = 2*nb
   entries of out_s / out_i / out_k [G, K] and its out_f[g] are what mh_beam_sample_topk writes at B = 1 for its rows alone with
   *seed = seed[g], step = null, t_add = t and that ban.  Then, when pos / kvlen are given, pos[r] += 1 and kvlen[r] += 1 for its
   rows g*nb .. g*nb+nb-1 and gen[g] += 1; with pos and kvlen both null nothing advances, gen included (the first pick after a
   refill, whose rows have no position yet).  An idle item's row workgroups leave before they load a logit or a bitmap word; its
   record is (0.0, -1) K times with out_f[g] = 0, and its out_k entries, pos / kvlen / gen and scratch rows are not touched.
   Limits and the draw / seen / params rules as mh_beam_sample_topk; a null live / gen / bprm, or only one of pos / kvlen, is
   MH_ERR_ARG; all before any launch. */
int mh_beam_sample_topk_items(const float* logits, long ldl, const float* scores, const unsigned* seen, float* part_k, float* part_a,
                              int* part_i, int* part_f, float* out_s, int* out_i, int* out_f, float* out_k, int G, int nb, int V,
                              int draw, const float* params, const unsigned long long* seed, const int* live, int* gen,
                              const int* bprm, int t_add, int* pos, int* kvlen, mh_stream_t s);
/* mh_beam_seen_update with a live flag per item (int32 [G], read by the kernel): an item with live[g] == 0 has its bitmap rows
   neither read nor written; a live one is updated as mh_beam_seen_update updates it (a parent outside the item is ignored). */
int mh_beam_seen_update_items(unsigned* seen, const int* src, const long* ids, int G, int nb, int V, const int* live, mh_stream_t s);

/* K12 conv stacks of VEInstructorV2 / VETokenizer (networks.py:98-127,159-189) as im2col + mh_gemm_bf16_nt. */
int mh_im2col_nhwc(const void* x, void* col, int B, int H, int W, int C, int kh, int kw, int pad, int Kpad,
                   mh_stream_t s);
int mh_col2im_nhwc(const void* dcol, float* dx, int B, int H, int W, int C, int kh, int kw, int pad, int Kpad,
                   mh_stream_t s);
int mh_relu_maxpool2_fwd(const void* y, int y_is_f32, long ldy, void* p, int B, int H, int W, int C, mh_stream_t s);
int mh_relu_maxpool2_bwd(const float* dp, const void* y, int y_is_f32, long ldy, void* dy, long lddy, int B, int H,
                         int W, int C, mh_stream_t s);
int mh_conv_pack_weight(const float* W, const float* bias, void* Wp, int Cout, int K, int Kpad, mh_stream_t s);
int mh_conv_unpack_grad(const float* dWp, float* dW, float* db, int Cout, int K, int Kpad, mh_stream_t s);

/* K13 assembly of inputs_embeds (myriad.py:354-375,395-421) and generic data movement. */
int mh_embed_gather(const void* table_bf16, const long* ids, const int* dst_rows, float* out, long n, int D, long ldo,
                    mh_stream_t s);
int mh_copy2d_f32(const float* src, long lds, float* dst, long ldd, long rows, int cols, int accumulate,
                  mh_stream_t s);
int mh_copy3d_f32(const float* src, long src_bstride, long lds, float* dst, long dst_bstride, long ldd, int nb,
                  long rows, int cols, int accumulate, mh_stream_t s);
int mh_gather_rows_f32_to_bf16(const float* src, long lds, const int* rows, void* dst, long n, int D, mh_stream_t s);
int mh_gather_rows_f32(const float* src, long lds, const int* rows, float* dst, long n, int D, mh_stream_t s);
/* The same for rows of any 2- or 4-byte element type (16-byte units: D and lds multiples of 16 / elem_bytes), and its inverse with
 * zero fill: dst[m, :] = inv[m] >= 0 ? src[inv[m], :] : 0 for every row m < M of dst (one launch instead of a fill + a scatter).
 * llama.py runs the LAST decoder layer's o_proj / MLP (modeling_llama.py:281-293) on the label-bearing rows only and expands the
 * row gradients back with these. */
int mh_gather_rows(const void* src, long lds, const int* rows, void* dst, long n, int D, int elem_bytes, mh_stream_t s);
int mh_expand_rows(const void* src, const int* inv, void* dst, long ldd, long M, int D, int elem_bytes, mh_stream_t s);
int mh_copy3d_bf16(const void* src, long src_bstride, long lds, void* dst, long dst_bstride, long ldd, int nb,
                   long rows, int cols, mh_stream_t s);
/* KV-cache append at a device-resident position + device counter bump: lets one decode step be captured in a
 * hipGraph and replayed per token (modeling_llama.py:190-195 concatenates; the cache is written in place). */
int mh_kv_append_bf16(const void* src, long ld_src, void* cache, long cache_bstride, long ld_cache, const int* pos_dev,
                      int B, int cols, mh_stream_t s);
/* One decode token per batch row: rotary on q (in place) and on k, then k|v written into cache row pos_dev[0]
 * (modeling_llama.py:186-195: apply_rotary_pos_emb + cat with past_key_value) -- rope + append in one launch.
 * qkv [B, ld] bf16 = [q | k | v] with W = n_heads*head_dim columns each; cache row layout [k | v]. */
int mh_rope_kv_append(void* qkv, long ld, int n_heads, int head_dim, const int* pos, const float* cos_tab,
                      const float* sin_tab, void* cache, long cache_bstride, long ld_cache, const int* pos_dev, int B,
                      mh_stream_t s);
int mh_add_i32(int* x, int n, int delta, mh_stream_t s);
/* Decode weight layout (modeling_llama.py:184-231 with the KV cache: every token multiplies <= 16 rows by every frozen
 * Linear).  mh_gemv_pack writes a stream-ordered copy of W [N, K] bf16 (mh_gemv_pack_elems(N, K) elements, -1 on bad
 * dims): the 16 B lane (lr, lg) of wave w reads at step t sit at ((block*NW + w)*per + t)*2 KiB + h*1 KiB + lane*16, so
 * the skinny-M kernel reads each KiB contiguously.  mh_gemv_packed = mh_gemm_bf16_nt for M <= 16 on that copy, bit-identical. */
long mh_gemv_pack_elems(int N, int K);
int mh_gemv_pack(const void* W, int ldb, int N, int K, void* out, mh_stream_t s);
int mh_gemv_packed(const void* A, int lda, const void* P, void* C, int ldc, int M, int N, int K, const float* bias,
                   const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
/* The decode step's Linear with the producer of its operand fused in (bit-identical to the two-launch forms): the RMSNorm
 * in front of q/k/v, gate|up and lm_head (modeling_llama.py:66-74; H [M, K] f32) and the SiLU gate in front of the down
 * projection (:139-140; gu [M, 2K] bf16, gate / up interleaved in blocks of 128).  Every workgroup rebuilds the <= 16
 * operand rows in LDS; MH_ERR_UNSUPPORTED when M * K * 2 bytes exceed 64 KiB (use the two-launch form). */
int mh_gemv_packed_rmsnorm(const float* H, long ldh, const float* norm_w, float eps, const void* P, void* C, int ldc, int M,
                           int N, int K, const float* bias, const float* residual, int ldr, int out_f32, float alpha,
                           mh_stream_t s);
int mh_gemv_packed_silu(const void* gu, long ldgu, const void* P, void* C, int ldc, int M, int N, int K, const float* bias,
                        const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
/* FP8 weight-only copy for the decode step (opt-in): mh_gemv_pack_fp8 writes q = e4m3fn(W / s_n) (round to nearest even,
 * saturated to +-448) in the stream order above at one byte per weight (mh_gemv_pack_fp8_elems(N, K) bytes: each KiB holds
 * one 64-deep step of a wave) and the row scales s_n = amax_n / 448 (1 for an all-zero row) into scale_out[N].  The three
 * fp8 products take the same arguments and contract as their bf16 forms plus the scales, and compute
 * C = alpha * s_n * A . q^T (+bias) (+residual): each code widened exactly to bf16, the same MFMA, s_n then alpha in the epilogue. */
long mh_gemv_pack_fp8_elems(int N, int K);
int mh_gemv_pack_fp8(const void* W, int ldb, int N, int K, void* q_out, float* scale_out, mh_stream_t s);
int mh_gemv_packed_fp8(const void* A, int lda, const void* Q, const float* scale, void* C, int ldc, int M, int N, int K,
                       const float* bias, const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
int mh_gemv_packed_fp8_rmsnorm(const float* H, long ldh, const float* norm_w, float eps, const void* Q, const float* scale,
                               void* C, int ldc, int M, int N, int K, const float* bias, const float* residual, int ldr,
                               int out_f32, float alpha, mh_stream_t s);
int mh_gemv_packed_fp8_silu(const void* gu, long ldgu, const void* Q, const float* scale, void* C, int ldc, int M, int N, int K,
                            const float* bias, const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
/* MXFP4 weight-only copy for the decode step (opt-in; OCP microscaling, e2m1 codes).  The format, for W [N, K] bf16, finite,
 * K % 128 == 0 (non-finite weights are outside the contract: their codes and scales are unspecified):
 *   block  = 32 consecutive k within a row;
 *   E      = the biased bf16 exponent field of the block's largest |w| (0 for a zero or subnormal maximum);
 *   b      = max(2, E - 2), the scale byte, X = 2^(b-127): the OCP rule floor(log2 amax) - emax(e2m1), clamped below so that
 *            every dequantised value is zero or a normal bf16; b <= 252;
 *   code   = sign | index into {0, 0.5, 1, 1.5, 2, 3, 4, 6} of w / X rounded to nearest, ties to the even code, saturated at
 *            +-6; the sign bit is copied from w, zeros included;
 *   byte   = two codes, the lower k in the low nibble;   dq = code * X, exact in bf16.
 * mh_gemv_pack_fp4 writes the codes in the stream order above at 128-deep steps (mh_gemv_pack_fp4_elems(N, K) bytes: lane
 * (lr, lg) of wave w reads at step t the 32 codes k = 128 (w per + t) + 32 lg .. +31 of row 16 block + lr, 16 B at
 * ((block*NW + w)*per + t)*1 KiB + lane*16, per = ceil(K / 128 / NW)) and the scale bytes beside them
 * (mh_gemv_pack_fp4_scale_elems(N, K) bytes: that lane's byte at ((block*NW + w)*ceil(per / 4) + t / 4)*256 + lane*4 + t % 4).
 * Steps past K and the bytes that pad a scale dword are zero blocks (codes 0, b = 2); rows past N repeat row N - 1.  Both
 * _elems return -1 on N <= 0, K <= 0 or K % 128 != 0; the packer returns MH_ERR_ARG on those, on ldb < K or ldb % 8 != 0, a
 * null scale_out, W / q_out not 16-byte or scale_out not 4-byte aligned, and writes nothing then.  The three fp4 products take
 * the arguments and the contract of their fp8 forms (<= 16 rows, MH_ERR_UNSUPPORTED of the fused forms above the LDS budget)
 * with the scale bytes in place of the row scales and K % 128 == 0, and compute C = alpha * A . dq(W)^T (+bias) (+residual):
 * each pair of codes widened exactly to bf16 with its block scale, the same MFMA, no epilogue scale. */
long mh_gemv_pack_fp4_elems(int N, int K);
long mh_gemv_pack_fp4_scale_elems(int N, int K);
int mh_gemv_pack_fp4(const void* W, int ldb, int N, int K, void* q_out, void* scale_out, mh_stream_t s);
int mh_gemv_packed_fp4(const void* A, int lda, const void* Q, const void* scale, void* C, int ldc, int M, int N, int K,
                       const float* bias, const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
int mh_gemv_packed_fp4_rmsnorm(const float* H, long ldh, const float* norm_w, float eps, const void* Q, const void* scale,
                               void* C, int ldc, int M, int N, int K, const float* bias, const float* residual, int ldr,
                               int out_f32, float alpha, mh_stream_t s);
int mh_gemv_packed_fp4_silu(const void* gu, long ldgu, const void* Q, const void* scale, void* C, int ldc, int M, int N, int K,
                            const float* bias, const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
/* The packed products at up to 64 rows (the decode slots above 16 rows): C[M <= 64, N] = alpha * A . W^T (+bias) (+residual)
 * on the copy mh_gemv_pack / mh_gemv_pack_fp8 / mh_gemv_pack_fp4 wrote -- no other layout.  Each takes the arguments of its
 * 16-row counterpart.  M > 64 is MH_ERR_ARG; M <= 0 or N <= 0 is MH_OK with nothing written; the alignment and K-step refusals
 * are the 16-row entries' (K % 64, K % 128 for fp4; lda % 8; A, the copy 16-byte and the scales 4-byte aligned).  M <= 16 runs
 * the 16-row kernel.  Bit contract: row m of a wide product carries the bits the 16-row entry gives that row on the same copy,
 * for every M, output type, bias, residual and alpha: per output element the K split over the waves, the step and MFMA order,
 * the cross-wave sum order and the epilogue order (fp8 row scale, alpha, bias, residual) are the 16-row kernel's; a workgroup
 * owns several adjacent column blocks so that one activation fragment feeds them all (csrc/gemv.hip). */
int mh_gemv_packed_wide(const void* A, int lda, const void* P, void* C, int ldc, int M, int N, int K, const float* bias,
                        const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
int mh_gemv_packed_fp8_wide(const void* A, int lda, const void* Q, const float* scale, void* C, int ldc, int M, int N, int K,
                            const float* bias, const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
int mh_gemv_packed_fp4_wide(const void* A, int lda, const void* Q, const void* scale, void* C, int ldc, int M, int N, int K,
                            const float* bias, const float* residual, int ldr, int out_f32, float alpha, mh_stream_t s);
/* q / v LoRA merged into the decode step's copy of the frozen qkv weight (opt-in, llama.py decode_merge_lora; PEFT merge_adapter).
 * W [3D, D] bf16 rows [q | k | v] with leading dimension ldw (the frozen columns of the bordered wqkv_ext), Aqv [2r, D] fp32 = the
 * masters A_q | A_v, Bq / Bv [D, r] fp32, s = alpha / r, r = 8 or 16.  Merged rule, per element:
 *   q rows n < D:        bf16(W[n,k] + s * acc), acc = sum over j = 0 .. r-1 in order of Bq[n,j] * A_q[j,k], starting from 0
 *   k rows D <= n < 2D:  W[n,k]
 *   v rows n >= 2D:      the q rule with Bv[n - 2D] and A_v
 * each product and sum a separate fp32 operation rounded to nearest even (no FMA contraction), then one round-to-nearest-even to
 * bf16.  mh_lora_merge writes the merged matrix row-major (out [3D, ldo]); mh_lora_merge_pack writes the mh_gemv_pack copy of it
 * (mh_gemv_pack_elems(3D, D) elements) and mh_lora_merge_pack_fp8 the mh_gemv_pack_fp8 codes and row scales of it
 * (mh_gemv_pack_fp8_elems(3D, D) bytes, 3D scales), bit for bit, each in one pass from W.  MH_ERR_ARG on D <= 0 or D % 64 != 0,
 * r not 8 / 16, ldw (ldo) < D or not a multiple of 8, a null pointer, W / Aqv / out / q_out not 16-byte aligned, or Bq / Bv /
 * scale_out not 4-byte aligned. */
int mh_lora_merge(const void* W, int ldw, const float* Aqv, const float* Bq, const float* Bv, int D, int r, float s, void* out,
                  int ldo, mh_stream_t stream);
int mh_lora_merge_pack(const void* W, int ldw, const float* Aqv, const float* Bq, const float* Bv, int D, int r, float s, void* out,
                       mh_stream_t stream);
int mh_lora_merge_pack_fp8(const void* W, int ldw, const float* Aqv, const float* Bq, const float* Bv, int D, int r, float s,
                           void* q_out, float* scale_out, mh_stream_t stream);
/* One decode token of attention (modeling_llama.py:186-222 with the KV cache): rotary on q / k, k | v appended at cache row
 * pos_dev[0], the one query against kv_len[b] keys -- mh_rope_kv_append + mh_attn_fwd(Sq = 1) in one launch, same bits.
 * qkv [B, ld_qkv] bf16 = [q | k | v] (q rotated in place), cache [B][T_cap][2 H D] rows [k | v], out [B, H D] bf16.
 * kv_len[b] > T_cap counts as T_cap; a row with kv_len[b] <= 0 still rotates and appends and gets a zero out row.  MH_ERR_ARG,
 * nothing launched, unless D % 8 == 0, 0 < D <= 128, H > 0, 0 < T_cap <= 8192, ld_qkv / ld_cache / cache_bstride % 8 == 0,
 * ldo % 4 == 0, ld_qkv >= 3 H D, ld_cache >= 2 H D and ldo >= H D (mh_attn_decode_rope_rows likewise). */
int mh_attn_decode_rope(void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                        const int* pos_dev, const int* kv_len, const float* cos_tab, const float* sin_tab, void* out, long ldo,
                        int B, int H, int D, int T_cap, float scale, mh_stream_t s);
/* The same token step with per-row state (decode slots): row b rotates q / k at pos[b] and appends k | v at cache row pos[b]
 * (the host keeps pos[b] < T_cap), the query sees kv_len[b] keys; a live row's out, rotated q and cache row have the bits of
 * mh_attn_decode_rope on that row alone with pos_dev[0] = pos[b].  live int[B] on the device: a row with live[b] == 0 reads no
 * cache row, writes neither qkv nor the cache, and gets a zero out row. */
int mh_attn_decode_rope_rows(void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                             const int* kv_len, const int* live, const float* cos_tab, const float* sin_tab, void* out, long ldo,
                             int B, int H, int D, int T_cap, float scale, mh_stream_t s);
/* K consecutive token steps of each of G sequences in one launch (attn_decode_draft.hip; the verify step of draft-and-verify
 * greedy decoding).  Row g*K + j of qkv [G*K, ld_qkv] is the token at position pos[g] + j of sequence g, 1 <= K <= 8; cache
 * [G][T_cap][2 H D]; pos and live int[G] on the device, so a captured launch replays while the position moves.  There is no kv_len:
 * the query of row j sees keys 0 .. pos[g] + j.  For a live sequence and every j < K, q (in place) and k are rotated at pos[g] + j,
 * k | v are appended at cache row pos[g] + j, and the out row ([G*K, ldo] bf16), the rotated q and the cache row have the bits of
 * mh_attn_decode_rope on that row alone at that position, run after rows 0 .. j-1 were appended: K sequential one-row steps.  Cache
 * rows < pos[g] are only read, cache rows >= pos[g] + K are not touched.  A sequence with live[g] == 0 touches nothing and gets
 * zero out rows; a row whose position would reach T_cap (the host keeps that from happening) writes no cache row, leaves its q
 * alone and gets a zero out row.  MH_ERR_UNSUPPORTED, nothing launched, unless D % 16 == 0, D <= 128, K <= 8 and the LDS of a
 * workgroup -- 4 * round_up(T_cap, 64) + 8192 + 2 K D bytes -- fits gfx950's 160 KiB; a call with G = 0 answers that question and
 * reads no pointer.  MH_ERR_ARG for misaligned strides (ld_qkv, ld_cache, cache_bstride % 8, ldo % 4) or pointers, and for
 * strides shorter than the rows (ld_qkv < 3 H D, ld_cache < 2 H D, ldo < H D). */
int mh_attn_decode_rope_draft(void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                              const int* live, const float* cos_tab, const float* sin_tab, void* out, long ldo, int G, int K,
                              int H, int D, int T_cap, float scale, mh_stream_t s);
/* The end of that verify step (draft.hip), after mh_argmax_pmax_rows over the G*K logit rows: nxt / margin / pmax [G*K] are the
 * rows' picks and ids [G*K] the tokens that were fed, ids[g*K] real and the rest guesses.  n_out = 1 + the number of leading
 * j < K - 1 with nxt[j] == ids[j + 1] and pmax[j] >= *top_p (a device float; <= 0: no row needs a draw, p_max is not looked at).
 * Writes rec[g] = 3K + 1 floats (the K ids, margins and p_max, then n_out), ids[g*K] = nxt[n_out - 1], pos[g] += n_out,
 * kvlen[g] = pos[g] + 1 and *step += 1 once per launch.  1 <= K <= 8 (else MH_ERR_ARG).  The cache rows of rejected guesses stay
 * behind, stale, at pos[g] .. (old pos[g]) + K - 1: the next verify step overwrites them and a plain step's kvlen stops short. */
int mh_draft_accept(const long* nxt, const float* margin, const float* pmax, long* ids, const float* top_p, float* rec, int* pos,
                    int* kvlen, int* step, int G, int K, mh_stream_t s);
/* mh_attn_decode_rope_draft for the decode slots: the same kernel with nrow int[G] on the device beside pos and live, 1 <=
 * nrow[g] <= K, the rows of group g that hold a token (the fed one and its real guesses).  Rows j < nrow[g] of a live group behave
 * exactly as in mh_attn_decode_rope_draft: the out row, the rotated q and the cache row have its bits.  Rows j >= nrow[g], like
 * every row of an idle group, read no cache row, leave q and the cache alone and get a zero out row.  The T_cap guard, the LDS rule
 * and the refusals are mh_attn_decode_rope_draft's; nrow must be non-null and 4-byte aligned (MH_ERR_ARG). */
int mh_attn_decode_rope_draft_rows(void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                                   const int* live, const int* nrow, const float* cos_tab, const float* sin_tab, void* out, long ldo,
                                   int G, int K, int H, int D, int T_cap, float scale, mh_stream_t s);
/* mh_draft_accept with per-group state (the decode slots' verify step): group g of K rows has nguess[g] real guesses behind its
 * fed token ids_k[g*K] (int[G] on the device, 0 .. K - 1; the ids past them are fillers) and a flag live[g].  A live group keeps
 * n_out = 1 + the number of leading j < nguess[g] with nxt[j] == ids_k[j + 1] and pmax[j] >= *top_p (<= 0: p_max is not looked
 * at); a filler is never confirmed, even where it equals the pick.  It writes rec[g] = 3K + 1 floats (the K ids, margins and
 * p_max, then n_out), ids_k[g*K] = next_ids[g] = nxt[n_out - 1] -- next_ids long[G] is the fed-id buffer of the plain one-row-per-
 * slot step, which can follow with no host copy --, pos[g] += n_out and kvlen[g] = pos[g] + 1.  An idle group records id -1 in
 * its K id entries, zeros elsewhere and n_out = 0, and changes none of ids_k, next_ids, pos, kvlen.  *step += 1 once per launch.
 * 1 <= K <= 8, else MH_ERR_ARG with nothing launched. */
int mh_draft_accept_rows(const long* nxt, const float* margin, const float* pmax, long* ids_k, long* next_ids, const int* nguess,
                         const int* live, const float* top_p, float* rec, int* pos, int* kvlen, int* step, int G, int K,
                         mh_stream_t s);
/* The verify step under the slot engine's per-row tail (draft_sample.hip): the launches that follow the logits [G*K, ldl] f32 of
 * a verify step when the repetition penalty, the per-request EOS ban or the device sampler is on.  Group g < G has K rows, 1 <= K
 * <= 8 (else MH_ERR_ARG, nothing launched), nrow[g] = 1 + its real guesses of them; live[g], gen[g], seed[g] and seen[g] (ceil(V /
 * 32) u32 words) are the slot's state as mh_sample_rows_slots / mh_repetition_penalty_rows_slots read it.  Row (g, j) is idle when
 * live[g] == 0 or j >= nrow[g].
 *
 * mh_repetition_penalty_draft_rows: row (g, j), not idle, gets HF's rule (x < 0 ? x * p : x / p, p = *penalty) on every id of the
 * bitmap seen[g] and on ids_k[g*K .. g*K + j], the tokens fed in rows 0 .. j -- each id once, also where an extra id is in the
 * bitmap already or repeats an earlier extra; extras outside [0, V) are skipped.  The row then holds the bits
 * mh_repetition_penalty_rows_slots leaves on it when its bitmap is seen[g] plus ids_k[g*K .. g*K + j - 1] and prev_ids is
 * ids_k[g*K + j].  The bitmap is only read (the K workgroups of a group share it); idle rows are left alone.  MH_ERR_ARG for a
 * null pointer, V < 1 or ldl < V. */
int mh_repetition_penalty_draft_rows(float* logits, long ldl, const unsigned* seen, const long* ids_k, const int* nrow,
                                     const int* live, int G, int K, int V, const float* penalty, mh_stream_t s);
/* mh_sample_rows_slots (draw != 0) / mh_argmax_pmax_rows_slots (draw == 0) for those rows: row (g, j) reads seed[g] and t = gen[g]
 * + j -- Philox counter (t, 0, 0, 0) -- and bans eos_id iff t < min_length (params[6] as in mh_sample_rows_slots).  Every output
 * of a row that is not idle (out, margin, pmax, and with the draw kept and u_out) has the bits of the slot entry on that row alone
 * with gen = gen[g] + j; an idle row writes out = -1, margin = pmax = 0 and (draw) kept = 0.  out / margin / pmax / kept / u_out
 * hold G*K entries; kept, u_out and seed are not touched without the draw.  nrow and live are required.  The shape limits and the
 * MH_ERR_UNSUPPORTED rules are mh_sample_rows_slots'. */
int mh_sample_rows_draft(const float* logits, long ldl, long* out, float* margin, float* pmax, int* kept, float* u_out, int G, int K,
                         int V, const float* params, const unsigned long long* seed, const int* gen, const int* nrow, const int* live,
                         int draw, mh_stream_t s);
/* mh_draft_accept_rows for those picks, with three additions.  (a) kept int[G*K] (may be null: the p_max rule of
 * mh_draft_accept_rows): a row with kept[j] < 0 -- the host must draw it -- ends the chain, so it can be the last kept row but no
 * guess behind it is confirmed; *top_p is not looked at then.  (b) seen (may be null): the bits of ids_k[g*K .. g*K + n_out - 1],
 * the fed token and the confirmed guesses, are set in seen[g] (ids outside [0, V) skipped; V is unused without seen); the kept
 * pick nxt[n_out - 1] joins when the next step feeds it, as in the plain step.  (c) gen[g] += n_out.  rec[g] = 4K + 1 floats: the
 * K ids, the K margins, the K p_max, the K kept counts (0.0 without kept), then n_out.  An idle group (live[g] == 0) records id
 * -1 in its K id entries, zeros elsewhere and n_out = 0, and changes none of ids_k, next_ids, pos, kvlen, gen, seen.  *step += 1
 * once per launch. */
int mh_draft_accept_sampled_rows(const long* nxt, const float* margin, const float* pmax, const int* kept, long* ids_k,
                                 long* next_ids, const int* nguess, const int* live, const float* top_p, unsigned* seen, float* rec,
                                 int* pos, int* kvlen, int* gen, int* step, int G, int K, int V, mh_stream_t s);
/* Packed prefill of several decode slots (attn_ragged.hip): causal self-attention over R sequences packed row-wise into qkv
 * [M, ld_qkv] bf16 = [q | k | v] (pre-rotary, only read), with the rotary at pos[row] and the KV-cache write fused in.  seg is the
 * device table int[R][3] of (row0, len, slot) and seg_host the host's copy of it: segment i is rows row0 .. row0 + len - 1, its
 * rotated k | v go to cache[slot] rows 0 .. len - 1 (cache [n_slots][T_cap][2 H D], addressed as in mh_attn_decode_rope_rows), its
 * queries see its own keys only, and its out rows ([M, ldo] bf16) and cache rows have the bits of mh_rope_inplace +
 * mh_copy3d_bf16 + mh_attn_fwd(causal) on that segment as a B = 1 batch.  Rows of qkv / out outside every segment, cache rows
 * >= len and unnamed slots are not touched.  cos / sin tables [max_pos, D / 2]; a position outside them is clamped.
 * MH_ERR_ARG, nothing launched, unless 0 < len <= T_cap, 0 <= slot < n_slots, the slots are distinct and the segments disjoint
 * and inside [0, M) (the kernel repeats the per-segment bounds on the device table); MH_ERR_UNSUPPORTED unless D % 16 == 0 and
 * D <= 128. */
int mh_attn_prefill_ragged(const void* qkv, long ld_qkv, const int* pos, const int* seg, const int* seg_host, int R, void* cache,
                           long cache_bstride, long ld_cache, int n_slots, int T_cap, const float* cos_tab, const float* sin_tab,
                           int max_pos, void* out, long ldo, int M, int H, int D, float scale, mh_stream_t s);
/* The same pass on top of a cached prefix (a chat turn's new rows after the reused part of its context): seg / seg_host are
 * int[R][4] of (row0, len, slot, past).  Segment i holds the len NEW rows of a request whose keys 0 .. past - 1 are rows of
 * cache[slot] already (rotated k | v, as every writer of these caches leaves them); its rotated k | v go to cache rows past ..
 * past + len - 1 and its out rows and those cache rows have the bits of mh_rope_inplace + mh_copy3d_bf16 into
 * cache[slot][past ..] + mh_attn_fwd(causal, Sq = len, Sk = past + len, q_off = past) on that segment at B = 1 (for len = 1 and
 * past < 8192 that is mh_attn_fwd's decode kernel, whose arithmetic the launch repeats for such a segment).  pos[] stays the
 * caller's.  No cache row >= past is read, rows < past and >= past + len are not written.  With past = 0 everywhere the results
 * are mh_attn_prefill_ragged's bits.  MH_ERR_ARG as there, and unless 0 <= past and past + len <= T_cap. */
int mh_attn_prefill_ragged_past(const void* qkv, long ld_qkv, const int* pos, const int* seg, const int* seg_host, int R,
                                void* cache, long cache_bstride, long ld_cache, int n_slots, int T_cap, const float* cos_tab,
                                const float* sin_tab, int max_pos, void* out, long ldo, int M, int H, int D, float scale,
                                mh_stream_t s);
/* The _past pass for segments that continue the SAME cached prefix (the candidate answers of one prompt): the same tables
 * int[R][4] of (row0, len, slot, past), but several segments may name one slot, with equal or different past (0 included), and
 * the cache is only read: rows < past of a named slot, and no byte of it is written.  Segment i's out rows have the bits of
 * mh_attn_prefill_ragged_past on that segment alone with a private copy of its slot (for len = 1 and past < 8192 the decode
 * kernel's arithmetic, as there); qkv is only read, rows of out outside every segment are not touched.  MH_ERR_ARG /
 * MH_ERR_UNSUPPORTED, nothing launched, as mh_attn_prefill_ragged_past, except that slots need not be distinct; the kernel
 * repeats the per-segment bounds on the device table. */
int mh_attn_prefill_ragged_shared(const void* qkv, long ld_qkv, const int* pos, const int* seg, const int* seg_host, int R,
                                  const void* cache, long cache_bstride, long ld_cache, int n_slots, int T_cap,
                                  const float* cos_tab, const float* sin_tab, int max_pos, void* out, long ldo, int M, int H, int D,
                                  float scale, mh_stream_t s);
/* The same token step with the keys split into chunks (attn_decode_split.hip): grid (ceil(T_cap / chunk), B*H), each workgroup
 * scores one chunk and writes fp32 (m, l, o[D]) into `partials`, a second launch merges the chunks in order and writes bf16 out
 * (bits fixed from run to run).  q is rotated in registers (qkv is not written); the cache row at pos_dev[0] gets the bits
 * mh_attn_decode_rope writes.  chunk = 128, 256 or 512 keys (0 = 128); partials_floats >= mh_attn_decode_split_ws_floats(). */
long mh_attn_decode_split_ws_floats(int B, int H, int T_cap, int chunk);
int mh_attn_decode_rope_split(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                              const int* pos_dev, const int* kv_len, const float* cos_tab, const float* sin_tab, void* out, long ldo,
                              float* partials, long partials_floats, int B, int H, int D, int T_cap, int chunk, float scale,
                              mh_stream_t s);
/* The split token step with per-row state (decode slots), the same kernels with their ROWS flag on: row b rotates at pos[b] and
 * appends k | v at cache row pos[b] (the host keeps pos[b] < T_cap), the query sees kv_len[b] keys; a live row's out and cache
 * row have the bits of mh_attn_decode_rope_split at B = 1 on that row with pos_dev[0] = pos[b] and the same chunk.  qkv is read
 * only (mh_attn_decode_rope_rows rotates q in place; this entry does not).  live int[B] on the device: a row with live[b] == 0
 * reads neither qkv nor the cache, writes neither the cache nor a partial record, and gets a zero out row.  kv_len, pos and live
 * are read on the device, so one captured launch pair replays while contexts grow and rows go idle and live again. */
int mh_attn_decode_rope_split_rows(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                                   const int* kv_len, const int* live, const float* cos_tab, const float* sin_tab, void* out,
                                   long ldo, float* partials, long partials_floats, int B, int H, int D, int T_cap, int chunk,
                                   float scale, mh_stream_t s);
/* K consecutive split token steps of each of G sequences in one launch pair (attn_decode_split_draft.hip; the verify step of
 * draft-and-verify decoding on the split-KV view).  The arguments are mh_attn_decode_rope_draft's -- row g*K + j of qkv is the
 * token at position pos[g] + j of sequence g, 1 <= K <= 8, pos and live int[G] on the device -- plus partials, partials_floats and
 * chunk as in mh_attn_decode_rope_split_rows; partials_floats >= mh_attn_decode_split_draft_ws_floats(G, K, H, T_cap, chunk) =
 * G K H ceil(T_cap / chunk) 132.  For a live sequence and every j < K the out row and cache row pos[g] + j have the bits of the
 * j-th of K sequential mh_attn_decode_rope_split_rows launches at B = 1 with the same chunk, pos = pos[g] + j and kv_len =
 * pos[g] + j + 1.  Grid (ceil(T_cap / chunk), G*H): one workgroup per (chunk, sequence, head) loads every cached key and value
 * once for all K queries; a second launch merges each row's chunks in order.  qkv is only read.  No cache row >= pos[g] is read
 * (rows a rejected guess left there may hold anything), rows < pos[g] are only read and rows >= pos[g] + K are not touched.  A
 * sequence with live[g] == 0 or pos[g] < 0 touches nothing and gets zero out rows; a row whose position would reach T_cap writes
 * no cache row and no record and gets a zero out row.  MH_ERR_UNSUPPORTED, nothing launched, unless D % 16 == 0, D <= 128 and K
 * <= 8; MH_ERR_ARG for a chunk other than 0 (= 128), 128, 256, 512, T_cap > 8192, a short partials buffer, null or misaligned
 * pointers, misaligned strides (ld_qkv, ld_cache, cache_bstride % 8, ldo % 4) and strides shorter than the rows.  A call with G = 0
 * answers whether the shape is supported and reads no pointer. */
long mh_attn_decode_split_draft_ws_floats(int G, int K, int H, int T_cap, int chunk);
int mh_attn_decode_rope_split_draft(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                                    const int* live, const float* cos_tab, const float* sin_tab, void* out, long ldo,
                                    float* partials, long partials_floats, int G, int K, int H, int D, int T_cap, int chunk,
                                    float scale, mh_stream_t s);
/* The same for the decode slots: nrow int[G] on the device, 1 <= nrow[g] <= K, the rows of group g that hold a token.  Rows j <
 * nrow[g] of a live group behave as in mh_attn_decode_rope_split_draft; rows j >= nrow[g] write no cache row and no record and get
 * a zero out row.  nrow must be non-null and 4-byte aligned (MH_ERR_ARG). */
int mh_attn_decode_rope_split_draft_rows(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache,
                                         const int* pos, const int* live, const int* nrow, const float* cos_tab,
                                         const float* sin_tab, void* out, long ldo, float* partials, long partials_floats, int G,
                                         int K, int H, int D, int T_cap, int chunk, float scale, mh_stream_t s);
/* K14 patch embedding operand (eva_vit.py:196-204): NCHW f32 image -> [B*np, Kpad] bf16 in (c,iy,ix) order */
int mh_patchify_nchw(const float* img, void* out, int B, int C, int H, int W, int P, int Kpad, mh_stream_t s);
int mh_scatter_rows_f32(const float* src, const int* rows, float* dst, long ldd, long n, int D, int accumulate,
                        mh_stream_t s);
int mh_cast_f32_to_bf16(const float* x, void* y, long n, mh_stream_t s);
int mh_cast_bf16_to_f32(const void* x, float* y, long n, mh_stream_t s);
int mh_transpose_to_bf16(const void* in, int in_is_f32, long ldi, void* out, long ldo, int R, int C, mh_stream_t s);
/* Master -> working-copy refresh of trainable weight matrices (freeze_vit: False), batched.  From a row-major contiguous f32
 * [R, C] source one pass writes the bf16 row-major copy dst (row stride ld_dst >= C elements) and the bf16 transposed copy
 * dst_t [C, R] (row stride ld_t >= R); either destination may be NULL, not both.  Only elements inside [R, C] are written (the
 * padding of a wider destination keeps its contents); the bits are those of mh_cast_f32_to_bf16 / mh_transpose_to_bf16.
 * One launch walks a DEVICE-resident table of n_desc descriptors (mh_refresh_bf16_pair_desc_bytes() bytes each, 16-byte
 * aligned), built on the host: mh_refresh_bf16_pair_pack writes entry `index` of a host table for a matrix whose first tile is
 * `first_tile` (0 for the first matrix) and returns the next matrix's first tile -- after the last matrix the launch's
 * total_tiles -- or MH_ERR_ARG (< 0) for a NULL / misaligned pointer, R or C <= 0, or a destination row shorter than the
 * source's.  Entries must be packed in index order.  mh_refresh_bf16_pair returns MH_ERR_ARG before any launch for a NULL or
 * misaligned table or counts that cannot belong to one. */
long mh_refresh_bf16_pair_desc_bytes(void);
long mh_refresh_bf16_pair_pack(void* host_table, int index, long first_tile, const float* src, void* dst, long ld_dst,
                               void* dst_t, long ld_t, int R, int C);
int mh_refresh_bf16_pair(const void* dev_table, int n_desc, long total_tiles, mh_stream_t s);
int mh_colsum_f32(const float* in, long ld, float* out, long R, int C, mh_stream_t s);
int mh_scale_f32(float* x, float a, long n, mh_stream_t s);

/* K15 AdamW (runner_base.py:104-139) on a flat f32 buffer with optional bf16 shadow; step is 1-based. */
int mh_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, long n, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step, double grad_scale, mh_stream_t s);

/* K18 data path: NSA / CutPaste self-supervised anomaly augmentation on uint8 crops resident in HBM --
   minigpt4/datasets/self_sup_tasks.py:254-268 (the 'swap' and 'uniform' blends) and :97-113 (the label).  The random patch
   geometry is sampled on the host exactly as the reference samples it (myriad_amd/self_sup.py); ops is a device array of
   56-byte records {int image, y0, x0, h, w, sy, sx, mode; long mask_off; double factor; long patch_off} -- mode & 3: 0 swap,
   1 uniform, 2 union mask only (a Poisson patch); mode & 4: the source pixels are the resampled patch [h][w][3] at patch_off
   of `patches` (may be NULL when no record sets the bit) -- masks the byte pool the records index, hs / ws HOST copies of
   h, w.  out starts as a copy of dest; union_mask [B,H,W] u8 zeroed.
   mh_patch_label: mode 0 binary, 1 continuous (factor [B] f64), 2 intensity, 3 logistic-intensity (k, x0). */
int mh_patch_blend_u8(void* out, const void* src, const void* masks, const void* ops, const int* hs, const int* ws,
                      int n_ops, int B, int H, int W, void* union_mask, const void* patches, mh_stream_t s);
int mh_patch_label(const void* dest, const void* out, const void* union_mask, void* sums_ws, void* lm_ws, float* label,
                   const double* factor, int B, int H, int W, int mode, int tol, double k, double x0, mh_stream_t s);
/* The two OpenCV steps of the shipped augmentation recipe (self_sup_tasks.py:213-227 cv2.resize, :269-288 cv2.seamlessClone
   with NORMAL_CLONE; anomaly_detection.py:118-141), from their published algorithms -- PARITY UNPINNED, OpenCV is absent.
   mh_patch_resize_u8: 8-bit INTER_LINEAR of the box (sy, sx, sh, sw) of src[image] to out [h][w][3]; xi / yi [w] / [h] left
   source indices, xw / yw [w][2] / [h][2] 11-bit weights (device ints; myriad_amd/self_sup.linear_resize_tables); an exact
   2 x 2 decimation is the rounded mean of 4 (tables may be NULL).
   mh_patch_poisson_u8: gradient-domain cloning of patch [hp][wp][3] into out[image] in place.  pms [hp][wp] the clone mask
   (border cleared), eroded [h][w] its ROI after erode(3x3) x 3, ROI h x w at (y0s, x0s) of the patch and (dy0, dx0) of the
   image; Sh [h-2][h-2], Sw [w-2][w-2] sine matrices, cy / cx their 2 cos terms (f64); ws mh_patch_poisson_ws_doubles(h, w)
   doubles.  float64 throughout, interior = floor(clamp(u, 0, 255) + 1e-6).  mixed = 0: cv2.NORMAL_CLONE; 1: cv2.MIXED_CLONE
   (self_sup_tasks.py:22,47,267: the patch's gradient pair is kept where |Px - Py| > |Dx - Dy|, else the destination's). */
int mh_patch_resize_u8(const void* src, int image, int H, int W, int sy, int sx, int sh, int sw, const int* xi, const int* xw,
                       const int* yi, const int* yw, void* out, int h, int w, mh_stream_t s);
long mh_patch_poisson_ws_doubles(int h, int w);
int mh_patch_poisson_u8(void* out, int image, int H, int W, const void* patch, int hp, int wp, const void* pms,
                        const void* eroded, int y0s, int x0s, int dy0, int dx0, int h, int w, const double* Sh, const double* cy,
                        const double* Sw, const double* cx, double* ws, int mixed, mh_stream_t s);

/* Gated AdamW: torch.optim.AdamW skips parameters whose .grad is None -- a module no rank used this step (random prompt
   stage, myriad.py:378; DDP find_unused_parameters, runner_base.py:96-98) keeps its parameters, moments and step count.
   used/steps are DEVICE scalars (use count summed over ranks by the gradient all-reduce; updates applied so far):
   mh_adamw_gated updates one contiguous range iff *used > 0 with step = *steps + 1 (bias corrections in double);
   mh_adamw_bump(used[n], steps[n]) then advances the counters of the used modules. */
int mh_adamw_gated(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, double grad_scale, const float* used, const int* steps, mh_stream_t s);
int mh_adamw_bump(const float* used, int* steps, int n, mh_stream_t s);

/* Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) and the non-finite step guard (the step
   torch.cuda.amp.GradScaler skips), decided on the device through a control block `double ctl[4]`:
     ctl[0] = s      the ONE multiplier the AdamW applies to the raw gradient, fp32-representable:
                     (float)(grad_scale * min(1, max_norm / (grad_scale * sqrt(sumsq) + 1e-6))), computed in double, rounded once;
                     (float)grad_scale with max_norm = +inf (no clipping)
     ctl[1] = norm   grad_scale * sqrt(sumsq): the total norm of the scaled gradient, in double (it cannot overflow)
     ctl[2] = apply  0 when `guard` is set and sumsq is not finite, else 1
     ctl[3] = skipped  running count of updates not applied (the caller zeroes it once)
   mh_grad_sumsq: sum of squares of g[0..n) in fp64 (products exact, no overflow: the sum is finite iff every element is),
   one partial per workgroup into partials[0 .. mh_grad_sumsq_slots(n)), `slots` = the room there; nothing is read and zeros
   are written when *used <= 0 (the module had no gradient).  Deterministic: same input, same bits.
   mh_clip_finalize: sumsq = the partials added in index order (thread t its contiguous chunk, then the chunks in order) plus
   rank_sums[0..world) in rank order (NULL, 0: none), then writes ctl.  mh_clip_rank_sum: the sharded data-parallel half step --
   rank_sums[rank] = the partials' sum, the other slots 0, for a sum all-reduce that is exact.
   mh_adamw_gated_ctl / mh_adamw_bump_ctl: mh_adamw_gated / mh_adamw_bump that return at once when ctl[2] == 0 and multiply
   the gradient by (float)ctl[0] (in place of grad_scale).  All refuse n % 4, null pointers, max_norm <= 0 and slots too small
   with MH_ERR_ARG before any launch. */
long mh_grad_sumsq_slots(long n);
int mh_grad_sumsq(const float* g, long n, const float* used, double* partials, long slots, mh_stream_t s);
int mh_clip_rank_sum(const double* partials, long n_partials, double* rank_sums, int world, int rank, mh_stream_t s);
int mh_clip_finalize(const double* partials, long n_partials, const double* rank_sums, int world, double max_norm,
                     double grad_scale, int guard, double* ctl, mh_stream_t s);
int mh_adamw_gated_ctl(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, const float* used, const int* steps, const double* ctl, mh_stream_t s);
int mh_adamw_bump_ctl(const float* used, int* steps, int n, const double* ctl, mh_stream_t s);

/* K16 anomaly-map heads of the vision expert (adrefexpert_v2.py:243-301).  All f32.
 * l2norm_rows: y = x / max(||x||, eps) (bf16 and/or f32 out) -- operands of the cosine similarities (:259, :283);
 * pair_logits: out[row] = scale * [<p,t0>, <p,t1>] / ||p|| against the per-sample [normal, abnormal] text pair (:283-284);
 * zs_accumulate: one tap of the zero-shot branch: mask_acc[B,h,h] += w*softmax(pair)[1], map_acc[B,S,S] += w*softmax(
 *   bilinear(align_corners=True) upsampled pair)[1] (:285-296);
 * rowmax_skip: acc[row] += w * max over columns c with c % period != 0 (best reference patch, class-token columns
 *   skipped; :260-261);  bilinear_ac: align_corners=True resize, optionally 1 - x (:265-268). */
int mh_l2norm_rows(const float* x, long ldx, void* y_bf16, float* y_f32, long ldy, int M, int D, float eps, mh_stream_t s);
int mh_pair_logits(const float* p, long ldp, const float* text, float* out, long rows, int rows_per_batch, int C, float scale,
                   mh_stream_t s);
int mh_zs_accumulate(const float* logits, float* mask_acc, float* map_acc, int B, int h, int S, float w, mh_stream_t s);
int mh_rowmax_skip(const float* scores, long lds, float* acc, long rows, int cols, int period, float w, mh_stream_t s);
int mh_bilinear_ac(const float* in, float* out, int B, int h, int w, int H, int W, int one_minus, mh_stream_t s);

/* K16b the one-shot head against a per-class reference bank (csrc/expert_bank.hip): the references of a class are encoded once
 * and kept as L2-normalised bf16 patch rows, one contiguous [R_total, D] bank per tap; a sample names its class by the row range
 * [bank_off[b], bank_off[b] + bank_rows[b]) (int32 device arrays of B entries; bank_rows[b] >= 1 and the range inside the bank
 * are the caller's contract).
 * mh_bank_sim_max (one launch per tap, whole batch): the query row of sample b, patch l is row b * q_sample_rows + q_row0 + l
 *   of q [*, D] bf16 (q_row0 = 1, q_sample_rows = 1 + L skips each sample's class token); part[(b * max_chunks + c) * L + l] =
 *   max_j <q[b, l], bank[bank_off[b] + j]> over the rows j of chunk c (mh_bank_sim_chunk_rows() rows each, the last one
 *   shorter), for c < ceil(bank_rows[b] / chunk rows); slots of later chunks are not written.  bf16 MFMA products, fp32
 *   accumulation along D in one fixed ascending order; rows past a class's end are masked to -inf, never read from the
 *   neighbouring class; the score matrix is never stored.  max_chunks >= the largest chunk count in the batch (workgroups past
 *   a sample's last chunk exit at once).  Refuses D % 32, L < 1, B < 1, max_chunks < 1, q_sample_rows < q_row0 + L and null
 *   pointers with MH_ERR_ARG before any launch.
 * mh_bank_sim_finish (one launch): part [T, B, max_chunks, L = h h] of T taps; sim[b, l] = sum over taps in ascending order of
 *   w * (max over the sample's chunks), as rowmax_skip accumulates it; simmask [B, h, h] = 1 - sim; amap [B, S, S] = 1 -
 *   bilinear_ac(sim): both bit-equal to mh_bilinear_ac(sim, ..., one_minus = 1) at (h, h) and (S, S).  h <= 128, S <= 4096. */
int mh_bank_sim_chunk_rows(void);
int mh_bank_sim_max(const void* q, long q_row0, long q_sample_rows, const void* bank, const int* bank_off, const int* bank_rows,
                    float* part, int B, int L, int D, int max_chunks, mh_stream_t s);
int mh_bank_sim_finish(const float* part, const int* bank_rows, float* sim, float* simmask, float* amap, int T, int B,
                       int max_chunks, int h, int S, float w, mh_stream_t s);

/* K16c greedy k-centre (farthest-point) coreset selection over one class of the reference bank (csrc/coreset.hip;
 * vision_expert.py: compact_references; the rule and its cover guarantee are DESIGN section 6).  taps: a HOST array of T device
 * pointers, one row-major bf16 matrix per tap with row stride ld elements; the class is the rows [row0, row0 + rows) of each.
 *   dist2(i, s) = sum over taps and columns of (x_t[i, k] - x_t[s, k])^2, bf16 widened to fp32, one fixed fp32 order that
 *   depends on (D, T) alone;  sel[0] = start, radius2[0] = +inf;  step j: mind[i] = min(mind[i], dist2(i, sel[j])) for every
 *   row of the class, mind[sel[j]] = -1;  sel[j + 1] = the lowest index among the rows of largest mind, radius2[j + 1] = that
 *   maximum;  cover2 = max mind after the last step (-1 when n == rows).
 * Outputs (device): sel [n] int32 (indices relative to row0), radius2 [n], mind [rows], cover2 [1]; mind need not be
 * initialised.  2 n launches on `s`, no host synchronisation, no float atomics: bitwise reproducible, and independent of row0
 * and of the rows outside the class, which are never read.  ws: mh_coreset_ws_bytes(rows) bytes of device scratch, 8-byte
 * aligned (one 8-byte arg-max partial per workgroup of 64 consecutive rows).  Cover guarantee for unit rows and a head that
 * takes the mean over taps of the per-tap maximum: 0 <= sim_full - sim_coreset <= sqrt(cover2) for any query.
 * MH_ERR_ARG, with nothing launched and nothing written, for a null pointer (the T tap pointers included; they must be 16-byte
 * aligned), T outside 1..8, D < 8 or D % 8, ld < D or ld % 8, row0 < 0, rows < 1, n outside 1..rows, start outside
 * 0..rows-1, a short workspace; MH_ERR_UNSUPPORTED for T * D > 16384 (the centre row staged in LDS: T = 8, D = 2048). */
long mh_coreset_ws_bytes(int rows);
int mh_coreset_select(const void* const* taps, int T, long ld, int D, long row0, int rows, int n, int start, int* sel,
                      float* radius2, float* mind, float* cover2, void* ws, long ws_bytes, mh_stream_t s);

/* K17 streaming localisation metrics for anomaly maps (csrc/seg_metrics.hip; seg_metrics.py, eval_protocol.seg_metrics_from_hist).
 * mh_mask_components: 8-connected components of B binary masks [B, H, W] (one byte per pixel, nonzero = anomalous), one workgroup
 *   per image with the union-find in LDS.  labels [B, H, W] int32: -1 on background, else the smallest linear index y W + x of
 *   the pixel's component; area [B, H, W] int32: the component's pixel count at that pixel, 0 elsewhere; n_regions [B] int32.
 *   Every element of the three outputs is written.  H W <= 65536 and (2 ceil(H/2) ceil(W/2) + 1) * 4 bytes of LDS <= 160 KiB (true
 *   for every image with both sides >= 4); anything else is refused with MH_ERR_ARG before any launch.
 *   mh_mask_components_lds_bytes: that LDS size, or -1 where the image is refused.
 * mh_seg_hist_update: hist [3, 2^20] int64 and counters [4] int64 are added to, with integer atomics only (the result does not
 *   depend on arrival order).  The key of a score is the top 20 bits of the order-preserving transform of its fp32 bits (-0 as +0;
 *   negative: all bits flipped; else the sign bit set); maps [B, H, W] fp32, or bf16 (maps_bf16 = 1; keyed exactly).  Row 0 counts
 *   the normal pixels per key, row 1 the anomalous ones, row 2 receives floor(2^40 / area of its region) per anomalous pixel
 *   (labels / area: mh_mask_components' outputs for `masks`).  counters: pixels, anomalous pixels, regions, non-finite scores; a
 *   NaN or +-inf score is counted there and nowhere in hist.  aggregate = 1: the lanes of a wave that share (row, key) add once;
 *   0: one atomic per lane.  Same sums either way. */
long mh_mask_components_lds_bytes(int H, int W);
int mh_mask_components(const void* masks, int* labels, int* area, int* n_regions, int B, int H, int W, mh_stream_t s);
int mh_seg_hist_update(long long* hist, long long* counters, const void* maps, int maps_bf16, const void* masks, const int* labels,
                       const int* area, int B, int H, int W, int aggregate, mh_stream_t s);

/* ---- opaque context: library state the caller owns explicitly ------------------------------------------------
 * An mh_ctx holds (1) a split-K scratch record -- mh_ctx_set_workspace(ctx, NULL, ptr, bytes) the main scratch,
 * (ctx, stream, ptr, bytes) that of one more stream that may split K concurrently; library calls use the record of the context
 * made current by mh_ctx_make_current (NULL = the process default that mh_set_workspace fills) -- and (2) the gradient
 * exchange of the data-parallel step (runner_base.py:94-98): an RCCL communicator, a side HIP stream and two events.
 * mh_ctx_comm_id writes the 128-byte id rank 0 generates; every rank passes it to mh_ctx_comm_init(ctx, id, rank, world).
 * mh_allreduce_start(ctx, buf, n, producer): in-place sum of buf[0..n) f32 over the ranks on the context's side stream, ordered
 * after what `producer` has queued; returns at once.  mh_allreduce_wait(ctx, consumer): `consumer` waits on the device for it.
 * RCCL is dlopen'ed by the comm calls only (MH_ERR_UNSUPPORTED if it cannot be loaded); world == 1 needs no communicator. */
typedef struct mh_ctx mh_ctx;
int mh_ctx_create(mh_ctx** out);
int mh_ctx_destroy(mh_ctx* ctx);
int mh_ctx_set_workspace(mh_ctx* ctx, mh_stream_t stream, void* ptr, long bytes);
int mh_ctx_make_current(mh_ctx* ctx);
int mh_ctx_comm_id(void* id128);
int mh_ctx_comm_init(mh_ctx* ctx, const void* id128, int rank, int world);
int mh_ctx_world(const mh_ctx* ctx);
int mh_allreduce_start(mh_ctx* ctx, float* buf, long n, mh_stream_t producer);
/* Round 4: wire type per call (MH_DT_F32 / MH_DT_BF16 elements) and the two halves of the sharded exchange
 * (runner.DataParallel mode 'rs_ag': reduce-scatter the gradients, AdamW on the own 1/world shard, all-gather the parameters).
 * mh_reduce_scatter_start: recv[0..n_per_rank) = sum over ranks of their send[rank * n_per_rank ..); send holds world *
 * n_per_rank elements.  mh_allgather_start: recv[r * n_per_rank ..) = rank r's send[0..n_per_rank).  Verbs started back to
 * back queue on the context's side stream; one mh_allreduce_wait covers everything started so far. */
#define MH_DT_F32 0
#define MH_DT_BF16 1
int mh_allreduce_start_dt(mh_ctx* ctx, void* buf, long n, int dt, mh_stream_t producer);
int mh_reduce_scatter_start(mh_ctx* ctx, const void* send, void* recv, long n_per_rank, int dt, mh_stream_t producer);
int mh_allgather_start(mh_ctx* ctx, const void* send, void* recv, long n_per_rank, int dt, mh_stream_t producer);
int mh_allreduce_wait(mh_ctx* ctx, mh_stream_t consumer);

/* library identity */
const char* mh_version(void);
int mh_target_arch(void); /* 950 */

/* Options: process-wide on/off switches between code paths that compute the same thing (the fused and the separate form of
 * an op are bit-identical; tests flip them to prove it) or between stated precisions.  Each starts from its MYRIAD_<NAME>
 * environment variable when set ("0" = off), else from the default:
 *   slab_bf16 (1)       bf16 split-K slabs of the 256x256 kernel; 0 = fp32 slabs
 *   gemm_skinny (1)     160-row tiles for 128 < M <= 320
 *   swiglu_fused (1)    SiLU gate in the epilogues of the gate|up forward / down dgrad GEMMs
 *   gelu_fused (1)      erf-GELU in the epilogues of the Q-Former MLP GEMMs
 *   attn_bwd_split (1)  two workgroups per (batch, head) in mh_attn_rope_bwd when B*H <= 128
 *   gemm_zero_pad (1)   rows past M / N of a 256x256 tile read as zeros; 0 = as copies of the last row
 *   gemm256_impl (1)    plan kernel 2 = gemm_x8_kernel; 0 = gemm_256_kernel
 *   lora_norm_fused (1) LoRA dx + input-norm backward as one kernel (mh_gemm_lora_rmsnorm_bwd); 0 = the two launches
 *   attn_full (1)       mh_attn_fwd without mask / bias and with Sk <= 288, head dim in (32, 96]: one workgroup stages the whole
 *                       K and V of a (batch, head) (attn_full.hip) instead of 64x64 tiles; 0 = the tiled kernel
 *   lora_wgrad_mfma (1) mh_lora_wgrad at r = 8, D % 128 == 0: the sums over token rows as MFMA products (per-row scalars as a bf16 head +
 *                       bf16 remainder, fp32 accumulation); 0 = the thread-per-column fp32 kernel
 *   gemm_skip_pad (1)   256x256 kernel: a wave whose rows lie past M but for at most two 16-row fragments issues no MFMAs for the others
 *                       (same results; the chip's clock under this loop is set by the matrix pipes' power); 0 = every wave runs the full loop
 *   gemm_split_xcd (1)  256x256 kernel, K-split launches: the workgroups of one XCD (round-robin dispatch, private L2) own ONE K split of a
 *                       band of tile columns, so each L2 streams its A panels' K range once; 0 = every XCD runs all splits of a tile
 *                       block and reads the whole A matrix (same results, the mapping only moves workgroups)
 * mh_set_option returns the previous value (0 / 1) or MH_ERR_ARG (unknown name, value not 0 / 1); mh_get_option the current
 * value or MH_ERR_ARG.  Not thread-safe against concurrent launches. */
int mh_set_option(const char* name, int value);
int mh_get_option(const char* name);
/* self-check of the hardware fp32 -> bf16 rounding (v_cvt_pk_bf16_f32) against the integer round-to-nearest-even form:
   hw / hw_pk / sw [n] bf16 = scalar conversion, packed conversion, integer form of x[n] (n even) */
int mh_bf16_round_check(const float* x, void* hw, void* hw_pk, void* sw, long n, mh_stream_t s);

/* K17 image front-end (data path, SURVEY 8 f-2 image side): what datasets/datasets/anomaly_detection.py:118-122,246 and
 * processors/blip_processors.py:21-29,120-147,189-203 do on the CPU with torchvision + Pillow -- Resize(BICUBIC) ->
 * CenterCrop -> ToTensor -> Normalize -- for one uint8 RGB image resident in HBM, bit-exact with Pillow's 8-bit resampler.
 * kh/bh, kv/bv: 22-bit fixed-point weights [res][ksz] and (first, count) bounds [res][2] of the full resize per axis (device
 * ints, built by the host exactly as Resample.c builds them); (crop_y0, crop_x0, out_h, out_w) the kept window; (y0, rows)
 * the input rows that window taps; tmp rows*out_w*3 bytes; lut [3][256] float = ((v/255) - mean) / std in float32.
 * out [3][out_h][out_w] f32 and/or u8_out [out_h][out_w][3] (the uint8 crop the NSA augmentation edits). */
int mh_image_resize_crop_norm(const void* img, int H, int W, long row_stride, const int* kh, const int* bh, int ksz_h,
                              const int* kv, const int* bv, int ksz_v, int crop_y0, int crop_x0, int out_h, int out_w, int y0,
                              int rows, void* tmp, const float* lut, float* out, void* u8_out, mh_stream_t s);
int mh_image_u8_normalize(const void* u8_hwc, long n_pix, const float* lut, float* out, mh_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
