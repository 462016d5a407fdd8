/*
 * tw_hip.h — C-ABI of libtw_hip.so, the MI355X (gfx950) kernels behind the taiwan-whisper
 * distillation hot path.
 *
 * The reference has no native plugin API: its hot path calls HF
 * Transformers / ATen / cuBLAS / SDPA / NCCL implicitly.  Each entry point below replaces
 * one of those implicit kernels and cites the reference line that triggers it.  The
 * Python host package (taiwan-whisper_amd/tw) binds these with ctypes; INTEGRATION.md shows
 * the binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain device pointers, int64 leading dimensions in ELEMENTS, row-major;
 *   - dtype codes: 0 = fp32, 1 = bf16, 2 = fp16;
 *   - every call is stream-ordered on `stream` (a hipStream_t), never synchronises,
 *     never allocates; workspaces are caller-provided;
 *   - return 0 on success, 1 = invalid argument/shape, 2 = unsupported, 3 = HIP launch error;
 *   - the library holds no global mutable state; calls are reentrant.
 */
#ifndef TW_HIP_H
#define TW_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* tw_stream_t; /* hipStream_t */

/* GEMM flags */
#define TW_GEMM_BIAS 1
#define TW_GEMM_ROUND 2
#define TW_GEMM_GELU 4
#define TW_GEMM_RES 8
#define TW_GEMM_ACCUM 16
#define TW_GEMM_AUX_OUT 32
#define TW_GEMM_DGELU 64
#define TW_GEMM_TILE128 256   /* force the 128x128 tile (A/B benchmarking) */
#define TW_GEMM_TILE256 512   /* force the 256x256 tile */
#define TW_GEMM_TILE256x128 1024  /* force the 256x128 tile with the 3-stage LDS ring */
#define TW_GEMM_TILE256PP 2048    /* force the 256x256 ping-pong kernel (a_trans = b_trans = 0 only) */
#define TW_GEMM_NOSPLIT 16384     /* no split-K and no whole-rounds + tail split */
#define TW_GEMM_TILE256x128_S2 262144  /* force the 256x128 tile with the 2-stage LDS ring */
#define TW_GEMM_GROUP_M(g) ((g) << 24) /* force the tile order: runs of g (1..15) m-tiles */


/* bf16 MFMA GEMM  C[b] = epi(alpha * A[b] . B[b]^T), A [M][K] (a_trans: [K][M]), B [N][K] (b_trans: [K][N]).
 * Replaces every nn.Linear / Conv1d (as GEMM) / tied proj_out matmul of the step, forward and
 * backward: HF modeling_whisper.py:279-345 (q/k/v/out_proj), :618-619 (conv1/conv2), :400-410 and
 * :495-505 (fc1 + GELU + fc2), :1080 (proj_out); run_distillation.py:1528,1534,1665 (fwd, teacher fwd, backward).
 * Epilogue order: +bias[n] (bf16) -> ROUND to bf16 -> DGELU (x gelu'(aux)) -> GELU (aux <- pre-act)
 *   -> +res[m % res_mod][n] -> +C_old (ACCUM) -> store as c_dtype.  K % 8 == 0 unless both operands are MN-major; a_trans needs M % 8 == 0,
 *   b_trans needs N % 8 == 0; lda, ldb % 8 == 0; A, B 16-byte aligned. */
int tw_gemm_bf16(const void* A, int64_t lda, int a_trans, const void* B, int64_t ldb, int b_trans, void* C,
                 int64_t ldc, int c_dtype, int M, int N, int K, int batch, int64_t sA, int64_t sB, int64_t sC,
                 float alpha, const void* bias, const void* res, int64_t ldr, int64_t sR, int res_dtype, int res_mod,
                 void* aux, int64_t ldaux, int64_t sAux, int flags, tw_stream_t stream);

/* How tw_gemm_bf16 (is_f16 = 0) / tw_gemm_f16 (is_f16 = 1) would run a call: the same validation and the same
 * planner, nothing launched, host only.  The arguments are the call's (without alpha and the stream); the pointers
 * are looked at for their alignment only, never dereferenced.  cus > 0: plan for that many CUs without calling
 * into HIP (works on a host without a GPU); cus = 0: the current device's count.  have_ws = 0: the plan of a call
 * that cannot get the split-K workspace (inside a stream capture when the block would have to grow).
 * out[6] = route, S (K chunks; 1 for the unsplit skinny kernel, 0 where K is not split), m_dp (m-tile rows of 256 on
 * the persistent kernel in routes 3 and 4), split_tile (128 / 256 in route 2), group_m, epilogue kind.  Routes:
 * 0 skinny, 1 skinny split-K, 2 dW split-K, 3 whole rounds + split-K tail, 4 whole rounds + 128x128 tail,
 * 5 persistent 256x256, 6 persistent + fp16 edge strips, 7 128x128 2-stage, 8 128x128 4-stage ring, 9 256x256
 * 2-stage, 10 256x128 3-stage ring, 11 256x128 2-stage ring; -1: nothing to compute.  Returns what the call would. */
int tw_gemm_route(const void* A, int64_t lda, int a_trans, const void* B, int64_t ldb, int b_trans, void* C,
                  int64_t ldc, int c_dtype, int M, int N, int K, int batch, int64_t sA, int64_t sB, int64_t sC,
                  const void* bias, const void* res, int64_t ldr, int64_t sR, int res_dtype, int res_mod, void* aux,
                  int64_t ldaux, int64_t sAux, int flags, int is_f16, int cus, int have_ws, int* out);

/* Decode-step Linear for up to 4 rows (batch-1 long-form): C = epi(A . W^T), one output column per wave.
 * A = x [M][K] bf16, or LayerNorm(x) when ln_w != NULL (fp32 gamma ln_w / beta ln_b, eps; K % 256 == 0;
 * A is bit-identical to tw_layernorm_fwd's bf16 output, so an LN launch + GEMM pair becomes one launch).
 * Replaces, per decode step, HF WhisperDecoderLayer's LayerNorm + nn.Linear pairs and the plain Linears
 * (modeling_whisper.py:448-506) for a batch of <= 4.  W [N][K] bf16; flags / bias / res / aux as
 * tw_gemm_bf16 (F_BIAS, F_ROUND, F_GELU, F_RES, F_AUX_OUT, F_ACCUM); C fp32 or bf16.  kv_cache != NULL fuses
 * tw_kv_append: columns n >= kv_col0 are also stored at kv_cache[m*kv_sb + (*t_dev)*kv_ld + n - kv_col0]
 * (the self-attention K/V row of the step, the fused QKV projection's k | v part). */
int tw_gemv_bf16(const void* x, int64_t ldx, const float* ln_w, const float* ln_b, float eps, const void* W,
                 int64_t ldw, void* C, int64_t ldc, int c_dtype, int M, int N, int K, const void* bias,
                 const void* res, int64_t ldr, int res_dtype, void* aux, int64_t ldaux, int flags,
                 void* kv_cache, int64_t kv_sb, int64_t kv_ld, int kv_col0, const int* t_dev, tw_stream_t stream);

/* LayerNorm fp32-statistics forward / backward (D % 64 == 0, D <= 1280).
 * Replaces nn.LayerNorm at HF modeling_whisper.py:392,402,470,485,498,642,790 (autocast fp32 op). */
int tw_layernorm_fwd(const void* x, int x_dtype, const float* w, const float* b, void* y, int y_dtype,
                     float* mean_out, float* rstd_out, int rows, int D, float eps, tw_stream_t stream);
/* Residual add fused into the LayerNorm that follows it (D % 256 == 0, 16-B aligned rows): x_out = x + r
 * (r = the preceding Linear's bf16 output: the HF residual `hidden_states = residual + hidden_states` at
 * modeling_whisper.py:399,412 / 479,495,506; fp32 stream x_dtype 0 under autocast, bf16 stream x_dtype 1
 * rounded once), y = bf16 LayerNorm(x_out).  x_out may alias x.  Bit-identical to tw_gemm_bf16's residual
 * epilogue followed by tw_layernorm_fwd. */
int tw_add_layernorm_fwd(const void* x, int x_dtype, const void* r, void* x_out, const float* w, const float* b,
                         void* y, float* mean_out, float* rstd_out, int rows, int D, float eps, tw_stream_t stream);
int tw_layernorm_bwd(const void* x, int x_dtype, const float* w, const float* mean, const float* rstd, const void* dy,
                     int dy_dtype, float* dx, int dx_accum, float* dw_out, float* db_out, int rows, int D,
                     float* workspace, int64_t workspace_floats, tw_stream_t stream);
/* tw_layernorm_bwd_ex: tw_layernorm_bwd that also writes g16 = the bf16 (g_dtype 1) / fp16 (2) rounding of the final dx
 * (the autocast cast of the stream gradient the preceding block's GEMMs read; g16 may be NULL). */
int tw_layernorm_bwd_ex(const void* x, int x_dtype, const float* w, const float* mean, const float* rstd, const void* dy,
                        int dy_dtype, float* dx, int dx_accum, float* dw_out, float* db_out, int rows, int D,
                        float* workspace, int64_t workspace_floats, void* g16, int g_dtype, tw_stream_t stream);

/* Flash attention, head_dim 64, bf16 (replaces SDPA at HF modeling_whisper.py:337-350 for encoder
 * self-attn, decoder causal self-attn and cross-attn).  lse: [B][H][Tq] fp32 (natural log).
 * scale must be > 0: the forward takes each row's max on the raw scores before scaling, so every bf16 / fp16
 * entry (tw_attn_fwd / _bwd, their _f16 and _varlen forms) returns TW_EINVAL for a zero, negative or NaN scale
 * before any launch.  (tw_attn_*_f32 scales the scores in its GEMM and takes the max afterwards: any scale.) */
int tw_attn_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                int64_t ldo, float* lse, int B, int H, int Tq, int Tk, int head_dim, int causal, float scale,
                tw_stream_t stream);
int tw_attn_bwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const void* O,
                int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ, int64_t lddq, void* dK,
                int64_t lddk, void* dV, int64_t lddv, int B, int H, int Tq, int Tk, int head_dim, int causal,
                float scale, float* workspace /* B*H*Tq floats */, tw_stream_t stream);
/* The same kernels over PACKED rows (the trainer's decoder: clip b keeps only its first n_b rows, the clips
 * concatenated).  offq: B + 1 cumulative query-row offsets (device int32): clip b's Q / O / dO / dQ rows are
 * offq[b] .. offq[b+1]-1; Mq = offq[B]; max_q = the longest clip (the grid's extent).  offk: the same for the
 * K / V / dK / dV rows (causal self-attention passes the query array), or NULL for dense keys at b*Tk (cross-attention);
 * Tk = the dense key count, or with offk the longest clip.  lse and the backward's workspace are [H][Mq] fp32 (entry
 * h*Mq + offq[b] + q).  Each clip's rows equal the dense entry called on that clip alone (B = 1) bit for bit; a clip
 * without queries gets zero dK / dV rows; nothing past row Mq is written.  _f16: fp16 tensors. */
int tw_attn_fwd_varlen(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                       int64_t ldo, float* lse, const int* offq, const int* offk, int B, int H, int Mq, int max_q, int Tk,
                       int head_dim, int causal, float scale, tw_stream_t stream);
int tw_attn_fwd_varlen_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                           int64_t ldo, float* lse, const int* offq, const int* offk, int B, int H, int Mq, int max_q,
                           int Tk, int head_dim, int causal, float scale, tw_stream_t stream);
int tw_attn_bwd_varlen(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                       const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ,
                       int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, const int* offq, const int* offk,
                       int B, int H, int Mq, int max_q, int Tk, int head_dim, int causal, float scale,
                       float* workspace /* H*Mq floats */, tw_stream_t stream);
int tw_attn_bwd_varlen_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                           const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ,
                           int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, const int* offq,
                           const int* offk, int B, int H, int Mq, int max_q, int Tk, int head_dim, int causal,
                           float scale, float* workspace, tw_stream_t stream);
/* The packed entries with a query-block list: the same arguments and results as the _varlen entries, and `blocks`,
 * one of the two lists of tw_pack_blocks (list 0 with dense keys, list 1 for the causal call with offk), with its
 * length nblk.  The forward and dQ launch one workgroup per (entry, head); dK / dV keep their key-side grid.  No
 * workgroup is launched for rows that no clip has, and every row's bits are those of the _varlen entries.  blocks
 * must be 16-byte aligned. */
int tw_attn_fwd_blocks(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                       int64_t ldo, float* lse, const int* offq, const int* offk, const int* blocks, int nblk,
                       int B, int H, int Mq, int max_q, int Tk, int head_dim, int causal, float scale,
                       tw_stream_t stream);
int tw_attn_fwd_blocks_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                           int64_t ldo, float* lse, const int* offq, const int* offk, const int* blocks, int nblk,
                           int B, int H, int Mq, int max_q, int Tk, int head_dim, int causal, float scale,
                           tw_stream_t stream);
int tw_attn_bwd_blocks(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                       const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ,
                       int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, const int* offq, const int* offk,
                       const int* blocks, int nblk, int B, int H, int Mq, int max_q, int Tk, int head_dim, int causal,
                       float scale, float* workspace /* H*Mq floats */, tw_stream_t stream);
int tw_attn_bwd_blocks_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                           const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ,
                           int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, const int* offq,
                           const int* offk, const int* blocks, int nblk, int B, int H, int Mq, int max_q, int Tk,
                           int head_dim, int causal, float scale, float* workspace, tw_stream_t stream);

/* Fused CE + temperature KL loss and its logits gradient (replaces run_distillation.py:1507-1516,
 * :1539-1549 and HF CE :1082-1087).  out3 = [loss, ce, kl*T^2]; dlogits (same dtype as the logits:
 * bf16 under autocast, fp32 on the fp32 path) may be NULL, or s_logits itself (the gradient written in place). */
int tw_kl_ce(const void* s_logits, const void* t_logits, int64_t ld, int logits_dtype, const int64_t* labels,
             int64_t rows, int V, float T, float ce_w, float kl_w, const int* n_valid, float grad_scale, float* row_out,
             float* out3, void* dlogits, tw_stream_t stream);

/* Whisper log-mel (replaces WhisperFeatureExtractor at run_distillation.py:1217).
 * wav [B][480000] fp32 -> mel_out [B][80][3000] fp32 and optional conv1 input [B][3002][80] bf16. */
int tw_logmel(const float* wav, int B, const float* basis, const int* mel_start, const float* mel_w, float* mel_out,
              void* conv_in, void* workspace /* B uint32 */, tw_stream_t stream);
/* Same front end over clips of any length (long-form inputs: HF __call__(truncation=False,
 * padding="longest"), run_eval.py:572-581): wav [B][n_samples] fp32 (shorter clips zero-padded to the
 * longest, as HF pads) -> mel_out [B][80][n_samples/160], conv_in [B][n_samples/160 + 2][80] bf16.
 * n_samples must exceed 200 (the reflect pad).  tw_logmel == tw_logmel_len(n_samples = 480000). */
int tw_logmel_len(const float* wav, int B, int64_t n_samples, const float* basis, const int* mel_start,
                  const float* mel_w, float* mel_out, void* conv_in, void* workspace, tw_stream_t stream);
/* The same front end with the mel count as an argument: n_mels = 80 (identical to tw_logmel_len) or 128
 * (the large-v3 family's num_mel_bins); any other count is TW_EINVAL.  mel_start [n_mels], mel_w [n_mels][32]
 * -> mel_out [B][n_mels][n_samples/160], conv_in [B][n_samples/160 + 2][n_mels] bf16. */
int tw_logmel_mels(const float* wav, int B, int64_t n_samples, int n_mels, const float* basis, const int* mel_start,
                   const float* mel_w, float* mel_out, void* conv_in, void* workspace, tw_stream_t stream);
int tw_mel_to_conv_input(const float* mel, void* xt, int B, int nmel, int T, tw_stream_t stream);

/* Decoder token + learned position embedding (HF modeling_whisper.py:736,754-761) and its
 * backward into the tied embedding gradient: deterministic (rows of one id summed in position order,
 * one writer per id); positions whose id == padding_idx add nothing (nn.Embedding's padding_idx,
 * = config.pad_token_id in HF WhisperDecoder; -1: none).  Scratch: the per-device block. */
int tw_embed_fwd(const int64_t* ids, const void* tok, int tok_dtype, const void* pos, int pos_dtype, void* out,
                 int out_dtype, int rows, int T, int pos_offset, int D, tw_stream_t stream);
int tw_embed_bwd(const int64_t* ids, const float* dh, float* dE, int rows, int D, int64_t padding_idx,
                 tw_stream_t stream);
/* Packed decoder rows.  tw_pack_plan: from labels [B][T], n_b = 1 + the last t with labels[b][t] >= 0 (0 without
 * one); off[0..B] (int32) = the running sum of n_b; src_rows[off[b] + t] = b*T + t for t < n_b, the padded row each
 * packed row came from (B*T entries, those past off[B] set to 0).
 * tw_embed_fwd_rows: tw_embed_fwd where row r takes position src_rows[r] % T.
 * tw_pos_grad_rows: gP[t] += sum over clips b with t < n_b of dx[off[b] + t] (fp32, clips in ascending order);
 * max_rows = the longest clip. */
int tw_pack_plan(const int64_t* labels, int B, int T, int* off, int64_t* src_rows, tw_stream_t stream);
/* The query blocks of packed rows, for tw_attn_*_blocks.  A block is 128 consecutive rows of one clip (the clip's last
 * block: what is left); from off [B+1] (max_rows >= the longest clip) two lists of the same blocks, entries of four
 * int32 {clip, first row, rows, tiles}: list 0 at blocks (dense keys; tiles = 0), list 1 at blocks + 4*cap (causal;
 * tiles = the 64-key tiles the block walks).  Order: descending tiles, ties by (clip, block).  *nblk = the number
 * of blocks.  cap >= B * ceil(max_rows / 128); blocks 16-byte aligned.  Deterministic (ranks, no atomics). */
int tw_pack_blocks(const int* off, int B, int max_rows, int* blocks, int cap, int* nblk, tw_stream_t stream);
int tw_embed_fwd_rows(const int64_t* ids, const int64_t* src_rows, const void* tok, int tok_dtype, const void* pos,
                      int pos_dtype, void* out, int out_dtype, int rows, int T, int pos_offset, int D,
                      tw_stream_t stream);
int tw_pos_grad_rows(const float* dx, const int* off, int B, int max_rows, int D, float* gP, tw_stream_t stream);

/* dst[c][r] = src[r][c], bf16 [rows][cols] (row stride ld_src) -> [cols][rows] (ld_dst): the tied
 * embedding as the K-major operand of the LM-head input gradient (dh = dlogits . E, K = vocabulary). */
int tw_transpose_bf16(const void* src, int64_t ld_src, int rows, int cols, void* dst, int64_t ld_dst,
                      tw_stream_t stream);
/* autocast weight cast fp32 -> bf16 (ACC:accelerator.py autocast of every Linear weight). */
int tw_cast_f32_bf16(const float* src, void* dst, int64_t n, tw_stream_t stream);
/* bias gradient: out[c] (+)= [round](sum_r x[r][c]) (round_bf16: 0 none, 1 to bf16, 2 to fp16; x fp32 / bf16 / fp16);
 * deterministic two-pass, workspace >= ceil(rows/64)*cols. */
int tw_colsum(const void* x, int x_dtype, int64_t ldx, int rows, int cols, float* out, int accum, int round_bf16,
              float* workspace, int64_t workspace_floats, tw_stream_t stream);

/* clip_grad_norm_ + AdamW (run_distillation.py:1450-1455,1666-1668). */
int tw_l2norm(const float* x, int64_t n, float* norm_out, float* workspace /* 1024 floats */, tw_stream_t stream);
int tw_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float b1, float b2,
             float eps, float wd, int step, const float* norm, float max_norm, tw_stream_t stream);
int tw_clip_scale(float* x, int64_t n, const float* norm, float max_norm, tw_stream_t stream);

/* conv-stem backward helpers (HF modeling_whisper.py:618-619). */
int tw_im2col3(const void* src, int64_t src_rows, void* dst, int B, int T_out, int stride, int C,
               tw_stream_t stream);
int tw_col2im_s2(const float* dA, float* dX, int B, int T_in, int T_out, int C, tw_stream_t stream);
/* GELU backward on a bf16 activation: out = bf16(bf16(g) * gelu'(pre)). */
int tw_gelu_bwd(const void* g, int g_dtype, const void* pre, void* out, int64_t n, tw_stream_t stream);

/* teacher decoder input = shift_tokens_right(labels) (run_distillation.py:1534, HF modeling_whisper.py:68-81);
 * number of labels >= 0 (kl_divergence normaliser, run_distillation.py:1512-1515). */
int tw_shift_tokens_right(const int64_t* labels, int64_t* out, int B, int T, int64_t pad, int64_t start,
                          tw_stream_t stream);
int tw_count_valid(const int64_t* labels, int64_t n, int* out, tw_stream_t stream);

/* Greedy decoding with a KV cache (generate_step run_distillation.py:1580-1584,
 * run_pseudo_labelling.py:917-922; HF generation_whisper.py greedy loop, per-step attention of
 * modeling_whisper.py:265-350 with past_key_values).
 * Position-independent steps (for graph capture): the step index t lives in device memory
 * (t_dev) and is read by the kernels that depend on it; tw_step_advance adds `by` to it.
 * tw_decode_attn: one query row per (batch b, head h): O[b][h*64..] = softmax(scale * q.K^T) V over
 * the first Tk key rows (Tk += *tk_dev when tk_dev != NULL); q at q + b*sqb + h*64, key j at
 * k + b*skb + j*ldk + h*64 (v alike), output at o + b*sob + h*64 (bf16).  head_dim 64, Tk <= 2048.
 * tw_greedy_select: HF SuppressTokens / SuppressTokensAtBegin (logits_process.py) + argmax
 * (lowest id on ties) over the first V logits of each bf16 row; suppress_bits / begin_bits are
 * V-bit masks; rows with done[b] != 0 emit eos; the token is written to ids[b*ld_ids + col] and
 * next_ids[b], and done[b] |= (token == eos).  With t_dev != NULL: col += *t_dev and the begin mask
 * applies when col == begin_col (apply_begin is ignored).
 * tw_embed_step: out[b] = tok[ids[b]] + pos[*t_dev] (decoder input embedding of one step).
 * tw_kv_append: cache[b*sb + (*t_dev)*ld_row + 0..n) = src[b*ld_src + 0..n) (16-B vectors: bf16 n % 8 == 0,
 * fp32 n % 4 == 0).
 * dtype / logits_dtype (0 = fp32, 1 = bf16) select the element type of q/K/V/O and of the logits rows:
 * bf16 under autocast, fp32 on the fp32 path (mixed_precision "no"). */
int tw_decode_attn(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, const void* v, int64_t ldv,
                   int64_t svb, void* o, int64_t sob, int B, int H, int Tk, const int* tk_dev, int head_dim,
                   float scale, int dtype, tw_stream_t stream);
/* tw_decode_attn_hs: tw_decode_attn with head strides for K and V -- key j of head h at k + b*skb + h*hsk + j*ldk
 * (v alike; tw_decode_attn is hsk = hsv = 64).  The head-major cross-attention K/V ([H][Tk][64] per clip:
 * hsk = Tk*64, ldk = 64) of ONE clip serve every row of a batch with skb = svb = 0 (the temperature-fallback batch
 * of one window: HF generate_with_fallback, generation_whisper.py; each row reads exactly the K/V of its batch-1
 * decode). */
int tw_decode_attn_hs(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, int64_t hsk,
                      const void* v, int64_t ldv, int64_t svb, int64_t hsv, void* o, int64_t sob, int B, int H, int Tk,
                      const int* tk_dev, int head_dim, float scale, int dtype, tw_stream_t stream);
/* tw_decode_attn_ks: tw_decode_attn_hs with a per-row key start -- k_start is a device array of B int32, and row b
 * attends keys [k_start[b], Tk) (Tk += *tk_dev as above).  It is the superset form: it takes the head strides, so
 * one entry serves the row-interleaved self-attention cache (hsk = hsv = 64) and head-major blocks, and with every
 * start 0 it computes what tw_decode_attn_hs computes (same kernels' bodies, same split rule: fixed Tk and fewer
 * than 640 (row, head) pairs split the keys into chunks; a chunk wholly below a row's start is empty).  Keys below
 * the start are never loaded, so a NaN / Inf in a masked K or V row cannot reach the output.  A start >= Tk (or
 * < 0) is clamped into [0, Tk - 1]: the last key is always attended and nothing outside [0, Tk) is read.  k_start
 * is read on the device, so a captured step stays valid when its contents change.  This is HF's decoder attention
 * mask for left-padded prompts (generation_whisper.py _prepare_decoder_input_ids with prompt_ids /
 * condition_on_prev_tokens): the pad columns' K/V sit in the cache and are masked from then on.  Row b's output is
 * bit-identical to tw_decode_attn_hs on that row alone with K / V advanced by k_start[b] rows and Tk - k_start[b]
 * keys (one-workgroup path).  bf16, fp16 and fp32. */
int tw_decode_attn_ks(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, int64_t hsk,
                      const void* v, int64_t ldv, int64_t svb, int64_t hsv, void* o, int64_t sob, int B, int H, int Tk,
                      const int* tk_dev, const int* k_start, int head_dim, float scale, int dtype, tw_stream_t stream);
/* tw_decode_attn_mq: tw_decode_attn_ks for Q consecutive query rows per batch row (1 <= Q <= 8) -- the verify pass
 * of assisted decoding (HF generate(assistant_model=...), run_eval.py:524-545,653-654), where the target scores
 * the k drafted tokens and the one before them in one pass.  Query j of row b is at q + b*sqb + j*sqq + h*64, its
 * output at o + b*sob + j*soq + h*64, and it attends keys [k_start[b], Tk + (causal ? j : 0)) (Tk += *tk_dev as
 * above; k_start may be NULL: every start 0; a start at or past a query's limit is clamped for that query as
 * tw_decode_attn_ks clamps it).  Every K and every V row is loaded once and used for all Q queries, so the 1500-frame
 * cross-attention K/V of a round is read once, not Q times; rows at or above the last query's limit and below the
 * start are never loaded.  Per query the arithmetic is that of the single-query body: the same lane layout, key
 * order, two-pass max / sum, the same split rule (fixed Tk and fewer than 640 (row, head) pairs, counted as for one
 * step; the chunk count from the last query's limit) and combine order, so query j's output is bit-identical to
 * tw_decode_attn_ks on that query alone with Tk + (causal ? j : 0) keys (for a causal call with a fixed Tk: when
 * every query falls on the same side of the split rule).  The one-workgroup path keeps the scores of the Q queries
 * in 48 KB of LDS: at most 12288 / Q' keys per query (Q' = Q rounded up to 1, 2, 4, 8; 1536 at Q = 8) -- a fixed Tk
 * beyond that returns 2, a device-side one is cut there.  4096 (row, head) pairs or more return 2.  bf16, fp16, fp32. */
int tw_decode_attn_mq(const void* q, int64_t sqb, int64_t sqq, const void* k, int64_t ldk, int64_t skb, int64_t hsk,
                      const void* v, int64_t ldv, int64_t svb, int64_t hsv, void* o, int64_t sob, int64_t soq, int B,
                      int H, int Q, int Tk, const int* tk_dev, const int* k_start, int causal, int head_dim,
                      float scale, int dtype, tw_stream_t stream);
/* tw_spec_accept: acceptance and rollback of one round of assisted decoding, one row, on the device (nothing is
 * synchronised with the host).  Before the call: *t_dev = t, the column of the last accepted token; drafts[0..k) the
 * assistant's tokens for columns t+1 .. t+k; ids[t+1 .. t+k+1] the target's tokens (the selection kernels, one launch
 * per logit row of the verify pass); slots[0..k] the log-prob each of those launches added to its own zeroed slot
 * (NULL together with sum_logp when nothing is tracked); done_snap the row's finished flag as it was before the
 * round.  n = the number of leading drafts equal to the target's token at the same column, counted up to and
 * including the first eos; the accepted tokens are the n + 1 target tokens at t+1 .. t+n+1, cut at column t_cap - 1
 * (the length cap: ids, the caches and the position lookups need k + 1 spare columns / rows past it).  The kernel
 * refills ids past the last accepted column (up to t+k+1) with eos, sets cur (and cur_a) to the last accepted token,
 * *t_dev (and *t_dev_a) to its column, done (done_a, and done_snap for the next round) from the snapshot and the
 * accepted tokens, last_ts (last_ts_a; NULL without timestamps) to the last token >= ts_begin among columns
 * begin_col .. the last accepted one (-1: none), adds the accepted slots to sum_logp in position order -- the
 * sequential decode's fp32 additions -- and zeroes the slots.  hist (nullable): hist[0] counts the rounds,
 * hist[1 + r] = n of round r while 1 + r < hist_cap.  A round that starts finished or at the length cap changes
 * nothing but the eos refill. */
int tw_spec_accept(const int64_t* drafts, int k, int64_t* ids, int t_cap, int64_t eos, int* t_dev, int* t_dev_a,
                   int64_t* cur, int64_t* cur_a, uint8_t* done, uint8_t* done_a, uint8_t* done_snap, int* last_ts,
                   int* last_ts_a, int begin_col, int ts_begin, float* slots, float* sum_logp, int* hist,
                   int hist_cap, tw_stream_t stream);
/* tw_spec_accept_lp: tw_spec_accept with tok_logp, this row of the per-token log-prob matrix (NULL: tw_spec_accept;
 * non-NULL needs slots).  Column t+1+j takes slots[j] for each accepted j < the accepted count -- the values added to
 * sum_logp, in the same order -- and the columns rolled back, up to t+k+1 (those refilled with eos), take 0.0f; the
 * row holds the ids' columns (t_cap + k + 1).  Everything else is tw_spec_accept's; the same error returns. */
int tw_spec_accept_lp(const int64_t* drafts, int k, int64_t* ids, int t_cap, int64_t eos, int* t_dev, int* t_dev_a,
                      int64_t* cur, int64_t* cur_a, uint8_t* done, uint8_t* done_a, uint8_t* done_snap, int* last_ts,
                      int* last_ts_a, int begin_col, int ts_begin, float* slots, float* sum_logp, float* tok_logp,
                      int* hist, int hist_cap, tw_stream_t stream);
/* tw_embed_step_multi: out[j] = tok[ids[j]] + pos[min(*t_dev + j, npos - 1)] for the Q consecutive positions of
 * one row (the verify pass; Q = 1: a step whose position is clamped to the table). */
int tw_embed_step_multi(const int64_t* ids, const void* tok, int tok_dtype, const void* pos, int pos_dtype, void* out,
                        int out_dtype, int Q, int D, const int* t_dev, int npos, tw_stream_t stream);
int tw_greedy_select(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                     const uint32_t* begin_bits, int apply_begin, int64_t eos, uint8_t* done, int64_t* ids,
                     int64_t ld_ids, int col, int64_t* next_ids, const int* t_dev, int begin_col, tw_stream_t stream);
/* tw_greedy_select_ts: as tw_greedy_select plus HF WhisperTimeStampLogitsProcessor (applied after the
 * suppress masks): <|notimestamps|> (no_ts) masked, pair / monotonicity rules from the previous two
 * generated tokens (columns >= begin_col of ids) and last_ts[b] (the row's last emitted timestamp,
 * -1 = none; updated here), the window's first step limited to timestamps <= ts_begin + max_initial
 * (max_initial < 0: no limit), and timestamps forced when logsumexp over them exceeds the best text
 * logit.  col += *t_dev when t_dev != NULL. */
int tw_greedy_select_ts(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                        const uint32_t* begin_bits, int64_t eos, uint8_t* done, int64_t* ids, int64_t ld_ids, int col,
                        int64_t* next_ids, const int* t_dev, int begin_col, int ts_begin, int no_ts, int max_initial,
                        int* last_ts, tw_stream_t stream);
/* Temperature fallback (HF generate_with_fallback, generation_whisper.py:970-1090; _need_fallback :1243-1290;
 * _retrieve_avg_logprobs :1958-1975; WhisperNoSpeechDetection logits_process.py:2050-2112).
 * tw_select_sample[_ts]: tw_greedy_select[_ts] with ctl = device int32[3] {bits of 1/T, seed lo, seed hi}
 * (1/T == 0: argmax; else Gumbel-max sampling over the processed row, i.e. multinomial(softmax(x/T)) with
 * a counter-based hash RNG keyed by (seed, b, col, id) -- not torch's RNG stream) and, when sum_logp !=
 * NULL, sum_logp[b] += log_softmax(processed row)[chosen] for rows not yet finished (the eos step
 * included).  B, V < 2^21.
 * tw_token_logprob: out[b] = log_softmax(logits[b*ld + 0..V))[token] (the no-speech probability is
 * exp(out) at the <|startoftranscript|> position). */
int tw_select_sample(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                     const uint32_t* begin_bits, int apply_begin, int64_t eos, uint8_t* done, int64_t* ids,
                     int64_t ld_ids, int col, int64_t* next_ids, const int* t_dev, int begin_col, const uint32_t* ctl,
                     float* sum_logp, tw_stream_t stream);
int tw_select_sample_ts(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                        const uint32_t* begin_bits, int64_t eos, uint8_t* done, int64_t* ids, int64_t ld_ids, int col,
                        int64_t* next_ids, const int* t_dev, int begin_col, int ts_begin, int no_ts, int max_initial,
                        int* last_ts, const uint32_t* ctl, float* sum_logp, tw_stream_t stream);
/* tw_select_sample[_ts]_lp: tw_select_sample[_ts] that also keeps the step's log-prob per column
 * (generate(return_token_logprobs=True)).  For every row b, tok_logp[b*ld_lp + c] = the fp32 value the call adds to
 * sum_logp[b], c the column the token goes to (col (+ *t_dev), as for ids): written for rows not yet finished, the
 * eos step included; a row that was already finished gets 0.0f, so every generated column is written once per decode.
 * The value is the log-softmax of the processed row at the chosen token: after the suppress and begin-suppress
 * masks, the timestamp rules and the repeat pre-pass (tw_repeat_process), of x itself when sampling at temperature T
 * (scores * T) -- HF's _retrieve_avg_logprobs convention, not the raw-logit one.  The row's owner thread stores
 * it; the selection, ids, done, last_ts and sum_logp are those of tw_select_sample[_ts] on the same inputs, bit for bit, and the stored values added
 * in column order in fp32 reproduce sum_logp.  sum_logp or tok_logp may be NULL, not both; with tok_logp NULL the
 * call is tw_select_sample[_ts].  ld_lp >= 1 + the largest column written (checked when t_dev == NULL).  Returns 1
 * for a bad shape or a null pointer (both of sum_logp and tok_logp among them), 2 for a dtype other than bf16 / fp16
 * / fp32 or B, V >= 2^21; nothing is written on error. */
int tw_select_sample_lp(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                        const uint32_t* begin_bits, int apply_begin, int64_t eos, uint8_t* done, int64_t* ids,
                        int64_t ld_ids, int col, int64_t* next_ids, const int* t_dev, int begin_col,
                        const uint32_t* ctl, float* sum_logp, float* tok_logp, int64_t ld_lp, tw_stream_t stream);
int tw_select_sample_ts_lp(const void* logits, int64_t ld, int logits_dtype, int B, int V,
                           const uint32_t* suppress_bits, const uint32_t* begin_bits, int64_t eos, uint8_t* done,
                           int64_t* ids, int64_t ld_ids, int col, int64_t* next_ids, const int* t_dev, int begin_col,
                           int ts_begin, int no_ts, int max_initial, int* last_ts, const uint32_t* ctl,
                           float* sum_logp, float* tok_logp, int64_t ld_lp, tw_stream_t stream);
int tw_token_logprob(const void* logits, int64_t ld, int logits_dtype, int B, int V, int token, float* out,
                     tw_stream_t stream);
/* tw_repeat_process: HF RepetitionPenaltyLogitsProcessor then NoRepeatNGramLogitsProcessor (logits_process.py;
 * generate(repetition_penalty=, no_repeat_ngram_size=)), the two processors GenerationMixin._get_logits_processor
 * runs before Whisper's own -- a pre-pass in front of the selection kernels above, which then take `out` as an fp32
 * row.  For each row b, out[b*ld_out + 0..V) = the first V logits of the row as fp32 (bf16, fp16 or fp32 in; the
 * output is always fp32 and never in place: HF upcasts 16-bit logits before any processor, and a penalised value
 * rounded back to 16 bits would move ties), processed for the history ids[b*ld_ids + 0..L), L = col + (t_dev ?
 * *t_dev : 0) -- the column the selection kernel is about to write; the whole decoder row so far counts, pad and
 * prompt columns included, as in HF:
 *   penalty != 1: every distinct token u of the history gets s[u] < 0 ? s[u] * penalty : s[u] / penalty, one
 *     correctly rounded fp32 operation on the unpenalised score (-0.0 and NaN take the quotient);
 *   ngram > 0: for every i in [0, L - ngram] with ids[i .. i+ngram-1) == ids[L-ngram+1 .. L), s[ids[i+ngram-1]] =
 *     -inf, after the penalty (ngram 1 bans every token of the history; L < ngram bans nothing).
 * penalty 1 and ngram 0 copy the row.  History ids outside [0, V) are ignored.  Input columns [V, ld) are never
 * used (they may hold NaN), output columns [V, ld_out) are not written.  Returns 1 for penalty <= 0 (or NaN),
 * ngram < 0, col < 0, B <= 0, V <= 0, ld < V or ld_out < V, 2 for another dtype; nothing is written then. */
int tw_repeat_process(const void* logits, int64_t ld, int logits_dtype, int B, int V, const int64_t* ids,
                      int64_t ld_ids, int col, const int* t_dev, float penalty, int ngram, float* out, int64_t ld_out,
                      tw_stream_t stream);
/* tw_lang_detect: HF WhisperGenerationMixin.detect_language on the logits of the <|startoftranscript|> step
 * (generation_whisper.py: every non-language logit masked to -inf, argmax).  lang_ids: a device table of L language
 * token ids (1 <= L <= 256), ascending and unique, each in [0, V).  The C entry cannot look into device memory: the
 * table is checked on the host where it is built (tw/generation.py language_table); the kernel reads an id outside
 * [0, V) as -inf rather than touching the row.  Per row b, in fp32 on the widened values x[j] = logits[b*ld +
 * lang_ids[j]] (bf16, fp16 or fp32 in; columns [V, ld) are never read):
 *   out_ids[b*id_stride] = lang_ids[argmax_j x[j]] with torch.argmax's rule: ties to the lowest id, a NaN above every
 *     number and the lowest-id NaN first; a row whose language logits are all -inf gives the lowest language id (HF's
 *     argmax over the whole masked row would give token 0 there: a difference no real checkpoint reaches, since its
 *     logits are finite).  id_stride >= 1 in elements: 1 for a plain [B] vector, T for column c of a [B][T] id matrix
 *     (out_ids pointing at that column); the other elements are not written.
 *   out_probs (may be NULL) [B][ld_p], ld_p >= L: out_probs[b][j] = expf(x[j] - max) / sum_j expf(x[j] - max), the
 *     softmax over the L language logits alone, in table order; a row that holds a NaN, or only -inf, gives NaN.
 *     Columns [L, ld_p) are not written.
 * One wave per row, every output element written once; no host read and no allocation (capturable in a graph).
 * Returns 1 for B < 0, V <= 0, ld < V, L < 1, L > 256, id_stride < 1, ld_p < L with out_probs given, or a null
 * logits / lang_ids / out_ids; 2 for another dtype; nothing is written then.  B == 0 is TW_OK with nothing launched. */
int tw_lang_detect(const void* logits, int64_t ld, int logits_dtype, int B, int V, const int* lang_ids, int L,
                   int64_t* out_ids, int64_t id_stride, float* out_probs, int64_t ld_p, tw_stream_t stream);
int tw_embed_step(const int64_t* ids, const void* tok, int tok_dtype, const void* pos, int pos_dtype, void* out,
                  int out_dtype, int B, int D, const int* t_dev, tw_stream_t stream);
/* tw_embed_step_off: out[b] = tok[ids[b]] + pos[max(*t_dev - pos_off[b], 0)] -- pos_off a device array of B int32,
 * the left-pad count of each row: positions counted from the row's first real token, the rule HF derives from an
 * attention mask ((mask.cumsum(-1) - 1).clamp(min=0), generation/utils.py); a padded row then decodes what its
 * unpadded prompt decodes. */
int tw_embed_step_off(const int64_t* ids, const void* tok, int tok_dtype, const void* pos, int pos_dtype, void* out,
                      int out_dtype, int B, int D, const int* t_dev, const int* pos_off, tw_stream_t stream);
/* tw_kv_head_major: the cross-attention K/V as the KV projection writes it (rows b*Tk + t of [B*Tk][ld], k at
 * columns 0..64H, v at 64H..128H) -> dst = K [B][H][Tk][64] followed by V [B][H][Tk][64], so tw_decode_attn reads
 * each (clip, head) as two contiguous runs (called as B*H one-head clips: ldk = 64, skb = Tk*64).  Replaces the
 * layout of HF's cross-attention past_key_values ([B][H][Tk][64], modeling_whisper.py WhisperAttention).  dtype bf16
 * or f32; ld a multiple of 16 B. */
int tw_kv_head_major(const void* src, int64_t ld, void* dst, int B, int Tk, int H, int dtype, tw_stream_t stream);
int tw_kv_append(const void* src, int64_t ld_src, void* cache, int64_t ld_row, int64_t sb, int B, int n, int dtype,
                 const int* t_dev, tw_stream_t stream);
int tw_step_advance(int* t_dev, int by, tw_stream_t stream);

/* ---- 8-bit cross-attention K/V cache (model.cross_kv_dtype = "fp8_e4m3"; csrc/xkv_fp8.hip).  Opt-in: the
 * cross-attention K/V is written once per 30 s window and read once per generated token, and that read bounds
 * batched decoding; as bytes it is half as large and half as long to read.
 * FORMAT.  Elements are OCP e4m3fn bytes (torch.float8_e4m3fn), rounded to nearest even.  Layout per decoder layer:
 * K [B][H][Tk][64] bytes, then V, as tw_kv_head_major lays out 16-bit elements.  One fp32 scale per (clip, head)
 * block of K and one of V: 2*B*H floats, the K scales then the V scales, block (b, h) at index b*H + h.  A scale is
 * 2^e, e the smallest integer with absmax * 2^-e <= 448, absmax over the block's Tk x 64 16-bit values (absmax =
 * m * 2^x, m in [0.5, 1): e = x - 9 when m <= 0.875, else x - 8), e clamped to [-100, 100]; absmax == 0 gives 1; a
 * block holding an inf or NaN gets a NaN scale, so every output that reads it is NaN.  An element is
 * RNE_e4m3(x * 2^-e): the product is exact and at most 448 in magnitude (absmax above 448 * 2^100, which the clamp
 * would let past the format's range, is outside any 16-bit activation this engine produces).  Dequantisation
 * (byte * 2^e) is exact: the value is a bf16 value, and an fp16 value wherever it is in fp16's normal range.
 * tw_kv_head_major_fp8: tw_kv_head_major's source -> the bytes (dst, 2*B*H*Tk*64 of them) and the scales.  One
 * workgroup per block, two passes (absmax, quantise).  dtype bf16 or fp16 (fp32: 2); a null pointer, ld not a
 * multiple of 16 B or below 128*H, or a misaligned pointer: 1.
 * tw_decode_attn_fp8: tw_decode_attn_ks (k_start may be NULL: every start 0) over such a cache.  k / v point at
 * bytes and ldk, skb, hsk, ldv, svb, hsv count bytes; block (b, h) is scaled by k_scale[b*ssb + h] and
 * v_scale[b*ssb + h] (ssb = 0 together with skb = svb = 0: one clip's blocks and scales for every row).  q and o are
 * `dtype` (bf16 or fp16; fp32: 2).  K and V are converted to fp32 exactly and accumulated as in the 16-bit kernels;
 * the K scale is folded into the score scale and the V scale applied once to the reduced output -- both exact, the
 * scales being powers of two -- so the result is the fp32 arithmetic of tw_decode_attn_ks over the dequantised
 * cache, in a different summation order only where the 16-bit call would take another kernel variant.  Only a
 * fixed Tk: tk_dev != NULL returns 2 (the self-attention cache stays 16-bit).  A null scale pointer returns 1.  The
 * variants and the split rule are tw_decode_attn_ks's; bytes below a row's start or at / past Tk are never loaded.
 * tw_decode_attn_mq_fp8: tw_decode_attn_mq over such a cache, with the same additions and restrictions. */
int tw_kv_head_major_fp8(const void* src, int64_t ld, void* dst, float* scales, int B, int Tk, int H, int dtype,
                         tw_stream_t stream);
int tw_decode_attn_fp8(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, int64_t hsk,
                       const void* v, int64_t ldv, int64_t svb, int64_t hsv, const float* k_scale,
                       const float* v_scale, int64_t ssb, void* o, int64_t sob, int B, int H, int Tk,
                       const int* tk_dev, const int* k_start, int head_dim, float scale, int dtype,
                       tw_stream_t stream);
int tw_decode_attn_mq_fp8(const void* q, int64_t sqb, int64_t sqq, const void* k, int64_t ldk, int64_t skb,
                          int64_t hsk, const void* v, int64_t ldv, int64_t svb, int64_t hsv, const float* k_scale,
                          const float* v_scale, int64_t ssb, void* o, int64_t sob, int64_t soq, int B, int H, int Q,
                          int Tk, const int* tk_dev, const int* k_start, int causal, int head_dim, float scale,
                          int dtype, tw_stream_t stream);

/* ---- 8-bit decoder weights for the batch <= 8 decode step (model.decode_weight_dtype = "fp8_e4m3";
 * csrc/gemv_w8.hip).  Opt-in: at batch <= 8 every Linear of a decode step is one GEMV launch that streams its weight
 * matrix once per generated token; as bytes the matrix is half as large.
 * FORMAT.  A weight matrix W [N][K] (16-bit, row-major, one output column per row) is kept as N*K OCP e4m3fn bytes
 * (torch.float8_e4m3fn), rounded to nearest even, row n at byte n*ld, plus one fp32 scale per row: N floats.  The
 * scale rule is the K/V format's above with "block" = one row of K values: a scale is 2^e, e the smallest integer
 * with absmax(row) * 2^-e <= 448 (absmax = m * 2^x, m in [0.5, 1): e = x - 9 when m <= 0.875, else x - 8), e
 * clamped to [-100, 100]; an all-zero row gets 1; a row holding an inf or NaN gets a NaN scale, so exactly that
 * output column is NaN.  A byte is RNE_e4m3(x * 2^-e): the product is exact and at most 448 in magnitude.
 * Dequantisation (byte * 2^e) is exact: the value has at most 4 significant bits, so it is a bf16 value, and it is
 * an fp16 value wherever it is a multiple of 2^-24 (fp16's smallest subnormal: a byte stands for a multiple of
 * 2^(e-9), so only rows with e < -15, absmax below 2^-6, can leave that grid) and at most 65504 in magnitude (an fp16
 * row whose absmax is 63488 = 248 * 2^8 or more rounds it up to 256 * 2^8 = 65536).  Whisper weights are inside both limits.
 * tw_quant_rows_fp8: rows src [N][ld] of `dtype` (bf16 or fp16; fp32: 2) -> bytes dst_bytes [N][ld_dst] and
 * scales [N].  One wave per row, two passes (absmax, quantise).  A null pointer, a pointer not 16-B aligned (scales:
 * 4-B), K % 16 != 0, ld or ld_dst below K or not a multiple of 16 B: 1.
 * tw_gemv_w8_bf16 / tw_gemv_w8_f16: tw_gemv_bf16 / tw_gemv_f16 over such a matrix, their contract in full (M <= 8
 * rows, optional fused LayerNorm with A bit-identical to tw_layernorm_fwd's output, the bias / round / GELU (+ aux
 * out) / residual / accumulate epilogues, fp32 or 16-bit C, the fused self-attention KV append) with these
 * differences: W points at bytes, ldw counts bytes and is a multiple of 16, K % 16 == 0, and w_scale holds the N row
 * scales (a null w_scale returns 1).  The bytes are converted to fp32 exactly and accumulated in fp32 (16 bytes = 16 k per lane per
 * load, lane l holding k = 16 l + 1024 u); the row's scale multiplies the reduced sum once, before the epilogue --
 * exact, a power of two -- so the result is the fp32 arithmetic of a GEMV over the dequantised matrix, in another
 * summation order than tw_gemv_bf16's.  Row m of an M-row call is bit-identical to that row computed with M = 1, and
 * the LN-fused call to tw_layernorm_fwd followed by the plain call. */
int tw_quant_rows_fp8(const void* src, int64_t ld, int dtype, int N, int K, void* dst_bytes, int64_t ld_dst,
                      float* scales, tw_stream_t stream);
int tw_gemv_w8_bf16(const void* x, int64_t ldx, const float* ln_w, const float* ln_b, float eps, const void* W,
                    int64_t ldw, const float* w_scale, void* C, int64_t ldc, int c_dtype, int M, int N, int K,
                    const void* bias, const void* res, int64_t ldr, int res_dtype, void* aux, int64_t ldaux, int flags,
                    void* kv_cache, int64_t kv_sb, int64_t kv_ld, int kv_col0, const int* t_dev, tw_stream_t stream);
int tw_gemv_w8_f16(const void* x, int64_t ldx, const float* ln_w, const float* ln_b, float eps, const void* W,
                   int64_t ldw, const float* w_scale, void* C, int64_t ldc, int c_dtype, int M, int N, int K,
                   const void* bias, const void* res, int64_t ldr, int res_dtype, void* aux, int64_t ldaux, int flags,
                   void* kv_cache, int64_t kv_sb, int64_t kv_ld, int kv_col0, const int* t_dev, tw_stream_t stream);

/* ---- fp32 arithmetic path (mixed_precision = "no", run_distillation.py:815-823: the reference's default
 * --dtype float32; the fp32 greedy decode pinned token-for-token to HF fp32 generate).  Exact-fp32 MFMA
 * (v_mfma_f32_16x16x4_f32), nothing rounded to bf16.
 * tw_gemm_f32: C[b] = epi(alpha * op(A[b]) op(B[b])^T) with the tw_gemm_bf16 operand conventions
 *   (A [M][K], a_trans: [K][M]; B [N][K], b_trans: [K][N]) and flags BIAS / GELU (+AUX_OUT) / DGELU / RES /
 *   ACCUM (ROUND and the tile flags are ignored); bias / res / aux fp32; two batch levels: batch entries
 *   bz = bo * batch_inner + bi at offsets bo*s? + bi*s?_in.  lda, ldb % 4 == 0, A and B 16-B aligned.
 * tw_attn_fwd_f32 / tw_attn_bwd_f32: SDPA over (B, H) with head_dim 64 and the tw_attn_* layouts, composed
 *   from tw_gemm_f32 products and exact row softmax kernels over a caller workspace (fwd >= Tq*round4(Tk)
 *   floats, bwd twice that; larger workspaces take more (b, h) pairs per pass).  lse [B][H][Tq] (natural log).
 * tw_mel_to_conv_input_f32 / tw_im2col3_f32 / tw_gelu_bwd_f32: the conv-stem helpers in fp32. */
int tw_gemm_f32(const float* A, int64_t lda, int a_trans, const float* B, int64_t ldb, int b_trans, float* C,
                int64_t ldc, int M, int N, int K, int batch, int64_t sA, int64_t sB, int64_t sC, int batch_inner,
                int64_t sA_in, int64_t sB_in, int64_t sC_in, float alpha, const float* bias, const float* res,
                int64_t ldr, int64_t sR, int res_mod, float* aux, int64_t ldaux, int64_t sAux, int flags,
                tw_stream_t stream);
int tw_attn_fwd_f32(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv, float* O,
                    int64_t ldo, float* lse, int B, int H, int Tq, int Tk, int head_dim, int causal, float scale,
                    float* workspace, int64_t workspace_floats, tw_stream_t stream);
int tw_attn_bwd_f32(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv,
                    const float* O, int64_t ldo, const float* dO, int64_t lddo, const float* lse, float* dQ,
                    int64_t lddq, float* dK, int64_t lddk, float* dV, int64_t lddv, int B, int H, int Tq, int Tk,
                    int head_dim, int causal, float scale, float* workspace, int64_t workspace_floats,
                    tw_stream_t stream);
int tw_mel_to_conv_input_f32(const float* mel, float* xt, int B, int nmel, int T, tw_stream_t stream);
int tw_im2col3_f32(const float* src, int64_t src_rows, float* dst, int B, int T_out, int stride, int C,
                   tw_stream_t stream);
int tw_gelu_bwd_f32(const float* g, const float* pre, float* out, int64_t n, tw_stream_t stream);

/* ---- fp16 arithmetic path: a torch_dtype=float16 model without autocast, the arithmetic of the reference's fp16
 * decode call sites (training/run_eval.py:99 `--dtype float16` default, :500-509 `model.to(dtype)`, :589
 * `input_features.to(dtype)`; training/run_pseudo_labelling.py:461-463 under run-pseudo-labelling.sh:30):
 * v_mfma_f32_16x16x32_f16 with fp32 accumulation, every 16-bit operand / output IEEE fp16 (RNE).
 * tw_gemm_f16: tw_gemm_bf16 for fp16 operands (the decode path uses the forward products only);
 *   A, B, bias, aux fp16; C and res fp16 (code 2) or fp32; epilogue order as tw_gemm_bf16 with the rounding
 *   to fp16, plus TW_GEMM_CLAMP16: after the residual add and the ACCUM add (the last step before the store), the
 *   value is rounded to fp16 and clamped to +-(65504 - 1000), so an overflow to +-inf lands on the bound too (HF
 *   WhisperEncoderLayer, modeling_whisper.py:409-411, the fp16 encoder stream).  RES, ACCUM and CLAMP16 combine
 *   with each other, and RES or ACCUM with DGELU, in that order on whole and on ragged tiles alike
 *   (tests/test_gemm_parity_gpu.py; GELU followed by RES / ACCUM and DGELU with CLAMP16 are not under test).
 * tw_gemv_f16: tw_gemv_bf16 for fp16 x / W / bias / C (LayerNorm fused as there, fp16 output of the LN).
 * tw_attn_fwd_f16: tw_attn_fwd for fp16 Q/K/V/O (P rounded to fp16 for the PV product, fp32 row sums).
 * tw_mel_to_conv_input_f16: log-mel [B][80][T] fp32 -> fp16 conv1 input [B][T+2][80] (the .to(float16) cast).
 * fp16-AUTOCAST TRAINING (run_distillation.py:815-817 --dtype float16: mixed_precision="fp16", fp16 teacher,
 * GradScaler; round 6) uses the same entries plus:
 *   tw_gemm_f16 with a_trans / b_trans (the dX and dW products; split-K dW rounds its fp32 chunk sum to fp16);
 *   tw_attn_bwd_f16: tw_attn_bwd for fp16 tensors; tw_gelu_bwd_f16: tw_gelu_bwd for an fp16 activation;
 *   tw_cast_f32_f16: autocast's fp32 -> fp16 weight cast; tw_colsum with round_bf16 = 2;
 *   tw_adamw_ex: tw_adamw with the 16-bit weight copy in p16_dtype (1 bf16, 2 fp16) and GradScaler.unscale_
 *   folded in: g and norm are the loss-scaled gradient and its norm, inv_scale = 1 / scale (a power of two,
 *   so g * inv_scale is exact); tw_adamw(...) == tw_adamw_ex(..., TW bf16, ..., inv_scale = 1).
 * The dtype-coded entries above (tw_layernorm_fwd, tw_embed_fwd / tw_embed_step, tw_decode_attn, the selection
 * kernels, tw_token_logprob, tw_kv_append, tw_kv_head_major, tw_kl_ce) take code 2 for fp16 rows. */
#define TW_GEMM_CLAMP16 128
int tw_gemm_f16(const void* A, int64_t lda, int a_trans, const void* B, int64_t ldb, int b_trans, void* C,
                int64_t ldc, int c_dtype, int M, int N, int K, int batch, int64_t sA, int64_t sB, int64_t sC,
                float alpha, const void* bias, const void* res, int64_t ldr, int64_t sR, int res_dtype, int res_mod,
                void* aux, int64_t ldaux, int64_t sAux, int flags, tw_stream_t stream);
int tw_gemv_f16(const void* x, int64_t ldx, const float* ln_w, const float* ln_b, float eps, const void* W,
                int64_t ldw, void* C, int64_t ldc, int c_dtype, int M, int N, int K, const void* bias,
                const void* res, int64_t ldr, int res_dtype, void* aux, int64_t ldaux, int flags,
                void* kv_cache, int64_t kv_sb, int64_t kv_ld, int kv_col0, const int* t_dev, tw_stream_t stream);
int tw_attn_fwd_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                    int64_t ldo, float* lse, int B, int H, int Tq, int Tk, int head_dim, int causal, float scale,
                    tw_stream_t stream);
int tw_mel_to_conv_input_f16(const float* mel, void* xt, int B, int nmel, int T, tw_stream_t stream);
int tw_attn_bwd_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const void* O,
                    int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ, int64_t lddq, void* dK,
                    int64_t lddk, void* dV, int64_t lddv, int B, int H, int Tq, int Tk, int head_dim, int causal,
                    float scale, float* workspace, tw_stream_t stream);
int tw_gelu_bwd_f16(const void* g, int g_dtype, const void* pre, void* out, int64_t n, tw_stream_t stream);
int tw_cast_f32_f16(const float* src, void* dst, int64_t n, tw_stream_t stream);
/* tw_add_layernorm_fwd_f16: tw_add_layernorm_fwd on the fp32 stream of fp16 autocast: r and y fp16 (x fp32 only) */
int tw_add_layernorm_fwd_f16(const void* x, int x_dtype, const void* r, void* x_out, const float* w, const float* b,
                             void* y, float* mean_out, float* rstd_out, int rows, int D, float eps, tw_stream_t stream);
int tw_adamw_ex(float* p, const float* g, float* m, float* v, void* p16, int p16_dtype, int64_t n, float lr, float b1,
                float b2, float eps, float wd, int step, const float* norm, float max_norm, float inv_scale,
                tw_stream_t stream);

/* ---- host code: FLAC decoding for the data feed (replaces soundfile / libsndfile's sf.read of the
 * reference corpus, dataset/cool_dataset.py:55).  `data` is the whole file in host memory.
 * tw_flac_info: info[4] = {channels, sample_rate, bits_per_sample, total samples per channel (0 = unknown)}.
 * tw_flac_decode: interleaved int32 samples into out[cap] (out == NULL: count only), *frames = samples per
 * channel; every frame's CRC-8 header and CRC-16 footer is checked (1 = malformed stream). */
int tw_flac_info(const uint8_t* data, int64_t n, int64_t* info);
int tw_flac_decode(const uint8_t* data, int64_t n, int32_t* out, int64_t cap, int64_t* frames);

#ifdef __cplusplus
}
#endif
#endif /* TW_HIP_H */
