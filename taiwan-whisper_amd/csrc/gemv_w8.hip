// 8-bit decoder weights for the batch <= 8 decode step (model.decode_weight_dtype = "fp8_e4m3").
//
// At batch <= 8 every Linear of a decode step is one GEMV launch that streams its weight matrix once per generated
// token (gemv_impl.h).  Here a weight matrix W [N][K] is kept as N*K OCP e4m3fn bytes plus one fp32 power-of-two
// scale per row (the format: include/tw_hip.h):
//
//  * tw_quant_rows_fp8: 16-bit rows -> bytes and scales.  One wave per row, two passes: absmax over the row's K values
//    (on the bit patterns), then x * 2^-e rounded to nearest even by the hardware conversion -- the rule, helpers and
//    special cases of the cross-attention K/V quantiser (xkv_fp8.hip), with "block" = one row.
//  * tw_gemv_w8_bf16 / tw_gemv_w8_f16: tw_gemv_bf16 / tw_gemv_f16 (gemm.hip gemv_kernel) over such a matrix.  The A
//    rows are staged exactly as there (gemv_stage_rows: as given, or through the fused LayerNorm), each wave streams
//    its W rows 16 bytes = 16 k per lane per load (non-temporal; lane l holds k = 16 l + 1024 u, u = 0, 1, ...),
//    v_cvt_pk_f32_fp8 widens the bytes exactly, fp32 FMAs in k order per lane, the butterfly of the 16-bit kernel
//    (wave_reduce_scatter), then the row's scale multiplies the reduced sum once -- a power of two commutes with every
//    fp32 rounding, so the result is the fp32 arithmetic of a GEMV over the dequantised matrix -- and epi_value runs
//    the 16-bit kernel's epilogue.  The per-output arithmetic does not depend on the row count or on the columns per
//    wave, so row m of an M-row call is bit-identical to that row computed alone, and the LN-fused call to the LN
//    kernel followed by the plain call.
#include "common.h"
#include "fp8_common.h"
#include "gemv_impl.h"

namespace {

using namespace twg;
using namespace tw8;

// ------------------------------------------------------------------------------------------------ quantiser
// one wave per row, 4 rows per workgroup; lane l takes the 16 values at k = 16 l + 1024 u
template <bool H>
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const bf16* __restrict__ src, int64_t ld,
                                                             uint8_t* __restrict__ dst, int64_t ld_dst,
                                                             float* __restrict__ scales, int N, int K) {
  const int lane = lane_id();
  const int n = blockIdx.x * 4 + wave_id_uniform();
  if (n >= N) return;
  const bf16* in = src + (int64_t)n * ld;
  uint8_t* out = dst + (int64_t)n * ld_dst;
  // pass 1: the largest magnitude, on the bit patterns (sign cleared, a 16-bit float orders as its bits; an inf or
  // NaN pattern is above every finite one)
  uint32_t mx = 0u;
  for (int k = lane * 16; k < K; k += 1024) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const s16x8 v = __builtin_bit_cast(s16x8, *(const bf16x8*)(in + k + h * 8));
#pragma unroll
      for (int j = 0; j < 8; ++j) mx = max(mx, (uint32_t)(uint16_t)v[j] & 0x7fffu);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
  const bool finite = mx < (H ? 0x7c00u : 0x7f80u);
  float scale = 1.f, inv = 1.f;
  if (!finite) {
    scale = inv = __uint_as_float(0x7fc00000u);
  } else if (mx != 0u) {
    const int e = scale_exp(__float_as_uint(e2f<H>(__builtin_bit_cast(bf16, (uint16_t)mx))));
    scale = __uint_as_float((uint32_t)(e + 127) << 23);
    inv = __uint_as_float((uint32_t)(127 - e) << 23);
  }
  if (lane == 0) scales[n] = scale;
  // pass 2 (the row was just read: L2 hits): 16 values -> 16 bytes, one 16-B store
  for (int k = lane * 16; k < K; k += 1024) {
    float f[16];
    words_f32<H>(*(const bf16x8*)(in + k), f);
    words_f32<H>(*(const bf16x8*)(in + k + 8), f + 8);
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] *= inv;
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = cvt4_e4m3(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]);
    *(u32x4*)(out + k) = w;
  }
}

// ------------------------------------------------------------------------------------------------ GEMV
// one 16-B piece of a weight row (16 e4m3 bytes), a non-temporal load as ldw8's: each weight is read once per step
__device__ __forceinline__ u32x4 ldw16(const uint8_t* q) { return __builtin_nontemporal_load((const u32x4*)q); }

// the pieces lane `lane` holds of a K-byte row: k = 16 lane + 1024 u < K
__device__ __forceinline__ int w8_pieces(int K, int lane) { return (K - lane * 16 + 1023) / 1024; }

// 16 e4m3 bytes -> fp32, exact (v_cvt_pk_f32_fp8: two bytes of a dword at a time)
__device__ __forceinline__ void w8_widen(const u32x4 w, float (&o)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
    o[4 * j] = lo[0]; o[4 * j + 1] = lo[1]; o[4 * j + 2] = hi[0]; o[4 * j + 3] = hi[1];
  }
}

// acc = fma(w[q], a[q], acc) for q = 0..15 in order, the 16-bit a widened exactly.  fp16: v_fma_mix_f32 with an fp32
// first operand and the fp16 half of the second widened inside the FMA (fma8's reason: no v_cvt_f32_f16 per element)
template <bool H>
__device__ __forceinline__ void w8_fma16(float& acc, const float (&w)[16], const bf16x8& a0, const bf16x8& a1) {
  if constexpr (H) {
    const gv_u32x4 u0 = __builtin_bit_cast(gv_u32x4, a0), u1 = __builtin_bit_cast(gv_u32x4, a1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t au = i < 4 ? u0[i] : u1[i - 4];
      asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[0,1,0]" : "+v"(acc) : "v"(w[2 * i]), "v"(au));
      asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(acc) : "v"(w[2 * i + 1]), "v"(au));
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) acc = fmaf(w[q], e2f<H>(a0[q]), acc);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc = fmaf(w[8 + q], e2f<H>(a1[q]), acc);
  }
}

// the first PRE pieces per lane of W rows n0 .. n0 + CPW - 1 (rows past N read row 0, never stored)
template <int CPW, int PRE>
__device__ __forceinline__ void w8_preload(const uint8_t* W, int64_t ldw, int N, int K, int n0, int lane,
                                           u32x4 (&wpre)[CPW][PRE]) {
  const int npre = min(PRE, w8_pieces(K, lane));
#pragma unroll
  for (int c = 0; c < CPW; ++c) {
    const int n = n0 + c;
    const uint8_t* wr = W + (int64_t)(n < N ? n : 0) * ldw;
#pragma unroll
    for (int u = 0; u < PRE; ++u) wpre[c][u] = (u < npre) ? ldw16(wr + lane * 16 + u * 1024) : u32x4{};
  }
}

// one piece of one column against the MR staged rows
template <bool H, int MR>
__device__ __forceinline__ void w8_piece(float (&acc)[MR], const u32x4 w, const bf16* xs, int K, int k0) {
  float wf[16];
  w8_widen(w, wf);
#pragma unroll
  for (int r = 0; r < MR; ++r) {
    const bf16* a = xs + (int64_t)r * K + k0;
    w8_fma16<H>(acc[r], wf, *(const bf16x8*)a, *(const bf16x8*)(a + 8));
  }
}

// columns n0 .. n0 + CPW - 1 against the staged rows, then gemv_finish's reduction and epilogue with the row scale
template <bool H, int MR, int CPW, int PRE>
__device__ __forceinline__ void w8_finish(const GemmP& p, const uint8_t* W, const float* __restrict__ w_scale,
                                          const GemvKV& kv, const bf16* xs, int n0, int lane,
                                          const u32x4 (&wpre)[CPW][PRE]) {
  const int K = p.K;
  const int npre = min(PRE, w8_pieces(K, lane));
  float acc[CPW][MR];
#pragma unroll
  for (int c = 0; c < CPW; ++c)
#pragma unroll
    for (int r = 0; r < MR; ++r) acc[c][r] = 0.f;
  // k order per lane: pieces u = 0, 1, ... at k = lane*16 + 1024u (the preloaded ones first, the rest streamed)
#pragma unroll
  for (int u = 0; u < PRE; ++u) {
    if (u < npre) {
#pragma unroll
      for (int c = 0; c < CPW; ++c) w8_piece<H, MR>(acc[c], wpre[c][u], xs, K, lane * 16 + u * 1024);
    }
  }
  for (int k0 = lane * 16 + PRE * 1024; k0 < K; k0 += 1024) {
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
      const int n = n0 + c;
      w8_piece<H, MR>(acc[c], ldw16(W + (int64_t)(n < p.N ? n : 0) * p.ldb + k0), xs, K, k0);
    }
  }
  static_assert(CPW * MR <= 64, "one output per lane");
  float vals[CPW * MR];
#pragma unroll
  for (int c = 0; c < CPW; ++c)
#pragma unroll
    for (int r = 0; r < MR; ++r) vals[c * MR + r] = acc[c][r];
  int idx;
  const float mine = wave_reduce_scatter<CPW * MR>(vals, lane, idx);
  const int c = idx / MR, r = idx % MR;
  const int n = n0 + c;
  if (idx >= 0 && r < p.M && n < p.N) {
    // the row's scale once on the reduced sum (a power of two: exact), then the 16-bit kernel's epilogue and stores
    const float v = epi_value<H>(p, r, n, mine * w_scale[n]);
    const int64_t co = (int64_t)r * p.ldc + n;
    if (p.c_dtype == TW_BF16) ((bf16*)p.C)[co] = f2e<H>(v);
    else ((float*)p.C)[co] = v;
    if (kv.cache && n >= kv.col0) {
      const int64_t t = (int64_t)*kv.t;
      const int64_t ko = r * kv.sb + t * kv.ld + (n - kv.col0);
      if (p.c_dtype == TW_BF16) ((bf16*)kv.cache)[ko] = f2e<H>(v);
      else ((float*)kv.cache)[ko] = v;
    }
  }
}

// gemv_kernel's frame (gemm.hip): LN parameters to LDS by LDS-DMA, weight preload, row staging, dots.  p.B is unused:
// W holds the bytes, p.ldb their row stride
template <bool H, int MR, int CPW, int PRE>
__global__ __launch_bounds__(256) void gemv_w8_kernel(GemmP p, const uint8_t* __restrict__ W,
                                                      const float* __restrict__ w_scale,
                                                      const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                      float eps, GemvKV kv) {
  extern __shared__ __attribute__((aligned(16))) char gemv_w8_smem[];
  bf16* xs = (bf16*)gemv_w8_smem;                      // [MR][K] 16-bit
  const int lane = lane_id(), wave = wave_id_uniform();
  const int n0 = (blockIdx.x * 4 + wave) * CPW;
  float* lnp = nullptr;
  if (lnw && p.K <= 1280) {
    lnp = (float*)(gemv_w8_smem + (size_t)MR * p.K * 2);
    const int per = p.K / 256;                         // 64-lane x 16-B pieces per array
    for (int i = wave; i < 2 * per; i += 4) {
      const float* src = i < per ? lnw : lnb;
      const int pc = (i % per) * 64;
      buf_load_lds16(make_rsrc(src), lnp + (i < per ? 0 : p.K) + pc * 4, (uint32_t)(pc + lane) * 16);
    }
  }
  u32x4 wpre[CPW][PRE];
  w8_preload<CPW, PRE>(W, p.ldb, p.N, p.K, n0, lane, wpre);
  gemv_stage_rows<H, MR>(p, lnw, lnb, eps, xs, wave, 4, lane, lnp);
  __syncthreads();
  if (n0 >= p.N) return;
  w8_finish<H, MR, CPW, PRE>(p, W, w_scale, kv, xs, n0, lane, wpre);
}

template <bool H>
int gemv_w8_run(const void* x, int64_t ldx, const float* ln_w, const float* ln_b, float eps, const void* W,
                int64_t ldw, const float* w_scale, void* C, int64_t ldc, int c_dtype, int M, int N, int K,
                const void* bias, const void* res, int64_t ldr, int res_dtype, void* aux, int64_t ldaux, int flags,
                void* kv_cache, int64_t kv_sb, int64_t kv_ld, int kv_col0, const int* t_dev, hipStream_t stream) {
  if (M <= 0 || N <= 0) return TW_OK;
  if (H) {
    if ((c_dtype != TW_F32 && c_dtype != TW_F16) || ((flags & F_RES) && res_dtype != TW_F32 && res_dtype != TW_F16))
      return TW_EUNSUPPORTED;
    if (c_dtype == TW_F16) c_dtype = TW_BF16;
    if (res_dtype == TW_F16) res_dtype = TW_BF16;
  } else if (flags & F_CLAMP16) {
    return TW_EINVAL;
  }
  if (M > 8 || K <= 0 || (K % 16) || (ldx % 8) || (ldw % 16) || ldw < K) return TW_EINVAL;
  if (!x || !W || !w_scale || !C) return TW_EINVAL;
  if (((uintptr_t)x & 15) || ((uintptr_t)W & 15) || ((uintptr_t)w_scale & 3)) return TW_EINVAL;
  if (ln_w && (!ln_b || (K % 256) || (((uintptr_t)ln_w | (uintptr_t)ln_b) & 15))) return TW_EINVAL;
  if ((flags & F_BIAS) && !bias) return TW_EINVAL;
  if ((flags & F_RES) && !res) return TW_EINVAL;
  if ((flags & (F_AUX_OUT | F_DGELU)) && !aux) return TW_EINVAL;
  if (c_dtype != TW_F32 && c_dtype != TW_BF16) return TW_EUNSUPPORTED;
  const int mr = M == 1 ? 1 : M == 2 ? 2 : M <= 4 ? 4 : 8;
  if ((size_t)mr * K * 2 > 80 * 1024) return TW_EUNSUPPORTED;        // A rows in LDS
  if (kv_cache && (!t_dev || kv_col0 < 0 || kv_col0 >= N)) return TW_EINVAL;
  const GemvKV kv{kv_cache, kv_sb, kv_ld, kv_col0, t_dev};
  GemmP p = {};
  p.A = (const bf16*)x; p.B = nullptr; p.C = C;
  p.lda = ldx; p.ldb = ldw; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  p.alpha = 1.f; p.bias = (const bf16*)bias;
  p.res = res; p.ldr = ldr; p.res_dtype = res_dtype; p.res_mod = 0;
  p.aux = (bf16*)aux; p.ldaux = ldaux; p.c_dtype = c_dtype; p.flags = flags;
  // columns per wave: the 16-bit kernel's rule (gemm.hip gemv_run).  Preloaded pieces per lane: 2 cover K = 2048
  // (every K = d_model Linear), 5 cover K = 5120 (fc2); longer rows stream the rest
  const int cpw = N >= 16384 ? (mr == 8 || mr == 1 ? 4 : 8) : (mr >= 4 && N >= 3072 && K <= 1536) ? 2 : 1;
  const dim3 grid((N + 4 * cpw - 1) / (4 * cpw));
  const size_t lds = (size_t)mr * K * 2 + (ln_w && K <= 1280 ? (size_t)2 * K * 4 : 0);
  const uint8_t* Wb = (const uint8_t*)W;
#define TW_GEMV_W8(MR_, CPW_, PRE_)                                                                            \
  hipLaunchKernelGGL((gemv_w8_kernel<H, MR_, CPW_, PRE_>), grid, dim3(256), lds, stream, p, Wb, w_scale, ln_w, \
                     ln_b, eps, kv)
  if (cpw == 8) {
    if (mr == 2) TW_GEMV_W8(2, 8, 2);
    else TW_GEMV_W8(4, 8, 2);
  } else if (cpw == 4) {
    if (mr == 1) TW_GEMV_W8(1, 4, 2);
    else TW_GEMV_W8(8, 4, 2);
  } else if (cpw == 2) {
    if (mr == 4) TW_GEMV_W8(4, 2, 2);
    else TW_GEMV_W8(8, 2, 2);
  } else if (K <= 2048) {
    if (mr == 1) TW_GEMV_W8(1, 1, 2);
    else if (mr == 2) TW_GEMV_W8(2, 1, 2);
    else if (mr == 4) TW_GEMV_W8(4, 1, 2);
    else TW_GEMV_W8(8, 1, 2);
  } else {
    if (mr == 1) TW_GEMV_W8(1, 1, 5);
    else if (mr == 2) TW_GEMV_W8(2, 1, 5);
    else if (mr == 4) TW_GEMV_W8(4, 1, 5);
    else TW_GEMV_W8(8, 1, 5);
  }
#undef TW_GEMV_W8
  TW_CHECK_LAUNCH();
  return TW_OK;
}

}  // namespace

extern "C" int tw_quant_rows_fp8(const void* src, int64_t ld, int dtype, int N, int K, void* dst_bytes,
                                 int64_t ld_dst, float* scales, hipStream_t stream) {
  if (dtype != TW_BF16 && dtype != TW_F16) return TW_EUNSUPPORTED;
  if (!src || !dst_bytes || !scales) return TW_EINVAL;
  if (N < 0 || K < 0 || (K % 16) || (ld % 8) || (ld_dst % 16) || ld < K || ld_dst < K) return TW_EINVAL;
  if ((((uintptr_t)src | (uintptr_t)dst_bytes) & 15) || ((uintptr_t)scales & 3)) return TW_EINVAL;
  if (N == 0 || K == 0) return TW_OK;
  const dim3 grid((unsigned)((N + 3) / 4));
  if (dtype == TW_F16)
    hipLaunchKernelGGL(quant_rows_fp8_kernel<true>, grid, dim3(256), 0, stream, (const bf16*)src, ld,
                       (uint8_t*)dst_bytes, ld_dst, scales, N, K);
  else
    hipLaunchKernelGGL(quant_rows_fp8_kernel<false>, grid, dim3(256), 0, stream, (const bf16*)src, ld,
                       (uint8_t*)dst_bytes, ld_dst, scales, N, K);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_gemv_w8_bf16(const void* x, int64_t ldx, const float* ln_w, const float* ln_b, float eps,
                               const void* W, int64_t ldw, const float* w_scale, void* C, int64_t ldc, int c_dtype,
                               int M, int N, int K, const void* bias, const void* res, int64_t ldr, int res_dtype,
                               void* aux, int64_t ldaux, int flags, void* kv_cache, int64_t kv_sb, int64_t kv_ld,
                               int kv_col0, const int* t_dev, hipStream_t stream) {
  return gemv_w8_run<false>(x, ldx, ln_w, ln_b, eps, W, ldw, w_scale, C, ldc, c_dtype, M, N, K, bias, res, ldr,
                            res_dtype, aux, ldaux, flags, kv_cache, kv_sb, kv_ld, kv_col0, t_dev, stream);
}

extern "C" int tw_gemv_w8_f16(const void* x, int64_t ldx, const float* ln_w, const float* ln_b, float eps,
                              const void* W, int64_t ldw, const float* w_scale, void* C, int64_t ldc, int c_dtype,
                              int M, int N, int K, const void* bias, const void* res, int64_t ldr, int res_dtype,
                              void* aux, int64_t ldaux, int flags, void* kv_cache, int64_t kv_sb, int64_t kv_ld,
                              int kv_col0, const int* t_dev, hipStream_t stream) {
  return gemv_w8_run<true>(x, ldx, ln_w, ln_b, eps, W, ldw, w_scale, C, ldc, c_dtype, M, N, K, bias, res, ldr,
                           res_dtype, aux, ldaux, flags, kv_cache, kv_sb, kv_ld, kv_col0, t_dev, stream);
}
