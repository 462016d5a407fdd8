// 8-bit cross-attention K/V cache (model.cross_kv_dtype = "fp8_e4m3").
//
// The cross-attention K/V of a decode is written once per 30 s window and read once per generated token, and that
// read bounds batched decoding ("c4 batch size").  Here it is kept as OCP e4m3fn bytes with one fp32
// power-of-two scale per (clip, head) block of K and of V:
//
//  * tw_kv_head_major_fp8: the row-interleaved 16-bit projection [B*Tk][ld] -> head-major bytes K [B][H][Tk][64]
//    then V (tw_kv_head_major's layout) and 2*B*H scales (K scales, then V scales).  One workgroup per block, two
//    passes: absmax over the block's Tk x 64 values, then x * 2^-e rounded to nearest even.  scale = 2^e, e the
//    smallest integer with absmax * 2^-e <= 448 (the largest e4m3 value), clamped to [-100, 100]; an all-zero block
//    has scale 1, a block with a non-finite value a NaN scale.  The product is exact and within the format's range,
//    so a byte dequantises (byte * 2^e) to a 16-bit value exactly wherever that value is normal.
//  * tw_decode_attn_fp8 / tw_decode_attn_mq_fp8: tw_decode_attn_ks / tw_decode_attn_mq over such a cache (fixed Tk
//    only): the bodies of decode_impl.h with K / V read as 8 e4m3 bytes per lane and converted by v_cvt_pk_f32_fp8;
//    the K scale is folded into the score scale and the V scale applied once to the reduced output -- powers of two
//    commute with every fp32 rounding, so the result is the fp32 arithmetic over the dequantised cache.  Variants and
//    the split rule are those of decode.hip.
#include "common.h"
#include "decode_impl.h"
#include "fp8_common.h"

#include <algorithm>

namespace {

using namespace twd;
using namespace tw8;   // cvt4_e4m3 / words_f32 / scale_exp

// ------------------------------------------------------------------------------------------------ quantiser
// grid = 2 * B * H workgroups: block (part = K / V, b, h)
template <bool H>
__global__ __launch_bounds__(256) void kv_head_major_fp8_kernel(const bf16* __restrict__ src, int64_t ld,
                                                                uint8_t* __restrict__ dst, float* __restrict__ scales,
                                                                int B, int Tk, int Hn) {
  __shared__ uint32_t s_max;
  const int blk = blockIdx.x, BH = B * Hn;
  const int part = blk / BH, bh = blk - part * BH, b = bh / Hn, h = bh - b * Hn;
  const int tid = threadIdx.x;
  const bf16* in = src + (int64_t)b * Tk * ld + part * (Hn * 64) + h * 64;
  uint8_t* out = dst + ((int64_t)part * BH + bh) * Tk * 64;
  const int nvec = Tk * 8;                                   // 16-B vectors of the block: 8 per source row
  if (tid == 0) s_max = 0u;
  __syncthreads();
  // pass 1: the largest magnitude, on the bit patterns (sign cleared, a 16-bit float orders as its bits; an inf or
  // NaN pattern is above every finite one)
  uint32_t mx = 0u;
  for (int i = tid; i < nvec; i += 256) {
    const s16x8 v = __builtin_bit_cast(s16x8, *(const bf16x8*)(in + (int64_t)(i >> 3) * ld + (i & 7) * 8));
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = max(mx, (uint32_t)(uint16_t)v[j] & 0x7fffu);
  }
  atomicMax(&s_max, mx);
  __syncthreads();
  mx = s_max;
  const bool finite = mx < (H ? 0x7c00u : 0x7f80u);
  float scale = 1.f, inv = 1.f;
  if (!finite) {
    scale = inv = __uint_as_float(0x7fc00000u);
  } else if (mx != 0u) {
    const int e = scale_exp(__float_as_uint(e2f<H>(__builtin_bit_cast(bf16, (uint16_t)mx))));
    scale = __uint_as_float((uint32_t)(e + 127) << 23);
    inv = __uint_as_float((uint32_t)(127 - e) << 23);
  }
  if (tid == 0) scales[blk] = scale;
  // pass 2 (the block is 192 KB at Tk = 1500: mostly L2 hits): 8 values -> 8 bytes, one 8-B store
  for (int i = tid; i < nvec; i += 256) {
    const bf16x8 v = *(const bf16x8*)(in + (int64_t)(i >> 3) * ld + (i & 7) * 8);
    float f[8];
    words_f32<H>(v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= inv;
    u32x2 w;
    w[0] = cvt4_e4m3(f[0], f[1], f[2], f[3]);
    w[1] = cvt4_e4m3(f[4], f[5], f[6], f[7]);
    *(u32x2*)(out + (int64_t)i * 8) = w;
  }
}

// ------------------------------------------------------------------------------------------------ attention
// the scales of a call: block (b, h) reads k[b * sb + h] and v[b * sb + h] (sb = 0: one clip's blocks for every row)
struct ScaleP {
  const float* k;
  const float* v;
  int64_t sb;
};

// the block's K scale into the score scale; returns its V scale
__device__ __forceinline__ float fold_scales(DecP& p, const ScaleP& s, int b, int h) {
  p.c *= s.k[b * s.sb + h];
  return s.v[b * s.sb + h];
}

template <typename E, bool KS>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_fp8_kernel(DecP p, ScaleP s) {
  const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int tk = eff_tk(p);
  const float vs = fold_scales(p, s, b, h);
  decode_attn_body<E, 4, true, e4m3>(p, b, h, KS ? clamp_start(p.k_start, b, tk) : 0, tk, nullptr, vs);
}

template <typename E, bool KS>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_fp8_split_kernel(DecP p, ScaleP s, int S, float* ws) {
  const int bh = blockIdx.x, c = blockIdx.y;
  const int b = bh / p.H, h = bh % p.H;
  const int tk = eff_tk(p);
  float* part = ws + ((int64_t)bh * gridDim.y + c) * 66;
  const int lo = KS ? max(c * S, clamp_start(p.k_start, b, tk)) : c * S, hi = min(tk, c * S + S);
  if (lo >= hi) {
    store_empty_partial(part);
    return;
  }
  const float vs = fold_scales(p, s, b, h);
  decode_attn_body<E, twd::DA_U, false, e4m3>(p, b, h, lo, hi, part, vs);
}

// the partials hold o already multiplied by the V scale: the combine is the 16-bit path's
template <typename E>
__global__ __launch_bounds__(64) void decode_attn_fp8_combine_kernel(DecP p, int nchunk, const float* ws) {
  combine_row<E>(p, blockIdx.x, nchunk, ws + (int64_t)blockIdx.x * nchunk * 66);
}

template <typename E, int QN>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_mq_fp8_kernel(DecP p, MqP q, ScaleP s) {
  __shared__ float sc[DA_MQ_LDS];
  constexpr int cap = DA_MQ_LDS / QN > DA_MAX_TK ? DA_MAX_TK : DA_MQ_LDS / QN;
  const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int tk0 = eff_tk(p);
  const float vs = fold_scales(p, s, b, h);
  int lo[QN], hi[QN];
  unsigned pend = 0;
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    lo[j] = hi[j] = 0;
    if (j < q.nq) {
      const int tk = min(tk0 + (q.causal ? j : 0), DA_MAX_TK);
      lo[j] = p.k_start ? clamp_start(p.k_start, b, tk) : 0;
      hi[j] = min(tk, lo[j] + cap);
      if (hi[j] > lo[j]) pend |= 1u << j;
    }
  }
  while (pend) {
    int glo, ghi[QN];
    mq_group<QN>(pend, lo, hi, glo, ghi);
    decode_attn_body_mq<E, QN, 4, true, e4m3>(p, q.sqq, q.soq, b, h, glo, ghi, sc, cap, nullptr, 0, vs);
    if (pend) __syncthreads();
  }
}

template <typename E, int QN>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_mq_fp8_split_kernel(DecP p, MqP q, ScaleP s, float* ws) {
  __shared__ float sc[QN * DA_SPLIT];
  const int bh = blockIdx.x, c = blockIdx.y, nchunk = gridDim.y;
  const int b = bh / p.H, h = bh % p.H;
  float* part = ws + (((int64_t)bh * q.nq) * nchunk + c) * 66;
  const int64_t pstride = (int64_t)nchunk * 66;
  const float vs = fold_scales(p, s, b, h);
  int lo[QN], hi[QN];
  unsigned pend = 0;
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    lo[j] = hi[j] = 0;
    if (j < q.nq) {
      const int tk = min(eff_tk(p) + (q.causal ? j : 0), DA_MAX_TK);
      lo[j] = max(c * DA_SPLIT, p.k_start ? clamp_start(p.k_start, b, tk) : 0);
      hi[j] = min(tk, c * DA_SPLIT + DA_SPLIT);
      if (hi[j] > lo[j]) pend |= 1u << j;
      else store_empty_partial(part + j * pstride);        // chunk past the query's keys or below its start
    }
  }
  while (pend) {
    int glo, ghi[QN];
    mq_group<QN>(pend, lo, hi, glo, ghi);
    decode_attn_body_mq<E, QN, twd::DA_U, false, e4m3>(p, q.sqq, q.soq, b, h, glo, ghi, sc, DA_SPLIT, part, pstride,
                                                       vs);
    if (pend) __syncthreads();
  }
}

template <typename E>
__global__ __launch_bounds__(64) void decode_attn_mq_fp8_combine_kernel(DecP p, MqP q, int nchunk, const float* ws) {
  const int j = blockIdx.x % q.nq, bh = blockIdx.x / q.nq;
  p.o = (E*)p.o + j * q.soq;
  combine_row<E>(p, bh, nchunk, ws + (int64_t)blockIdx.x * nchunk * 66);
}

// run the statement with E = the Q / O element type of a 16-bit dtype code (the callers have refused the others)
#define FP8_DISPATCH(dt, ...)                     \
  do {                                            \
    if ((dt) == TW_BF16) { using E = bf16; __VA_ARGS__; } \
    else { using E = f16; __VA_ARGS__; }          \
  } while (0)

template <bool KS>
int launch_sq(const DecP& p, const ScaleP& s, int B, int dtype, hipStream_t stream) {
  const int pairs = B * p.H;
  const int nchunk = (p.Tk + DA_SPLIT - 1) / DA_SPLIT;
  if (dec_split(nullptr, pairs, nchunk)) {
    float* ws = (float*)tw_device_workspace(stream, (size_t)pairs * nchunk * 66 * sizeof(float));
    if (ws) {
      FP8_DISPATCH(dtype, hipLaunchKernelGGL((decode_attn_fp8_split_kernel<E, KS>), dim3(pairs, nchunk),
                                             dim3(DA_THREADS), 0, stream, p, s, DA_SPLIT, ws));
      FP8_DISPATCH(dtype, hipLaunchKernelGGL(decode_attn_fp8_combine_kernel<E>, dim3(pairs), dim3(64), 0, stream, p,
                                             nchunk, ws));
      TW_CHECK_LAUNCH();
      return TW_OK;
    }
  }
  FP8_DISPATCH(dtype, hipLaunchKernelGGL((decode_attn_fp8_kernel<E, KS>), dim3(pairs), dim3(DA_THREADS), 0, stream,
                                         p, s));
  TW_CHECK_LAUNCH();
  return TW_OK;
}

template <int QN>
int launch_mq(const DecP& p, const MqP& q, const ScaleP& s, int B, int nchunk, bool split, int dtype,
              hipStream_t stream) {
  float* ws = split ? (float*)tw_device_workspace(stream, (size_t)B * p.H * q.nq * nchunk * 66 * sizeof(float))
                    : nullptr;
  if (ws) {
    FP8_DISPATCH(dtype, hipLaunchKernelGGL((decode_attn_mq_fp8_split_kernel<E, QN>), dim3(B * p.H, nchunk),
                                           dim3(DA_THREADS), 0, stream, p, q, s, ws));
    FP8_DISPATCH(dtype, hipLaunchKernelGGL(decode_attn_mq_fp8_combine_kernel<E>, dim3(B * p.H * q.nq), dim3(64), 0,
                                           stream, p, q, nchunk, ws));
  } else {
    FP8_DISPATCH(dtype, hipLaunchKernelGGL((decode_attn_mq_fp8_kernel<E, QN>), dim3(B * p.H), dim3(DA_THREADS), 0,
                                           stream, p, q, s));
  }
  TW_CHECK_LAUNCH();
  return TW_OK;
}

// the checks of the two attention entry points beyond dec_fill's
int fp8_checks(const float* k_scale, const float* v_scale, int64_t ssb, const int* tk_dev, int dtype) {
  if (tk_dev) return TW_EUNSUPPORTED;             // the self-attention cache stays 16-bit
  if (dtype != TW_BF16 && dtype != TW_F16) return TW_EUNSUPPORTED;
  if (!k_scale || !v_scale || ssb < 0) return TW_EINVAL;
  return TW_OK;
}

}  // namespace

extern "C" int tw_kv_head_major_fp8(const void* src, int64_t ld, void* dst, float* scales, int B, int Tk, int H,
                                    int dtype, hipStream_t stream) {
  if (dtype != TW_BF16 && dtype != TW_F16) return TW_EUNSUPPORTED;
  if (B <= 0 || Tk <= 0 || H <= 0) return TW_OK;
  if (!src || !dst || !scales) return TW_EINVAL;
  if ((ld & 7) || ld < 2 * 64 * H || (((uintptr_t)src | (uintptr_t)dst) & 15) || ((uintptr_t)scales & 3))
    return TW_EINVAL;
  if ((int64_t)2 * B * H > 0x7fffffff || (int64_t)Tk * 8 > 0x7fffffff) return TW_EUNSUPPORTED;
  const dim3 grid((unsigned)(2 * B * H));
  if (dtype == TW_F16)
    hipLaunchKernelGGL(kv_head_major_fp8_kernel<true>, grid, dim3(256), 0, stream, (const bf16*)src, ld,
                       (uint8_t*)dst, scales, B, Tk, H);
  else
    hipLaunchKernelGGL(kv_head_major_fp8_kernel<false>, grid, dim3(256), 0, stream, (const bf16*)src, ld,
                       (uint8_t*)dst, scales, B, Tk, H);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_decode_attn_fp8(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, int64_t hsk,
                                  const void* v, int64_t ldv, int64_t svb, int64_t hsv, const float* k_scale,
                                  const float* v_scale, int64_t ssb, void* o, int64_t sob, int B, int H, int Tk,
                                  const int* tk_dev, const int* k_start, int head_dim, float scale, int dtype,
                                  hipStream_t stream) {
  if (head_dim != 64) return TW_EUNSUPPORTED;
  if (const int st = fp8_checks(k_scale, v_scale, ssb, tk_dev, dtype)) return st;
  if (B <= 0 || H <= 0) return TW_OK;
  DecP p;
  if (const int st = dec_fill(p, q, sqb, k, ldk, skb, hsk, v, ldv, svb, hsv, o, sob, H, Tk, Tk, nullptr, k_start,
                              scale))
    return st;
  const ScaleP s{k_scale, v_scale, ssb};
  return k_start ? launch_sq<true>(p, s, B, dtype, stream) : launch_sq<false>(p, s, B, dtype, stream);
}

extern "C" int tw_decode_attn_mq_fp8(const void* q, int64_t sqb, int64_t sqq, const void* k, int64_t ldk, int64_t skb,
                                     int64_t hsk, const void* v, int64_t ldv, int64_t svb, int64_t hsv,
                                     const float* k_scale, const float* v_scale, int64_t ssb, void* o, int64_t sob,
                                     int64_t soq, int B, int H, int Q, int Tk, const int* tk_dev, const int* k_start,
                                     int causal, int head_dim, float scale, int dtype, hipStream_t stream) {
  if (head_dim != 64) return TW_EUNSUPPORTED;
  if (Q < 1 || Q > DA_MQ) return TW_EINVAL;
  if (const int st = fp8_checks(k_scale, v_scale, ssb, tk_dev, dtype)) return st;
  if (B <= 0 || H <= 0) return TW_OK;
  const int tk_last = Tk + (causal ? Q - 1 : 0);
  if (B * H >= DA_BIG) return TW_EUNSUPPORTED;
  DecP p;
  if (const int st = dec_fill(p, q, sqb, k, ldk, skb, hsk, v, ldv, svb, hsv, o, sob, H, Tk, tk_last, nullptr, k_start,
                              scale))
    return st;
  if ((sqq & 7) || sqq < 0 || soq < 0) return TW_EINVAL;
  const int QN = Q <= 1 ? 1 : Q <= 2 ? 2 : Q <= 4 ? 4 : 8;
  const int nchunk = (tk_last + DA_SPLIT - 1) / DA_SPLIT;
  const bool split = dec_split(nullptr, B * H, nchunk);
  if (!split && tk_last > DA_MQ_LDS / QN) return TW_EUNSUPPORTED;
  MqP m;
  m.sqq = sqq; m.soq = soq; m.nq = Q; m.causal = causal ? 1 : 0;
  const ScaleP s{k_scale, v_scale, ssb};
  switch (QN) {
    case 1: return launch_mq<1>(p, m, s, B, nchunk, split, dtype, stream);
    case 2: return launch_mq<2>(p, m, s, B, nchunk, split, dtype, stream);
    case 4: return launch_mq<4>(p, m, s, B, nchunk, split, dtype, stream);
    default: return launch_mq<8>(p, m, s, B, nchunk, split, dtype, stream);
  }
}
