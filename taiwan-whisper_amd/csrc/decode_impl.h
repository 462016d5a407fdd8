// Decode attention bodies (one query row per (clip, head) over a KV cache) of the kernels in decode.hip.
#pragma once
#include "common.h"

#include <type_traits>

namespace twd {

constexpr int DA_THREADS = 256;
constexpr int DA_MAX_TK = 2048;
constexpr int DA_SPLIT = 128;   // keys per workgroup of the split (flash-decoding) variant
constexpr int DA_U = 4;           // key sub-steps per wave iteration (loads in flight per lane)
constexpr int DA_BIG = 4096;      // (clip, head) pairs from which the one-workgroup-per-pair kernel takes DA_U = 2

struct DecP {
  const void* q; int64_t sqb;
  const void* k; int64_t ldk, skb;
  const void* v; int64_t ldv, svb;
  void* o; int64_t sob;
  int64_t hsk, hsv;   // head strides of K and V (64: heads side by side in a row; Tk*64: head-major blocks)
  int H, Tk;
  const int* tk_dev;  // nullable: effective Tk = *tk_dev + Tk (graph-captured decode steps)
  const int* k_start; // nullable: row b attends keys from k_start[b] (left-padded prompts); null: every row from key 0
  float c;        // scale * log2(e)
};

// K / V rows of the one-workgroup-per-pair kernel are read once per decode step: NT streams them past the caches
// (nontemporal loads, 16-bit forms; the fp32 path reads plainly)
template <bool NT>
__device__ __forceinline__ void load8_kv(const bf16* p, float* o) {
  if constexpr (NT) {
    const bf16x8 v = __builtin_nontemporal_load((const bf16x8*)p);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bf2f(v[j]);
  } else {
    load8(p, o);
  }
}
template <bool NT>
__device__ __forceinline__ void load8_kv(const f16* p, float* o) {
  if constexpr (NT) {
    const f16x8 v = __builtin_nontemporal_load((const f16x8*)p);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (float)v[j];
  } else {
    load8(p, o);
  }
}
template <bool NT>
__device__ __forceinline__ void load8_kv(const float* p, float* o) { load8(p, o); }

// K/V element of the 8-bit cross-attention cache (csrc/xkv_fp8.hip): one OCP e4m3fn byte.  8 elements are one 8-B
// load; v_cvt_pk_f32_fp8 converts two bytes of a dword at a time (exact: every e4m3 value is an fp32 value).
struct e4m3 { uint8_t b; };
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
template <bool NT>
__device__ __forceinline__ void load8_kv(const e4m3* p, float* o) {
  u32x2 w;
  if constexpr (NT) w = __builtin_nontemporal_load((const u32x2*)p);
  else w = *(const u32x2*)p;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
    o[4 * j] = lo[0]; o[4 * j + 1] = lo[1]; o[4 * j + 2] = hi[0]; o[4 * j + 3] = hi[1];
  }
}

// lane = (key slot ks = lane >> 3, 8-element chunk ch = lane & 7); a wave covers 8 keys per step.
// E = bf16 (autocast path) or float (fp32 path: exact expf, no rounding of the output).
// The body attends keys [lo, hi).  part == nullptr: normalise and store O.  Otherwise (split over keys,
// flash-decoding) store the chunk's unnormalised o[64], its max m (log2 domain) and sum l to part[0..65]
// for decode_attn_combine_kernel.
// KV = the K / V element type: E, or e4m3 (the 8-bit cross-attention cache; K / V strides then count bytes).  Its
// callers fold the block's K scale into p.c and pass the V scale as vs: both are powers of two, so c * sK and the
// one multiplication of the reduced o by vs are exact, and the result is the fp32 arithmetic of the dequantised cache.
template <typename E, int DA_U = twd::DA_U, bool NT = false, typename KV = E>
__device__ __forceinline__ void decode_attn_body(const DecP& p, int b, int h, int lo, int hi, float* part,
                                                 float vs = 1.f) {
  __shared__ float sc[DA_MAX_TK];
  __shared__ float red[DA_THREADS / 64][64];
  __shared__ float red_l[DA_THREADS / 64];
  __shared__ float red_m[DA_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ks = lane >> 3, ch = lane & 7;
  constexpr bool F32 = sizeof(E) == 4;
  const E* qb = (const E*)p.q + b * p.sqb + h * 64 + ch * 8;
  const KV* kb = (const KV*)p.k + b * p.skb + h * p.hsk + ch * 8;
  const KV* vb = (const KV*)p.v + b * p.svb + h * p.hsv + ch * 8;
  float qv[8];
  load8(qb, qv);
  // pass 1: scores (log2 domain) -> LDS, running max.  A wave takes 8 keys x DA_U sub-steps per iteration
  // (keys k0 + 8u + ks): DA_U independent 16-B loads per lane in flight before the reductions.
  float mx = -INFINITY;
  for (int k0 = lo + wave * 8 * DA_U; k0 < hi; k0 += DA_THREADS / 8 * DA_U) {
    float t[DA_U][8];
#pragma unroll
    for (int u = 0; u < DA_U; ++u) {
      const int key = k0 + 8 * u + ks;
      if (key < hi) load8_kv<NT>(kb + (int64_t)key * p.ldk, t[u]);
    }
#pragma unroll
    for (int u = 0; u < DA_U; ++u) {
      const int key = k0 + 8 * u + ks;
      float sv = 0.f;
      if (key < hi) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sv = fmaf(qv[j], t[u][j], sv);
      }
      sv = oct_sum_dpp(sv);          // xor 1, 2, 4 on the VALU (bit-identical to the shuffles: common.h)
      if (key < hi) {
        sv *= p.c;
        if (ch == 0) sc[key - lo] = sv;
        mx = fmaxf(mx, sv);
      }
    }
  }
  mx = wave_max_dpp(mx);
  if (lane == 0) red_m[wave] = mx;
  __syncthreads();
  float m = red_m[0];
#pragma unroll
  for (int w = 1; w < DA_THREADS / 64; ++w) m = fmaxf(m, red_m[w]);
  // pass 2: p = exp2(s - m), l = sum p, o = sum p * V (same key order within each lane slot)
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int k0 = lo + wave * 8 * DA_U; k0 < hi; k0 += DA_THREADS / 8 * DA_U) {
    float t[DA_U][8];
#pragma unroll
    for (int u = 0; u < DA_U; ++u) {
      const int key = k0 + 8 * u + ks;
      if (key < hi) load8_kv<NT>(vb + (int64_t)key * p.ldv, t[u]);
    }
#pragma unroll
    for (int u = 0; u < DA_U; ++u) {
      const int key = k0 + 8 * u + ks;
      if (key < hi) {
        const float pe = F32 ? exp2f(sc[key - lo] - m) : __builtin_amdgcn_exp2f(sc[key - lo] - m);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = fmaf(pe, t[u][j], o[j]);
        if (ch == 0) l += pe;
      }
    }
  }
  // reduce over the 8 key slots of the wave (lanes ch, ch+8, ..., ch+56), then over waves
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = stride8_sum_dpp(o[j]);    // xor 8, 16, 32
  l = wave_sum_dpp(l);
  if (ks == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wave][ch * 8 + j] = o[j];
  }
  if (lane == 0) red_l[wave] = l;
  __syncthreads();
  if (tid < 64) {
    float acc = 0.f, lt = 0.f;
#pragma unroll
    for (int w = 0; w < DA_THREADS / 64; ++w) {
      acc += red[w][tid];
      lt += red_l[w];
    }
    if constexpr (!std::is_same_v<KV, E>) acc *= vs;
    if (part) {
      part[tid] = acc;
      if (tid == 0) {
        part[64] = m;
        part[65] = lt;
      }
    } else {
      ((E*)p.o)[b * p.sob + h * 64 + tid] = e_from_f32<E>(acc / lt);
    }
  }
}

// Multi-query form of decode_attn_body (the verify pass of assisted decoding: QN consecutive query rows of one
// (clip, head), rows sqq apart, outputs soq apart): every K and every V vector is loaded ONCE and used for all the
// queries.  Query j attends keys [lo, hi[j]) -- one common lo, which fixes the key -> (wave, sub-step, lane slot)
// walk, so per query every operation below is the one decode_attn_body performs for that query alone, in the same
// order: the outputs are bit-identical.  hi[j] <= lo leaves query j out (nothing computed or stored for it).
// Keys at or above max_j hi[j] are never loaded.  sc: LDS scores, QN rows of `cap` floats (hi[j] - lo <= cap).
// part == nullptr: normalise and store O; otherwise query j's partial goes to part + j * pstride (66 floats).
constexpr int DA_MQ = 8;                // most query rows per (clip, head)
constexpr int DA_MQ_LDS = 12288;        // score floats of the one-workgroup multi-query kernel (48 KB)
// KV, vs: as in decode_attn_body.
template <typename E, int QN, int DA_U = twd::DA_U, bool NT = false, typename KV = E>
__device__ __forceinline__ void decode_attn_body_mq(const DecP& p, int64_t sqq, int64_t soq, int b, int h, int lo,
                                                    const int (&hi)[QN], float* sc, int cap, float* part,
                                                    int64_t pstride, float vs = 1.f) {
  __shared__ float red[DA_THREADS / 64][QN][64];
  __shared__ float red_l[DA_THREADS / 64][QN];
  __shared__ float red_m[DA_THREADS / 64][QN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ks = lane >> 3, ch = lane & 7;
  constexpr bool F32 = sizeof(E) == 4;
  const E* qb = (const E*)p.q + b * p.sqb + h * 64 + ch * 8;
  const KV* kb = (const KV*)p.k + b * p.skb + h * p.hsk + ch * 8;
  const KV* vb = (const KV*)p.v + b * p.svb + h * p.hsv + ch * 8;
  int himax = lo;
#pragma unroll
  for (int j = 0; j < QN; ++j) himax = max(himax, hi[j]);
  float qv[QN][8];
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    if (hi[j] > lo) {
      load8(qb + j * sqq, qv[j]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) qv[j][i] = 0.f;
    }
  }
  // pass 1: one K load per key, QN scores
  float mx[QN];
#pragma unroll
  for (int j = 0; j < QN; ++j) mx[j] = -INFINITY;
  for (int k0 = lo + wave * 8 * DA_U; k0 < himax; k0 += DA_THREADS / 8 * DA_U) {
    float t[DA_U][8];
#pragma unroll
    for (int u = 0; u < DA_U; ++u) {
      const int key = k0 + 8 * u + ks;
      if (key < himax) load8_kv<NT>(kb + (int64_t)key * p.ldk, t[u]);
    }
#pragma unroll
    for (int u = 0; u < DA_U; ++u) {
      const int key = k0 + 8 * u + ks;
#pragma unroll
      for (int j = 0; j < QN; ++j) {
        if (k0 + 8 * u >= hi[j]) continue;             // uniform: none of this sub-step's keys is query j's
        float sv = 0.f;
        if (key < hi[j]) {
#pragma unroll
          for (int i = 0; i < 8; ++i) sv = fmaf(qv[j][i], t[u][i], sv);
        }
        sv = oct_sum_dpp(sv);
        if (key < hi[j]) {
          sv *= p.c;
          if (ch == 0) sc[j * cap + key - lo] = sv;
          mx[j] = fmaxf(mx[j], sv);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    mx[j] = wave_max_dpp(mx[j]);
    if (lane == 0) red_m[wave][j] = mx[j];
  }
  __syncthreads();
  float m[QN];
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    m[j] = red_m[0][j];
#pragma unroll
    for (int w = 1; w < DA_THREADS / 64; ++w) m[j] = fmaxf(m[j], red_m[w][j]);
  }
  // pass 2: one V load per key, QN weighted sums
  float o[QN][8];
  float l[QN];
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[j][i] = 0.f;
  }
  for (int k0 = lo + wave * 8 * DA_U; k0 < himax; k0 += DA_THREADS / 8 * DA_U) {
    float t[DA_U][8];
#pragma unroll
    for (int u = 0; u < DA_U; ++u) {
      const int key = k0 + 8 * u + ks;
      if (key < himax) load8_kv<NT>(vb + (int64_t)key * p.ldv, t[u]);
    }
#pragma unroll
    for (int u = 0; u < DA_U; ++u) {
      const int key = k0 + 8 * u + ks;
#pragma unroll
      for (int j = 0; j < QN; ++j) {
        if (key < hi[j]) {
          const float s = sc[j * cap + key - lo];
          const float pe = F32 ? exp2f(s - m[j]) : __builtin_amdgcn_exp2f(s - m[j]);
#pragma unroll
          for (int i = 0; i < 8; ++i) o[j][i] = fmaf(pe, t[u][i], o[j][i]);
          if (ch == 0) l[j] += pe;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < QN; ++j) {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[j][i] = stride8_sum_dpp(o[j][i]);
    l[j] = wave_sum_dpp(l[j]);
    if (ks == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) red[wave][j][ch * 8 + i] = o[j][i];
    }
    if (lane == 0) red_l[wave][j] = l[j];
  }
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int j = 0; j < QN; ++j) {
      if (hi[j] <= lo) continue;
      float acc = 0.f, lt = 0.f;
#pragma unroll
      for (int w = 0; w < DA_THREADS / 64; ++w) {
        acc += red[w][j][tid];
        lt += red_l[w][j];
      }
      if constexpr (!std::is_same_v<KV, E>) acc *= vs;
      if (part) {
        float* pj = part + j * pstride;
        pj[tid] = acc;
        if (tid == 0) {
          pj[64] = m[j];
          pj[65] = lt;
        }
      } else {
        ((E*)p.o)[b * p.sob + j * soq + h * 64 + tid] = e_from_f32<E>(acc / lt);
      }
    }
  }
}

// O = sum_c 2^(m_c - M) o_c / sum_c 2^(m_c - M) l_c over the chunks of one (clip, head), in chunk order,
// by the 64 lanes of one wave (lane = output dimension).  Lane c loads chunk c's (m, l) and every lane its
// column of all chunks up front (independent loads instead of a dependent chain), weights by shuffles.
constexpr int DA_MAX_CHUNK = 16;
template <typename E>
__device__ __forceinline__ void combine_row(const DecP& p, int bh, int nchunk, const float* part) {
  const int lane = threadIdx.x & 63;
  const int b = bh / p.H, h = bh % p.H;
  const float mc = lane < nchunk ? part[lane * 66 + 64] : -INFINITY;
  const float lc = lane < nchunk ? part[lane * 66 + 65] : 0.f;
  float oc[DA_MAX_CHUNK];
#pragma unroll
  for (int c = 0; c < DA_MAX_CHUNK; ++c) oc[c] = c < nchunk ? part[c * 66 + lane] : 0.f;
  const float M = wave_max_dpp(mc);
  const float wc = mc == -INFINITY ? 0.f : (sizeof(E) == 4 ? exp2f(mc - M) : __builtin_amdgcn_exp2f(mc - M));
  float acc = 0.f, lt = 0.f;
#pragma unroll
  for (int c = 0; c < DA_MAX_CHUNK; ++c) {
    if (c < nchunk) {
      const float w = readlane_f(wc, c), l = readlane_f(lc, c);
      if (readlane_f(mc, c) != -INFINITY) {
        acc = fmaf(w, oc[c], acc);
        lt = fmaf(w, l, lt);
      }
    }
  }
  ((E*)p.o)[b * p.sob + h * 64 + lane] = e_from_f32<E>(acc / lt);
}

// ---- what the kernels of decode.hip (16-bit / fp32 K and V) and xkv_fp8.hip (e4m3 K and V) share around the bodies

// effective key count of a call: the fixed Tk plus the device-side step index, bounded by the score buffer
__device__ __forceinline__ int eff_tk(const DecP& p) { return min(p.Tk + (p.tk_dev ? *p.tk_dev : 0), DA_MAX_TK); }

// per-row key start (left-padded decoder prompts: HF's decoder attention mask): row b attends keys
// [k_start[b], tk), the start clamped into [0, tk - 1] so at least the last key -- the step's own -- is used and no
// row below 0 or at / past tk is read.  The body walks from lo, so row b's result is bit-identical to the plain
// call run on that row alone with K / V advanced by k_start[b] rows over tk - k_start[b] keys; without k_start
// every row starts at key 0.  The single-query kernels take the choice as a template argument (KS): with a
// run-time test of p.k_start the plain one-workgroup kernel measured 174 -> 186 us at 128 clips x 20 heads
// (profiles/decode_refactor_ab.txt), so the KS = false instantiations are the kernels without the feature.
__device__ __forceinline__ int clamp_start(const int* k_start, int b, int tk) {
  return max(min(k_start[b], tk - 1), 0);
}

// the partial of a chunk that holds none of a query's keys (m = -inf, l = 0): the combine kernels skip it
__device__ __forceinline__ void store_empty_partial(float* part) {
  if (threadIdx.x < 64) part[threadIdx.x] = 0.f;
  if (threadIdx.x == 0) {
    part[64] = -INFINITY;
    part[65] = 0.f;
  }
}

// multi-query calls: the query rows of one (clip, head) and the grouping of the queries that share a key start
struct MqP {
  int64_t sqq, soq;
  int nq, causal;
};
template <int QN>
__device__ __forceinline__ void mq_group(unsigned& pend, const int (&lo)[QN], const int (&hi)[QN], int& glo,
                                         int (&ghi)[QN]) {
  bool found = false;
  glo = 0;
#pragma unroll
  for (int j = 0; j < QN; ++j)
    if (!found && ((pend >> j) & 1u)) { glo = lo[j]; found = true; }
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    const bool in = ((pend >> j) & 1u) && lo[j] == glo;
    ghi[j] = in ? hi[j] : glo;
    if (in) pend &= ~(1u << j);
  }
}

// The checks the decode-attention entry points share (statuses as include/tw_hip.h lists them) and the DecP of the
// call.  tk_last: the most keys a query of a fixed-Tk call attends.  K / V strides count K / V elements.
inline int dec_fill(DecP& p, const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, int64_t hsk,
                    const void* v, int64_t ldv, int64_t svb, int64_t hsv, void* o, int64_t sob, int H, int Tk,
                    int tk_last, const int* tk_dev, const int* k_start, float scale) {
  if ((!tk_dev && Tk <= 0) || tk_last > DA_MAX_TK) return TW_EUNSUPPORTED;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return TW_EINVAL;
  if ((sqb | ldk | skb | ldv | svb | hsk | hsv) & 7) return TW_EINVAL;
  if (skb < 0 || svb < 0 || hsk < 0 || hsv < 0) return TW_EINVAL;
  p.q = q; p.sqb = sqb;
  p.k = k; p.ldk = ldk; p.skb = skb;
  p.v = v; p.ldv = ldv; p.svb = svb;
  p.o = o; p.sob = sob;
  p.hsk = hsk; p.hsv = hsv;
  p.H = H; p.Tk = Tk; p.tk_dev = tk_dev; p.k_start = k_start; p.c = scale * 1.4426950408889634f;
  return TW_OK;
}
// fixed-Tk calls on few (clip, head) pairs split the keys into chunks of DA_SPLIT
inline bool dec_split(const int* tk_dev, int pairs, int nchunk) {
  return !tk_dev && pairs < 640 && nchunk >= 2 && nchunk <= DA_MAX_CHUNK;
}

}  // namespace twd
