// Language detection over one decoder step's logits (gfx950).
//
//  * tw_lang_detect: HF WhisperGenerationMixin.detect_language's last two lines (generation_whisper.py: every
//    non-language logit masked to -inf, then argmax) without the mask: the L language logits of each row are
//    gathered through a device table of their token ids, and per row the kernel writes the id of the largest one
//    and, optionally, the softmax over those L values alone.
//
// One wave per row: L <= 256, so a lane holds at most LD_PER entries (entry j on lane j & 63), gathered as L
// scattered loads from a row of ~52k columns; the argmax and the sum are wave butterflies (__shfl_xor), no LDS and
// no barrier.  The argmax carries (value, table index) pairs under torch.argmax's order -- NaN above everything,
// then the larger value, ties and NaNs to the lower index -- which is a total order, so the butterfly's result does
// not depend on the pairing.  Every output element is written once by one lane.
#include "common.h"
#include "tw_hip.h"

#define LD_MAX 256
#define LD_PER (LD_MAX / 64)

// (a, ia) ranks above (b, ib): torch.argmax's rule on distinct indices
__device__ __forceinline__ bool ld_above(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na | nb) return na && (!nb || ia < ib);
  return a > b || (a == b && ia < ib);
}

template <typename E>
__global__ __launch_bounds__(64) void lang_detect_kernel(const E* __restrict__ logits, int64_t ld, int V,
                                                         const int* __restrict__ table, int L,
                                                         int64_t* __restrict__ out_ids, int64_t id_stride,
                                                         float* __restrict__ out_probs, int64_t ld_p) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const E* __restrict__ row = logits + b * ld;
  float x[LD_PER];
  float best = 0.f;
  int bi = LD_MAX;                        // above every real index: an empty lane loses to any entry
#pragma unroll
  for (int k = 0; k < LD_PER; ++k) {
    const int j = lane + 64 * k;
    x[k] = -__builtin_inff();
    if (j < L) {
      const int id = table[j];
      // the table is checked where it is built; an id outside [0, V) reads nothing and counts as -inf
      if ((unsigned)id < (unsigned)V) x[k] = to_f32(row[id]);
      if (bi == LD_MAX || ld_above(x[k], j, best, bi)) { best = x[k]; bi = j; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi < LD_MAX && (bi == LD_MAX || ld_above(ov, oi, best, bi))) { best = ov; bi = oi; }
  }
  // L >= 1: bi is a real index on every lane now, and `best` its value (the row's maximum, or NaN)
  if (lane == 0) out_ids[b * id_stride] = (int64_t)table[bi];
  if (!out_probs) return;
  // softmax over the L values: a NaN maximum, or -inf - -inf on an all -inf row, makes every term NaN
  float e[LD_PER], s = 0.f;
#pragma unroll
  for (int k = 0; k < LD_PER; ++k) {
    e[k] = lane + 64 * k < L ? expf(x[k] - best) : 0.f;
    s += e[k];
  }
  s = wave_sum(s);
  float* __restrict__ pr = out_probs + b * ld_p;
#pragma unroll
  for (int k = 0; k < LD_PER; ++k)
    if (lane + 64 * k < L) pr[lane + 64 * k] = __fdiv_rn(e[k], s);
}

extern "C" int tw_lang_detect(const void* logits, int64_t ld, int logits_dtype, int B, int V, const int* lang_ids,
                              int L, int64_t* out_ids, int64_t id_stride, float* out_probs, int64_t ld_p,
                              tw_stream_t stream) {
  if (B < 0 || V <= 0 || ld < V || L < 1 || L > LD_MAX || id_stride < 1) return TW_EINVAL;
  if (!logits || !lang_ids || !out_ids || (out_probs && ld_p < L)) return TW_EINVAL;
  if (logits_dtype != TW_F32 && logits_dtype != TW_BF16 && logits_dtype != TW_F16) return TW_EUNSUPPORTED;
  if (B == 0) return TW_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(B), block(64);
  if (logits_dtype == TW_BF16)
    hipLaunchKernelGGL(lang_detect_kernel<bf16>, grid, block, 0, s, (const bf16*)logits, ld, V, lang_ids, L, out_ids,
                       id_stride, out_probs, ld_p);
  else if (logits_dtype == TW_F16)
    hipLaunchKernelGGL(lang_detect_kernel<f16>, grid, block, 0, s, (const f16*)logits, ld, V, lang_ids, L, out_ids,
                       id_stride, out_probs, ld_p);
  else
    hipLaunchKernelGGL(lang_detect_kernel<float>, grid, block, 0, s, (const float*)logits, ld, V, lang_ids, L,
                       out_ids, id_stride, out_probs, ld_p);
  TW_CHECK_LAUNCH();
  return TW_OK;
}
