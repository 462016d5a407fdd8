// Repetition penalty and no-repeat n-gram as a pre-pass of the token selection (gfx950).
//
//  * tw_repeat_process: HF RepetitionPenaltyLogitsProcessor followed by NoRepeatNGramLogitsProcessor
//    (logits_process.py), the two processors GenerationMixin._get_logits_processor puts in front of
//    Whisper's own: out[b][0..V) = the fp32 view of logits row b with every token of the row's
//    history ids[b][0..L) penalised once (x < 0 ? x * p : x / p, from the unpenalised score) and
//    every token that would complete an n-gram already in the history set to -inf.  The selection
//    kernels (decode.hip) then read `out` as an fp32 row, unchanged.
//
// A workgroup owns RP_SLICE consecutive columns of one row.  It scans the row's history (L <= 448
// ids for Whisper) into two RP_SLICE-bit masks in LDS -- tokens to penalise, tokens to ban -- and,
// after one barrier, streams its columns once: 16-B loads, the penalty and then the ban on the
// marked elements in registers, 16-B fp32 stores.  Every output element is written exactly once by
// one thread, so duplicates in the history, and a token that is both penalised and banned, need no
// ordering between stores: the ban is applied after the penalty in the same registers.
#include "common.h"
#include "tw_hip.h"

#define RP_THREADS 256
#define RP_VEC 8
#define RP_SLICE (RP_THREADS * RP_VEC)

struct RepP {
  const void* logits;
  int64_t ld;
  const int64_t* ids;
  int64_t ld_ids;
  const int* t_dev;
  float* out;
  int64_t ld_out;
  int V, col, ngram, vec;
  float penalty;
};

// set token u's bit when it falls into the slice that starts at column c0
__device__ __forceinline__ void rp_mark(uint32_t* bits, int64_t u, int c0) {
  const uint64_t r = (uint64_t)(u - c0);            // u < c0 (negative ids included) wraps past RP_SLICE
  if (r < (uint64_t)RP_SLICE) atomicOr(&bits[r >> 5], 1u << (r & 31));
}

template <typename E>
__global__ __launch_bounds__(RP_THREADS) void repeat_process_kernel(RepP p) {
  __shared__ uint32_t pen[RP_SLICE / 32], ban[RP_SLICE / 32];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int c0 = blockIdx.x * RP_SLICE, c = c0 + tid * RP_VEC;
  const E* __restrict__ src = (const E*)p.logits + (int64_t)b * p.ld;
  float* __restrict__ dst = p.out + (int64_t)b * p.ld_out;
  const int64_t* __restrict__ h = p.ids + (int64_t)b * p.ld_ids;
  int L = p.col + (p.t_dev ? *p.t_dev : 0);
  if (L < 0) L = 0;
  // the row's columns first: their latency hides behind the history scan.  Columns >= V are never read
  // into a result (the input's pad columns may hold anything) and never written.
  const bool full = p.vec && c + RP_VEC <= p.V;
  float x[RP_VEC];
  if (full) {
    load8(src + c, x);
  } else {
#pragma unroll
    for (int j = 0; j < RP_VEC; ++j) x[j] = c + j < p.V ? to_f32(src[c + j]) : 0.f;
  }
  if (tid < RP_SLICE / 32) pen[tid] = ban[tid] = 0u;
  __syncthreads();
  if (p.penalty != 1.0f)
    for (int i = tid; i < L; i += RP_THREADS) rp_mark(pen, h[i], c0);
  const int n = p.ngram;
  if (n > 0) {
    // window i = ids[i .. i+n) repeats when its first n-1 ids equal the last n-1 of the history; its last id is
    // then banned.  i <= L - n: the window that starts at the suffix itself is one id short (HF: cur_len < n bans
    // nothing, and a suffix never bans its own successor).  64-bit compares.
    const int64_t* tail = h + (L - n + 1);
    for (int i = tid; i <= L - n; i += RP_THREADS) {
      bool same = true;
      for (int j = 0; j < n - 1; ++j) same &= h[i + j] == tail[j];
      if (same) rp_mark(ban, h[i + n - 1], c0);
    }
  }
  __syncthreads();
  const int sh = (tid & 3) * RP_VEC;
  const uint32_t pb = (pen[tid >> 2] >> sh) & 0xffu, bb = (ban[tid >> 2] >> sh) & 0xffu;
  if (pb | bb) {
    const float pnl = p.penalty;
#pragma unroll
    for (int j = 0; j < RP_VEC; ++j) {
      // one correctly rounded fp32 multiply or divide (torch.where(s < 0, s * p, s / p)); -0.0 and NaN take
      // the quotient, as `s < 0` is false for them
      if ((pb >> j) & 1u) x[j] = x[j] < 0.f ? __fmul_rn(x[j], pnl) : __fdiv_rn(x[j], pnl);
      if ((bb >> j) & 1u) x[j] = -__builtin_inff();
    }
  }
  if (full) {
    store8(dst + c, x);
  } else {
#pragma unroll
    for (int j = 0; j < RP_VEC; ++j)
      if (c + j < p.V) dst[c + j] = x[j];
  }
}

extern "C" int tw_repeat_process(const void* logits, int64_t ld, int logits_dtype, int B, int V, const int64_t* ids,
                                 int64_t ld_ids, int col, const int* t_dev, float penalty, int ngram, float* out,
                                 int64_t ld_out, tw_stream_t stream) {
  if (!(penalty > 0.f) || ngram < 0 || B <= 0 || V <= 0 || ld < V || ld_out < V || col < 0) return TW_EINVAL;
  if (!logits || !ids || !out || B > 65535) return TW_EINVAL;
  if (logits_dtype != TW_F32 && logits_dtype != TW_BF16 && logits_dtype != TW_F16) return TW_EUNSUPPORTED;
  const int esz = logits_dtype == TW_F32 ? 4 : 2;
  // 16-B vectors need every row of both matrices to start on a 16-B boundary; otherwise element by element
  const int vec = !(((uintptr_t)logits | (uintptr_t)out | (uint64_t)(ld * esz) | (uint64_t)(ld_out * 4)) & 15);
  RepP p{logits, ld, ids, ld_ids, t_dev, out, ld_out, V, col, ngram, vec, penalty};
  const dim3 grid((V + RP_SLICE - 1) / RP_SLICE, B);
  hipStream_t s = (hipStream_t)stream;
  if (logits_dtype == TW_BF16) hipLaunchKernelGGL(repeat_process_kernel<bf16>, grid, dim3(RP_THREADS), 0, s, p);
  else if (logits_dtype == TW_F16) hipLaunchKernelGGL(repeat_process_kernel<f16>, grid, dim3(RP_THREADS), 0, s, p);
  else hipLaunchKernelGGL(repeat_process_kernel<float>, grid, dim3(RP_THREADS), 0, s, p);
  TW_CHECK_LAUNCH();
  return TW_OK;
}
