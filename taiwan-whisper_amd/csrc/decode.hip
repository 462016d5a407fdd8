// Greedy decoding with a KV cache (generate_step, run_distillation.py:1580-1584;
// HF generation_whisper.py greedy path; logits processors logits_process.py SuppressTokens /
// SuppressTokensAtBegin).
//
//  * tw_decode_attn: one query row per (batch, head) against Tk cached keys — the decoder's
//    self-attention over its cache (Tk = t + 1) and cross-attention over the encoder frames
//    (Tk = 1500).  HBM-bound: every K and V row is read once, 16 B per lane (8 lanes per
//    128-B head row), scores kept in LDS, exact two-pass softmax (max, then exp / sum / P·V).
//  * tw_greedy_select: per batch row, argmax over the vocabulary of the fp32 view of the
//    logits with suppressed ids masked (bitmask; the begin-suppress set only at the first
//    generated step), finished rows forced to eos (= pad), token written to the id matrix and
//    to the next step's input vector, finished flag updated.  Ties resolve to the lowest id
//    (torch.argmax).
//  * tw_select_sample[_ts]: the same selection with the temperature-fallback extensions of HF
//    generate_with_fallback (generation_whisper.py:970-1090): sampling at temperature T by the
//    Gumbel-max trick over the processed row (argmax of x/T + G, G = -log(-log U), U from a
//    counter-based hash of (seed, row, column, id): distributed as multinomial(softmax(x/T)),
//    not torch's RNG stream), and the running sum of log-softmax(processed row)[chosen] that
//    _retrieve_avg_logprobs computes (scores * T undoes the temperature warper).  T and the
//    seed live in a device control word, so one captured decode graph serves every fallback
//    temperature.  tw_select_sample[_ts]_lp (the LP instantiations) also store that log-prob at the token's
//    column of a per-token matrix (generate(return_token_logprobs=True)); tw_spec_accept_lp does so for the
//    accepted columns of an assisted round.
//  * tw_token_logprob: log-softmax of a raw logits row at one id (WhisperNoSpeechDetection).
#include "common.h"
#include "decode_impl.h"

#include <algorithm>
#include <cstdlib>

namespace {

using namespace twd;

// U = loads in flight per lane, K/V streamed with nontemporal loads (round 4, tools/bench_decode_attn.py, same box,
// profiles/r04_uv_decode_attn_ab.log): at the c4 shape (fp16, 512 clips x 20 heads over 1500 frames) U = 4 plain
// 665 us, U = 4 nontemporal 620, U = 2 nontemporal 609 (6.45 TB/s), U = 8 782 (occupancy); at 128 x 20 pairs
// U = 4 nontemporal 168 vs U = 2 190 -- hence U = 2 from DA_BIG pairs.
template <typename E, int U, bool KS>
__device__ __forceinline__ void decode_attn_pair(const DecP& p) {
  const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int tk = eff_tk(p);
  decode_attn_body<E, U, true>(p, b, h, KS ? clamp_start(p.k_start, b, tk) : 0, tk, nullptr);
}
template <typename E, bool KS>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_u4_kernel(DecP p) { decode_attn_pair<E, 4, KS>(p); }
template <typename E, bool KS>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_u2_kernel(DecP p) { decode_attn_pair<E, 2, KS>(p); }

// split over keys (few (clip, head) pairs: batch-1 long-form): blockIdx.y = chunk of S keys; a chunk past the
// effective Tk or wholly below the row's start stores an empty partial, the chunk the start falls into begins
// there; decode_attn_combine_kernel merges them.
// (Tried, r02: the last-arriving chunk combining in place -- agent-scope release + arrival counter --
// saves the second launch at batch 1 (14.6 -> 13.7 us) but every workgroup's release writes back the
// whole L2: 27 -> 202 us at B = 16, and c5 measured no faster.  Two launches it is.)
template <typename E, bool KS>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_split_kernel(DecP p, int S, float* ws) {
  const int bh = blockIdx.x, c = blockIdx.y;
  const int b = bh / p.H, h = bh % p.H;
  const int tk = eff_tk(p);
  float* part = ws + ((int64_t)bh * gridDim.y + c) * 66;
  const int lo = KS ? max(c * S, clamp_start(p.k_start, b, tk)) : c * S, hi = min(tk, c * S + S);
  if (lo >= hi) {
    store_empty_partial(part);
    return;
  }
  decode_attn_body<E>(p, b, h, lo, hi, part);
}

template <typename E>
__global__ __launch_bounds__(64) void decode_attn_combine_kernel(DecP p, int nchunk, const float* ws) {
  combine_row<E>(p, blockIdx.x, nchunk, ws + (int64_t)blockIdx.x * nchunk * 66);
}

// Multi-query decode attention (tw_decode_attn_mq: the verify pass of assisted decoding).  nq <= QN query rows per
// (clip, head); query j attends keys [start_j, tk_j), tk_j = Tk (+ *tk_dev) (+ j when causal), start_j the row's
// k_start clamped into [0, tk_j - 1] (clamp_start).  The queries that share a start -- all of them
// unless the start reaches a query's limit -- go through decode_attn_body_mq together (each K / V row loaded once);
// a query whose clamped start differs walks the keys from its own start, as its single-query call does, in a
// pass of its own.
// (MqP and mq_group: decode_impl.h)
template <typename E, int QN>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_mq_kernel(DecP p, MqP q) {
  __shared__ float sc[DA_MQ_LDS];
  constexpr int cap = DA_MQ_LDS / QN > DA_MAX_TK ? DA_MAX_TK : DA_MQ_LDS / QN;
  const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int tk0 = eff_tk(p);
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
    decode_attn_body_mq<E, QN, 4, true>(p, q.sqq, q.soq, b, h, glo, ghi, sc, cap, nullptr, 0);
    if (pend) __syncthreads();
  }
}

// split over keys: blockIdx.y = chunk of DA_SPLIT keys; query j's partials at ws + ((bh * nq + j) * nchunk + c) * 66
template <typename E, int QN>
__global__ __launch_bounds__(DA_THREADS) void decode_attn_mq_split_kernel(DecP p, MqP q, float* ws) {
  __shared__ float sc[QN * DA_SPLIT];
  const int bh = blockIdx.x, c = blockIdx.y, nchunk = gridDim.y;
  const int b = bh / p.H, h = bh % p.H;
  float* part = ws + (((int64_t)bh * q.nq) * nchunk + c) * 66;
  const int64_t pstride = (int64_t)nchunk * 66;
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
    decode_attn_body_mq<E, QN>(p, q.sqq, q.soq, b, h, glo, ghi, sc, DA_SPLIT, part, pstride);
    if (pend) __syncthreads();
  }
}

template <typename E>
__global__ __launch_bounds__(64) void decode_attn_mq_combine_kernel(DecP p, MqP q, int nchunk, const float* ws) {
  const int j = blockIdx.x % q.nq, bh = blockIdx.x / q.nq;
  p.o = (E*)p.o + j * q.soq;
  combine_row<E>(p, bh, nchunk, ws + (int64_t)blockIdx.x * nchunk * 66);
}

// Acceptance and rollback of one round of assisted decoding, one row, one wave (tw_spec_accept in tw_hip.h).
struct AccP {
  const int64_t* drafts; int k;
  int64_t* ids; int t_cap; int64_t eos;
  int* t_dev; int* t_dev_a;
  int64_t* cur; int64_t* cur_a;
  uint8_t* done; uint8_t* done_a; uint8_t* done_snap;
  int* last_ts; int* last_ts_a; int begin_col, ts_begin;
  float* slots; float* sum_logp;
  int* hist; int hist_cap;
  float* tok_logp;            // nullable: the row of the per-token log-prob matrix (tw_spec_accept_lp)
};
__global__ __launch_bounds__(64) void spec_accept_kernel(AccP a) {
  const int lane = threadIdx.x;
  const int t = *a.t_dev;
  const bool was_done = a.done_snap[0] != 0;
  const bool frozen = was_done || t + 1 >= a.t_cap;
  // n: leading drafts equal to the target's token at the same column, counted up to and including the first eos
  int n = 0;
  for (int j = 0; j < a.k; ++j) {
    const int64_t g = a.ids[t + 1 + j];
    if (g != a.drafts[j]) break;
    ++n;
    if (g == a.eos) break;
  }
  const int adv = frozen ? 0 : min(n + 1, a.t_cap - 1 - t);     // accepted target tokens: columns t+1 .. t+adv
  bool fin = was_done;
  for (int j = 1; j <= adv; ++j) fin = fin || a.ids[t + j] == a.eos;
  const int64_t cur = a.ids[t + adv];
  float s = 0.f;
  if (a.sum_logp) {
    s = a.sum_logp[0];
    for (int j = 0; j < adv; ++j) s += a.slots[j];              // position order: the sequential decode's additions
  }
  // last timestamp among the accepted generated columns [begin_col, t + adv], scanned backwards 64 columns a step
  int lts = -1;
  if (a.last_ts) {
    for (int c0 = t + adv; c0 >= a.begin_col; c0 -= 64) {
      const int c = c0 - lane;
      const bool is_ts = c >= a.begin_col && a.ids[c] >= a.ts_begin;
      const unsigned long long hit = __ballot(is_ts);
      if (hit) {
        lts = (int)a.ids[c0 - (__ffsll((long long)hit) - 1)];
        break;
      }
    }
  }
  // column t + lane of the per-token matrix: the accepted slot, 0 at the columns rolled back
  const float tlp = (a.tok_logp && lane >= 1 && lane <= adv) ? a.slots[lane - 1] : 0.f;
  __syncthreads();                                              // every read above precedes the stores below
  if (lane > adv && lane <= a.k + 1) a.ids[t + lane] = a.eos;   // columns past t + adv back to the eos fill
  if (a.tok_logp && lane >= 1 && lane <= a.k + 1) a.tok_logp[t + lane] = tlp;
  if (a.slots && lane <= a.k) a.slots[lane] = 0.f;
  if (lane != 0) return;
  *a.t_dev = t + adv;
  if (a.t_dev_a) *a.t_dev_a = t + adv;
  a.cur[0] = cur;
  if (a.cur_a) a.cur_a[0] = cur;
  const uint8_t d = fin ? 1 : 0;
  a.done[0] = d;
  a.done_snap[0] = d;
  if (a.done_a) a.done_a[0] = d;
  if (a.last_ts) {
    a.last_ts[0] = lts;
    if (a.last_ts_a) a.last_ts_a[0] = lts;
  }
  if (a.sum_logp) a.sum_logp[0] = s;
  if (a.hist && !frozen) {
    const int r = a.hist[0];
    if (r + 1 < a.hist_cap) a.hist[1 + r] = n;
    a.hist[0] = r + 1;
  }
}

// x[j] = tok[ids[j]] + pos[min(*t_dev + j, npos - 1)]: the Q consecutive positions of one row's verify pass (a round
// that reaches past the last position embeds its surplus rows at the last one; their tokens are discarded)
__global__ void embed_step_multi_kernel(const int64_t* __restrict__ ids, const void* __restrict__ tok, int tok_dtype,
                                        const void* __restrict__ pos, int pos_dtype, void* __restrict__ out,
                                        int out_dtype, int D, const int* __restrict__ t_dev, int npos) {
  const int j = blockIdx.x;
  const int64_t id = ids[j];
  const int64_t t = min(*t_dev + j, npos - 1);
  for (int e = threadIdx.x; e < D; e += blockDim.x) {
    const float s = ld_as_f32(tok, tok_dtype, id * D + e) + ld_as_f32(pos, pos_dtype, t * D + e);
    st_from_f32(out, out_dtype, (int64_t)j * D + e, s);
  }
}

struct SelP {
  const void* logits; int64_t ld;
  int V;
  const uint32_t* suppress;   // V-bit mask (nullable)
  const uint32_t* begin;      // V-bit mask applied when apply_begin (nullable)
  int apply_begin;
  int64_t eos;
  uint8_t* done;
  int64_t* ids; int64_t ld_ids; int col;
  int64_t* next;              // [B] next-step input ids
  const int* t_dev;           // nullable: col = *t_dev + col, begin mask applied when col == begin_col
  int begin_col;
  const uint32_t* ctl;        // nullable: per row b, ctl[3b] = bits of 1/T (0: greedy), ctl[3b+1], [3b+2] = seed lo, hi
  float* sum_logp;            // nullable: += log-prob of the chosen token while the row is live
  float* tok_logp;            // nullable, read by the LP instantiations only: [b*ld_lp + col] = that log-prob (0 for a
  int64_t ld_lp;              // row already finished)
  int vec;                    // rows 16-B aligned and padded to a multiple of 8 ids: 16-B loads
};

// f(v, x, suppressed, begin_suppressed) over this thread's ids of a logits row: chunks of 8
// consecutive ids (one 16-B load, one word of each mask), chunk c = tid, tid + 256, ...
template <typename E, class F>
__device__ __forceinline__ void for_row(const SelP& p, const E* row, F&& f, int lo = 0, int hi = -1) {
  if (hi < 0) hi = p.V;                                  // [lo, hi), lo a multiple of 8
  for (int v0 = lo + (int)threadIdx.x * 8; v0 < hi; v0 += 256 * 8) {
    float xs[8];
    if (p.vec) {
      load8(row + v0, xs);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) xs[j] = v0 + j < p.V ? to_f32(row[v0 + j]) : -INFINITY;
    }
    const uint32_t ws = p.suppress ? p.suppress[v0 >> 5] >> (v0 & 31) : 0u;   // 8 ids never straddle a word
    const uint32_t wb = p.begin ? p.begin[v0 >> 5] >> (v0 & 31) : 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (v0 + j < hi) f(v0 + j, xs[j], ((ws >> j) & 1u) != 0u, ((wb >> j) & 1u) != 0u);
  }
}

// (max, sum exp(x - max)) pairs: running logsumexp
__device__ __forceinline__ void lse_add(float& m, float& s, float x) {
  if (x > m) { s = s * __expf(m - x) + 1.f; m = x; }
  else s += __expf(x - m);
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float mx = fmaxf(m, om);
  s = (mx == -INFINITY) ? 0.f : s * __expf(m - mx) + os * __expf(om - mx);
  m = mx;
}
__device__ __forceinline__ float lse_val(float m, float s) { return m == -INFINITY ? -INFINITY : m + __logf(s); }

// Gumbel(0,1) noise of token v at (row b, column col): splitmix64 of a distinct 64-bit key
// (b, col, v < 2^21 each) -> 24-bit uniform in (0, 1)
__device__ __forceinline__ float gumbel(uint64_t seed, int b, int col, int v) {
  uint64_t x = seed + 0x9E3779B97F4A7C15ull *
                          ((((uint64_t)(uint32_t)b) << 42) ^ (((uint64_t)(uint32_t)col) << 21) ^ (uint64_t)(uint32_t)v);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  const float u = ((float)(x >> 40) + 0.5f) * (1.0f / 16777216.0f);
  return -__logf(-__logf(u));
}

// row b's sampling control: its own temperature and seed, so the rows of one batch can be independent fallback
// attempts (each row's draw keyed by (its seed, column, id) only: a row decodes the same tokens whatever batch
// it runs in)
__device__ __forceinline__ void read_ctl(const uint32_t* ctl, int b, float& inv_t, uint64_t& seed) {
  inv_t = ctl ? __uint_as_float(ctl[3 * b]) : 0.f;
  seed = ctl ? ((uint64_t)ctl[3 * b + 2] << 32 | ctl[3 * b + 1]) : 0ull;
}

// block (256 threads) argmax with lowest-id ties, result broadcast to thread 0's registers
__device__ __forceinline__ void block_argmax(float& v, int& i, float (*sv)[4], int (*si)[4], int slot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  if (lane == 0) { sv[slot][wave] = v; si[slot][wave] = i; }
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 4; ++w)
      if (sv[slot][w] > v || (sv[slot][w] == v && si[slot][w] < i)) { v = sv[slot][w]; i = si[slot][w]; }
}
__device__ __forceinline__ void block_lse(float& m, float& s, float (*sv)[4], int slot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  if (lane == 0) { sv[slot][wave] = m; sv[slot + 1][wave] = s; }
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 4; ++w) lse_merge(m, s, sv[slot][w], sv[slot + 1][w]);
}

__device__ __forceinline__ bool bit(const uint32_t* m, int v) { return m && ((m[v >> 5] >> (v & 31)) & 1u); }

// LP: the instantiations behind tw_select_sample[_ts]_lp, which also keep the step's log-prob per column (tok_logp).
// Whether the scan gathers the row's logsumexp, and the owner thread's bookkeeping of the chosen token's log-prob
// (lp() computes it): the value added to the running sum while the row is live is the value stored at the column.
template <bool LP>
__device__ __forceinline__ bool sel_lse(const SelP& p) {
  return p.sum_logp != nullptr || (LP && p.tok_logp != nullptr);
}
template <bool LP, class F>
__device__ __forceinline__ void sel_logp(const SelP& p, int b, bool fin, F&& lp) {
  if (LP ? !sel_lse<true>(p) : (!p.sum_logp || fin)) return;
  const float x = fin ? 0.f : lp();
  if (p.sum_logp && !fin) p.sum_logp[b] += x;
  if (LP && p.tok_logp) p.tok_logp[b * p.ld_lp + p.col] = x;
}

// Selection over a row is split into scan (per-thread accumulation over a slice of the vocabulary),
// block reduction, and finish (thread 0: merge, pick, bookkeeping).  Few rows (batch-1 long-form): the
// row is cut into G slices, one workgroup each, partials to the per-device scratch block, and a second
// kernel merges them in slice order and finishes -- one 256-thread workgroup per row scanning 51 865
// logits took ~78 us per step; many rows: one workgroup per row does all three.
struct GreedyAcc {
  float best, sbest, m, se;
  int besti, sbesti;
};
constexpr int SEL_WORDS = 8;     // words per partial in the scratch block

__device__ __forceinline__ void greedy_init(GreedyAcc& a) {
  a.best = a.sbest = a.m = -INFINITY;
  a.se = 0.f;
  a.besti = a.sbesti = 0x7fffffff;
}
__device__ __forceinline__ void greedy_merge(GreedyAcc& a, const GreedyAcc& o, bool sample, bool lse) {
  if (o.best > a.best || (o.best == a.best && o.besti < a.besti)) { a.best = o.best; a.besti = o.besti; }
  if (sample && (o.sbest > a.sbest || (o.sbest == a.sbest && o.sbesti < a.sbesti))) { a.sbest = o.sbest; a.sbesti = o.sbesti; }
  if (lse) lse_merge(a.m, a.se, o.m, o.se);
}
template <bool LP, typename E>
__device__ __forceinline__ void greedy_scan(const SelP& p, const E* row, int b, bool sample, float inv_t, uint64_t seed,
                                            GreedyAcc& a, int lo, int hi) {
  const bool lse = sel_lse<LP>(p);
  for_row(p, row, [&](int v, float x, bool sup, bool beg) {
    if (sup || (p.apply_begin && beg)) x = -INFINITY;
    if (x > a.best || (x == a.best && v < a.besti)) { a.best = x; a.besti = v; }
    if (x > -INFINITY) {
      if (lse) lse_add(a.m, a.se, x);
      if (sample) {
        const float g = x * inv_t + gumbel(seed, 0, p.col, v);
        if (g > a.sbest || (g == a.sbest && v < a.sbesti)) { a.sbest = g; a.sbesti = v; }
      }
    }
  }, lo, hi);
}
// block reduction: the result in thread 0's a
__device__ __forceinline__ void greedy_block(GreedyAcc& a, bool sample, bool lse, float (*sv)[4], int (*si)[4]) {
  block_argmax(a.best, a.besti, sv, si, 0);
  if (sample) block_argmax(a.sbest, a.sbesti, sv, si, 1);
  if (lse) block_lse(a.m, a.se, sv, 2);
}
template <bool LP, typename E>
__device__ __forceinline__ void greedy_finish(const SelP& p, const E* row, int b, const GreedyAcc& a, bool sample) {
  int pick = sample ? a.sbesti : a.besti;
  if (pick == 0x7fffffff) pick = 0;              // every logit masked / NaN: id 0 (torch argmax of all -inf)
  const bool fin = p.done[b] != 0;
  const int64_t tok = fin ? p.eos : (int64_t)pick;
  p.ids[b * p.ld_ids + p.col] = tok;
  p.next[b] = tok;
  p.done[b] = (fin || tok == p.eos) ? 1 : 0;
  sel_logp<LP>(p, b, fin, [&] { return to_f32(row[pick]) - lse_val(a.m, a.se); });
}
__device__ __forceinline__ void sel_prologue(SelP& p) {
  if (p.t_dev) {
    p.col += *p.t_dev;
    p.apply_begin = p.col == p.begin_col;
  }
}

// grid (G, B): G == 1 -> scan the whole row and finish; G > 1 -> partial of slice blockIdx.x into ws
template <typename E, bool LP>
__global__ __launch_bounds__(256) void greedy_select_kernel(SelP p, int slice, float* ws) {
  __shared__ float sv[4][4];
  __shared__ int si[4][4];
  const int g = blockIdx.x, G = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
  sel_prologue(p);
  float inv_t;
  uint64_t seed;
  read_ctl(p.ctl, b, inv_t, seed);
  const bool sample = inv_t > 0.f, lse = sel_lse<LP>(p);
  const E* row = (const E*)p.logits + b * p.ld;
  GreedyAcc a;
  greedy_init(a);
  const int lo = G == 1 ? 0 : g * slice, hi = G == 1 ? p.V : min(p.V, lo + slice);
  greedy_scan<LP>(p, row, b, sample, inv_t, seed, a, lo, hi);
  greedy_block(a, sample, lse, sv, si);
  if (tid != 0) return;
  if (G == 1) {
    greedy_finish<LP>(p, row, b, a, sample);
  } else {
    float* w = ws + ((int64_t)b * G + g) * SEL_WORDS;
    w[0] = a.best; w[1] = a.sbest; w[2] = a.m; w[3] = a.se;
    w[4] = __int_as_float(a.besti); w[5] = __int_as_float(a.sbesti);
  }
}

template <typename E, bool LP>
__global__ __launch_bounds__(64) void greedy_merge_kernel(SelP p, int G, const float* ws) {
  const int b = blockIdx.x;
  if (threadIdx.x != 0) return;
  sel_prologue(p);
  float inv_t;
  uint64_t seed;
  read_ctl(p.ctl, b, inv_t, seed);
  const bool sample = inv_t > 0.f, lse = sel_lse<LP>(p);
  GreedyAcc a;
  greedy_init(a);
  for (int g = 0; g < G; ++g) {
    const float* w = ws + ((int64_t)b * G + g) * SEL_WORDS;
    GreedyAcc o;
    o.best = w[0]; o.sbest = w[1]; o.m = w[2]; o.se = w[3];
    o.besti = __float_as_int(w[4]); o.sbesti = __float_as_int(w[5]);
    greedy_merge(a, o, sample, lse);
  }
  greedy_finish<LP>(p, (const E*)p.logits + b * p.ld, b, a, sample);
}


// Timestamp decoding (HF WhisperTimeStampLogitsProcessor, applied after the suppress processors):
// <|notimestamps|> masked; timestamps in pairs (after ts,ts -> text; after text,ts -> ts or eos);
// timestamps non-decreasing (none below the last one, or below last+1 unless closing a pair);
// at the window's first step only timestamps <= ts_begin + max_initial; and when the probability
// mass of all timestamps exceeds the best text token (logsumexp over timestamps > max text logit,
// the log_softmax shift cancels) only timestamps are eligible.  One pass per row gathers the
// text argmax, the timestamp argmax and the timestamp logsumexp; last_ts[b] keeps the row's last
// emitted timestamp (-1: none in this window).
struct SelTsP {
  SelP s;
  int begin_col;              // first generated column of the window
  int ts_begin, no_ts, max_initial;
  int* last_ts;
};

struct TsAcc {
  float bt, bs, se, tm, tse;      // best text, best timestamp, sum exp(ts - bs), text logsumexp (m, s)
  int it, is;
};
__device__ __forceinline__ void ts_init(TsAcc& a) {
  a.bt = a.bs = a.tm = -INFINITY;
  a.se = a.tse = 0.f;
  a.it = a.is = 0x7fffffff;
}
__device__ __forceinline__ void ts_merge(TsAcc& a, const TsAcc& o, bool lse) {
  if (o.bt > a.bt || (o.bt == a.bt && o.it < a.it)) { a.bt = o.bt; a.it = o.it; }
  const float mx = fmaxf(a.bs, o.bs);
  const float ns = (mx == -INFINITY) ? 0.f : a.se * __expf(a.bs - mx) + o.se * __expf(o.bs - mx);
  if (o.bs > a.bs || (o.bs == a.bs && o.is < a.is)) a.is = o.is;
  a.bs = mx;
  a.se = ns;
  if (lse) lse_merge(a.tm, a.tse, o.tm, o.tse);
}
// the row's timestamp-rule state at column p.col
struct TsRow {
  bool first, last_ts, pen_ts;
  int lim, ts_hi;
};
__device__ __forceinline__ TsRow ts_row(const SelTsP& q, int b) {
  const SelP& p = q.s;
  TsRow r;
  r.first = p.col == q.begin_col;
  const int64_t* idr = p.ids + b * p.ld_ids;
  const bool has1 = p.col - 1 >= q.begin_col, has2 = p.col - 2 >= q.begin_col;
  r.last_ts = has1 && idr[p.col - 1] >= q.ts_begin;
  r.pen_ts = !has2 || idr[p.col - 2] >= q.ts_begin;
  const int lt = q.last_ts[b];
  r.lim = lt < 0 ? q.ts_begin : ((r.last_ts && !r.pen_ts) ? lt : lt + 1);
  r.ts_hi = (r.first && q.max_initial >= 0) ? q.ts_begin + q.max_initial : 0x7fffffff;
  return r;
}
// eligibility of id v before the "timestamp mass wins" rule
__device__ __forceinline__ bool ts_masked(const SelTsP& q, const TsRow& r, int v, bool sup, bool beg) {
  bool m = sup || (r.first && beg) || v == q.no_ts;
  if (v >= q.ts_begin) {
    if (r.last_ts && r.pen_ts) m = true;
    if (v < r.lim || v > r.ts_hi) m = true;
  } else if ((r.last_ts && !r.pen_ts && v < q.s.eos) || r.first) {
    m = true;
  }
  return m;
}
template <bool LP, typename E>
__device__ __forceinline__ void ts_scan(const SelTsP& q, const TsRow& r, const E* row, TsAcc& a, int lo, int hi) {
  const bool lse = sel_lse<LP>(q.s);
  for_row(q.s, row, [&](int v, float x, bool sup, bool beg) {
    if (ts_masked(q, r, v, sup, beg) || !(x > -INFINITY)) return;
    if (v >= q.ts_begin) {
      if (x > a.bs) { a.se = a.se * __expf(a.bs - x) + 1.f; a.bs = x; a.is = v; }
      else { a.se += __expf(x - a.bs); if (x == a.bs && v < a.is) a.is = v; }
    } else {
      if (x > a.bt || (x == a.bt && v < a.it)) { a.bt = x; a.it = v; }
      if (lse) lse_add(a.tm, a.tse, x);
    }
  }, lo, hi);
}
// block reduction (waves by shuffles, then thread 0 over the 4 waves): the result in thread 0's a
__device__ __forceinline__ void ts_block(TsAcc& a, bool lse, float (*sv)[8], int (*si)[2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    TsAcc x;
    x.bt = __shfl_xor(a.bt, o, 64); x.bs = __shfl_xor(a.bs, o, 64); x.se = __shfl_xor(a.se, o, 64);
    x.tm = __shfl_xor(a.tm, o, 64); x.tse = __shfl_xor(a.tse, o, 64);
    x.it = __shfl_xor(a.it, o, 64); x.is = __shfl_xor(a.is, o, 64);
    ts_merge(a, x, lse);
  }
  if (lane == 0) {
    sv[wave][0] = a.bt; sv[wave][1] = a.bs; sv[wave][2] = a.se; sv[wave][3] = a.tm; sv[wave][4] = a.tse;
    si[wave][0] = a.it; si[wave][1] = a.is;
  }
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 4; ++w) {
      TsAcc x;
      x.bt = sv[w][0]; x.bs = sv[w][1]; x.se = sv[w][2]; x.tm = sv[w][3]; x.tse = sv[w][4];
      x.it = si[w][0]; x.is = si[w][1];
      ts_merge(a, x, lse);
    }
}
// finish (whole workgroup; the merged accumulator in thread 0's a): the timestamp-mass rule, the
// temperature-sampling pass over the processed row (Gumbel-max) when T > 0, the pick and bookkeeping
template <typename E, bool LP>
__device__ __forceinline__ void ts_finish(const SelTsP& q, const TsRow& r, int b, TsAcc& a, float (*sx)[4],
                                          int (*sxi)[4]) {
  __shared__ int s_mask_text;
  const SelP& p = q.s;
  const int tid = threadIdx.x;
  float inv_t;
  uint64_t seed;
  read_ctl(p.ctl, b, inv_t, seed);
  const bool sample = inv_t > 0.f;
  const E* row = (const E*)p.logits + b * p.ld;
  if (tid == 0) {
    const float ts_lse = a.bs == -INFINITY ? -INFINITY : a.bs + __logf(a.se);
    s_mask_text = (a.bs > -INFINITY && ts_lse > a.bt) ? 1 : 0;   // timestamp mass wins: text masked
  }
  __syncthreads();
  const bool mask_text = s_mask_text != 0;
  int spick = 0x7fffffff;
  if (sample) {                                          // second pass: Gumbel-max over the processed row
    float sb = -INFINITY;
    for_row(p, row, [&](int v, float x, bool sup, bool beg) {
      if (ts_masked(q, r, v, sup, beg) || !(x > -INFINITY) || (mask_text && v < q.ts_begin)) return;
      const float g = x * inv_t + gumbel(seed, 0, p.col, v);
      if (g > sb || (g == sb && v < spick)) { sb = g; spick = v; }
    });
    block_argmax(sb, spick, sx, sxi, 2);
  }
  if (tid == 0) {
    const float ts_l = lse_val(a.bs, a.se);
    int best;
    if (mask_text) best = a.is;
    else if (a.bt >= a.bs && a.it != 0x7fffffff) best = a.it;       // text ids < timestamp ids: ties -> text
    else if (a.is != 0x7fffffff) best = a.is;
    else best = 0;
    if (sample) best = spick == 0x7fffffff ? best : spick;
    const bool fin = p.done[b] != 0;
    const int64_t tok = fin ? p.eos : (int64_t)best;
    p.ids[b * p.ld_ids + p.col] = tok;
    p.next[b] = tok;
    p.done[b] = (fin || tok == p.eos) ? 1 : 0;
    if (!fin && tok >= q.ts_begin) q.last_ts[b] = (int)tok;
    sel_logp<LP>(p, b, fin, [&] {
      float lse = ts_l;
      if (!mask_text) {
        float m = a.tm, ss = a.tse;
        if (a.bs > -INFINITY) lse_merge(m, ss, a.bs, a.se);
        lse = lse_val(m, ss);
      }
      return to_f32(row[best]) - lse;
    });
  }
}

// grid (G, B): G == 1 -> whole row + finish; G > 1 -> partial of slice blockIdx.x into ws
template <typename E, bool LP>
__global__ __launch_bounds__(256) void greedy_select_ts_kernel(SelTsP q, int slice, float* ws) {
  __shared__ float sv[4][8];
  __shared__ int si[4][2];
  __shared__ float sx[4][4];
  __shared__ int sxi[4][4];
  const int g = blockIdx.x, G = gridDim.x, b = blockIdx.y;
  if (q.s.t_dev) q.s.col += *q.s.t_dev;
  const TsRow r = ts_row(q, b);
  const bool lse = sel_lse<LP>(q.s);
  const E* row = (const E*)q.s.logits + b * q.s.ld;
  TsAcc a;
  ts_init(a);
  const int lo = G == 1 ? 0 : g * slice, hi = G == 1 ? q.s.V : min(q.s.V, lo + slice);
  ts_scan<LP>(q, r, row, a, lo, hi);
  ts_block(a, lse, sv, si);
  if (G == 1) {
    ts_finish<E, LP>(q, r, b, a, sx, sxi);
  } else if (threadIdx.x == 0) {
    float* w = ws + ((int64_t)b * G + g) * SEL_WORDS;
    w[0] = a.bt; w[1] = a.bs; w[2] = a.se; w[3] = a.tm; w[4] = a.tse;
    w[5] = __int_as_float(a.it); w[6] = __int_as_float(a.is);
  }
}

template <typename E, bool LP>
__global__ __launch_bounds__(256) void ts_merge_kernel(SelTsP q, int G, const float* ws) {
  __shared__ float sx[4][4];
  __shared__ int sxi[4][4];
  const int b = blockIdx.x;
  if (q.s.t_dev) q.s.col += *q.s.t_dev;
  const TsRow r = ts_row(q, b);
  const bool lse = sel_lse<LP>(q.s);
  TsAcc a;
  ts_init(a);
  if (threadIdx.x == 0)
    for (int g = 0; g < G; ++g) {
      const float* w = ws + ((int64_t)b * G + g) * SEL_WORDS;
      TsAcc o;
      o.bt = w[0]; o.bs = w[1]; o.se = w[2]; o.tm = w[3]; o.tse = w[4];
      o.it = __float_as_int(w[5]); o.is = __float_as_int(w[6]);
      ts_merge(a, o, lse);
    }
  ts_finish<E, LP>(q, r, b, a, sx, sxi);
}

// out[b] = log_softmax(logits[b, :V])[token]   (fp32 of the bf16 / fp32 row)
template <typename E>
__global__ __launch_bounds__(256) void token_logprob_kernel(const E* __restrict__ logits, int64_t ld, int V,
                                                            int token, float* __restrict__ out) {
  __shared__ float sv[4][4];
  const int b = blockIdx.x;
  const E* row = logits + b * ld;
  float m = -INFINITY, s = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) {
    const float x = to_f32(row[v]);
    if (x > -INFINITY) lse_add(m, s, x);
  }
  block_lse(m, s, sv, 0);
  if (threadIdx.x == 0) out[b] = to_f32(row[token]) - lse_val(m, s);
}

// x[b] = tok[ids[b]] + pos[*t_dev]   (decoder input embedding of step t, HF modeling_whisper.py:720-735)
__global__ void embed_step_kernel(const int64_t* __restrict__ ids, const void* __restrict__ tok, int tok_dtype,
                                  const void* __restrict__ pos, int pos_dtype, void* __restrict__ out, int out_dtype,
                                  int D, const int* __restrict__ t_dev) {
  const int b = blockIdx.x;
  const int64_t id = ids[b];
  const int64_t t = *t_dev;
  for (int e = threadIdx.x; e < D; e += blockDim.x) {
    const float s = ld_as_f32(tok, tok_dtype, id * D + e) + ld_as_f32(pos, pos_dtype, t * D + e);
    st_from_f32(out, out_dtype, (int64_t)b * D + e, s);
  }
}

// x[b] = tok[ids[b]] + pos[max(*t_dev - pos_off[b], 0)]: a row left-padded by pos_off[b] columns counts its positions
// from its first real token (the rule HF derives from an attention mask: (mask.cumsum(-1) - 1).clamp(min=0))
__global__ void embed_step_off_kernel(const int64_t* __restrict__ ids, const void* __restrict__ tok, int tok_dtype,
                                      const void* __restrict__ pos, int pos_dtype, void* __restrict__ out,
                                      int out_dtype, int D, const int* __restrict__ t_dev,
                                      const int* __restrict__ pos_off) {
  const int b = blockIdx.x;
  const int64_t id = ids[b];
  const int64_t t = max(*t_dev - pos_off[b], 0);
  for (int e = threadIdx.x; e < D; e += blockDim.x) {
    const float s = ld_as_f32(tok, tok_dtype, id * D + e) + ld_as_f32(pos, pos_dtype, t * D + e);
    st_from_f32(out, out_dtype, (int64_t)b * D + e, s);
  }
}

// cache[b][*t_dev][0:n] = src[b][0:n]   (16-B vectors: 8 bf16 or 4 fp32)
template <typename E>
__global__ void kv_append_kernel(const E* __restrict__ src, int64_t ld_src, E* __restrict__ cache,
                                 int64_t ld_row, int64_t sb, int n, const int* __restrict__ t_dev) {
  constexpr int W = 16 / sizeof(E);
  const int b = blockIdx.y;
  const int64_t t = *t_dev;
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) * W;
  if (i < n) *(f32x4*)(cache + b * sb + t * ld_row + i) = *(const f32x4*)(src + b * ld_src + i);
}

__global__ void step_advance_kernel(int* t_dev, int by) {
  if (threadIdx.x == 0) *t_dev += by;
}

// vector row loads when every row starts 16-B aligned and has room for the last 8-id chunk
int sel_vec(const void* logits, int64_t ld, int V) {
  return ((uintptr_t)logits % 16 == 0 && ld % 8 == 0 && ld >= (int64_t)((V + 7) / 8) * 8) ? 1 : 0;
}

// run the statement with E = the element type of a dtype code: TW_DISPATCH_DT(dt, hipLaunchKernelGGL(K<E>, ...))
#define TW_DISPATCH_DT(dt, ...)                              \
  do {                                                       \
    if ((dt) == TW_BF16) { using E = bf16; __VA_ARGS__; }    \
    else if ((dt) == TW_F16) { using E = f16; __VA_ARGS__; } \
    else if ((dt) == TW_F32) { using E = float; __VA_ARGS__; } \
    else return TW_EUNSUPPORTED;                             \
  } while (0)
// launch K<bf16>, K<f16> or K<float> by the dtype code
#define TW_LAUNCH_DT(dt, K, grid, block, ...) \
  TW_DISPATCH_DT(dt, hipLaunchKernelGGL(K<E>, grid, block, 0, stream, __VA_ARGS__))

// slices per row: enough workgroups to cover the chip for a handful of rows, one per row from 256 rows
// up; the slices are multiples of 8 ids (for_row's 16-B chunks)
int sel_slices(int B, int V) {
  int G = 1;
  while (G < 32 && (int64_t)B * G * 2 <= 512) G *= 2;
  const int slice = ((V + G - 1) / G + 7) / 8 * 8;
  return (V + slice - 1) / slice;
}

// the scan and merge kernels of the two selection families (plain / timestamp rules) and the merge's block size;
// LP: the instantiations that also store the per-token log-prob (the _lp entries with a tok_logp)
template <bool LP>
struct GreedyK {
  template <typename E> static constexpr auto scan = greedy_select_kernel<E, LP>;
  template <typename E> static constexpr auto merge = greedy_merge_kernel<E, LP>;
  static constexpr int merge_block = 64;
};
template <bool LP>
struct TsK {
  template <typename E> static constexpr auto scan = greedy_select_ts_kernel<E, LP>;
  template <typename E> static constexpr auto merge = ts_merge_kernel<E, LP>;
  static constexpr int merge_block = 256;
};
template <class K, class P>
int launch_select(const P& p, int B, int V, int logits_dtype, hipStream_t stream) {
  const int G = sel_slices(B, V);
  const int slice = ((V + G - 1) / G + 7) / 8 * 8;
  float* ws = G > 1 ? (float*)tw_device_workspace(stream, (size_t)B * G * SEL_WORDS * sizeof(float)) : nullptr;
  if (G > 1 && ws) {
    TW_LAUNCH_DT(logits_dtype, K::template scan, dim3(G, B), dim3(256), p, slice, ws);
    TW_LAUNCH_DT(logits_dtype, K::template merge, dim3(B), dim3(K::merge_block), p, G, ws);
  } else {
    TW_LAUNCH_DT(logits_dtype, K::template scan, dim3(1, B), dim3(256), p, V, (float*)nullptr);
  }
  TW_CHECK_LAUNCH();
  return TW_OK;
}

// the argument checks every selection entry point makes, and the SelP of the call
bool sel_bad(int64_t ld, int V, const uint8_t* done, const int64_t* ids, const int64_t* next_ids) {
  return V <= 0 || ld < V || !done || !ids || !next_ids;
}
SelP sel_fill(const void* logits, int64_t ld, int V, const uint32_t* suppress_bits, const uint32_t* begin_bits,
              int apply_begin, int64_t eos, uint8_t* done, int64_t* ids, int64_t ld_ids, int col, int64_t* next_ids,
              const int* t_dev, int begin_col, const uint32_t* ctl, float* sum_logp) {
  SelP p;
  p.logits = logits; p.ld = ld; p.V = V;
  p.suppress = suppress_bits; p.begin = begin_bits; p.apply_begin = apply_begin;
  p.eos = eos; p.done = done; p.ids = ids; p.ld_ids = ld_ids; p.col = col; p.next = next_ids;
  p.t_dev = t_dev; p.begin_col = begin_col;
  p.ctl = ctl; p.sum_logp = sum_logp; p.tok_logp = nullptr; p.ld_lp = 0; p.vec = sel_vec(logits, ld, V);
  return p;
}
// the checks the _lp entries add: something to track, and a row stride that holds the column when the host knows it
bool lp_bad(const float* sum_logp, const float* tok_logp, int64_t ld_lp, int col, const int* t_dev) {
  return (!sum_logp && !tok_logp) || (tok_logp && (ld_lp < 1 || col < 0 || (!t_dev && ld_lp <= col)));
}

// (dec_fill and dec_split: decode_impl.h)

// launch K<E, true> when the call has a per-row key start, K<E, false> when not
#define DEC_LAUNCH_KS(K, grid, ...)                                                                          \
  do {                                                                                                       \
    if (p.k_start) TW_DISPATCH_DT(dtype, hipLaunchKernelGGL((K<E, true>), grid, dim3(DA_THREADS), 0, stream, __VA_ARGS__));  \
    else TW_DISPATCH_DT(dtype, hipLaunchKernelGGL((K<E, false>), grid, dim3(DA_THREADS), 0, stream, __VA_ARGS__));           \
  } while (0)

// tw_decode_attn / _hs / _ks: k_start null for the first two
int decode_attn(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, int64_t hsk, const void* v,
                int64_t ldv, int64_t svb, int64_t hsv, void* o, int64_t sob, int B, int H, int Tk, const int* tk_dev,
                const int* k_start, int head_dim, float scale, int dtype, hipStream_t stream) {
  if (head_dim != 64) return TW_EUNSUPPORTED;
  if (B <= 0 || H <= 0) return TW_OK;
  DecP p;
  if (const int st = dec_fill(p, q, sqb, k, ldk, skb, hsk, v, ldv, svb, hsv, o, sob, H, Tk, Tk, tk_dev, k_start, scale))
    return st;
  // few (clip, head) pairs (batch-1 long-form, small batches): split the keys into chunks of DA_SPLIT over
  // the grid's y dimension, then combine.  Measured (tools/bench_decode_attn.py, H = 20, Tk = 1500): B = 1
  // 26.9 -> 14.6 us, B = 16 46.9 -> 31.2 us; from B = 64 (1280 pairs) the one-workgroup-per-pair kernel is
  // faster (90.6 vs 114.8 us).  With tk_dev (self-attention over a graph-captured cache) the host does
  // not know Tk, so the chunks would have to cover the kernel's DA_MAX_TK bound: measured on c5 (batch-1
  // long-form, Tk <= 448) that costs more than it saves (2.75 -> 2.93 ms per decode step), so only fixed-Tk calls
  // below 640 pairs split.
  const int nchunk = (Tk + DA_SPLIT - 1) / DA_SPLIT;
  if (dec_split(tk_dev, B * H, nchunk)) {
    float* ws = (float*)tw_device_workspace(stream, (size_t)B * H * nchunk * 66 * sizeof(float));
    if (ws) {
      DEC_LAUNCH_KS(decode_attn_split_kernel, dim3(B * H, nchunk), p, DA_SPLIT, ws);
      TW_LAUNCH_DT(dtype, decode_attn_combine_kernel, dim3(B * H), dim3(64), p, nchunk, ws);
      TW_CHECK_LAUNCH();
      return TW_OK;
    }
  }
  if (B * H >= DA_BIG) DEC_LAUNCH_KS(decode_attn_u2_kernel, dim3(B * H), p);
  else DEC_LAUNCH_KS(decode_attn_u4_kernel, dim3(B * H), p);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

template <int QN>
int launch_mq(const DecP& p, const MqP& q, int B, int nchunk, bool split, int dtype, hipStream_t stream) {
  float* ws = split ? (float*)tw_device_workspace(stream, (size_t)B * p.H * q.nq * nchunk * 66 * sizeof(float)) : nullptr;
  if (ws) {
    TW_DISPATCH_DT(dtype, hipLaunchKernelGGL((decode_attn_mq_split_kernel<E, QN>), dim3(B * p.H, nchunk),
                                             dim3(DA_THREADS), 0, stream, p, q, ws));
    TW_LAUNCH_DT(dtype, decode_attn_mq_combine_kernel, dim3(B * p.H * q.nq), dim3(64), p, q, nchunk, ws);
  } else {
    TW_DISPATCH_DT(dtype, hipLaunchKernelGGL((decode_attn_mq_kernel<E, QN>), dim3(B * p.H), dim3(DA_THREADS), 0,
                                             stream, p, q));
  }
  TW_CHECK_LAUNCH();
  return TW_OK;
}

}  // namespace

namespace {
// tw_greedy_select_ts (ctl, sum_logp null), tw_select_sample_ts (tok_logp null) and tw_select_sample_ts_lp
int select_ts(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
              const uint32_t* begin_bits, int64_t eos, uint8_t* done, int64_t* ids, int64_t ld_ids,
              int col, int64_t* next_ids, const int* t_dev, int begin_col, int ts_begin,
              int no_ts, int max_initial, int* last_ts, const uint32_t* ctl,
              float* sum_logp, float* tok_logp, int64_t ld_lp, hipStream_t stream) {
  if (sel_bad(ld, V, done, ids, next_ids) || !last_ts || ts_begin <= eos || ts_begin > V) return TW_EINVAL;
  SelTsP q;
  q.s = sel_fill(logits, ld, V, suppress_bits, begin_bits, 0, eos, done, ids, ld_ids, col, next_ids, t_dev, begin_col,
                 ctl, sum_logp);
  q.begin_col = begin_col; q.ts_begin = ts_begin; q.no_ts = no_ts; q.max_initial = max_initial; q.last_ts = last_ts;
  if (!tok_logp) return launch_select<TsK<false>>(q, B, V, logits_dtype, stream);
  q.s.tok_logp = tok_logp; q.s.ld_lp = ld_lp;
  return launch_select<TsK<true>>(q, B, V, logits_dtype, stream);
}
// tw_select_sample (tok_logp null) and tw_select_sample_lp
int select_plain(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                 const uint32_t* begin_bits, int apply_begin, int64_t eos, uint8_t* done, int64_t* ids, int64_t ld_ids,
                 int col, int64_t* next_ids, const int* t_dev, int begin_col, const uint32_t* ctl, float* sum_logp,
                 float* tok_logp, int64_t ld_lp, hipStream_t stream) {
  if (sel_bad(ld, V, done, ids, next_ids)) return TW_EINVAL;
  if (B >= (1 << 21) || V >= (1 << 21)) return TW_EUNSUPPORTED;     // RNG key widths
  SelP p = sel_fill(logits, ld, V, suppress_bits, begin_bits, apply_begin, eos, done, ids, ld_ids, col, next_ids, t_dev,
                    begin_col, ctl, sum_logp);
  if (!tok_logp) return launch_select<GreedyK<false>>(p, B, V, logits_dtype, stream);
  p.tok_logp = tok_logp; p.ld_lp = ld_lp;
  return launch_select<GreedyK<true>>(p, B, V, logits_dtype, stream);
}
}  // namespace

extern "C" int tw_greedy_select_ts(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                                   const uint32_t* begin_bits, int64_t eos, uint8_t* done, int64_t* ids, int64_t ld_ids,
                                   int col, int64_t* next_ids, const int* t_dev, int begin_col, int ts_begin,
                                   int no_ts, int max_initial, int* last_ts, hipStream_t stream) {
  if (B <= 0) return TW_OK;
  return select_ts(logits, ld, logits_dtype, B, V, suppress_bits, begin_bits, eos, done, ids, ld_ids, col, next_ids,
                   t_dev, begin_col, ts_begin, no_ts, max_initial, last_ts, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int tw_select_sample_ts(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                                   const uint32_t* begin_bits, int64_t eos, uint8_t* done, int64_t* ids, int64_t ld_ids,
                                   int col, int64_t* next_ids, const int* t_dev, int begin_col, int ts_begin,
                                   int no_ts, int max_initial, int* last_ts, const uint32_t* ctl, float* sum_logp,
                                   hipStream_t stream) {
  if (B <= 0) return TW_OK;
  if (B >= (1 << 21) || V >= (1 << 21)) return TW_EUNSUPPORTED;     // RNG key widths
  return select_ts(logits, ld, logits_dtype, B, V, suppress_bits, begin_bits, eos, done, ids, ld_ids, col, next_ids,
                   t_dev, begin_col, ts_begin, no_ts, max_initial, last_ts, ctl, sum_logp, nullptr, 0, stream);
}

extern "C" int tw_select_sample_ts_lp(const void* logits, int64_t ld, int logits_dtype, int B, int V,
                                      const uint32_t* suppress_bits, const uint32_t* begin_bits, int64_t eos,
                                      uint8_t* done, int64_t* ids, int64_t ld_ids, int col, int64_t* next_ids,
                                      const int* t_dev, int begin_col, int ts_begin, int no_ts, int max_initial,
                                      int* last_ts, const uint32_t* ctl, float* sum_logp, float* tok_logp,
                                      int64_t ld_lp, hipStream_t stream) {
  if (B <= 0) return TW_OK;
  if (lp_bad(sum_logp, tok_logp, ld_lp, col, t_dev)) return TW_EINVAL;
  if (B >= (1 << 21) || V >= (1 << 21)) return TW_EUNSUPPORTED;     // RNG key widths
  return select_ts(logits, ld, logits_dtype, B, V, suppress_bits, begin_bits, eos, done, ids, ld_ids, col, next_ids,
                   t_dev, begin_col, ts_begin, no_ts, max_initial, last_ts, ctl, sum_logp, tok_logp, ld_lp, stream);
}

extern "C" int tw_token_logprob(const void* logits, int64_t ld, int logits_dtype, int B, int V, int token,
                                float* out, hipStream_t stream) {
  if (B <= 0) return TW_OK;
  if (V <= 0 || ld < V || token < 0 || token >= V || !out) return TW_EINVAL;
  TW_LAUNCH_DT(logits_dtype, token_logprob_kernel, dim3(B), dim3(256), (const E*)logits, ld, V, token, out);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_embed_step(const int64_t* ids, const void* tok, int tok_dtype, const void* pos, int pos_dtype,
                             void* out, int out_dtype, int B, int D, const int* t_dev, hipStream_t stream) {
  if (B <= 0) return TW_OK;
  if (!t_dev || D <= 0) return TW_EINVAL;
  hipLaunchKernelGGL(embed_step_kernel, dim3(B), dim3(256), 0, stream, ids, tok, tok_dtype, pos, pos_dtype, out,
                     out_dtype, D, t_dev);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_embed_step_off(const int64_t* ids, const void* tok, int tok_dtype, const void* pos, int pos_dtype,
                                 void* out, int out_dtype, int B, int D, const int* t_dev, const int* pos_off,
                                 hipStream_t stream) {
  if (B <= 0) return TW_OK;
  if (!t_dev || !pos_off || D <= 0) return TW_EINVAL;
  hipLaunchKernelGGL(embed_step_off_kernel, dim3(B), dim3(256), 0, stream, ids, tok, tok_dtype, pos, pos_dtype, out,
                     out_dtype, D, t_dev, pos_off);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

// cross-attention K/V, row-interleaved [rows = B*Tk][ld] (k at columns 0..d, v at d..2d, head h at 64h..) ->
// head-major dst: K [B][H][Tk][64] then V [B][H][Tk][64] (one (clip, head) reads two contiguous Tk*64 runs)
template <typename E>
__global__ void kv_head_major_kernel(const E* __restrict__ src, int64_t ld, E* __restrict__ dst, int Tk, int H,
                                     int64_t rows) {
  constexpr int W = 16 / sizeof(E);
  const int d = H * 64, nv = 2 * d / W;                     // 16-B vectors per source row
  const int64_t total = rows * nv;
  const int64_t half = rows * d;                            // elements of the K part
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / nv;
    const int c = (int)(i - r * nv) * W;                    // source column
    const int part = c >= d, cc = c - part * d, h = cc >> 6, e = cc & 63;
    const int64_t b = r / Tk, t = r - b * Tk;
    const int4 v = *(const int4*)(src + r * ld + c);
    *(int4*)(dst + part * half + ((b * H + h) * Tk + t) * 64 + e) = v;
  }
}

extern "C" int tw_kv_head_major(const void* src, int64_t ld, void* dst, int B, int Tk, int H, int dtype,
                                hipStream_t stream) {
  if (B <= 0 || Tk <= 0 || H <= 0) return TW_OK;
  const int w = dtype == TW_F32 ? 3 : 7;
  if ((ld & w) || ld < 2 * 64 * H || (((uintptr_t)src | (uintptr_t)dst) & 15)) return TW_EINVAL;
  const int64_t rows = (int64_t)B * Tk;
  const int64_t nvec = rows * (2 * 64 * H) / (w + 1);
  const dim3 grid((unsigned)std::min<int64_t>((nvec + 255) / 256, 16384));
  // a copy: the 16-bit types move as bf16
  TW_LAUNCH_DT(dtype == TW_F16 ? TW_BF16 : dtype, kv_head_major_kernel, grid, dim3(256), (const E*)src, ld, (E*)dst, Tk,
               H, rows);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_kv_append(const void* src, int64_t ld_src, void* cache, int64_t ld_row, int64_t sb, int B, int n,
                            int dtype, const int* t_dev, hipStream_t stream) {
  if (B <= 0 || n <= 0) return TW_OK;
  const int w = dtype == TW_F32 ? 3 : 7;          // 16-B vectors: 4 fp32 / 8 bf16
  if (!t_dev || (n & w) || (ld_src & w) || (ld_row & w) || (sb & w) || (((uintptr_t)src | (uintptr_t)cache) & 15))
    return TW_EINVAL;
  // a copy: the 16-bit types move as bf16
  TW_LAUNCH_DT(dtype == TW_F16 ? TW_BF16 : dtype, kv_append_kernel, dim3((n / (w + 1) + 255) / 256, B), dim3(256),
               (const E*)src, ld_src, (E*)cache, ld_row, sb, n, t_dev);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_step_advance(int* t_dev, int by, hipStream_t stream) {
  if (!t_dev) return TW_EINVAL;
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, stream, t_dev, by);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_decode_attn_hs(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, int64_t hsk,
                                 const void* v, int64_t ldv, int64_t svb, int64_t hsv, void* o, int64_t sob, int B,
                                 int H, int Tk, const int* tk_dev, int head_dim, float scale, int dtype,
                                 hipStream_t stream) {
  return decode_attn(q, sqb, k, ldk, skb, hsk, v, ldv, svb, hsv, o, sob, B, H, Tk, tk_dev, nullptr, head_dim, scale,
                     dtype, stream);
}

extern "C" int tw_decode_attn(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, const void* v,
                              int64_t ldv, int64_t svb, void* o, int64_t sob, int B, int H, int Tk, const int* tk_dev,
                              int head_dim, float scale, int dtype, hipStream_t stream) {
  return decode_attn(q, sqb, k, ldk, skb, 64, v, ldv, svb, 64, o, sob, B, H, Tk, tk_dev, nullptr, head_dim, scale,
                     dtype, stream);
}

// tw_decode_attn_hs with a per-row key start: a call with every start 0 computes what tw_decode_attn_hs computes
extern "C" int tw_decode_attn_ks(const void* q, int64_t sqb, const void* k, int64_t ldk, int64_t skb, int64_t hsk,
                                 const void* v, int64_t ldv, int64_t svb, int64_t hsv, void* o, int64_t sob, int B,
                                 int H, int Tk, const int* tk_dev, const int* k_start, int head_dim, float scale,
                                 int dtype, hipStream_t stream) {
  if (!k_start && head_dim == 64 && B > 0 && H > 0) return TW_EINVAL;
  return decode_attn(q, sqb, k, ldk, skb, hsk, v, ldv, svb, hsv, o, sob, B, H, Tk, tk_dev, k_start, head_dim, scale,
                     dtype, stream);
}

// tw_decode_attn_ks for Q consecutive query rows per batch row: the same argument checks, the same split rule (the
// (row, head) pairs counted as for one step, the chunks from the last query's key count), the same bodies per query
extern "C" int tw_decode_attn_mq(const void* q, int64_t sqb, int64_t sqq, const void* k, int64_t ldk, int64_t skb,
                                 int64_t hsk, const void* v, int64_t ldv, int64_t svb, int64_t hsv, void* o,
                                 int64_t sob, int64_t soq, int B, int H, int Q, int Tk, const int* tk_dev,
                                 const int* k_start, int causal, int head_dim, float scale, int dtype,
                                 hipStream_t stream) {
  if (head_dim != 64) return TW_EUNSUPPORTED;
  if (Q < 1 || Q > DA_MQ) return TW_EINVAL;
  if (B <= 0 || H <= 0) return TW_OK;
  if (dtype != TW_BF16 && dtype != TW_F16 && dtype != TW_F32) return TW_EUNSUPPORTED;
  const int tk_last = Tk + (causal ? Q - 1 : 0);
  if (B * H >= DA_BIG) return TW_EUNSUPPORTED;
  DecP p;
  if (const int st = dec_fill(p, q, sqb, k, ldk, skb, hsk, v, ldv, svb, hsv, o, sob, H, Tk, tk_last, tk_dev, k_start,
                              scale))
    return st;
  if ((sqq & 7) || sqq < 0 || soq < 0) return TW_EINVAL;
  const int QN = Q <= 1 ? 1 : Q <= 2 ? 2 : Q <= 4 ? 4 : 8;
  const int nchunk = (tk_last + DA_SPLIT - 1) / DA_SPLIT;
  const bool split = dec_split(tk_dev, B * H, nchunk);
  // one-workgroup path: a query's scores live in DA_MQ_LDS / QN floats of LDS
  if (!split && !tk_dev && tk_last > DA_MQ_LDS / QN) return TW_EUNSUPPORTED;
  MqP m;
  m.sqq = sqq; m.soq = soq; m.nq = Q; m.causal = causal ? 1 : 0;
  switch (QN) {
    case 1: return launch_mq<1>(p, m, B, nchunk, split, dtype, stream);
    case 2: return launch_mq<2>(p, m, B, nchunk, split, dtype, stream);
    case 4: return launch_mq<4>(p, m, B, nchunk, split, dtype, stream);
    default: return launch_mq<8>(p, m, B, nchunk, split, dtype, stream);
  }
}

extern "C" int tw_spec_accept_lp(const int64_t* drafts, int k, int64_t* ids, int t_cap, int64_t eos, int* t_dev,
                                 int* t_dev_a, int64_t* cur, int64_t* cur_a, uint8_t* done, uint8_t* done_a,
                                 uint8_t* done_snap, int* last_ts, int* last_ts_a, int begin_col, int ts_begin,
                                 float* slots, float* sum_logp, float* tok_logp, int* hist, int hist_cap,
                                 hipStream_t stream) {
  if (k < 1 || k >= DA_MQ || !drafts || !ids || !t_dev || !cur || !done || !done_snap || t_cap < 1 || begin_col < 0)
    return TW_EINVAL;
  if ((sum_logp != nullptr) != (slots != nullptr) || (hist && hist_cap < 1) || (tok_logp && !slots)) return TW_EINVAL;
  AccP a;
  a.drafts = drafts; a.k = k; a.ids = ids; a.t_cap = t_cap; a.eos = eos;
  a.t_dev = t_dev; a.t_dev_a = t_dev_a; a.cur = cur; a.cur_a = cur_a;
  a.done = done; a.done_a = done_a; a.done_snap = done_snap;
  a.last_ts = last_ts; a.last_ts_a = last_ts_a; a.begin_col = begin_col; a.ts_begin = ts_begin;
  a.slots = slots; a.sum_logp = sum_logp; a.hist = hist; a.hist_cap = hist_cap; a.tok_logp = tok_logp;
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(64), 0, stream, a);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_spec_accept(const int64_t* drafts, int k, int64_t* ids, int t_cap, int64_t eos, int* t_dev,
                              int* t_dev_a, int64_t* cur, int64_t* cur_a, uint8_t* done, uint8_t* done_a,
                              uint8_t* done_snap, int* last_ts, int* last_ts_a, int begin_col, int ts_begin,
                              float* slots, float* sum_logp, int* hist, int hist_cap, hipStream_t stream) {
  return tw_spec_accept_lp(drafts, k, ids, t_cap, eos, t_dev, t_dev_a, cur, cur_a, done, done_a, done_snap, last_ts,
                           last_ts_a, begin_col, ts_begin, slots, sum_logp, nullptr, hist, hist_cap, stream);
}

extern "C" int tw_embed_step_multi(const int64_t* ids, const void* tok, int tok_dtype, const void* pos, int pos_dtype,
                                   void* out, int out_dtype, int Q, int D, const int* t_dev, int npos,
                                   hipStream_t stream) {
  if (Q <= 0) return TW_OK;
  if (!t_dev || D <= 0 || npos < 1) return TW_EINVAL;
  hipLaunchKernelGGL(embed_step_multi_kernel, dim3(Q), dim3(256), 0, stream, ids, tok, tok_dtype, pos, pos_dtype, out,
                     out_dtype, D, t_dev, npos);
  TW_CHECK_LAUNCH();
  return TW_OK;
}

extern "C" int tw_greedy_select(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                                const uint32_t* begin_bits, int apply_begin, int64_t eos, uint8_t* done, int64_t* ids,
                                int64_t ld_ids, int col, int64_t* next_ids, const int* t_dev, int begin_col,
                                hipStream_t stream) {
  if (B <= 0) return TW_OK;
  if (sel_bad(ld, V, done, ids, next_ids)) return TW_EINVAL;
  return launch_select<GreedyK<false>>(sel_fill(logits, ld, V, suppress_bits, begin_bits, apply_begin, eos, done, ids,
                                                ld_ids, col, next_ids, t_dev, begin_col, nullptr, nullptr),
                                       B, V, logits_dtype, stream);
}

extern "C" int tw_select_sample(const void* logits, int64_t ld, int logits_dtype, int B, int V, const uint32_t* suppress_bits,
                                const uint32_t* begin_bits, int apply_begin, int64_t eos, uint8_t* done, int64_t* ids,
                                int64_t ld_ids, int col, int64_t* next_ids, const int* t_dev, int begin_col,
                                const uint32_t* ctl, float* sum_logp, hipStream_t stream) {
  if (B <= 0) return TW_OK;
  return select_plain(logits, ld, logits_dtype, B, V, suppress_bits, begin_bits, apply_begin, eos, done, ids, ld_ids, col,
                      next_ids, t_dev, begin_col, ctl, sum_logp, nullptr, 0, stream);
}

extern "C" int tw_select_sample_lp(const void* logits, int64_t ld, int logits_dtype, int B, int V,
                                   const uint32_t* suppress_bits, const uint32_t* begin_bits, int apply_begin,
                                   int64_t eos, uint8_t* done, int64_t* ids, int64_t ld_ids, int col, int64_t* next_ids,
                                   const int* t_dev, int begin_col, const uint32_t* ctl, float* sum_logp,
                                   float* tok_logp, int64_t ld_lp, hipStream_t stream) {
  if (B <= 0) return TW_OK;
  if (lp_bad(sum_logp, tok_logp, ld_lp, col, t_dev)) return TW_EINVAL;
  return select_plain(logits, ld, logits_dtype, B, V, suppress_bits, begin_bits, apply_begin, eos, done, ids, ld_ids, col,
                      next_ids, t_dev, begin_col, ctl, sum_logp, tok_logp, ld_lp, stream);
}
