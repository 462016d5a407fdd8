// Flash attention, head dim 64, bf16 in/out, fp32 softmax:
//   encoder self-attention (1500 x 1500), decoder causal self-attention (447 x 447) and
//   cross-attention (447 x 1500) of HF WhisperAttention (modeling_whisper.py:265-350;
//   q pre-scaled by hd^-0.5 -> here `scale` is applied to the fp32 scores, identical
//   because 2^-3 scaling is exact).
//
// Layout: rows of [B*T][ld] with head h at columns h*64 .. h*64+63, so Q/K/V are read
// in place from the fused QKV (or KV) projection output and O is written where out_proj
// reads it.  LSE [B][H][Tq] ([H][rows] for packed rows: AttnP) (natural log of the scaled-score row sum) is kept for the
// backward pass.
//
// MFMA v_mfma_f32_16x16x32_bf16 in the "swapped" orientation: S^T = K·Q^T, so each lane
// holds 4 keys of one query; the probabilities then ARE the B operand of O^T = V^T·P^T
// (accumulator-as-operand, keys in permuted order 4g+r / 16+4g+r) and V^T comes from
// ds_read_b64_tr_b16 reads of a row-major V tile.  Every LDS tile is [64 rows][64] bf16
// with 16-B chunk c of row r stored at c ^ (r & 7): conflict-free for both the ds_read_b128
// row reads and the transposed reads.
//
// Structure.  Three kernels (forward, dQ, dK/dV), each instantiated <H, VL> (fp16 words; packed rows).  What they
// share is written once: attn_frame() (the workgroup's clip, head, rows and base pointers), stage_kv(), causal_nkt(),
// hidden() (the mask), store4() and zero().  Each kernel keeps its own pipeline.  On the host one attn_fill() builds
// the AttnP of a dense or packed call, attn_check() decides its status, TW_DISPATCH_HVL picks the instantiation and
// attn_fwd() / attn_bwd() launch; the twelve C entries forward to those.  The packed kernels run either on a padded
// grid (the _varlen entries) or one workgroup per (entry, head) of a query-block list (the _blocks entries:
// place_entry(), tw_pack_blocks in misc.hip).
#include "common.h"

#include <cstdlib>
#include <type_traits>

namespace {

constexpr int QW = 32;          // query rows per wave
constexpr int QB = 4 * QW;      // query rows per workgroup
constexpr int KT = 64;          // keys per LDS tile
constexpr int TB = KT * 64 * 2; // bytes per [64][64] bf16 tile

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ int swz(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

// [64 rows][64 cols] tile from rows row0.. of a [rows][ld] matrix; rows >= rows_valid read 0.
__device__ __forceinline__ void stage_tile(const bf16* base, int64_t ld, int rows_valid, char* lds, int wave,
                                           int lane) {
  const auto rs = make_rsrc(base);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pce = wave + 4 * i;
    const int r = pce * 8 + (lane >> 3);
    const int c = (lane & 7) ^ (r & 7);
    const uint32_t off = r < rows_valid ? (uint32_t)(((int64_t)r * ld + c * 8) * 2) : TW_OOB;
    buf_load_lds16(rs, lds + pce * 1024, off);
  }
}

// row fragment: lane gives T[rbase + (l&15)][kk*32 + 8*(l>>4) .. +7]
__device__ __forceinline__ bf16x8 rd_row(const char* t, int rbase, int kk, int lane) {
  const int r = rbase + (lane & 15);
  return *(const bf16x8*)(t + swz(r, kk * 4 + (lane >> 4)));
}

// transposed fragment for k-step s over rows: lane gives T^T[cbase + i][rows perm(s)]
//   elements 0..3: rows s*32 + 4g + 0..3 ; elements 4..7: rows s*32 + 16 + 4g + 0..3
__device__ __forceinline__ bf16x8 rd_tr(const char* t, int cbase, int s, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int col = cbase + 4 * (i & 3);
  const int r0 = s * 32 + 4 * g + (i >> 2);
  const int r1 = r0 + 16;
  const int ch = col >> 3, inoff = (col & 7) * 2;
  const char* a0 = t + swz(r0, ch) + inoff;
  const char* a1 = t + swz(r1, ch) + inoff;
  s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)a0);
  s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)a1);
  s16x8 v = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// global fragment: lane gives M[row0 + (l&15)][kk*32 + 8*(l>>4) .. +7] (zero past rows_valid)
__device__ __forceinline__ bf16x8 ld_frag(const bf16* base, int64_t ld, int row, int rows_valid, int kk, int lane) {
  if (row >= rows_valid) return bf16x8{};
  return *(const bf16x8*)(base + (int64_t)row * ld + kk * 32 + 8 * (lane >> 4));
}

// P as the 16-bit operand type of the instantiation (bf16 words, or fp16 words for the fp16 path)
template <bool H>
__device__ __forceinline__ bf16x8 pack8e(const f32x4& a, const f32x4& b) {
  return bf16x8{f2e<H>(a[0]), f2e<H>(a[1]), f2e<H>(a[2]), f2e<H>(a[3]),
                f2e<H>(b[0]), f2e<H>(b[1]), f2e<H>(b[2]), f2e<H>(b[3])};
}

// four fp32 values rounded to the instantiation's 16-bit type, one 8-byte store
template <bool H>
__device__ __forceinline__ void store4(bf16* dst, const f32x4& v) {
  *(bf16x4*)dst = bf16x4{f2e<H>(v[0]), f2e<H>(v[1]), f2e<H>(v[2]), f2e<H>(v[3])};
}

template <int N, int M>
__device__ __forceinline__ void zero(f32x4 (&a)[N][M]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) a[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

struct AttnP {
  const bf16* Q; const bf16* K; const bf16* V; bf16* O; float* lse;
  const bf16* dO; float* Dv; bf16* dQ; bf16* dK; bf16* dV;
  int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  int B, H, Tq, Tk, causal;
  float scale, scale_log2;
  // Packed rows (the VL instantiations, tw_attn_*_varlen): B + 1 cumulative row offsets.  With offq, clip b's
  // queries (Q, O, dO, dQ) are rows offq[b] .. offq[b+1]-1 of their matrices and Tq is only the longest clip (the
  // grid's extent); with offk the keys (K, V, dK, dV) likewise, else they stay dense at b*Tk.  Both null: dense.
  // lse and Dv are then [H][Mq] (Mq = offq[B], every packed query row): entry h*Mq + offq[b] + q.
  const int* offq; const int* offk;
  int Mq;
  // The query-block list of a packed launch (tw_pack_blocks: one {clip, first row, rows, tiles} entry per 128-row
  // block that has rows), or null: the padded grid of the entries without a list, and of every dK/dV launch.
  const int4* wl;
};

// rows of clip b: dense [b*T, b*T + T), or [off[b], off[b+1]) of a packed matrix
template <bool VL>
__device__ __forceinline__ void clip_rows(const int* off, int b, int& T, int64_t& row0) {
  row0 = (int64_t)b * T;
  if constexpr (VL) {
    if (off) {
      row0 = off[b];
      T = off[b + 1] - off[b];
    }
  }
}

constexpr float LOG2E = 1.4426950408889634f;

// XCD-aware bijective remap of a 2-D (blocks_per_head, heads) grid: the blocks of one
// (batch, head) land on one XCD (blocks b and b+8 share one), so its K/V (or Q/dO) tiles are
// fetched into that XCD's L2 once instead of once per XCD.
__device__ __forceinline__ void remap_bh(int& xblk, int& bh) {
  const int nx = gridDim.x, nwg = gridDim.x * gridDim.y;
  const int bid = blockIdx.y * nx + blockIdx.x;
  const int q = nwg / 8, rr = nwg % 8, xcd = bid % 8;
  const int tid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + bid / 8;
  bh = tid / nx;
  xblk = tid % nx;
}
constexpr float NEG_BIG = -1e30f;

__device__ __forceinline__ float fmx(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// One workgroup's place in the problem: its (clip, head), the clip's extents and rows, and its own 128 rows (query
// rows in the forward and dQ kernels, key rows in dK/dV).
struct Frame {
  int lane, wave, g, li;      // g = lane >> 4, li = lane & 15
  int h;
  int blk, row;               // first row of the workgroup / of this wave
  int Tq, Tk;                 // this clip's
  int off;                    // causal diagonal offset Tk - Tq
  int64_t qrow0, krow0;       // the clip's first row in the query-side / key-side matrices
  int64_t lse0;               // lse / Dv index of the clip's query 0
  const bf16 *Qb, *Kb, *Vb;   // row 0 of the clip, this head's columns
  // this head's columns of the clip's row r in any query-side (Q, O, dO, dQ) / key-side (K, V, dK, dV) matrix
  template <class T> __device__ __forceinline__ T* qrow(T* base, int64_t ld, int r = 0) const {
    return base + (qrow0 + r) * ld + h * 64;
  }
  template <class T> __device__ __forceinline__ T* krow(T* base, int64_t ld, int r = 0) const {
    return base + (krow0 + r) * ld + h * 64;
  }
};

// Placement of a (heads, list entries) grid, bijective: (entry, head) of this workgroup.  Workgroup bid runs on XCD
// bid % 8, in bid order.
// Dense keys (cross-attention; the list is in (clip, block) order and every entry walks the same tiles): remap_bh with
// the heads as the inner index, so XCD x takes a contiguous run of entries with all their heads and the blocks of one
// clip, neighbours in the list, read that clip's K/V through one L2.
// Causal (the list is in descending tile order): entry i goes to XCD i % 8 with all its heads, so every XCD walks
// its own descending sequence (longest first) and the eight carry the same load; a clip's K/V there is at most 7
// tiles.  The last nent % 8 entries have no residue class of their own and take the remaining workgroups in order.
__device__ __forceinline__ void place_entry(bool causal, int& ent, int& h) {
  if (!causal) {
    remap_bh(h, ent);
    return;
  }
  const int H = gridDim.x, nent = gridDim.y;
  const int bid = blockIdx.y * H + blockIdx.x;
  const int full = nent & ~7;
  if (bid < full * H) {
    const int t = bid >> 3;
    h = t % H;
    ent = (t / H) * 8 + (bid & 7);
  } else {
    const int local = bid - full * H, r = nent - full;
    ent = full + local % r;
    h = local / r;
  }
}

// A VL kernel on the padded grid leaves when blk is past its clip's last row (blk >= Tq, or Tk in dK/dV): that test is
// workgroup-uniform (blk, Tq and Tk depend on the block index only) and must stay ahead of any LDS-DMA or barrier.
// With a list (AttnP::wl) every workgroup has rows.
template <bool VL>
__device__ __forceinline__ Frame attn_frame(const AttnP& p) {
  Frame f;
  f.lane = lane_id();
  f.wave = wave_id_uniform();
  f.g = f.lane >> 4;
  f.li = f.lane & 15;
  int b, bh = 0;
  if (VL && p.wl) {
    int ent;
    place_entry(p.causal, ent, f.h);
    const int4 e = p.wl[ent];
    b = e.x;
    f.blk = e.y;
  } else {
    int xblk;
    remap_bh(xblk, bh);
    b = bh / p.H;
    f.h = bh % p.H;
    f.blk = xblk * QB;
  }
  f.row = f.blk + f.wave * QW;
  f.Tq = p.Tq;
  f.Tk = p.Tk;
  clip_rows<VL>(p.offq, b, f.Tq, f.qrow0);
  clip_rows<VL>(p.offk, b, f.Tk, f.krow0);
  f.lse0 = VL ? (int64_t)f.h * p.Mq + f.qrow0 : (int64_t)bh * f.Tq;
  f.Qb = f.qrow(p.Q, p.ldq);
  f.Kb = f.krow(p.K, p.ldk);
  f.Vb = f.krow(p.V, p.ldv);
  f.off = f.Tk - f.Tq;
  return f;
}

// K tile kt and V tile kt into stage buf of a [stages][K, V] LDS ring
__device__ __forceinline__ void stage_kv(const AttnP& p, const Frame& f, char* smem, int buf, int kt) {
  char* Ks = smem + buf * 2 * TB;
  const int k0 = kt * KT;
  stage_tile(f.Kb + (int64_t)k0 * p.ldk, p.ldk, f.Tk - k0, Ks, f.wave, f.lane);
  stage_tile(f.Vb + (int64_t)k0 * p.ldv, p.ldv, f.Tk - k0, Ks + TB, f.wave, f.lane);
}

// key tiles a query block walks: all of them, or under the causal mask those its last query can see
__device__ __forceinline__ int causal_nkt(const AttnP& p, const Frame& f) {
  int nkt = (f.Tk + KT - 1) / KT;
  if (p.causal) {
    const int qmax = min(f.Tq - 1, f.blk + QB - 1);
    const int kend = qmax + f.off + 1;
    nkt = min(nkt, (kend + KT - 1) / KT);
  }
  return nkt;
}

// The mask: key `key` is hidden from query q (past the key tail, or above the causal diagonal).  QT: a query past Tq
// hides every key; the forward leaves that test out (rows past Tq hold zero Q fragments and are never stored).
// Stated as "hidden", not "visible": in this form all three loops compile to the instructions they were measured
// with; the other polarity reshapes the forward's masked tiles.
template <bool QT>
__device__ __forceinline__ bool hidden(const AttnP& p, const Frame& f, int q, int key) {
  return (QT ? key >= f.Tk || q >= f.Tq : key >= f.Tk) || (p.causal && key > q + f.off);
}

// ------------------------------------------------------------------------------------
// H = false: bf16 Q/K/V/O (autocast); H = true: fp16 (the fp16 decode path: P rounded to fp16 for PV,
// as SDPA's fp16 flash kernel rounds it)
// K/V arrive in a 3-deep LDS ring: two tiles in flight (prefetch distance 2: the DMA of tile kt+2 overlaps the
// compute of tiles kt and kt+1), counted vmcnt + a raw s_barrier (a __syncthreads() would drain every DMA in
// flight).  (Round 3's opt-in lazy max and the 2-stage ring were deleted in round 4: DESIGN.md, Attention.)
// VL: packed rows (AttnP::offq / offk); without a block list the grid spans the longest clip and a block past its
// clip's last query leaves at once (workgroup-uniform, before any LDS-DMA or barrier); with one (AttnP::wl) every
// workgroup has rows
template <bool H, bool VL>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnP p) {
  constexpr int ST = 3;
  __shared__ __attribute__((aligned(16))) char smem[ST * 2 * TB];   // [ST stages][K, V]
  const Frame f = attn_frame<VL>(p);
  if (VL && f.blk >= f.Tq) return;
  const int lane = f.lane, g = f.g, li = f.li, qw = f.row, Tq = f.Tq, Tk = f.Tk;

  bf16x8 qf[2][2];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[qi][kk] = ld_frag(f.Qb, p.ldq, qw + qi * 16 + li, Tq, kk, lane);

  f32x4 o[4][2];
  zero(o);
  float m[2] = {NEG_BIG, NEG_BIG}, l[2] = {0.f, 0.f};

  const int nkt = causal_nkt(p, f);
  // S^T = K Q^T for one tile, boundary tiles masked (key tail / causal diagonal)
  auto scores = [&](const bf16x8 (&kf)[4][2], f32x4 (&s)[4][2], int k0) {
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      s[kj][0] = mma16<H>(kf[kj][1], qf[0][1], mma16<H>(kf[kj][0], qf[0][0], z));
      s[kj][1] = mma16<H>(kf[kj][1], qf[1][1], mma16<H>(kf[kj][0], qf[1][0], z));
    }
    const bool need_mask = (k0 + KT > Tk) || (p.causal && k0 + KT - 1 > qw + f.off);
    if (need_mask) {
#pragma unroll
      for (int qi = 0; qi < 2; ++qi) {
        const int q = qw + qi * 16 + li;
#pragma unroll
        for (int kj = 0; kj < 4; ++kj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (hidden<false>(p, f, q, k0 + kj * 16 + 4 * g + r)) s[kj][qi][r] = -INFINITY;
          }
      }
    }
  };
  // online softmax (log2 domain), per query column: max on raw scores (scale > 0); p = exp2(s*c - m) is
  // one FMA + one exp; O is rescaled only when some row max of this wave grew.  Returns the lane-partial
  // sums of the weights (added to l by the caller).
  auto exact = [&](f32x4 (&s)[4][2], float (&ls)[2]) {
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      // row max: a tree over the lane's 16 scores, then across the 4 lanes of the query column
      // (l, l^16, l^32, l^48) with v_permlane16/32_swap (VALU) instead of two ds_bpermute trips
      // (a chain of 3-input maxes: 8 v_maximum3_f32 for the 16 scores.  IEEE maximum, not fmaxf: fmaxf in the
      // kernels' IEEE mode first quiets each MFMA result with a v_max_f32 x, x; maximum needs none and propagates
      // a NaN score, which the weights would carry to O and l anyway)
      float tmax = fmx(fmx(s[0][qi][0], s[0][qi][1]), s[0][qi][2]);
#pragma unroll
      for (int e = 3; e < 15; e += 2)
        tmax = fmx(fmx(tmax, s[e >> 2][qi][e & 3]), s[(e + 1) >> 2][qi][(e + 1) & 3]);
      tmax = fmx(tmax, s[3][qi][3]);
      {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
        tmax = fmx(__uint_as_float(a[0]), __uint_as_float(a[1]));
        const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
        tmax = fmx(__uint_as_float(c[0]), __uint_as_float(c[1]));
      }
      const float mn = fmaxf(m[qi], tmax * p.scale_log2);
      if (__any(mn > m[qi])) {
        const float alpha = __builtin_amdgcn_exp2f(m[qi] - mn);
        l[qi] *= alpha;
#pragma unroll
        for (int hj = 0; hj < 4; ++hj) o[hj][qi] *= alpha;
      }
      m[qi] = mn;
      float a = 0.f;      // sequential (a 4-way split moved the micro-config KL by 1e-3 vs the oracle)
      // s*c - m as one scalar v_fma_f32 per score (a v_pk_fma_f32 costs more issue cycles than two
      // v_fma_f32 beside MFMAs: MI355X_MICROARCH constants table), then v_exp_f32 on it directly
      const float nm = -mn;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(fmaf(s[kj][qi][r], p.scale_log2, nm));
          s[kj][qi][r] = e;
          a += e;
        }
      ls[qi] = a;
    }
  };
  stage_kv(p, f, smem, 0, 0);
  if (nkt > 1) {
    stage_kv(p, f, smem, 1, 1);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // tile 0 landed (4 DMA per tile per wave), tile 1 flies
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();

  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt % 3;
    const char* Ks = smem + cur * 2 * TB;
    const char* Vs = Ks + TB;
    // all K and V fragments of this tile into registers BEFORE the next tile's LDS-DMA is
    // issued: otherwise the compiler cannot prove the DMA does not alias these reads and
    // drains vmcnt(0) in the middle of the tile (exposing the whole load latency)
    bf16x8 kf[4][2], vf[4][2];
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) kf[kj][kk] = rd_row(Ks, kj * 16, kk, lane);
#pragma unroll
    for (int hj = 0; hj < 4; ++hj)
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) vf[hj][ss] = rd_tr(Vs, hj * 16, ss, lane);
    if (kt + 2 < nkt) stage_kv(p, f, smem, (kt + 2) % 3, kt + 2);   // the slot tile kt-1 was read from
    const int k0 = kt * KT;
    f32x4 s[4][2];
    scores(kf, s, k0);
    float ls[2];
    exact(s, ls);
    l[0] += ls[0];
    l[1] += ls[1];
    // O^T += V^T P^T
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const bf16x8 p0 = pack8e<H>(s[2 * ss][0], s[2 * ss + 1][0]);
      const bf16x8 p1 = pack8e<H>(s[2 * ss][1], s[2 * ss + 1][1]);
#pragma unroll
      for (int hj = 0; hj < 4; ++hj) {
        o[hj][0] = mma16<H>(vf[hj][ss], p0, o[hj][0]);
        o[hj][1] = mma16<H>(vf[hj][ss], p1, o[hj][1]);
      }
    }
    // tile kt+1 must have landed for every wave; tile kt+2 (issued this iteration) may stay in flight
    if (kt + 2 < nkt) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // epilogue
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const float lt = swap32_sum(swap16_sum(l[qi]));   // xor 16 then 32 on permlane swaps (bit-identical: common.h)
    const int q = qw + qi * 16 + li;
    if (q < Tq) {
      const float inv = 1.f / lt;
      bf16* Ob = f.qrow(p.O, p.ldo, q);
#pragma unroll
      for (int hj = 0; hj < 4; ++hj) store4<H>(Ob + hj * 16 + 4 * g, o[hj][qi] * inv);
      if (g == 0 && p.lse) p.lse[f.lse0 + q] = (m[qi] + log2f(lt)) / LOG2E;
    }
  }
}


// ------------------------------------------------------------------------------------
// dQ: per query block, loop over key tiles (K, V in LDS).  Also computes D[q] = sum_e dO[q][e] O[q][e] for its rows
// (each lane's 16 products, then the 4 lanes of a row by xor-16 / xor-32 swaps) and stores it for the dK/dV kernel,
// which runs after it: no separate pass over dO and O.
template <bool H, bool VL>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(AttnP p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TB];
  const Frame f = attn_frame<VL>(p);
  if (VL && f.blk >= f.Tq) return;
  const int lane = f.lane, g = f.g, li = f.li, qw = f.row, Tq = f.Tq, Tk = f.Tk;
  const bf16* dOb = f.qrow(p.dO, p.lddo);
  const bf16* Ob = f.qrow(p.O, p.ldo);
  bf16x8 qf[2][2], dof[2][2];
  float lse2[2], Dq[2];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const int q = qw + qi * 16 + li;
    float dd = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      qf[qi][kk] = ld_frag(f.Qb, p.ldq, q, Tq, kk, lane);
      dof[qi][kk] = ld_frag(dOb, p.lddo, q, Tq, kk, lane);
      const bf16x8 of = ld_frag(Ob, p.ldo, q, Tq, kk, lane);
#pragma unroll
      for (int e = 0; e < 8; ++e) dd += e2f<H>(dof[qi][kk][e]) * e2f<H>(of[e]);
    }
    lse2[qi] = q < Tq ? p.lse[f.lse0 + q] * LOG2E : 0.f;
    Dq[qi] = swap32_sum(swap16_sum(dd));                 // rows past Tq: zero fragments, D = 0
    if (g == 0 && q < Tq) p.Dv[f.lse0 + q] = Dq[qi];
  }
  f32x4 dq[4][2];
  zero(dq);

  const int nkt = causal_nkt(p, f);
  stage_kv(p, f, smem, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) stage_kv(p, f, smem, cur ^ 1, kt + 1);
    const char* Ks = smem + cur * 2 * TB;
    const char* Vs = Ks + TB;
    f32x4 s[4][2], dp[4][2];
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
      s[kj][0] = s[kj][1] = dp[kj][0] = dp[kj][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 kf = rd_row(Ks, kj * 16, kk, lane);
        const bf16x8 vf = rd_row(Vs, kj * 16, kk, lane);
        s[kj][0] = mma16<H>(kf, qf[0][kk], s[kj][0]);
        s[kj][1] = mma16<H>(kf, qf[1][kk], s[kj][1]);
        dp[kj][0] = mma16<H>(vf, dof[0][kk], dp[kj][0]);
        dp[kj][1] = mma16<H>(vf, dof[1][kk], dp[kj][1]);
      }
    }
    const int k0 = kt * KT;
    // P recomputed with the forward's exp2 (v_exp_f32) and, on interior tiles (no key tail, no query tail, not on
    // the causal diagonal: wave-uniform), without the per-element mask
    const bool need_mask = (k0 + KT > Tk) || (qw + QW > Tq) || (p.causal && k0 + KT - 1 > qw + f.off);
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      const int q = qw + qi * 16 + li;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = !need_mask || !hidden<true>(p, f, q, k0 + kj * 16 + 4 * g + r);
          // masked scores as exp2(-inf) = 0: a select, not a branch per element (interior tiles: ok is always true)
          const float pr = __builtin_amdgcn_exp2f(ok ? s[kj][qi][r] * p.scale_log2 - lse2[qi] : -INFINITY);
          s[kj][qi][r] = pr * (dp[kj][qi][r] - Dq[qi]);   // dS^T
        }
    }
    // dQ^T += K^T dS^T
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const bf16x8 d0 = pack8e<H>(s[2 * ss][0], s[2 * ss + 1][0]);
      const bf16x8 d1 = pack8e<H>(s[2 * ss][1], s[2 * ss + 1][1]);
#pragma unroll
      for (int hj = 0; hj < 4; ++hj) {
        const bf16x8 kt_ = rd_tr(Ks, hj * 16, ss, lane);
        dq[hj][0] = mma16<H>(kt_, d0, dq[hj][0]);
        dq[hj][1] = mma16<H>(kt_, d1, dq[hj][1]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const int q = qw + qi * 16 + li;
    if (q < Tq) {
      bf16* out = f.qrow(p.dQ, p.lddq, q);
#pragma unroll
      for (int hj = 0; hj < 4; ++hj) store4<H>(out + hj * 16 + 4 * g, dq[hj][qi] * p.scale);
    }
  }
}

// dK, dV: per key block (32 keys per wave, 128 per workgroup), loop over query tiles
// Two workgroups per CU (round 4): 218 VGPRs, two waves per SIMD hide each other's LDS / exp / MFMA latencies.  At
// one workgroup per CU (round 3: 268-276 VGPRs, accumulators shuffled through AGPRs) the encoder-shape backward
// took 6.1 ms against 4.6 ms now (tools/bench_attn.py, same box, profiles/r04_h_attn_bwd_ab.log).
template <bool H, bool VL>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkdv_kernel(AttnP p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TB + 2 * 2 * 64 * 4];
  const Frame f = attn_frame<VL>(p);   // blk, row: this workgroup's / wave's first key
  if (VL && f.blk >= f.Tk) return;     // a clip without queries still writes its (zero) dK / dV rows below
  const int lane = f.lane, g = f.g, li = f.li, kw = f.row, Tq = f.Tq, Tk = f.Tk;
  const bf16* dOb = f.qrow(p.dO, p.lddo);
  float* rowc = (float*)(smem + 4 * TB);   // [2 stages][lse2 64 | D 64]

  bf16x8 kf[2][2], vf[2][2];
#pragma unroll
  for (int kj = 0; kj < 2; ++kj)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      kf[kj][kk] = ld_frag(f.Kb, p.ldk, kw + kj * 16 + li, Tk, kk, lane);
      vf[kj][kk] = ld_frag(f.Vb, p.ldv, kw + kj * 16 + li, Tk, kk, lane);
    }
  f32x4 dk[4][2], dv[4][2];
  zero(dk);
  zero(dv);

  const int nqt_all = (Tq + KT - 1) / KT;
  int qt0 = 0;
  if (p.causal) {
    const int qmin = f.blk - f.off;   // first query that can see this key block
    qt0 = qmin > 0 ? qmin / KT : 0;
  }
  auto stage = [&](int buf, int qt) {
    char* Qs = smem + buf * 2 * TB;
    const int q0 = qt * KT;
    stage_tile(f.Qb + (int64_t)q0 * p.ldq, p.ldq, Tq - q0, Qs, f.wave, lane);
    stage_tile(dOb + (int64_t)q0 * p.lddo, p.lddo, Tq - q0, Qs + TB, f.wave, lane);
    if (threadIdx.x < 64) {
      const int q = q0 + threadIdx.x;
      rowc[buf * 128 + threadIdx.x] = q < Tq ? p.lse[f.lse0 + q] * LOG2E : 0.f;
      rowc[buf * 128 + 64 + threadIdx.x] = q < Tq ? p.Dv[f.lse0 + q] : 0.f;
    }
  };
  if (qt0 < nqt_all) {
    stage(0, qt0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  for (int qt = qt0; qt < nqt_all; ++qt) {
    const int cur = (qt - qt0) & 1;
    if (qt + 1 < nqt_all) stage(cur ^ 1, qt + 1);
    const char* Qs = smem + cur * 2 * TB;
    const char* dOs = Qs + TB;
    const float* lrow = rowc + cur * 128;
    const int q0 = qt * KT;
    // S[q][key], dP[q][key] for 64 q x 32 keys
    f32x4 s[4][2], dp[4][2];
#pragma unroll
    for (int qf = 0; qf < 4; ++qf) {
      s[qf][0] = s[qf][1] = dp[qf][0] = dp[qf][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 qa = rd_row(Qs, qf * 16, kk, lane);
        const bf16x8 da = rd_row(dOs, qf * 16, kk, lane);
        s[qf][0] = mma16<H>(qa, kf[0][kk], s[qf][0]);
        s[qf][1] = mma16<H>(qa, kf[1][kk], s[qf][1]);
        dp[qf][0] = mma16<H>(da, vf[0][kk], dp[qf][0]);
        dp[qf][1] = mma16<H>(da, vf[1][kk], dp[qf][1]);
      }
    }
    // interior tiles (no query tail, no key tail, not on the causal diagonal: wave-uniform) skip the mask
    const bool need_mask = (q0 + KT > Tq) || (kw + QW > Tk) || (p.causal && kw + QW - 1 > q0 + f.off);
#pragma unroll
    for (int qf = 0; qf < 4; ++qf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ql = qf * 16 + 4 * g + r;
        const int q = q0 + ql;
        const float l2 = lrow[ql], Dq = lrow[64 + ql];
#pragma unroll
        for (int kj = 0; kj < 2; ++kj) {
          const bool ok = !need_mask || !hidden<true>(p, f, q, kw + kj * 16 + li);
          const float pr = __builtin_amdgcn_exp2f(ok ? s[qf][kj][r] * p.scale_log2 - l2 : -INFINITY);   // select, no branch
          s[qf][kj][r] = pr;                              // P
          dp[qf][kj][r] = pr * (dp[qf][kj][r] - Dq);      // dS
        }
      }
    // dV^T += dO^T P ; dK^T += Q^T dS
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const bf16x8 p0 = pack8e<H>(s[2 * ss][0], s[2 * ss + 1][0]);
      const bf16x8 p1 = pack8e<H>(s[2 * ss][1], s[2 * ss + 1][1]);
      const bf16x8 d0 = pack8e<H>(dp[2 * ss][0], dp[2 * ss + 1][0]);
      const bf16x8 d1 = pack8e<H>(dp[2 * ss][1], dp[2 * ss + 1][1]);
#pragma unroll
      for (int hj = 0; hj < 4; ++hj) {
        const bf16x8 dot = rd_tr(dOs, hj * 16, ss, lane);
        const bf16x8 qt_ = rd_tr(Qs, hj * 16, ss, lane);
        dv[hj][0] = mma16<H>(dot, p0, dv[hj][0]);
        dv[hj][1] = mma16<H>(dot, p1, dv[hj][1]);
        dk[hj][0] = mma16<H>(qt_, d0, dk[hj][0]);
        dk[hj][1] = mma16<H>(qt_, d1, dk[hj][1]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#pragma unroll
  for (int kj = 0; kj < 2; ++kj) {
    const int key = kw + kj * 16 + li;
    if (key < Tk) {
      bf16* ok_ = f.krow(p.dK, p.lddk, key);
      bf16* ov_ = f.krow(p.dV, p.lddv, key);
#pragma unroll
      for (int hj = 0; hj < 4; ++hj) {
        store4<H>(ok_ + hj * 16 + 4 * g, dk[hj][kj] * p.scale);
        store4<H>(ov_ + hj * 16 + 4 * g, dv[hj][kj]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// Host side.  Dense entries: B clips of Tq x Tk, lse (and the backward's workspace, the D = rowsum(dO*O) vector)
// [B][H][Tq].
// Packed rows (the trainer's decoder: clip b holds only its first n_b rows, the clips concatenated).  offq: B + 1
// cumulative query-row offsets (device, int32), Mq = offq[B], max_q = the longest clip.  offk: the same for the
// keys (causal self-attention passes one array for both), or null for dense keys at b*Tk (cross-attention against
// the encoder's 1500 rows); Tk is the dense key count, or with offk the longest clip's.  lse (and the backward's
// workspace) are [H][Mq].  The per-clip tile order is the dense kernels', so every clip's rows equal a dense call
// on that clip alone bit for bit.  A clip without queries gets zero dK / dV rows.

// The AttnP of any entry: a dense call passes offq = offk = null, Mq = 0; a packed one its max_q as Tq.  The forward
// leaves the backward's tensors out.
AttnP attn_fill(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const void* O,
                int64_t ldo, const float* lse, int B, int H, int Tq, int Tk, int causal, float scale, const int* offq,
                const int* offk, int Mq, const void* dO = nullptr, int64_t lddo = 0, void* dQ = nullptr,
                int64_t lddq = 0, void* dK = nullptr, int64_t lddk = 0, void* dV = nullptr, int64_t lddv = 0,
                float* workspace = nullptr) {
  AttnP p = {};
  p.Q = (const bf16*)Q; p.K = (const bf16*)K; p.V = (const bf16*)V; p.O = (bf16*)O; p.lse = (float*)lse;
  p.dO = (const bf16*)dO; p.Dv = workspace; p.dQ = (bf16*)dQ; p.dK = (bf16*)dK; p.dV = (bf16*)dV;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.lddo = lddo; p.lddq = lddq; p.lddk = lddk; p.lddv = lddv;
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk; p.causal = causal;
  p.scale = scale; p.scale_log2 = scale * LOG2E;
  p.offq = offq; p.offk = offk; p.Mq = Mq;
  return p;
}

constexpr int ATTN_LAUNCH = -1;

// The status of a call that launches nothing, else ATTN_LAUNCH.  packed: a tw_attn_*_varlen entry (p.Tq is its
// max_q); bwd: the backward pass, whose dQ kernel reads O and dO in 16-byte fragments (the forward stores O in 8-byte
// pieces).  The order of the tests is part of the C ABI's behaviour.
int attn_check(const AttnP& p, int head_dim, bool packed, bool bwd) {
  if (head_dim != 64) return TW_EUNSUPPORTED;
  // scale > 0 (the forward takes the row max on raw scores), NaN failing too: tested on the bits (0 < bits <= +inf),
  // because this file is built with -fno-honor-nans, which lets the compiler turn !(scale > 0.f) into scale <= 0.f
  if (__builtin_bit_cast(uint32_t, p.scale) - 1u >= 0x7f800000u) return TW_EINVAL;
  if (packed) {
    if (!(p.offq != nullptr && p.B > 0 && p.Mq >= 0 && p.Tq >= 0 && p.Tq <= p.Mq && p.Tk >= 0 &&
          !(p.causal && p.Tq > p.Tk)))
      return TW_EINVAL;
    // without queries the backward still has dK / dV to zero (dense keys)
    if (p.Tk == 0 || (!bwd && (p.Mq == 0 || p.Tq == 0))) return TW_OK;
  } else if (p.B <= 0 || p.Tq <= 0 || p.Tk <= 0) {
    return TW_OK;
  }
  if ((((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V) & 15) || ((p.ldq | p.ldk | p.ldv) & 7)) return TW_EINVAL;
  if (bwd ? (((uintptr_t)p.dO | (uintptr_t)p.O) & 15) || ((p.lddo | p.ldo) & 7) : (p.ldo & 3) != 0) return TW_EINVAL;
  if (!packed && p.causal && p.Tq > p.Tk) return TW_EINVAL;
  return ATTN_LAUNCH;
}

// run the statement with H (fp16 words, else bf16) and VL (packed rows) as constants:
// TW_DISPATCH_HVL(half, packed, hipLaunchKernelGGL((K<H, VL>), ...))
#define TW_DISPATCH_HVL(half, packed, ...)                                      \
  do {                                                                          \
    if ((half) && (packed)) { constexpr bool H = true, VL = true; __VA_ARGS__; } \
    else if (half) { constexpr bool H = true, VL = false; __VA_ARGS__; }        \
    else if (packed) { constexpr bool H = false, VL = true; __VA_ARGS__; }      \
    else { constexpr bool H = false, VL = false; __VA_ARGS__; }                 \
  } while (0)

dim3 attn_grid(const AttnP& p, int rows) { return dim3((rows + QB - 1) / QB, p.B * p.H); }

// The query blocks of a packed call with a list (the _blocks entries): the list in the order of the call's kind
// (tw_pack_blocks) and its length.  No list (dense calls, the _varlen entries): null, 0.
struct Blocks {
  const int* list;
  int n;
};

// the grid of a list (place_entry): one workgroup per (head, entry)
dim3 list_grid(const AttnP& p, const Blocks& bl) { return dim3(p.H, bl.n); }
AttnP with_list(AttnP p, const Blocks& bl) {
  p.wl = (const int4*)bl.list;
  return p;
}

int blocks_check(const Blocks& bl) {
  return bl.list != nullptr && ((uintptr_t)bl.list & 15) == 0 && bl.n >= 0 && bl.n <= 65535 ? TW_OK : TW_EINVAL;
}

// half: fp16 Q/K/V/O (HF Whisper with torch_dtype=float16: SDPA over fp16 projections, run_eval.py:99,500-509)
// bl: the forward launches one workgroup per (entry, head) and none without rows.
int attn_fwd(const AttnP& p, int head_dim, bool packed, bool half, hipStream_t stream, const Blocks* bl = nullptr) {
  if (const int st = attn_check(p, head_dim, packed, false); st != ATTN_LAUNCH) return st;
  if (bl) {
    if (const int st = blocks_check(*bl); st != TW_OK) return st;
    if (bl->n == 0) return TW_OK;
  }
  const AttnP pl = bl ? with_list(p, *bl) : p;
  TW_DISPATCH_HVL(half, packed,
                  hipLaunchKernelGGL((attn_fwd_kernel<H, VL>), bl ? list_grid(p, *bl) : attn_grid(p, p.Tq), dim3(256), 0,
                                     stream, pl));
  TW_CHECK_LAUNCH();
  return TW_OK;
}

// half: fp16 Q/K/V/O/dO/dQ/dK/dV (the student's SDPA backward under fp16 autocast, run_distillation.py:815-817
// mixed_precision="fp16"): the bf16 kernels instantiated for fp16 words (P and dS rounded to fp16 for their MFMAs)
int attn_bwd(const AttnP& p, int head_dim, bool packed, bool half, hipStream_t stream, const Blocks* bl = nullptr) {
  if (const int st = attn_check(p, head_dim, packed, true); st != ATTN_LAUNCH) return st;
  if (bl)
    if (const int st = blocks_check(*bl); st != TW_OK) return st;
  // dQ (and D, which the dK/dV kernel reads) first, then dK/dV; with packed queries and dense keys the dK/dV launch
  // runs even when no clip has a query (zeros).  With a list dQ runs one workgroup per (entry, head); dK/dV is
  // key-side and keeps its grid.
  const AttnP pq = bl ? with_list(p, *bl) : p;
  TW_DISPATCH_HVL(half, packed, {
    if (bl ? bl->n > 0 : p.Tq > 0)
      hipLaunchKernelGGL((attn_bwd_dq_kernel<H, VL>), bl ? list_grid(p, *bl) : attn_grid(p, p.Tq), dim3(256), 0,
                         stream, pq);
    hipLaunchKernelGGL((attn_bwd_dkdv_kernel<H, VL>), attn_grid(p, p.Tk), dim3(256), 0, stream, p);
  });
  TW_CHECK_LAUNCH();
  return TW_OK;
}

}  // namespace

extern "C" int tw_attn_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                           int64_t ldo, float* lse, int B, int H, int Tq, int Tk, int head_dim, int causal, float scale,
                           hipStream_t stream) {
  return attn_fwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Tq, Tk, causal, scale, nullptr, nullptr, 0),
                  head_dim, false, false, stream);
}

extern "C" int tw_attn_fwd_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                               void* O, int64_t ldo, float* lse, int B, int H, int Tq, int Tk, int head_dim, int causal,
                               float scale, hipStream_t stream) {
  return attn_fwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Tq, Tk, causal, scale, nullptr, nullptr, 0),
                  head_dim, false, true, stream);
}

extern "C" int tw_attn_bwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                           const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ,
                           int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, int B, int H, int Tq, int Tk,
                           int head_dim, int causal, float scale, float* workspace, hipStream_t stream) {
  return attn_bwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Tq, Tk, causal, scale, nullptr, nullptr, 0, dO,
                            lddo, dQ, lddq, dK, lddk, dV, lddv, workspace),
                  head_dim, false, false, stream);
}

extern "C" int tw_attn_bwd_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                               const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ,
                               int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, int B, int H, int Tq,
                               int Tk, int head_dim, int causal, float scale, float* workspace, hipStream_t stream) {
  return attn_bwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Tq, Tk, causal, scale, nullptr, nullptr, 0, dO,
                            lddo, dQ, lddq, dK, lddk, dV, lddv, workspace),
                  head_dim, false, true, stream);
}

extern "C" int tw_attn_fwd_varlen(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                  void* O, int64_t ldo, float* lse, const int* offq, const int* offk, int B, int H,
                                  int Mq, int max_q, int Tk, int head_dim, int causal, float scale,
                                  hipStream_t stream) {
  return attn_fwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_q, Tk, causal, scale, offq, offk, Mq),
                  head_dim, true, false, stream);
}

extern "C" int tw_attn_fwd_varlen_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                                      int64_t ldv, void* O, int64_t ldo, float* lse, const int* offq, const int* offk,
                                      int B, int H, int Mq, int max_q, int Tk, int head_dim, int causal, float scale,
                                      hipStream_t stream) {
  return attn_fwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_q, Tk, causal, scale, offq, offk, Mq),
                  head_dim, true, true, stream);
}

extern "C" int tw_attn_bwd_varlen(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                  const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ,
                                  int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, const int* offq,
                                  const int* offk, int B, int H, int Mq, int max_q, int Tk, int head_dim, int causal,
                                  float scale, float* workspace, hipStream_t stream) {
  return attn_bwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_q, Tk, causal, scale, offq, offk, Mq, dO,
                            lddo, dQ, lddq, dK, lddk, dV, lddv, workspace),
                  head_dim, true, false, stream);
}

extern "C" int tw_attn_bwd_varlen_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                                      int64_t ldv, const void* O, int64_t ldo, const void* dO, int64_t lddo,
                                      const float* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV,
                                      int64_t lddv, const int* offq, const int* offk, int B, int H, int Mq, int max_q,
                                      int Tk, int head_dim, int causal, float scale, float* workspace,
                                      hipStream_t stream) {
  return attn_bwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_q, Tk, causal, scale, offq, offk, Mq, dO,
                            lddo, dQ, lddq, dK, lddk, dV, lddv, workspace),
                  head_dim, true, true, stream);
}

// The packed entries with a query-block list (tw_pack_blocks): `blocks` is the list in the order of the call's kind
// (dense keys or causal), nblk entries.
extern "C" int tw_attn_fwd_blocks(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                  void* O, int64_t ldo, float* lse, const int* offq, const int* offk,
                                  const int* blocks, int nblk, int B, int H, int Mq, int max_q, int Tk, int head_dim,
                                  int causal, float scale, hipStream_t stream) {
  const Blocks bl = {blocks, nblk};
  return attn_fwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_q, Tk, causal, scale, offq, offk, Mq),
                  head_dim, true, false, stream, &bl);
}

extern "C" int tw_attn_fwd_blocks_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                                      int64_t ldv, void* O, int64_t ldo, float* lse, const int* offq, const int* offk,
                                      const int* blocks, int nblk, int B, int H, int Mq, int max_q, int Tk,
                                      int head_dim, int causal, float scale, hipStream_t stream) {
  const Blocks bl = {blocks, nblk};
  return attn_fwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_q, Tk, causal, scale, offq, offk, Mq),
                  head_dim, true, true, stream, &bl);
}

extern "C" int tw_attn_bwd_blocks(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                  const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ,
                                  int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, const int* offq,
                                  const int* offk, const int* blocks, int nblk, int B, int H, int Mq, int max_q, int Tk,
                                  int head_dim, int causal, float scale, float* workspace, hipStream_t stream) {
  const Blocks bl = {blocks, nblk};
  return attn_bwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_q, Tk, causal, scale, offq, offk, Mq, dO,
                            lddo, dQ, lddq, dK, lddk, dV, lddv, workspace),
                  head_dim, true, false, stream, &bl);
}

extern "C" int tw_attn_bwd_blocks_f16(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                                      int64_t ldv, const void* O, int64_t ldo, const void* dO, int64_t lddo,
                                      const float* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV,
                                      int64_t lddv, const int* offq, const int* offk, const int* blocks, int nblk,
                                      int B, int H, int Mq, int max_q, int Tk, int head_dim, int causal,
                                      float scale, float* workspace, hipStream_t stream) {
  const Blocks bl = {blocks, nblk};
  return attn_bwd(attn_fill(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_q, Tk, causal, scale, offq, offk, Mq, dO,
                            lddo, dQ, lddq, dK, lddk, dV, lddv, workspace),
                  head_dim, true, true, stream, &bl);
}
