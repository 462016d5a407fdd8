"""The 8-bit cross-attention K/V format (include/tw_hip.h, cross_kv_dtype="fp8_e4m3") restated in torch on the CPU,
and what the tests of it share.

quantise_ref: per block of Tk x 64 16-bit values, scale = 2^e with e the smallest integer such that
absmax * 2^-e <= 448 (clamped to [-100, 100]; 1 for an all-zero block; NaN for a block with a non-finite value), and
bytes = RNE_e4m3fn(x * 2^-e) by torch's own float8_e4m3fn cast.  RefFp8: the oracle model with exactly that applied
to the cross-attention K and V of every decoder layer, per (clip, head).
"""
import torch

from oracle.whisper_ref import Ref

E4M3_MAX = 448.0
MARGIN = 0.05               # tests/test_decode_gpu.py's margin of the 16-bit engine against Ref


def quantise_ref(x16):
    """x16 [..., Tk, 64] bf16 / fp16 -> (e4m3fn values of the same shape, fp32 scales [...])."""
    assert x16.dtype in (torch.bfloat16, torch.float16)
    lead, n = x16.shape[:-2], x16.shape[-2] * x16.shape[-1]
    flat = x16.float().reshape(-1, n)
    amax = flat.abs().amax(1)
    m, x = torch.frexp(amax)                                       # amax = m * 2^x, m in [0.5, 1)
    e = torch.where(m <= 0.875, x - 9, x - 8).clamp(-100, 100)
    one = torch.ones_like(amax)
    scale, inv = torch.ldexp(one, e), torch.ldexp(one, -e)
    zero, bad = amax == 0, ~torch.isfinite(amax)
    scale = torch.where(zero, one, scale)
    inv = torch.where(zero, one, inv)
    scale = torch.where(bad, torch.full_like(one, float("nan")), scale)
    inv = torch.where(bad, torch.full_like(one, float("nan")), inv)
    q = (flat * inv[:, None]).to(torch.float8_e4m3fn)
    return q.reshape(x16.shape), scale.reshape(lead)


def dequantise_ref(q, scale):
    """fp32 values of a quantised block set (exact)."""
    return q.float() * scale[..., None, None]


class RefFp8(Ref):
    """oracle.whisper_ref.Ref with the cross-attention K and V of every decoder layer through quantise_ref per
    (clip, head) before the attention; everything else inherited."""

    def mha(self, x, kv, pfx, H, causal):
        if not pfx.endswith(".encoder_attn"):
            return super().mha(x, kv, pfx, H, causal)
        B, Tq, d = x.shape
        hd = d // H
        q = self.lin(x, self.p[pfx + ".q_proj.weight"], self.p[pfx + ".q_proj.bias"]) * hd ** -0.5
        k = self.lin(kv, self.p[pfx + ".k_proj.weight"])
        v = self.lin(kv, self.p[pfx + ".v_proj.weight"], self.p[pfx + ".v_proj.bias"])
        Tk = kv.shape[1]
        sh = lambda t, T: t.view(B, T, H, hd).transpose(1, 2)
        rq = lambda t: dequantise_ref(*quantise_ref(sh(t, Tk).contiguous().to(self.half)))
        o = self.attn(sh(q, Tq), rq(k), rq(v), causal)
        o = o.transpose(1, 2).reshape(B, Tq, d)
        return self.lin(o, self.p[pfx + ".out_proj.weight"], self.p[pfx + ".out_proj.bias"])


def agreement(ids, ref_ids, ref_scores, P, eos=50257, margin=MARGIN):
    """ids / ref_ids [B, P + L] (prompt included), ref_scores the reference's processed score rows per generated
    position.  Per row the tokens must equal the reference's up to the row's first difference; there the reference's
    own score row must hold the two tokens within `margin` of each other (a near-tie, which accumulation order may
    decide either way; margin None: any difference, for counting only), and the rest of the row -- a different
    history -- is left out.
    -> (positions left out, generated positions of the reference up to each row's eos)."""
    left = total = 0
    for b in range(ref_ids.shape[0]):
        ref = ref_ids[b, P:].tolist()
        n = ref.index(eos) + 1 if eos in ref else len(ref)
        got = ids[b, P:].tolist() + [eos] * n
        total += n
        for j in range(n):
            if got[j] != ref[j]:
                row = ref_scores[j][b].float()
                gap = float(row.max() - row[got[j]])
                assert margin is None or gap <= margin, (b, j, got[j], ref[j], gap)
                left += n - j - 1
                break
    return left, total


def blocks(B, H, Tk, dtype, seed):
    """Random K-like blocks [B, H, Tk, 64] of a 16-bit dtype with the format's edge cases planted: +-0, values that
    land exactly on e4m3 ties after scaling (the absmax is pinned to 448 * 2^-3, so the scale is 2^-3), and values in
    the e4m3 subnormal range."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, Tk, 64, generator=g)
    flat = x.view(B, H, -1)
    flat.clamp_(-50.0, 50.0)
    flat[..., 0] = 56.0                                    # absmax = 448 / 8: scale 2^-3 exactly
    s = 0.125
    # in units of the scale: ties of the normal range (spacing 2 in [16, 32), 1/8 in [1, 2), 16 in [128, 256)), ties
    # of the subnormal range (odd multiples of 2^-10: the grid is 2^-9), the smallest normal and the largest
    # subnormal, below half the smallest subnormal, and the two zeros
    ties = torch.tensor([17.0, 19.0, -21.0, 1.0625, -1.1875, 200.0, -248.0, 2.0 ** -10, 3 * 2.0 ** -10,
                         -5 * 2.0 ** -10, 13 * 2.0 ** -10, 2.0 ** -6, 7 * 2.0 ** -9, 2.0 ** -11, 0.0, -0.0, 30.0]) * s
    n = min(len(ties), flat.shape[-1] - 1)
    flat[..., 1:1 + n] = ties[:n]
    return x.to(dtype)
