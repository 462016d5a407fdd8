"""The kernels of the 8-bit cross-attention K/V cache (csrc/xkv_fp8.hip) against the format's CPU restatement
(tests/xkv_fp8_cases.py):

* tw_kv_head_major_fp8: bytes and scales equal quantise_ref bit for bit (bf16 and fp16; +-0, e4m3 ties in the normal
  and the subnormal range, an all-zero block, a block of bf16 subnormals at the exponent clamp), guard bytes intact;
* tw_decode_attn_fp8 / tw_decode_attn_mq_fp8 per element against fp64 attention over the DEQUANTISED cache at the bar
  of tests/test_decode_kstart_gpu.py (2^-7 max|ref| + 1e-3), and against the 16-bit entry run on the dequantised cache
  within one output ulp (2 U max|ref|: the same real number from identical inputs, another fp32 summation order at
  most), on the one-workgroup, split and multi-query paths;
* bit-identities: shared block == per-row copies, a k_start row == the single-row call advanced, run == rerun,
  multi-query row == the single-query call;
* masking: every cache carries NaN bytes (0x7F) in guard rows past Tk and in the rows below each k_start;
* status codes.
"""
import ctypes

import pytest
import torch

import xkv_fp8_cases as xc
from attn_cases import U

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]
NAN_BYTE = 0x7F


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,H,Tk", [(1, 1, 1), (2, 3, 37), (1, 20, 1500)])
def test_quantiser_is_bit_exact(B, H, Tk, dt):
    from tw import ops
    k, v = xc.blocks(B, H, Tk, dt, seed=Tk), xc.blocks(B, H, Tk, dt, seed=Tk + 1) * 3
    if B >= 2:
        k[1, 0] = 0                                                     # all-zero block: scale 1
        k[0, 2, 3, 5] = float("-0.0")
        tiny = 2.0 ** -130 if dt == torch.bfloat16 else 2.0 ** -24      # subnormals (bf16: the exponent clamp)
        v[1, 2] = tiny
        v[1, 2, 4, 7] = -3 * tiny
        v[0, 1] *= 2.0 ** -9                                            # a scale far from 1
    d = 64 * H
    ld = 2 * d + 8                                                      # a padded source row
    src = torch.full((B * Tk, ld), 7.0, dtype=dt)
    src[:, :d] = k.transpose(1, 2).reshape(B * Tk, d)
    src[:, d:2 * d] = v.transpose(1, 2).reshape(B * Tk, d)
    n, ns = 2 * B * H * Tk * 64, 2 * B * H
    dst = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    scales = torch.full((ns + 4,), 777.0, dtype=torch.float32, device=DEV)
    ops.kv_head_major_fp8(src.to(DEV), ld, dst, scales, B, Tk, H)
    (qk, sk), (qv, sv) = xc.quantise_ref(k), xc.quantise_ref(v)
    want = torch.cat([qk.view(torch.uint8).reshape(-1), qv.view(torch.uint8).reshape(-1)])
    want_s = torch.cat([sk.reshape(-1), sv.reshape(-1)])
    got, got_s = dst.cpu(), scales.cpu()
    assert torch.equal(got_s[:ns], want_s), (got_s[:ns], want_s)
    bad = (got[:n] != want).nonzero().view(-1)
    assert bad.numel() == 0, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]]
    assert bool((got[n:] == 0xAB).all()) and bool((got_s[ns:] == 777.0).all())


def test_quantiser_non_finite_block_and_status_codes():
    from tw import _native, ops
    B, H, Tk = 1, 2, 5
    src = torch.randn(B * Tk, 2 * 64 * H).to(torch.bfloat16)
    src[3, 70] = float("inf")                                           # K block of head 1
    dst = torch.zeros(2 * B * H * Tk * 64, dtype=torch.uint8, device=DEV)
    scales = torch.zeros(2 * B * H, dtype=torch.float32, device=DEV)
    sd = src.to(DEV)
    ops.kv_head_major_fp8(sd, 2 * 64 * H, dst, scales, B, Tk, H)
    s = scales.cpu()
    assert torch.isnan(s[1]) and bool(torch.isfinite(s[[0, 2, 3]]).all())
    f = _native.lib().tw_kv_head_major_fp8
    st = torch.cuda.current_stream().cuda_stream
    assert f(sd.data_ptr(), 2 * 64 * H, dst.data_ptr(), scales.data_ptr(), B, Tk, H, ops.F32, st) == 2
    assert f(sd.data_ptr(), 2 * 64 * H + 4, dst.data_ptr(), scales.data_ptr(), B, Tk, H, ops.BF16, st) == 1
    assert f(sd.data_ptr(), 2 * 64 * H, dst.data_ptr(), None, B, Tk, H, ops.BF16, st) == 1
    assert f(None, 2 * 64 * H, dst.data_ptr(), scales.data_ptr(), B, Tk, H, ops.BF16, st) == 1


# ------------------------------------------------------------------------------------------ attention
PAD = 2             # guard rows past Tk in every block, NaN bytes


class Cache:
    """A quantised K/V cache [B][H][Tk + PAD][64] on the device with NaN bytes in the guard rows and below `starts`,
    its scales, and the same cache dequantised to `dt` (NaN in the same rows)."""

    def __init__(self, B, H, Tk, dt, seed, starts=None):
        g = torch.Generator().manual_seed(seed)
        mag = 2.0 ** ((torch.arange(B * H) % 5).float() - 2).view(B, H, 1, 1)       # block scales that differ
        k = (torch.randn(B, H, Tk, 64, generator=g) * mag).to(dt)
        v = (torch.randn(B, H, Tk, 64, generator=g) * mag.flip(1)).to(dt)
        self.B, self.H, self.Tk, self.Tg, self.dt = B, H, Tk, Tk + PAD, dt
        self.starts = starts
        (qk, self.sk), (qv, self.sv) = xc.quantise_ref(k), xc.quantise_ref(v)
        self.k, self.v = xc.dequantise_ref(qk, self.sk), xc.dequantise_ref(qv, self.sv)       # fp32, exact
        assert torch.equal(self.k.to(dt).float(), self.k) and torch.equal(self.v.to(dt).float(), self.v)
        self.kb, self.vb = self._guard(qk.view(torch.uint8), NAN_BYTE), self._guard(qv.view(torch.uint8), NAN_BYTE)
        self.kd, self.vd = self._guard(self.k.to(dt), float("nan")), self._guard(self.v.to(dt), float("nan"))
        self.skd, self.svd = self.sk.to(DEV), self.sv.to(DEV)

    def _guard(self, t, fill):
        out = torch.full((self.B, self.H, self.Tg, 64), fill, dtype=t.dtype)
        out[:, :, :self.Tk] = t
        for b, s in enumerate(self.starts or []):
            out[b, :, :max(min(s, self.Tk - 1), 0)] = fill
        return out.to(DEV)

    def ref(self, q):
        """q [B, Q, H*64] -> fp64 attention over the dequantised cache [B, Q, H*64]."""
        B, H, Tk = self.B, self.H, self.Tk
        out = torch.empty(q.shape, dtype=torch.float64)
        for b in range(B):
            s0 = max(min(self.starts[b], Tk - 1), 0) if self.starts else 0
            kk, vv = self.k[b, :, s0:].double(), self.v[b, :, s0:].double()
            qq = q[b].double().view(-1, H, 64)
            s = torch.einsum("qhe,hke->qhk", qq, kk) * 0.125
            out[b] = torch.einsum("qhk,hke->qhe", torch.softmax(s, -1), vv).reshape(qq.shape[0], -1)
        return out

    def _ks(self):
        return torch.tensor(self.starts, dtype=torch.int32, device=DEV) if self.starts else None

    def run_fp8(self, q):
        """q [B, Q, d] on the device; Q == 1 through tw_decode_attn_fp8, else tw_decode_attn_mq_fp8."""
        from tw import ops
        B, H, Tk, Tg = self.B, self.H, self.Tk, self.Tg
        Q, d = q.shape[1], H * 64
        o = torch.full_like(q, float("nan"))
        if Q == 1:
            ops.decode_attn_fp8(q, d, self.kb, 64, H * Tg * 64, self.vb, 64, H * Tg * 64, self.skd, self.svd, H, o, d,
                                B, H, Tk, 0.125, hsk=Tg * 64, hsv=Tg * 64, k_start=self._ks())
        else:
            ops.decode_attn_mq_fp8(q, Q * d, d, self.kb, 64, H * Tg * 64, self.vb, 64, H * Tg * 64, self.skd, self.svd,
                                   H, o, Q * d, d, B, H, Q, Tk, 0.125, hsk=Tg * 64, hsv=Tg * 64, k_start=self._ks())
        return o

    def run_16(self, q):
        """The existing 16-bit entries over the dequantised cache."""
        from tw import ops
        B, H, Tk, Tg = self.B, self.H, self.Tk, self.Tg
        Q, d = q.shape[1], H * 64
        o = torch.full_like(q, float("nan"))
        if Q == 1:
            ops.decode_attn(q, d, self.kd, 64, H * Tg * 64, self.vd, 64, H * Tg * 64, o, d, B, H, Tk, 0.125,
                            hsk=Tg * 64, hsv=Tg * 64, k_start=self._ks())
        else:
            ops.decode_attn_mq(q, Q * d, d, self.kd, 64, H * Tg * 64, self.vd, 64, H * Tg * 64, o, Q * d, d, B, H, Q,
                               Tk, 0.125, hsk=Tg * 64, hsv=Tg * 64, k_start=self._ks())
        return o


def _q(B, Q, H, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Q, H * 64, generator=g) * 2).to(dt).to(DEV)


def _check(c, q):
    ref = c.ref(q.cpu())
    o8, o16 = c.run_fp8(q).double().cpu(), c.run_16(q).double().cpu()
    top = float(ref.abs().max())
    e_ref, e_16 = float((o8 - ref).abs().max()), float((o8 - o16).abs().max())
    print(f"max|ref| {top:.4g}  |fp8 - fp64| {e_ref:.3g} (bar {2 ** -7 * top + 1e-3:.3g})  "
          f"|fp8 - 16-bit| {e_16:.3g} (bar {2 * U[c.dt] * top:.3g})")
    assert bool(torch.isfinite(o8).all())                   # no NaN byte of a guard or masked row was read
    assert e_ref <= 2 ** -7 * top + 1e-3
    assert e_16 <= 2 * U[c.dt] * top


SINGLE = [  # B, H, Tk, starts
    (2, 3, 1, None),                                         # one workgroup: a single key
    (2, 3, 70, [0, 69]),                                     # more than one wave iteration; a start at the last key
    (33, 20, 257, None),                                     # 660 pairs: one workgroup per pair past the split rule
    (1, 20, 1500, None),                                     # split: 12 chunks, the last one short
    (2, 20, 230, [128 + 9, 17]),                             # split: k_start inside both chunks
]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,H,Tk,starts", SINGLE)
def test_attention_per_element(B, H, Tk, starts, dt):
    c = Cache(B, H, Tk, dt, seed=B * 1000 + Tk, starts=starts)
    _check(c, _q(B, 1, H, dt, seed=Tk))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q", [1, 3, 8])
@pytest.mark.parametrize("B,H,Tk", [(1, 20, 1500), (1, 4, 70)])
def test_multi_query_per_element(B, H, Tk, Q, dt):
    from tw import ops
    c = Cache(B, H, Tk, dt, seed=Tk + Q)
    q = _q(B, Q, H, dt, seed=Q)
    ref = c.ref(q.cpu())
    Tg, d = c.Tg, H * 64
    o = torch.full_like(q, float("nan"))
    ops.decode_attn_mq_fp8(q, Q * d, d, c.kb, 64, H * Tg * 64, c.vb, 64, H * Tg * 64, c.skd, c.svd, H, o, Q * d, d, B,
                           H, Q, Tk, 0.125, hsk=Tg * 64, hsv=Tg * 64)
    o16 = torch.full_like(q, float("nan"))
    ops.decode_attn_mq(q, Q * d, d, c.kd, 64, H * Tg * 64, c.vd, 64, H * Tg * 64, o16, Q * d, d, B, H, Q, Tk, 0.125,
                       hsk=Tg * 64, hsv=Tg * 64)
    top = float(ref.abs().max())
    assert bool(torch.isfinite(o).all())
    assert float((o.double().cpu() - ref).abs().max()) <= 2 ** -7 * top + 1e-3
    assert float((o.double() - o16.double()).abs().max()) <= 2 * U[dt] * top
    # each query is the single-query call's result, bit for bit
    for j in range(Q):
        assert torch.equal(o[:, j:j + 1], c.run_fp8(q[:, j:j + 1].contiguous()))


# ------------------------------------------------------------------------------------------ bit-identities
@pytest.mark.parametrize("B,H,Tk", [(5, 4, 70), (3, 20, 1500), (40, 20, 200)])
def test_shared_block_equals_per_row_copies(B, H, Tk):
    """Batch stride 0 over one clip's blocks and scales (DecodeSession's shared mode) == B copies read as B*H
    one-head clips (its per-row mode), on the one-workgroup and the split path; and a rerun is identical."""
    from tw import ops
    dt = torch.bfloat16
    c = Cache(1, H, Tk, dt, seed=B + Tk)
    Tg, d, n1 = c.Tg, H * 64, H * (Tk + PAD) * 64
    q = _q(B, 1, H, dt, seed=B)
    o1 = torch.full_like(q, float("nan"))
    ops.decode_attn_fp8(q, d, c.kb, 64, 0, c.vb, 64, 0, c.skd, c.svd, 0, o1, d, B, H, Tk, 0.125, hsk=Tg * 64,
                        hsv=Tg * 64)
    kr, vr = c.kb.repeat(B, 1, 1, 1), c.vb.repeat(B, 1, 1, 1)
    sk, sv = c.skd.repeat(B, 1).contiguous(), c.svd.repeat(B, 1).contiguous()
    o2 = torch.full_like(q, float("nan"))
    ops.decode_attn_fp8(q, 64, kr, 64, Tg * 64, vr, 64, Tg * 64, sk, sv, 1, o2, 64, B * H, 1, Tk, 0.125)
    o3 = torch.full_like(q, float("nan"))
    ops.decode_attn_fp8(q, 64, kr, 64, Tg * 64, vr, 64, Tg * 64, sk, sv, 1, o3, 64, B * H, 1, Tk, 0.125)
    assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2) and torch.equal(o2, o3)
    assert n1 == c.kb.numel()


def test_k_start_row_equals_the_single_row_call_advanced():
    from tw import ops
    dt, B, H, Tk, starts = torch.float16, 3, 2, 100, [0, 17, 99]
    c = Cache(B, H, Tk, dt, seed=11, starts=starts)
    q = _q(B, 1, H, dt, seed=4)
    o = c.run_fp8(q)
    Tg, d = c.Tg, H * 64
    for b, s in enumerate(starts):
        ob = torch.full((1, 1, d), float("nan"), dtype=dt, device=DEV)
        ops.decode_attn_fp8(q[b], d, c.kb[b, :, s:], 64, 0, c.vb[b, :, s:], 64, 0, c.skd[b], c.svd[b], 0, ob, d, 1, H,
                            Tk - s, 0.125, hsk=Tg * 64, hsv=Tg * 64)
        assert torch.equal(ob[0], o[b]), b


# ------------------------------------------------------------------------------------------ status codes
def test_status_codes():
    from tw import _native, ops
    c = Cache(1, 2, 5, torch.bfloat16, seed=2)
    q = _q(1, 1, 2, torch.bfloat16, seed=2)
    o = torch.empty_like(q)
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    lib = _native.lib()
    hs = c.Tg * 64

    def sq(ks, vs, tk_dev, dtype=ops.BF16):
        return lib.tw_decode_attn_fp8(q.data_ptr(), 128, c.kb.data_ptr(), 64, 2 * hs, hs, c.vb.data_ptr(), 64, 2 * hs,
                                      hs, ks, vs, 2, o.data_ptr(), 128, 1, 2, 5, tk_dev, None, 64, 0.125, dtype, st)

    def mq(ks, vs, tk_dev, Q=2):
        return lib.tw_decode_attn_mq_fp8(q.data_ptr(), 128, 0, c.kb.data_ptr(), 64, 2 * hs, hs, c.vb.data_ptr(), 64,
                                         2 * hs, hs, ks, vs, 2, o.data_ptr(), 128, 0, 1, 2, Q, 5, tk_dev, None, 0, 64,
                                         0.125, ops.BF16, st)

    ks, vs = c.skd.data_ptr(), c.svd.data_ptr()
    assert sq(ks, vs, None) == 0 and mq(ks, vs, None) == 0
    assert sq(ks, vs, t_dev.data_ptr()) == 2 and mq(ks, vs, t_dev.data_ptr()) == 2      # fixed Tk only
    assert sq(None, vs, None) == 1 and sq(ks, None, None) == 1 and mq(None, vs, None) == 1
    assert sq(ks, vs, None, ops.F32) == 2 and mq(ks, vs, None, Q=9) == 1
    torch.cuda.synchronize()
