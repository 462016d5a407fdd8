"""tw_quant_rows_fp8 and tw_gemv_w8_bf16 / tw_gemv_w8_f16 (csrc/gemv_w8.hip) on the GPU, against the format's CPU
restatement (tests/w8_cases.py) and the fp64 product of the dequantised operands."""
import pytest
import torch

import w8_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
_W = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _weights(N, K, dt):
    """weight_cases(N, K) once per shape and dtype: (W16 cpu, planted rows, bytes dev, scales dev, dequantised fp64
    cpu) -- the bytes and scales are the CPU restatement's, so the GEMV tests do not lean on the quantiser kernel."""
    key = (N, K, dt)
    if key not in _W:
        W, rows = wc.weight_cases(N, K, dt, seed=N + K)
        q, s = wc.quantise_rows_ref(W)
        _W[key] = (W, rows, q.view(torch.uint8).to(DEV), s.to(DEV), wc.dequantise_rows_ref(q, s).double())
    return _W[key]


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,K", [(5, 256), (520, 1280), (3, 5120), (1, 16)])
def test_quantiser_matches_the_restatement(N, K, dt):
    from tw import ops
    W, rows, q_ref, s_ref, _ = _weights(N, K, dt)
    q = torch.full((N, K), 0x55, dtype=torch.uint8, device=DEV)
    s = torch.full((N,), -3.0, device=DEV)
    ops.quant_rows_fp8(W.to(DEV), q, s)
    bad = torch.isnan(s_ref)
    assert torch.equal(torch.isnan(s), bad)                                 # a NaN scale compares by isnan
    assert torch.equal(s[~bad], s_ref[~bad])
    assert torch.equal(q[~bad], q_ref[~bad])
    assert bool(((q[bad] & 0x7f) == 0x7f).all())            # a NaN-scale row: NaN bytes (their sign is left open)
    for kind in ("inf", "nan"):
        if kind in rows:
            assert bool(bad[rows[kind]])
    # strided source and destination rows (ld > K, multiples of 16 B)
    if N > 1:
        src = torch.zeros(N, K + 8, dtype=dt, device=DEV)
        src[:, :K] = W.to(DEV)
        dst = torch.full((N, K + 16), 0x55, dtype=torch.uint8, device=DEV)
        ops.quant_rows_fp8(src[:, :K], dst[:, :K], s)
        assert torch.equal(dst[:, :K][~bad], q_ref[~bad]) and bool((dst[:, K:] == 0x55).all())


def test_quantiser_error_returns():
    from tw._native import lib
    f = lib().tw_quant_rows_fp8
    st = torch.cuda.current_stream().cuda_stream
    src = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    s32 = torch.zeros(4, 64, dtype=torch.float32, device=DEV)
    dst = torch.zeros(4, 64, dtype=torch.uint8, device=DEV)
    sc = torch.zeros(4, device=DEV)
    BF16, F16, F32 = 1, 2, 0
    assert f(src.data_ptr(), 64, BF16, 4, 64, dst.data_ptr(), 64, sc.data_ptr(), st) == 0
    assert f(src.data_ptr(), 64, F16, 4, 64, dst.data_ptr(), 64, sc.data_ptr(), st) == 0
    assert f(s32.data_ptr(), 64, F32, 4, 64, dst.data_ptr(), 64, sc.data_ptr(), st) == 2          # fp32
    assert f(None, 64, BF16, 4, 64, dst.data_ptr(), 64, sc.data_ptr(), st) == 1                   # null pointers
    assert f(src.data_ptr(), 64, BF16, 4, 64, None, 64, sc.data_ptr(), st) == 1
    assert f(src.data_ptr(), 64, BF16, 4, 64, dst.data_ptr(), 64, None, st) == 1
    assert f(src.data_ptr() + 2, 64, BF16, 3, 48, dst.data_ptr(), 64, sc.data_ptr(), st) == 1     # misaligned
    assert f(src.data_ptr(), 64, BF16, 3, 48, dst.data_ptr() + 8, 64, sc.data_ptr(), st) == 1
    assert f(src.data_ptr(), 64, BF16, 4, 24, dst.data_ptr(), 64, sc.data_ptr(), st) == 1         # K % 16
    assert f(src.data_ptr(), 68, BF16, 3, 48, dst.data_ptr(), 64, sc.data_ptr(), st) == 1         # strides: 16 B
    assert f(src.data_ptr(), 64, BF16, 3, 48, dst.data_ptr(), 72, sc.data_ptr(), st) == 1
    torch.cuda.synchronize()
    assert bool((dst == 0).all())


# ------------------------------------------------------------------------------------------------ GEMV value
SHAPES = [(1, 8, 256), (3, 520, 256), (2, 3840, 1280), (4, 1280, 5120), (8, 1280, 1280), (1, 51865, 1280),
          (5, 51904, 1280)]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemv_value(M, N, K, dt):
    """fp32 C, no ROUND, no bias against the fp64 product of the dequantised operands: per element
    |err| <= (K/64 + 8) * 2^-24 * sum_k |w_k a_k| (each lane's FMA chain, the 6 butterfly additions, an exact
    scale); the rounded 16-bit output with a bias at the bar of the 16-bit kernel's own tests; a NaN-scale row makes
    exactly its own output column NaN; and the scales commute: every scale times 8 gives exactly 8 x the output."""
    from tw import ops
    W, rows, q, s, deq = _weights(N, K, dt)
    ok = wc.finite_rows(rows, N)
    g = torch.Generator().manual_seed(M * 7 + N + K)
    x = (torch.randn(M, K, generator=g) * 2 + 0.5).to(dt)
    b = (torch.randn(N, generator=g) * 0.1).to(dt)
    xd, bd = x.to(DEV), b.to(DEV)
    C = torch.full((M, N), 7.0, device=DEV)
    ops.gemv_w8(xd, q, s, C)
    Cc = C.cpu()
    assert torch.equal(torch.isnan(Cc), (~ok)[None, :].expand(M, N))        # exactly the NaN-scale columns
    ref = x.double() @ deq[ok].t()
    mag = x.double().abs() @ deq[ok].abs().t()
    err = (Cc[:, ok].double() - ref).abs()
    bound = (K / 64 + 8) * 2.0 ** -24 * mag
    print(f"({M}, {N}, {K}) {dt}: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    # scales x 8 -> exactly 8 x the output
    C8 = torch.empty_like(C)
    ops.gemv_w8(xd, q, s * 8, C8)
    assert torch.equal(C8.cpu()[:, ok], Cc[:, ok] * 8)
    # rounded 16-bit output with the bias
    C16 = torch.empty(M, N, dtype=dt, device=DEV)
    ops.gemv_w8(xd, q, s, C16, bias=bd, flags=ops.GEMM_ROUND)
    want = ref + b.double()[ok]
    e16 = (C16.cpu()[:, ok].double() - want).abs()
    if dt == torch.bfloat16:        # tests/test_kernels_gpu.py::test_gemv_decode: one bf16 ulp + 1e-5
        assert bool((e16 <= 2 ** -8 * want.abs() + 1e-5).all()), float(e16.max())
    else:                           # tests/test_fp16_gpu.py's _ulps(got, fp16(ref), mag) <= 1: the fp32 order noise
        want = want.half().double()                 # 2^-16 * mag forgiven, then one fp16 ulp of the rounded reference
        d = ((C16.cpu()[:, ok].double() - want).abs() - 2.0 ** -16 * (mag + b.double().abs()[ok])).clamp_min(0)
        ulps = d / 2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -14))) - 10)
        assert float(ulps.max()) <= 1.0, float(ulps.max())


# ------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,K,ln", [(1280, 1280, True), (3840, 1280, False), (1280, 5120, False), (51865, 1280, True)])
def test_gemv_rows_independent_of_batch(dt, N, K, ln):
    """tests/test_kernels_gpu.py::test_gemv_rows_independent_of_batch for the w8 entries: each row of an M-row call
    (M = 2..8) is bit-identical to the row computed alone, with round + GELU and with the residual."""
    from tw import ops
    W, rows, q, s, _ = _weights(N, K, dt)
    g = torch.Generator().manual_seed(N + K)
    x = (torch.randn(8, K, generator=g) * 2 + 0.3).to(dt).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(dt).to(DEV)
    r = (torch.randn(8, N, generator=g)).to(dt).to(DEV)
    lw, lb = (torch.randn(K, generator=g) * 0.2 + 1).to(DEV), (torch.randn(K, generator=g) * 0.1).to(DEV)
    kw = dict(ln_w=lw, ln_b=lb) if ln else {}
    ok = wc.finite_rows(rows, N).to(DEV)

    def same(a, c):      # bit-identical finite columns; a NaN-scale column is NaN in both (its payload is not stated)
        return torch.equal(a[:, ok], c[:, ok]) and bool(torch.isnan(a[:, ~ok]).all() and torch.isnan(c[:, ~ok]).all())
    for flags, res in ((ops.GEMM_ROUND | ops.GEMM_GELU, None), (ops.GEMM_ROUND, r)):
        one = torch.empty(8, N, dtype=dt, device=DEV)
        for i in range(8):
            ops.gemv_w8(x[i:i + 1], q, s, one[i:i + 1], bias=b, flags=flags,
                        res=None if res is None else res[i:i + 1], **kw)
        for M in range(2, 9):
            C = torch.empty(M, N, dtype=dt, device=DEV)
            ops.gemv_w8(x[:M], q, s, C, bias=b, flags=flags, res=None if res is None else res[:M], **kw)
            assert same(C, one[:M]), (M, flags)


# ------------------------------------------------------------------------------------------------ fused steps
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N,K", [(1, 1280, 1280), (3, 520, 256), (2, 3840, 1280), (4, 1280, 5120), (8, 1280, 1280)])
def test_gemv_fused_steps(M, N, K, dt):
    """The steps of tests/test_kernels_gpu.py::test_gemv_decode for the w8 entries: LN-fused == LN kernel + plain
    call, the fused KV append writes exactly row t, the GELU aux out is the pre-activation, the in-place residual on
    a 16-bit and an fp32 stream."""
    from tw import ops
    W, rows, q, s, _ = _weights(N, K, dt)
    ok = wc.finite_rows(rows, N).to(DEV)
    g = torch.Generator().manual_seed(M + N + K)
    xd = (torch.randn(M, K, generator=g) * 2 + 0.5).to(dt).to(DEV)
    bd = (torch.randn(N, generator=g) * 0.1).to(dt).to(DEV)
    lwd, lbd = (torch.randn(K, generator=g) * 0.2 + 1).to(DEV), (torch.randn(K, generator=g) * 0.1).to(DEV)
    nan_cols = lambda a: bool(torch.isnan(a[..., ~ok]).all())
    same = lambda a, c: torch.equal(a[..., ok], c[..., ok]) and nan_cols(a) and nan_cols(c)
    y = torch.empty_like(xd)
    C2 = torch.empty(M, N, dtype=dt, device=DEV)
    if K <= 1280:
        ops.layernorm_fwd(xd, lwd, lbd, y)
        C1 = torch.empty_like(C2)
        ops.gemv_w8(xd, q, s, C1, ln_w=lwd, ln_b=lbd, bias=bd, flags=ops.GEMM_ROUND)
        ops.gemv_w8(y, q, s, C2, bias=bd, flags=ops.GEMM_ROUND)
        assert same(C1, C2)
    else:
        y.copy_(xd)
        ops.gemv_w8(y, q, s, C2, bias=bd, flags=ops.GEMM_ROUND)
    # fused KV-cache append: columns >= col0 also land in row t, and nowhere else
    col0, Tm, t = N // 3 // 8 * 8, 9, 5
    cache = torch.zeros(M, Tm, N - col0, dtype=dt, device=DEV)
    tdev = torch.tensor([t], dtype=torch.int32, device=DEV)
    C3 = torch.empty_like(C2)
    ops.gemv_w8(y, q, s, C3, bias=bd, flags=ops.GEMM_ROUND, kv=(cache, Tm * (N - col0), N - col0, col0, tdev, Tm))
    assert same(C3, C2)
    okc = ok[col0:]
    assert torch.equal(cache[:, t][:, okc], C2[:, col0:][:, okc]) and bool(torch.isnan(cache[:, t][:, ~okc]).all())
    assert bool((cache[:, :t] == 0).all()) and bool((cache[:, t + 1:] == 0).all())
    # GELU with the pre-activation output
    h = torch.empty(M, N, dtype=dt, device=DEV)
    pre = torch.empty_like(h)
    ops.gemv_w8(y, q, s, h, bias=bd, aux=pre, flags=ops.GEMM_ROUND | ops.GEMM_GELU | ops.GEMM_AUX_OUT)
    assert same(pre, C2)
    gl = torch.nn.functional.gelu(pre.float()[:, ok])
    tol = 2 ** -7 if dt == torch.bfloat16 else 2 ** -10
    assert bool(((h.float()[:, ok] - gl).abs() <= torch.maximum(gl.abs() * tol, torch.full_like(gl, 1e-6))).all())
    # residual, in place, 16-bit and fp32 streams
    if N == K:
        for rt in (dt, torch.float32):
            r = torch.randn(M, N, generator=g).to(rt).to(DEV)
            r0 = r.clone()
            ops.gemv_w8(y, q, s, r, bias=bd, res=r, flags=ops.GEMM_ROUND)
            want = C2.float() + r0.float()
            got = r.float()
            if rt == torch.float32:
                assert torch.equal(got[:, ok], want[:, ok])              # one exact fp32 add of two 16-bit-ish values
            else:
                assert torch.equal(got[:, ok], want.to(rt).float()[:, ok])      # one rounding of the sum
