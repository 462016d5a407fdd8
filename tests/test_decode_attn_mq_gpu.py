"""tw_decode_attn_mq (the verify pass of assisted decoding: Q consecutive query rows per batch row, each K / V row
loaded once) against tw_decode_attn_ks: every query's output is bit-identical to the single-query entry called on
that query alone with its own key limit -- bf16, fp16 and fp32; causal over a device-side length (the one-workgroup
kernel) and non-causal over a fixed Tk (one workgroup at Tk = 8, the split + combine path at 130 and 1500) in both
head-major layouts; zero and non-zero key starts, a start at or past a query's limit included.  The K / V rows at or
above the last query's limit and below every query's start hold NaN throughout: they are never loaded."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
H = 2
D = H * 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    assert not bool(torch.isnan(a.float()).any()) and not bool(torch.isnan(b.float()).any())
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Q", [1, 2, 5, 8])
def test_causal_device_length(dt, Q):
    """Self-attention shape: query j of a row attends keys [start, L + j), L - 1 read from the device."""
    from tw import ops
    g = torch.Generator().manual_seed(17 * Q + 3)
    for B in (1, 2):
        for L in (1, 7, 8, 9, 130):
            Tmax = L + Q + 3
            last = L + Q - 1                                     # the last query's limit
            q = torch.randn(B, Q, D, generator=g).to(dt).to(DEV)
            k = torch.randn(B, Tmax, D, generator=g).to(dt).to(DEV)
            v = torch.randn(B, Tmax, D, generator=g).to(dt).to(DEV)
            for starts in ([0] * B, [min(3, L - 1), 0][:B], [L, L + 1][:B]):
                kp, vp = k.clone(), v.clone()
                for t in (kp, vp):
                    t[:, last:] = float("nan")
                    for b in range(B):                           # query 0 has the lowest clamped start: min(s, L - 1)
                        t[b, :min(starts[b], L - 1)] = float("nan")
                ks = torch.tensor(starts, dtype=torch.int32, device=DEV)
                t_dev = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
                o = torch.full((B, Q, D), float("nan"), dtype=dt, device=DEV)
                ops.decode_attn_mq(q, Q * D, D, kp, D, Tmax * D, vp, D, Tmax * D, o, Q * D, D, B, H, Q, 1, 0.125,
                                   tk_dev=t_dev, tk_max=Tmax, k_start=ks, causal=True)
                for j in range(Q):
                    tj = torch.tensor([L - 1 + j], dtype=torch.int32, device=DEV)
                    ref = torch.empty(B, D, dtype=dt, device=DEV)
                    ops.decode_attn(q[:, j], Q * D, k, D, Tmax * D, v, D, Tmax * D, ref, D, B, H, 1, 0.125,
                                    tk_dev=tj, tk_max=Tmax, k_start=ks)
                    assert _same(o[:, j], ref), (B, L, starts, j)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Q", [1, 2, 5, 8])
@pytest.mark.parametrize("Tk", [8, 130, 1500])
def test_cross_fixed_tk(dt, Q, Tk):
    """Cross-attention shape: every query attends keys [start, Tk) of head-major K / V blocks, one clip's blocks
    shared by the rows (batch stride 0) or a block set per row; two NaN rows behind every head's Tk rows."""
    from tw import ops
    g = torch.Generator().manual_seed(Tk * 31 + Q)
    hs = (Tk + 2) * 64
    for B in (1, 2):
        for shared in (True, False):
            nb = 1 if shared else B
            q = torch.randn(B, Q, D, generator=g).to(dt).to(DEV)
            k = torch.randn(nb, H, Tk + 2, 64, generator=g).to(dt).to(DEV)
            v = torch.randn(nb, H, Tk + 2, 64, generator=g).to(dt).to(DEV)
            sb = 0 if shared else H * hs
            for starts in ([0] * B, [5, Tk + 3][:B]):
                kp, vp = k.clone(), v.clone()
                for t in (kp, vp):
                    t[:, :, Tk:] = float("nan")
                    if not shared:
                        for b in range(B):
                            t[b, :, :min(starts[b], Tk - 1)] = float("nan")
                    else:
                        t[:, :, :min(min(s, Tk - 1) for s in starts)] = float("nan")
                ks = torch.tensor(starts, dtype=torch.int32, device=DEV)
                o = torch.full((B, Q, D), float("nan"), dtype=dt, device=DEV)
                ops.decode_attn_mq(q, Q * D, D, kp, 64, sb, vp, 64, sb, o, Q * D, D, B, H, Q, Tk, 0.125, hsk=hs, hsv=hs,
                                   k_start=ks)
                for j in range(Q):
                    ref = torch.empty(B, D, dtype=dt, device=DEV)
                    ops.decode_attn(q[:, j], Q * D, k, 64, sb, v, 64, sb, ref, D, B, H, Tk, 0.125, hsk=hs, hsv=hs,
                                    k_start=ks)
                    assert _same(o[:, j], ref), (B, shared, starts, j)
            # no start array: every start 0
            o0 = torch.full((B, Q, D), float("nan"), dtype=dt, device=DEV)
            ops.decode_attn_mq(q, Q * D, D, k, 64, sb, v, 64, sb, o0, Q * D, D, B, H, Q, Tk, 0.125, hsk=hs, hsv=hs)
            ref = torch.empty(B, D, dtype=dt, device=DEV)
            ops.decode_attn(q[:, Q - 1], Q * D, k, 64, sb, v, 64, sb, ref, D, B, H, Tk, 0.125, hsk=hs, hsv=hs)
            assert _same(o0[:, Q - 1], ref)


def test_against_fp64_reference():
    """An independent check of the values themselves (the bit-identity above is against the engine's own kernel):
    fp32, Q = 5, causal, vs softmax attention in fp64."""
    from tw import ops
    g = torch.Generator().manual_seed(5)
    B, Q, L = 2, 5, 9
    Tmax = L + Q
    q = torch.randn(B, Q, D, generator=g)
    k = torch.randn(B, Tmax, D, generator=g)
    v = torch.randn(B, Tmax, D, generator=g)
    o = torch.empty(B, Q, D, device=DEV)
    t_dev = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
    ops.decode_attn_mq(q.to(DEV), Q * D, D, k.to(DEV), D, Tmax * D, v.to(DEV), D, Tmax * D, o, Q * D, D, B, H, Q, 1,
                       0.125, tk_dev=t_dev, tk_max=Tmax, causal=True)
    for j in range(Q):
        n = L + j
        qq = q[:, j].double().view(B, H, 64)
        kk = k[:, :n].double().view(B, n, H, 64).transpose(1, 2)
        vv = v[:, :n].double().view(B, n, H, 64).transpose(1, 2)
        s = torch.einsum("bhe,bhke->bhk", qq, kk) * 0.125
        ref = torch.einsum("bhk,bhke->bhe", torch.softmax(s, -1), vv).reshape(B, D)
        assert float((o[:, j].double().cpu() - ref).abs().max()) <= 1e-5


@pytest.mark.parametrize("Q,hd", [(0, 64), (9, 64), (2, 32)])
def test_invalid_arguments_launch_nothing(Q, hd):
    from tw import ops
    q = torch.zeros(1, 8, D, device=DEV)
    k = torch.zeros(1, 16, D, device=DEV)
    o = torch.full((1, 8, D), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"status [12]"):
        ops.decode_attn_mq(q, 8 * D, D, k, D, 16 * D, k, D, 16 * D, o, 8 * D, D, 1, H, Q, 8, 0.125, head_dim=hd)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
