"""Variable-length (packed rows) attention, tw_attn_{fwd,bwd}_varlen[_f16], against the dense entry points called one
clip at a time (B = 1, Tq = n_b).  The packed kernels walk each clip's key / query tiles in the dense kernels' order,
so O, LSE, dQ, dK and dV must be bit-identical; a clip without queries gets an all-zero dK / dV block against dense
keys; rows of the packed outputs past M keep their guard values.

Lengths [1, 37, 64, 130, 0]: a single row, a partial wave, exactly one 64-key tile, a clip that crosses the 128-query
workgroup block and the 64-key tile, and an empty clip.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [1, 37, 64, 130, 0]
H, HD = 2, 64
D = H * HD
GUARD = 8          # extra rows behind every packed output
SCALE = 0.125


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rand(shape, dtype, g):
    return torch.randn(shape, generator=g).to(dtype).cuda()


def _guarded(rows, cols, dtype):
    """[rows + GUARD, cols] filled with a recognisable value; -> (buffer, its untouched copy)."""
    t = torch.full((rows + GUARD, cols), -7.0, dtype=dtype, device="cuda")
    return t, t.clone()


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: not bit-identical, max |d| " \
                                            f"{float((a.float() - b.float()).abs().max()):.3e}"


def _offsets():
    off = [0]
    for n in LENS:
        off.append(off[-1] + n)
    return off, torch.tensor(off, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_causal_self_attention_packed(dtype):
    from tw import ops
    g = torch.Generator().manual_seed(11)
    off, offd = _offsets()
    B, M, mx = len(LENS), off[-1], max(LENS)
    qkv = _rand((M, 3 * D), dtype, g)
    do = _rand((M, D), dtype, g)
    o, o0 = _guarded(M, D, dtype)
    lse = torch.full((H * M + GUARD,), -7.0, device="cuda")
    ops.attn_fwd_varlen(qkv, 3 * D, qkv[:, D:], 3 * D, qkv[:, 2 * D:], 3 * D, o, D, lse, offd, offd, B, H, M, mx, mx,
                        True, SCALE)
    dqkv, dqkv0 = _guarded(M, 3 * D, dtype)
    ops.attn_bwd_varlen(qkv, 3 * D, qkv[:, D:], 3 * D, qkv[:, 2 * D:], 3 * D, o, D, do, D, lse, dqkv, 3 * D,
                        dqkv[:, D:], 3 * D, dqkv[:, 2 * D:], 3 * D, offd, offd, B, H, M, mx, mx, True, SCALE)
    torch.cuda.synchronize()
    _same(o[M:], o0[M:], "O guard rows")
    _same(dqkv[M:], dqkv0[M:], "dQKV guard rows")
    assert bool((lse[H * M:] == -7.0).all()), "LSE guard"
    for b, n in enumerate(LENS):
        if n == 0:
            continue
        r = slice(off[b], off[b + 1])
        x = qkv[r]
        ro = torch.empty(n, D, dtype=dtype, device="cuda")
        rl = torch.empty(H * n, device="cuda")
        ops.attn_fwd(x, 3 * D, x[:, D:], 3 * D, x[:, 2 * D:], 3 * D, ro, D, rl, 1, H, n, n, True, SCALE)
        rd = torch.empty(n, 3 * D, dtype=dtype, device="cuda")
        ops.attn_bwd(x, 3 * D, x[:, D:], 3 * D, x[:, 2 * D:], 3 * D, ro, D, do[r], D, rl, rd, 3 * D, rd[:, D:], 3 * D,
                     rd[:, 2 * D:], 3 * D, 1, H, n, n, True, SCALE)
        torch.cuda.synchronize()
        _same(o[r], ro, f"clip {b} O")
        _same(lse[: H * M].view(H, M)[:, r], rl.view(H, n), f"clip {b} LSE")
        for nm, c in (("dQ", 0), ("dK", 1), ("dV", 2)):
            _same(dqkv[r, c * D:(c + 1) * D], rd[:, c * D:(c + 1) * D], f"clip {b} {nm}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cross_attention_packed_queries_dense_keys(dtype):
    from tw import ops
    g = torch.Generator().manual_seed(12)
    off, offd = _offsets()
    B, M, mx, Tk = len(LENS), off[-1], max(LENS), 70
    q = _rand((M, D), dtype, g)
    kv = _rand((B * Tk, 2 * D), dtype, g)
    do = _rand((M, D), dtype, g)
    o, o0 = _guarded(M, D, dtype)
    lse = torch.full((H * M + GUARD,), -7.0, device="cuda")
    ops.attn_fwd_varlen(q, D, kv, 2 * D, kv[:, D:], 2 * D, o, D, lse, offd, None, B, H, M, mx, Tk, False, SCALE)
    dq, dq0 = _guarded(M, D, dtype)
    dkv, dkv0 = _guarded(B * Tk, 2 * D, dtype)
    ops.attn_bwd_varlen(q, D, kv, 2 * D, kv[:, D:], 2 * D, o, D, do, D, lse, dq, D, dkv, 2 * D, dkv[:, D:], 2 * D,
                        offd, None, B, H, M, mx, Tk, False, SCALE)
    torch.cuda.synchronize()
    _same(o[M:], o0[M:], "O guard rows")
    _same(dq[M:], dq0[M:], "dQ guard rows")
    _same(dkv[B * Tk:], dkv0[B * Tk:], "dKV guard rows")
    assert bool((lse[H * M:] == -7.0).all()), "LSE guard"
    for b, n in enumerate(LENS):
        kb = kv[b * Tk:(b + 1) * Tk]
        if n == 0:
            assert not bool(_bits(dkv[b * Tk:(b + 1) * Tk]).any()), f"clip {b}: dK / dV of a clip without queries"
            continue
        r = slice(off[b], off[b + 1])
        ro = torch.empty(n, D, dtype=dtype, device="cuda")
        rl = torch.empty(H * n, device="cuda")
        ops.attn_fwd(q[r], D, kb, 2 * D, kb[:, D:], 2 * D, ro, D, rl, 1, H, n, Tk, False, SCALE)
        rq = torch.empty(n, D, dtype=dtype, device="cuda")
        rkv = torch.empty(Tk, 2 * D, dtype=dtype, device="cuda")
        ops.attn_bwd(q[r], D, kb, 2 * D, kb[:, D:], 2 * D, ro, D, do[r], D, rl, rq, D, rkv, 2 * D, rkv[:, D:], 2 * D,
                     1, H, n, Tk, False, SCALE)
        torch.cuda.synchronize()
        _same(o[r], ro, f"clip {b} O")
        _same(lse[: H * M].view(H, M)[:, r], rl.view(H, n), f"clip {b} LSE")
        _same(dq[r], rq, f"clip {b} dQ")
        _same(dkv[b * Tk:(b + 1) * Tk, :D], rkv[:, :D], f"clip {b} dK")
        _same(dkv[b * Tk:(b + 1) * Tk, D:], rkv[:, D:], f"clip {b} dV")
