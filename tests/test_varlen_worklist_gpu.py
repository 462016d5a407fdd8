"""Packed-row attention over a query-block list (tw_pack_blocks, tw_attn_{fwd,bwd}_blocks[_f16]): only blocks that have
rows are launched and the placement of the workgroups follows the list.  None of that may reach the results: O, LSE,
dQ and D (and dK, dV) of every clip must equal the dense entry called on that clip alone (B = 1) bit for bit, whatever
the order of the clips.

H = 2, head dim 64.  Lengths [0, 1, 16, 63, 64, 65, 128, 129, 200] in one call: a clip without rows; short tails
around a wave's 32 rows and the 64-key tile (1, 16, 63, 64, 65; 129 leaves a one-row tail behind a full block); a clip
whose last block is exactly full (128); clips of two blocks (129, 200).  (A half-height forward for tails of at most
64 rows was measured and left out -- DESIGN.md §4 -- so the list has one part.)  Cross-attention has Tk = 70 (two key
tiles, the second with a masked tail); self-attention is causal.  The second call of every case holds the same clips in reversed order.  The dense per-clip results are computed once
per (kind, dtype) and shared.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [0, 1, 16, 63, 64, 65, 128, 129, 200]
H, HD, TK = 2, 64, 70
D = H * HD
GUARD = 8
SCALE = 0.125


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: not bit-identical, max |d| " \
                                            f"{float((a.float() - b.float()).abs().max()):.3e}"


@functools.lru_cache(maxsize=None)
def _clips(causal, dtype):
    """Per clip (in LENS order): its inputs and the dense entries' results on it alone.  Causal: q, k, v are the
    columns of one [n, 3D] matrix; cross: q [n, D] against kv [TK, 2D]."""
    from tw import ops
    g = torch.Generator().manual_seed(21 + int(causal))
    out = []
    for n in LENS:
        c = {"n": n}
        if causal:
            c["qkv"] = torch.randn((n, 3 * D), generator=g).to(dtype).cuda()
        else:
            c["q"] = torch.randn((n, D), generator=g).to(dtype).cuda()
            c["kv"] = torch.randn((TK, 2 * D), generator=g).to(dtype).cuda()
        c["do"] = torch.randn((n, D), generator=g).to(dtype).cuda()
        if n:
            o = torch.empty(n, D, dtype=dtype, device="cuda")
            lse = torch.empty(H * n, device="cuda")
            dd = torch.empty(H * n, device="cuda")
            if causal:
                x = c["qkv"]
                ops.attn_fwd(x, 3 * D, x[:, D:], 3 * D, x[:, 2 * D:], 3 * D, o, D, lse, 1, H, n, n, True, SCALE)
                dx = torch.empty(n, 3 * D, dtype=dtype, device="cuda")
                ops.attn_bwd(x, 3 * D, x[:, D:], 3 * D, x[:, 2 * D:], 3 * D, o, D, c["do"], D, lse, dx, 3 * D,
                             dx[:, D:], 3 * D, dx[:, 2 * D:], 3 * D, 1, H, n, n, True, SCALE, workspace=dd)
                c.update(dq=dx[:, :D], dk=dx[:, D:2 * D], dv=dx[:, 2 * D:])
            else:
                q, kv = c["q"], c["kv"]
                ops.attn_fwd(q, D, kv, 2 * D, kv[:, D:], 2 * D, o, D, lse, 1, H, n, TK, False, SCALE)
                dq = torch.empty(n, D, dtype=dtype, device="cuda")
                dkv = torch.empty(TK, 2 * D, dtype=dtype, device="cuda")
                ops.attn_bwd(q, D, kv, 2 * D, kv[:, D:], 2 * D, o, D, c["do"], D, lse, dq, D, dkv, 2 * D, dkv[:, D:],
                             2 * D, 1, H, n, TK, False, SCALE, workspace=dd)
                c.update(dq=dq, dk=dkv[:, :D], dv=dkv[:, D:])
            c.update(o=o, lse=lse.view(H, n), dd=dd.view(H, n))
        out.append(c)
    torch.cuda.synchronize()
    return out


def _guarded(rows, cols, dtype):
    return torch.full((rows + GUARD, cols), -7.0, dtype=dtype, device="cuda")


@pytest.mark.parametrize("order", ["given", "reversed"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal_self", "cross"])
def test_block_list_results_equal_dense_per_clip(causal, dtype, order):
    from tw import ops
    from tw.modeling import PackedRows
    clips = _clips(causal, dtype)
    idx = list(range(len(LENS)))
    if order == "reversed":
        idx.reverse()
    lens = [LENS[i] for i in idx]
    pk = PackedRows.from_lens(lens, max(LENS), "cuda")
    B, M, mx = pk.B, pk.M, pk.max_len
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    bl = pk.block_list(causal)
    assert bl[1] == sum((n + 127) // 128 for n in lens) == 10
    do = torch.cat([clips[i]["do"] for i in idx])
    o = _guarded(M, D, dtype)
    lse = torch.full((H * M + GUARD,), -7.0, device="cuda")
    ws = torch.full((H * M + GUARD,), -7.0, device="cuda")
    if causal:
        x = torch.cat([clips[i]["qkv"] for i in idx])
        ops.attn_fwd_varlen(x, 3 * D, x[:, D:], 3 * D, x[:, 2 * D:], 3 * D, o, D, lse, pk.off, pk.off, B, H, M, mx, mx,
                            True, SCALE, blocks=bl)
        dx = _guarded(M, 3 * D, dtype)
        ops.attn_bwd_varlen(x, 3 * D, x[:, D:], 3 * D, x[:, 2 * D:], 3 * D, o, D, do, D, lse, dx, 3 * D, dx[:, D:],
                            3 * D, dx[:, 2 * D:], 3 * D, pk.off, pk.off, B, H, M, mx, mx, True, SCALE, blocks=bl,
                            workspace=ws)
        dq, guards = dx[:, :D], [dx[M:]]
        dk = lambda b: dx[off[b]:off[b + 1], D:2 * D]
        dv = lambda b: dx[off[b]:off[b + 1], 2 * D:]
    else:
        q = torch.cat([clips[i]["q"] for i in idx])
        kv = torch.cat([clips[i]["kv"] for i in idx])
        ops.attn_fwd_varlen(q, D, kv, 2 * D, kv[:, D:], 2 * D, o, D, lse, pk.off, None, B, H, M, mx, TK, False, SCALE,
                            blocks=bl)
        dq = _guarded(M, D, dtype)
        dkv = _guarded(B * TK, 2 * D, dtype)
        ops.attn_bwd_varlen(q, D, kv, 2 * D, kv[:, D:], 2 * D, o, D, do, D, lse, dq, D, dkv, 2 * D, dkv[:, D:], 2 * D,
                            pk.off, None, B, H, M, mx, TK, False, SCALE, blocks=bl, workspace=ws)
        guards = [dq[M:], dkv[B * TK:]]
        dk = lambda b: dkv[b * TK:(b + 1) * TK, :D]
        dv = lambda b: dkv[b * TK:(b + 1) * TK, D:]
    torch.cuda.synchronize()
    for t in [o[M:], lse[H * M:], ws[H * M:]] + guards:
        assert bool((t == -7.0).all()), "a guard row was written"
    for b, i in enumerate(idx):
        c, r = clips[i], slice(off[b], off[b + 1])
        if c["n"] == 0:
            if not causal:
                assert not bool(_bits(dk(b)).any()) and not bool(_bits(dv(b)).any()), "dK / dV of a clip without rows"
            continue
        what = f"clip of {c['n']} rows at {b}"
        _same(o[r], c["o"], what + " O")
        _same(lse[: H * M].view(H, M)[:, r], c["lse"], what + " LSE")
        _same(dq[r], c["dq"], what + " dQ")
        _same(ws[: H * M].view(H, M)[:, r], c["dd"], what + " D")
        _same(dk(b), c["dk"], what + " dK")
        _same(dv(b), c["dv"], what + " dV")


def _expected_lists(lens):
    """(list 0, list 1) as tw_pack_blocks documents them: descending tiles (list 0: no tiles), ties by (clip, block)."""
    blocks = [(b, k * 128, min(128, n - k * 128), (min(n, k * 128 + 128) + 63) // 64)
              for b, n in enumerate(lens) for k in range((n + 127) // 128)]
    l0 = sorted(blocks, key=lambda e: (e[0], e[1]))
    l1 = sorted(blocks, key=lambda e: (-e[3], e[0], e[1]))
    return [list(e[:3]) + [0] for e in l0], [list(e) for e in l1]


@pytest.mark.parametrize("case", ["lens", "reversed", "many"])
def test_pack_blocks_lists_and_counts(case):
    from tw import ops
    if case == "many":       # more blocks than the kernel has threads per pass is not needed: more clips than waves
        g = torch.Generator().manual_seed(9)
        lens = torch.randint(0, 448, (70,), generator=g).tolist()
        lens[3], lens[40] = 447, 0
    else:
        lens = LENS if case == "lens" else LENS[::-1]
    B, T = len(lens), max(lens)
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    offd = torch.tensor(off, dtype=torch.int32, device="cuda")
    cap = B * ((T + 127) // 128)
    blocks = torch.full((2, cap, 4), -1, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ops.pack_blocks(offd, B, T, blocks, count)
    l0, l1 = _expected_lists(lens)
    nblk = len(l0)
    assert count.tolist() == [nblk]
    got = blocks.tolist()
    assert got[0][:nblk] == l0 and got[1][:nblk] == l1
    assert all(e == [-1] * 4 for lst in got for e in lst[nblk:]), "entries past the list were written"
    # each non-empty block once, with its rows
    want = sorted((b, k * 128, min(128, n - k * 128)) for b, n in enumerate(lens) for k in range((n + 127) // 128))
    for lst in (got[0][:nblk], got[1][:nblk]):
        assert sorted((e[0], e[1], e[2]) for e in lst) == want
