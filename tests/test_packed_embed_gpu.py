"""Packed decoder rows outside the attention: the row plan (tw_pack_plan), the embedding forward by given positions
(tw_embed_fwd_rows) and the position-embedding gradient (tw_pos_grad_rows), against torch gather / scatter on the same
device.  d = 256, lengths [3, 1, 8].  The forward is exact (one fp32 add, one rounding).  The gradient is exact too: the
kernel adds a position's rows in ascending clip order from 0 and then adds the sum to gP, and the reference below adds
them in the same order (at most 3 terms per position, gP starting from zero)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS, T, D = [3, 1, 8], 8, 256


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def test_pack_plan_lengths_offsets_and_rows():
    from tw import ops
    B, Tl = 20, 70                       # more clips than the kernel's 16 waves, rows longer than one wave
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(0, Tl + 1, (B,), generator=g).tolist()
    lens[0], lens[5], lens[19] = Tl, 0, 1
    lab = torch.full((B, Tl), -100, dtype=torch.int64)
    for b, n in enumerate(lens):
        if n:
            lab[b, :n] = torch.randint(0, 1000, (n,), generator=g)
            lab[b, : n // 3] = -100      # leading masked rows (a prompt) stay inside the clip
            lab[b, n - 1] = 7
    off = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    src = torch.full((B * Tl,), -1, dtype=torch.int64, device="cuda")
    ops.pack_plan(lab.cuda(), off, src)
    want_off = [0]
    for n in lens:
        want_off.append(want_off[-1] + n)
    assert off.tolist() == want_off
    want_src = [b * Tl + t for b, n in enumerate(lens) for t in range(n)]
    got = src.tolist()
    assert got[: len(want_src)] == want_src
    assert all(v == 0 for v in got[len(want_src):])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_fwd_rows_matches_gather(dtype):
    from tw.modeling import PackedRows
    from tw import ops
    g = torch.Generator().manual_seed(4)
    pk = PackedRows.from_lens(LENS, T, "cuda")
    tok = torch.randn(50, D, generator=g).to(dtype).cuda()
    pos = torch.randn(T, D, generator=g).to(dtype).cuda()
    ids = torch.randint(0, 50, (pk.M,), generator=g).cuda()
    out = torch.full((pk.M + 2, D), -7.0, dtype=dtype, device="cuda")
    ops.embed_fwd_rows(ids, pk.src, tok, pos, out[: pk.M], T)
    t = torch.tensor([t for n in LENS for t in range(n)], device="cuda")
    want = (tok.float()[ids] + pos.float()[t]).to(dtype)
    assert torch.equal(out[: pk.M], want)
    assert bool((out[pk.M:] == -7.0).all())


def test_pos_grad_rows_matches_ordered_scatter():
    from tw.modeling import PackedRows
    from tw import ops
    g = torch.Generator().manual_seed(5)
    pk = PackedRows.from_lens(LENS, T, "cuda")
    dx = torch.randn(pk.M, D, generator=g).cuda()
    gP = torch.zeros(T + 2, D, device="cuda")
    ops.pos_grad_rows(dx, pk.off, pk.B, pk.M, pk.max_len, gP)
    want = torch.zeros(T + 2, D, device="cuda")
    r0 = 0
    for n in LENS:                       # ascending clip order, as the kernel
        want[:n] += dx[r0: r0 + n]
        r0 += n
    assert torch.equal(gP, want)
    # accumulates into an existing gradient
    ops.pos_grad_rows(dx, pk.off, pk.B, pk.M, pk.max_len, gP)
    assert torch.equal(gP, want + want)
