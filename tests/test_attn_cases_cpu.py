"""The attention cases of tests/attn_cases.py, proven on the CPU in fp64: every probe hits its key by >= 40 nats
(or ties its pair exactly), inputs and exact expected outputs survive the 16-bit type, the exact expectations agree
with fp64 autograd, and a rounding model of the kernels stays inside the derived bounds with headroom.  What
tests/test_attn_parity_gpu.py asserts of the kernels rests on these."""
import math

import pytest
import torch

import attn_cases as ac

_ids = lambda c: c.id


def _rt(x, dtype):
    return torch.equal(ac.r16(x, dtype), x)


def test_case_lists_cover_the_issue_shapes():
    shapes = {(c.Tq, c.Tk, c.causal) for c in ac.PROBE_CASES}
    assert shapes == {(a, b, False) for a, b in ac.NONCAUSAL} | {(a, b, True) for a, b in ac.CAUSAL}
    for key in ac.FULL:
        for cases in (ac.PROBE_CASES, ac.RANDOM_CASES):
            if cases is ac.RANDOM_CASES and key not in ac.RANDOM_SHAPES:
                continue
            got = {(c.B, c.H, c.dtype) for c in cases if (c.Tq, c.Tk, c.causal) == key}
            assert got == {(B, H, dt) for B, H in ac.BH for dt in ac.DTYPES}
    assert {(c.B, c.H, c.dtype) for c in ac.PROBE_CASES if (c.Tq, c.Tk, c.causal) not in ac.FULL} == \
        {(2, 3, torch.bfloat16), (1, 1, torch.float16)}
    assert len({(c.Tq, c.Tk, c.causal) for c in ac.RANDOM_CASES}) == 4
    # grids (blocks x B*H) both a multiple of 8 and not, and beyond 8
    grids = {-(-T // 128) * c.B * c.H for c in ac.ALL_CASES for T in (c.Tq, c.Tk)}
    assert any(g % 8 == 0 for g in grids) and any(g % 8 and g > 8 for g in grids) and 1 in grids
    assert len({c.id for c in ac.ALL_CASES}) == len(ac.ALL_CASES)


def test_code_gap():
    j = torch.arange(2 ** ac.NBITS)
    c = ac.code(j)
    s = ac.AMP * ac.SCALE * (c @ c.T)
    top = ac.AMP * ac.SCALE * ac.NBITS * ac.REP
    assert torch.equal(s.diagonal(), torch.full((len(j),), top, dtype=torch.float64))
    assert float((s - 2 * top * torch.eye(len(j), dtype=torch.float64)).max()) == top - ac.GAP == top - 40.0


@pytest.mark.parametrize("case", ac.PROBE_CASES, ids=_ids)
def test_probe_case(case):
    inp, ref = ac.build(case), ac.reference(case)
    for t in (inp.q, inp.k, inp.v, inp.do):
        assert _rt(t, case.dtype) and bool(torch.isfinite(t).all())
    assert bool((inp.v != 0).all()) and bool((inp.do != 0).all())      # the e^-40 tail is absorbed everywhere
    s = ac.scores(inp.q, inp.k, case.causal)
    if not case.exact:
        # the first forbidden key: the aimed-at key is masked for every query but the last, the rest is a mixture
        hidden = ac.mask(case.Tq, case.Tk, True)[torch.arange(case.Tq), inp.ta[0, 0]]
        assert bool(hidden[:-1].all()) and not bool(hidden[-1])
        return
    ex = ac.exact(case)
    tied = inp.ta != inp.tb
    sa, sb = s.gather(-1, inp.ta.unsqueeze(-1)).squeeze(-1), s.gather(-1, inp.tb.unsqueeze(-1)).squeeze(-1)
    assert torch.equal(sa, sb) and torch.equal(sa, s.max(-1).values)    # exact tie (or the same key)
    rest = s.masked_fill(ex.p > 0, float("-inf")).max(-1).values
    assert float((sa - rest).min()) >= ac.GAP == 40.0
    assert torch.equal(s.argmax(-1)[~tied], inp.ta[~tied])
    pa = ref.p.gather(-1, inp.ta.unsqueeze(-1)).squeeze(-1)
    assert torch.equal(pa[tied], torch.full_like(pa[tied], 0.5)) and torch.equal(pa[~tied], torch.ones_like(pa[~tied]))
    if case.map == "tie":
        assert int(tied.sum()) >= tied.numel() - case.B * case.H       # at most the query that sees key 0 only
    # the exact expectations: fp64 autograd agrees to the e^-40 tail, and they are 16-bit values
    assert float((ex.o - ref.o).abs().max()) < 1e-12 and float((ex.lse - ref.lse).abs().max()) < 1e-12
    assert float((ex.dq - ref.dq).abs().max()) < 1e-10 and float((ex.dk - ref.dk).abs().max()) < 1e-10
    assert float((ex.dv - ac.r16(ref.dv, case.dtype)).abs().max()) < 1e-12
    for t in (ex.o, ex.dq, ex.dk, ex.dv):
        assert _rt(t, case.dtype)
    assert bool((ex.o != 0).all()) and bool((ex.dv[ex.hit] != 0).all())
    assert bool((ex.dv[~ex.hit] == 0).all())
    if case.map != "tie":
        assert not bool(ex.dq.any()) and not bool(ex.dk.any())           # one-hot P: dS = 0
    elif case.Tk > 2 or not case.causal:
        assert bool((ex.dq.abs().amax(-1)[tied] >= 2.0 ** -4).all())     # dS = +-dO[q][0] / 4: every tied row has content
        assert float(ex.dk.abs().max()) >= 1.0
    assert float(ex.o.abs().max()) < -ac.SENTINEL and float(ex.dv.abs().max()) < -ac.SENTINEL


_worst = {}


@pytest.mark.parametrize("case", ac.RANDOM_CASES + [c for c in ac.PROBE_CASES if not c.exact] + ac.INDEPENDENT_CASES,
                         ids=_ids)
def test_rounding_model_inside_bounds(case):
    """fp64 with the kernels' 16-bit rounding points stays inside every bound, below 0.8 of it on O.  dV and dK come
    within a few percent where one (q, j) term makes the whole element: two roundings against a two-rounding bound
    (the kernels' fp32 noise then has the 2^-16 term).  test_print_model_ratios prints the worst ratios."""
    inp, ref, bnd = ac.build(case), ac.reference(case), ac.bounds(case)
    for t in (inp.q, inp.k, inp.v, inp.do):
        assert _rt(t, case.dtype) and bool(torch.isfinite(t).all())
    for b in bnd:
        assert bool(torch.isfinite(b).all()) and bool((b >= 0).all())
    assert bool((bnd.lse >= 2.0 ** -20).all())
    got = ac.model(case)
    for nm in ("o", "dq", "dk", "dv"):
        err, bar = (got[nm] - getattr(ref, nm)).abs(), getattr(bnd, nm)
        ratio = float((err / bar.clamp(min=1e-300)).max())
        key = (nm, ac.DT_NAME[case.dtype])
        _worst[key] = max(_worst.get(key, 0.0), ratio)
        assert ratio <= (0.8 if nm == "o" else 1.0), (nm, ratio)
    assert float((got["lse"] - ref.lse).abs().max()) < 1e-12


def test_print_model_ratios():
    assert _worst, "runs after test_rounding_model_inside_bounds"
    for (nm, dt), r in sorted(_worst.items()):
        print(f"rounding model worst err/bound {nm:3s} {dt}: {r:.3f}")


def test_random_ramps_move_the_row_max():
    for case in ac.RANDOM_CASES:
        if case.ramp and case.B == 1:
            k = ac.build(case).k[0, 0, :, ac.HD - 1]
            assert bool(((k[1:] - k[:-1]) * case.ramp >= 0).all()) and abs(float(k[-1] - k[0])) >= 5.9


@pytest.mark.parametrize("case", [c for c in ac.ALL_CASES if (c.Tq, c.Tk, c.B) in ((33, 65, 2), (129, 200, 3))][:8],
                         ids=_ids)
def test_layout_round_trip(case):
    """The fused buffers hold the case (head h at column h*64), guards are NaN / lures, outputs start as sentinels."""
    inp = ac.build(case)
    lay = ac.Layout(inp)
    B, H, Tq, Tk, d = case.B, case.H, case.Tq, case.Tk, case.H * 64
    for b in range(B):
        for h in range(H):
            assert torch.equal(lay.q[b * Tq:(b + 1) * Tq, h * 64:(h + 1) * 64].double(), inp.q[b, h])
            assert torch.equal(lay.k[b * Tk:(b + 1) * Tk, h * 64:(h + 1) * 64].double(), inp.k[b, h])
            assert torch.equal(lay.v[b * Tk:(b + 1) * Tk, h * 64:(h + 1) * 64].double(), inp.v[b, h])
            assert torch.equal(lay.do[b * Tq:(b + 1) * Tq, h * 64:(h + 1) * 64].double(), inp.do[b, h])
    assert lay.qkv.shape == (B * Tq + 64, 3 * d) and lay.kv.shape == (B * Tk + 64, 2 * d)
    assert bool(lay.qkv[:, d:].isnan().all()) and bool(lay.qkv[B * Tq:].isnan().all())
    assert bool(lay.v[B * Tk:, :d].isnan().all()) and bool(lay.do[B * Tq:].isnan().all())
    lure = lay.k[B * Tk:, :d].double()
    assert bool(torch.isfinite(lure).all())
    if case.kind == "probe":       # guard key g scores twice the top score against the query it copies
        q = inp.q[-1, :, torch.arange(64) % Tq]                       # [H][64][64]
        s = (q * lure.view(64, H, 64).transpose(0, 1)).sum(-1) * ac.SCALE
        assert float(s.min()) >= 2 * 200.0
    assert lay.guards_intact() == []
    out = lay.outputs()
    assert all(bool((t == ac.SENTINEL).all()) for t in out.values())
    assert out["o"].shape == inp.q.shape and out["dk"].shape == inp.k.shape and out["lse"].shape == (B, H, Tq)
    lay.o[B * Tq, 0] = 1.0
    lay.dkv[0, 2 * d] = 1.0
    assert lay.guards_intact() == ["o", "dkv"]
