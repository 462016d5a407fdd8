"""The flash-attention kernels of csrc/attention.hip (forward, dQ, dK/dV; bf16 and fp16) against the cases, fp64
references and derived bounds of tests/attn_cases.py (proven on the CPU by tests/test_attn_cases_cpu.py).

Probe cases are asserted exactly: O[q] is V[target(q)] bit for bit, dV[target(q)] is dO[q], a tied pair gives the
exactly representable 1/2, 1/2 values, and whatever is exactly 0 stays below the cancellation bar.  Random cases and
the "first forbidden key" probe are asserted element by element against first-order rounding bounds.  Shapes sit on
the kernels' edges (128 query rows per workgroup, 32 per wave, 64-key tiles, the 1 / 2 / >= 4 tile prologues of the
forward's 3-deep ring, causal with Tq < Tk), grids are and are not multiples of 8 (remap_bh), inputs live in the
model's fused buffers with NaN / lure guard rows and every output has sentinel guard rows and columns."""
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
_ids = lambda c: c.id


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _run(case, o=None, lse=None):
    """Forward (unless o / lse are given) and backward on the case's fused buffers -> (layout, outputs)."""
    from tw import ops
    c, lay = case, ac.Layout(ac.build(case), DEV, o, lse)
    if o is None:
        ops.attn_fwd(lay.q, lay.ldq, lay.k, lay.ldkv, lay.v, lay.ldkv, lay.o, lay.ldo, lay.lse, c.B, c.H, c.Tq, c.Tk,
                     c.causal, ac.SCALE)
    ops.attn_bwd(lay.q, lay.ldq, lay.k, lay.ldkv, lay.v, lay.ldkv, lay.o, lay.ldo, lay.do, lay.d, lay.lse, lay.dq,
                 lay.ldo, lay.dk, lay.lddkv, lay.dv, lay.lddkv, c.B, c.H, c.Tq, c.Tk, c.causal, ac.SCALE)
    torch.cuda.synchronize()
    out = lay.outputs()
    for nm, t in out.items():
        assert bool(torch.isfinite(t).all()), f"{nm}: NaN or Inf"
    assert lay.guards_intact() == [], "a write outside the tensor"
    return lay, out


@pytest.mark.parametrize("case", [c for c in ac.PROBE_CASES if c.exact], ids=_ids)
def test_probe_exact(case):
    inp, ex = ac.build(case), ac.exact(case)
    _, got = _run(case)
    # forward: the targeted V row (the mean of the tied pair), bit for bit
    assert torch.equal(got["o"], ex.o), _where(got["o"], ex.o)
    lerr = (got["lse"] - ex.lse).abs()
    assert bool((lerr <= 4 * 2.0 ** -24 * ex.lse.abs()).all()), float((lerr / ex.lse.abs()).max())
    # dV: the targeted rows bit for bit, the others hold the e^-40 tail only
    hit = ex.hit.unsqueeze(-1).expand_as(ex.dv)
    assert torch.equal(got["dv"][hit], ex.dv[hit]), _where(got["dv"] * hit, ex.dv * hit)
    assert float(got["dv"][~hit].abs().max() if (~hit).any() else 0.0) < 1e-12
    # dQ, dK: bit for bit where the exact value is not 0; where it is, dp and D cancel up to fp32 summation order
    bar = ac.zero_bar(case)
    for nm in ("dq", "dk"):
        want, g = getattr(ex, nm), got[nm]
        nz = want != 0
        assert torch.equal(g[nz], want[nz]), (nm, _where(g * nz, want))
        assert float(g[~nz].abs().max()) <= bar, (nm, float(g[~nz].abs().max()), bar)
    print(f"{case.id}: lse err/bar {float((lerr / (4 * 2.0 ** -24 * ex.lse.abs())).max()):.3f}, "
          f"|dq|, |dk| at exact zeros {float(got['dq'][ex.dq == 0].abs().max()):.2e} "
          f"{float(got['dk'][ex.dk == 0].abs().max()):.2e} (bar {bar:.2e})")


def _where(got, want):
    bad = (got != want).nonzero()
    if not len(bad):
        return "equal"
    i = tuple(bad[0].tolist())
    return f"{len(bad)} elements differ, first at [b, h, row, col] = {i}: got {float(got[i])}, want {float(want[i])}"


def _bounded(case, got, names):
    ref, bnd = ac.reference(case), ac.bounds(case)
    ratios = {}
    for nm in names:
        err, bar = (got[nm] - getattr(ref, nm)).abs(), getattr(bnd, nm)
        ratios[nm] = float((err / bar.clamp(min=1e-300)).max())
    print(f"{case.id}: max err/bound " + " ".join(f"{nm} {r:.3f}" for nm, r in ratios.items()))
    for nm, r in ratios.items():
        assert r <= 1.0, (nm, r)


@pytest.mark.parametrize("case", ac.RANDOM_CASES + [c for c in ac.PROBE_CASES if not c.exact], ids=_ids)
def test_bounded(case):
    _, got = _run(case)
    _bounded(case, got, ("o", "lse", "dq", "dk", "dv"))


@pytest.mark.parametrize("case", ac.INDEPENDENT_CASES, ids=_ids)
def test_backward_on_reference_forward(case):
    """o and lse from the fp64 reference (rounded to the dtype / to fp32), not from the forward kernel: the backward
    kernels are judged on their own."""
    ref = ac.reference(case)
    _, got = _run(case, o=ac.r16(ref.o, case.dtype), lse=ref.lse)
    assert torch.equal(got["o"], ac.r16(ref.o, case.dtype))          # the backward leaves o alone
    _bounded(case, got, ("dq", "dk", "dv"))


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=lambda d: ac.DT_NAME[d])
@pytest.mark.parametrize("scale", [0.0, -0.125, float("nan")])
def test_scale_must_be_positive(dtype, scale):
    """The forward takes the row max before scaling: every 16-bit entry refuses !(scale > 0) with TW_EINVAL (1)
    before any launch (the outputs keep their sentinels)."""
    from tw import ops
    case = ac.Case("rand", "a1", 2, 3, 33, 33, True, dtype, 1.0, 0)
    lay = ac.Layout(ac.build(case), DEV)
    c = case
    offq = torch.tensor([0, 33, 66], dtype=torch.int32, device=DEV)
    fwd = (lay.q, lay.ldq, lay.k, lay.ldkv, lay.v, lay.ldkv, lay.o, lay.ldo, lay.lse)
    bwd = fwd[:8] + (lay.do, lay.d, lay.lse, lay.dq, lay.ldo, lay.dk, lay.lddkv, lay.dv, lay.lddkv)
    calls = [lambda: ops.attn_fwd(*fwd, c.B, c.H, c.Tq, c.Tk, True, scale),
             lambda: ops.attn_bwd(*bwd, c.B, c.H, c.Tq, c.Tk, True, scale),
             lambda: ops.attn_fwd_varlen(*fwd, offq, offq, c.B, c.H, 66, 33, 33, True, scale),
             lambda: ops.attn_bwd_varlen(*bwd, offq, offq, c.B, c.H, 66, 33, 33, True, scale)]
    for f in calls:
        with pytest.raises(RuntimeError, match="status 1"):
            f()
    torch.cuda.synchronize()
    assert all(bool((t == ac.SENTINEL).all()) for t in lay.outputs().values()) and lay.guards_intact() == []
