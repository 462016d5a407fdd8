"""The case table of the GEMM parity suite (tests/gemm_cases.py) proven on the CPU before any GPU sees it: every case's
expected plan against the library's planner (ops.gemm_route with 256 CUs: nothing launched), the table's coverage of
routes, epilogue kinds, layouts and operand types, the exactness of the integer products, the range and spread of the
expected outputs, and the comparators against planted faults (edits of CPU tensors)."""
import collections
import math

import pytest
import torch

import gemm_cases as gc
import gemm_routes as gr
from gemm_cases import BF16, F16, F32

SMALL = [c for c in gc.CASES if c.id not in gc.LARGE]


def ask(c, have_ws=True, force=None):
    from tw import ops
    h = c.dtype
    return ops.gemm_route(
        h, h, c.c_dtype, c.M, c.N, c.K, lda=c.lda, ldb=c.ldb, ldc=c.ldc, a_trans=c.a_trans, b_trans=c.b_trans,
        bias=h if c.bias else None, res=c.res_dtype, ldr=c.ldr, res_mod=c.res_mod,
        aux=h if c.flags & (gr.F_AUX_OUT | gr.F_DGELU) else None, ldaux=c.ldaux,
        flags=c.flags | (c.force if force is None else force), batch=c.batch, sA=c.sA, sB=c.sB, sC=c.sC, sR=c.sR,
        sAux=c.sAux, cus=256, have_ws=have_ws)


def test_every_plan_is_the_planners():
    bad = []
    for c in gc.CASES:
        p = ask(c)
        if (p.route, p.S, p.m_dp, p.split_tile, p.epi) != (c.route, c.S, c.m_dp, c.split_tile, c.epi):
            bad.append((c.id, "planned", tuple(p), "expected", (c.route, c.S, c.m_dp, c.split_tile, c.epi)))
        if c.no_ws is not None and ask(c, have_ws=False).route != c.no_ws:
            bad.append((c.id, "without a workspace", ask(c, have_ws=False).route, "expected", c.no_ws))
        for extra, route in c.twins:
            q = ask(c, force=c.force | extra)
            if q.route != route or q.epi != c.epi:
                bad.append((c.id, "twin", extra, tuple(q), "expected", route))
    assert not bad, (len(bad), bad[:12])


def test_a_nosplit_twin_is_the_plan_without_a_workspace():
    """The GPU test cannot take the workspace away; where a case names both, the NOSPLIT twin it runs is the kernel the
    call falls back to."""
    n = 0
    for c in gc.CASES:
        for extra, route in c.twins:
            if extra == gr.NOSPLIT and c.no_ws is not None:
                assert route == c.no_ws, c.id
                n += 1
    assert n >= 20


# (route, operand type) pairs the table leaves out, each with its reason in the case module's docstring
EXCLUDED = {("persistent_edges", BF16)}
# routes fp16 instantiates for K-major operands only: no case on a transposed layout
F16_KMAJOR_ONLY = {"t256x128_s3", "t256x128_s2", "t128_ring4", "persistent", "persistent_edges"}


# (route, epilogue kind, operand type) the planner produces and the table leaves out: none
EXCLUDED_PAIRS = set()


def producible():
    """Every (route, epilogue kind, operand type) the planner yields over the table's shapes x the four layouts x every
    epilogue spec x dense / padded leading dimensions x the routing flags x batch 1 / 3."""
    forces = (0, gr.NOSPLIT, gr.TILE256x128_S2) + tuple(gc.FORCE.values())
    out = set()
    for h in (BF16, F16):
        for name, sp in gc.SPECS.items():
            if sp.flags & gr.F_CLAMP16 and h == BF16:
                continue
            for M, N, K in gc.shapes():
                for at, bt in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    if (at and M % 8) or (bt and N % 8) or (not (at and bt) and K % 8):
                        continue
                    for pad, batch in ((False, 1), (True, 1), (True, 3)):
                        if batch == 3 and M * N > 1 << 20:
                            continue
                        c = gc.mk(h, "?", M, N, K, name, at=at, bt=bt, pad=pad, batch=batch)
                        for f in forces:
                            p = ask(c, force=f)
                            out.add((p.route, p.epi, h))
    return out


def test_coverage():
    seen = collections.defaultdict(set)
    for c in gc.CASES:
        seen["route"].add((c.route, c.dtype))
        seen["epi"].add((c.epi, c.dtype))
        seen["layout"].add((c.a_trans, c.b_trans, c.dtype))
        seen["pair"].add((c.route, c.epi, c.dtype))
        seen["route_layout"].add((c.route, c.a_trans, c.b_trans, c.dtype))
        if c.route == "splitk_dw":
            seen["split_tile"].add((c.split_tile, c.dtype))
        if c.route == "rounds_sk_tail":
            seen["m_dp"].add((c.m_dp > 0, c.dtype))
    want = {(r, h) for r in gr.ROUTES for h in (BF16, F16)} - EXCLUDED
    assert seen["route"] == want, (want - seen["route"], seen["route"] - want)
    assert seen["epi"] == {(e, h) for e in gr.EPI for h in (BF16, F16)}
    assert seen["layout"] == {(a, b, h) for a in (False, True) for b in (False, True) for h in (BF16, F16)}
    assert seen["split_tile"] == {(t, h) for t in (128, 256) for h in (BF16, F16)}
    assert seen["m_dp"] == {(z, h) for z in (False, True) for h in (BF16, F16)}
    # the exclusions are exactly what the planner cannot produce: asking for them lands elsewhere
    for c in gc.CASES:
        if c.dtype == F16 and (c.a_trans or c.b_trans):
            assert c.route not in F16_KMAJOR_ONLY, c.id
            for f in (gr.TILE256x128, gr.TILE256x128 | gr.TILE256x128_S2, gr.TILE256PP):
                assert ask(c, force=f).route == "t128", c.id
        if c.dtype == BF16 and c.force & gr.TILE256PP and not (c.a_trans or c.b_trans):
            assert ask(c).route == "persistent", c.id
    # every (route, epilogue kind) pair the planner produces appears, per operand type, but the named ones
    can = producible()
    missing = can - seen["pair"] - EXCLUDED_PAIRS
    assert not missing, sorted((r, e, gc.NAME[h]) for r, e, h in missing)
    assert seen["pair"] <= can and not EXCLUDED_PAIRS & seen["pair"] and EXCLUDED_PAIRS <= can
    # every kernel instantiation of dispatch<H, AT, BT> sees a ragged M, a ragged N and a K tail
    tiles = {"t128": (128, 128), "t128_ring4": (128, 128), "t256": (256, 256), "t256x128_s3": (256, 128),
             "t256x128_s2": (256, 128), "persistent": (256, 256)}
    for (r, at, bt, h) in sorted(seen["route_layout"], key=str):
        if r not in tiles or (h == F16 and r == "persistent"):
            continue
        cs = [c for c in gc.CASES if (c.route, c.a_trans, c.b_trans, c.dtype) == (r, at, bt, h)]
        bm, bn = tiles[r]
        assert any(c.M % bm for c in cs) and any(c.N % bn for c in cs) and any(c.K % 64 for c in cs), (r, at, bt, h)
    assert len(gc.CASES) < 1200 and len(gc.LARGE) <= 32


def test_the_table_shapes_are_in_the_planner_comparison():
    assert set(gc.shapes()) <= set(gr.TEST_SHAPES)


@pytest.fixture(scope="module")
def refs():
    """(case, inputs, reference) of every case below the large grids, computed once."""
    out = []
    for c in SMALL:
        inp = gc.build(c)
        out.append((c, inp, gc.reference(c, inp)))
    return out


def test_exact_products(refs):
    for c in gc.CASES:
        if c.family != "randn":
            assert c.K * c.R * c.R <= 1 << 24, c.id
            assert c.R == gc.amplitude(c.dtype, c.K) and c.R >= 32       # five bits at the longest K
            a = c.alpha
            assert a > 0 and a == 2.0 ** round(math.log2(a)), c.id
    n = 0
    for c, inp, ref in refs:
        if c.family == "randn" or c.batch * c.M * c.N * c.K >= 10 ** 8:
            continue
        acc = torch.matmul(inp["A"], inp["B"].transpose(1, 2)).double() * c.alpha
        want = gc.reference_int64(c, inp)
        got = acc + inp["bias"].to(c.dtype).double() if c.bias else acc
        assert torch.equal(got, want), c.id
        assert torch.equal(got.float().double(), got), c.id            # and it is an fp32 value
        n += 1
    assert n > 300


def test_range_and_spread(refs):
    tot, inexact = collections.Counter(), collections.Counter()
    for c, inp, ref in refs:
        if c.family != "exact" or c.c_dtype == F32:
            continue
        if not c.flags & gr.F_CLAMP16:
            assert ref["finite"], c.id
        else:
            v = ref["C"].float().abs()
            assert float(v.max()) <= 64512.0 and bool((v >= 64504.0).any()) and bool((v < 60000.0).any()), c.id
        tot[c.dtype] += ref["C"].numel()
        inexact[c.dtype] += int(ref["inexact"].sum())
    for h in (BF16, F16):
        assert inexact[h] >= 0.01 * tot[h], (gc.NAME[h], inexact[h], tot[h])
        # ... and values that needed no rounding are there too
        assert tot[h] - inexact[h] >= 0.01 * tot[h], (gc.NAME[h], inexact[h], tot[h])


def test_gelu_cases_stay_in_range(refs):
    for c, inp, ref in refs:
        if c.family == "gelu" and "aux" in ref:
            x = ref["aux"].float().abs()
            assert float(x.max()) <= 16.0 and float(x.median()) > 0.1, (c.id, float(x.max()))


# ------------------------------------------------------------------------------------------------ planted faults
def _case(cid_part, pred=lambda c: True, **kw):
    cs = [c for c in gc.CASES if cid_part in c.id and all(getattr(c, k) == v for k, v in kw.items()) and pred(c)]
    assert cs, cid_part
    return cs[0]


def _buffers(c):
    inp = gc.build(c)
    ref = gc.reference(c, inp)
    C, aux = gc.expected_buffers(c, inp, ref)
    return inp, ref, C


@pytest.mark.parametrize("cid", ["bf16-t128-nn-store16-", "fp16-t256-nn-res32-", "bf16-skinny_splitk-nn-res16-",
                                 "fp16-splitk_dw-tt-accum32-"])
def test_comparator_one_ulp(cid):
    c = _case(cid)
    inp, ref, C = _buffers(c)
    assert gc.compare_exact(c, "C", C.clone(), C, c.ldc, c.sC) is None
    got = C.clone()
    v = gc.view(got, c.batch, c.M, c.N, c.ldc, c.sC)
    m, n = c.M - 1, c.N // 2
    gc._bits(v)[0, m, n] += 1
    rep = gc.compare_exact(c, "C", got, C, c.ldc, c.sC)
    assert rep and "1 of" in rep and f"row {m}, column {n}" in rep and "pad" not in rep, rep


def test_comparator_missing_k_step():
    c = _case("bf16-t128-nn-", lambda c: c.M >= 32 and c.K > 64 and c.K % 64 and c.family == "exact")
    inp, ref, C = _buffers(c)
    A = inp["A"].clone()
    A[:, 16:32, c.K // 64 * 64:] = 0        # the K tail never reaches rows 16..31 of the first tile
    bad = gc.reference(c, inp, A=A)
    got, _ = gc.expected_buffers(c, inp, bad)
    rep = gc.compare_exact(c, "C", got, C, c.ldc, c.sC)
    assert rep and "first at batch 0, row 16," in rep, rep
    assert int((gc._bits(got) != gc._bits(C)).sum()) <= 16 * c.N


def test_comparator_swapped_tiles():
    c = _case("bf16-t128-nn-", M=264, N=264)
    inp, ref, C = _buffers(c)
    w = ref["C"].clone()
    w[:, 0:128, 0:128], w[:, 0:128, 128:256] = ref["C"][:, 0:128, 128:256], ref["C"][:, 0:128, 0:128]
    got, _ = gc.expected_buffers(c, inp, dict(ref, C=w))
    rep = gc.compare_exact(c, "C", got, C, c.ldc, c.sC)
    assert rep and "first at batch 0, row 0, column 0" in rep, rep


def test_comparator_residual_row():
    c = _case("-resmod32-", dtype=BF16, route="t128")
    assert c.M > c.res_mod > 0
    inp, ref, C = _buffers(c)
    g = torch.Generator().manual_seed(1)
    rows = torch.cat([inp["res"], gc._ints(g, (c.batch, c.M - c.res_mod, c.N), -16, 16) * inp["unit"]], 1)
    bad = gc.reference(c, inp, res_rows=rows)
    assert torch.equal(bad["C"][:, :c.res_mod], ref["C"][:, :c.res_mod])
    got, _ = gc.expected_buffers(c, inp, bad)
    rep = gc.compare_exact(c, "C", got, C, c.ldc, c.sC)
    assert rep and f"first at batch 0, row {c.res_mod}," in rep, rep


@pytest.mark.parametrize("h", [BF16, F16])
def test_comparator_bias_after_rounding(h):
    c = _case("-t128-nn-store16-", dtype=h)
    inp, ref, C = _buffers(c)
    got, _ = gc.expected_buffers(c, inp, gc.reference(c, inp, bias_after_round=True))
    assert gc.compare_exact(c, "C", got, C, c.ldc, c.sC)


def test_comparator_pad_and_guard():
    c = _case("bf16-t256-nn-gelu_aux-", batch=3)
    assert c.ldc > c.N and c.sC > c.M * c.ldc
    inp, ref, C = _buffers(c)
    got = C.clone()
    got[5 * c.ldc + c.N] = 1.0              # a pad column of row 5
    rep = gc.compare_exact(c, "C", got, C, c.ldc, c.sC)
    assert rep and "1 pad / guard elements changed" in rep and "row 5" in rep and "pad column" in rep, rep
    got = C.clone()
    got[-1] = 0.0                           # the guard tail
    rep = gc.compare_exact(c, "C", got, C, c.ldc, c.sC)
    assert rep and "past the last row of batch 2" in rep, rep
    got = C.clone()
    got[c.M * c.ldc + 3] = 0.0              # between two batch entries
    rep = gc.compare_exact(c, "C", got, C, c.ldc, c.sC)
    assert rep and "past the last row of batch 0" in rep, rep
    # the bounded comparator sees them too, and an element outside its bound
    r, rep = gc.compare_bounded(c, "C", C.clone(), inp["C_buf"], ref["C64"], ref["bound"], c.ldc, c.sC)
    assert r == 0.0 and rep is None
    got = C.clone()
    got[-1] = 0.0
    v = gc.view(got, c.batch, c.M, c.N, c.ldc, c.sC)
    big = int(ref["C64"][1].abs().argmax())
    m, n = divmod(big, c.N)
    gc._bits(v)[1, m, n] += 2               # two ulp
    r, rep = gc.compare_bounded(c, "C", got, inp["C_buf"], ref["C64"], ref["bound"], c.ldc, c.sC)
    assert r > 1.0 and f"worst at batch 1, row {m}, column {n}" in rep and "guard elements changed" in rep, rep


def test_nan_pads_reach_a_product_that_reads_them():
    """An operand pad that is multiplied in shows up: the reference over the padded rows is NaN."""
    c = _case("bf16-t128-nn-", lambda c: c.lda > c.K and not c.flags & gr.F_ACCUM)
    inp = gc.build(c)
    assert c.lda > c.K
    rows = inp["A_buf"][:c.M * c.lda].view(c.M, c.lda).float()
    assert bool(torch.isnan(rows[:, c.K:]).all()) and not bool(torch.isnan(rows[:, :c.K]).any())
    assert bool(torch.isnan(inp["A_buf"][-gc.GUARD:].float()).all())
    assert bool(torch.isnan(gc.view(inp["C_buf"], 1, c.M, c.N, c.ldc, c.sC).float()).all())
    assert bool((inp["C_buf"][-gc.GUARD:].float() == gc.SENTINEL).all())
