"""The LayerNorm, KL/CE and helper kernels of csrc/layernorm.hip, csrc/klce.hip and csrc/misc.hip against the cases,
fp64 references and derived per-element bounds of tests/train_cases.py (proven on the CPU by
tests/test_train_cases_cpu.py).  Each test builds its case on the CPU, runs the kernel once through tw.ops and
compares element by element; a miss reports the worst element (index, got, want, bound).  Each family prints its
largest error / bound ratio under -s (profiles/train_kernels_parity.txt holds those lines from an MI355X)."""
import numpy as np
import pytest
import torch

import train_cases as tc
from train_cases import BF16, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
_ids = lambda c: c.id
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    for fam, r in sorted(WORST.items()):
        print(f"\n[train-parity] {fam}: max err/bound {r:.3f}", end="")
    print()


def _check(fam, what, got, want, bound):
    """got within bound of want, element by element; records the family's worst ratio."""
    got, want, bound = got.detach().cpu().double(), want.double(), bound.double().expand_as(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    r = float(ratio.max()) if ratio.numel() else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), r)
    if not r <= 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        pytest.fail(f"{what}: err/bound {r:.3f} at {tuple(int(k) for k in i)}: got {float(got[i])!r}, want "
                    f"{float(want[i])!r}, bound {float(bound[i]):.3e}")


def _exact(fam, what, got, want):
    got = got.detach().cpu()
    same = got.view(torch.int16) == want.view(torch.int16) if got.element_size() == 2 else \
        got.view(torch.int32) == want.view(torch.int32) if got.element_size() == 4 else got == want
    WORST.setdefault(fam, 0.0)
    if not bool(same.all()):
        WORST[fam] = float("inf")
        i = tuple(int(k) for k in (~same).nonzero()[0])
        pytest.fail(f"{what}: {int((~same).sum())} elements differ, first at {i}: got {float(got[i])!r}, want "
                    f"{float(want[i])!r}")


def _guarded(shape, dtype, fill=tc.SENTINEL, guard=256):
    """A sentinel-filled buffer with a guard tail -> (view of the first prod(shape) elements, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), fill, dtype=dtype, device=DEV)
    return buf[:n].view(*shape), buf


def _guard_ok(buf, n, fill=tc.SENTINEL):
    return bool((buf[n:] == fill).all())


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("case", tc.LN_FWD_CASES, ids=_ids)
def test_ln_fwd(case):
    from tw import ops
    c, inp = case, tc.ln_fwd_build(case)
    ref = tc.ln_ref(inp["x"], inp["w"], inp["b"])
    bnd = tc.ln_fwd_bounds(inp["x"], inp["w"], ref, c.y_dtype)
    y, ybuf = _guarded((c.rows, c.D), c.y_dtype)
    mean, mbuf = _guarded((c.rows,), F32)
    rstd, rbuf = _guarded((c.rows,), F32)
    ops.layernorm_fwd(inp["x"].to(DEV), inp["w"].to(DEV), inp["b"].to(DEV), y, mean, rstd, eps=tc.EPS)
    torch.cuda.synchronize()
    assert _guard_ok(ybuf, y.numel()) and _guard_ok(mbuf, c.rows) and _guard_ok(rbuf, c.rows), "a write past the output"
    _check("ln_fwd", f"{c.id} [{c.route}] y", y, ref["y"], bnd["y"])
    _check("ln_fwd", f"{c.id} [{c.route}] mean", mean, ref["mean"], bnd["mean"])
    _check("ln_fwd", f"{c.id} [{c.route}] rstd", rstd, ref["rstd"], bnd["rstd"])
    if c.variant == "const":        # every partial sum is exact: mean = x, xhat = 0, y = b rounded once
        _exact("ln_fwd", f"{c.id} y = b", y, inp["b"].to(c.y_dtype).expand(c.rows, c.D).contiguous())


@pytest.mark.parametrize("case", tc.ADD_LN_CASES, ids=_ids)
def test_add_ln(case):
    from tw import ops
    c, inp = case, tc.add_ln_build(case)
    ref = tc.ln_ref(inp["x_out"], inp["w"], inp["b"])
    bnd = tc.ln_fwd_bounds(inp["x_out"], inp["w"], ref, c.r_dtype)
    x = inp["x"].to(DEV)
    x_out = x if c.inplace else _guarded((c.rows, c.D), c.x_dtype)[0]
    y, ybuf = _guarded((c.rows, c.D), c.r_dtype)
    mean = torch.empty(c.rows, dtype=F32, device=DEV)
    rstd = torch.empty(c.rows, dtype=F32, device=DEV)
    ops.add_layernorm_fwd(x, inp["r"].to(DEV), x_out, inp["w"].to(DEV), inp["b"].to(DEV), y, mean, rstd, eps=tc.EPS)
    torch.cuda.synchronize()
    assert _guard_ok(ybuf, y.numel()), "a write past y"
    _exact("add_ln", f"{c.id} [{c.route}] x_out", x_out, inp["x_out"])
    _check("add_ln", f"{c.id} [{c.route}] y", y, ref["y"], bnd["y"])
    _check("add_ln", f"{c.id} mean", mean, ref["mean"], bnd["mean"])
    _check("add_ln", f"{c.id} rstd", rstd, ref["rstd"], bnd["rstd"])


@pytest.mark.parametrize("case", tc.LN_BWD_CASES, ids=_ids)
def test_ln_bwd(case):
    from tw import ops
    c, inp = case, tc.ln_bwd_build(case)
    ref = tc.ln_bwd_ref(inp, c.accum)
    bnd = tc.ln_bwd_bounds(inp, ref, c.accum)
    dx, dxbuf = _guarded((c.rows, c.D), F32, fill=float("nan"))      # dx_accum = 0: a read of dx shows as NaN
    if c.accum:
        dx.copy_(inp["dx_base"])
    g16 = gbuf = None
    if c.g16 is not None:
        g16, gbuf = _guarded((c.rows, c.D), c.g16)
    dw = inp["dw_base"].to(DEV) if c.params else None
    db = inp["db_base"].to(DEV) if c.params else None
    ops.layernorm_bwd(inp["x"].to(DEV), inp["w"].to(DEV), inp["mean"].to(DEV), inp["rstd"].to(DEV), inp["dy"].to(DEV),
                      dx, dw, db, dx_accum=c.accum, g16=g16)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dxbuf[dx.numel():]).all()), "a write past dx"
    tag = f"{c.id} [{c.route.name}{' stride' if c.route.grid_stride else ''}{' capped' if c.route.capped else ''}]"
    _check("ln_bwd", f"{tag} dx", dx, ref["dx"], bnd["dx"])
    if c.params:
        _check("ln_bwd", f"{tag} dw", dw, ref["dw"], bnd["dw"])
        _check("ln_bwd", f"{tag} db", db, ref["db"], bnd["db"])
    if g16 is not None:
        assert _guard_ok(gbuf, g16.numel()), "a write past g16"
        _exact("ln_bwd_g16", f"{tag} g16 = RNE(dx)", g16, dx.cpu().to(c.g16))


# ------------------------------------------------------------------------------------------------ KL/CE
def _klce_run(c, inp, kl_w=None, inplace=False):
    from tw import ops
    lab = inp["labels"].to(DEV)
    nv = ops.count_valid(lab, torch.zeros(1, dtype=torch.int32, device=DEV))
    s, t = inp["s"].to(DEV), inp["t"].to(DEV)                    # rows + 1: the last is the guard row
    d = s if inplace else torch.full_like(s, tc.SENTINEL)
    guard = d[c.rows].clone()
    out3, row = ops.kl_ce(s[:c.rows], t[:c.rows], lab, c.V, nv, T=c.T, ce_w=c.ce_w, kl_w=c.kl_w if kl_w is None else kl_w,
                          grad_scale=c.gs, dlogits=d[:c.rows])
    torch.cuda.synchronize()
    assert torch.equal(d[c.rows], guard), "the guard row after the last row was written"
    return out3.cpu(), row.cpu().view(c.rows, 2), d[:c.rows].cpu(), int(nv.item())


@pytest.mark.parametrize("case", tc.KLCE_CASES, ids=_ids)
def test_klce(case):
    c, inp = case, tc.klce_build(case)
    out3, row, d, nv = _klce_run(c, inp)
    lab = inp["labels"]
    assert nv == int((lab >= 0).sum())
    ref = tc.klce_ref(inp["s"], inp["t"], lab, c.V, c.T, c.ce_w, c.kl_w, c.gs, nv)
    bnd = tc.klce_bounds(ref, c.V, c.T, c.ce_w, c.kl_w, c.dtype)
    _check("klce", f"{c.id} dlogits", d[:, :c.V], ref["grad"], bnd["grad"])
    _check("klce", f"{c.id} row ce", row[:, 0], ref["row"][:, 0], bnd["row"][:, 0])
    _check("klce", f"{c.id} row kl", row[:, 1], ref["row"][:, 1], bnd["row"][:, 1])
    _check("klce", f"{c.id} out3", out3, ref["out3"], bnd["out3"])
    assert bool((d[:, c.V:] == 0).all()), "pad columns of dlogits are not 0"
    assert bool((d[lab < 0] == 0).all()), "an ignored row of dlogits is not 0"
    _, row2, d2, _ = _klce_run(c, inp, inplace=True)
    _exact("klce", f"{c.id} in place", d2, d)
    _exact("klce", f"{c.id} in place rows", row2, row)
    if c.variant == "equal":        # q and p are one expression: the KL term is exactly 0
        _, _, d0, _ = _klce_run(c, inp, kl_w=0.0)
        _exact("klce", f"{c.id} s == t", d, d0)


# ------------------------------------------------------------------------------------------------ helpers
@pytest.mark.parametrize("case", tc.IM2COL_CASES, ids=_ids)
def test_im2col3(case):
    from tw import ops
    c, src = case, tc.im2col_build(case)
    dst, buf = _guarded((c.B * c.T_out, 3 * c.C), c.dtype)
    ops.im2col3(src.to(DEV), src.shape[1], dst, c.B, c.T_out, c.stride, c.C)
    torch.cuda.synchronize()
    assert _guard_ok(buf, dst.numel()), "a write past dst"
    _exact("im2col3", c.id, dst, tc.im2col_ref(src, c.T_out, c.stride).contiguous())


@pytest.mark.parametrize("case", tc.COL2IM_CASES, ids=_ids)
def test_col2im_s2(case):
    from tw import ops
    c, dA = case, tc.col2im_build(case)
    dX, buf = _guarded((c.B * c.T_in, c.C), F32)
    ops.col2im_s2(dA.to(DEV), dX, c.B, c.T_in, c.T_out, c.C)
    torch.cuda.synchronize()
    assert _guard_ok(buf, dX.numel()), "a write past dX"
    _exact("col2im_s2", c.id, dX, tc.col2im_ref(dA, c.B, c.T_in, c.T_out, c.C))


@pytest.mark.parametrize("dtype", tc.HALF, ids=lambda d: tc.DT_NAME[d])
@pytest.mark.parametrize("n", tc.CAST_LENGTHS)
def test_cast(n, dtype):
    from tw import ops
    x = tc.cast_input(n)
    dst, buf = _guarded((n,), dtype)
    ops.cast_bf16(x.to(DEV), dst)
    torch.cuda.synchronize()
    assert _guard_ok(buf, n), "a write past dst"
    WORST.setdefault("cast", 0.0)
    if not tc.same_bits_or_nan(dst.cpu(), tc.cast_ref(x, dtype)):
        WORST["cast"] = float("inf")
        want = tc.cast_ref(x, dtype)
        bad = ((dst.cpu().view(torch.int16) != want.view(torch.int16)) & ~torch.isnan(want.float())).nonzero()
        i = int(bad[0]) if len(bad) else -1
        pytest.fail(f"cast n={n}: first difference at {i}: x bits {int(x.view(torch.int32)[i]) & 0xFFFFFFFF:#010x}, got "
                    f"{float(dst[i])!r}, want {float(want[i])!r}")


@pytest.mark.parametrize("dtype", (BF16, F16, F32), ids=lambda d: tc.DT_NAME[d])
def test_gelu_bwd(dtype):
    from tw import ops
    pre = tc.gelu_patterns(dtype)
    n = pre.numel()
    for gval in tc.GELU_G:
        g = torch.full((n,), gval, dtype=F32)
        out, buf = _guarded((n,), dtype)
        ops.gelu_bwd(g.to(DEV), pre.to(DEV), out)
        torch.cuda.synchronize()
        assert _guard_ok(buf, n)
        want, bar = tc.gelu_bwd_ref(g, pre, dtype)
        _check("gelu_bwd", f"gelu_bwd {tc.DT_NAME[dtype]} g={gval}", out, want, bar)


@pytest.mark.parametrize("dtype", tc.HALF, ids=lambda d: tc.DT_NAME[d])
def test_gelu_bwd_is_the_gemm_dgelu_epilogue(dtype):
    """tw_gelu_bwd == the GEMM's DGELU epilogue on the same (g, pre), bit for bit, on every finite 16-bit pre pattern:
    dy . I with a 256 x 256 identity W has the accumulator dy exactly, so the epilogue sees r(g) and pre."""
    from tw import ops
    pre = tc.gelu_matrix(tc.gelu_patterns(dtype))
    M, N = pre.shape
    eye = torch.eye(N, dtype=dtype, device=DEV)
    pre_d = pre.to(DEV)
    for gval in tc.GELU_G:
        dy = torch.full((M, N), gval, dtype=dtype, device=DEV)          # r(g)
        via_gemm, gbuf = _guarded((M, N), dtype)
        ops.gemm(dy, eye, via_gemm, M, N, N, lda=N, ldb=N, ldc=N, aux=pre_d, ldaux=N,
                 flags=ops.GEMM_ROUND | ops.GEMM_DGELU)
        direct, dbuf = _guarded((M, N), dtype)
        ops.gelu_bwd(dy, pre_d, direct)
        torch.cuda.synchronize()
        assert _guard_ok(gbuf, M * N) and _guard_ok(dbuf, M * N)
        _exact("gelu_bwd_vs_dgelu", f"gelu_bwd vs DGELU epilogue {tc.DT_NAME[dtype]} g={gval}", direct, via_gemm.cpu())


@pytest.mark.parametrize("n", tc.CLIP_N)
def test_clip_scale(n):
    from tw import ops
    from tw._native import call
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    ws = torch.empty(1024, dtype=F32, device=DEV)
    for max_norm in (2 * float(x.double().norm()), 1.0):
        xd, buf = _guarded((n,), F32)
        xd.copy_(x)
        norm = ops.l2norm(xd, torch.empty(1, dtype=F32, device=DEV), ws)
        call("tw_clip_scale", xd.data_ptr(), n, norm.data_ptr(), float(max_norm), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert _guard_ok(buf, n)
        _exact("clip_scale", f"clip_scale n={n} max={max_norm:g}", xd, tc.clip_ref(x, float(norm.item()), max_norm))


@pytest.mark.parametrize("n", tc.L2_N)
def test_l2norm(n):
    from tw import ops
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
    out = ops.l2norm(x.to(DEV), torch.empty(1, dtype=F32, device=DEV), torch.empty(1024, dtype=F32, device=DEV))
    want = x.double().norm().reshape(1)
    _check("l2norm", f"l2norm n={n}", out, want, tc.l2norm_rel_bound(n) * want)


@pytest.mark.parametrize("case", tc.ADAM_CASES, ids=_ids)
def test_adamw(case):
    from tw import ops
    c, inp = case, tc.adam_build(case)
    p, m, v = (inp[k].to(DEV) for k in ("p", "m", "v"))
    p16 = p16buf = None
    if c.p16 is not None:
        p16, p16buf = _guarded((c.n,), c.p16)
    for k, g in enumerate(inp["grads"]):
        p0, m0, v0 = p.cpu(), m.cpu(), v.cpu()           # each step is judged from the kernel's own previous state
        norm = tc.adam_norm(c, g)
        ops.adamw(p, g.to(DEV), m, v, p16, step=c.step + k, wd=c.wd, norm=None if norm is None else norm.to(DEV),
                  max_norm=tc.ADAM_MAX_NORM if norm is not None else 0.0, **tc.ADAM_HP)
        torch.cuda.synchronize()
        rp, rm, rv, bnd = tc.adam_ref(p0, g, m0, v0, c.step + k, c.wd, norm, **tc.ADAM_HP)
        for nm, got, want in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
            _check("adamw", f"{c.id} step {c.step + k} {nm}", got, want, bnd[nm])
        if p16 is not None:
            assert _guard_ok(p16buf, c.n)
            _exact("adamw", f"{c.id} p16 = RNE(p)", p16, p.cpu().to(c.p16))


@pytest.mark.parametrize("case", tc.COLSUM_CASES, ids=_ids)
def test_colsum(case):
    from tw import ops
    c, inp = case, tc.colsum_build(case)
    want, bound = tc.colsum_ref(c, inp)
    out, buf = _guarded((c.cols,), F32)
    out.copy_(inp["base"])
    x = inp["x"].to(DEV)
    ops.colsum(x.view(-1)[c.offset:], c.ldx, c.rows, c.cols, out, accum=c.accum, round_bf16=c.rounding)
    torch.cuda.synchronize()
    assert _guard_ok(buf, c.cols), "a write past out"
    _check("colsum", c.id, out, want, bound)


@pytest.mark.parametrize("kind", ("all", "none", "some"))
@pytest.mark.parametrize("n", tc.COUNT_N)
def test_count_valid(n, kind):
    from tw import ops
    lab = tc.count_labels(n, kind, torch.Generator().manual_seed(n))
    out = ops.count_valid(lab.to(DEV), torch.full((1,), 12345, dtype=torch.int32, device=DEV))
    WORST.setdefault("count_valid", 0.0)
    assert int(out.item()) == int((lab >= 0).sum())


@pytest.mark.parametrize("dtype", (BF16, F16, F32), ids=lambda d: tc.DT_NAME[d])
def test_mel_to_conv_input(dtype):
    from tw import ops
    mel = torch.randn(2, 80, 7, generator=torch.Generator().manual_seed(7))
    xt, buf = _guarded((2, 9, 80), dtype)
    ops.mel_to_conv_input(mel.to(DEV), xt)
    torch.cuda.synchronize()
    assert _guard_ok(buf, xt.numel())
    _exact("mel_to_conv_input", f"mel_to_conv_input {tc.DT_NAME[dtype]}", xt, tc.mel_ref(mel, dtype))


@pytest.mark.parametrize("tok_dtype,out_dtype", tc.EMBED_CASES, ids=lambda d: tc.DT_NAME[d])
def test_embed_fwd(tok_dtype, out_dtype):
    from tw import ops
    inp = tc.embed_build(tok_dtype, torch.Generator().manual_seed(11))
    rows, D = inp["ids"].numel(), inp["tok"].shape[1]
    out, buf = _guarded((rows, D), out_dtype)
    ops.embed_fwd(inp["ids"].to(DEV), inp["tok"].to(DEV), inp["pos"].to(DEV), out, inp["T"], inp["pos_offset"])
    torch.cuda.synchronize()
    assert _guard_ok(buf, out.numel())
    _exact("embed_fwd", f"embed_fwd {tc.DT_NAME[tok_dtype]}->{tc.DT_NAME[out_dtype]}", out, tc.embed_ref(inp, out_dtype))
