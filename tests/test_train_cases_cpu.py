"""Proves the cases of tests/train_cases.py before any kernel sees them (no GPU): the fp64 references equal torch's
own operators with fp64 autograd (or a second, independent formulation), an honest fp32 evaluation of the same
formulas stays inside every bound in two summation orders, each named wrong arithmetic leaves its bound on a named
case, the case tables reach every instantiation and route of the host dispatchers, and the tables stay small."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_cases as tc
from train_cases import BF16, F16, F32

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "taiwan-whisper_amd", "csrc")


def _ratio(got, want, bound):
    return float(((got.double() - want).abs() / bound.clamp(min=1e-300)).max())


def _sum2(x, order):
    """Row sums in fp32 in two orders: torch's own, and 64 lane chains followed by their sum."""
    if order == 0:
        return x.sum(-1, keepdim=True)
    return x.reshape(x.shape[0], -1, 64).sum(1).sum(-1, keepdim=True)


def _ln_fwd_f32(x, w, b, order, eps=tc.EPS, one_pass=False, divisor=None, drop_eps=False):
    x = x.float()
    D = x.shape[-1]
    mean = _sum2(x, order) / D
    if one_pass:
        var = _sum2(x * x, order) / D - mean * mean
    else:
        var = _sum2((x - mean) ** 2, order) / (divisor or D)
    rstd = torch.rsqrt(var + (0.0 if drop_eps else eps))
    return mean[:, 0], rstd[:, 0], (x - mean) * rstd * w + b


# ------------------------------------------------------------------------------------------------ references
def test_ln_reference_is_torch_layer_norm():
    c = tc.LnBwd(5, 320, F32, F32, True, None)
    inp = tc.ln_bwd_build(c)
    x = inp["x"].double().requires_grad_(True)
    w = inp["w"].double().requires_grad_(True)
    b = torch.zeros(320, dtype=torch.float64, requires_grad=True)
    y = F.layer_norm(x, (320,), w, b, tc.EPS)
    ref = tc.ln_ref(inp["x"], inp["w"], torch.zeros(320))
    assert torch.allclose(y, ref["y"], rtol=1e-12, atol=1e-12)
    # backward: the reference takes the fp32-rounded statistics; with the fp64 ones it is autograd's
    inp64 = dict(inp, mean=ref["mean"], rstd=ref["rstd"])
    y.backward(inp["dy"].double())
    rb = tc.ln_bwd_ref(inp64, accum=False)
    assert torch.allclose(x.grad, rb["dx"], rtol=1e-10, atol=1e-12)
    assert torch.allclose(w.grad, rb["dw"] - inp["dw_base"].double(), rtol=1e-10, atol=1e-12)
    assert torch.allclose(b.grad, rb["db"] - inp["db_base"].double(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("T,ce_w,kl_w,gs", [(1.0, 0.8, 1.0, 1.0), (2.0, 1.0, 0.0, 0.25), (3.0, 0.0, 1.0, 65536.0),
                                           (2.0, 0.8, 1.0, 1.0), (3.0, 0.8, 1.0, 0.25)])
def test_klce_reference_is_oracle(T, ce_w, kl_w, gs):
    from oracle import distill_ref
    c = tc.KlCe(F32, 13, 16, 5, T, ce_w, kl_w, gs)
    inp = tc.klce_build(c)
    lab = inp["labels"]
    nv = int((lab >= 0).sum())
    ref = tc.klce_ref(inp["s"], inp["t"], lab, c.V, T, ce_w, kl_w, gs, nv)
    s = inp["s"][:c.rows, :c.V].double().requires_grad_(True)
    t = inp["t"][:c.rows, :c.V].double()
    ce = F.cross_entropy(s, lab, ignore_index=-100)
    loss08, kl = distill_ref.distill_loss(s[None], t[None], lab[None], ce, temperature=T, kl_weight=kl_w)
    if ce_w == 0.8:
        assert torch.allclose(loss08, ref["out3"][0], rtol=1e-10)
    (gs * (ce_w * ce + kl_w * kl)).backward()
    assert torch.allclose(ce, ref["out3"][1], rtol=1e-12) and torch.allclose(kl, ref["out3"][2], rtol=1e-10, atol=1e-14)
    assert torch.allclose(ce_w * ce + kl_w * kl, ref["out3"][0], rtol=1e-10)
    assert torch.allclose(s.grad, ref["grad"], rtol=1e-9, atol=1e-14 * gs)


def test_helper_references_second_formulation():
    for c in tc.IM2COL_CASES[::7]:
        src = tc.im2col_build(c)
        assert torch.equal(tc.im2col_ref(src, c.T_out, c.stride), tc.im2col_ref_loops(src, c.T_out, c.stride))
    # col2im is the adjoint of the s2 im2col on a zero-padded input: autograd of the unfold, and the inner product
    for c in tc.COL2IM_CASES:
        dA = tc.col2im_build(c)
        x = torch.randn(c.B, c.T_in, c.C, dtype=torch.float64, requires_grad=True)
        xp = F.pad(x, (0, 0, 1, 2))          # p1 on the left; two zero rows cover the last window for odd T_in
        A = tc.im2col_ref(xp, c.T_out, 2)
        (A * dA.double()).sum().backward()
        ref = tc.col2im_ref(dA, c.B, c.T_in, c.T_out, c.C)
        assert torch.allclose(x.grad.reshape(-1, c.C), ref.double(), rtol=0, atol=1e-6), c.id
        assert abs(float(((A * dA.double()).sum() - (x * ref.double().reshape(x.shape)).sum()).detach())) < 1e-4
    x = tc.cast_patterns()
    assert x.numel() == 393216
    assert tc.same_bits_or_nan(tc.cast_ref_bits(x, BF16), tc.cast_ref(x, BF16))
    xs = torch.linspace(-6, 6, 1001, dtype=torch.float64, requires_grad=True)
    F.gelu(xs).sum().backward()
    assert torch.allclose(xs.grad, tc.gelu_grad64(xs.detach()), rtol=1e-12, atol=1e-15)
    mel = torch.randn(2, 80, 7)
    assert torch.equal(tc.mel_ref(mel, BF16)[:, 1:8], mel.permute(0, 2, 1).bfloat16())


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_reference_is_torch_adamw(wd):
    """Five steps, and one at step 1000 from a given state, against torch.optim.AdamW(foreach=False) in fp64 with the
    fp32 hyper-parameters the kernel receives."""
    hp = {k: float(np.float32(v)) for k, v in tc.ADAM_HP.items()}
    wdf = float(np.float32(wd))
    for c in (tc.Adam(1009, wd, "none", 1, 5), tc.Adam(1009, wd, "none", 1000, 1)):
        inp = tc.adam_build(c)
        p = torch.nn.Parameter(inp["p"].double())
        opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wdf,
                                foreach=False)
        if c.step > 1:
            opt.state[p] = {"step": torch.tensor(float(c.step - 1)), "exp_avg": inp["m"].double().clone(),
                            "exp_avg_sq": inp["v"].double().clone()}
        rp, rm, rv = inp["p"].double(), inp["m"].double(), inp["v"].double()
        for k, g in enumerate(inp["grads"]):
            p.grad = g.double()
            opt.step()
            rp, rm, rv, _ = tc.adam_ref(rp, g, rm, rv, c.step + k, wd, None, **tc.ADAM_HP)
            assert torch.allclose(p.detach(), rp, rtol=1e-12, atol=1e-15), (c.id, k)
            assert torch.allclose(opt.state[p]["exp_avg_sq"], rv, rtol=1e-12, atol=1e-300)


# ------------------------------------------------------------------------------------------------ honest fp32 fits
@pytest.mark.parametrize("order", [0, 1])
def test_ln_fwd_honest_fp32_fits(order):
    worst = 0.0
    for c in tc.LN_FWD_CASES:
        inp = tc.ln_fwd_build(c)
        ref = tc.ln_ref(inp["x"], inp["w"], inp["b"])
        bnd = tc.ln_fwd_bounds(inp["x"], inp["w"], ref, c.y_dtype)
        mean, rstd, y = _ln_fwd_f32(inp["x"], inp["w"], inp["b"], order)
        r = max(_ratio(y.to(c.y_dtype), ref["y"], bnd["y"]), _ratio(mean, ref["mean"], bnd["mean"]),
                _ratio(rstd, ref["rstd"], bnd["rstd"]))
        assert r <= 1.0, (c.id, r)
        worst = max(worst, r)
    print("ln_fwd honest fp32 worst err/bound", worst)


@pytest.mark.parametrize("order", [0, 1])
def test_add_ln_honest_fp32_fits(order):
    for c in tc.ADD_LN_CASES:
        inp = tc.add_ln_build(c)
        ref = tc.ln_ref(inp["x_out"], inp["w"], inp["b"])
        bnd = tc.ln_fwd_bounds(inp["x_out"], inp["w"], ref, c.r_dtype)
        mean, rstd, y = _ln_fwd_f32(inp["x_out"], inp["w"], inp["b"], order)
        r = max(_ratio(y.to(c.r_dtype), ref["y"], bnd["y"]), _ratio(mean, ref["mean"], bnd["mean"]),
                _ratio(rstd, ref["rstd"], bnd["rstd"]))
        assert r <= 1.0, (c.id, r)


def _ln_bwd_f32(inp, accum, order, drop_s2=False, half_rows=False):
    x, w, dy = inp["x"].float(), inp["w"], inp["dy"].float()
    mu, rs = inp["mean"][:, None], inp["rstd"][:, None]
    D = x.shape[-1]
    xhat, g = (x - mu) * rs, w * dy
    s1, s2 = _sum2(g, order) / D, _sum2(g * xhat, order) / D
    dx = rs * (g - s1 - (0 if drop_s2 else xhat * s2))
    if accum:
        dx = dx + inp["dx_base"]
    n = x.shape[0] // 2 if half_rows else x.shape[0]
    t = (dy * xhat)[:n]
    dw = t.sum(0) if order == 0 else t.flip(0).sum(0)
    return dx, inp["dw_base"] + dw, inp["db_base"] + (dy[:n].sum(0) if order == 0 else dy[:n].flip(0).sum(0))


@pytest.mark.parametrize("order", [0, 1])
def test_ln_bwd_honest_fp32_fits(order):
    for c in tc.LN_BWD_CASES:
        inp = tc.ln_bwd_build(c)
        ref, dx, dw, db = tc.ln_bwd_ref(inp, c.accum), *_ln_bwd_f32(inp, c.accum, order)
        bnd = tc.ln_bwd_bounds(inp, ref, c.accum)
        for nm, got in (("dx", dx), ("dw", dw), ("db", db)):
            assert _ratio(got, ref[nm], bnd[nm]) <= 1.0, (c.id, nm, _ratio(got, ref[nm], bnd[nm]))


def _klce_f32(c, inp, nv, order, **mut):
    """The kernel's formulas in fp32 torch (logsumexp as max + log sum exp; order 1 sums the reversed row)."""
    V, T = c.V, c.T
    Vs = mut.get("softmax_cols", V)
    lab = inp["labels"]
    s, t = inp["s"][:c.rows, :Vs].float(), inp["t"][:c.rows, :Vs].float()
    valid = lab >= 0
    invT = torch.tensor(1.0 / T, dtype=torch.float32)
    sm_ = (lambda a: a.flip(1).sum(1, keepdim=True)) if order else (lambda a: a.sum(1, keepdim=True))

    def lse(a):
        m = a.max(1, keepdim=True).values
        return m + torch.log(sm_(torch.exp(a - m)))
    lse1, lses, lset = lse(s), lse(s * invT), lse(t * invT)
    sm, q, p = torch.exp(s - lse1), torch.exp(s * invT - lses), torch.exp(t * invT - lset)
    ce = (lse1[:, 0] - s.gather(1, lab.clamp(min=0)[:, None])[:, 0]) * valid
    kl = (sm_(p * (t - s))[:, 0] * invT - lset[:, 0] + lses[:, 0]) * valid
    N = float(max(nv, 1))
    onehot = torch.zeros_like(s).scatter_(1, (lab.clamp(min=0) + mut.get("label_shift", 0))[:, None] % Vs, 1.0)
    gce = torch.tensor(c.gs * c.ce_w / N, dtype=torch.float32)
    gkl = torch.tensor(c.gs * c.kl_w * (1.0 if mut.get("gkl_no_T") else T) / N, dtype=torch.float32)
    grad = ((gce * (sm - onehot) + gkl * (q - p)) * valid[:, None])[:, :V]
    TT = T if mut.get("loss_T1") else T * T
    cem, klm = ce.sum() / N, kl.sum() / N * TT
    return grad.to(c.dtype), torch.stack([ce, kl], 1), torch.stack([c.ce_w * cem + c.kl_w * klm, cem, klm])


def _klce_ratios(c, order=0, **mut):
    inp = tc.klce_build(c)
    nv = int((inp["labels"] >= 0).sum())
    ref = tc.klce_ref(inp["s"], inp["t"], inp["labels"], c.V, c.T, c.ce_w, c.kl_w, c.gs, nv)
    bnd = tc.klce_bounds(ref, c.V, c.T, c.ce_w, c.kl_w, c.dtype)
    grad, row, out3 = _klce_f32(c, inp, nv, order, **mut)
    return {"grad": _ratio(grad, ref["grad"], bnd["grad"]), "row": _ratio(row, ref["row"], bnd["row"]), "out3": _ratio(out3, ref["out3"], bnd["out3"])}


@pytest.mark.parametrize("order", [0, 1])
def test_klce_honest_fp32_fits(order):
    worst = {}
    for c in tc.KLCE_CASES:
        r = _klce_ratios(c, order)
        assert max(r.values()) <= 1.0, (c.id, r)
        worst = {k: max(v, worst.get(k, 0)) for k, v in r.items()}
    print("klce honest fp32 worst err/bound", worst)


def test_helpers_honest_fp32_fit():
    for c in tc.ADAM_CASES:
        inp = tc.adam_build(c)
        p, m, v = inp["p"], inp["m"], inp["v"]
        for k, g in enumerate(inp["grads"]):
            norm = tc.adam_norm(c, g)
            rp, rm, rv, bnd = tc.adam_ref(p, g, m, v, c.step + k, c.wd, norm, **tc.ADAM_HP)
            p, m, v = _adam_f32(p, g, m, v, c.step + k, c.wd, norm)
            for nm, got, want in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
                assert _ratio(got, want, bnd[nm]) <= 1.0, (c.id, k, nm, _ratio(got, want, bnd[nm]))
    for c in tc.COLSUM_CASES:
        inp = tc.colsum_build(c)
        want, bound = tc.colsum_ref(c, inp)
        x = inp["x"][:, c.offset:c.offset + c.cols].float()
        for s in (x.sum(0), x.flip(0).sum(0)):
            s = s.to({0: F32, 1: BF16, 2: F16}[c.rounding]).float()
            assert _ratio(inp["base"] + s if c.accum else s, want, bound) <= 1.0, c.id
    for n in tc.L2_N:
        x = torch.randn(n, generator=torch.Generator().manual_seed(n))
        want = float(x.double().norm())
        for got in (float((x * x).sum().sqrt()), float((x * x).flip(0).sum().sqrt())):
            assert abs(got - want) <= tc.l2norm_rel_bound(n) * want, n


def _adam_f32(p, g, m, v, step, wd, norm, sqrt_bc2=True):
    f = np.float32
    lr, b1, b2, eps = (f(tc.ADAM_HP[k]) for k in ("lr", "b1", "b2", "eps"))
    coef = f(1)
    if norm is not None:
        coef = min(f(1), f(tc.ADAM_MAX_NORM) / (f(norm.item()) + f(1e-6)))
    bc1, bc2 = f(1) - f(b1 ** f(step)), f(1) - f(b2 ** f(step))
    gi = g * coef
    p = p * (f(1) - lr * f(wd))
    m = m + (f(1) - b1) * (gi - m)
    v = v * b2 + (f(1) - b2) * gi * gi
    denom = v.sqrt() / (np.sqrt(bc2) if sqrt_bc2 else bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


# ------------------------------------------------------------------------------------------------ wrong arithmetic
def _fwd_case_ratio(c, **mut):
    inp = tc.ln_fwd_build(c)
    ref = tc.ln_ref(inp["x"], inp["w"], inp["b"])
    bnd = tc.ln_fwd_bounds(inp["x"], inp["w"], ref, c.y_dtype)
    if mut.get("one_pass"):             # in fp32: the mutant is the cancellation itself
        _, rstd, y = _ln_fwd_f32(inp["x"], inp["w"], inp["b"], 0, one_pass=True)
    else:
        x, w, b = inp["x"].double(), inp["w"].double(), inp["b"].double()
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).sum(-1, keepdim=True) / (c.D - 1 if mut.get("dm1") else c.D)
        rstd = (var + (0.0 if mut.get("no_eps") else tc.EPS)) ** -0.5
        y, rstd = (x - mean) * rstd * w + b, rstd[:, 0]
    bad = ~torch.isfinite(y).all() or ~torch.isfinite(rstd).all()
    return float("inf") if bad else max(_ratio(y, ref["y"], bnd["y"]), _ratio(rstd, ref["rstd"], bnd["rstd"]))


def test_wrong_layernorm_does_not_fit():
    assert _fwd_case_ratio(tc.LnFwd(9, 1280, F32, F32, "offset"), one_pass=True) > 1
    assert _fwd_case_ratio(tc.LnFwd(9, 64, BF16, BF16, "offset"), one_pass=True) > 1
    assert _fwd_case_ratio(tc.LnFwd(9, 1280, F32, F32), dm1=True) > 1
    assert _fwd_case_ratio(tc.LnFwd(9, 64, F32, BF16), dm1=True) > 1
    assert _fwd_case_ratio(tc.LnFwd(9, 256, F32, F32, "const"), no_eps=True) > 1
    for c, mut in ((tc.LnBwd(5, 256, F32, F32, False, None), dict(drop_s2=True)),
                   (tc.LnBwd(4101, 768, F32, F32, *tc.LNB_COMBOS[0]), dict(half_rows=True))):
        c = next(k for k in tc.LN_BWD_CASES if (k.rows, k.D, k.x_dtype, k.dy_dtype) == (c.rows, c.D, F32, F32))
        inp = tc.ln_bwd_build(c)
        inp64 = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
        ref = tc.ln_bwd_ref(inp, c.accum)
        bnd = tc.ln_bwd_bounds(inp, ref, c.accum)
        x, w, dy = inp64["x"], inp64["w"], inp64["dy"]
        xhat, g = ref["xhat"], ref["g"]
        rs = inp64["rstd"][:, None]
        dx = rs * (g - g.mean(-1, keepdim=True) - (0 if mut.get("drop_s2") else xhat * (g * xhat).mean(-1, keepdim=True)))
        dx = dx + (inp64["dx_base"] if c.accum else 0)
        n = c.rows // 2 if mut.get("half_rows") else c.rows
        dw = inp64["dw_base"] + (dy * xhat)[:n].sum(0)
        which = "dx" if mut.get("drop_s2") else "dw"
        assert _ratio(dx if which == "dx" else dw, ref[which], bnd[which]) > 1, (c.id, mut)


def test_wrong_klce_does_not_fit():
    base = tc.KlCe(F32, 13, 16, 5, 2.0, 0.8, 1.0, 1.0)
    assert _klce_ratios(base, loss_T1=True)["out3"] > 1
    assert _klce_ratios(base, gkl_no_T=True)["grad"] > 1
    assert _klce_ratios(base, softmax_cols=16)["grad"] > 1          # pad columns in the softmax (V = 13)
    assert _klce_ratios(base, softmax_cols=16)["row"] > 1
    assert _klce_ratios(base, label_shift=1)["grad"] > 1
    assert _klce_ratios(tc.KlCe(BF16, 2049, 2056, 5, 2.0, 0.8, 1.0, 1.0), label_shift=1)["grad"] > 1


def test_wrong_helpers_do_not_fit():
    x = tc.cast_patterns()
    assert not tc.same_bits_or_nan(tc.cast_ref_bits(x, BF16, truncate=True), tc.cast_ref(x, BF16))
    c = next(k for k in tc.ADAM_CASES if k.step == 1000 and k.clip == "none")
    inp = tc.adam_build(c)
    g = inp["grads"][0]
    rp, _, _, bnd = tc.adam_ref(inp["p"], g, inp["m"], inp["v"], 1000, c.wd, None, **tc.ADAM_HP)
    mp, _, _, _ = tc.adam_ref(inp["p"], g, inp["m"], inp["v"], 1000, c.wd, None, sqrt_bc2=False, **tc.ADAM_HP)
    assert _ratio(mp, rp, bnd["p"]) > 1
    c = tc.Col2im(1, 64, 20)
    dA = tc.col2im_build(c)
    assert not torch.equal(tc.col2im_ref(dA, 1, 20, c.T_out, 64), tc.col2im_ref(dA, 1, 20, c.T_out, 64, guard=False))


# ------------------------------------------------------------------------------------------------ coverage, sizes
def test_routes_cover_every_instantiation():
    src = open(os.path.join(CSRC, "layernorm.hip")).read()
    host = src[src.index('extern "C"'):]
    named = set()
    for m in re.finditer(r"ln_fwd_bf16_kernel<(\d)(?:, (true|false))?(?:, (true|false))?>", host):
        n, add, h = m.groups()
        named.add(f"half<{n}{',ADD' if add == 'true' else ''}{',H' if h == 'true' else ''}>")
    for m in re.finditer(r"ln_fwd_kernel<(\d+), (\d+)(, true)?(, true)?>", host):
        v, j, add, rh = m.groups()
        named.add(f"fwd<{v},{j}{',ADD' if add else ''}{',RH' if rh else ''}>")
    named |= {f"bwd<4,{n}>" for n in re.findall(r"TW_LN_BWD\((\d)\);", host)}
    named |= {f"bwd<{v},{j}>" for v, j in re.findall(r"\(ln_bwd_kernel<(\d+), (\d+)>\)", host) if v != "4"}
    assert len(named) == 5 * 3 + 4 + 6, sorted(named)
    reached = {c.route for c in tc.LN_FWD_CASES + tc.ADD_LN_CASES} | {c.route.name for c in tc.LN_BWD_CASES}
    assert named == reached, (sorted(named - reached), sorted(reached - named))
    fam = lambda r: r.name == "bwd<1,20>"
    for one in (True, False):
        assert any(c.route.grid_stride for c in tc.LN_BWD_CASES if fam(c.route) == one)
    for name in {c.route.name for c in tc.LN_BWD_CASES}:
        assert any(c.route.grid_stride for c in tc.LN_BWD_CASES if c.route.name == name), name
    assert any(c.route.capped for c in tc.LN_BWD_CASES) and all(c.D == 1280 for c in tc.LN_BWD_CASES if c.route.capped)
    assert {c.route.capped for c in tc.LN_BWD_CASES if c.D == 1280} == {True, False}
    # every (dx_accum, g16) on every route; dw = db = None once
    for name in {c.route.name for c in tc.LN_BWD_CASES}:
        assert {(c.accum, c.g16) for c in tc.LN_BWD_CASES if c.route.name == name} == set(tc.LNB_COMBOS)
    assert any(not c.params for c in tc.LN_BWD_CASES)
    kl = open(os.path.join(CSRC, "klce.hip")).read()
    assert set(re.findall(r"hipLaunchKernelGGL\(klce_kernel<(\w+)>", kl)) == {"bf16", "f16", "float"}
    assert {c.dtype for c in tc.KLCE_CASES} == {BF16, F16, F32}
    for dt in tc.KLCE_DTYPES:
        vs = {c.V for c in tc.KLCE_CASES if c.dtype == dt}
        assert any(v < 2048 for v in vs) and any(v > 2048 for v in vs)
        assert {c.T for c in tc.KLCE_CASES if c.dtype == dt} == {1.0, 2.0, 3.0}
        assert {(c.ce_w, c.kl_w) for c in tc.KLCE_CASES if c.dtype == dt} == {(0.8, 1.0), (1.0, 0.0), (0.0, 1.0)}
        assert {c.gs for c in tc.KLCE_CASES if c.dtype == dt} == {1.0, 0.25, 65536.0}
        assert any(c.labels == "none" for c in tc.KLCE_CASES if c.dtype == dt)
    assert any(c.ld - c.V >= 16 and c.V % 8 for c in tc.KLCE_CASES)       # ragged chunk + more than one padded chunk


def test_fp16_gradient_does_not_overflow_at_the_large_scale():
    for c in tc.KLCE_CASES:
        if c.dtype == F16 and c.gs > 1:
            inp = tc.klce_build(c)
            nv = int((inp["labels"] >= 0).sum())
            g = tc.klce_ref(inp["s"], inp["t"], inp["labels"], c.V, c.T, c.ce_w, c.kl_w, c.gs, nv)["grad"]
            assert float(g.abs().max()) < 65504 / 1.01, c.id


def test_sizes_stay_small():
    assert tc.largest_tensor_bytes() < tc.MAX_TENSOR_BYTES
    n = sum(len(t) for t in (tc.LN_FWD_CASES, tc.ADD_LN_CASES, tc.LN_BWD_CASES, tc.KLCE_CASES, tc.IM2COL_CASES,
                             tc.COL2IM_CASES, tc.ADAM_CASES, tc.COLSUM_CASES))
    assert n < 1200, n
