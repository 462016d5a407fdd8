"""tw_gemm_bf16 / tw_gemm_f16 against the cases, the exact references and the comparators of tests/gemm_cases.py (proven
on the CPU by tests/test_gemm_cases_cpu.py): every route, layout, epilogue kind and operand type, bit for bit.

Each test builds its case on the CPU, asks the library which route the call takes on this device, runs ops.gemm once
and compares the whole C (and aux) buffer -- interior, pad columns, the gaps between batch entries and the guard tail --
with the expected one.  The GELU / GELU-backward outputs and the randn cases are compared element by element under the
bounds stated in tests/gemm_cases.py; a miss reports the route, the element and the epilogue.  Where a case names other
kernels for the same call (a forced tile; NOSPLIT: the plan a call without the split-K workspace falls back to), they
run against the same reference.  Each bounded family prints its largest error / bound ratio under -s, with the number
of cases per route and operand type (profiles/gemm_parity.txt holds those lines from an MI355X)."""
import collections

import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
COUNT = collections.Counter()
GELU_BITS = collections.Counter()
EXACT = collections.Counter()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n == 256, f"the route expectations are written for the MI355X's 256 CUs; this device has {n}"
    yield
    for fam, r in sorted(WORST.items()):
        if fam.startswith("exact"):
            print(f"\n[gemm-parity] {fam}: {EXACT[fam, True]} runs bit-identical, {EXACT[fam, False]} not", end="")
        else:
            print(f"\n[gemm-parity] {fam}: max err/bound {r:.3f}", end="")
    for h in ("bf16", "fp16"):
        if GELU_BITS[h, "n"]:
            print(f"\n[gemm-parity] {h} gelu: {GELU_BITS[h, 'diff']} of {GELU_BITS[h, 'n']} outputs differ from the "
                  f"reference value's bits", end="")
    for (route, h), n in sorted(COUNT.items()):
        print(f"\n[gemm-parity] cases {route} {h}: {n}", end="")
    print()


def _call(c, t, C, aux, force):
    from tw import ops
    kw = dict(lda=c.lda, ldb=c.ldb, ldc=c.ldc, a_trans=c.a_trans, b_trans=c.b_trans, bias=t.get("bias"),
              res=t.get("res"), ldr=c.ldr, res_mod=c.res_mod, aux=aux, ldaux=c.ldaux, flags=c.flags | force,
              batch=c.batch, sA=c.sA, sB=c.sB, sC=c.sC, sR=c.sR, sAux=c.sAux)
    plan = ops.gemm_route(t["A"], t["B"], C, c.M, c.N, c.K, cus=0, **kw)
    ops.gemm(t["A"], t["B"], C, c.M, c.N, c.K, alpha=c.alpha, **kw)
    torch.cuda.synchronize()
    return plan


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.id)
def test_gemm(case):
    c = case
    inp = gc.build(c)
    ref = gc.reference(c, inp)
    want_C, want_aux = gc.expected_buffers(c, inp, ref)
    t = {k: inp[k + "_buf"].to(DEV) for k in ("A", "B", "bias", "res") if k + "_buf" in inp}
    h = gc.NAME[c.dtype]
    COUNT[c.route, h] += 1
    fam = f"{c.family} {h}" + (" gelu'" if c.family == "dgelu" else "")
    for force, route in ((c.force, c.route),) + tuple((c.force | f, r) for f, r in c.twins):
        C = inp["C_buf"].to(DEV)
        aux = inp["aux_buf"].to(DEV) if "aux_buf" in inp else None
        plan = _call(c, t, C, aux, force)
        assert plan.route == route, (c.id, plan, route)
        if force == c.force:
            assert (plan.S, plan.m_dp, plan.split_tile, plan.epi) == (c.S, c.m_dp, c.split_tile, c.epi), (c.id, plan)
        what = f"[{plan.route}, {plan.epi}, flags {c.flags:#x}]"
        bad = []
        for name, buf in (("A", inp["A_buf"]), ("B", inp["B_buf"])):         # the operands are read-only
            assert torch.equal(t[name].cpu().view(torch.int16), buf.view(torch.int16)), f"{c.id}: {name} was written"
        if aux is not None:
            want = want_aux if want_aux is not None else inp["aux_buf"]           # DGELU: aux is an input
            bad.append(gc.compare_exact(c, f"aux {what}", aux, want, c.ldaux, c.sAux))
        if c.family == "exact":
            WORST.setdefault(fam, 0.0)
            rep = gc.compare_exact(c, f"C {what}", C, want_C, c.ldc, c.sC)
            EXACT[fam, rep is None] += 1
            bad.append(rep)
        else:
            r, rep = gc.compare_bounded(c, f"C {what}", C, inp["C_buf"], ref["C64"], ref["bound"], c.ldc, c.sC)
            WORST[fam] = max(WORST.get(fam, 0.0), r)
            bad.append(rep)
            if c.family == "gelu":
                got = gc.view(C.cpu(), c.batch, c.M, c.N, c.ldc, c.sC).contiguous()
                GELU_BITS[h, "n"] += got.numel()
                GELU_BITS[h, "diff"] += int((got.view(torch.int16) != ref["C"].view(torch.int16)).sum())
        bad = [b for b in bad if b]
        assert not bad, "\n".join(bad)
