"""Cases, operand builders, the reference and the comparators of the GEMM parity suite (tests/test_gemm_parity_gpu.py;
proven on the CPU by tests/test_gemm_cases_cpu.py).  CPU only: torch / numpy, nothing here touches a GPU.

Exact products.  Operands are integers in [-R, R] with K R^2 <= 2^24, so every partial sum of a product, in any order,
under any K split, ring depth or chunk regrouping, is an integer of magnitude <= 2^24: exact in fp32.  alpha is a
power of two; bias, residual and C_old are small integer multiples of a power-of-two unit that alpha divides.  The fp32
value in front of every rounding point is therefore known exactly, each rounding to bf16 / fp16 is torch's RNE cast
of it, and the expected output of every route is known to the bit without asking any kernel.

The reference follows the epilogue order documented in include/tw_hip.h (tw_gemm_bf16 / tw_gemm_f16):
    alpha * acc + bias -> ROUND -> DGELU (x gelu'(aux)) -> GELU (aux <- pre-activation) -> + res[m % res_mod]
    -> + C_old (ACCUM) -> CLAMP16 (the fp16-rounded value clamped to +-64504) -> store as c_dtype.

GELU and GELU backward are not exact: their pre-activation / rounded product is, the activation is compared with the
fp64 function of it under the project's bar (tests/train_cases.py gelu_bwd, tests/test_kernels_gpu.py
test_gemm_gelu_exhaustive): one ulp of the output type at the reference value or 5e-7 |x| (forward) / 5e-7 |g|
(backward), whichever is larger, plus half the smallest fp16 subnormal on fp16.  The ulp is ulp_at(): the project's
relative form, floored at the fp16 subnormal spacing 2^-24 (under the relative form alone the fp16 GELU backward
reached err / bound 1.66 on an MI355X, every miss one step between neighbouring fp16 subnormals, |want| < 6.1e-5).
The bf16 forward reference is the table of gelu_exact_bf16_bits() applied to the pre-activation's bits.

randn cases (non-integer operands, whatever integers cannot excite) carry the any-order bound
    |err| <= K 2^-24 sum_k |a_k b_k| + u |want|,     u = the output type's unit roundoff (0 for fp32).

Buffers.  Every operand and output lives in a flat buffer with a guard tail; rows are `ld` apart, batch entries
`stride` apart.  Pad columns (ld > the row's extent), the gap between batch entries and the guard tail hold NaN in
inputs -- a pad that is multiplied in shows up -- and the sentinel -768 in outputs.  The M x N interior of C holds NaN
where ACCUM is off (C_old must not be read) and the integer C_old where it is on; the interior of a GELU aux holds NaN.

Routes the table leaves out (tests/test_gemm_cases_cpu.py lists exactly these):
  persistent_edges / bf16: the bf16 persistent kernel has ragged tiles of its own, the planner never yields the route.
  t256x128_s3, t256x128_s2, t128_ring4, persistent on fp16 transposed layouts: dispatch<H, AT, BT> instantiates the
    rings and the persistent kernel for K-major operands only on fp16; the planner falls back to t128.
(route, epilogue kind) pairs: every pair the planner produces over the table's shapes, layouts, epilogues and routing
flags appears per operand type; tests/test_gemm_cases_cpu.py derives that set from the planner and names what is left
out.  rounds_sk_tail with m_dp > 0 (16.8 M outputs a case) runs one exact and one randn case per type; its kinds run at
m_dp = 0.
The plan of a call that cannot get the split-K workspace is run through its NOSPLIT twin (the same kernel: the CPU test
checks that the two plans agree); the workspace itself cannot be taken away from a test.
"""
import collections
import math
import zlib

import numpy as np
import torch

from gemm_routes import (F_ACCUM, F_AUX_OUT, F_CLAMP16, F_DGELU, F_GELU, F_ROUND, NOSPLIT, TILE128,
                         TILE256, TILE256PP, TILE256x128, TILE256x128_S2)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SENTINEL = -768.0
GUARD = 256
CLAMP = 64504.0
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
ULP = {BF16: 2.0 ** -7, F16: 2.0 ** -10, F32: 2.0 ** -23}          # one ulp relative to the value (train_cases)
UNIT = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 0.0}                # unit roundoff
F16_HALF_SUB = 2.0 ** -25


def GROUP_M(g):
    return g << 24


# id; dtype (operand type); a_trans, b_trans; M N K; lda ldb ldc ldr ldaux; batch, sA sB sC sR sAux; alpha; bias (bool);
# flags (epilogue bits without BIAS / RES); c_dtype; res_dtype (None: no residual); res_mod; force (routing bits);
# route, S, m_dp, split_tile, epi: the plan expected on 256 CUs; no_ws: the route expected without the split-K
# workspace (None: not asked); twins: ((extra routing bits, route), ...) run against the same reference;
# family: exact / gelu / dgelu / randn; R: the operand amplitude
Case = collections.namedtuple(
    "Case", "id dtype a_trans b_trans M N K lda ldb ldc ldr ldaux batch sA sB sC sR sAux alpha bias flags c_dtype "
            "res_dtype res_mod force route S m_dp split_tile epi no_ws twins family R")

# ------------------------------------------------------------------------------------------------ epilogue specs
# name -> (c16, bias, flags, res: None / "h" (operand type) / "f" (fp32), res_mod, family, fast kind, alpha: 1 / 0.5)
Spec = collections.namedtuple("Spec", "c16 bias flags res res_mod family kind half")
SPECS = {
    "store16": Spec(True, True, F_ROUND, None, 0, "exact", "store_bf16", False),
    "store16_nb": Spec(True, False, F_ROUND, None, 0, "exact", "store_bf16", True),
    "store32": Spec(False, False, 0, None, 0, "exact", "store_f32", False),
    "store32_br": Spec(False, True, F_ROUND, None, 0, "exact", "store_f32", True),
    "gelu": Spec(True, True, F_ROUND | F_GELU, None, 0, "gelu", "gelu", False),
    "gelu_aux": Spec(True, True, F_ROUND | F_GELU | F_AUX_OUT, None, 0, "gelu", "gelu_aux", False),
    "res16": Spec(True, True, F_ROUND, "h", 0, "exact", "res_bf16", False),
    "res32": Spec(False, True, F_ROUND, "f", 0, "exact", "res_f32", False),
    "dgelu": Spec(True, False, F_ROUND | F_DGELU, None, 0, "dgelu", "dgelu", False),
    # always the generic epilogue
    "accum32": Spec(False, False, F_ROUND | F_ACCUM, None, 0, "exact", "generic", False),
    "accum32_ba": Spec(False, True, F_ACCUM, None, 0, "exact", "generic", True),
    "resmod32": Spec(False, True, F_ROUND, "f", 100, "exact", "generic", False),
    "resmod16": Spec(True, True, F_ROUND, "h", 100, "exact", "generic", True),
    "res_other": Spec(True, True, F_ROUND, "f", 0, "exact", "generic", False),
    "res_accum": Spec(False, True, F_ROUND | F_ACCUM, "f", 0, "exact", "generic", False),
    "res_accum16": Spec(True, True, F_ROUND | F_ACCUM, "h", 0, "exact", "generic", False),
    # GELU backward followed by a residual / C_old (fp32 C: the sum is not rounded to 16 bits again)
    "dgelu_res32": Spec(False, False, F_ROUND | F_DGELU, "f", 0, "dgelu", "generic", False),
    "dgelu_accum32": Spec(False, False, F_ROUND | F_DGELU | F_ACCUM, None, 0, "dgelu", "generic", False),
    # fp16 only
    "clamp16": Spec(True, True, F_ROUND | F_CLAMP16, "h", 0, "exact", "res_bf16", False),
    "clamp_res32": Spec(False, True, F_ROUND | F_CLAMP16, "f", 0, "exact", "generic", False),
    "clamp_accum": Spec(True, True, F_ROUND | F_CLAMP16 | F_ACCUM, "h", 0, "exact", "generic", False),
}
FWD = ("store16", "gelu_aux", "res32", "store32", "gelu", "res16", "resmod32", "accum32_ba", "res_other", "res_accum",
       "store32_br", "store16_nb", "resmod16", "res_accum16", "dgelu", "dgelu_res32", "dgelu_accum32")
FWD_F16 = FWD + ("clamp16", "clamp_res32", "clamp_accum")
DW = ("accum32", "store32", "accum32_ba")
DX = ("store16_nb", "dgelu", "store32", "dgelu_res32", "dgelu_accum32")


def amplitude(dtype, K):
    return min(int(math.isqrt((1 << 24) // K)), 255 if dtype == BF16 else 2047)


def _pow2_floor(x):
    return 2.0 ** math.floor(math.log2(x))


def pick_alpha(dtype, K, R, spec):
    """A power of two.  sigma = sqrt(K) R^2 / 3 is the standard deviation of the integer accumulator.  GELU: six sigma
    at 8 (pre-activations in about [-8, 8]); DGELU: sigma at 1; fp16: bias, residual and C_old included, twelve sigma
    below 60000 (finite) -- sixteen times that under CLAMP16, so most values pass +-64504; bf16: 1, or 0.5."""
    sigma = math.sqrt(K) * R * R / 3.0
    if spec.family == "gelu":
        return _pow2_floor(8.0 / (6.0 * sigma))
    if spec.family == "dgelu":
        return _pow2_floor(1.0 / sigma)
    if dtype == F16:
        a = _pow2_floor(60000.0 / (12.0 * sigma))
        if spec.flags & F_CLAMP16:
            a *= 16.0
        return a * (0.5 if spec.half else 1.0)
    return 0.5 if spec.half else 1.0


def unit_of(c):
    """The power of two bias, residual and C_old are integer multiples of: about an eighth of alpha sigma, never below
    alpha (so alpha acc + bias stays a multiple of alpha: exact in fp32)."""
    sigma = math.sqrt(c.K) * c.R * c.R / 3.0
    boost = 16.0 if c.flags & F_CLAMP16 else 1.0          # (pick_alpha's; the addends themselves stay finite in fp16)
    return max(_pow2_floor(c.alpha * sigma / boost) / 8.0, c.alpha)


def _up8(x):
    return (x + 7) // 8 * 8


def _kind(spec, ldc, ldr, ldaux, batch, sC, sR, sAux):
    """The epilogue kind the host is expected to pick: the spec's fast kind, demoted to generic by a leading dimension
    or batch stride that breaks the 16-byte vectors (8 elements of a 16-bit row, 4 of an fp32 one)."""
    a = 8 if spec.c16 else 4
    ok = ldc % a == 0 and (batch == 1 or sC % a == 0)
    if spec.kind in ("gelu_aux", "dgelu"):
        ok = ok and ldaux % 8 == 0 and (batch == 1 or sAux % 8 == 0)
    if spec.kind in ("res_bf16", "res_f32"):
        ok = ok and ldr % a == 0 and (batch == 1 or sR % a == 0)
    return spec.kind if ok and spec.kind != "generic" else "generic"


def mk(dtype, route, M, N, K, spec, *, at=0, bt=0, pad=False, batch=1, force=0, S=0, m_dp=0, split_tile=0, no_ws=None,
       twins=(), ldc=None, ldr=None, ldaux=None, sC_extra=0, family=None, tag="", alpha=None):
    """A case.  pad: every leading dimension 8 past the 8-aligned extent, batch entries 16 past the dense stride."""
    sp = SPECS[spec]
    p = 8 if pad else 0
    lda = (_up8(M) if at else _up8(K)) + p
    ldb = (_up8(N) if bt else _up8(K)) + p
    ldc = (_up8(N) + p if pad else N) if ldc is None else ldc
    ldr = (_up8(N) + p if pad else N) if ldr is None else ldr
    ldaux = (_up8(N) + p if pad else N) if ldaux is None else ldaux
    gap = 16 if pad else 0
    sA, sB = (K if at else M) * lda + gap, (K if bt else N) * ldb + gap
    sC, sAux = M * ldc + gap + sC_extra, M * ldaux + gap
    sR = (sp.res_mod or M) * ldr + gap
    fam = family or sp.family
    R = amplitude(dtype, K)
    al = pick_alpha(dtype, K, R, sp) if alpha is None else alpha
    if fam == "randn":
        al = 1.0
    epi = _kind(sp, ldc, ldr, ldaux, batch, sC, sR, sAux)
    h = NAME[dtype]
    lay = "nt"[at] + "nt"[bt]
    cid = f"{h}-{route}-{lay}-{spec}-{M}x{N}x{K}" + ("-pad" if pad else "") + (f"-b{batch}" if batch > 1 else "") + \
        (f"-{tag}" if tag else "")
    return Case(cid, dtype, bool(at), bool(bt), M, N, K, lda, ldb, ldc, ldr, ldaux, batch, sA, sB, sC, sR, sAux, al,
                sp.bias, sp.flags, dtype if sp.c16 else F32, {None: None, "h": dtype, "f": F32}[sp.res], sp.res_mod,
                force, route, S, m_dp, split_tile, epi, no_ws, tuple(twins), fam, R)


# ------------------------------------------------------------------------------------------------ the table
EDGE_M = (1, 8, 127, 128, 129, 255, 256, 257)
EDGE_M8 = (8, 16, 120, 128, 136, 248, 256, 264)            # where the layout needs 8-aligned extents
EDGE_K = (8, 64, 72, 128, 192, 200, 256, 320)
FORCE = {"t128": TILE128, "t256": TILE256, "t256x128_s3": TILE256x128, "t256x128_s2": TILE256x128 | TILE256x128_S2,
         "persistent": TILE256PP}
# the other kernels a K-major call is also run on (same reference): every forced tile computes the same product
KM_TWINS = {"t128": ((TILE256, "t256"),), "t256": (), "t256x128_s3": (), "t256x128_s2": (), "persistent": ()}


def _f16_pp_route(M, N, K, batch, kind, res_mod):
    """Where the fp16 forced-persistent call lands: the fp16 persistent kernel runs whole 256 x 256 tiles with a fast
    epilogue and K % 64 == 0; a ragged grid takes the edge-strip route when M, N >= 256 (unbatched, plain residual),
    everything else the 128 x 128 kernel (its 4-stage ring: every such grid here has at most 256 tiles)."""
    assert -(-M // 128) * -(-N // 128) * batch <= 256
    if M % 256 or N % 256:
        ok = K % 64 == 0 and kind != "generic" and batch == 1 and res_mod == 0 and M >= 256 and N >= 256
        return "persistent_edges" if ok else "t128_ring4"
    return "t128_ring4" if (K % 64 or kind == "generic") else "persistent"


def _forced_cases():
    out = []
    for dtype in (BF16, F16):
        for kern in ("t128", "t256", "t256x128_s3", "t256x128_s2", "persistent"):
            for at, bt in ((0, 0), (0, 1), (1, 0), (1, 1)):
                kmajor = not at and not bt
                if kern == "persistent" and not kmajor:
                    continue                      # the forced persistent kernel is K-major only
                rings = kern in ("t256x128_s3", "t256x128_s2")
                if dtype == F16 and rings and not kmajor:
                    continue                      # not instantiated (module docstring)
                specs = (FWD_F16 if dtype == F16 else FWD) if kmajor else DW if (at and bt) else DX
                Ms = EDGE_M8 if at else EDGE_M
                Ns = EDGE_M8 if bt else EDGE_M
                shapes = [(Ms[i], Ns[(i + 3) % 8], EDGE_K[(i + 5) % 8]) for i in range(8)]
                shapes += [(Ms[(i + 4) % 8], Ns[i], EDGE_K[i]) for i in range(8)] if kmajor else []
                shapes.append((Ms[6], Ns[4], 5128 if (at and bt) else 5120))       # one long K (dW: a K tail too)
                shapes.append((Ms[7], Ns[7], EDGE_K[3]))                           # 2 x 2 tiles of 256, ragged both ways
                for i, (M, N, K) in enumerate(shapes):
                    spec = specs[i % len(specs)]
                    pad = i % 2 == 1
                    c = mk(dtype, kern, M, N, K, spec, at=at, bt=bt, pad=pad, force=FORCE[kern],
                           twins=KM_TWINS[kern] if kmajor and i % 4 == 0 else ())
                    if dtype == F16 and kern == "persistent":
                        c = c._replace(route=_f16_pp_route(M, N, K, 1, c.epi, c.res_mod))
                        c = c._replace(id=c.id.replace("-persistent-", f"-{c.route}-") + "-pp")
                    out.append(c)
                # every epilogue the layout uses, on a grid with whole and ragged tiles (2 x 2 tiles, both edges ragged)
                for j, spec in enumerate(specs):
                    M, N = (264, 264) if kern in ("t128", "t256x128_s3", "t256x128_s2") else (520, 520)
                    Kt = 192 if (dtype == F16 and kern == "persistent") else 72          # (the edge strips: K % 64 == 0)
                    c = mk(dtype, kern, M, N, Kt if j % 2 else 128, spec, at=at, bt=bt, pad=True, force=FORCE[kern],
                           tag="epi")
                    if dtype == F16 and kern == "persistent":
                        c = c._replace(route=_f16_pp_route(M, N, c.K, 1, c.epi, c.res_mod))
                        c = c._replace(id=c.id.replace("-persistent-", f"-{c.route}-") + "-pp")
                    out.append(c)
                if dtype == F16 and kern == "persistent":       # whole tiles: the fp16 persistent kernel itself
                    for j, spec in enumerate(specs):
                        K = 192 if j % 2 else 128
                        c = mk(dtype, kern, 512, 256, K, spec, pad=j % 4 >= 2, force=FORCE[kern], tag="full")
                        c = c._replace(route=_f16_pp_route(512, 256, K, 1, c.epi, c.res_mod))
                        out.append(c._replace(id=c.id.replace("-persistent-", f"-{c.route}-") + "-pp"))
    return out


def _batched_cases():
    out = []
    for dtype in (BF16, F16):
        for kern in ("t128", "t256", "t256x128_s3", "t256x128_s2", "persistent"):
            for j, spec in enumerate(("store16", "gelu_aux", "res16", "res32", "resmod32")):
                M, N, K = (136, 264, 72) if kern != "persistent" else (256, 512, 128)
                c = mk(dtype, kern, M, N, K, spec, pad=True, batch=3, force=FORCE[kern])
                if dtype == F16 and kern == "persistent":
                    c = c._replace(route=_f16_pp_route(M, N, K, 3, c.epi, c.res_mod))
                    c = c._replace(id=c.id.replace("-persistent-", f"-{c.route}-") + "-pp")
                out.append(c)
            # a batch stride of C that breaks its 16-byte alignment: the generic epilogue
            M, N, K = (136, 264, 72) if kern != "persistent" else (256, 512, 128)
            c = mk(dtype, kern, M, N, K, "store16", batch=3, force=FORCE[kern], sC_extra=4, tag="sC4")
            if dtype == F16 and kern == "persistent":
                c = c._replace(route="t128_ring4", id=c.id.replace("-persistent-", "-t128_ring4-") + "-pp")
            out.append(c)
        for at, bt, spec in ((0, 1, "dgelu"), (1, 0, "store16_nb"), (1, 1, "accum32")):
            for kern in ("t128", "t256"):
                out.append(mk(dtype, kern, 136, 264, 72, spec, at=at, bt=bt, pad=True, batch=3, force=FORCE[kern]))
    return out


def _group_cases():
    """GEMM_GROUP_M(g) on the persistent kernel, 5 x 3 tiles: the m-tile count is no multiple of 3 or 8; a tile that is
    skipped leaves NaN, one written by the wrong coordinates differs."""
    out = []
    for dtype in (BF16, F16):
        for g in (1, 3, 8):
            out.append(mk(dtype, "persistent", 1280, 768, 64, "store16", force=TILE256PP | GROUP_M(g), tag=f"g{g}"))
        out.append(mk(dtype, "t128", 520, 392, 72, "store16", force=TILE128 | GROUP_M(3), tag="g3"))
    return out


def _skinny_cases():
    out = []
    Ms, Ns, Ks = (1, 5, 32, 33, 64, 65, 128), (1, 15, 16, 17, 51, 264), (8, 40, 72, 1280)
    for dtype in (BF16, F16):
        specs = FWD_F16 if dtype == F16 else FWD
        n = 0
        for i, M in enumerate(Ms):
            for j in range(2):
                N, K = Ns[(i + 3 * j) % 6], Ks[(i + j) % 4]
                rb = 2 if M > 64 else 1
                S = min(-(-512 // (-(-N // 16) * rb)), -(-K // 32) // 4)
                S = 1 if M <= 32 else max(S, 1)
                out.append(mk(dtype, "skinny_splitk" if S > 1 else "skinny", M, N, K, specs[n % len(specs)], pad=n % 2 == 1,
                              S=S, no_ws="skinny", twins=((NOSPLIT, "skinny"),) if S > 1 else ()))
                n += 1
        # the unsplit kernel with every epilogue (M <= 32 never splits)
        for j, spec in enumerate(specs):
            M, N, K = ((5, 264, 72), (32, 16, 1280))[j % 2]
            out.append(mk(dtype, "skinny", M, N, K, spec, pad=j % 4 >= 2, S=1, no_ws="skinny", tag="epi"))
        # skinny_splitk with every epilogue, on the two shapes of the issue
        for j, spec in enumerate(specs):
            M, N, K = ((65, 40, 264), (128, 200, 1280))[j % 2]
            rb = 2
            S = min(-(-512 // (-(-N // 16) * rb)), -(-K // 32) // 4)
            out.append(mk(dtype, "skinny_splitk", M, N, K, spec, pad=j % 4 >= 2, S=S, no_ws="skinny",
                          twins=((NOSPLIT, "skinny"),), tag="epi"))
    return out


def _planned_cases():
    """The routes the planner picks by itself at the smallest shapes that reach them (asked of the planner on the CPU:
    tests/test_gemm_cases_cpu.py)."""
    out = []
    for dtype in (BF16, F16):
        fwd = FWD_F16 if dtype == F16 else FWD
        # t128_ring4: the default for K-major grids of at most 256 128-tiles
        for j, spec in enumerate(fwd):
            M, N, K = ((129, 136, 72), (257, 264, 200), (300, 200, 256), (136, 129, 8))[j % 4]
            out.append(mk(dtype, "t128_ring4", M, N, K, spec, pad=j % 2 == 1, twins=((TILE128, "t128"),)))
        out.append(mk(dtype, "t128_ring4", 264, 136, 5120 - 64, "store16"))
        # dW split-K: both operands MN-major, fp32 C, flags within {ROUND, ACCUM}
        half = lambda K: 0.5 * pick_alpha(dtype, K, amplitude(dtype, K), SPECS["accum32"])
        for spec, al in (("accum32", None), ("store32", None), ("accum32", half)):
            out.append(mk(dtype, "splitk_dw", 136, 136, 1024, spec, at=1, bt=1, S=2, split_tile=128, no_ws="t128",
                          twins=((NOSPLIT, "t128"),), alpha=al and al(1024), tag="a" if al else ""))
            out.append(mk(dtype, "splitk_dw", 200, 264, 2048, spec, at=1, bt=1, pad=True, S=4, split_tile=128,
                          no_ws="t128", twins=((NOSPLIT, "t128"),), alpha=al and al(2048), tag="a" if al else ""))
        out.append(mk(dtype, "splitk_dw", 776, 3080, 6144, "accum32", at=1, bt=1, S=4, split_tile=256, no_ws="t128",
                      twins=((NOSPLIT, "t128"),)))
        # rounds_sk_tail with m_dp = 0: less than one round of 256-tiles, K >= 3072
        # (a row-periodic residual keeps off the route; fp16 runs it with a fast epilogue only)
        sk = tuple(s for s in fwd if not SPECS[s].res_mod and (dtype == BF16 or SPECS[s].kind != "generic"))
        for j, spec in enumerate(sk):
            if dtype == BF16:
                M, N, K = ((256, 264, 3072), (300, 520, 3072))[j % 2]
            else:
                M, N, K = ((256, 256, 3072), (512, 768, 3072))[j % 2]      # fp16: whole 256 x 256 tiles only
            out.append(mk(dtype, "rounds_sk_tail", M, N, K, spec, pad=j % 4 >= 2, S=12, m_dp=0, no_ws="t128_ring4",
                          twins=((NOSPLIT, "t128_ring4"),) if j < 4 else ()))
        # persistent_edges (fp16) and the fp16 fall-backs to t128 come from the forced-persistent cases; the planner's
        # own persistent + edges needs >= 256 256-tiles and sits with the large grids below
    return out


def _large_cases():
    """The routes only a grid of at least 256 256-tiles reaches (16.8 M outputs a case): the only cases above 32 MB per
    tensor.  rounds_dp_tail meets every epilogue kind here, on a ragged tail (128 whole m-tile rows + 100 rows) and on
    the 17 x 16 tiles that rounds_sk_tail falls back to without its workspace (the same m_dp = 16 split at K = 64:
    that fall-back itself cannot be forced, NOSPLIT keeps off both tail routes)."""
    out = []
    for dtype in (BF16, F16):
        out.append(mk(dtype, "rounds_sk_tail", 4352, 4096, 3072, "res16", S=8, m_dp=16, no_ws="rounds_dp_tail"))
        kinds = ("store16", "gelu_aux", "store32", "gelu", "res16", "res32", "dgelu") + \
            (("accum32_ba",) if dtype == BF16 else ())          # (fp16 runs the route with a fast epilogue only)
        for j, spec in enumerate(kinds):
            M, N, m_dp = ((32868, 512, 128), (4352, 4096, 16))[j % 2]
            out.append(mk(dtype, "rounds_dp_tail", M, N, 64, spec, m_dp=m_dp, pad=j % 4 >= 2))
        out.append(mk(dtype, "persistent", 4096, 4096, 1024, "store16"))
        for route, M, N, K, kw in (("rounds_sk_tail", 4352, 4096, 3072, dict(S=8, m_dp=16, no_ws="rounds_dp_tail")),
                                   ("rounds_dp_tail", 32868, 512, 64, dict(m_dp=128)),
                                   ("persistent", 4096, 4096, 1024, {})):
            out.append(mk(dtype, route, M, N, K, "store16_nb", family="randn", tag="randn", **kw))
        out.append(mk(dtype, "persistent", 4096, 4096, 1024, "store32", family="randn", tag="randn"))
    return out


def _build_table():
    cases = _forced_cases() + _batched_cases() + _group_cases() + _skinny_cases() + _planned_cases() + _large_cases()
    ids = [c.id for c in cases]
    dup = {i for i in ids if ids.count(i) > 1}
    assert not dup, sorted(dup)
    return cases


CASES = _build_table()
LARGE = frozenset(c.id for c in CASES if c.M * c.N * c.batch > 8 << 20)


def shapes():
    return sorted({(c.M, c.N, c.K) for c in CASES})


# ------------------------------------------------------------------------------------------------ buffers
def place(x, ld, stride, fill, dtype):
    """[batch, rows, cols] into a flat buffer: rows `ld` apart, batch entries `stride` apart, `fill` in the pad
    columns, between the entries and in the GUARD tail."""
    b, r, c = x.shape
    assert ld >= c and (b == 1 or stride >= r * ld)
    buf = torch.full(((b - 1) * stride + r * ld + GUARD,), fill, dtype=dtype)
    buf.as_strided((b, r, c), (stride, ld, 1)).copy_(x)
    return buf


def view(buf, b, r, c, ld, stride):
    return buf.as_strided((b, r, c), (stride, ld, 1))


def interior(n, b, r, c, ld, stride):
    m = torch.zeros(n, dtype=torch.bool)
    m.as_strided((b, r, c), (stride, ld, 1)).fill_(True)
    return m


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.id.encode()))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def build(c):
    """The CPU tensors of a case.  Logical operands: A [batch, M, K], B [batch, N, K] (fp32 holding values of the operand
    type), bias [N], res [batch, rows, N], c_old [batch, M, N], aux_in [batch, M, N] (DGELU); the flat buffers the kernel
    gets: A_buf, B_buf, bias_buf, res_buf, C_buf, aux_buf."""
    g, h, nan = _gen(c), c.dtype, float("nan")
    b, M, N, K = c.batch, c.M, c.N, c.K
    if c.family == "randn":
        A = torch.randn(b, M, K, generator=g).to(h).float()
        B = torch.randn(b, N, K, generator=g).to(h).float()
    else:
        A, B = _ints(g, (b, M, K), -c.R, c.R), _ints(g, (b, N, K), -c.R, c.R)
    u = unit_of(c)
    inp = {"A": A, "B": B, "unit": u}
    inp["A_buf"] = place(A.transpose(1, 2) if c.a_trans else A, c.lda, c.sA, nan, h)
    inp["B_buf"] = place(B.transpose(1, 2) if c.b_trans else B, c.ldb, c.sB, nan, h)
    if c.bias:
        inp["bias"] = _ints(g, (N,), -8, 8) * u
        inp["bias_buf"] = place(inp["bias"].view(1, 1, N), N, N, nan, h)
    if c.res_dtype is not None:
        rows = c.res_mod or M
        inp["res"] = _ints(g, (b, rows, N), -16, 16) * u
        inp["res_buf"] = place(inp["res"], c.ldr, c.sR, nan, c.res_dtype)
    if c.flags & F_ACCUM:
        inp["c_old"] = _ints(g, (b, M, N), -16, 16) * u
        inp["C_buf"] = place(inp["c_old"], c.ldc, c.sC, SENTINEL, c.c_dtype)
    else:
        inp["C_buf"] = place(torch.full((b, M, N), nan), c.ldc, c.sC, SENTINEL, c.c_dtype)
    if c.flags & F_DGELU:
        inp["aux_in"] = _ints(g, (b, M, N), -64, 64) / 8.0           # pre-activations on a grid of [-8, 8]
        inp["aux_buf"] = place(inp["aux_in"], c.ldaux, c.sAux, nan, h)
    elif c.flags & F_AUX_OUT:
        inp["aux_buf"] = place(torch.full((b, M, N), nan), c.ldaux, c.sAux, SENTINEL, h)
    return inp


# ------------------------------------------------------------------------------------------------ reference
def gelu_exact_bf16_bits():
    """bf16 bits of GELU for every bf16 bit pattern: PyTorch's erf-form formula in fp32 (reference),
    x * 0.5 * (1 + erf(x * M_SQRT1_2)) (the reference's autocast F.gelu), with a correctly rounded
    fp32 erf (math.erf in double, rounded once), then bf16 round-to-nearest-even;
    +inf -> +inf, -inf -> -0, NaN -> NaN (the kernels' stated edge behaviour)."""
    bits = np.arange(1 << 16, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        x = (bits << 16).view(np.float32).copy()
        xa = x * np.float32(0.70710678118654752440)
    fin = np.isfinite(x)
    e = np.zeros_like(x)
    e[fin] = np.array([math.erf(v) for v in xa[fin].astype(np.float64).tolist()]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        g = (x * np.float32(0.5)) * (np.float32(1.0) + e)
    out = torch.from_numpy(g).bfloat16().view(torch.int16).numpy().view(np.uint16).copy()
    out[np.isposinf(x)] = 0x7f80
    out[np.isneginf(x)] = 0x8000
    out[np.isnan(x)] = 0x7fc0
    return bits.astype(np.uint16), out


_GELU_TABLE = []


def gelu_bf16_table(pre):
    """GELU of a bf16 tensor through the table of gelu_exact_bf16_bits -> bf16."""
    if not _GELU_TABLE:
        _GELU_TABLE.append(torch.from_numpy(gelu_exact_bf16_bits()[1].astype(np.int32)))
    idx = pre.view(torch.int16).to(torch.int32) & 0xffff
    return _GELU_TABLE[0][idx.long()].to(torch.int16).view(torch.bfloat16)


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_grad64(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def ulp_at(w64, dtype):
    """One ulp of the 16-bit type at the reference value: the project's relative form |w| 2^-7 (bf16) / |w| 2^-10 (fp16)
    (tests/train_cases.py), and never less than the spacing of the type at w -- 2^-24 for an fp16 subnormal, where the
    relative form falls below the distance between neighbouring values and a reference that sits next to a rounding
    boundary is one such step from its neighbour."""
    rel = w64.abs() * ULP[dtype]
    if dtype == F16:
        return rel.clamp(min=2.0 ** -24)
    return rel


def _exact32(v64, what):
    v = v64.float()
    if not bool((v.double() == v64).all()):
        raise AssertionError(f"{what} is not exact in fp32")
    return v


def reference(c, inp, *, bias_after_round=False, res_rows=None, A=None):
    """The documented epilogue on the exact accumulator -> dict:
    C: [batch, M, N] in c_dtype (exact families: every bit expected; bounded families: the reference value rounded),
    C64 / bound: fp64 reference and per-element bound (gelu, dgelu, randn), aux: the expected pre-activation (AUX_OUT),
    inexact: 16-bit outputs whose value before the last rounding was a tie or not representable (the spread test).
    The keyword arguments plant faults for tests/test_gemm_cases_cpu.py: the bias added after the rounding, residual
    rows taken from `res_rows` [batch, M, N] (row m instead of m % res_mod), another A."""
    h, f = c.dtype, c.flags
    A = inp["A"] if A is None else A
    Bt = inp["B"].transpose(1, 2)
    out = {}
    if c.family == "randn":
        acc = torch.matmul(A.double(), Bt.double())
        mag = torch.matmul(A.abs(), Bt.abs()).double()
        assert not f & ~F_ROUND and not c.bias and c.res_dtype is None
        out["C64"], out["C"] = acc, acc.to(c.c_dtype)
        out["bound"] = c.K * 2.0 ** -24 * mag + UNIT[c.c_dtype] * acc.abs()
        return out
    acc = torch.matmul(A, Bt)                                   # fp32, exact: every partial sum is an integer <= 2^24
    assert float(acc.abs().max()) <= 2 ** 24
    v64 = acc.double() * c.alpha
    if c.bias and not bias_after_round:
        v64 = v64 + inp["bias"].to(h).double()
    v = _exact32(v64, "alpha * acc + bias")
    if f & F_ROUND:
        v = v.to(h).float()
    if c.bias and bias_after_round:
        v = v + inp["bias"].to(h).float()
    if f & F_DGELU:
        assert not f & (F_GELU | F_CLAMP16)
        g64 = v.double()
        w64 = (g64 * gelu_grad64(inp["aux_in"].to(h))).to(h).double()
        bound = torch.maximum(ulp_at(w64, h), 5e-7 * g64.abs()) + (F16_HALF_SUB if h == F16 else 0.0)
        if c.res_dtype is not None or f & F_ACCUM:
            # one fp32 addition behind the 16-bit GELU-backward value, stored as fp32: its error, plus the rounding
            # of the sum to fp32 (2^-24 relative)
            assert c.c_dtype == F32 and not c.res_mod and (c.res_dtype is None) != (not f & F_ACCUM)
            add = inp["res"].to(c.res_dtype).double() if c.res_dtype is not None else inp["c_old"].double()
            w64 = w64 + add
            bound = bound + 2.0 ** -24 * (w64.abs() + bound)
        else:
            assert c.c_dtype == h
        out["C64"], out["C"], out["bound"] = w64, w64.to(c.c_dtype), bound
        return out
    if f & F_GELU:
        assert not f & (F_ACCUM | F_CLAMP16) and c.res_dtype is None and c.c_dtype == h
        pre = v.to(h)
        if f & F_AUX_OUT:
            out["aux"] = pre
        w = gelu_bf16_table(pre) if h == BF16 else gelu64(pre).to(h)
        out["C"], out["C64"] = w, w.double()
        out["bound"] = torch.maximum(ulp_at(w.double(), h), 5e-7 * pre.double().abs()) + \
            (F16_HALF_SUB if h == F16 else 0.0)
        return out
    if c.res_dtype is not None:
        if res_rows is not None:
            r = res_rows
        elif c.res_mod:
            r = inp["res"][:, torch.arange(c.M) % c.res_mod]
        else:
            r = inp["res"]
        v = v + r.to(c.res_dtype).float()
    if f & F_ACCUM:
        v = v + inp["c_old"].to(c.c_dtype).float()
    if f & F_CLAMP16:
        v = v.to(F16).float().clamp(-CLAMP, CLAMP)
    out["C"] = v.to(c.c_dtype)
    if c.c_dtype != F32:
        out["inexact"] = out["C"].float() != v
        out["finite"] = bool(torch.isfinite(out["C"].float()).all())
    return out


def reference_int64(c, inp):
    """alpha * acc + bias from an int64 product, as fp64 (the exactness test's second opinion on the fp32 matmul)."""
    acc = torch.matmul(inp["A"].long(), inp["B"].transpose(1, 2).long())
    v = acc.double() * c.alpha
    return v + inp["bias"].to(c.dtype).double() if c.bias else v


def expected_buffers(c, inp, ref):
    """The whole C (and aux) buffer after the call: the initial buffer with the interior replaced."""
    C = inp["C_buf"].clone()
    view(C, c.batch, c.M, c.N, c.ldc, c.sC).copy_(ref["C"])
    aux = None
    if "aux" in ref:
        aux = inp["aux_buf"].clone()
        view(aux, c.batch, c.M, c.N, c.ldaux, c.sAux).copy_(ref["aux"])
    return C, aux


# ------------------------------------------------------------------------------------------------ comparators
def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _where(c, flat_index, ld, stride):
    """flat buffer index -> 'batch b, row m, column n' (or the pad / gap / guard it lies in)."""
    b, rem = (divmod(flat_index, stride) if c.batch > 1 else (0, flat_index))
    b = min(b, c.batch - 1)
    rem = flat_index - b * stride
    m, n = divmod(rem, ld)
    if m >= c.M:
        return f"past the last row of batch {b} (offset {rem - c.M * ld})"
    return f"batch {b}, row {m}, column {n}" + (" (pad column)" if n >= c.N else "")


def compare_exact(c, what, got, want, ld, stride):
    """Bit equality of two whole flat buffers -> None, or the report: how many interior elements differ and the first,
    whether any pad, gap or guard element changed and where."""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    diff = _bits(got) != _bits(want)
    if not bool(diff.any()):
        return None
    inside = interior(want.numel(), c.batch, c.M, c.N, ld, stride)
    din, dout = diff & inside, diff & ~inside
    msg = [f"{c.id} {what}:"]
    if bool(din.any()):
        i = int(din.nonzero()[0])
        msg.append(f"{int(din.sum())} of {int(inside.sum())} elements differ, first at {_where(c, i, ld, stride)}: "
                   f"got {float(got[i])!r}, want {float(want[i])!r}")
    if bool(dout.any()):
        i = int(dout.nonzero()[0])
        msg.append(f"{int(dout.sum())} pad / guard elements changed, first at {_where(c, i, ld, stride)} "
                   f"(flat {i} of {want.numel()}): got {float(got[i])!r}, was {float(want[i])!r}")
    return " ".join(msg)


def compare_bounded(c, what, got, init, want64, bound, ld, stride):
    """Interior within `bound` of want64 element by element, everything outside it bit-equal to the initial buffer
    -> (worst err / bound ratio, None or the report with the worst element)."""
    got = got.detach().cpu()
    inside = interior(init.numel(), c.batch, c.M, c.N, ld, stride)
    msg = []
    dout = (_bits(got) != _bits(init)) & ~inside
    if bool(dout.any()):
        i = int(dout.nonzero()[0])
        msg.append(f"{int(dout.sum())} pad / guard elements changed, first at {_where(c, i, ld, stride)}: got "
                   f"{float(got[i])!r}, was {float(init[i])!r}")
    g = view(got, c.batch, c.M, c.N, ld, stride).double()
    err = (g - want64).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    r = float(ratio.max())
    if not r <= 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        i = tuple(int(k) for k in i)
        msg.append(f"err/bound {r:.3f} ({int((ratio > 1).sum())} above 1), worst at batch {i[0]}, row {i[1]}, column "
                   f"{i[2]}: got {float(g[i])!r}, want {float(want64[i])!r}, bound {float(bound[i]):.3e}")
    return r, (f"{c.id} {what}: " + " ".join(msg)) if msg else None
