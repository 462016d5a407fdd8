"""Cases, fp64 references and per-element error bounds for the training-side kernels of csrc/layernorm.hip,
csrc/klce.hip and csrc/misc.hip (torch / numpy on the CPU only; tests/test_train_cases_cpu.py proves the cases,
tests/test_train_kernels_parity_gpu.py runs them on the kernels).  Every reference starts from the rounded inputs
the kernel sees and is evaluated in fp64; every bound is first order in e = 2^-24 (fp32 unit roundoff), per element,
with constants counted from the kernels' operation sequences (below), never fitted to what a kernel returns.
u = unit roundoff of a 16-bit output (2^-8 bf16, 2^-11 fp16: half an ulp at the bottom of a binade, what one RNE
rounding can cost; 0 for fp32), eta = half the smallest fp16 subnormal
(2^-25) on fp16 outputs, else 0.

LayerNorm forward (two passes over registers).  A row sum is a per-lane chain plus a butterfly: D/64 terms + 6
levels on the wave-per-row kernels, D/32 terms + 5 levels on the half-wave kernels; K = D/32 + 6 bounds both.
  mean   sum (K e sum|x|), division by D (correctly rounded; 2 e allowed): E_mean = (K + 2) e mean|x|  (c1 = K + 2)
  var    d = x - mean (1), d*d (2 + 1), sum (K), / D (2), + eps (1): (K + 6) e relative.  The error of the mean
         cancels to first order (sum d = 0) and enters as E_mean^2 / (var + eps), kept as a second-order term.
  rstd   rsqrtf at 1 ulp = 2 e, half of var's: c_r = (K + 6) / 2 + 2, E_rstd / rstd = c_r e + (E_mean rstd)^2 / 2
  y      ((x - mean) rstd) w + b: subtraction 1, c_r, two products 2: c2 = c_r + 3; the final sum (or fma) 2 |y|
  E_y = e (c1 |w| rstd mean|x| + c2 |xhat w| + 2 |y|) + |xhat w| (E_mean rstd)^2 / 2 + u |y| + eta
Add-LayerNorm: x_out = round(x + r) is one IEEE fp32 add (then one RNE to bf16 on the bf16 stream): bit for bit;
y is bounded as above against the LayerNorm of that x_out.

LayerNorm backward (mean, rstd are fp32 inputs shared with the reference).  Row sums: D/64 terms + 6 levels,
Kb = D/64 + 6.  g = w dy (1), xhat = (x - mu) rs (2), s1 = mean g: (Kb + 3) e mean|g|, s2 = mean(g xhat):
(Kb + 6) e mean|g xhat|; g - s1 - xhat s2 and the product with rs add at most 6 roundings of terms bounded by the
three magnitudes, the accumulate onto dx one more: c3 = Kb + 13.
  E_dx = e c3 rstd (|g_i| + mean|g| + |xhat_i| mean|g xhat|) + e |dx_base|
  E_dw = e (L + 4) sum_r |dy xhat| + e |base|      E_db = e (L + 1) sum_r |dy| + e |base|
L = longest addition chain = rows per wave ceil(rows / (4 nblk)) + 4 waves + ceil(nblk / 16) partials per thread row
+ 16 thread rows, with the grid nblk = min(1024, ceil(rows / 4)) the host chooses.  At D = 1280 the grid may be cut
to the occupancy cap, anywhere between one block per CU and nblk: rows per wave takes the smallest grid, the partials
the largest (either alone is no upper bound).  + 3 for dy xhat (2 + 1), + 1 for the add onto the base.
g16 is the RNE rounding of the dx the same call wrote: bit for bit.

KL/CE.  __expf(a) is v_exp_f32 on a log2(e): 1 ulp plus the rounding of the scaled argument; the bound of an exp is
2^-23 (2 + |a|) relative, of __logf 2^-22 |log|.  A thread owns R = ceil(ceil(V / 8) / 256) chunks.  Element j of a
sum z = sum exp(a_j - m) travels through 1 + R rescales + 9 merges (6 shuffles, 3 across waves), whose arguments add
up to |a_j - m| (the running max only rises): 2^-23 (2 (R + 10) + |a_j - m|); the additions are 8 R + 9 long.  So
dz / z <= 2^-23 (c_z + W), c_z = 2 (R + 10) + (8 R + 9) / 2, W = sum_j softmax_j |a_j - m|, and
  E_lse = 2^-23 (c_z + W + 2 |log z| + |lse|)          (log, and the sum m + log z)
The argument of the gradient's exps, a_v - lse, carries E_lse, the rounding of 1/T and of a_v / T (2^-23 |a_v|) and
the subtraction; with 4 more roundings in gce (sm - 1) + gkl (q - p):
  c = c_z + 8 + max over the three softmaxes of (W + 2 |log z| + |lse| + max_v |a_v|)           (per row)
  E_g = u |g| + eta + 2^-23 [gce sm (c + |s - lse|) + gkl (q (c + |s/T - lse_s|) + p (c + |t/T - lse_t|))]
        + 4 e (gce 1[v = label] + |g|)      (the roundings of gce, sm - 1 and the fp32 sum where sm, q, p are tiny)
  E_ce = E_lse(s) + e |ce|
  E_kl = 2^-23 [(2 c_z + 6 + W_t) A + B] / T + E_lse(s/T) + E_lse(t/T) + 2^-23 (A / T + |lse_s| + |lse_t|),
         A = sum p |t - s|, B = sum p |t - s| |t - m_t| / T
  out3: sum_r E_row / N + 30 e sum_r |row| / N (fp64 partial sums, a 6-level butterfly, 16 waves, the division, T^2
  and the weights), on [ce, T^2 kl] and on their weighted sum.
Exactly 0: pad columns, ignored rows.  s == t: q and p are one expression, so dlogits equals the kl_w = 0 call's bits.

Helpers.  im2col3, col2im_s2 (at most two terms, a commutative fp32 add), the casts, mel_to_conv_input, count_valid
and an inactive clip_scale are exact.  embed_fwd: one fp32 add, one rounding.  l2norm: ceil(n / (256 nb)) terms per
thread + 6 + 3 + ceil(nb / 64) + 6 additions, + 1 for the square, halved by the root, + 2: relative e (L / 2 + 2).
colsum: 16 rows per wave + 3 + ceil(nchunk / 64) + 63 additions, against the unrounded fp64 sum s: e L sum|x| on the
fp32 sum, u (|s| + e L sum|x|) + eta for its one rounding to 16 bits, e (|base| + |out|) for the accumulate.
clip_scale (active): coef = max / (norm + 1e-6) as numpy fp32, x * coef one product: exact against numpy fp32.
AdamW (one step from a given fp32 state; lr, betas, eps, wd are the fp32 values the kernel receives).  powf at
2 ulp: bc = 1 - b^step has relative error rb = e (4 b^step / bc + 1).  gi = g inv coef: rg = 5.
  E_m = e ((1 - b1) (rg + 3) (|gi| + |m|) + |m'|)
  E_v = e (2 b2 |v| + (2 rg + 3) (1 - b2) gi^2 + |v'|)
  denom = sqrt(v') / sqrt(bc2) + eps: rd = E_v / (2 v') + e (rb2 / 2 + 4) relative (taken on the whole of denom)
  E_p = 3 e |p (1 - lr wd)| + |upd| (E_m / |m'| + rd + e (rb1 + 4)) + e |p'|,  upd = lr / bc1 m' / denom
The 16-bit copy is the RNE rounding of the kernel's own p: bit for bit.
gelu_bwd: out = r(r(g) gelu'(pre)) with the bar of test_gemm_gelu_exhaustive: 1 ulp of the output or 5e-7 |g|."""
import functools
import math
import zlib
from typing import NamedTuple, Optional

import numpy as np
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
HALF = (BF16, F16)
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16", None: "none"}
E32 = 2.0 ** -24
U = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
ETA = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -25}
EPS = 1e-5
CUS = 256                     # CUs of the MI355X: the worst case of the D = 1280 occupancy cap (one block per CU)
CAP_BLOCKS = 3 * CUS          # 162 VGPRs = 3 waves per SIMD = 3 blocks per CU (csrc/layernorm.hip)
SENTINEL = -768.0             # exact in bf16 and fp16
MAX_TENSOR_BYTES = 32 << 20


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ routes
def ln_fwd_route(D, x_dtype, y_dtype):
    assert D % 64 == 0 and D <= 1280
    if x_dtype == y_dtype and x_dtype in HALF and D % 256 == 0:
        return f"half<{D // 256}{',H' if x_dtype == F16 else ''}>"
    return "fwd<4,5>" if D % 256 == 0 else "fwd<1,20>"


def add_ln_route(D, x_dtype, r_dtype):
    assert D % 256 == 0 and D <= 1280
    if x_dtype == F32:
        return "fwd<4,5,ADD,RH>" if r_dtype == F16 else "fwd<4,5,ADD>"
    assert x_dtype == BF16 and r_dtype == BF16
    return f"half<{D // 256},ADD>"


class BwdRoute(NamedTuple):
    name: str
    grid_stride: bool        # some wave walks more than one row
    capped: bool             # the grid is cut to the occupancy cap (certain from 3 blocks per CU on a 256-CU part)
    nblk_min: int            # the smallest grid the host may choose
    nblk_max: int            # the largest


def ln_bwd_route(D, rows):
    assert D % 64 == 0 and D <= 1280
    nblk = min(1024, (rows + 3) // 4)
    v4 = D % 256 == 0
    name = f"bwd<4,{D // 256}>" if v4 else "bwd<1,20>"
    cap = v4 and D > 1024
    return BwdRoute(name, rows > 4 * nblk, cap and nblk > CAP_BLOCKS, min(nblk, CUS) if cap else nblk, nblk)


# ------------------------------------------------------------------------------------------------ LayerNorm forward
class LnFwd(NamedTuple):
    rows: int
    D: int
    x_dtype: torch.dtype
    y_dtype: torch.dtype
    variant: str = "randn"

    @property
    def id(self):
        return f"lnf-{self.variant}-{self.rows}x{self.D}-{DT_NAME[self.x_dtype]}-{DT_NAME[self.y_dtype]}"

    @property
    def route(self):
        return ln_fwd_route(self.D, self.x_dtype, self.y_dtype)


LN_D = (64, 192, 256, 512, 768, 1024, 1216, 1280)
LN_PAIRS = ((F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32))
LN_ROWS_FULL, LN_ROWS_TWO = (5, 9), (1, 3, 4, 7, 8, 333)
LN_VARIANTS = ("offset", "const", "outlier")


def _ln_fwd_cases():
    out = [LnFwd(r, D, a, b) for r in LN_ROWS_FULL for D in LN_D for a, b in LN_PAIRS]
    out += [LnFwd(r, D, a, b) for r in LN_ROWS_TWO for D in LN_D for a, b in ((F32, BF16), (BF16, BF16), (F16, F16))]
    out += [LnFwd(9, D, a, b, v) for v in LN_VARIANTS for D in (64, 256, 1280) for a, b in LN_PAIRS]
    return out


def ln_input(variant, rows, D, dtype, g):
    if variant == "randn":
        x = 3 * _randn(g, rows, D) + 1
    elif variant == "offset":
        x = (1000 + 0.01 * _randn(g, rows, D)) if dtype == F32 else (64 + _randn(g, rows, D))
    elif variant == "const":       # small multiples of 1/2: every partial sum is exact in fp32
        x = (torch.arange(rows, dtype=torch.float64)[:, None] % 7 - 3).expand(rows, D) * 0.5 + 0 * _randn(g, rows, D)
    else:
        x = _randn(g, rows, D)
        x[torch.arange(rows), torch.randint(0, D, (rows,), generator=g)] = 1e4
    return x.to(dtype)


def ln_params(D, g):
    return (1 + 0.5 * _randn(g, D)).float(), (0.3 * _randn(g, D)).float()


@functools.lru_cache(maxsize=None)
def ln_fwd_build(c: LnFwd):
    g = _gen(c.id)
    w, b = ln_params(c.D, g)
    return {"x": ln_input(c.variant, c.rows, c.D, c.x_dtype, g), "w": w, "b": b}


def ln_ref(x, w, b, eps=EPS):
    """fp64 LayerNorm of the given (already rounded) x -> dict(mean, rstd, xhat, y)."""
    x, w, b = x.double(), w.double(), b.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    xhat = (x - mean) * rstd
    return {"mean": mean[:, 0], "rstd": rstd[:, 0], "xhat": xhat, "y": xhat * w + b}


def ln_fwd_bounds(x, w, ref, y_dtype):
    D = x.shape[-1]
    K = D / 32 + 6
    c1, cr = K + 2, (K + 6) / 2 + 2
    c2 = cr + 3
    absx = x.double().abs().mean(-1)
    rstd = ref["rstd"]
    e_mean = E32 * c1 * absx
    second = 0.5 * (e_mean * rstd) ** 2
    xw = (ref["xhat"] * w.double()).abs()
    ey = (E32 * (c1 * w.double().abs() * (rstd * absx)[:, None] + c2 * xw + 2 * ref["y"].abs()) + xw * second[:, None]
          + U[y_dtype] * ref["y"].abs() + ETA[y_dtype])
    return {"y": ey, "mean": e_mean + E32 * ref["mean"].abs(), "rstd": rstd * (E32 * cr + second)}


class AddLn(NamedTuple):
    rows: int
    D: int
    x_dtype: torch.dtype
    r_dtype: torch.dtype
    inplace: bool

    @property
    def id(self):
        return f"addln-{self.rows}x{self.D}-{DT_NAME[self.x_dtype]}-{DT_NAME[self.r_dtype]}-{'in' if self.inplace else 'out'}"

    @property
    def route(self):
        return add_ln_route(self.D, self.x_dtype, self.r_dtype)


ADD_LN_D = (256, 512, 768, 1024, 1280)      # 512 beside the four asked for: half<2,ADD>
ADD_LN_FORMS = ((F32, BF16), (BF16, BF16), (F32, F16))


def _add_ln_cases():
    return [AddLn(r, D, a, b, ip) for r in (1, 9) for D in ADD_LN_D for a, b in ADD_LN_FORMS for ip in (False, True)]


@functools.lru_cache(maxsize=None)
def add_ln_build(c: AddLn):
    g = _gen(c.id)
    w, b = ln_params(c.D, g)
    x = (3 * _randn(g, c.rows, c.D) + 1).to(c.x_dtype)
    r = (2 * _randn(g, c.rows, c.D)).to(c.r_dtype)
    x_out = (x.float() + r.float()).to(c.x_dtype)          # one IEEE fp32 add, one rounding on the bf16 stream
    return {"x": x, "r": r, "w": w, "b": b, "x_out": x_out}


# ------------------------------------------------------------------------------------------------ LayerNorm backward
class LnBwd(NamedTuple):
    rows: int
    D: int
    x_dtype: torch.dtype
    dy_dtype: torch.dtype
    accum: bool
    g16: Optional[torch.dtype]
    params: bool = True          # False: dw = db = None

    @property
    def id(self):
        return (f"lnb-{self.rows}x{self.D}-{DT_NAME[self.x_dtype]}-{DT_NAME[self.dy_dtype]}-a{int(self.accum)}-"
                f"g{DT_NAME[self.g16]}{'' if self.params else '-noparams'}")

    @property
    def route(self):
        return ln_bwd_route(self.D, self.rows)


LNB_D = (64, 320, 1216, 256, 512, 768, 1024, 1280)
LNB_ROWS = (1, 5, 333, 4101)
LNB_COMBOS = [(a, g) for a in (False, True) for g in (None, BF16, F16)]


def _ln_bwd_cases():
    out, i = [], 0
    for D in LNB_D:
        for rows in LNB_ROWS:
            pairs = [(a, b) for a in (F32, BF16, F16) for b in (F32, BF16, F16)] if rows == 5 else [(F32, F32), (BF16, BF16)]
            for a, b in pairs:
                out.append(LnBwd(rows, D, a, b, *LNB_COMBOS[i % 6]))
                i += 1
        # every (dx_accum, g16) combination on every route at the smallest shape with more than one block
        out += [LnBwd(5, D, F32, BF16, a, g) for a, g in LNB_COMBOS if LnBwd(5, D, F32, BF16, a, g) not in out]
    out.append(LnBwd(333, 768, BF16, BF16, True, BF16, params=False))
    return out


@functools.lru_cache(maxsize=4)
def ln_bwd_build(c: LnBwd):
    g = _gen(c.id)
    w, _ = ln_params(c.D, g)
    x = (3 * _randn(g, c.rows, c.D) + 1).to(c.x_dtype)
    dy = (_randn(g, c.rows, c.D) * (0.5 + torch.rand(c.rows, 1, generator=g, dtype=torch.float64))).to(c.dy_dtype)
    st = ln_ref(x, w, torch.zeros(c.D))
    dx_base = _randn(g, c.rows, c.D).float()
    return {"x": x, "w": w, "dy": dy, "mean": st["mean"].float(), "rstd": st["rstd"].float(), "dx_base": dx_base,
            "dw_base": _randn(g, c.D).float(), "db_base": _randn(g, c.D).float()}


def ln_bwd_ref(inp, accum):
    x, w, dy = inp["x"].double(), inp["w"].double(), inp["dy"].double()
    mu, rs = inp["mean"].double()[:, None], inp["rstd"].double()[:, None]
    xhat, g = (x - mu) * rs, w * dy
    s1, s2 = g.mean(-1, keepdim=True), (g * xhat).mean(-1, keepdim=True)
    dx = rs * (g - s1 - xhat * s2)
    if accum:
        dx = dx + inp["dx_base"].double()
    return {"dx": dx, "dw": inp["dw_base"].double() + (dy * xhat).sum(0), "db": inp["db_base"].double() + dy.sum(0),
            "xhat": xhat, "g": g}


def ln_bwd_chain(rows, D):
    r = ln_bwd_route(D, rows)
    return -(-rows // (4 * r.nblk_min)) + 4 + -(-r.nblk_max // 16) + 16


def ln_bwd_bounds(inp, ref, accum):
    rows, D = inp["x"].shape
    c3 = D / 64 + 6 + 13
    g, xhat, rs = ref["g"], ref["xhat"], inp["rstd"].double()[:, None]
    e_dx = E32 * c3 * rs * (g.abs() + g.abs().mean(-1, keepdim=True) + xhat.abs() * (g * xhat).abs().mean(-1, keepdim=True))
    if accum:
        e_dx = e_dx + E32 * inp["dx_base"].double().abs()
    L, dy = ln_bwd_chain(rows, D), inp["dy"].double()
    return {"dx": e_dx, "dw": E32 * (L + 4) * (dy * xhat).abs().sum(0) + E32 * inp["dw_base"].double().abs(),
            "db": E32 * (L + 1) * dy.abs().sum(0) + E32 * inp["db_base"].double().abs()}


# ------------------------------------------------------------------------------------------------ KL/CE
class KlCe(NamedTuple):
    dtype: torch.dtype
    V: int
    ld: int
    rows: int
    T: float
    ce_w: float
    kl_w: float
    gs: float
    variant: str = "randn"
    labels: str = "mixed"        # "mixed" | "none" (every label -100)

    @property
    def id(self):
        return (f"klce-{self.variant}-{DT_NAME[self.dtype]}-V{self.V}-r{self.rows}-T{self.T:g}-w{self.ce_w:g}_{self.kl_w:g}"
                f"-gs{self.gs:g}{'-allignored' if self.labels == 'none' else ''}")


KLCE_VLD = ((8, 8), (13, 16), (2047, 2048), (2049, 2056), (4099, 4160))
KLCE_VARIANTS = ("randn", "peaked", "ramp_up", "ramp_down", "equal")
KLCE_DTYPES = (BF16, F16, F32)


def _klce_cases():
    out = [KlCe(dt, V, ld, 5, 2.0, 0.8, 1.0, 1.0, v) for dt in KLCE_DTYPES for V, ld in KLCE_VLD for v in KLCE_VARIANTS]
    # one axis at a time on a thread-without-chunk and a multi-chunk shape.  grad_scale 65536 runs in fp16 too: with
    # 4 or more valid rows |g| <= 65536 (1 + 2) / 4 stays below the fp16 maximum 65504 (it would overflow at rows = 1,
    # where the scale is not used)
    for V, ld in ((13, 16), (2049, 2056)):
        for dt in KLCE_DTYPES:
            base = dict(dtype=dt, V=V, ld=ld, rows=5, T=2.0, ce_w=0.8, kl_w=1.0, gs=1.0)
            for k, vals in (("rows", (1, 37)), ("T", (1.0, 3.0)), ("gs", (0.25, 65536.0))):
                out += [KlCe(**{**base, k: v}) for v in vals]
            out += [KlCe(**{**base, "ce_w": a, "kl_w": b}) for a, b in ((1.0, 0.0), (0.0, 1.0))]
            out.append(KlCe(**{**base, "T": 3.0, "gs": 0.25, "rows": 37, "variant": "ramp_up"}))
            out.append(KlCe(**{**base, "labels": "none"}))
    return out


def klce_labels(c: KlCe, g):
    V, rows = c.V, c.rows
    if c.labels == "none":
        return torch.full((rows,), -100, dtype=torch.int64)
    lab = torch.randint(0, V, (rows,), generator=g)
    special = [V // 2, -100, 0, V - 1, 8 * ((V - 1) // 8)]      # the last: first column of the ragged last chunk
    for i in range(rows):
        if i < 5 and rows >= 5:
            lab[i] = special[i]
        elif rows >= 5 and i % 6 == 1:
            lab[i] = -100
    if rows == 1:
        lab[0] = V - 1
    return lab


@functools.lru_cache(maxsize=None)
def klce_build(c: KlCe):
    g = _gen(c.id)
    V, rows = c.V, c.rows
    v = torch.arange(V, dtype=torch.float64)
    s, t = 3 * _randn(g, rows, V), 3 * _randn(g, rows, V)
    if c.variant == "peaked":
        s, t = s / 3, t / 3
        t[:, V // 3] += 60
        s[:, (V // 3 + 3) % V] += 30
    elif c.variant in ("ramp_up", "ramp_down"):
        ramp = (40 if c.variant == "ramp_up" else -40) * v / V
        s, t = s / 3 + ramp, t / 3 + ramp
    elif c.variant == "equal":
        t = s.clone()
    S = torch.full((rows + 1, c.ld), 7.0, dtype=torch.float64)      # pad columns hold a finite lure; + one guard row
    Tt = torch.full((rows + 1, c.ld), -5.0, dtype=torch.float64)
    S[:rows, :V], Tt[:rows, :V] = s, t
    return {"s": S.to(c.dtype), "t": Tt.to(c.dtype), "labels": klce_labels(c, g)}


def klce_ref(s, t, labels, V, T, ce_w, kl_w, gs, n_valid):
    """fp64 restatement of csrc/klce.hip's header: row losses [rows, 2], out3, dlogits [rows, V]."""
    rows = labels.numel()
    s, t = s[:rows, :V].double(), t[:rows, :V].double()
    valid = labels >= 0
    lab = labels.clamp(min=0)
    lse1, lses, lset = (torch.logsumexp(a, 1, keepdim=True) for a in (s, s / T, t / T))
    sm, q, p = torch.exp(s - lse1), torch.exp(s / T - lses), torch.exp(t / T - lset)
    ce = (lse1[:, 0] - s.gather(1, lab[:, None])[:, 0]) * valid
    kl = ((p * (t - s)).sum(1) / T - lset[:, 0] + lses[:, 0]) * valid
    N = max(int(n_valid), 1)
    onehot = torch.zeros_like(s).scatter_(1, lab[:, None], 1.0)
    gce, gkl = gs * ce_w / N, gs * kl_w * T / N
    grad = (gce * (sm - onehot) + gkl * (q - p)) * valid[:, None]
    ce_m, kl_m = ce.sum() / N, kl.sum() / N * T * T
    return {"row": torch.stack([ce, kl], 1), "out3": torch.stack([ce_w * ce_m + kl_w * kl_m, ce_m, kl_m]), "grad": grad,
            "parts": dict(s=s, t=t, sm=sm, q=q, p=p, lse1=lse1, lses=lses, lset=lset, gce=gce, gkl=gkl, valid=valid, N=N, onehot=onehot)}


def klce_bounds(ref, V, T, ce_w, kl_w, dtype):
    P = ref["parts"]
    R = -(-((V + 7) // 8) // 256)
    cz = 2 * (R + 10) + (8 * R + 9) / 2
    e23 = 2.0 ** -23

    def lse_terms(a, lse, soft):
        m = a.max(1, keepdim=True).values
        W = (soft * (a - m).abs()).sum(1, keepdim=True)
        logz = (lse - m).abs()
        return W, e23 * (cz + W + 2 * logz + lse.abs()), W + 2 * logz + lse.abs() + a.abs().max(1, keepdim=True).values

    s, t = P["s"], P["t"]
    W1, el1, h1 = lse_terms(s, P["lse1"], P["sm"])
    Ws, els, hs = lse_terms(s / T, P["lses"], P["q"])
    Wt, elt, ht = lse_terms(t / T, P["lset"], P["p"])
    c = cz + 8 + torch.maximum(torch.maximum(h1, hs), ht)
    g = ref["grad"]
    eg = (U[dtype] * g.abs() + ETA[dtype] + 4 * E32 * (abs(P["gce"]) * P["onehot"] + g.abs())
          + e23 * (abs(P["gce"]) * P["sm"] * (c + (s - P["lse1"]).abs())
          + abs(P["gkl"]) * (P["q"] * (c + (s / T - P["lses"]).abs()) + P["p"] * (c + (t / T - P["lset"]).abs()))))
    eg = eg * P["valid"][:, None]
    ce, kl = ref["row"][:, 0], ref["row"][:, 1]
    e_ce = (el1[:, 0] + E32 * ce.abs()) * P["valid"]
    mt = (t / T).max(1, keepdim=True).values
    A = (P["p"] * (t - s).abs()).sum(1)
    B = (P["p"] * (t - s).abs() * (t / T - mt).abs()).sum(1)
    e_kl = (e23 * ((2 * cz + 6 + Wt[:, 0]) * A + B) / T + els[:, 0] + elt[:, 0]
            + e23 * (A / T + P["lses"][:, 0].abs() + P["lset"][:, 0].abs())) * P["valid"]
    N = P["N"]
    o_ce = e_ce.sum() / N + 30 * E32 * ce.abs().sum() / N
    o_kl = (e_kl.sum() / N + 30 * E32 * kl.abs().sum() / N) * T * T
    tiny = 2.0 ** -126
    return {"grad": eg, "row": torch.stack([e_ce, e_kl], 1) + tiny,
            "out3": torch.stack([abs(ce_w) * o_ce + abs(kl_w) * o_kl + E32 * ref["out3"][0].abs(), o_ce, o_kl]) + tiny}


# ------------------------------------------------------------------------------------------------ helpers
class Im2col(NamedTuple):
    dtype: torch.dtype
    stride: int
    B: int
    C: int
    T_out: int

    @property
    def id(self):
        return f"im2col-{DT_NAME[self.dtype]}-s{self.stride}-b{self.B}-c{self.C}-t{self.T_out}"


def _im2col_cases():
    return [Im2col(dt, st, B, C, T) for dt in (BF16, F16, F32) for st in (1, 2) for B in (1, 3)
            for C in (64, 80, 128, 384) for T in (1, 7, 20)]


def im2col_t_in(c):
    return c.T_out if c.stride == 1 else 2 * c.T_out


def im2col_build(c: Im2col):
    rows = im2col_t_in(c) + 2
    return _randn(_gen(c.id), c.B, rows, c.C).to(c.dtype)


def im2col_ref(src, T_out, stride):
    """dst[b*T_out + t][k*C + c] = src[b][t*stride + k][c] by torch.unfold."""
    B, _, C = src.shape
    u = src.unfold(1, 3, stride)[:, :T_out]                 # [B, T_out, C, 3]
    return u.permute(0, 1, 3, 2).reshape(B * T_out, 3 * C)


def im2col_ref_loops(src, T_out, stride):
    B, _, C = src.shape
    out = torch.empty(B * T_out, 3 * C, dtype=src.dtype)
    for b in range(B):
        for t in range(T_out):
            for k in range(3):
                out[b * T_out + t, k * C:(k + 1) * C] = src[b, t * stride + k]
    return out


class Col2im(NamedTuple):
    B: int
    C: int
    T_in: int

    @property
    def id(self):
        return f"col2im-b{self.B}-c{self.C}-t{self.T_in}"

    @property
    def T_out(self):
        return (self.T_in - 1) // 2 + 1


COL2IM_CASES = [Col2im(B, C, T) for B in (1, 3) for C in (64, 384) for T in (1, 2, 20, 21)]


def col2im_build(c: Col2im):
    return _randn(_gen(c.id), c.B * c.T_out, 3 * c.C).float()


def col2im_ref(dA, B, T_in, T_out, C, guard=True):
    """The adjoint of im2col3 (k3, s2, p1) on the unpadded rows, fp32 adds: dX[b][s] = sum over 2t + k - 1 = s."""
    dA = dA.reshape(B, T_out, 3, C)
    dX = torch.zeros(B, T_in, C, dtype=dA.dtype)
    for t in range(T_out):
        for k in range(3):
            s = 2 * t + k - 1
            if 0 <= s < T_in:
                dX[:, s] += dA[:, t, k]
    if not guard:       # the mutant: odd rows lose their t0 = (s + 1) / 2 term
        for s in range(1, T_in, 2):
            if (s + 1) // 2 < T_out:
                dX[:, s] -= dA[:, (s + 1) // 2, 0]
    return dX.reshape(B * T_in, C)


CAST_LOWS = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
CAST_LENGTHS = (1, 3, 4, 5, 393216, 4 * 2 ** 20 + 7)


@functools.lru_cache(maxsize=1)
def cast_patterns():
    """Every 16-bit high half x 6 low halves as fp32 (393 216 values): ties to even of both parities, carries into the
    exponent, overflow to inf, both subnormal ranges, NaN."""
    hi = np.arange(65536, dtype=np.uint32) << 16
    bits = (hi[:, None] | np.array(CAST_LOWS, dtype=np.uint32)[None, :]).reshape(-1)
    return torch.from_numpy(bits.view(np.float32).copy())


def cast_input(n):
    p = cast_patterns()
    return p[:n].clone() if n <= p.numel() else p.repeat(-(-n // p.numel()))[:n].clone()


def cast_ref(x, dtype):
    return x.to(dtype)


def cast_ref_bits(x, dtype, truncate=False):
    """Second formulation, integer arithmetic on the bits (bf16 only); truncate: the mutant."""
    assert dtype == BF16
    b = x.numpy().view(np.uint32).astype(np.uint64)
    r = b if truncate else b + 0x7FFF + ((b >> 16) & 1)
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    out = np.where(nan, (b >> 16) | 0x40, r >> 16).astype(np.uint16)
    return torch.from_numpy(out.view(np.int16).copy()).view(BF16)


def same_bits_or_nan(got, want):
    """16-bit tensors equal bit for bit where want is not NaN, NaN where it is."""
    nan = torch.isnan(want.float())
    ok = (got.view(torch.int16) == want.view(torch.int16)) | nan
    return bool(ok.all()) and bool(torch.isnan(got.float())[nan].all())


def gelu_grad64(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


GELU_G = (1.0, -3.0, 0.37)


def gelu_patterns(dtype):
    """Every finite 16-bit pattern of the dtype (fp32: the bf16 patterns as fp32)."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    p = bits.view(BF16 if dtype == F32 else dtype)
    p = p[torch.isfinite(p.float())]
    return p.float() if dtype == F32 else p


def gelu_matrix(v, cols=256):
    """A flat table as [M, cols] with M a multiple of cols (zero padded): the operand shape of the DGELU GEMM."""
    rows = -(-v.numel() // (cols * cols)) * cols
    out = torch.zeros(rows * cols, dtype=v.dtype)
    out[:v.numel()] = v
    return out.view(rows, cols)


def gelu_bwd_ref(g, pre, dtype):
    """-> (want fp64, bar): r(r(g) gelu'(pre)) and max(1 ulp of the output, 5e-7 |g|)."""
    gv = g.to(dtype).double()
    exact = gv * gelu_grad64(pre)
    want = exact.to(dtype).double()
    ulp = {F32: 2.0 ** -23, BF16: 2.0 ** -7, F16: 2.0 ** -10}[dtype]
    return want, torch.maximum(want.abs() * ulp, 5e-7 * gv.abs())


CLIP_N = (10007, 8192 * 256 + 5)
L2_N = (1, 255, 10007, 300001)


def clip_ref(x, norm, max_norm):
    coef = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return x.clone() if coef >= 1 else torch.from_numpy(x.numpy() * np.float32(coef))


def l2norm_rel_bound(n):
    nb = max(1, min(1024, -(-n // 256)))
    L = -(-n // (256 * nb)) + 6 + 3 + -(-nb // 64) + 6 + 1
    return E32 * (L / 2 + 2)


class Adam(NamedTuple):
    n: int
    wd: float
    clip: str            # "none" | "inactive" | "active"
    step: int            # first step of the run
    steps: int           # consecutive steps
    p16: Optional[torch.dtype] = BF16

    @property
    def id(self):
        return f"adamw-n{self.n}-wd{self.wd:g}-{self.clip}-step{self.step}x{self.steps}-{DT_NAME[self.p16]}"


ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_MAX_NORM = 1.0


def _adam_cases():
    out = [Adam(10007, wd, clip, 1, 5, p16) for wd in (0.0, 0.01) for clip, p16 in
           (("none", BF16), ("inactive", F16), ("active", BF16))]
    out += [Adam(10007, wd, clip, 1000, 1, None) for wd in (0.0, 0.01) for clip in ("none", "active")]
    out += [Adam(8192 * 256 + 3, 0.01, "active", 1, 1, F16), Adam(8192 * 256 + 3, 0.0, "none", 1000, 1, BF16)]
    return out


def adam_build(c: Adam):
    g = _gen(c.id)
    n = c.n
    p = _randn(g, n).float()
    if c.step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = (0.1 * _randn(g, n)).float(), (0.01 * _randn(g, n) ** 2).float()
    scale = {"none": 1.0, "inactive": 0.5 / math.sqrt(n), "active": 1.0}[c.clip]
    grads = [(scale * _randn(g, n) * (1 + 0.1 * k)).float() for k in range(c.steps)]
    return {"p": p, "m": m, "v": v, "grads": grads}


def adam_norm(c: Adam, g):
    """fp32 norm handed to the kernel (None without clipping): the fp64 norm rounded once."""
    return None if c.clip == "none" else g.double().norm().float().reshape(1)


def adam_ref(p, g, m, v, step, wd, norm, *, lr, b1, b2, eps, max_norm=ADAM_MAX_NORM, inv_scale=1.0, sqrt_bc2=True):
    """One AdamW step in fp64 from fp32 state; hyper-parameters are the fp32 values the kernel receives.
    -> (p', m', v', bounds dict)."""
    f = lambda a: float(np.float32(a))
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    coef = 1.0
    if norm is not None and max_norm > 0:
        coef = min(1.0, f(max_norm) / (float(norm) * inv_scale + f(1e-6)))
    gi = g * inv_scale * coef
    p1 = p * (1 - lr * wd)
    m2 = m + (1 - b1) * (gi - m)
    v2 = v * b2 + (1 - b2) * gi * gi
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v2.sqrt() / (math.sqrt(bc2) if sqrt_bc2 else bc2) + eps
    upd = lr / bc1 * (m2 / denom)
    p2 = p1 - upd
    rg, rb1, rb2 = 5, 4 * b1 ** step / bc1 + 1, 4 * b2 ** step / bc2 + 1
    e_m = E32 * ((1 - b1) * (rg + 3) * (gi.abs() + m.abs()) + m2.abs())
    e_v = E32 * (2 * b2 * v.abs() + (2 * rg + 3) * (1 - b2) * gi * gi + v2.abs())
    tiny = 1e-300
    rd = e_v / (2 * v2 + tiny) + E32 * (rb2 / 2 + 4)
    e_p = 3 * E32 * p1.abs() + upd.abs() * (e_m / (m2.abs() + tiny) + rd + E32 * (rb1 + 4)) + E32 * p2.abs()
    return p2, m2, v2, {"p": e_p + 2.0 ** -140, "m": e_m + 2.0 ** -140, "v": e_v + 2.0 ** -140}


class Colsum(NamedTuple):
    rows: int
    cols: int
    dtype: torch.dtype
    accum: bool
    rounding: int
    offset: int          # column offset into a wider matrix (ldx = cols + 24 when > 0, a multiple of 8), else ldx = cols

    @property
    def id(self):
        return (f"colsum-{self.rows}x{self.cols}-{DT_NAME[self.dtype]}-a{int(self.accum)}-r{self.rounding}-"
                f"o{self.offset}")

    @property
    def ldx(self):
        return self.cols + 24 if self.offset else self.cols


def _colsum_cases():
    out, i = [], 0
    combos = [(a, r) for a in (False, True) for r in (0, 1, 2)]
    for rows in (1, 63, 64, 65, 4097):
        for cols in (8, 70, 512, 520):
            for dt in (BF16, F16, F32):
                a, r = combos[i % 6]
                out.append(Colsum(rows, cols, dt, a, r, 8 * (i % 3)))
                i += 1
    return out


def colsum_build(c: Colsum):
    g = _gen(c.id)
    return {"x": (_randn(g, c.rows, c.ldx) + 0.25).to(c.dtype), "base": _randn(g, c.cols).float()}


def colsum_ref(c: Colsum, inp):
    x = inp["x"][:, c.offset:c.offset + c.cols].double()
    s = x.sum(0)
    rdt = {0: F32, 1: BF16, 2: F16}[c.rounding]
    nchunk = -(-c.rows // 64)
    L = 16 + 3 + -(-nchunk // 64) + 63
    want, e_sum = s, E32 * L * x.abs().sum(0)
    bound = e_sum + U[rdt] * (s.abs() + e_sum) + ETA[rdt]
    if c.accum:
        want = want + inp["base"].double()
        bound = bound + E32 * (inp["base"].double().abs() + want.abs())
    return want, bound


COUNT_N = (1, 28608, 262149)


def count_labels(n, kind, g):
    if kind == "all":
        return torch.randint(0, 50000, (n,), generator=g)
    if kind == "none":
        return torch.full((n,), -100, dtype=torch.int64)
    lab = torch.randint(0, 50000, (n,), generator=g)
    lab[torch.rand(n, generator=g) < 0.3] = -100
    return lab


def mel_ref(mel, dtype):
    """mel [B, nmel, T] fp32 -> [B, T + 2, nmel] of dtype with zero rows 0 and T + 1."""
    B, nmel, T = mel.shape
    out = torch.zeros(B, T + 2, nmel, dtype=dtype)
    out[:, 1:T + 1] = mel.transpose(1, 2).to(dtype)
    return out


EMBED_CASES = [(tok, out) for tok in (F32, BF16, F16) for out in (F32, BF16 if tok != F16 else F16)]


def embed_build(tok_dtype, g, vocab=50, D=384, B=2, T=7, max_pos=16):
    return {"ids": torch.randint(0, vocab, (B, T), generator=g), "tok": _randn(g, vocab, D).to(tok_dtype),
            "pos": _randn(g, max_pos, D).to(tok_dtype), "T": T, "pos_offset": 3}


def embed_ref(inp, out_dtype):
    B, T = inp["ids"].shape
    pos = inp["pos"][inp["pos_offset"]:inp["pos_offset"] + T]
    s = inp["tok"].float()[inp["ids"]] + pos.float()[None]          # one IEEE fp32 add
    return s.to(out_dtype).reshape(B * T, -1)


LN_FWD_CASES = _ln_fwd_cases()
ADD_LN_CASES = _add_ln_cases()
LN_BWD_CASES = _ln_bwd_cases()
KLCE_CASES = _klce_cases()
IM2COL_CASES = _im2col_cases()
ADAM_CASES = _adam_cases()
COLSUM_CASES = _colsum_cases()


def largest_tensor_bytes():
    """The largest single tensor any case hands to a kernel (fp32 at the widest)."""
    sz = [c.rows * c.D * 4 for c in LN_FWD_CASES + ADD_LN_CASES + LN_BWD_CASES]
    sz += [(c.rows + 1) * c.ld * 4 for c in KLCE_CASES]
    sz += [max(CAST_LENGTHS) * 4, max(CLIP_N) * 4, max(L2_N) * 4, max(COUNT_N) * 8]
    sz += [c.n * 4 for c in ADAM_CASES] + [c.rows * c.ldx * 4 for c in COLSUM_CASES]
    sz += [c.B * (im2col_t_in(c) + 2) * c.C * 4 * 3 for c in IM2COL_CASES]
    return max(sz)
