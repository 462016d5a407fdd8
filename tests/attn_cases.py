"""Cases, fp64 references and error bounds for the flash-attention kernels of csrc/attention.hip (torch on the
CPU only; tests/test_attn_cases_cpu.py proves the cases, tests/test_attn_parity_gpu.py runs them on the kernels).

Key probes.  Key j carries code(j): bit b of j as +-1 in columns 5b .. 5b+4 (11 bits x 5 repeats = 55 columns, the
other 9 zero).  A query aimed at key t is 32 * code(t): with scale 0.125 its score is 220 nats on key t and at least
40 nats less on every other key (one differing bit flips 5 columns: 2 * 5 * 32 * 0.125), so softmax is one-hot to
e^-40 = 4e-18.  A query with the columns of bit 0 zeroed ties keys a and a^1 exactly (200 nats each, 40 above the
rest): P = 1/2, 1/2.  V[j] holds the bits of j as 1 / 2 in columns 0..10, small non-zero integers of the pair j >> 1
elsewhere and the (batch, head) number in column 63; dO is small non-zero integers.  Nothing is zero, so the e^-40
tail (which bf16 still represents) is absorbed by an O(1) fp32 accumulator and outputs can be compared bit for bit;
a tied pair's V rows differ in column 0 only, which keeps dS = +-dO[q][0] / 4 and every gradient exact in 16 bits.

Random cases: randn at query amplitude 1 and 4, optionally with a per-key score offset that rises or falls with j
(query column 63 = 8, key column 63 = the offset in nats), so the running row max grows every tile or never.

Bounds (u = 2^-8 bf16, 2^-11 fp16), first order, per element:
  O    2u A + 2^-16 A,  A = sum_j P_qj |V_j|          (P rounded to 16 bits for the PV product, O rounded once)
  dV   2u C + 2^-16 C,  C = sum_q P_qj |dO_q|
  dS   E_qj = P_qj (u (|dp_qj| + |D_q|) + sum_e |dO_qe| 2u A_qe)   (dS rounded to 16 bits; D from the rounded O)
  dQ   scale sum_j E_qj |K_j| + u |dQ|,   dK   scale sum_q E_qj |Q_q| + u |dK|
  plus the underflow of the 16-bit P and dS, eta = half the smallest subnormal (2^-134 bf16, 2^-25 fp16) per unmasked
  (q, j): eta sum_j |V_j| on O, eta sum_q |dO_q| on dV, eta on E_qj; and eta on every output, rounded the same way.
  lse  max(4 x the error of the same computation in fp32 torch on the CPU, 2^-20 max(1, |lse|))."""
import functools
import math
from typing import NamedTuple

import torch

SCALE = 0.125
HD = 64
NBITS, REP = 11, 5
AMP = 32.0
GAP = 2 * REP * AMP * SCALE            # 40 nats between the targeted key and any other
GUARD = 64                             # guard rows after the last clip, guard columns right of every output
SENTINEL = -768.0                      # exact in bf16 and fp16; no output of any case equals it
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ETA = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}      # half the smallest subnormal number
DTYPES = (torch.bfloat16, torch.float16)
DT_NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}

NONCAUSAL = [(1, 1), (1, 64), (5, 70), (31, 63), (32, 64), (33, 65), (127, 128), (128, 129), (129, 192), (129, 193),
             (257, 321)]
CAUSAL = [(1, 1), (33, 33), (64, 64), (65, 65), (129, 129), (193, 193),
          (5, 70), (33, 97), (64, 128), (129, 200), (1, 193)]
# the full dtype x (B, H) product runs on these; every other shape at (2, 3) bf16 and (1, 1) fp16
FULL = {(33, 65, False), (129, 193, False), (129, 200, True)}
# (2, 4) beside the three asked for: with these shapes' 1 to 3 blocks per head, (1, 1), (2, 3) and (3, 5) give grids
# of 1 .. 45 workgroups of which none is a multiple of 8, the case where remap_bh() has no remainder
BH = [(1, 1), (2, 3), (3, 5), (2, 4)]
RANDOM_SHAPES = [(33, 65, False), (257, 321, False), (129, 200, True), (193, 193, True)]
RANDOM_VARIANTS = [("a1", 1.0, 0), ("a4", 4.0, 0), ("a4up", 4.0, 1), ("a4down", 4.0, -1)]
MAPS_NONCAUSAL = ("bij", "last", "first", "tie")
MAPS_CAUSAL = ("diag", "forbid", "first", "tie")
EXACT_MAPS = ("bij", "diag", "last", "first", "tie")


class Case(NamedTuple):
    kind: str          # "probe" | "rand"
    map: str           # probe: target map; rand: variant name
    B: int
    H: int
    Tq: int
    Tk: int
    causal: bool
    dtype: torch.dtype
    amp: float = AMP
    ramp: int = 0

    @property
    def id(self):
        return (f"{self.kind}-{self.map}-{self.Tq}x{self.Tk}{'c' if self.causal else ''}-b{self.B}h{self.H}-"
                f"{DT_NAME[self.dtype]}")

    @property
    def exact(self):
        return self.kind == "probe" and self.map in EXACT_MAPS


def _combos(Tq, Tk, causal):
    if (Tq, Tk, causal) in FULL:
        return [(B, H, dt) for dt in DTYPES for B, H in BH]
    return [(2, 3, torch.bfloat16), (1, 1, torch.float16)]


def map_fits(m, Tq, Tk, causal):
    if m == "tie":
        return Tk >= 2
    if m == "bij":
        return not causal and Tq <= Tk
    if m == "last":
        return not causal
    if m in ("diag", "forbid"):
        return causal
    return m == "first"


def _cases():
    probe, rand = [], []
    for causal, shapes, maps in ((False, NONCAUSAL, MAPS_NONCAUSAL), (True, CAUSAL, MAPS_CAUSAL)):
        for Tq, Tk in shapes:
            for m in maps:
                if map_fits(m, Tq, Tk, causal):
                    probe += [Case("probe", m, B, H, Tq, Tk, causal, dt) for B, H, dt in _combos(Tq, Tk, causal)]
    for Tq, Tk, causal in RANDOM_SHAPES:
        for nm, amp, ramp in RANDOM_VARIANTS:
            rand += [Case("rand", nm, B, H, Tq, Tk, causal, dt, amp, ramp) for B, H, dt in _combos(Tq, Tk, causal)]
    return probe, rand


PROBE_CASES, RANDOM_CASES = _cases()
ALL_CASES = PROBE_CASES + RANDOM_CASES
# the backward on inputs it did not produce itself: o and lse from the fp64 reference, rounded
INDEPENDENT_CASES = [Case("rand", "a4", 2, 3, 129, 200, True, dt, 4.0, 0) for dt in DTYPES]


def r16(x, dtype):
    """x rounded to the 16-bit dtype, as fp64."""
    return x.to(dtype).double()


# ----------------------------------------------------------------------------- probe inputs
def code(j):
    """[...] int64 key indices -> [..., 64] fp64 of +-1 (columns 55.. zero)."""
    bits = (j.unsqueeze(-1) >> torch.arange(NBITS)) & 1
    c = (2 * bits - 1).double().repeat_interleave(REP, -1)
    return torch.nn.functional.pad(c, (0, HD - NBITS * REP))


def _coprime(n):
    return next(s for s in (7, 5, 3, 11, 13, 1) if math.gcd(s, n) == 1)


def targets(m, Tq, Tk, causal, bh):
    """-> (ta, tb) [Tq] int64: the key (ta == tb) or the tied pair each query aims at."""
    q = torch.arange(Tq)
    off = Tk - Tq
    if m == "bij":
        ta = (q * _coprime(Tk) + 3 * bh + 1) % Tk
    elif m == "diag":
        ta = q + off
    elif m == "forbid":
        ta = torch.clamp(q + off + 1, max=Tk - 1)
    elif m == "last":
        ta = torch.full((Tq,), Tk - 1)
    elif m == "first":
        ta = torch.zeros(Tq, dtype=torch.int64)
    elif m == "tie":
        if causal:       # the last pair the mask allows in full; the query that sees key 0 only stays one-hot
            lim = q + off
            p = (lim + 1) // 2 - 1
            ta = torch.where(lim >= 1, 2 * p, torch.zeros_like(p))
            return ta, torch.where(lim >= 1, ta + 1, ta)
        npair = Tk // 2
        ta = 2 * ((q * _coprime(npair) + bh) % npair)
        return ta, ta + 1
    else:
        raise ValueError(m)
    return ta, ta.clone()


def probe_v(Tk, bh):
    j, c = torch.arange(Tk).unsqueeze(1), torch.arange(HD).unsqueeze(0)
    v = ((j >> 1) * (c + 3) + c) % 13 - 6
    v[v == 0] = 7
    v[:, :NBITS] = 1 + ((j >> torch.arange(NBITS)) & 1)
    v[:, HD - 1] = bh + 1
    return v.double()


def probe_do(Tq, bh, positive):
    q, c = torch.arange(Tq).unsqueeze(1), torch.arange(HD).unsqueeze(0)
    d = ((q + 5 * bh) * (c + 1) + 2 * c) % 7 - 3
    d[d == 0] = 4
    return (d.abs() if positive else d).double()


class Inputs:
    """q, do [B][H][Tq][64], k, v [B][H][Tk][64] in fp64 (exact in the case's dtype); probes: ta, tb [B][H][Tq]."""

    def __init__(self, case, q, k, v, do, ta=None, tb=None):
        self.case, self.q, self.k, self.v, self.do, self.ta, self.tb = case, q, k, v, do, ta, tb


@functools.lru_cache(maxsize=4)
def build(case):
    B, H, Tq, Tk = case.B, case.H, case.Tq, case.Tk
    if case.kind == "probe":
        qs, ks, vs, dos, tas, tbs = [], [], [], [], [], []
        for bh in range(B * H):
            ta, tb = targets(case.map, Tq, Tk, case.causal, bh)
            qc = code(ta)
            qc[ta != tb, :REP] = 0.0                       # bit 0 masked: ties ta and ta ^ 1
            qs.append(AMP * qc)
            ks.append(code(torch.arange(Tk)))
            vs.append(probe_v(Tk, bh))
            dos.append(probe_do(Tq, bh, positive=case.map not in ("bij", "diag", "forbid")))
            tas.append(ta)
            tbs.append(tb)
        st = lambda xs, T: torch.stack(xs).view(B, H, T, -1)
        return Inputs(case, st(qs, Tq), st(ks, Tk), st(vs, Tk), st(dos, Tq),
                      torch.stack(tas).view(B, H, Tq), torch.stack(tbs).view(B, H, Tq))
    g = torch.Generator().manual_seed(1000 * Tq + Tk + 17 * B + H)
    rn = lambda T: torch.randn(B, H, T, HD, generator=g, dtype=torch.float64)
    q, k, v, do = case.amp * rn(Tq), rn(Tk), rn(Tk), rn(Tq)
    if case.ramp:
        q[..., HD - 1] = 1.0 / SCALE
        k[..., HD - 1] = case.ramp * (6.0 * torch.arange(Tk, dtype=torch.float64) / max(Tk - 1, 1) - 3.0)
    return Inputs(case, *(r16(t, case.dtype) for t in (q, k, v, do)))


# ----------------------------------------------------------------------------- fp64 reference and bounds
def mask(Tq, Tk, causal):
    """[Tq][Tk] bool, True where key j is hidden from query q (j > q + Tk - Tq)."""
    if not causal:
        return torch.zeros(Tq, Tk, dtype=torch.bool)
    return torch.ones(Tq, Tk, dtype=torch.bool).triu(1 + Tk - Tq)


def scores(q, k, causal, scale=SCALE):
    s = (q @ k.transpose(-1, -2)) * scale
    return s.masked_fill(mask(q.shape[-2], k.shape[-2], causal), float("-inf"))


class Ref(NamedTuple):
    o: torch.Tensor
    lse: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor
    p: torch.Tensor
    lse_err32: float       # max |lse(fp32 torch) - lse(fp64)| of this case


@functools.lru_cache(maxsize=4)
def reference(case):
    """fp64 O, lse and (autograd) dQ, dK, dV on the case's 16-bit inputs."""
    inp = build(case)
    q, k, v = (t.clone().requires_grad_(True) for t in (inp.q, inp.k, inp.v))
    s = scores(q, k, case.causal)
    p = torch.softmax(s, -1)
    o = p @ v
    o.backward(inp.do)
    lse = torch.logsumexp(s.detach(), -1)
    lse32 = torch.logsumexp(scores(inp.q.float(), inp.k.float(), case.causal), -1)
    return Ref(o.detach(), lse, q.grad, k.grad, v.grad, p.detach(), float((lse32.double() - lse).abs().max()))


class Bounds(NamedTuple):
    o: torch.Tensor
    lse: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor


def bounds(case):
    inp, ref, u, eta = build(case), reference(case), U[case.dtype], ETA[case.dtype]
    p = ref.p
    seen = (~mask(case.Tq, case.Tk, case.causal)).double()          # a masked P or dS is an exact 0
    A = p @ inp.v.abs()
    C = p.transpose(-1, -2) @ inp.do.abs()
    dp = inp.do @ inp.v.transpose(-1, -2)
    D = (inp.do * ref.o).sum(-1, keepdim=True)
    E = p * (u * (dp.abs() + D.abs()) + (inp.do.abs() * 2 * u * A).sum(-1, keepdim=True)) + eta * seen
    # the eta terms: attention.hip pack8e<H>() rounds P (forward: relative to the running max, l >= 1 afterwards;
    # dK/dV kernel: the normalised P) and dS to 16 bits, where a value below the smallest normal number keeps an
    # absolute error of half the smallest subnormal instead of a relative one (fp16: every P below 6e-5)
    return Bounds(o=2 * u * A + 2.0 ** -16 * A + eta * (seen @ inp.v.abs()) + eta,
                  lse=torch.clamp(2.0 ** -20 * torch.clamp(ref.lse.abs(), min=1.0), min=4 * ref.lse_err32),
                  dq=SCALE * (E @ inp.k.abs()) + u * ref.dq.abs() + eta,
                  dk=SCALE * (E.transpose(-1, -2) @ inp.q.abs()) + u * ref.dk.abs() + eta,
                  dv=2 * u * C + 2.0 ** -16 * C + eta * (seen.transpose(-1, -2) @ inp.do.abs()) + eta)


class Exact(NamedTuple):
    o: torch.Tensor
    lse: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor
    p: torch.Tensor
    hit: torch.Tensor     # [B][H][Tk] bool: key j is some query's target


def exact(case):
    """What an exact probe must give, from the one-hot (or 1/2, 1/2) P itself: no exp, no e^-40 tail.  dV is rounded
    to the dtype where many queries share one key (its fp32 sum is exact, the stored value is its rounding)."""
    inp = build(case)
    assert case.exact
    p = torch.zeros(case.B, case.H, case.Tq, case.Tk, dtype=torch.float64)
    p.scatter_add_(-1, inp.ta.unsqueeze(-1), torch.full(inp.ta.shape + (1,), 0.5, dtype=torch.float64))
    p.scatter_add_(-1, inp.tb.unsqueeze(-1), torch.full(inp.tb.shape + (1,), 0.5, dtype=torch.float64))
    o = p @ inp.v
    ds = p * (inp.do @ inp.v.transpose(-1, -2) - (inp.do * o).sum(-1, keepdim=True))
    top = (inp.q * torch.gather(inp.k, 2, inp.ta.unsqueeze(-1).expand(-1, -1, -1, HD))).sum(-1) * SCALE
    lse = top + (inp.ta != inp.tb).double() * math.log(2.0)
    return Exact(o, lse, SCALE * ds @ inp.k, SCALE * ds.transpose(-1, -2) @ inp.q,
                 r16(p.transpose(-1, -2) @ inp.do, case.dtype), p, p.sum(-2) > 0)


def zero_bar(case):
    """|dQ|, |dK| where the exact value is 0: dp and D cancel only up to the fp32 summation order."""
    inp = build(case)
    return 2.0 ** -20 * float(inp.do.abs().max()) * float(inp.v.abs().max()) * 64


# ----------------------------------------------------------------------------- CPU rounding model of the kernels
def model(case, o_in=None, lse_in=None):
    """fp64 arithmetic with the kernels' 16-bit rounding points: the unnormalised P rounded for P V, O rounded; the
    backward on that O (or o_in / lse_in): P and dS rounded for their products, every output rounded."""
    inp, dt = build(case), case.dtype
    s = scores(inp.q, inp.k, case.causal)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    o = r16((r16(e, dt) @ inp.v) / l, dt)
    lse = (m + torch.log(l)).squeeze(-1)
    ob = o if o_in is None else o_in
    p = torch.exp(s - (lse if lse_in is None else lse_in).unsqueeze(-1))
    ds = r16(p * (inp.do @ inp.v.transpose(-1, -2) - (inp.do * ob).sum(-1, keepdim=True)), dt)
    return dict(o=o, lse=lse, dq=r16(SCALE * ds @ inp.k, dt), dk=r16(SCALE * ds.transpose(-1, -2) @ inp.q, dt),
                dv=r16(r16(p, dt).transpose(-1, -2) @ inp.do, dt))


# ----------------------------------------------------------------------------- device layout
class Layout:
    """The case in the fused buffers the model uses: Q in a [rows][3d] buffer, K | V in a [rows][2d] one, head h at
    column h*64, 64 guard rows after the last clip.  Unused columns and the guard rows of Q, V and dO are NaN; the
    guard rows of K hold 2 x the code (random cases: 8 x the sign) of the queries, so a key read past Tk would win
    its row and pull a NaN.  Outputs are sentinel-filled with 64 guard rows and 64 guard columns."""

    def __init__(self, inp, device="cpu", o=None, lse=None):
        c = inp.case
        B, H, Tq, Tk, dt = c.B, c.H, c.Tq, c.Tk, c.dtype
        d = H * HD
        self.case, self.d, self.ldq, self.ldkv, self.ldo, self.lddkv = c, d, 3 * d, 2 * d, d + GUARD, 2 * d + GUARD
        rows = lambda t, T: t.transpose(1, 2).reshape(B * T, d)
        nan = float("nan")
        qkv = torch.full((B * Tq + GUARD, 3 * d), nan, dtype=torch.float64)
        qkv[:B * Tq, :d] = rows(inp.q, Tq)
        kv = torch.full((B * Tk + GUARD, 2 * d), nan, dtype=torch.float64)
        kv[:B * Tk, :d] = rows(inp.k, Tk)
        kv[:B * Tk, d:] = rows(inp.v, Tk)
        lure = inp.q[-1].transpose(0, 1)[torch.arange(GUARD) % Tq].reshape(GUARD, d)    # [64][H*64]
        kv[B * Tk:, :d] = 2 * lure / AMP if c.kind == "probe" else 8 * torch.sign(lure)
        do = torch.full((B * Tq + GUARD, d), nan, dtype=torch.float64)
        do[:B * Tq] = rows(inp.do, Tq)
        dev = lambda t: t.to(dt).to(device)
        self.qkv, self.kv, self.do = dev(qkv), dev(kv), dev(do)
        sent = lambda r, cols: torch.full((r, cols), SENTINEL, dtype=dt, device=device)
        self.o, self.dq = sent(B * Tq + GUARD, self.ldo), sent(B * Tq + GUARD, self.ldo)
        self.dkv = sent(B * Tk + GUARD, self.lddkv)
        self.lse = torch.full((B * H * Tq + GUARD,), SENTINEL, dtype=torch.float32, device=device)
        if o is not None:       # the backward's o / lse given, not the forward's
            self.o[:B * Tq, :d] = dev(rows(o, Tq))
            self.lse[:B * H * Tq] = lse.reshape(-1).float().to(device)

    @property
    def q(self):
        return self.qkv
    @property
    def k(self):
        return self.kv
    @property
    def v(self):
        return self.kv[:, self.d:]
    @property
    def dk(self):
        return self.dkv
    @property
    def dv(self):
        return self.dkv[:, self.d:]

    def _split(self, buf, T):
        c = self.case
        return buf[:c.B * T].cpu().double().view(c.B, T, -1, HD).transpose(1, 2)

    def outputs(self):
        """-> o, lse, dq, dk, dv as fp64 [B][H][T][64] ([B][H][Tq] for lse) on the CPU."""
        c, d = self.case, self.d
        return dict(o=self._split(self.o[:, :d], c.Tq), dq=self._split(self.dq[:, :d], c.Tq),
                    dk=self._split(self.dkv[:, :d], c.Tk), dv=self._split(self.dkv[:, d:2 * d], c.Tk),
                    lse=self.lse[:c.B * c.H * c.Tq].cpu().double().view(c.B, c.H, c.Tq))

    def guards_intact(self, backward=True):
        """Names of the output buffers whose guard rows or columns no longer hold the sentinel."""
        c, d = self.case, self.d
        bad = []
        bufs = [("o", self.o, c.B * c.Tq, d)]
        if backward:
            bufs += [("dq", self.dq, c.B * c.Tq, d), ("dkv", self.dkv, c.B * c.Tk, 2 * d)]
        for nm, buf, r, cols in bufs:
            b = buf.cpu().float()
            if not (bool((b[r:] == SENTINEL).all()) and bool((b[:, cols:] == SENTINEL).all())):
                bad.append(nm)
        if not bool((self.lse[c.B * c.H * c.Tq:].cpu() == SENTINEL).all()):
            bad.append("lse")
        return bad
