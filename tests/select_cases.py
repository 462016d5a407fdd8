"""Planted inputs and the plain reference of the token selection kernels (csrc/decode.hip: tw_greedy_select,
tw_select_sample, tw_greedy_select_ts, tw_select_sample_ts, tw_token_logprob), shared by test_select_cases_cpu.py
(which proves the cases can see the bugs they are meant for) and test_select_kernels_gpu.py (which runs the kernels).

Reference: plain torch on the CPU in fp64 over the logits after rounding to the dtype under test, so kernel and
reference see the same input bits and ids are compared exactly.  Per row: -inf at suppressed ids (and at the
begin-suppressed ids when the begin mask applies), oracle.greedy_ref.timestamp_rules for the _ts kernels, the lowest
index among the entries equal to the maximum, id 0 when nothing is finite; log-prob = fp64 log_softmax of the
processed row at the pick.

A Group is one call configuration (column, begin_col, max_initial, begin mask on / off); its rows are the distinct
planted rows, tiled to whatever batch size the test runs.
"""
from dataclasses import dataclass, field

import torch

from oracle.greedy_ref import timestamp_rules

NEG = float("-inf")
LOGP_ATOL = 1e-4            # the selector's log-prob bar (test_fallback_gpu.py), logits |x| <~ 10
MASS_MARGIN = 1e-3          # |logsumexp(eligible timestamps) - max(eligible text)| of every case but (d)
BATCHES = (1, 17, 100, 256, 257)
SLICES = (32, 16, 4, 2, 1)  # what sel_slices gives at BATCHES
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
LAYOUTS = ("vec", "ld_eq_v", "ld_odd", "offset1")
SLP0 = -1.5                 # sum_logp before the call: the kernels accumulate


@dataclass(frozen=True)
class Vocab:
    name: str
    V: int
    ld: int
    eos: int
    no_ts: int
    ts_begin: int
    sup: tuple              # suppressed ids: the first and the last mask word among them
    beg: tuple              # begin-suppressed ids
    mid: int                # a timestamp in the middle of the range

    @property
    def ceil8(self):
        return (self.V + 7) // 8 * 8


REAL = Vocab("real", 51865, 51904, 50257, 50363, 50364, (3, 100, 5000, 51865 - 4), (220, 50257), 50364 + 700)
SMALL = Vocab("small", 1003, 1008, 600, 630, 631, (3, 100, 500, 1003 - 4), (22, 600), 631 + 180)
VOCABS = {"real": REAL, "small": SMALL}

TEXT_BEST, TEXT_FORBID, TEXT_GEN = 77, 50, 40       # planted text ids (none suppressed)


def slices(B, V):
    """(G, slice width) of a batch of B rows: the loop of sel_slices / launch_select in csrc/decode.hip."""
    G = 1
    while G < 32 and B * G * 2 <= 512:
        G *= 2
    width = ((V + G - 1) // G + 7) // 8 * 8
    return (V + width - 1) // width, width


@dataclass
class Row:
    name: str
    x: torch.Tensor                     # fp32 [V], before rounding to the dtype under test
    gen: list = field(default_factory=list)
    done: int = 0
    kind: str = ""                      # "mass_a" / "mass_b" / "mass_d" / "forbid:<rule>" / ...
    state: str = ""
    prompt: tuple = ()


@dataclass
class Group:
    name: str
    voc: Vocab
    ts: bool
    begin_col: int
    col: int
    max_initial: int                    # -1: none
    begin_on: bool                      # greedy: apply_begin; ts: a begin mask is passed (it applies at the first step)
    rows: list

    @property
    def first(self):
        return self.col == self.begin_col

    def width(self):
        return self.col + 3


def row_last_ts(voc, row):
    st = [t for t in row.gen if t >= voc.ts_begin]
    return st[-1] if st else -1


def row_ids(g, row):
    """The id matrix row before the call: prompt, generated prefix, zeros."""
    ids = torch.zeros(g.width(), dtype=torch.int64)
    pre = list(row.prompt) + list(row.gen)
    assert len(pre) == g.col and len(row.prompt) == g.begin_col
    ids[:g.col] = torch.tensor(pre, dtype=torch.int64) if pre else ids[:0]
    return ids


# ------------------------------------------------------------------------------------------------ reference

def rounded(x, dtype):
    return x.to(dtype).double()


def processed_row(g, row, dtype, apply_mass=True, rules=timestamp_rules):
    """fp64 row after the suppress masks and (ts groups) the timestamp rules."""
    voc = g.voc
    r = rounded(row.x, dtype)
    r[list(voc.sup)] = NEG
    if g.ts:
        if g.first and g.begin_on:
            r[list(voc.beg)] = NEG
        r = rules(r, list(row.gen), g.first, voc.ts_begin, voc.no_ts, voc.eos,
                  g.max_initial if g.max_initial >= 0 else None, apply_mass)
    elif g.begin_on:
        r[list(voc.beg)] = NEG
    return r


def lowest_argmax(r):
    """Lowest index among the finite entries equal to the maximum; 0 when nothing is finite."""
    fin = torch.isfinite(r)
    if not bool(fin.any()):
        return 0
    m = r[fin].max()
    return int(torch.nonzero(r == m)[0])


def reference(g, row, dtype, pick=None):
    """Outputs of one call on one row: dict(tok, done, last_ts, logp, any_finite).  pick: the drawn id of a sampled
    row (its log-prob is read off the same processed row)."""
    voc = g.voc
    r = processed_row(g, row, dtype)
    best = lowest_argmax(r) if pick is None else pick
    any_finite = bool(torch.isfinite(r).any())
    lt = row_last_ts(voc, row)
    if row.done:
        return dict(tok=voc.eos, done=1, last_ts=lt, logp=None, any_finite=any_finite, row=r)
    logp = float(torch.log_softmax(r, -1)[best]) if any_finite else None
    if g.ts and best >= voc.ts_begin:
        lt = best
    return dict(tok=best, done=int(best == voc.eos), last_ts=lt, logp=logp, any_finite=any_finite, row=r)


def mass_margin(g, row, dtype):
    """|logsumexp(eligible timestamps) - max(eligible text)| in fp64 (inf when either side is empty)."""
    r = processed_row(g, row, dtype, apply_mass=False)
    ts, tx = r[g.voc.ts_begin:], r[:g.voc.ts_begin]
    if not bool(torch.isfinite(ts).any()) or not bool(torch.isfinite(tx).any()):
        return float("inf")
    return abs(float(torch.logsumexp(ts, -1)) - float(tx.max()))


# ------------------------------------------------------------------------------------------------ rows

def _base(voc, gen_, ts_shift=0.0):
    x = (torch.randn(voc.V, generator=gen_) * 3.0).clamp_(-9.5, 9.5)
    if ts_shift:
        x[voc.ts_begin:] = (torch.randn(voc.V - voc.ts_begin, generator=gen_) * 1.5 + ts_shift).clamp_(-10.0, 0.0)
    return x


def greedy_groups(voc, seed=11):
    """Planted rows of greedy_select / select_sample, once with the begin mask applied and once without."""
    gen_ = torch.Generator().manual_seed(seed)
    V = voc.V
    rows = []

    def add(name, plant, done=0, base=None):
        x = _base(voc, gen_) if base is None else base
        for i, v in plant:
            if 0 <= i < V:
                x[i] = v
        rows.append(Row(name, x, done=done, kind=name))

    add("random", [])
    add("win_first", [(0, 12.0)])
    add("win_last", [(V - 1, 12.0)])                    # the scalar tail chunk (V % 8 != 0)
    for B in BATCHES:
        G, w = slices(B, V)
        if G == 1:
            continue
        for k in sorted({1, G // 2, G - 1} - {0}):
            add(f"win_slice_end_G{G}_k{k}", [(k * w - 1, 12.0)])
            add(f"win_slice_start_G{G}_k{k}", [(k * w, 12.0)])
            add(f"tie_across_slice_G{G}_k{k}", [(k * w - 1, 12.0), (k * w, 12.0)])
    # a workgroup's scan strides 2048 ids a pass from its slice's first id.  Only slices wider than 2048 have a
    # second pass: the real vocabulary at G <= 16 (the small one, 1003 ids, never has one).  Ids 2047 / 2048 are the
    # pass boundary wherever the scan starts at id 0 (G = 1, and slice 0 of G = 2, 4, 16); the *_G<g>_k1 rows put the
    # same boundary into slice 1 of G = 2, 4 and 16, where it is counted from the slice's own first id.
    if V > 2048:
        add("win_pass_end", [(2047, 12.0)])             # thread 255's last id of the first pass
        add("win_pass_start", [(2048, 12.0)])           # thread 0's first id of the second
        add("tie_across_pass", [(2047, 12.0), (2048, 12.0)])
        add("tie_same_thread_two_passes", [(2048 + 13, 12.0), (13, 12.0)])
        for B in BATCHES:
            G, w = slices(B, V)
            if G == 1 or w <= 2048:
                continue
            add(f"win_pass_end_G{G}_k1", [(w + 2047, 12.0)])
            add(f"win_pass_start_G{G}_k1", [(w + 2048, 12.0)])
            add(f"tie_across_pass_G{G}_k1", [(w + 2047, 12.0), (w + 2048, 12.0)])
    add("tie_same_chunk", [(16, 12.0), (21, 12.0)])
    add("tie_lanes", [(8 * 5 + 1, 12.0), (8 * 9, 12.0)])
    add("tie_waves", [(8 * 10 + 2, 12.0), (8 * (64 + 3), 12.0)])
    add("tie_slices", [(45, 12.0), (V - 45, 12.0)])
    add("tie_three", [(V - 1, 12.0), (V // 2, 12.0), (V // 3, 12.0)])
    add("sup_winner", [(voc.sup[1], 13.0), (300, 12.0)])
    add("sup_first_word", [(voc.sup[0], 13.0)])
    add("sup_last_word", [(voc.sup[3], 13.0)])
    add("beg_winner", [(voc.beg[0], 13.0), (301, 12.0)])
    add("eos_winner", [(voc.eos, 13.0), (302, 12.0)])   # begin mask off: picks eos and sets done
    add("done_row", [(5, 12.0)], done=1)
    add("done_row_eos_best", [(voc.eos, 12.0)], done=1)
    x = _base(voc, gen_)
    x[torch.rand(V, generator=gen_) < 0.3] = NEG
    add("some_neg_inf", [(V - 7, 11.0)], base=x)
    x = torch.full((V,), NEG)
    add("one_finite", [(V - 2, -3.0)], base=x)
    add("all_neg_inf", [], base=torch.full((V,), NEG))
    x = torch.full((V,), NEG)
    add("only_suppressed_finite", [(voc.sup[1], 4.0), (voc.sup[3], 5.0)], base=x)
    out = []
    for on in (False, True):
        out.append(Group(f"greedy_begin{int(on)}", voc, False, 2, 2, -1, on,
                         [Row(r.name, r.x, done=r.done, kind=r.kind, prompt=(1, 2)) for r in rows]))
    return out


PREFIXES = ("first", "ts", "ts_text", "ts_text_text", "ts_text_ts", "ts_text_ts_ts", "ts_ts")


def _prefixes(voc):
    """state name -> list of generated prefixes, the last timestamp at ts_begin, a middle value and V - 1."""
    tb, mid, top, tx = voc.ts_begin, voc.mid, voc.V - 1, TEXT_GEN
    return {
        "first": [[]],
        "ts": [[tb], [mid], [top]],
        "ts_text": [[tb, tx], [mid, tx], [top, tx]],
        "ts_text_text": [[tb, tx, tx + 1], [mid, tx, tx + 1], [top, tx, tx + 1]],
        "ts_text_ts": [[tb, tx, tb], [tb, tx, mid], [mid, tx, top]],
        "ts_text_ts_ts": [[tb, tx, tb, tb], [tb, tx, mid, mid], [tb, tx, top, top]],
        "ts_ts": [[tb, tb], [mid, mid], [top, top]],
    }


def _prompt(voc, gen, begin_col):
    """Five prompt ids holding timestamps (a conditioned prompt).  At the first step it ends in two timestamps, at
    later steps in a text id: whichever a selector that looked before begin_col would misread."""
    if begin_col == 0:
        return ()
    assert begin_col == 5
    if not gen:
        return (TEXT_GEN + 2, voc.ts_begin + 30, TEXT_GEN + 3, voc.V - 9, voc.V - 9)
    return (TEXT_GEN + 2, voc.ts_begin + 30, voc.V - 9, voc.V - 9, TEXT_GEN + 3)


def _ts_state_rows(g, state, gen, gen_):
    """The planted rows of one rule state.  Every row has <|notimestamps|> as its maximum (14), the best text id at
    12 (11 at eos + 2, the best id left in the open-pair state), timestamps far below unless planted."""
    voc = g.voc
    V, tb = voc.V, voc.ts_begin
    prompt = _prompt(voc, gen, g.begin_col)
    rows = []

    def base():
        x = _base(voc, gen_, ts_shift=-5.0)
        x[voc.no_ts] = 14.0
        x[TEXT_BEST] = 12.0
        x[voc.eos + 2] = 11.0
        return x

    def add(kind, x, done=0):
        rows.append(Row(f"{state}{gen}/{kind}", x, list(gen), done, kind, state, prompt))

    probe = Row("", base(), list(gen), prompt=prompt)
    elig = processed_row(g, probe, torch.float32, apply_mass=False)
    ok = (torch.nonzero(torch.isfinite(elig[tb:])).flatten() + tb).tolist()       # eligible timestamps
    bt = float(elig[:tb].max())                                                     # 12, 11 or -inf
    level = bt if bt > NEG else 8.0

    add("base", base())
    if ok:
        x = base(); x[ok[0]] = 13.0
        add("allowed_ts_at_lim", x)
    stamps = [t for t in gen if t >= tb]
    last_is, pen_is = bool(gen) and gen[-1] >= tb, len(gen) < 2 or gen[-2] >= tb
    if stamps:
        lim = stamps[-1] if (last_is and not pen_is) else stamps[-1] + 1
        if lim - 1 >= tb:
            x = base(); x[lim - 1] = 13.0
            add("forbid:ts_below_lim", x)
    if last_is and not pen_is:
        x = base(); x[TEXT_FORBID] = 13.0
        add("forbid:text_in_open_pair", x)
    if last_is and pen_is:
        x = base(); x[min(max(stamps[-1] + 1, tb + 5), V - 1)] = 13.0
        add("forbid:ts_in_closed_pair", x)
    if g.first:
        x = base(); x[TEXT_FORBID] = 13.0
        add("forbid:text_at_first", x)
        if g.max_initial >= 0:
            x = base(); x[tb + g.max_initial + 1] = 13.0
            add("forbid:ts_above_max_initial", x)
    if ok:
        n = min(30, len(ok))
        pick = sorted({ok[round(i * (len(ok) - 1) / max(n - 1, 1))] for i in range(n)})
        # (a) the mass of ~30 timestamps 2 below the best text beats it; with fewer than 8 eligible they sit above
        x = base(); x[pick] = level - 2.0 if len(pick) >= 20 else level + 0.5
        add("mass_a", x)
        x = base(); x[pick] = level - 6.0
        add("mass_b", x)
        if bt > NEG:
            x = base(); x[tb:] = NEG; x[ok[len(ok) // 2]] = bt
            add("mass_d", x)
    x = base()
    x[torch.rand(V, generator=gen_) < 0.2] = NEG
    x[voc.no_ts] = 14.0
    add("some_neg_inf", x)
    return rows


def ts_groups(voc, seed=23):
    """Every rule state of the timestamp selectors as call groups: begin_col 0 and 5 (a conditioned prompt holding
    timestamps), the first step under max_initial -1 / 0 / 50 with the begin mask off and on, later steps with a
    begin mask passed (it must not apply) and max_initial varied (it must not apply either)."""
    gen_ = torch.Generator().manual_seed(seed)
    pre = _prefixes(voc)
    by_len = {}
    for state, gens in pre.items():
        for gen in gens:
            by_len.setdefault(len(gen), []).append((state, gen))
    later_mi = {1: 0, 2: 50, 3: -1, 4: 0}
    out = []
    for bc in (0, 5):
        for n in sorted(by_len):
            cfgs = [(mi, on) for mi in (-1, 0, 50) for on in (False, True)] if n == 0 else [(later_mi[n], True)]
            for mi, on in cfgs:
                g = Group(f"ts_bc{bc}_len{n}_mi{mi}_beg{int(on)}", voc, True, bc, bc + n, mi, on, [])
                for state, gen in by_len[n]:
                    g.rows += _ts_state_rows(g, state, gen, gen_)
                g.rows.append(Row(f"len{n}/done_row", g.rows[0].x, list(g.rows[0].gen), 1, "done", g.rows[0].state,
                                  g.rows[0].prompt))
                out.append(g)
    return out


_cache = {}


def groups(kind, vocab):
    """The case table of a kernel family ("greedy" / "ts") on a vocabulary, built once per process."""
    key = (kind, vocab)
    if key not in _cache:
        _cache[key] = (greedy_groups if kind == "greedy" else ts_groups)(VOCABS[vocab])
    return _cache[key]


_ref_cache = {}


def group_reference(kind, vocab, gi, dtype):
    """[reference(row) for the rows of group gi], computed once per dtype."""
    key = (kind, vocab, gi, dtype)
    if key not in _ref_cache:
        g = groups(kind, vocab)[gi]
        _ref_cache[key] = [reference(g, r, dtype) for r in g.rows]
    return _ref_cache[key]
