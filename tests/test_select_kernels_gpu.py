"""The token selection kernels of csrc/decode.hip against the plain fp64 reference of tests/select_cases.py.

Parity bar: ids, next_ids, done and last_ts equal to the reference exactly (the reference reads the logits after
rounding to the dtype under test, so both sides see the same bits), over the five slice counts of sel_slices
(B = 1, 17, 100, 256, 257 -> G = 32, 16, 4, 2, 1), bf16 / fp16 / fp32 logits, the 16-byte vector load path and the
scalar path forced three ways, and the host / device column modes; log-probs within 1e-4 absolute of the fp64
log_softmax of the processed row (the selector's bar in test_fallback_gpu.py); sampled tokens inside the processed
row's support and, over 8192 draws, a chi-square p > 1e-4 against softmax(processed / T)."""
import numpy as np
import pytest
import torch

import select_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_DT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
dtypes = pytest.mark.parametrize("dtype", sc.DTYPES, ids=lambda d: _DT[d])
vocabs = pytest.mark.parametrize("vocab", ["small", "real"])
batches = pytest.mark.parametrize("B", sc.BATCHES)


class _Dev:
    """A group's rows and their state before the call, on the device."""

    def __init__(self, g, dtype):
        self.tab = torch.stack([r.x for r in g.rows]).to(dtype).to(DEV)
        self.ids0 = torch.stack([sc.row_ids(g, r) for r in g.rows]).to(DEV)
        self.done0 = torch.tensor([r.done for r in g.rows], dtype=torch.uint8, device=DEV)
        self.last0 = torch.tensor([sc.row_last_ts(g.voc, r) for r in g.rows], dtype=torch.int32, device=DEV)
        self.sup = self.beg = None


_dev_cache = {}


def _dev(kind, vocab, dtype):
    """Device copies of every group of (kind, vocab) in dtype; one (kind, vocab, dtype) is kept at a time."""
    from tw import ops as F
    key = (kind, vocab, dtype)
    if key not in _dev_cache:
        _dev_cache.clear()
        voc = sc.VOCABS[vocab]
        out = []
        for g in sc.groups(kind, vocab):
            d = _Dev(g, dtype)
            d.sup = F.token_bitmask(voc.sup, voc.V, DEV)
            d.beg = F.token_bitmask(voc.beg, voc.V, DEV)
            out.append(d)
        _dev_cache[key] = out
    return _dev_cache[key]


_consts = {}


def _const(key, make):
    """Small device constants (column words, padding values, zeroed control words), uploaded once."""
    if key not in _consts:
        _consts[key] = make()
    return _consts[key]


def _layout(rows, voc, layout):
    """rows [B, V] placed as the kernel's logits operand -> (tensor whose data_ptr is row 0, ld).  Columns [V, ld)
    hold, row by row in turn, +inf, the largest finite value and NaN."""
    B, V = rows.shape
    if layout == "ld_eq_v":
        return rows.contiguous(), V
    if layout == "vec":
        ld = voc.ld
        view = torch.empty(B, ld, dtype=rows.dtype, device=DEV)
    elif layout == "ld_odd":
        ld = voc.ceil8 + 1
        view = torch.empty(B, ld, dtype=rows.dtype, device=DEV)
    else:                                                   # one element into an aligned buffer
        ld = voc.ld
        flat = torch.zeros(B * ld + 16, dtype=rows.dtype, device=DEV)
        view = flat[1:1 + B * ld].view(B, ld)
    view[:, :V] = rows
    pad = _const(("pad", rows.dtype, B), lambda: torch.tensor(
        [float("inf"), torch.finfo(rows.dtype).max, float("nan")], dtype=rows.dtype, device=DEV)[
            torch.arange(B, device=DEV) % 3][:, None])
    view[:, V:] = pad
    vec = view.data_ptr() % 16 == 0 and ld % 8 == 0 and ld >= voc.ceil8
    assert vec == (layout == "vec")
    return view, ld


def _call(F, g, d, kernel, logits, ld, ids, done, nxt, last, tdev, ctl=None, slp=None, col=None, begin_on=None):
    """One selector call on a batch in host-column or device-column mode."""
    voc, B = g.voc, ids.shape[0]
    col = g.col if col is None else col
    begin_on = g.begin_on if begin_on is None else begin_on
    t_dev = _const(("t", col - 1), lambda: torch.tensor([col - 1], dtype=torch.int32, device=DEV)) if tdev else None
    c = 1 if tdev else col
    if g.ts:
        beg = d.beg if begin_on else None
        kw = dict(ts_begin=voc.ts_begin, no_ts=voc.no_ts, max_initial=g.max_initial, t_dev=t_dev)
        if kernel == "greedy":
            F.greedy_select_ts(logits, ld, B, voc.V, d.sup, beg, voc.eos, done, ids, c, nxt, last, g.begin_col, **kw)
        else:
            F.select_sample_ts(logits, ld, B, voc.V, d.sup, beg, voc.eos, done, ids, c, nxt, last, g.begin_col, ctl,
                               slp, **kw)
    else:
        apply = bool(begin_on) and not tdev                 # device mode decides by *t_dev + col == begin_col
        bc = (col if begin_on else col + 1) if tdev else -1
        if kernel == "greedy":
            F.greedy_select(logits, ld, B, voc.V, d.sup, d.beg, apply, voc.eos, done, ids, c, nxt, t_dev=t_dev,
                            begin_col=bc)
        else:
            F.select_sample(logits, ld, B, voc.V, d.sup, d.beg, apply, voc.eos, done, ids, c, nxt, ctl, slp,
                            t_dev=t_dev, begin_col=bc)


def _run(F, g, d, B, layout, tdev, kernel, ctl_of=None):
    """Every row of the group through the kernel in batches of B (rows repeat cyclically to fill a batch) -> the
    outputs of every batch position of every call on the host, with "row" = the group row each position held.
    ctl_of(row indices) -> control words of a batch (default: 1/T = 0)."""
    N = len(g.rows)
    out = dict(row=[], ids=[], nxt=[], done=[], last=[], slp=[])
    ar = torch.arange(B, device=DEV)
    for s in range(0, N, B):
        idx = (ar + s) % N
        logits, ld = _layout(d.tab[idx], g.voc, layout)
        ids, done, last = d.ids0[idx], d.done0[idx], d.last0[idx]
        nxt = torch.full((B,), -7, dtype=torch.int64, device=DEV)
        slp = torch.full((B,), sc.SLP0, dtype=torch.float32, device=DEV)
        ctl = (_const(("ctl0", B), lambda: torch.zeros(3 * B, dtype=torch.int32, device=DEV)) if ctl_of is None
               else ctl_of(idx.cpu().tolist()))
        _call(F, g, d, kernel, logits, ld, ids, done, nxt, last, tdev, ctl, slp)
        for k, v in zip(("row", "ids", "nxt", "done", "last", "slp"), (idx, ids, nxt, done, last, slp)):
            out[k].append(v)
    torch.cuda.synchronize()
    return {k: torch.cat(v).cpu() for k, v in out.items()}


def _expected(g, d, refs):
    """Per group row: the reference's outputs, its log-prob (0 where there is none) and which rows carry one."""
    ids = d.ids0.cpu().clone()
    tok = torch.tensor([r["tok"] for r in refs], dtype=torch.int64)
    ids[:, g.col] = tok
    live = torch.tensor([not row.done and r["any_finite"] for row, r in zip(g.rows, refs)])
    return dict(ids=ids, nxt=tok, done=torch.tensor([r["done"] for r in refs], dtype=torch.uint8),
                last=torch.tensor([r["last_ts"] for r in refs], dtype=torch.int32),
                logp=torch.tensor([r["logp"] if r["logp"] is not None else 0.0 for r in refs], dtype=torch.float64),
                live=live, fin=torch.tensor([bool(row.done) for row in g.rows]))


def _check_exact(g, got, exp, what):
    """Every batch position of every call against the reference of the row it held."""
    row = got["row"]
    for k in ("ids", "nxt", "done", "last"):
        want = exp[k][row]
        if torch.equal(got[k], want):
            continue
        bad = torch.nonzero((got[k] != want).reshape(len(row), -1).any(-1)).flatten().tolist()
        ex = [(p, g.rows[int(row[p])].name, got[k][p].tolist(), want[p].tolist()) for p in bad[:6]]
        raise AssertionError(f"{what} {g.name} {k}: {len(bad)} of {len(row)} positions differ, "
                             f"(position, row, got, want) e.g. {ex}")


def _check_logp(g, got, exp, what):
    """sum_logp of every batch position: untouched on finished rows, += the fp64 log-prob elsewhere (rows with
    nothing finite are only held to the id, as the comment at greedy_finish).  -> the largest error."""
    row, v = got["row"], got["slp"].double()
    fin, live = exp["fin"][row], exp["live"][row]
    assert bool((v[fin] == sc.SLP0).all()), (what, g.name, "a finished row's sum_logp changed")
    err = (v - (sc.SLP0 + exp["logp"][row])).abs()[live]
    if err.numel() == 0:
        return 0.0
    p = int(err.argmax())
    assert float(err.max()) <= sc.LOGP_ATOL, (what, g.name, g.rows[int(row[live][p])].name, float(err.max()))
    return float(err.max())


def _matrix(kind, vocab, dtype, B):
    from tw import ops as F
    assert sc.slices(B, sc.VOCABS[vocab].V)[0] == sc.SLICES[sc.BATCHES.index(B)]
    worst = 0.0
    for gi, (g, d) in enumerate(zip(sc.groups(kind, vocab), _dev(kind, vocab, dtype))):
        refs = sc.group_reference(kind, vocab, gi, dtype)
        exp = _expected(g, d, refs)
        for layout in sc.LAYOUTS:
            for tdev in (False, True):
                for kernel in ("greedy", "sample"):
                    what = f"{kernel} B={B} {layout} t_dev={int(tdev)}"
                    got = _run(F, g, d, B, layout, tdev, kernel)
                    _check_exact(g, got, exp, what)
                    if kernel == "sample":
                        worst = max(worst, _check_logp(g, got, exp, what))
    print(f"\n[select] {kind} {vocab} {_DT[dtype]} B={B}: max |sum_logp - fp64| = {worst:.3e}")


@batches
@dtypes
@vocabs
def test_greedy_matrix(vocab, dtype, B):
    """greedy_select and select_sample at 1/T = 0: winner positions, ties, masked winners, padding columns, -inf
    rows, finished rows, eos."""
    _matrix("greedy", vocab, dtype, B)


@batches
@dtypes
@vocabs
def test_timestamp_matrix(vocab, dtype, B):
    """greedy_select_ts and select_sample_ts at 1/T = 0 over every state of the timestamp rules."""
    _matrix("ts", vocab, dtype, B)


@vocabs
def test_sum_logp_accumulates_over_two_columns(vocab):
    from tw import ops as F
    dtype, B = torch.bfloat16, 17
    on, off = sc.groups("greedy", vocab)[1], sc.groups("greedy", vocab)[0]
    d = _dev("greedy", vocab, dtype)[1]
    N = len(on.rows)
    r1 = [sc.reference(on, r, dtype) for r in on.rows]
    ar = torch.arange(B, device=DEV)
    for s in range(0, N, B):
        idx = (ar + s) % N
        logits, ld = _layout(d.tab[idx], on.voc, "vec")
        ids, done, last = d.ids0[idx], d.done0[idx], d.last0[idx]
        nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
        slp = torch.full((B,), sc.SLP0, dtype=torch.float32, device=DEV)
        ctl = torch.zeros(3 * B, dtype=torch.int32, device=DEV)
        _call(F, on, d, "sample", logits, ld, ids, done, nxt, last, False, ctl, slp)
        slp1 = slp.clone()
        _call(F, on, d, "sample", logits, ld, ids, done, nxt, last, False, ctl, slp, col=on.col + 1, begin_on=False)
        torch.cuda.synchronize()
        slp1, slp2 = slp1.cpu().double(), slp.cpu().double()
        for j, i in enumerate(idx.cpu().tolist()):
            row, a = on.rows[i], r1[i]
            b = sc.reference(off, sc.Row(row.name, row.x, done=a["done"]), dtype)
            assert ids[j, on.col:on.col + 2].cpu().tolist() == [a["tok"], b["tok"]], row.name
            assert int(done[j]) == b["done"] and int(nxt[j]) == b["tok"], row.name
            if not a["any_finite"] or not b["any_finite"]:
                continue                                    # nothing finite: held to the ids only
            # each column's increment against its own fp64 log-prob (0 once the row is finished)
            assert abs(float(slp1[j]) - (sc.SLP0 + (a["logp"] or 0.0))) <= sc.LOGP_ATOL, (row.name, float(slp1[j]))
            assert abs(float(slp2[j] - slp1[j]) - (b["logp"] or 0.0)) <= sc.LOGP_ATOL, (row.name, float(slp2[j]))
            if b["logp"] is None:
                assert float(slp2[j]) == float(slp1[j]), row.name


def _ctl(F, temps, seeds):
    return F.sample_ctl(list(temps), list(seeds)).to(DEV)


@dtypes
def test_sampled_tokens_stay_in_the_processed_support(dtype):
    """Every rule state on the small vocabulary: 2048 rows of the same logits, distinct seeds, T = 1.  Each drawn id
    is finite in the reference's processed row (text ids excluded when the mass rule fires); last_ts follows it."""
    from tw import ops as F
    B = 2048
    voc = sc.SMALL
    ctl = _ctl(F, [1.0] * B, [17 + 7919 * b for b in range(B)])
    for gi, (g, d) in enumerate(zip(sc.groups("ts", "small"), _dev("ts", "small", dtype))):
        refs = sc.group_reference("ts", "small", gi, dtype)
        toks, lasts = [], []
        for i, row in enumerate(g.rows):
            logits, ld = _layout(d.tab[i:i + 1].expand(B, -1), voc, "vec")
            ids = d.ids0[i:i + 1].repeat(B, 1)
            done = torch.zeros(B, dtype=torch.uint8, device=DEV)
            last = d.last0[i:i + 1].repeat(B)
            nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
            slp = torch.zeros(B, dtype=torch.float32, device=DEV)
            _call(F, g, d, "sample", logits, ld, ids, done, nxt, last, bool(i & 1), ctl, slp)
            toks.append(ids[:, g.col]); lasts.append(last)
        toks, lasts = torch.stack(toks).cpu(), torch.stack(lasts).cpu()
        for i, (row, r) in enumerate(zip(g.rows, refs)):
            ok = torch.isfinite(r["row"])
            if not bool(ok.any()):
                assert bool((toks[i] == 0).all()), (g.name, row.name)
                continue
            assert bool(ok[toks[i]].all()), (g.name, row.name, sorted(set(toks[i][~ok[toks[i]]].tolist()))[:8])
            want_last = torch.where(toks[i] >= voc.ts_begin, toks[i], torch.full_like(toks[i], sc.row_last_ts(voc, row)))
            assert torch.equal(lasts[i].long(), want_last), (g.name, row.name)


def _find(vocab, state, kind, begin_col=5):
    for gi, g in enumerate(sc.groups("ts", vocab)):
        for i, r in enumerate(g.rows):
            if g.begin_col == begin_col and r.state == state and r.kind == kind:
                return gi, i
    raise KeyError((state, kind))


@pytest.mark.parametrize("T", [0.5, 2.0])
@pytest.mark.parametrize("state,kind", [("ts_text_ts", "mass_b"), ("ts_text", "mass_a")],
                         ids=["open_pair", "mass_fired"])
def test_sampled_distribution_and_logprob_ts(state, kind, T):
    """8192 draws of select_sample_ts against softmax(processed / T) (chi-square, p > 1e-4), and sum_logp against the
    fp64 log_softmax of the untempered processed row at the drawn id."""
    from tw import ops as F
    B, dtype, voc = 8192, torch.bfloat16, sc.SMALL
    gi, i = _find("small", state, kind)
    g, d = sc.groups("ts", "small")[gi], _dev("ts", "small", dtype)[gi]
    r = sc.group_reference("ts", "small", gi, dtype)[i]["row"]
    if kind == "mass_a":
        assert not bool(torch.isfinite(r[:voc.ts_begin]).any())             # the mass rule fired: timestamps only
    logits, ld = _layout(d.tab[i:i + 1].expand(B, -1), voc, "vec")
    ids = d.ids0[i:i + 1].repeat(B, 1)
    done = torch.zeros(B, dtype=torch.uint8, device=DEV)
    last = d.last0[i:i + 1].repeat(B)
    nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
    slp = torch.full((B,), sc.SLP0, dtype=torch.float32, device=DEV)
    _call(F, g, d, "sample", logits, ld, ids, done, nxt, last, False,
          _ctl(F, [T] * B, [4321 + 7919 * b for b in range(B)]), slp)
    torch.cuda.synchronize()
    tok = ids[:, g.col].cpu()
    assert bool(torch.isfinite(r[tok]).all())
    p = torch.softmax(r / T, -1)
    from test_fallback_gpu import _chi2_pvalue
    pv = _chi2_pvalue(torch.bincount(tok, minlength=voc.V).double(), p * B)
    lp = torch.log_softmax(r, -1)[tok]
    err = float((slp.cpu().double() - (sc.SLP0 + lp)).abs().max())
    print(f"\n[select] sample_ts {state}/{kind} T={T}: chi-square p = {pv:.4g}, max |sum_logp - fp64| = {err:.3e}, "
          f"{len(set(tok.tolist()))} distinct ids")
    assert pv > 1e-4
    assert err <= sc.LOGP_ATOL


@pytest.mark.parametrize("kind", ["greedy", "ts"])
def test_a_row_draws_the_same_token_in_any_batch(kind):
    """read_ctl's promise: the same logits row with the same (T, seed) gives the same token alone (32 slices), as row
    9 of 17 (16 slices) and as row 200 of 257 (one workgroup per row)."""
    from tw import ops as F
    dtype, vocab = torch.bfloat16, "real"
    gs = sc.groups(kind, vocab)
    gi = len(gs) - 1 if kind == "greedy" else next(i for i, g in enumerate(gs) if g.begin_col == 5 and g.col == 8)
    g, d = gs[gi], _dev(kind, vocab, dtype)[gi]
    N = len(g.rows)
    picks = [i for i, r in enumerate(g.rows) if not r.done][::max(1, N // 6)][:6]
    for n, i in enumerate(picks):
        for T in (0.7, 1.5):
            seed = 1000003 * (n + 1) + int(T * 10)
            toks = []
            for B, at in ((1, 0), (17, 9), (257, 200)):
                idx = (torch.arange(B, device=DEV) + 3 * n) % N
                idx[at] = i
                temps = [1.0 + 0.01 * (b % 7) for b in range(B)]
                seeds = [99 + b for b in range(B)]
                temps[at], seeds[at] = T, seed
                logits, ld = _layout(d.tab[idx], g.voc, "vec")
                ids, done, last = d.ids0[idx], torch.zeros(B, dtype=torch.uint8, device=DEV), d.last0[idx]
                nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
                slp = torch.zeros(B, dtype=torch.float32, device=DEV)
                _call(F, g, d, "sample", logits, ld, ids, done, nxt, last, B == 17, _ctl(F, temps, seeds), slp)
                toks.append(int(ids[at, g.col]))
            assert toks[0] == toks[1] == toks[2], (g.rows[i].name, T, toks)
            assert bool(torch.isfinite(sc.group_reference(kind, vocab, gi, dtype)[i]["row"][toks[0]]))


@pytest.mark.parametrize("kind,vocab,B", [("greedy", "real", 100), ("ts", "small", 17), ("ts", "real", 256)])
def test_mixed_control_words_in_one_batch(kind, vocab, B):
    """Rows with 1/T = 0 give exactly the plain selector's ids whatever their neighbours do; rows with T > 0 stay in
    the processed support and their sum_logp is the fp64 log-prob of the drawn id."""
    from tw import ops as F
    dtype = torch.bfloat16
    voc = sc.VOCABS[vocab]

    def ctl_of(rows):
        return _ctl(F, [0.0 if i % 2 == 0 else 1.0 for i in rows], [31 + 7 * i for i in rows])

    for gi, (g, d) in enumerate(zip(sc.groups(kind, vocab), _dev(kind, vocab, dtype))):
        refs = sc.group_reference(kind, vocab, gi, dtype)
        plain = _run(F, g, d, B, "vec", False, "greedy")
        got = _run(F, g, d, B, "vec", True, "sample", ctl_of)
        assert torch.equal(plain["row"], got["row"])
        lsm = {}
        for p, i in enumerate(got["row"].tolist()):
            row, r = g.rows[i], refs[i]
            tok = int(got["nxt"][p])
            assert int(got["ids"][p, g.col]) == tok
            if i % 2 == 0 or row.done or not r["any_finite"]:
                assert tok == int(plain["nxt"][p]) == r["tok"], (g.name, row.name, p)
                continue
            assert bool(torch.isfinite(r["row"][tok])), (g.name, row.name, p, tok)
            if i not in lsm:
                lsm[i] = torch.log_softmax(r["row"], -1)
            lp = float(lsm[i][tok])
            assert abs(float(got["slp"][p]) - (sc.SLP0 + lp)) <= sc.LOGP_ATOL, (g.name, row.name, p)
            assert int(got["done"][p]) == int(tok == voc.eos)
            if g.ts:
                assert int(got["last"][p]) == (tok if tok >= voc.ts_begin else sc.row_last_ts(voc, row))


@dtypes
@vocabs
def test_token_logprob(vocab, dtype):
    """log_softmax of a raw row at one id against fp64: rows holding -inf, a token whose own logit is -inf (-> -inf),
    V no multiple of 256, +inf / NaN in the padding columns."""
    from tw import ops as F
    voc = sc.VOCABS[vocab]
    V, ld, B = voc.V, voc.ld, 7
    assert V % 256 != 0
    gen_ = torch.Generator().manual_seed(41)
    x = (torch.randn(B, V, generator=gen_) * 3.0).clamp_(-9.5, 9.5)
    tokens = [0, 1, V - 1, voc.no_ts - 1, 255, 256]
    x[1][torch.rand(V, generator=gen_) < 0.3] = sc.NEG
    x[2, :V - 40] = sc.NEG
    x[3, tokens] = sc.NEG                                    # the token's own logit is -inf
    x[4, V - 1] = 12.0
    x[1, tokens] = torch.tensor([1.0, -2.0, 3.0, 0.5, -7.0, 9.0])
    x[2, tokens] = 2.0
    full = torch.empty(B, ld, dtype=dtype)
    full[:, :V] = x.to(dtype)
    pad = torch.tensor([float("inf"), float("nan")], dtype=dtype)
    full[:, V:] = pad[torch.arange(B) % 2][:, None]
    dev = full.to(DEV)
    ref = torch.log_softmax(full[:, :V].double(), -1)
    worst = 0.0
    for t in tokens:
        out = torch.full((B,), 7.0, dtype=torch.float32, device=DEV)
        F.token_logprob(dev, ld, B, V, t, out)
        got, want = out.cpu().double(), ref[:, t]
        inf = torch.isinf(want)
        assert bool(inf[3]) and torch.equal(got[inf], want[inf]), (t, got, want)
        np.testing.assert_allclose(got[~inf].numpy(), want[~inf].numpy(), rtol=0, atol=sc.LOGP_ATOL)
        worst = max(worst, float((got[~inf] - want[~inf]).abs().max()))
    print(f"\n[select] token_logprob {vocab} {_DT[dtype]}: max |logp - fp64| = {worst:.3e}")
