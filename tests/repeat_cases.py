"""The repetition-penalty / no-repeat-n-gram pre-pass (csrc/repeat.hip, tw_repeat_process): a plain CPU restatement of
HF's two processors and the case table of its parity tests.

restate() is written from HF's semantics, not from its code (tests/test_repeat_cpu.py holds it to HF's
RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor bit for bit on this table):
  * penalty p != 1: every distinct token u of a row's history gets s[u] < 0 ? s[u] * p : s[u] / p, computed once from
    the unpenalised fp32 score with p rounded to fp32;
  * n-gram size n > 0: for every i in [0, L - n] with ids[i : i+n-1] == ids[L-n+1 : L], s[ids[i+n-1]] = -inf, after
    the penalty (n = 1 bans every token of the history; L < n bans nothing).

The table: vocabularies of 130 and 51865 ids (rows of ld = V rounded up to 64), every n in NGRAMS, every history
length in lengths(n), every penalty in PENALTIES, and per combination the 8 histories of KINDS over a row of scores
whose history tokens take the values of specials(dtype) in turn."""
import numpy as np
import torch

NEG = float("-inf")
VOCABS = {"small": 130, "real": 51865}
EOS = {"small": 100, "real": 50257}
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
BATCHES = (1, 8)
NGRAMS = (0, 1, 2, 3, 6)
PENALTIES = (1.0, 1.3, 0.5)
L_MAX = 447
KINDS = ("same", "period2", "period3", "norepeat", "eos_mid", "edges", "pool5", "edges3_eos_end")
ROWS = len(KINDS)
TRAP_OFFSET = 17               # the id the columns past the history hold: a token of no history


def ld_of(V):
    return (V + 63) // 64 * 64


def lengths(n):
    """History lengths for n-gram size n: 0, 1, n-2, n-1, n and the longest Whisper row."""
    return sorted({L for L in (0, 1, n - 2, n - 1, n, L_MAX) if L >= 0})


def combos():
    return [(n, L, p) for n in NGRAMS for L in lengths(n) for p in PENALTIES]


def specials(dtype):
    """Scores the history tokens take: positive, negative, both zeros, -inf, the largest finite value of the dtype and
    its negative, values whose quotient by 1.3 / 0.5 and product are not all exactly representable, and NaN."""
    big = float(torch.finfo(dtype).max)
    return [2.5, -1.75, 0.0, -0.0, NEG, big, 0.7, -big, -3.1415927, float("nan"), 1.0 / 3.0]


def history(kind, L, V, eos):
    """One row's history of length L.  norepeat: distinct ids while L <= V (a 130-id vocabulary cannot hold 447
    distinct ones: there the row repeats with period V)."""
    a, b, c = 5 % V, (V // 2 + 1) % V, (V - 7) % V
    if kind == "same":
        h = [a] * L
    elif kind == "period2":
        h = [(a, b)[i % 2] for i in range(L)]
    elif kind == "period3":
        h = [(a, b, c)[i % 3] for i in range(L)]
    elif kind == "norepeat":
        h = [(7 * i + 3) % V for i in range(L)]               # 7 is coprime to both vocabulary sizes
    elif kind == "eos_mid":
        h = [(a, b, c)[i % 3] for i in range(L)]
        for i in range(L // 2, min(L, L // 2 + 3)):
            h[i] = eos
    elif kind == "edges":
        h = [(0, V - 1)[i % 2] for i in range(L)]
    elif kind == "pool5":
        rng = np.random.default_rng(1000 + L)
        h = [int(t) for t in rng.choice([0, a, b, c, V - 1], size=L)]
    else:                                                       # edges3_eos_end
        h = [(V - 1, 0, b)[i % 3] for i in range(L)]
        for i in range(max(0, L - 2), L):
            h[i] = eos
    return h


def histories(L, V, eos):
    return [history(k, L, V, eos) for k in KINDS]


def id_matrix(hists, L, V, width=L_MAX + 3):
    """int64 [rows, width]: the histories, then a trap id no history holds -- a kernel that reads past L changes the
    trap's score."""
    ids = torch.full((len(hists), width), (V - TRAP_OFFSET) % V, dtype=torch.int64)
    for r, h in enumerate(hists):
        assert len(h) == L
        if L:
            ids[r, :L] = torch.tensor(h, dtype=torch.int64)
    return ids


def score_table(V, dtype, seed=7):
    """fp32 [ROWS, V] scores already rounded to dtype.  Every id a history of the table can hold takes a value of
    specials(dtype), shifted per row, so each special meets ids 0, V - 1, eos and the loop tokens in some row."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(ROWS, V, generator=g) * 3.0).to(dtype).float()
    sp = specials(dtype)
    eos = [e for v, e in zip(VOCABS.values(), EOS.values()) if v == V][0]
    toks = [0, 5 % V, (V // 2 + 1) % V, (V - 7) % V, V - 1, eos, (V - TRAP_OFFSET) % V] + \
        [(7 * i + 3) % V for i in range(12)]
    for r in range(ROWS):
        for k, t in enumerate(toks):
            x[r, t] = torch.tensor(sp[(k + r) % len(sp)]).to(dtype).float()
    return x


def restate(scores, hists, penalty, ngram):
    """scores fp32 [B, V], hists: B id lists -> fp32 [B, V] after the two processors."""
    assert scores.dtype == torch.float32
    out = scores.clone()
    V = scores.shape[1]
    p = torch.tensor(float(penalty), dtype=torch.float32)
    for b, h in enumerate(hists):
        L = len(h)
        if float(penalty) != 1.0:
            for u in sorted(set(h)):
                if 0 <= u < V:
                    s = scores[b, u]
                    out[b, u] = s * p if bool(s < 0) else s / p
        if ngram > 0 and L >= ngram:
            tail = h[L - ngram + 1:]
            for i in range(L - ngram + 1):
                if h[i:i + ngram - 1] == tail and 0 <= h[i + ngram - 1] < V:
                    out[b, h[i + ngram - 1]] = NEG
    return out


def same_bits(a, b):
    """Bit-identical, NaN positions included (a NaN's payload is not compared)."""
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb]))
