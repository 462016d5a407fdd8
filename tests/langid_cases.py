"""Language detection (csrc/langid.hip, tw_lang_detect): a plain CPU restatement and the case table of its parity
tests.

lang_detect_ref() is written from the semantics, not from HF's code (tests/test_langid_cpu.py holds its ids to HF's
own expression -- mask every other logit to -inf, argmax -- on every finite row): per row, over the fp32 values at
the table's ids, the id of the largest value with ties to the lowest id and a NaN above every number (the lowest-id
NaN first), and in float64 the softmax over those values alone (a NaN, or only -inf, in them: a NaN row).

The table: vocabularies of 130 (rows of 192), 51865 and 51866 ids (rows of 51904), L in LS language ids in a
contiguous and in a scattered table (the latter holds id 0 and id V - 1), and per combination the rows of KINDS."""
import torch

NEG = float("-inf")
VOCABS = {"small": (130, 192), "v2": (51865, 51904), "v3": (51866, 51904)}
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
BATCHES = (1, 8)
LS = (1, 2, 63, 64, 65, 99, 100, 256)
TABLES = ("contiguous", "scattered")
KINDS = ("random", "max_first", "max_last", "tie_groups", "tie_in_group", "non_language_larger", "some_neg_inf",
         "all_neg_inf", "nan_one", "tie_after_rounding")
ROWS = len(KINDS)
FINITE = tuple(k for k in KINDS if k not in ("all_neg_inf", "nan_one"))


def table_of(kind, L, V):
    """L ascending unique language ids.  contiguous: large-v2's block from 50259 (from 3 at the small vocabulary,
    wrapped to fit); scattered: evenly spread with id 0 and id V - 1 at the ends."""
    if L > V:
        return None
    if kind == "contiguous":
        first = min(50259 if V > 51000 else 3, V - L)
        return list(range(first, first + L))
    if L == 1:
        return [V - 1]
    ids = sorted({(j * (V - 1)) // (L - 1) for j in range(L)})
    assert len(ids) == L and ids[0] == 0 and ids[-1] == V - 1
    return ids


def combos(vocab):
    V = VOCABS[vocab][0]
    return [(L, tk) for L in LS for tk in TABLES if table_of(tk, L, V) is not None]


def score_rows(V, table, dtype, seed=11):
    """fp32 [ROWS, V] scores already rounded to dtype, one row per KINDS entry."""
    L = len(table)
    g = torch.Generator().manual_seed(seed + L)
    x = (torch.randn(ROWS, V, generator=g) * 3.0).clamp(-9.0, 9.0)
    t = torch.tensor(table)
    big = 12.0
    for r, kind in enumerate(KINDS):
        if kind == "max_first":
            x[r, table[0]] = big
        elif kind == "max_last":
            x[r, table[-1]] = big
        elif kind == "tie_groups":            # entries of different 64-lane groups (where L allows), the later first
            for j in (L - 1, L // 2, min(L - 1, 1)):
                x[r, table[j]] = big
        elif kind == "tie_in_group":          # two entries of the first 64
            for j in (min(L - 1, 40), min(L - 1, 7)):
                x[r, table[j]] = big
        elif kind == "non_language_larger":
            other = [i for i in (0, 1, V // 2, V - 2, V - 1, table[0] - 1, table[-1] + 1) if 0 <= i < V
                     and i not in table]
            for i in other:
                x[r, i] = 2 * big
        elif kind == "some_neg_inf":
            x[r, t[::2]] = NEG
            if L == 1:
                x[r, table[0]] = 1.5
        elif kind == "all_neg_inf":
            x[r, t] = NEG
        elif kind == "nan_one":
            x[r, table[0]] = big                    # a larger number in front of the NaNs (L = 1: the NaN alone)
            x[r, table[L // 2]] = float("nan")
            x[r, table[-1]] = float("nan")
        elif kind == "tie_after_rounding":
            # distinct in fp32, equal once rounded to bf16 (8 bits) or fp16 (11 bits); the larger fp32 one is later
            x[r, t] = x[r, t].clamp(max=6.0)
            x[r, table[0]] = 8.0
            x[r, table[-1]] = 8.0 + 2.0 ** -10
            x[r, table[L // 2]] = 8.0 + 2.0 ** -9 if L > 2 else x[r, table[L // 2]]
    return x.to(dtype).float()


def lang_detect_ref(x, table):
    """x fp32 [B, V], table: ascending ids -> (ids int64 [B], probs float64 [B, L])."""
    assert x.dtype == torch.float32
    t = torch.tensor(table, dtype=torch.int64)
    g = x[:, t]
    ids = []
    for row in g.tolist():
        best = 0
        for j in range(1, len(row)):
            a, b = row[j], row[best]
            if a != a:
                if b == b:
                    best = j
            elif b == b and a > b:
                best = j
        ids.append(table[best])
    g64 = g.double()
    m = g64.max(dim=1, keepdim=True).values            # NaN when the row holds one
    e = torch.exp(g64 - m)                             # -inf - -inf = NaN on an all -inf row
    return torch.tensor(ids, dtype=torch.int64), e / e.sum(dim=1, keepdim=True)


def prob_bound(x, table, p64):
    """The derived bound on |p - p64| for fp32 device probabilities: p64 * (L + 6 + |x_j - max|) * 2^-23 -- the
    fp32 subtraction's half-ulp scaled by the exponent's argument, expf within 2 ulp, L additions of positive
    terms, one division, and a factor 2."""
    t = torch.tensor(table, dtype=torch.int64)
    g = x[:, t].double()
    d = (g - g.max(dim=1, keepdim=True).values).abs()
    d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
    return p64 * (len(table) + 6 + d) * 2.0 ** -23
