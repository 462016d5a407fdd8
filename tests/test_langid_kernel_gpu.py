"""tw_lang_detect (csrc/langid.hip) against the CPU restatement of tests/langid_cases.py.

Parity bar.  Ids: bit-exact to the restatement on the whole case table, written to a contiguous [B] vector and into
column 1 of a [B, T] matrix whose other elements keep a sentinel.  Probabilities, against the float64 restatement:
|p - p64| <= p64 * (L + 6 + |x_j - max|) * 2^-23 (langid_cases.prob_bound: derived from the fp32 operations, not
measured); NaN rows (a NaN language logit, or only -inf) are NaN in every column.  The logits' columns [V, ld) hold NaN
throughout and change nothing; out_probs' columns [L, ld_p) keep the sentinel.  The worst err / bound ratio per dtype
is printed, and appended to $TW_PARITY_DIR/langid_parity.txt when that variable names a directory (profiles/langid_parity.txt
is such a run's file)."""
import os

import pytest
import torch

import langid_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT_ID = -777
SENT_P = 12345.0
_DT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _chunks(B):
    return [(r, min(B, lc.ROWS - r)) for r in range(0, lc.ROWS, B)]


@pytest.mark.parametrize("B", lc.BATCHES)
@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lambda d: _DT[d])
@pytest.mark.parametrize("vocab", list(lc.VOCABS))
def test_lang_detect_matches_restatement(vocab, dtype, B):
    from tw import ops as F
    V, ld = lc.VOCABS[vocab]
    bad, worst, nan_rows = [], 0.0, 0
    for L, tk in lc.combos(vocab):
        table = lc.table_of(tk, L, V)
        x = lc.score_rows(V, table, dtype)
        want_ids, p64 = lc.lang_detect_ref(x, table)
        bound = lc.prob_bound(x, table, p64)
        logits = torch.full((lc.ROWS, ld), float("nan"), dtype=dtype, device=DEV)
        logits[:, :V] = x.to(dtype).to(DEV)
        tab = torch.tensor(table, dtype=torch.int32, device=DEV)
        ids = torch.full((lc.ROWS,), SENT_ID, dtype=torch.int64, device=DEV)
        mat = torch.full((lc.ROWS, 5), SENT_ID, dtype=torch.int64, device=DEV)
        ld_p = L + 3
        probs = torch.full((lc.ROWS, ld_p), SENT_P, dtype=torch.float32, device=DEV)
        for r, n in _chunks(B):
            F.lang_detect(logits[r:], ld, n, V, tab, ids[r:r + n], probs[r:r + n])
            F.lang_detect(logits[r:], ld, n, V, tab, mat[r:r + n, 1])
        ids, mat, probs = ids.cpu(), mat.cpu(), probs.cpu()
        if not torch.equal(ids, want_ids) or not torch.equal(mat[:, 1], want_ids):
            bad.append(("ids", L, tk, ids.tolist(), want_ids.tolist()))
        if not bool((mat[:, [0, 2, 3, 4]] == SENT_ID).all()) or not bool((probs[:, L:] == SENT_P).all()):
            bad.append(("sentinel", L, tk))
        nan = torch.isnan(p64).any(dim=1)
        assert bool(torch.isnan(p64[nan]).all())
        nan_rows += int(nan.sum())
        p = probs[:, :L].double()
        if not bool(torch.isnan(p[nan]).all()) or bool(torch.isnan(p[~nan]).any()):
            bad.append(("nan", L, tk))
        err = (p[~nan] - p64[~nan]).abs()
        if not bool((err <= bound[~nan]).all()):
            bad.append(("probs", L, tk, float((err / bound[~nan].clamp_min(1e-300)).max())))
        pos = bound[~nan] > 0
        if bool(pos.any()):
            worst = max(worst, float((err[pos] / bound[~nan][pos]).max()))
    print(f"lang_detect {vocab} {_DT[dtype]} B={B}: worst |p - p64| / bound = {worst:.4f}")
    if os.environ.get("TW_PARITY_DIR"):
        with open(os.path.join(os.environ["TW_PARITY_DIR"], "langid_parity.txt"), "a") as f:
            f.write(f"{vocab:6s} {_DT[dtype]:5s} B={B}: worst |p - p64| / bound = {worst:.4f}\n")
    assert not bad, bad[:6]
    assert nan_rows >= 2 * len(lc.combos(vocab))                    # the NaN and the all -inf row of every combination


def test_lang_detect_unaligned():
    """ld == V == 130 (rows not 16-byte aligned) and both outputs one element into their buffers."""
    from tw import ops as F
    V = 130
    for dtype in lc.DTYPES:
        for L, tk in ((65, "scattered"), (99, "contiguous")):
            table = lc.table_of(tk, L, V)
            x = lc.score_rows(V, table, dtype)
            want_ids, p64 = lc.lang_detect_ref(x, table)
            logits = x.to(dtype).to(DEV).contiguous()
            tab = torch.tensor(table, dtype=torch.int32, device=DEV)
            fi = torch.full((lc.ROWS + 2,), SENT_ID, dtype=torch.int64, device=DEV)
            fp = torch.full((lc.ROWS * L + 2,), SENT_P, dtype=torch.float32, device=DEV)
            F.lang_detect(logits, V, lc.ROWS, V, tab, fi[1:1 + lc.ROWS], fp[1:1 + lc.ROWS * L].view(lc.ROWS, L))
            fi, fp = fi.cpu(), fp.cpu()
            assert torch.equal(fi[1:-1], want_ids) and int(fi[0]) == SENT_ID and int(fi[-1]) == SENT_ID
            assert float(fp[0]) == SENT_P and float(fp[-1]) == SENT_P
            p = fp[1:-1].view(lc.ROWS, L).double()
            nan = torch.isnan(p64).any(dim=1)
            assert bool(torch.isnan(p[nan]).all())
            assert bool(((p[~nan] - p64[~nan]).abs() <= lc.prob_bound(x, table, p64)[~nan]).all())


def test_lang_detect_bad_arguments_write_nothing():
    from tw import _native
    lib = _native.lib()
    V, ld, B, L = 130, 192, 2, 5
    logits = torch.zeros(B, ld, dtype=torch.float32, device=DEV)
    tab = torch.tensor([3, 4, 5, 6, 7], dtype=torch.int32, device=DEV)
    ids = torch.full((B,), SENT_ID, dtype=torch.int64, device=DEV)
    probs = torch.full((B, 8), SENT_P, dtype=torch.float32, device=DEV)

    def call(ld=ld, dt=0, B=B, V=V, L=L, ld_p=8, tab_p=tab.data_ptr(), ids_p=ids.data_ptr(), probs_p=probs.data_ptr(),
             logits_p=logits.data_ptr(), id_stride=1):
        return lib.tw_lang_detect(logits_p, ld, dt, B, V, tab_p, L, ids_p, id_stride, probs_p, ld_p,
                                  torch.cuda.current_stream().cuda_stream)
    for kw in (dict(B=-1), dict(V=0), dict(V=-3), dict(ld=V - 1), dict(L=0), dict(L=257), dict(ld_p=L - 1),
               dict(tab_p=None), dict(ids_p=None), dict(logits_p=None), dict(id_stride=0), dict(id_stride=-1)):
        assert call(**kw) == 1, kw
    for dt in (3, -1, 7):
        assert call(dt=dt) == 2, dt
    assert call(B=0) == 0                                           # nothing to do: TW_OK, nothing launched
    torch.cuda.synchronize()
    assert bool((ids == SENT_ID).all()) and bool((probs == SENT_P).all())
    assert call(ld_p=L - 1, probs_p=None) == 0                      # no probabilities: ld_p is not looked at
    torch.cuda.synchronize()
    assert bool((ids == 3).all()) and bool((probs == SENT_P).all())   # all-equal logits: the lowest id
    assert call() == 0                                              # the same arguments, valid: it runs
    torch.cuda.synchronize()
    assert bool((ids == 3).all()) and bool((probs[:, :L] == 0.2).all()) and bool((probs[:, L:] == SENT_P).all())
