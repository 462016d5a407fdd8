"""tw_repeat_process (csrc/repeat.hip) against the CPU restatement of tests/repeat_cases.py.

Parity bar: out[:, :V] bit-identical to the restatement applied to the fp32 view of the same logits, -inf and NaN
positions included; the output's columns [V, ld) untouched; NaN in the input's columns [V, ld) without effect.  Per
(vocabulary, dtype, batch) every (n, L, p) of the case table runs in both column forms: t_dev = NULL with col = L, and
t_dev on the device with col = 1, *t_dev = L - 1.  Batch 8 takes the 8 histories of a combination in one call, batch 1
one call per history."""
import ctypes

import pytest
import torch

import repeat_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0
_DT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_tdev = {}


def _t(v):
    if v not in _tdev:
        _tdev[v] = torch.tensor([v], dtype=torch.int32, device=DEV)
    return _tdev[v]


@pytest.mark.parametrize("B", rc.BATCHES)
@pytest.mark.parametrize("dtype", rc.DTYPES, ids=lambda d: _DT[d])
@pytest.mark.parametrize("vocab", list(rc.VOCABS))
def test_repeat_process_matches_restatement(vocab, dtype, B):
    from tw import ops as F
    V, eos, ld = rc.VOCABS[vocab], rc.EOS[vocab], rc.ld_of(rc.VOCABS[vocab])
    x = rc.score_table(V, dtype)                                    # fp32 view of the dtype's values
    logits = torch.full((rc.ROWS, ld), float("nan"), dtype=dtype, device=DEV)
    logits[:, :V] = x.to(dtype).to(DEV)
    out = torch.empty(rc.ROWS, ld, dtype=torch.float32, device=DEV)
    bad = []
    touched = 0
    for n, L, p in rc.combos():
        hists = rc.histories(L, V, eos)
        want = rc.restate(x, hists, p, n).to(DEV)
        ids = rc.id_matrix(hists, L, V).to(DEV)
        touched += int(not rc.same_bits(want.cpu(), x))
        for tdev in (False, True):
            col, t = (1, _t(L - 1)) if tdev else (L, None)
            out.fill_(SENTINEL)
            if B == rc.ROWS:
                F.repeat_process(logits, ld, B, V, ids, col, out, p, n, t_dev=t)
            else:
                for r in range(rc.ROWS):
                    F.repeat_process(logits[r:], ld, 1, V, ids[r:], col, out[r:], p, n, t_dev=t)
            if not rc.same_bits(out[:, :V], want) or not bool((out[:, V:] == SENTINEL).all()):
                bad.append((n, L, p, tdev))
    assert not bad, bad[:10]
    assert touched > len(rc.combos()) // 2


def test_repeat_process_unaligned_rows_take_the_scalar_path():
    """ld == V (130: rows not 16-byte aligned) and an output one element into its buffer: same bits."""
    from tw import ops as F
    V, eos = rc.VOCABS["small"], rc.EOS["small"]
    for dtype in rc.DTYPES:
        x = rc.score_table(V, dtype)
        logits = x.to(dtype).to(DEV).contiguous()
        for n, L, p in ((2, 447, 1.3), (1, 5, 0.5), (0, 0, 1.0)):
            hists = rc.histories(L, V, eos)
            ids = rc.id_matrix(hists, L, V).to(DEV)
            flat = torch.full((rc.ROWS * V + 8,), SENTINEL, dtype=torch.float32, device=DEV)
            out = flat[1:1 + rc.ROWS * V].view(rc.ROWS, V)
            F.repeat_process(logits, V, rc.ROWS, V, ids, L, out, p, n)
            assert rc.same_bits(out, rc.restate(x, hists, p, n).to(DEV)), (dtype, n, L, p)
            assert float(flat[0]) == SENTINEL and bool((flat[1 + rc.ROWS * V:] == SENTINEL).all())


def test_repeat_process_bad_arguments_write_nothing():
    from tw import _native
    lib = _native.lib()
    V, ld, B = 130, 192, 2
    logits = torch.zeros(B, ld, dtype=torch.float32, device=DEV)
    ids = torch.zeros(B, 8, dtype=torch.int64, device=DEV)
    out = torch.full((B, ld), SENTINEL, dtype=torch.float32, device=DEV)

    def call(ld=ld, dt=0, B=B, V=V, col=4, penalty=1.3, ngram=2, ld_out=ld):
        return lib.tw_repeat_process(logits.data_ptr(), ld, dt, B, V, ids.data_ptr(), ids.stride(0), col, None,
                                     ctypes.c_float(penalty), ngram, out.data_ptr(), ld_out,
                                     torch.cuda.current_stream().cuda_stream)
    for kw in (dict(penalty=0.0), dict(penalty=-1.3), dict(penalty=float("nan")), dict(ngram=-1), dict(B=0),
               dict(B=-1), dict(V=0), dict(ld=V - 1), dict(ld_out=V - 1), dict(col=-1)):
        assert call(**kw) == 1, kw
    for dt in (3, -1, 7):
        assert call(dt=dt) == 2, dt
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == 0                                              # the same arguments, valid: it runs
    torch.cuda.synchronize()
    assert bool((out[:, :V] != SENTINEL).all()) and bool((out[:, V:] == SENTINEL).all())
