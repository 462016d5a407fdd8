"""Status codes of the eight 16-bit attention entries of csrc/attention.hip (tw_attn_{fwd,bwd}[_varlen][_f16]), called
through tw._native.call on one valid layout (B = 2, H = 3, Tq = Tk = 33, causal) with one argument perturbed per call.
The order of the entries' checks is behaviour: head_dim (2), then scale (1), then (packed) the row description (1),
then the empty call (0, nothing launched), then alignment (1), then (dense) causal with Tq > Tk (1).  No call of the
table launches a kernel: every output keeps its sentinel.  Only the control calls and the forward with ldo + 4 (a
legal leading dimension for the forward's 8-byte stores, not for the backward's 16-byte reads of O) launch; they run
last.

Three rows are stated more narrowly than "one argument", because the packed description is checked as a whole before
the empty call is recognised: Mq = 0 alone leaves max_q = 33 > Mq (1), the empty packing is Mq = max_q = 0 (forward
0; the backward would launch its dK / dV zero fill, so it is not in the table); Tk = 0 alone is causal with
max_q > Tk (1), and 0 without the causal flag.  A packed call with B = 0 is refused (1) where a dense one is empty (0).
"""
import re

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"

FWD = ("Q", "ldq", "K", "ldk", "V", "ldv", "O", "ldo", "lse")
BWD = FWD[:8] + ("dO", "lddo", "lse", "dQ", "lddq", "dK", "lddk", "dV", "lddv")
ORDER = {
    "tw_attn_fwd": FWD + ("B", "H", "Tq", "Tk", "head_dim", "causal", "scale", "stream"),
    "tw_attn_bwd": BWD + ("B", "H", "Tq", "Tk", "head_dim", "causal", "scale", "ws", "stream"),
    "tw_attn_fwd_varlen": FWD + ("offq", "offk", "B", "H", "Mq", "Tq", "Tk", "head_dim", "causal", "scale", "stream"),
    "tw_attn_bwd_varlen": BWD + ("offq", "offk", "B", "H", "Mq", "Tq", "Tk", "head_dim", "causal", "scale", "ws",
                                 "stream"),
}
DENSE, PACKED = ("tw_attn_fwd", "tw_attn_bwd"), ("tw_attn_fwd_varlen", "tw_attn_bwd_varlen")
FORWARD, BACKWARD = ("tw_attn_fwd", "tw_attn_fwd_varlen"), ("tw_attn_bwd", "tw_attn_bwd_varlen")
ALL = DENSE + PACKED

# (what, entries, the perturbed arguments (a callable of the valid ones), status); packed entries take max_q as "Tq"
TABLE = [
    ("head_dim 32", ALL, lambda a: dict(head_dim=32), 2),
    ("Q + one element", ALL, lambda a: dict(Q=a["Q"] + 2), 1),
    ("ldk + 4", ALL, lambda a: dict(ldk=a["ldk"] + 4), 1),
    ("ldo + 4, backward", BACKWARD, lambda a: dict(ldo=a["ldo"] + 4), 1),
    ("dO + one element", BACKWARD, lambda a: dict(dO=a["dO"] + 2), 1),
    ("causal, Tq = Tk + 1", ALL, lambda a: dict(Tq=a["Tk"] + 1), 1),
    ("B = 0, dense", DENSE, lambda a: dict(B=0), 0),
    ("B = 0, packed", PACKED, lambda a: dict(B=0), 1),
    ("null offq", PACKED, lambda a: dict(offq=None), 1),
    ("max_q = Mq + 1", PACKED, lambda a: dict(Tq=a["Mq"] + 1), 1),
    ("Mq = max_q = 0, forward", ("tw_attn_fwd_varlen",), lambda a: dict(Mq=0, Tq=0), 0),
    ("Mq = 0 alone", PACKED, lambda a: dict(Mq=0), 1),
    ("Tk = 0, not causal", PACKED, lambda a: dict(Tk=0, causal=0), 0),
    ("Tk = 0 alone (causal)", PACKED, lambda a: dict(Tk=0), 1),
    # precedence
    ("head_dim 32 and scale 0", ALL, lambda a: dict(head_dim=32, scale=0.0), 2),
    ("scale 0 and B = 0", ALL, lambda a: dict(scale=0.0, B=0), 1),
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _status(name, args):
    from tw import _native
    try:
        return _native.call(name, *args)
    except RuntimeError as e:
        return int(re.search(r"status (\d+)", str(e)).group(1))


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=lambda d: ac.DT_NAME[d])
def test_status_codes(dtype):
    c = ac.Case("rand", "a1", 2, 3, 33, 33, True, dtype, 1.0, 0)
    lay = ac.Layout(ac.build(c), DEV)
    off = torch.tensor([0, 33, 66], dtype=torch.int32, device=DEV)
    ws = torch.full((c.B * c.H * c.Tq,), ac.SENTINEL, dtype=torch.float32, device=DEV)
    valid = dict(Q=lay.q.data_ptr(), ldq=lay.ldq, K=lay.k.data_ptr(), ldk=lay.ldkv, V=lay.v.data_ptr(), ldv=lay.ldkv,
                 O=lay.o.data_ptr(), ldo=lay.ldo, lse=lay.lse.data_ptr(), dO=lay.do.data_ptr(), lddo=lay.d,
                 dQ=lay.dq.data_ptr(), lddq=lay.ldo, dK=lay.dk.data_ptr(), lddk=lay.lddkv, dV=lay.dv.data_ptr(),
                 lddv=lay.lddkv, offq=off.data_ptr(), offk=off.data_ptr(), B=c.B, H=c.H, Tq=c.Tq, Tk=c.Tk,
                 Mq=c.B * c.Tq, head_dim=ac.HD, causal=1, scale=ac.SCALE, ws=ws.data_ptr(),
                 stream=torch.cuda.current_stream().cuda_stream)
    suffix = "_f16" if dtype == torch.float16 else ""

    def run(entry, **over):
        a = dict(valid, **over)
        return _status(entry + suffix, [a[k] for k in ORDER[entry]])

    got = {(what, e): run(e, **over(valid)) for what, entries, over, _ in TABLE for e in entries}
    want = {(what, e): st for what, entries, _, st in TABLE for e in entries}
    torch.cuda.synchronize()
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert all(bool((t == ac.SENTINEL).all()) for t in lay.outputs().values()), "a refused or empty call launched"
    assert bool((ws == ac.SENTINEL).all()) and lay.guards_intact() == []
    # the calls that launch: the valid control of every entry, then the forward with ldo + 4
    for e in ALL:
        assert run(e) == 0, e
    torch.cuda.synchronize()
    assert lay.guards_intact() == []
    assert not any(bool((t == ac.SENTINEL).any()) for t in lay.outputs().values()), "the control calls wrote everything"
    for e in FORWARD:
        assert run(e, ldo=valid["ldo"] + 4) == 0, e
    torch.cuda.synchronize()
