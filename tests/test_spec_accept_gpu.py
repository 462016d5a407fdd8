"""tw_spec_accept (acceptance and rollback of one round of assisted decoding, on the device) against a few lines of
Python: handcrafted drafts and target tokens for k = 4 -- every n from 0 to 4, an eos inside the accepted run, an eos
as the first target token, a row already done, a round cut by the length cap -- checking the id row with its eos
refill, cur, both step counters, the finished flags, last_ts with and without timestamp tokens in the accepted run,
the summed log-prob (exactly the sequential fp32 sum) and the per-round history."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, TS0, K, P = 50257, 50364, 4, 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _reference(ids, t, drafts, t_cap, done0, slots, sum0):
    """The kernel's contract, restated."""
    ids = list(ids)
    n = 0
    for j in range(K):
        if ids[t + 1 + j] != drafts[j]:
            break
        n += 1
        if ids[t + 1 + j] == EOS:
            break
    frozen = bool(done0) or t + 1 >= t_cap
    adv = 0 if frozen else min(n + 1, t_cap - 1 - t)
    done = bool(done0) or any(x == EOS for x in ids[t + 1:t + adv + 1])
    for c in range(t + adv + 1, t + K + 2):
        ids[c] = EOS
    s = np.float32(sum0)
    for j in range(adv):
        s = np.float32(s + np.float32(slots[j]))
    last = -1
    for c in range(t + adv, P - 1, -1):
        if ids[c] >= TS0:
            last = ids[c]
            break
    return dict(n=n, frozen=frozen, ids=ids, t=t + adv, cur=ids[t + adv], done=int(done), sum=s, last_ts=last)


CASES = {
    # name: (generated so far, target tokens of the k + 1 positions, drafts, done before, t_cap)
    "n0": ([TS0, 11], [21, 22, 23, 24, 25], [99, 22, 23, 24], 0, 40),
    "n1": ([TS0, 11], [21, 22, 23, 24, 25], [21, 99, 23, 24], 0, 40),
    "n2": ([TS0, 11], [21, 22, 23, 24, 25], [21, 22, 99, 24], 0, 40),
    "n3_ts_inside": ([TS0, 11], [21, TS0 + 7, TS0 + 7, 24, 25], [21, TS0 + 7, TS0 + 7, 99], 0, 40),
    "n4": ([TS0, 11], [21, 22, 23, 24, 25], [21, 22, 23, 24], 0, 40),
    "no_ts_at_all": ([11, 12], [21, 22, 23, 24, 25], [21, 22, 23, 24], 0, 40),
    "ts_only_in_rejected": ([11, 12], [21, 22, TS0 + 3, 24, 25], [21, 99, TS0 + 3, 24], 0, 40),
    "eos_inside": ([TS0, 11], [21, EOS, EOS, EOS, EOS], [21, EOS, EOS, EOS], 0, 40),
    "eos_first": ([TS0, 11], [EOS, EOS, EOS, EOS, EOS], [EOS, EOS, EOS, EOS], 0, 40),
    "eos_first_rejected": ([TS0, 11], [EOS, EOS, EOS, EOS, EOS], [7, EOS, EOS, EOS], 0, 40),
    "already_done": ([TS0, 11, EOS], [EOS, EOS, EOS, EOS, EOS], [EOS, EOS, EOS, EOS], 1, 40),
    "cap_mid_round": ([TS0, 11], [21, 22, 23, 24, 25], [21, 22, 23, 24], 0, P + 2 + 3),
    "at_cap": ([TS0, 11], [21, 22, 23, 24, 25], [21, 22, 23, 24], 0, P + 2),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("track", [False, True])
def test_accept(name, track):
    from tw import ops
    gen, target, drafts, done0, t_cap = CASES[name]
    width = t_cap + K + 1
    row = [50258, 50260, 50359] + gen
    t = len(row) - 1
    row = row + target + [EOS] * (width - len(row) - len(target))
    # a second row around it: the kernel touches one row only
    ids = torch.tensor([[1] * width, row, [2] * width], dtype=torch.int64, device=DEV)
    slots = [-0.1234567, -1.7654321, -3.3e-4, -2.5, -0.75]
    sum0 = -4.4444444
    ref = _reference(row, t, drafts, t_cap, done0, slots, sum0)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
    u8 = lambda v: torch.tensor([v], dtype=torch.uint8, device=DEV)
    t_dev, t_dev_a = i32(t), i32(t + K + 1)                     # the assistant ran k + 1 steps ahead
    cur, cur_a = torch.tensor([row[t]], device=DEV), torch.tensor([drafts[-1]], device=DEV)
    # the flags as the round's launches leave them: polluted by rejected positions
    done, done_a, snap = u8(1), u8(1), u8(done0)
    last_ts, last_ts_a = i32(TS0 + 999), i32(TS0 + 998)
    sl = torch.tensor(slots, dtype=torch.float32, device=DEV) if track else None
    sm = torch.tensor([sum0], dtype=torch.float32, device=DEV) if track else None
    hist = torch.zeros(4, dtype=torch.int32, device=DEV)
    hist[0], hist[1] = 1, 9                                      # one earlier round on record
    ops.spec_accept(torch.tensor(drafts, device=DEV), K, ids[1], t_cap, EOS, t_dev, cur, done, snap, t_dev_a=t_dev_a,
                    cur_a=cur_a, done_a=done_a, last_ts=last_ts, last_ts_a=last_ts_a, begin_col=P, ts_begin=TS0,
                    slots=sl, sum_logp=sm, hist=hist)
    torch.cuda.synchronize()
    assert ids[1].tolist() == ref["ids"]
    assert ids[0].tolist() == [1] * width and ids[2].tolist() == [2] * width
    assert int(t_dev) == ref["t"] == int(t_dev_a)
    assert int(cur) == ref["cur"] == int(cur_a)
    assert int(done) == ref["done"] == int(done_a) == int(snap)
    assert int(last_ts) == ref["last_ts"] == int(last_ts_a)
    if track:
        assert np.float32(sm.item()) == ref["sum"]              # exactly the sequential fp32 additions
        assert sl.tolist() == [0.0] * (K + 1)
    if ref["frozen"]:
        assert hist.tolist() == [1, 9, 0, 0]
    else:
        assert hist.tolist() == [2, 9, ref["n"], 0]


def test_expected_counts():
    """The handcrafted cases do cover what they are named for."""
    want = {"n0": 0, "n1": 1, "n2": 2, "n3_ts_inside": 3, "n4": 4, "eos_inside": 2, "eos_first": 1,
            "eos_first_rejected": 0}
    for name, n in want.items():
        gen, target, drafts, done0, t_cap = CASES[name]
        row = [0] * P + gen + target + [EOS] * 8
        assert _reference(row, P + len(gen) - 1, drafts, t_cap, done0, [0.0] * 5, 0.0)["n"] == n, name
    r = _reference([0] * P + [TS0, 11] + [21, 22, 23, 24, 25] + [EOS] * 8, P + 1, [21, 22, 23, 24], P + 5, 0, [0.0] * 5, 0.0)
    assert r["t"] == P + 4 and r["n"] == 4                       # cut by the cap: 3 of the 5 tokens stand


def test_history_stops_at_capacity_and_invalid_k():
    from tw import ops
    ids = torch.full((1, 64), EOS, dtype=torch.int64, device=DEV)
    ids[0, :4] = torch.tensor([50258, 50260, 50359, 5])
    hist = torch.zeros(2, dtype=torch.int32, device=DEV)
    z8 = lambda: torch.zeros(1, dtype=torch.uint8, device=DEV)
    t_dev = torch.tensor([3], dtype=torch.int32, device=DEV)
    cur = torch.zeros(1, dtype=torch.int64, device=DEV)
    for _ in range(3):                                            # three live rounds, room for one entry
        ids[0, int(t_dev) + 1] = 9
        ops.spec_accept(torch.tensor([1, 1, 1, 1], device=DEV), K, ids[0], 40, EOS, t_dev, cur, z8(), z8(), hist=hist)
    assert hist.tolist() == [3, 0] and int(t_dev) == 6
    with pytest.raises((RuntimeError, AssertionError)):
        ops.spec_accept(torch.zeros(8, dtype=torch.int64, device=DEV), 8, ids[0], 40, EOS, t_dev, cur, z8(), z8())
