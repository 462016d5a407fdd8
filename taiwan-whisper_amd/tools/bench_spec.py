"""Assisted decoding in isolation, at large-v2 target dims with a distil-32-2 assistant (random weights), fp16 and
bf16, every timing from a captured graph: ms per plain target step, ms per verify pass (DecodeSession.step_multi)
at Q = 2..8, ms per assistant step, the break-even number of accepted drafts per round these imply, and the
achieved bytes/s of tw_decode_attn_mq on the cross-attention shape against the single-query kernel launched Q times.

Random weights accept almost nothing, so an end-to-end speed-up is NOT measured here: the break-even column says how
many drafts per round a real assistant would have to get accepted for a round of k drafts to beat k + 1 plain steps.

    python tools/bench_spec.py [reps]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch

from tw import ops as F


def _time(g, reps):
    """ms per replay: median of 5 timings of `reps` replays (after one warm replay)."""
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return sorted(ts)[2]


def _graph(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def _model(name, h):
    from oracle.weights import CONFIGS
    from tw.config import WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration, random_init_
    cfg = WhisperConfig(**CONFIGS[name])
    return random_init_(WhisperForConditionalGeneration(cfg, dtype=h, device="cuda"), seed=1)


def steps(h, reps):
    from tw.generation import DecodeSession
    dev, d, Tk = "cuda", 1280, 1500
    tag = "fp16" if h == torch.float16 else "bf16"
    enc = (torch.randn(Tk, d, device=dev) * 0.5).to(h)
    m = _model("large-v2", h)
    sess = DecodeSession(m, enc, 1, Tk, 256, spare=8)
    sess.cur.fill_(50364)

    def plain():
        sess.t_dev.fill_(100)
        sess.step()
    t_plain = _time(_graph(plain), reps)
    print(f"{tag} target   plain step at t=100            {t_plain:7.3f} ms", flush=True)
    verify = {}
    for Q in range(2, 9):
        ids = torch.full((Q,), 50364, dtype=torch.int64, device=dev)

        def multi():
            sess.t_dev.fill_(100)
            sess.step_multi(Q, ids)
        verify[Q] = _time(_graph(multi), reps)
        print(f"{tag} target   verify pass Q={Q} at t=100      {verify[Q]:7.3f} ms  ({verify[Q] / t_plain:4.2f} plain steps)",
              flush=True)
    del sess, m
    a = _model("distil-32-2", h)
    sa = DecodeSession(a, enc, 1, Tk, 256, spare=8)
    sa.cur.fill_(50364)

    def draft():
        sa.t_dev.fill_(100)
        sa.step()
    t_a = _time(_graph(draft), reps)

    def fill():
        sa.t_dev.fill_(100)
        sa.step(head=False)
    t_f = _time(_graph(fill), reps)
    print(f"{tag} assistant distil-32-2 step              {t_a:7.3f} ms   cache-fill step (no LM head) {t_f:7.3f} ms",
          flush=True)
    # a round of k drafts costs k assistant steps + one cache-fill step + the verify pass at Q = k + 1 and yields
    # n + 1 tokens when n drafts are accepted; the plain decode yields one token per t_plain
    for k in range(1, 8):
        cost = k * t_a + t_f + verify[k + 1]
        need = cost / t_plain - 1.0
        print(f"{tag} round k={k}: {cost:7.3f} ms = {cost / t_plain:4.2f} plain steps -> break-even at {need:4.2f} accepted "
              f"drafts per round{' (out of reach)' if need > k else ''}", flush=True)
    del sa, a


def cross_attn(h, reps):
    """tw_decode_attn_mq over one clip's head-major K/V (H = 20, Tk = 1500) vs Q single-query launches; bytes = the
    K and V elements, counted once per launch that reads them."""
    dev, H, Tk = "cuda", 20, 1500
    d = H * 64
    tag = "fp16" if h == torch.float16 else "bf16"
    kv = (torch.randn(2 * H * Tk * 64, device=dev) * 0.5).to(h)
    n1 = H * Tk * 64
    once = 2 * n1 * kv.element_size()
    for Q in (1, 2, 4, 5, 8):
        q = (torch.randn(Q, d, device=dev) * 0.5).to(h)
        o = torch.empty(Q, d, dtype=h, device=dev)
        o1 = torch.empty(Q, d, dtype=h, device=dev)

        def mq():
            for _ in range(16):
                F.decode_attn_mq(q, Q * d, d, kv, 64, 0, kv[n1:], 64, 0, o, Q * d, d, 1, H, Q, Tk, 0.125,
                                 hsk=Tk * 64, hsv=Tk * 64)

        def single():
            for _ in range(16):
                for j in range(Q):
                    F.decode_attn(q[j:j + 1], d, kv, 64, 0, kv[n1:], 64, 0, o1[j:j + 1], d, 1, H, Tk, 0.125,
                                  hsk=Tk * 64, hsv=Tk * 64)
        t_mq = _time(_graph(mq), reps) / 16 * 1e3
        t_1 = _time(_graph(single), reps) / 16 * 1e3
        same = torch.equal(o.view(torch.int16), o1.view(torch.int16))
        print(f"{tag} cross attn Q={Q}: mq {t_mq:7.2f} us ({once / t_mq / 1e3:7.1f} GB/s of K/V read once)   "
              f"{Q} single launches {t_1:7.2f} us ({Q * once / t_1 / 1e3:7.1f} GB/s of K/V read {Q} times)   "
              f"bit-identical {same}", flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    torch.manual_seed(0)
    for h in (torch.float16, torch.bfloat16):
        cross_attn(h, reps)
        steps(h, reps)
