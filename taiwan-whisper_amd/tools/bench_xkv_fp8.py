"""The cross-attention read of a decode step, 16-bit against the 8-bit K/V cache (cross_kv_dtype="fp8_e4m3"), in one
process with the two sides alternating:

  * the kernel alone (tw_decode_attn / tw_decode_attn_fp8 as DecodeSession calls them: (clip, head) pairs as one-head
    clips over head-major [Tk][64] blocks) at Tk = 1500 and 20, 2560 and 10240 pairs (batch 1, 128, 512 at large-v2's
    20 heads): us per call and TB/s of the K/V bytes the call has to read (2 * pairs * Tk * 64 elements);
  * a whole graph-replayed DecodeSession step at batch 128 with large-v2 dimensions (fp16, random weights), both ways.

Each figure is the median of `rounds` alternating timings (device events around `reps` launches), with the spread
(min .. max) beside it; a difference counts when the two ranges do not overlap.  At 20 pairs the K/V (7.7 MB, 3.8 MB)
stays in the caches and the call is launch-bound: that row measures overheads.

    python tools/bench_xkv_fp8.py [rounds] [--no-step] [--dtype=fp16|bf16]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch

from tw import ops as F

DEV = "cuda"
TK = 1500


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def _ab(fa, fb, reps, rounds):
    """Alternating timings of fa and fb -> ((median, min, max) of fa, the same of fb), us."""
    for f in (fa, fb):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(_time(fa, reps))
        tb.append(_time(fb, reps))
    st = lambda t: (sorted(t)[len(t) // 2], min(t), max(t))
    return st(ta), st(tb)


def _verdict(a, b):
    if b[2] < a[1]:
        return f"fp8 faster, x{a[0] / b[0]:.2f} (ranges apart)"
    if a[2] < b[1]:
        return f"fp8 SLOWER, x{a[0] / b[0]:.2f} (ranges apart)"
    return f"no difference beyond the spread (x{a[0] / b[0]:.2f})"


def kernels(dt, rounds):
    for pairs in (20, 2560, 10240):
        n = pairs * TK * 64
        g = torch.Generator(device=DEV).manual_seed(pairs)
        q = torch.randn(pairs, 64, device=DEV, generator=g).to(dt)
        kv16 = (torch.randn(2 * n, device=DEV, generator=g) * 0.5).to(dt)
        kv8 = torch.randint(0, 0x40, (2 * n,), device=DEV, generator=g, dtype=torch.uint8)     # e4m3 bytes below 2.0
        sc = torch.ones(2 * pairs, dtype=torch.float32, device=DEV)
        o16, o8 = torch.empty_like(q), torch.empty_like(q)
        f16 = lambda: F.decode_attn(q, 64, kv16, 64, TK * 64, kv16[n:], 64, TK * 64, o16, 64, pairs, 1, TK, 0.125)
        f8 = lambda: F.decode_attn_fp8(q, 64, kv8, 64, TK * 64, kv8[n:], 64, TK * 64, sc, sc[pairs:], 1, o8, 64,
                                       pairs, 1, TK, 0.125)
        reps = 200 if pairs == 20 else 20
        a, b = _ab(f16, f8, reps, rounds)
        for name, t, bytes_ in (("16-bit", a, 2 * n * 2), ("fp8   ", b, 2 * n)):
            print(f"attn  pairs {pairs:6d} {name}  {t[0]:8.1f} us  ({t[1]:.1f} .. {t[2]:.1f})  "
                  f"{bytes_ / t[0] / 1e6:6.2f} TB/s of {bytes_ / 1e6:.1f} MB K/V", flush=True)
        print(f"attn  pairs {pairs:6d} -> {_verdict(a, b)}", flush=True)
        del kv16, kv8


def step(dt, rounds, B=128):
    from oracle.weights import CONFIGS
    from tw.config import WhisperConfig
    from tw.generation import DecodeSession
    from tw.modeling import WhisperForConditionalGeneration, random_init_
    cfg = WhisperConfig(**CONFIGS["large-v2"])
    m = random_init_(WhisperForConditionalGeneration(cfg, dtype=dt, device=DEV), seed=0)
    Tk, d = cfg.max_source_positions, cfg.d_model
    enc = (torch.randn(B * Tk, d, device=DEV) * 0.5).to(dt)
    graphs, sess = {}, {}
    for name, fmt in (("16-bit", None), ("fp8   ", "fp8_e4m3")):
        m.cross_kv_dtype = fmt
        s = sess[name] = DecodeSession(m, enc, B, Tk, 256)
        s.t_dev.fill_(100)
        s.cur.fill_(50364)
        s.step()
        torch.cuda.synchronize()
        g = graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s.step()
            F.step_advance(s.t_dev, -1)              # every replay decodes position 100 again
        mb = sum(t.numel() * t.element_size() for t in s.cross_kv) / B / 1e6
        print(f"step  {name} cross K/V {mb:.1f} MB per clip", flush=True)
    m.cross_kv_dtype = None
    a, b = _ab(graphs["16-bit"].replay, graphs["fp8   "].replay, 10, rounds)
    for name, t in (("16-bit", a), ("fp8   ", b)):
        print(f"step  large-v2 {str(dt).split('.')[-1]} batch {B} at t=100 {name}  {t[0] / 1e3:8.3f} ms/step  "
              f"({t[1] / 1e3:.3f} .. {t[2] / 1e3:.3f})", flush=True)
    print(f"step  -> {_verdict(a, b)}", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    dt = torch.bfloat16 if "--dtype=bf16" in sys.argv else torch.float16
    rounds = int(args[0]) if args else 7
    kernels(dt, rounds)
    if "--no-step" not in sys.argv:
        step(dt, rounds)
