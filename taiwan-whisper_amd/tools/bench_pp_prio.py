"""Subtraction diagnostics of the persistent ping-pong GEMM (gemm_pp_kernel), interleaved in one process on random
data, forward shapes of the distillation step.  p4 is the kernel; every other variant gives wrong results.  p4e: the
epilogue without its stores; p4z: the epilogue stored into tile 0 (L2-resident stores, no HBM write traffic); these
two are meant for the diagnostic build of the library (make CXXFLAGS+=-DTW_PP_DIAG_VARIANTS), though their tests are
still compiled into the default build's epilogue (gemm.hip pp_epi_part says why).  p5e / p6e / p7e (the main loop
without the A-half-1 reads / without restaging / without counted waits, each without stores) and p4l, p4le (every
tile stages one block's panels per XCD: L2 hits) need the diagnostic build: the default build ignores their bits and
runs p4 / p4e.  The flag values are gemm_impl.h's F_DIAG_*.  (The round-2 four-phase variants p0 / p1 / p2x are gone with that schedule.)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from tw import ops

SHAPES = [("enc qkv", 96000, 3840, 1280, 0), ("enc out", 96000, 1280, 1280, 0), ("enc fc1", 96000, 5120, 1280, 1),
          ("enc fc2", 96000, 1280, 5120, 0), ("xattn kv", 96000, 2560, 1280, 0), ("dec fc1", 28608, 5120, 1280, 1),
          ("lm head", 28608, 51904, 1280, 0)]
VARIANTS = (sys.argv[1] if len(sys.argv) > 1 else "p4,p4e").split(",")
DT = torch.float16 if "fp16" in sys.argv[2:] else torch.bfloat16     # `... p4 fp16`: the fp16 instantiation
SKIP_STORES, STORE_TILE0, L2_PANELS, VARIANT_SHIFT = 4096, 1 << 20, 1 << 22, 15
FLAG = {"p4": 0, "p4e": SKIP_STORES, "p4z": STORE_TILE0, "p5e": (5 << VARIANT_SHIFT) | SKIP_STORES,
        "p6e": (6 << VARIANT_SHIFT) | SKIP_STORES, "p7e": (7 << VARIANT_SHIFT) | SKIP_STORES,
        "p4l": L2_PANELS, "p4le": L2_PANELS | SKIP_STORES}


def vflag(v):
    return ops.GEMM_TILE256PP | FLAG[v]


def main(rounds=5):
    dev = "cuda"
    for name, M, N, K, gelu in SHAPES:
        A = torch.randn(M, K, device=dev).to(DT)
        W = torch.randn(N, K, device=dev).to(DT)
        C = torch.empty(M, N, dtype=DT, device=dev)
        bias = torch.randn(N, device=dev).to(DT)
        base = ops.GEMM_ROUND

        def run(v):
            if gelu:
                ops.gemm(A, W, C, M, N, K, lda=K, ldb=K, ldc=N, bias=bias, flags=base | ops.GEMM_GELU | vflag(v))
            else:
                ops.gemm(A, W, C, M, N, K, lda=K, ldb=K, ldc=N, bias=bias, flags=base | vflag(v))
        outs = {}
        for v in VARIANTS:
            run(v)
            outs[v] = C.clone()
        same = all(torch.equal(outs[v], outs[VARIANTS[0]]) for v in VARIANTS if v == "p4")
        times = {v: [] for v in VARIANTS}
        for _ in range(rounds):
            for v in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    run(v)
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) / 3)
        fl = 2.0 * M * N * K
        line = f"{name:9s} M={M:6d} N={N:6d} K={K:5d} same={same} "
        for v in VARIANTS:
            t = sorted(times[v])[rounds // 2]
            line += f" {v}: {fl / t / 1e9:7.1f}TF"
        print(line, flush=True)
        del A, W, C, outs


if __name__ == "__main__":
    main()
