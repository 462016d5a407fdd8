"""Log-mel front end micro-bench: 64 clips of 30 s (the training micro-batch) at 80 and at 128 mel bins.

Each call (the DFT + mel kernel and the finalize kernel, mel_out and the bf16 conv input written) is timed with its own
pair of HIP events after a warm-up; the median over the repetitions is reported.  80 bins go through tw_logmel (the
entry every earlier build has), 128 bins through tw_logmel_mels.

  python tools/bench_logmel.py [--reps 50] [--warmup 5] [--lib /path/to/other/libtw_hip.so]

--lib times another build of the library on the same GPU in the same process order (an A/B control for the 80-bin
path: it runs the same instructions whichever way the kernel is templated); a library without tw_logmel_mels is timed
at 80 bins only.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tw import _native  # noqa: E402
from tw.data import synthetic_audio  # noqa: E402
from tw.feature_extraction import mel_tables  # noqa: E402

P, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def load(path):
    if path is None:
        return _native.lib()
    l = ctypes.CDLL(path)
    l.tw_logmel.argtypes, l.tw_logmel.restype = _native.SIGNATURES["tw_logmel"], I32
    if hasattr(l, "tw_logmel_mels"):
        l.tw_logmel_mels.argtypes, l.tw_logmel_mels.restype = _native.SIGNATURES["tw_logmel_mels"], I32
    return l


def run(l, wav, n_mels, reps, warmup):
    B, n = wav.shape
    dev = wav.device
    basis, start, w = mel_tables(dev, n_mels)
    mel = torch.empty(B, n_mels, n // 160, dtype=torch.float32, device=dev)
    conv = torch.empty(B, n // 160 + 2, n_mels, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        if n_mels == 80:
            rc = l.tw_logmel(wav.data_ptr(), B, basis.data_ptr(), start.data_ptr(), w.data_ptr(), mel.data_ptr(),
                             conv.data_ptr(), ws.data_ptr(), stream)
        else:
            rc = l.tw_logmel_mels(wav.data_ptr(), B, n, n_mels, basis.data_ptr(), start.data_ptr(), w.data_ptr(),
                                  mel.data_ptr(), conv.data_ptr(), ws.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"log-mel call failed with status {rc}")

    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return dict(n_mels=n_mels, median_us=statistics.median(us), min_us=us[0], p90_us=us[int(0.9 * (reps - 1))],
                checksum=float(mel.double().sum().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--lib", type=str, default=None)
    a = ap.parse_args()
    l = load(a.lib)
    wav = synthetic_audio(a.clips, device="cuda")
    for n_mels in (80, 128):
        if n_mels != 80 and not hasattr(l, "tw_logmel_mels"):
            continue
        r = run(l, wav, n_mels, a.reps, a.warmup)
        r.update(clips=a.clips, seconds=30, reps=a.reps, lib=a.lib or "in-tree")
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
