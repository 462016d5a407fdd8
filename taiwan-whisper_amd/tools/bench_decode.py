"""Config c4 throughput: large-v2 batched greedy decode, random-init bf16 weights,
synthetic 30 s features; eos is suppressed so every clip runs exactly --new-tokens steps
(deterministic work, as §8d prescribes: max_new_tokens 224).

    python tools/bench_decode.py [--batch 64] [--new-tokens 224] [--clips 128] [--eager] [--dtype float16]
                                 [--repetition_penalty 1.3] [--no_repeat_ngram_size 3]
                                 [--language zh | auto | zh,en,...] [--runs 5] [--detect]
                                 [--return_token_logprobs] [--decode_weight_dtype fp8_e4m3]
--language auto detects every clip's language (generate(language="auto")); a comma list names one language per clip
(repeated to the batch).  --runs N times N calls and prints each; --detect times detect_language alone instead.
--return_token_logprobs decodes with generate(return_token_logprobs=True) (the tracking selectors' _lp entries).
--decode_weight_dtype fp8_e4m3 decodes over 8-bit decoder weights (model.decode_weight_dtype; tw_gemv_w8_* at batch <= 8).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--new-tokens", type=int, default=224)
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--config", default="large-v2")
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16"])
    ap.add_argument("--repetition_penalty", type=float, default=1.0)
    ap.add_argument("--no_repeat_ngram_size", type=int, default=0)
    ap.add_argument("--language", default="zh", help="a language, 'auto', or a comma list (one per clip, cycled)")
    ap.add_argument("--runs", type=int, default=0, help="time this many single calls and print each (ms)")
    ap.add_argument("--detect", action="store_true", help="time detect_language alone (with --runs)")
    ap.add_argument("--return_token_logprobs", action="store_true",
                    help="generate(return_token_logprobs=True): per-token log-probs beside the ids")
    ap.add_argument("--decode_weight_dtype", default="auto", choices=["auto", "fp8_e4m3"],
                    help="model.decode_weight_dtype: the decode step's Linear weights as e4m3 bytes with row scales")
    ap.add_argument("--longform-seconds", type=float, default=0.0,
                    help="config c5: one input of this many seconds, return_timestamps, --new-tokens per window")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from oracle.weights import CONFIGS
    from tw.config import GenerationConfig, WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration, random_init_
    cfg = WhisperConfig(**CONFIGS[a.config])
    m = WhisperForConditionalGeneration(cfg, dtype=getattr(torch, a.dtype))
    if a.dtype == "float16":
        m.set_compute("fp16")
    random_init_(m, seed=0)
    m.decode_weight_dtype = a.decode_weight_dtype
    m.generation_config = GenerationConfig(suppress_tokens=[50257], begin_suppress_tokens=[220, 50257],
                                           lang_to_id={"<|zh|>": 50260})
    if a.language != "zh":      # large-v2's 99 language ids, so that detection has its real table
        names = ["en", "zh"] + [f"l{i}" for i in range(2, 99)]
        m.generation_config["lang_to_id"] = {f"<|{c}|>": 50259 + i for i, c in enumerate(names)}

    def lang(n):
        names = a.language.split(",")
        return a.language if len(names) == 1 else [names[i % len(names)] for i in range(n)]
    if a.longform_seconds > 0:
        T = int(a.longform_seconds * 100)
        lf = torch.randn(1, 80, T, device="cuda") * 0.3
        trace = []
        m.generate(lf[:, :, :3500], return_timestamps=True, language=lang(1), task="transcribe", max_new_tokens=8,
                   use_graph=not a.eager)                                                     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(lf, return_timestamps=True, language=lang(1), task="transcribe", max_new_tokens=a.new_tokens,
                         use_graph=not a.eager, _trace=trace)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = sum(len(t["raw"]) for t in trace)
        print(f"c5 long-form {a.config}: {a.longform_seconds:.0f} s audio, {len(trace)} windows, {steps} decode steps, "
              f"{out.shape[1]} output tokens: {dt:.2f} s wall ({a.longform_seconds / dt:.1f}x real time, "
              f"{dt / max(steps, 1) * 1e3:.2f} ms/step at batch 1)", flush=True)
        return
    rep = dict(repetition_penalty=a.repetition_penalty, no_repeat_ngram_size=a.no_repeat_ngram_size)
    if a.return_token_logprobs:
        rep["return_token_logprobs"] = True
    feats = torch.randn(a.batch, 80, 3000, device="cuda") * 0.3
    m.generate(feats[:2], language=lang(2), task="transcribe", max_new_tokens=4, use_graph=not a.eager, **rep)  # warm-up
    torch.cuda.synchronize()
    if a.runs > 0:
        def one():
            if a.detect:
                return m.detect_language(feats)
            return m.generate(feats, language=lang(a.batch), task="transcribe", max_new_tokens=a.new_tokens,
                              use_graph=not a.eager, **rep)
        one()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            one()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        what = "detect_language" if a.detect else (f"generate language={a.language} {a.new_tokens} tokens"
                                                   f"{' token_logprobs' if a.return_token_logprobs else ''}")
        per = "" if a.detect else f", median {sorted(ms)[len(ms) // 2] / a.new_tokens:.3f} ms/step"
        what += "" if a.decode_weight_dtype == "auto" else f" weights {a.decode_weight_dtype}"
        print(f"{what} {a.config} {a.dtype} batch {a.batch}: per call ms {' '.join(f'{x:.2f}' for x in ms)} "
              f"(min {min(ms):.2f}, median {sorted(ms)[len(ms) // 2]:.2f}, max {max(ms):.2f}{per})", flush=True)
        return
    n_sub = max(1, a.clips // a.batch)
    t0 = time.perf_counter()
    for _ in range(n_sub):
        out = m.generate(feats, language=lang(a.batch), task="transcribe", max_new_tokens=a.new_tokens,
                         use_graph=not a.eager, **rep)
        out = out[0] if a.return_token_logprobs else out
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    clips = n_sub * a.batch
    print(f"c4 greedy {a.config} {a.dtype} penalty {a.repetition_penalty} ngram {a.no_repeat_ngram_size}"
          f"{' token_logprobs' if a.return_token_logprobs else ''}: "
          f"{clips} clips x {out.shape[1]} tokens, batch {a.batch}: {dt:.2f} s "
          f"-> {clips / dt:.2f} clips/s, {dt / n_sub / a.new_tokens * 1e3:.2f} ms/step "
          f"({'eager' if a.eager else 'graph'})", flush=True)


if __name__ == "__main__":
    main()
