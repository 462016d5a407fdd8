"""Generate tests/golden/repeat.npz: HF Transformers 5.15 fp32 on the CPU, generate(repetition_penalty=,
no_repeat_ngram_size=) on the micro model and inputs of the prompted fixtures (make_golden_prompted.py).

Run in the build container (it needs HF Transformers):   python tests/golden/make_golden_repeat.py

Cases (tests/repeat_inputs.py holds their settings):
  rp, ng, both_prompt, ts   short-form greedy: the penalty alone, the n-gram size alone, both with prompt_ids, both
                            with timestamps -> {tag}_ids
  cond3                     3 recordings in one long-form call, condition_on_prev_tokens, both options: the rows'
                            prompts differ in length and are left-padded
  lf1                       one 65 s recording (3 windows), timestamps, both options, condition_on_prev_tokens and a fallback
                            schedule every window passes at temperature 0
The long-form cases store what make_golden_prompted.store stores per decoded window (_win_b, _win_seek, _win_ids,
_win_prompt, _win_plen, _win_margin, _win_avg, _win_ns).

Asserted before anything is written: (a) every case's ids differ from the same call without the two options; (b) at
every generated step of every case HF's best processed score leads the second best by more than
repeat_inputs.TIE_MARGIN; (c) lf1 took no fallback (one attempt per window, at temperature 0)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import CONFIGS, _MarginSpy, hf_model, logmel, make_weights, ts_generation_config  # noqa: E402
from make_golden_prompted import run_longform, store  # noqa: E402

from prompted_inputs import PROMPT_IDS, conditioned_features  # noqa: E402
from repeat_inputs import LONG, LONG_INPUTS, OPTION_KEYS, SHORT, TIE_MARGIN  # noqa: E402


def _model():
    cfg = CONFIGS["micro"]
    m = hf_model(cfg, make_weights(cfg, 1, lin_std=0.2)).eval()
    m.generation_config = ts_generation_config()
    return m


def _without(kw):
    return {k: v for k, v in kw.items() if k not in OPTION_KEYS}


def _differs(a, b):
    n = min(a.shape[1], b.shape[1])
    return a.shape != b.shape or bool((a[:, :n] != b[:, :n]).any())


def gen_short(out):
    from transformers.generation.logits_process import LogitsProcessorList
    clips = [logmel.synthetic_clip(0), logmel.synthetic_clip(2, 9.0), logmel.synthetic_clip(4, 25.0)]
    feats = torch.from_numpy(logmel.log_mel_batch(clips))
    for tag, (n, kw, prompted) in SHORT.items():
        extra = dict(prompt_ids=torch.tensor(PROMPT_IDS)) if prompted else {}
        m = _model()
        eos = m.generation_config.eos_token_id
        spy = _MarginSpy()
        with torch.no_grad():
            ids = m.generate(feats[:n], logits_processor=LogitsProcessorList([spy]), **kw, **extra).numpy()
            m.generation_config = ts_generation_config()
            plain = m.generate(feats[:n], **_without(kw), **extra).numpy()
        assert _differs(ids, plain), f"(a) {tag}: the options change nothing"
        # (b) per row, the steps up to and including its first eos (HF pads a finished row; those steps decide nothing)
        worst = np.inf
        for r, row in enumerate(ids.tolist()):
            steps = row.index(eos) + 1 if eos in row else len(row)
            assert steps <= len(spy.steps), (tag, steps, len(spy.steps))
            worst = min([worst] + [float(spy.steps[t][r]) for t in range(steps)])
        assert worst > TIE_MARGIN, f"(b) {tag}: a step's top-2 margin is {worst}"
        out[f"{tag}_ids"] = ids
        print(tag, ids.shape, "min margin", worst, flush=True)


def gen_long(out):
    for tag, kw in LONG.items():
        lens, seed = LONG_INPUTS[tag]
        feats, mask = conditioned_features(lens=lens, seed=seed)
        ids, rec = run_longform(_model(), feats, mask, **kw)
        plain, _ = run_longform(_model(), feats, mask, **_without(kw))
        assert _differs(ids, plain), f"(a) {tag}: the options change nothing"
        worst = min(min(r) for r in rec["margin"])
        assert worst > TIE_MARGIN, f"(b) {tag}: a step's top-2 margin is {worst}"
        wins = list(zip(rec["b"], rec["seek"]))
        if isinstance(kw["temperature"], tuple):
            assert len(wins) == len(set(wins)) >= 2, f"(c) {tag}: a window was decoded again (fallback): {wins}"
        if tag == "cond3":
            assert any(len(p) < pl for p, pl in zip(rec["prompt"], rec["plen"])), "cond3: no left-padded row"
        store(out, tag, ids, rec)


def main():
    path = os.path.join(HERE, "repeat.npz")
    out = {}
    gen_short(out)
    gen_long(out)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
