"""Generate tests/golden/prompted.npz: HF Transformers 5.15 fp32 on the CPU, decoder prompts.

Run in the build container (it needs HF Transformers):   python tests/golden/make_golden_prompted.py
PROMPTED_CASES=short,pl,cond,lv2 selects the parts (the others are kept from the existing file).

  short  `generate(prompt_ids=...)` short-form on the greedy / beam fixtures' micro model and clips
           pa_ids      greedy, no timestamps, language zh, max_length 64 (the unprompted call is greedy.npz)
           pa_ts_ids   greedy, return_timestamps, max_new_tokens 48 (the unprompted call is greedy_ts.npz ts_short_ids)
           pb_ids      num_beams 2, no timestamps, max_length 64
  pl     long-form, the 3 recordings of batched_longform_features in ONE call with prompt_ids
  cond   long-form, the 3 recordings of prompted_inputs.conditioned_features in one call with
         condition_on_prev_tokens=True: `cond0` at temperature 0.0, `condf` with fallback.npz's schedule (temperature
         (0.0,), thresholds that never fire)
  lv2    `condf` at the large-v2 dims of batched_longform.npz (same weights seed) on 2 recordings: candidates
         LV2_PICK of prompted_inputs.LV2_CANDIDATES.  With those weights HF cuts the first window of every
         default-scale Gaussian recording at the same timestamp (equal prompts in every iteration), so the inputs were
         searched: `lv2search` decodes all candidates in one call and prints each iteration's prompt lengths (the
         result is recorded beside LV2_PICK).

Every long-form part stores the call's output ({tag}_ids) and, per decoded window in HF's order (seek iteration, then
batch row): _win_b (recording), _win_seek, _win_ids (the tokens HF's gate saw, -1-padded), _win_prompt (the row's
decoder_input_ids without its left padding, -1-padded), _win_plen (the padded prompt length of its iteration),
_win_margin (per step top-1 minus top-2 processed score, nan-padded) and, with thresholds, _win_avg / _win_ns.
Only token ids, seeks and prompts are stored; the weights are regenerated from seeds.

The conditions the tests rely on are asserted here, on the recorded trace, before the file is written.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import (CONFIGS, SPECIAL, SUPPRESS, _MarginSpy, batched_longform_features, hf_model,  # noqa: E402
                         logmel, make_weights, ts_generation_config)

from prompted_inputs import PROMPT_IDS, conditioned_features  # noqa: E402

assert PROMPT_IDS[0] == SPECIAL["startofprev"] and not set(PROMPT_IDS[1:]) & set(SUPPRESS)


def _pad2(rows, fill, dtype):
    n = max(len(r) for r in rows)
    return np.array([list(r) + [fill] * (n - len(r)) for r in rows], dtype=dtype)


def run_longform(m, feats, mask, **kw):
    """One HF long-form generate call with every decoded window recorded."""
    from transformers.generation.logits_process import LogitsProcessorList, WhisperNoSpeechDetection
    cls = type(m)
    orig_need, orig_gwf = cls._need_fallback, cls.generate_with_fallback
    pad = m.generation_config.pad_token_id
    rec = {"b": [], "seek": [], "ids": [], "prompt": [], "plen": [], "avg": [], "ns": [], "margin": []}
    it = {}
    spy = _MarginSpy()

    def gwf_spy(self, *a, **k):
        it["map"], it["seek"], it["start"] = list(k["batch_idx_map"]), k["seek"].clone(), len(spy.steps)
        it["dec"] = k["decoder_input_ids"].clone()
        return orig_gwf(self, *a, **k)

    def need_spy(self, seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size,
                 temperature):
        b = it["map"][index]
        row = it["dec"][index].tolist()
        npad = 0
        while row[npad] == pad:
            npad += 1
        rec["b"].append(b)
        rec["seek"].append(int(it["seek"][b]))
        rec["ids"].append([int(t) for t in seek_sequence.tolist()])
        rec["prompt"].append(row[npad:])
        rec["plen"].append(len(row))
        if isinstance(seek_outputs[index], dict):          # with thresholds: the per-step scores are kept
            scores = seek_outputs[index]["scores"]
            rec["avg"].append(float(self._retrieve_avg_logprobs(scores, seek_sequence, temperature)))
        else:
            scores = seek_sequence
        for p_ in logits_processor or []:
            if isinstance(p_, WhisperNoSpeechDetection):
                rec["ns"].append(float(p_.no_speech_prob[index]))
        steps = spy.steps[it["start"]:]
        rec["margin"].append([float(s_[index]) for s_ in steps[:len(scores)]])
        return orig_need(self, seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size,
                         temperature)
    cls._need_fallback, cls.generate_with_fallback = need_spy, gwf_spy
    try:
        with torch.no_grad():
            ids = m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), return_timestamps=True,
                             language="zh", task="transcribe", logits_processor=LogitsProcessorList([spy]),
                             **kw).numpy()
    finally:
        cls._need_fallback, cls.generate_with_fallback = orig_need, orig_gwf
    return ids, rec


def store(out, tag, ids, rec):
    out[f"{tag}_ids"] = ids
    out[f"{tag}_win_b"] = np.array(rec["b"], dtype=np.int64)
    out[f"{tag}_win_seek"] = np.array(rec["seek"], dtype=np.int64)
    out[f"{tag}_win_ids"] = _pad2(rec["ids"], -1, np.int64)
    out[f"{tag}_win_prompt"] = _pad2(rec["prompt"], -1, np.int64)
    out[f"{tag}_win_plen"] = np.array(rec["plen"], dtype=np.int64)
    out[f"{tag}_win_margin"] = _pad2(rec["margin"], np.nan, np.float32)
    if rec["avg"]:
        out[f"{tag}_win_avg"] = np.array(rec["avg"], dtype=np.float64)
    if rec["ns"]:
        out[f"{tag}_win_ns"] = np.array(rec["ns"], dtype=np.float64)
    print(tag, "windows", list(zip(rec["b"], rec["seek"], [len(p) for p in rec["prompt"]], rec["plen"],
                                   [len(i) for i in rec["ids"]])), "min margin",
          min(min(r) for r in rec["margin"]), flush=True)


def check_conditioned(rec, cut_off, n_task):
    """The conditions tests/test_prompted_gpu.py asserts again from the fixture."""
    by_level, cur, seen = [], [], set()
    for b, p in zip(rec["b"], rec["prompt"]):
        if b in seen:
            by_level.append(cur)
            cur, seen = [], set()
        seen.add(b)
        cur.append(len(p))
    by_level.append(cur)
    assert any(len(set(lv)) > 1 for lv in by_level), "no level with rows whose prompts differ in length"
    assert any(len(p) > n_task + 1 for p in rec["prompt"]), "no row with previous text"
    assert any(len(p) == 1 + cut_off + n_task for p in rec["prompt"]), "no prompt cut at max_target_positions//2 - 1"


def gen_short(out):
    cfg = CONFIGS["micro"]
    m = hf_model(cfg, make_weights(cfg, 1, lin_std=0.2)).eval()
    clips3 = [logmel.synthetic_clip(0), logmel.synthetic_clip(2, 9.0), logmel.synthetic_clip(4, 25.0)]
    f3 = torch.from_numpy(logmel.log_mel_batch(clips3))
    f2 = torch.from_numpy(logmel.log_mel_batch(clips3[:2]))
    pid = torch.tensor(PROMPT_IDS)
    calls = {"n": 0}
    cls = type(m)
    orig = cls.generate_with_fallback

    def count(self, *a, **k):
        calls["n"] += 1
        return orig(self, *a, **k)
    cls.generate_with_fallback = count
    try:
        with torch.no_grad():
            m.generation_config = ts_generation_config()
            calls["n"] = 0
            out["pa_ids"] = m.generate(f3, prompt_ids=pid, language="zh", task="transcribe", max_length=64).numpy()
            na = calls["n"]
            # the same call without the prompt is greedy.npz
            un = m.generate(f3, language="zh", task="transcribe", max_length=64).numpy()
            m.generation_config = ts_generation_config()
            out["pa_ts_ids"] = m.generate(f2, prompt_ids=pid, return_timestamps=True, language="zh", task="transcribe",
                                          max_new_tokens=48).numpy()
            m.generation_config = ts_generation_config()
            calls["n"] = 0
            out["pb_ids"] = m.generate(f3, prompt_ids=pid, language="zh", task="transcribe", max_length=64,
                                       num_beams=2).numpy()
            nb = calls["n"]
    finally:
        cls.generate_with_fallback = orig
    assert na == 1 and nb == 1, ("a no-timestamp call decoded more than one window", na, nb)
    g = np.load(os.path.join(HERE, "greedy.npz"))["greedy_ids"]
    n = min(g.shape[1], un.shape[1])
    assert (g[:, :n] == un[:, :n]).all(), "the unprompted call is not greedy.npz"
    n = min(g.shape[1], out["pa_ids"].shape[1])
    assert (g[:, :n] != out["pa_ids"][:, :n]).any(), "the prompt changes nothing (no timestamps)"
    gt = np.load(os.path.join(HERE, "greedy_ts.npz"))["ts_short_ids"]
    n = min(gt.shape[1], out["pa_ts_ids"].shape[1])
    assert (gt[:, :n] != out["pa_ts_ids"][:, :n]).any(), "the prompt changes nothing (timestamps)"
    out["prompt_ids"] = np.array(PROMPT_IDS, dtype=np.int64)
    print("short", out["pa_ids"].shape, out["pa_ts_ids"].shape, out["pb_ids"].shape, flush=True)


def gen_pl(out):
    cfg = CONFIGS["micro"]
    m = hf_model(cfg, make_weights(cfg, 1, lin_std=0.2)).eval()
    m.generation_config = ts_generation_config()
    feats, mask = batched_longform_features()
    ids, rec = run_longform(m, feats, mask, prompt_ids=torch.tensor(PROMPT_IDS), temperature=(0.0,),
                            logprob_threshold=-1e9, no_speech_threshold=1.0)
    store(out, "pl", ids, rec)


def gen_cond(out):
    cfg = CONFIGS["micro"]
    feats, mask = conditioned_features()
    for tag, kw in (("cond0", dict(temperature=0.0)),
                    ("condf", dict(temperature=(0.0,), logprob_threshold=-1e9, no_speech_threshold=1.0))):
        m = hf_model(cfg, make_weights(cfg, 1, lin_std=0.2)).eval()
        m.generation_config = ts_generation_config()
        ids, rec = run_longform(m, feats, mask, condition_on_prev_tokens=True, **kw)
        store(out, tag, ids, rec)
        check_conditioned(rec, cfg["max_target_positions"] // 2 - 1, 3)


def _lv2_model():
    from make_golden import lv2_decode_weights
    cfg = CONFIGS["large-v2"]
    lv2 = np.load(os.path.join(HERE, "lv2_decode.npz"))
    m = hf_model(cfg, lv2_decode_weights(cfg, int(lv2["seed"]), lv2["v_bias"])).eval()
    m.generation_config = ts_generation_config()
    return cfg, m


class _Enough(Exception):
    pass


def search_lv2(out):
    """PROMPTED_CASES=lv2search: every candidate recording of prompted_inputs.LV2_CANDIDATES in ONE conditioned HF call
    at the large-v2 dims, stopped once the prompts of the first PROMPTED_LV2_LEVELS (3) seek iterations are known;
    prints, per iteration, each row's recording, seek and unpadded prompt length.  Two candidates whose prompts differ
    in length in one iteration can make the fixture (LV2_PICK)."""
    from prompted_inputs import LV2_CANDIDATES, lv2_candidate_features
    cfg, m = _lv2_model()
    feats, mask = lv2_candidate_features(list(range(len(LV2_CANDIDATES))))
    cls = type(m)
    orig = cls.generate_with_fallback
    pad = m.generation_config.pad_token_id
    levels = []
    stop = int(os.environ.get("PROMPTED_LV2_LEVELS", "3"))

    def spy(self, *a, **k):
        rows = k["decoder_input_ids"].tolist()
        levels.append([(b, int(k["seek"][b]), len(r) - next(i for i, t in enumerate(r) if t != pad))
                       for b, r in zip(k["batch_idx_map"], rows)])
        print("lv2search iteration", len(levels), levels[-1], flush=True)
        if len(levels) >= stop:
            raise _Enough()
        return orig(self, *a, **k)
    cls.generate_with_fallback = spy
    try:
        with torch.no_grad():
            m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), return_timestamps=True,
                       language="zh", task="transcribe", condition_on_prev_tokens=True, temperature=(0.0,),
                       logprob_threshold=-1e9, no_speech_threshold=1.0)
    except _Enough:
        pass
    finally:
        cls.generate_with_fallback = orig


def gen_lv2(out):
    from prompted_inputs import LV2_PICK, lv2_candidate_features
    cfg, m = _lv2_model()
    feats, mask = lv2_candidate_features(LV2_PICK)
    ids, rec = run_longform(m, feats, mask, condition_on_prev_tokens=True, temperature=(0.0,), logprob_threshold=-1e9,
                            no_speech_threshold=1.0)
    store(out, "lv2_condf", ids, rec)
    check_conditioned(rec, cfg["max_target_positions"] // 2 - 1, 3)


def main():
    path = os.path.join(HERE, "prompted.npz")
    out = {}
    if os.path.exists(path):
        z = np.load(path)
        out.update({k: z[k] for k in z.files})
    for case in os.environ.get("PROMPTED_CASES", "short,pl,cond,lv2").split(","):
        {"short": gen_short, "pl": gen_pl, "cond": gen_cond, "lv2search": search_lv2, "lv2": gen_lv2}[case](out)
        np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
