"""Generate tests/golden/langid.npz: HF Transformers 5.15 fp32 on the CPU, language detection on the micro model
and inputs of the repetition fixtures (make_golden_repeat.py), with large-v2's 99 language ids in the generation
config.

Run in the build container (it needs HF Transformers):   python tests/golden/make_golden_langid.py
LANGID_SEARCH=1 prints, for every draw of langid_inputs.LONG_SEEDS, the detected languages of the recordings and the
worst margin, and writes nothing.

Cases (tests/langid_inputs.py holds their settings):
  detect_ids                     detect_language on the 3 clips; lang_margin: their top-2 gap among the language logits
  auto, auto_ts, auto_prompt     generate(language=None): short-form, with timestamps, with prompt_ids -> {tag}_ids
  list                           generate(language=["zh", "en", "zh"])
  lf, lf_cond                    one long-form call of 3 recordings with language=None, without / with
                                 condition_on_prev_tokens, stored as make_golden_prompted.store stores a call;
                                 lf_lang_ids: the recordings' detected languages
Asserted before anything is written: (a) the detected ids of the 3 clips, and of the 3 recordings, are not all equal;
(b) the top-2 gap among the language logits and at every generated step exceeds repeat_inputs.TIE_MARGIN; (c) each
case's ids differ from the same call with language="zh"."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import CONFIGS, TS_GENERATION, _MarginSpy, hf_model, logmel, make_weights  # noqa: E402
from make_golden_prompted import store  # noqa: E402

from langid_inputs import (LANG_TO_ID, LIST_LANGUAGES, LONG, LONG_INPUTS, LONG_LENS, LONG_SEEDS, SHORT,  # noqa: E402
                           WEIGHT_SEED)
from prompted_inputs import PROMPT_IDS, conditioned_features  # noqa: E402
from repeat_inputs import TIE_MARGIN  # noqa: E402


def generation_config():
    from transformers import GenerationConfig
    return GenerationConfig(**{**TS_GENERATION, "lang_to_id": dict(LANG_TO_ID)})


def _model():
    cfg = CONFIGS["micro"]
    m = hf_model(cfg, make_weights(cfg, WEIGHT_SEED, lin_std=0.2)).eval()
    m.generation_config = generation_config()
    return m


def _differs(a, b):
    n = min(a.shape[1], b.shape[1])
    return a.shape != b.shape or bool((a[:, :n] != b[:, :n]).any())


def detect(feats):
    """HF detect_language on `feats` -> (ids, per row the gap between the two largest language logits)."""
    m = _model()
    with torch.no_grad():
        ids = m.detect_language(input_features=feats).numpy()
        sot = torch.full((feats.shape[0], 1), m.generation_config.decoder_start_token_id, dtype=torch.long)
        lg = m(input_features=feats[:, :, :3000], decoder_input_ids=sot, use_cache=False).logits[:, -1]
    lang = lg[:, sorted(LANG_TO_ID.values())].float()
    top = lang.topk(min(2, lang.shape[1]), dim=-1).values
    assert (lang.argmax(-1).numpy() + min(LANG_TO_ID.values()) == ids).all()
    return ids.astype(np.int64), (top[:, 0] - top[:, 1]).numpy()


def _step_margin(spy, ids, eos, tag):
    worst = np.inf
    for r, row in enumerate(ids.tolist()):
        steps = row.index(eos) + 1 if eos in row else len(row)
        assert steps <= len(spy.steps), (tag, steps, len(spy.steps))
        worst = min([worst] + [float(spy.steps[t][r]) for t in range(steps)])
    return worst


def gen_short(out):
    from transformers.generation.logits_process import LogitsProcessorList
    clips = [logmel.synthetic_clip(0), logmel.synthetic_clip(2, 9.0), logmel.synthetic_clip(4, 25.0)]
    feats = torch.from_numpy(logmel.log_mel_batch(clips))
    ids, gap = detect(feats)
    assert len(set(ids.tolist())) > 1, f"(a) the clips' detected languages are all {ids}"
    assert gap.min() > TIE_MARGIN, f"(b) language logits within {gap.min()}"
    out["detect_ids"], out["lang_margin"] = ids, gap.astype(np.float32)
    print("detect", ids, "language margin", gap, flush=True)
    for tag, (kw, prompted) in SHORT.items():
        extra = dict(prompt_ids=torch.tensor(PROMPT_IDS)) if prompted else {}
        language = LIST_LANGUAGES if tag == "list" else None
        m = _model()
        eos = m.generation_config.eos_token_id
        spy = _MarginSpy()
        with torch.no_grad():
            got = m.generate(feats, language=language, logits_processor=LogitsProcessorList([spy]), **kw,
                             **extra).numpy()
            zh = _model().generate(feats, language="zh", **kw, **extra).numpy()
        assert _differs(got, zh), f"(c) {tag}: equal to the language='zh' call"
        if not kw.get("return_timestamps"):             # the seek loop's steps are checked window by window below
            worst = _step_margin(spy, got, eos, tag)
        else:
            worst = min(float(s.min()) for s in spy.steps)
        assert worst > TIE_MARGIN, f"(b) {tag}: a step's top-2 margin is {worst}"
        out[f"{tag}_ids"] = got
        print(tag, got.shape, "min margin", worst, flush=True)


def run_longform(m, feats, mask, language, **kw):
    """make_golden_prompted.run_longform with the call's `language`: one HF long-form call, every window recorded."""
    from transformers.generation.logits_process import LogitsProcessorList
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
        steps = spy.steps[it["start"]:]
        rec["margin"].append([float(s_[index]) for s_ in steps[:len(seek_sequence)]])
        return orig_need(self, seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size,
                         temperature)
    cls._need_fallback, cls.generate_with_fallback = need_spy, gwf_spy
    try:
        with torch.no_grad():
            ids = m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), return_timestamps=True,
                             language=language, logits_processor=LogitsProcessorList([spy]), **kw).numpy()
    finally:
        cls._need_fallback, cls.generate_with_fallback = orig_need, orig_gwf
    return ids, rec


def long_case(tag, lens, seed):
    feats, mask = conditioned_features(lens=lens, seed=seed)
    lang, gap = detect(torch.from_numpy(feats))
    ids, rec = run_longform(_model(), feats, mask, None, **LONG[tag])
    zh, _ = run_longform(_model(), feats, mask, "zh", **LONG[tag])
    worst = min(min(min(r) for r in rec["margin"] if r), float(gap.min()))
    return dict(lang=lang, ids=ids, rec=rec, differs=_differs(ids, zh), worst=worst)


def gen_long(out):
    lens, seed = LONG_INPUTS
    for tag in LONG:
        c = long_case(tag, lens, seed)
        assert len(set(c["lang"].tolist())) > 1, f"(a) {tag}: the recordings' detected languages are all {c['lang']}"
        assert c["worst"] > TIE_MARGIN, f"(b) {tag}: a top-2 margin is {c['worst']}"
        assert c["differs"], f"(c) {tag}: equal to the language='zh' call"
        # every window's prompt carries its recording's language
        assert all(p[-2] == c["lang"][b] for b, p in zip(c["rec"]["b"], c["rec"]["prompt"])), tag
        store(out, tag, c["ids"], c["rec"])
        out["lf_lang_ids"] = c["lang"]


def search():
    for seed in LONG_SEEDS:
        for tag in LONG:
            c = long_case(tag, LONG_LENS, seed)
            print("seed", seed, tag, "languages", c["lang"].tolist(), "worst margin", c["worst"], "differs from zh",
                  c["differs"], flush=True)


def main():
    if os.environ.get("LANGID_SEARCH"):
        return search()
    path = os.path.join(HERE, "langid.npz")
    out = {}
    gen_short(out)
    gen_long(out)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
