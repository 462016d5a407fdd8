"""generate's host side (tw/generation.py generate, tw/generate_plan.py plan_generate) as a table of calls over scripted
stand-ins: with the decoders scripted and _detect replaced, a call is pure Python, so what it does can be compared
exactly between two commits.  tests/golden/make_golden_generate_host.py records the table on one commit
(generate_host.json); tests/test_generate_plan_cpu.py runs it on the working tree, compares, and plans every case
without a model.

A case: form ("short": `rows` inputs of `frames` feature frames, or of 4 encoder rows each with input="tuple" /
"output"; "long": one recording per entry of `frames`, with its attention mask), the keyword arguments of generate in
plain values (kw; `_trace` / `_keep` True stand for a fresh list), assist (None, or what the stand-in assistant is),
gc (extra generation config entries of the model), detected (what the replaced _detect answers).
A valid call records the form, every decoder built (class and constructor arguments), every run's prompt rows and
keyword names, the (B, Tk) of every _detect call, the ids and the languages; an invalid one its exception type and
message.  ORDER names, per precedence step of generate's argument checks, one case that violates it alone;
PAIRS, per adjacent pair of steps, one that violates both (or why no call can)."""
import types

import torch

import longform_host_cases as lh
from test_langid_cpu import _RecordingDecoder
from tw.config import GenerationConfig

EOS, SOT, ZH, EN, PREV = 50257, 50258, 50260, 50259, 50361
LOG = dict(built=[], prompts=[], runs=[], detects=[])


def _plain(v):
    """A constructor argument as JSON holds it: the stand-in objects by name."""
    if isinstance(v, (bool, int, float, str, type(None))):
        return v
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, GenerationConfig):
        return "gc"
    if isinstance(v, types.SimpleNamespace):
        return "assistant" if getattr(v, "is_assistant", False) else "model"
    raise TypeError(type(v))


def recording(base, name):
    """`base` logging its construction and every run."""
    class Recording(base):
        def __init__(self, *a, **kw):
            LOG["built"].append(dict(decoder=name, args=_plain(a), kwargs={k: _plain(v) for k, v in kw.items()}))
            super().__init__(*a, **kw)

        def run(self, enc16, prompt, **kw):
            LOG["prompts"].append(torch.as_tensor(prompt).tolist())
            LOG["runs"].append(sorted(kw))
            return super().run(enc16, prompt, **kw)
    return Recording


class _ShortSpec(_RecordingDecoder):
    """generation._SpecDecoder for the short-form path, over the recording stand-in of _Decoder."""

    def __init__(self, model, assistant, gc, Tk, P, ml, timestamps, use_graph, track=False, k=None):
        super().__init__(model, gc, 1, Tk, P, ml, timestamps, use_graph)
        self.k, self.accepted = k, [k, 1]


class _ShortBeam:
    """generation._BeamDecoder for the short-form path: one prompt for every clip."""

    def __init__(self, model, gc, B, nb, Tk, P, max_length, timestamps=None):
        self.B = B

    def run(self, enc16, prompt, **kw):
        assert prompt.dim() == 1
        return torch.tensor([[7, 8, EOS]] * self.B)


STANDINS = dict(short=dict(_Decoder=_RecordingDecoder, _SpecDecoder=_ShortSpec, _BeamDecoder=_ShortBeam),
                long=dict(_Decoder=lh.ScriptedDecoder, _SpecDecoder=lh.ScriptedSpecDecoder,
                          _BeamDecoder=lh.ScriptedBeamDecoder))
# every window of the long-form cases (recording r, stretch k: 10 * r + k), greedy and beam
SCRIPT = {(w, t): lh._tokens(100 + 10 * w, 3 + w % 4, 100 + w) for w in (0, 1, 10, 11) for t in (0.0, "beam")}


def gen_config(**extra):
    kw = dict(decoder_start_token_id=SOT, eos_token_id=EOS, pad_token_id=EOS, no_timestamps_token_id=50363,
              suppress_tokens=[1, PREV, 50362], lang_to_id={"<|zh|>": ZH, "<|en|>": EN})
    kw.update(extra)
    return GenerationConfig(**kw)


def model(case):
    m = lh.model()
    m.generation_config = gen_config(**case.get("gc", {}))
    m.config.eos_token_id = EOS
    m.Vp = 51904
    return m


def assistant(case, m):
    """None, or the stand-in assistant the case describes: assist = dict(k=..., and what differs from a valid one)."""
    a = case.get("assist")
    if a is None:
        return None
    cfg = types.SimpleNamespace(vocab_size=a.get("vocab_size", m.config.vocab_size), d_model=a.get("d_model", 128))
    asst = types.SimpleNamespace(is_assistant=True, decoder_only=a.get("decoder_only", False), conv_input=m.conv_input,
                                 encode=m.encode, act_dtype=m.act_dtype, generation_config=a.get("gc"), config=cfg)
    if a.get("no_config"):
        del asst.config
    return asst


def arguments(case, m):
    """The case's keyword arguments of generate as the call takes them (no inputs)."""
    kw = dict(case["kw"])
    if "decoder_input_ids" in kw:
        kw["decoder_input_ids"] = torch.tensor(kw["decoder_input_ids"])
    for hook in ("_trace", "_keep"):
        if kw.get(hook):
            kw[hook] = []
    if "assist" in case:
        kw["assistant_model"] = assistant(case, m)
    return kw


def shape(case):
    """What plan_generate is told of the inputs: rows, frames, have_features, have_encoder_outputs."""
    if case["form"] == "long":
        return dict(rows=len(case["frames"]), frames=(max(case["frames"]) + 2999) // 3000 * 3000, have_features=True,
                    have_encoder_outputs=False)
    enc = case.get("input", "features") != "features"
    return dict(rows=case.get("rows", 2), frames=None if enc else case.get("frames", 3000), have_features=not enc,
                have_encoder_outputs=enc)


def run_case(generation, case):
    """One case on the module `generation` -> its record."""
    names = STANDINS[case["form"]]
    saved = {n: getattr(generation, n) for n in list(names) + ["_detect", "_longform"]}
    for cls in (lh.ScriptedDecoder, lh.ScriptedBeamDecoder):
        cls.script, cls.logp, cls.ns = SCRIPT, {}, {}
    for v in LOG.values():
        del v[:]
    lh.LOG["runs"], lh.LOG["encodes"] = [], []
    form = []
    m = model(case)
    kw = arguments(case, m)
    sh = shape(case)
    if case["form"] == "long":
        feats, kw["attention_mask"] = lh.features(case["frames"])
    elif sh["have_features"]:
        feats = torch.zeros(sh["rows"], 80, sh["frames"])
    else:
        feats, hidden = None, torch.zeros(sh["rows"], 4, 128)
        kw["encoder_outputs"] = (hidden,) if case["input"] == "tuple" else types.SimpleNamespace(
            last_hidden_state=hidden)

    def fake_detect(model, gc, enc16, B, Tk, want_probs=False):
        LOG["detects"].append([B, Tk])
        return torch.tensor(case.get("detected", [EN, ZH, EN])[:B]), None, [EN, ZH]

    def longform(*a, **k):
        form.append("long")
        return saved["_longform"](*a, **k)
    try:
        for n, cls in names.items():
            setattr(generation, n, recording(cls, n))
        generation._detect, generation._longform = fake_detect, longform
        try:
            out = generation.generate(m, feats, **kw)
        except Exception as e:
            return dict(error=type(e).__name__, message=str(e))
    finally:
        for n, v in saved.items():
            setattr(generation, n, v)
    ids, langs = out if isinstance(out, tuple) else (out, None)
    rec = dict(form=form[0] if form else "short", built=list(LOG["built"]), prompts=list(LOG["prompts"]),
               runs=list(LOG["runs"]), detects=list(LOG["detects"]), ids=ids.tolist(),
               languages=None if langs is None else langs.tolist())
    if kw.get("_trace") is not None:
        rec["trace"] = [{k: v for k, v in t.items() if k != "gate_ms"} for t in kw["_trace"]]
    if kw.get("_keep") is not None:
        rec["kept"] = len(kw["_keep"])
    return rec


LANGUAGES = dict(none=None, name="zh", id=EN, list=["zh", "en"], auto="auto")
FALLBACK = dict(temperature=(0.0, 0.4), compression_ratio_threshold=1.35, logprob_threshold=-1.0,
                no_speech_threshold=0.6)


def _cases():
    c = {}
    # ---- valid short-form calls: every language form x every decoder / prompt / input form
    forms = dict(greedy=dict(kw=dict(_keep=True)), beam=dict(kw=dict(num_beams=2), detected=[ZH, ZH]),
                 assisted=dict(kw=dict(num_assistant_tokens=3, _trace=True, _keep=True), assist=dict(), rows=1),
                 prompt_ids=dict(kw=dict(prompt_ids=[PREV, 9, 10])),
                 decoder_input_ids=dict(kw=dict(decoder_input_ids=[SOT, EN, 50359])),
                 enc_tuple=dict(kw=dict(task="translate"), input="tuple"),
                 enc_output=dict(kw=dict(use_graph=False), input="output"))
    for fname, f in forms.items():
        for lname, lang in LANGUAGES.items():
            if fname == "decoder_input_ids" and lname == "auto":
                continue                                  # an argument error: below
            if fname == "beam" and lname == "list":
                lang = ["zh", "zh"]                       # different names: an argument error, below
            rows = f.get("rows", 2)
            if isinstance(lang, list):
                lang = (lang * 2)[:rows]
            for ret in (False, True):
                if ret and (lang is None or fname == "decoder_input_ids"):
                    continue                              # argument errors: below
                kw = dict(f["kw"], language=lang, max_length=32)
                if ret:
                    kw["return_language"] = True
                case = dict(form="short", rows=rows, kw=kw, **{k: v for k, v in f.items() if k not in ("kw", "rows")})
                c[f"short-{fname}-{lname}" + ("-ret" if ret else "")] = case
    c["short-greedy-auto-task"] = dict(form="short", kw=dict(language="auto", task="transcribe", max_new_tokens=8,
                                                             return_language=True, prompt_condition_type="first-segment"))
    c["short-dii-2d-timestamps"] = dict(form="short", kw=dict(decoder_input_ids=[[SOT, ZH], [SOT, EN]],
                                                              return_timestamps=True, language="no-such-language"))
    c["short-repeat"] = dict(form="short", kw=dict(language="zh", repetition_penalty=1.3, no_repeat_ngram_size=2))
    c["short-repeat-from-gc"] = dict(form="short", gc=dict(repetition_penalty=1.2), kw=dict(language="zh"))
    c["short-inert-fallback-keywords"] = dict(form="short", kw=dict(language="zh", temperature=0.0, do_sample=False,
                                                                    seed=3, fallback_batch=False,
                                                                    condition_on_prev_tokens=True))
    c["short-beam-auto-differ"] = dict(form="short", kw=dict(language="auto", num_beams=2, max_length=32))
    c["short-beam-prompts-differ"] = dict(form="short", kw=dict(num_beams=2, decoder_input_ids=[[SOT, ZH], [SOT, EN]]))
    c["short-assisted-encoder-rows"] = dict(form="short", input="tuple", rows=2, assist=dict(), kw=dict(language="zh"))
    c["short-assisted-own-encoder-needs-features"] = dict(form="short", input="tuple", rows=1, assist=dict(),
                                                          kw=dict(language="zh"))
    c["short-assisted-decoder-only"] = dict(form="short", input="tuple", rows=1, assist=dict(decoder_only=True),
                                            kw=dict(language="zh", return_timestamps=True))
    # ---- no room below the length cap
    for lname in ("name", "auto"):
        for ret in (False, True):
            kw = dict(language=LANGUAGES[lname], max_new_tokens=0)
            if ret:
                kw["return_language"] = True
            c[f"short-no-room-{lname}" + ("-ret" if ret else "")] = dict(form="short", kw=kw)
    c["short-no-room-auto-prompt_ids-ret"] = dict(form="short", kw=dict(language="auto", prompt_ids=[PREV, 9],
                                                                        max_new_tokens=0, return_language=True))
    c["long-no-room"] = dict(form="long", frames=[6000], kw=dict(language="zh", max_new_tokens=0))
    # ---- valid long-form calls
    lf = dict(task="transcribe", max_new_tokens=40, use_graph=False, return_timestamps=True, _trace=True)
    c["long-name"] = dict(form="long", frames=[6000, 2500], kw=dict(lf, language="zh"))
    c["long-none-over-30s"] = dict(form="long", frames=[6000], kw=dict(lf, return_timestamps=False))
    c["long-30s-timestamps"] = dict(form="long", frames=[3000], kw=dict(lf, language=ZH, return_language=True))
    c["long-list-ret"] = dict(form="long", frames=[6000, 2500], kw=dict(lf, language=["zh", "en"], return_language=True))
    c["long-auto-ret"] = dict(form="long", frames=[6000, 2500], kw=dict(lf, language="auto", return_language=True))
    c["long-auto-no-task"] = dict(form="long", frames=[6000], kw=dict(lf, language="auto", task=None))
    c["long-beam"] = dict(form="long", frames=[6000, 2500], kw=dict(lf, language="zh", num_beams=2, **FALLBACK))
    c["long-beam-auto"] = dict(form="long", frames=[6000, 2500], detected=[EN, EN],
                               kw=dict(lf, language="auto", num_beams=2, return_language=True))
    c["long-beam-auto-differ"] = dict(form="long", frames=[6000, 2500], kw=dict(lf, language="auto", num_beams=2))
    c["long-assisted"] = dict(form="long", frames=[6000], assist=dict(), kw=dict(lf, language="zh", **FALLBACK))
    c["long-assisted-auto"] = dict(form="long", frames=[6000], assist=dict(decoder_only=True),
                                   kw=dict(lf, language="auto", num_assistant_tokens=20))
    c["long-repeat"] = dict(form="long", frames=[6000], kw=dict(lf, language="zh", repetition_penalty=1.3,
                                                                 no_repeat_ngram_size=2, **FALLBACK))
    c["long-conditioned"] = dict(form="long", frames=[6000, 6000],
                                 kw=dict(lf, language="zh", condition_on_prev_tokens=True, seed=7, fallback_batch=False,
                                         **FALLBACK))
    c["long-prompt_ids"] = dict(form="long", frames=[6000], kw=dict(lf, language="zh", prompt_ids=[PREV, 9]))
    c["long-decoder_input_ids-ignored"] = dict(form="long", frames=[6000],
                                               kw=dict(lf, language="zh", return_timestamps=False,
                                                       decoder_input_ids=[SOT, EN]))
    # ---- one invalid call for every error the planner owns, in the order of generate's checks
    short = dict(form="short")
    c["bad-keyword"] = dict(short, kw=dict(language="zh", no_such_option=1))
    c["bad-condition-type"] = dict(short, kw=dict(prompt_condition_type="every-segment"))
    c["bad-all-segments"] = dict(short, kw=dict(prompt_condition_type="all-segments"))
    c["bad-prompt_ids-with-decoder_input_ids"] = dict(short, kw=dict(prompt_ids=[PREV, 9], decoder_input_ids=[SOT]))
    c["bad-prompt_ids-conditioned"] = dict(short, kw=dict(prompt_ids=[PREV, 9], condition_on_prev_tokens=True))
    c["bad-tokens-without-assistant"] = dict(short, kw=dict(num_assistant_tokens=3))
    c["bad-assistant-beams"] = dict(short, rows=1, assist=dict(), kw=dict(num_beams=2))
    c["bad-assistant-tokens"] = dict(short, rows=1, assist=dict(), kw=dict(num_assistant_tokens=0))
    c["bad-assistant-no-config"] = dict(short, rows=1, assist=dict(no_config=True), kw={})
    c["bad-assistant-vocabulary"] = dict(short, rows=1, assist=dict(vocab_size=51864), kw={})
    c["bad-assistant-generation-config"] = dict(short, rows=1, assist=dict(gc=dict(suppress_tokens=[1, 2])), kw={})
    c["bad-assistant-width"] = dict(short, rows=1, assist=dict(decoder_only=True, d_model=256), kw={})
    c["bad-assistant-rows"] = dict(short, rows=2, assist=dict(), kw={})
    c["bad-penalty"] = dict(short, kw=dict(repetition_penalty=0.0))
    c["bad-ngram"] = dict(short, kw=dict(no_repeat_ngram_size=-1))
    c["bad-repeat-beam"] = dict(short, kw=dict(repetition_penalty=1.3, no_repeat_ngram_size=2, num_beams=2))
    c["bad-repeat-assistant"] = dict(short, rows=1, assist=dict(), kw=dict(no_repeat_ngram_size=2))
    c["bad-language-list-none"] = dict(short, kw=dict(language=["zh", None]))
    c["bad-language-list-length"] = dict(short, kw=dict(language=["zh"]))
    c["bad-language-list-unknown"] = dict(short, kw=dict(language=["zh", "xx"]))
    c["bad-auto-decoder_input_ids"] = dict(short, kw=dict(language="auto", decoder_input_ids=[SOT, ZH]))
    c["bad-auto-no-table"] = dict(short, gc=dict(lang_to_id={}), kw=dict(language="auto"))
    c["bad-auto-table"] = dict(short, gc=dict(lang_to_id={"a": 5, "b": 5}), kw=dict(language="auto"))
    c["bad-return_language-none"] = dict(short, kw=dict(return_language=True))
    c["bad-return_language-none-long"] = dict(form="long", frames=[6000], kw=dict(return_language=True))
    c["bad-return_language-decoder_input_ids"] = dict(short, kw=dict(language="zh", return_language=True,
                                                                     decoder_input_ids=[SOT, ZH]))
    c["bad-beam-languages"] = dict(short, kw=dict(language=["zh", "en"], num_beams=2))
    c["bad-short-fallback"] = dict(short, kw=dict(language="zh", temperature=(0.0, 0.4)))
    c["bad-short-threshold"] = dict(short, kw=dict(language="zh", no_speech_threshold=0.6))
    c["bad-language-unknown"] = dict(short, kw=dict(language="xx"))
    c["bad-language-unknown-long"] = dict(form="long", frames=[6000], kw=dict(language="xx"))
    # ---- which error wins: both of two adjacent steps violated
    for (i, j), case in PAIRS.items():
        if isinstance(case, dict):
            c[f"pair-{i}-{j}"] = case
    return c


# the precedence of generate's argument checks: step -> a case that violates it alone
ORDER = {1: "bad-keyword", 2: "bad-all-segments", 3: "bad-prompt_ids-with-decoder_input_ids",
         4: "bad-assistant-vocabulary", 5: "bad-assistant-rows", 6: "bad-penalty", 7: "bad-repeat-beam",
         8: "bad-language-list-length", 9: "bad-auto-decoder_input_ids", 10: "bad-auto-no-table",
         11: "bad-return_language-decoder_input_ids", 12: "bad-beam-languages", 13: "bad-short-fallback"}
_S = dict(form="short")
PAIRS = {
    (1, 2): dict(_S, kw=dict(no_such_option=1, prompt_condition_type="every-segment")),
    (2, 3): dict(_S, kw=dict(prompt_condition_type="all-segments", prompt_ids=[PREV, 9], decoder_input_ids=[SOT])),
    (3, 4): dict(_S, kw=dict(prompt_ids=[PREV, 9], decoder_input_ids=[SOT], num_assistant_tokens=3)),
    (4, 5): dict(_S, rows=2, assist=dict(vocab_size=51864), kw={}),
    (5, 6): dict(_S, rows=2, assist=dict(), kw=dict(repetition_penalty=0.0)),
    (6, 7): dict(_S, kw=dict(repetition_penalty=-1.0, no_repeat_ngram_size=2, num_beams=2)),
    (7, 8): dict(_S, kw=dict(no_repeat_ngram_size=2, num_beams=2, language=["zh"])),
    (8, 9): "step 8 fails on a list of languages, step 9 needs language='auto': no call has both",
    (9, 10): dict(_S, gc=dict(lang_to_id={}), kw=dict(language="auto", decoder_input_ids=[SOT, ZH])),
    (10, 11): "step 10 needs language='auto' without decoder_input_ids; step 11 needs language=None or "
              "decoder_input_ids: no call has both",
    (11, 12): dict(_S, kw=dict(language=["zh", "en"], num_beams=2, return_language=True, decoder_input_ids=[SOT, ZH])),
    (12, 13): dict(_S, kw=dict(language=["zh", "en"], num_beams=2, temperature=0.4)),
}
CASES = _cases()
# invalid calls whose error depends on a device result (encoder rows, detected languages, the prompt's length): the
# planner accepts them, generate raises where the result appears
LATE = {"short-beam-auto-differ", "short-beam-prompts-differ", "short-assisted-encoder-rows",
        "short-assisted-own-encoder-needs-features", "long-no-room", "long-beam-auto-differ"}
