"""Language detection without a GPU: the restatement of the kernel parity tests against HF's own expression, the C
declaration against the ctypes signature, generate's argument checks and the per-row prompts of the short- and
long-form paths with scripted decoders (the stand-ins of tests/test_generation_cpu.py and
tests/longform_host_cases.py)."""
import os
import re
import types

import pytest
import torch

import langid_cases as lc
import longform_host_cases as lh
from tw import generation
from tw.config import GenerationConfig

EOS, SOT, ZH, EN, TRANSCRIBE, NO_TS = 50257, 50258, 50260, 50259, 50359, 50363
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the oracle itself
def _hf_ids(x, table):
    """HF detect_language's last lines: every non-language logit to -inf, argmax."""
    logits = x.clone()
    mask = torch.ones_like(logits[0], dtype=torch.bool)
    mask[list(table)] = False
    logits[:, mask] = -float("inf")
    return logits.argmax(-1)


@pytest.mark.parametrize("vocab", list(lc.VOCABS))
@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_restatement_ids_equal_hf_expression(vocab, dtype):
    V = lc.VOCABS[vocab][0]
    finite = [lc.KINDS.index(k) for k in lc.FINITE]
    ties = 0
    for L, tk in lc.combos(vocab):
        table = lc.table_of(tk, L, V)
        assert table == sorted(set(table)) and 0 <= table[0] and table[-1] < V and len(table) == L
        x = lc.score_rows(V, table, dtype)
        ids, p = lc.lang_detect_ref(x, table)
        assert torch.equal(ids[finite], _hf_ids(x[finite], table)), (vocab, dtype, L, tk)
        assert bool(torch.isnan(p[lc.KINDS.index("all_neg_inf")]).all()) and bool(torch.isnan(
            p[lc.KINDS.index("nan_one")]).all())
        assert int(ids[lc.KINDS.index("all_neg_inf")]) == table[0]
        assert int(ids[lc.KINDS.index("nan_one")]) == table[L // 2]           # the lowest-id NaN, not the larger number
        assert torch.allclose(p[finite].sum(1), torch.ones(len(finite), dtype=torch.float64))
        g = x[lc.KINDS.index("tie_groups"), table]
        ties += int((g == g.max()).sum() > 1)
    assert ties >= len(lc.combos(vocab)) // 2                               # the table holds real ties
    if dtype != torch.float32:                                              # ... and ties made by the rounding
        table = lc.table_of("scattered", 100, V) if V >= 100 else lc.table_of("scattered", 65, V)
        r = lc.KINDS.index("tie_after_rounding")
        x16, x32 = lc.score_rows(V, table, dtype)[r], lc.score_rows(V, table, torch.float32)[r]
        assert int(lc.lang_detect_ref(x16[None], table)[0]) == table[0]
        assert int(lc.lang_detect_ref(x32[None], table)[0]) == table[len(table) // 2]


def test_planted_fault_is_caught():
    """A detector that takes the highest id on ties disagrees with the restatement on the table's tie rows."""
    V = lc.VOCABS["small"][0]
    table = lc.table_of("contiguous", 100, V)
    x = lc.score_rows(V, table, torch.float32)
    g = x[:, table]
    wrong = torch.tensor([table[len(table) - 1 - int(torch.flip(row, [0]).argmax())] for row in g])
    ids, _ = lc.lang_detect_ref(x, table)
    differ = [lc.KINDS[r] for r in range(lc.ROWS) if int(wrong[r]) != int(ids[r])]
    assert "tie_groups" in differ and "tie_in_group" in differ and "all_neg_inf" in differ


def test_header_declares_what_the_binding_holds():
    from tw import _native
    with open(os.path.join(REPO, "include", "tw_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"int tw_lang_detect\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == len(_native.SIGNATURES["tw_lang_detect"])


# ------------------------------------------------------------------------------------------ argument checks
def _gc(**extra):
    kw = dict(decoder_start_token_id=SOT, eos_token_id=EOS, pad_token_id=EOS, no_timestamps_token_id=NO_TS,
              suppress_tokens=[], lang_to_id={"<|zh|>": ZH, "<|en|>": EN})
    kw.update(extra)
    return GenerationConfig(**kw)


def _model(**gc_extra):
    cfg = types.SimpleNamespace(max_source_positions=1500, max_target_positions=448, vocab_size=51865, d_model=128,
                                eos_token_id=EOS)
    return types.SimpleNamespace(config=cfg, device=torch.device("cpu"), compute="bf16",
                                 generation_config=_gc(**gc_extra))


FEATS = torch.zeros(2, 80, 3000)


def test_language_argument_errors():
    m = _model()
    with pytest.raises(ValueError, match="length of the list must match the batch size"):
        generation.generate(m, FEATS, language=["zh"])
    with pytest.raises(ValueError, match="Expected length of 2, but got 3"):
        generation.generate(m, FEATS, language=("zh", "en", "zh"), return_timestamps=True)
    with pytest.raises(TypeError, match="containing `None`"):
        generation.generate(m, FEATS, language=["zh", None])
    with pytest.raises(ValueError, match="unknown language"):
        generation.generate(m, FEATS, language=["zh", "xx"])
    with pytest.raises(ValueError, match="decoder_input_ids"):
        generation.generate(m, FEATS, language="auto", decoder_input_ids=torch.tensor([SOT, ZH]))
    for empty in (dict(lang_to_id={}), dict(lang_to_id=None)):
        with pytest.raises(ValueError, match="generation_config"):
            generation.generate(_model(**empty), FEATS, language="auto")
        with pytest.raises(ValueError, match="generation_config"):
            generation.detect_language(_model(**empty), FEATS)
    with pytest.raises(ValueError, match="return_language"):
        generation.generate(m, FEATS, return_language=True)
    with pytest.raises(ValueError, match="owns the prompt"):
        generation.generate(m, FEATS, language="zh", decoder_input_ids=torch.tensor([SOT, ZH]), return_language=True)
    with pytest.raises(ValueError, match="return_language"):          # before anything is encoded or decoded
        generation.generate(m, torch.zeros(2, 80, 6000), max_new_tokens=8, use_graph=False, return_language=True)
    with pytest.raises(NotImplementedError, match="different languages"):
        generation.generate(m, FEATS, language=["zh", "en"], num_beams=2)
    with pytest.raises(ValueError, match="either `input_features` or `encoder_outputs`"):
        generation.detect_language(m)
    with pytest.raises(ValueError, match="only one of `input_features` or `encoder_outputs`"):
        generation.detect_language(m, FEATS, encoder_outputs=(torch.zeros(2, 1500, 128),))
    with pytest.raises(TypeError, match="return_languages"):
        generation.generate(m, FEATS, language="zh", return_languages=True)


def test_language_table_is_checked_where_it_is_built():
    assert generation.language_table(_gc(), 51865) == [EN, ZH]
    for bad in ({"a": 5, "b": 5}, {"a": -1}, {"a": 51865}, {str(i): i for i in range(257)}):
        with pytest.raises(ValueError, match="lang_to_id"):
            generation.language_table(_gc(lang_to_id=bad), 51865)
    assert generation.language_rows(_gc(), None, 3) is None and generation.language_rows(_gc(), "auto", 3) == "auto"
    assert generation.language_rows(_gc(), "zh", 2) == [ZH, ZH]
    assert generation.language_rows(_gc(), ("en", "<|zh|>", ZH), 3) == [EN, ZH, ZH]


def test_build_prompt_forms():
    gc = _gc()
    assert generation.build_prompt(gc, "zh", None) == [SOT, ZH, TRANSCRIBE, NO_TS]
    assert generation.build_prompt(gc, ZH, None, detected=True) == [SOT, ZH, NO_TS]        # HF: no task token
    assert generation.build_prompt(gc, ZH, "transcribe", True, detected=True) == [SOT, ZH, TRANSCRIBE]
    assert generation.build_prompt(gc, None, None) == [SOT, NO_TS]


# ------------------------------------------------------------------------------------------ short form, scripted
class _RecordingDecoder:
    """generation._Decoder for the short-form path: records the prompt and the keywords of run."""
    seen = []

    def __init__(self, model, gc, B, Tk, P, ml, timestamps, use_graph, **kw):
        self.B, self.P = B, P
        self.sel = types.SimpleNamespace(ids=torch.zeros(B, ml, dtype=torch.int64))

    def run(self, enc16, prompt, **kw):
        type(self).seen.append(dict(prompt=prompt.tolist(), kw=sorted(kw), detect=kw.get("detect")))
        self.sel.ids[:, :self.P] = prompt
        if kw.get("detect") is not None:
            self.sel.ids[:, 1] = torch.tensor([ZH, EN][:self.B])            # what the device kernel would write
        return torch.tensor([[7, 8, EOS]] * self.B)


def _short_model():
    m = lh.model()
    m.generation_config = _gc()
    m.Vp = 51904
    return m


def test_short_form_rows_take_their_languages(monkeypatch):
    monkeypatch.setattr(generation, "_Decoder", _RecordingDecoder)
    seen = _RecordingDecoder.seen
    del seen[:]
    m = _short_model()
    out, lang = generation.generate(m, FEATS, language=["zh", "en"], return_language=True, max_length=32)
    assert seen[-1]["prompt"] == [[SOT, ZH, TRANSCRIBE, NO_TS], [SOT, EN, TRANSCRIBE, NO_TS]]
    assert seen[-1]["kw"] == [] and lang.tolist() == [ZH, EN] and out.tolist() == [[7, 8, EOS]] * 2
    # a fixed language: the prompt and the call of before, and the language repeated
    out, lang = generation.generate(m, FEATS, language="zh", task="transcribe", return_language=True, max_length=32)
    assert seen[-1]["prompt"] == [[SOT, ZH, TRANSCRIBE, NO_TS]] * 2 and seen[-1]["kw"] == []
    assert lang.tolist() == [ZH, ZH]
    generation.generate(m, FEATS, max_length=32)
    assert seen[-1]["prompt"] == [[SOT, NO_TS]] * 2 and seen[-1]["kw"] == []
    # with decoder_input_ids the caller owns the prompt and `language` is not looked at, as before: not even resolved
    generation.generate(m, FEATS, language="no-such-language", decoder_input_ids=torch.tensor([SOT, EN]), max_length=32)
    assert seen[-1]["prompt"] == [[SOT, EN]] * 2 and seen[-1]["kw"] == []
    # "auto": the fused path -- a placeholder language in column 1, the id table handed to run, the languages read
    # from column 1 of the decoder's id matrix afterwards
    out, lang = generation.generate(m, FEATS, language="auto", task="transcribe", return_language=True, max_length=32)
    assert seen[-1]["prompt"] == [[SOT, EN, TRANSCRIBE, NO_TS]] * 2 and seen[-1]["kw"] == ["detect"]
    assert seen[-1]["detect"].tolist() == [EN, ZH] and seen[-1]["detect"].dtype == torch.int32
    assert lang.tolist() == [ZH, EN]
    generation.generate(m, FEATS, language="auto", max_length=32)
    assert seen[-1]["prompt"] == [[SOT, EN, NO_TS]] * 2                      # no task passed: no task token (HF)


def test_separate_pass_forms_detect_first(monkeypatch):
    """prompt_ids and beam search cannot take the fused path: they call the detection pass and build host prompts."""
    monkeypatch.setattr(generation, "_Decoder", _RecordingDecoder)
    calls = []

    def fake_detect(model, gc, enc16, B, Tk, want_probs=False):
        calls.append((B, Tk))
        return torch.tensor([EN, ZH][:B]), None, [EN, ZH]
    monkeypatch.setattr(generation, "_detect", fake_detect)
    seen = _RecordingDecoder.seen
    m = _short_model()
    out, lang = generation.generate(m, FEATS, language="auto", prompt_ids=[50361, 9], return_language=True,
                                    max_length=32)
    assert calls == [(2, 1)] and lang.tolist() == [EN, ZH] and seen[-1]["kw"] == []
    assert seen[-1]["prompt"] == [[50361, 9, SOT, EN, NO_TS], [50361, 9, SOT, ZH, NO_TS]]
    with pytest.raises(NotImplementedError, match="different languages"):
        generation.generate(m, FEATS, language="auto", num_beams=2, max_length=32)


# ------------------------------------------------------------------------------------------ long form, scripted
def _longform(monkeypatch, language, **kw):
    names = dict(_Decoder=lh.ScriptedDecoder, _SpecDecoder=lh.ScriptedSpecDecoder, _BeamDecoder=lh.ScriptedBeamDecoder)
    for n, cls in names.items():
        monkeypatch.setattr(generation, n, cls)
    case = lh.CASES["cond3_batched"]
    for cls in (lh.ScriptedDecoder, lh.ScriptedBeamDecoder):
        cls.script, cls.logp, cls.ns = case["script"], case.get("logp", {}), case.get("ns", {})
    lh.LOG["runs"], lh.LOG["encodes"] = [], []
    feats, mask = lh.features(case["frames"])
    trace = []
    out = generation.generate(lh.model(), feats, attention_mask=mask, language=language, task="transcribe",
                              max_new_tokens=40, use_graph=False, return_timestamps=True, _trace=trace, **case["kw"],
                              **kw)
    return out, [{k: v for k, v in t.items() if k != "gate_ms"} for t in trace]


def test_long_form_per_recording_prompts_reach_every_window(monkeypatch):
    langs = [ZH, EN, ZH]
    (out, lang), trace = _longform(monkeypatch, langs, return_language=True)
    assert lang.tolist() == langs and len(trace) > 6
    conditioned = 0
    for t in trace:
        assert t["prompt"][-3:] == [SOT, langs[t["b"]], TRANSCRIBE], t
        conditioned += int(len(t["prompt"]) > 3)
    assert conditioned >= 2 and {t["b"] for t in trace} == {0, 1, 2}
    # the same languages for every recording: the trace of the fixed-language call, prompts included
    fixed, tf = _longform(monkeypatch, "zh")
    same, ts = _longform(monkeypatch, ["zh", "zh", "zh"])
    assert torch.equal(fixed, same) and tf == ts
    # the languages change nothing but the prompts (the scripted decoders do not read them)
    strip = [{k: v for k, v in t.items() if k != "prompt"} for t in trace]
    assert strip == [{k: v for k, v in t.items() if k != "prompt"} for t in tf] and torch.equal(out, fixed)


def test_long_form_auto_detects_once_on_the_raw_first_windows(monkeypatch):
    calls = []

    def fake_detect(model, gc, enc16, B, Tk, want_probs=False):
        calls.append((B, enc16.flatten().tolist()))
        return torch.tensor([EN, ZH, EN][:B]), None, [EN, ZH]
    monkeypatch.setattr(generation, "_detect", fake_detect)
    gc_langs = {"<|zh|>": ZH, "<|en|>": EN}
    monkeypatch.setattr(lh, "_gc", lambda: GenerationConfig(
        decoder_start_token_id=SOT, eos_token_id=EOS, pad_token_id=EOS, no_timestamps_token_id=NO_TS,
        suppress_tokens=[1, lh.PREV, 50362], lang_to_id=gc_langs))
    (out, lang), trace = _longform(monkeypatch, "auto", return_language=True)
    # one detection call for the whole batch, on each recording's first window (window ids 0, 10, 20)
    assert calls == [(3, [0.0, 10.0, 20.0])] and lang.tolist() == [EN, ZH, EN]
    assert all(t["prompt"][-3:] == [SOT, [EN, ZH, EN][t["b"]], TRANSCRIBE] for t in trace)
    with pytest.raises(NotImplementedError, match="different languages"):
        _longform(monkeypatch, "auto", num_beams=2)
