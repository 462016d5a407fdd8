"""generate's host side against the commit before it was split into plan -> encode -> languages -> prompts -> decode
(tests/golden/generate_host.json, recorded there by tests/golden/make_golden_generate_host.py over the case table of
tests/generate_plan_cases.py): every decoder built and its constructor arguments, the prompt rows and keyword names of
every run, the _detect calls, the ids and languages, and every argument error with its message are compared exactly.
Then the planner alone (tw/generate_plan.py plan_generate, given a config and a generation config and no model): each
case's Request against what the recorded call did, the precedence of the argument checks, and the table's coverage of
generate's arguments and of the planner's raise statements."""
import ast
import dataclasses
import inspect
import json
import os
import traceback
import types

import pytest

import generate_plan_cases as gp
from conftest import GOLDEN
from tw import generate_plan, generation

with open(os.path.join(GOLDEN, "generate_host.json")) as _f:
    RECORDED = json.load(_f)
INVALID = sorted(n for n, r in RECORDED["cases"].items() if "error" in r)
PLANNED = sorted(n for n in gp.CASES if n not in INVALID or n in gp.LATE)      # the planner returns a Request


def test_table_is_the_recorded_one():
    assert len(RECORDED["commit"]) == 40
    assert sorted(RECORDED["cases"]) == sorted(gp.CASES)
    assert gp.LATE <= set(INVALID)


@pytest.mark.parametrize("name", sorted(gp.CASES))
def test_equals_recorded(name):
    got = json.loads(json.dumps(gp.run_case(generation, gp.CASES[name])))
    assert got == RECORDED["cases"][name]


def plan(name):
    """The case planned without a model: a config, a generation config and the inputs' shape."""
    case = gp.CASES[name]
    m = gp.model(case)
    cfg = types.SimpleNamespace(**vars(m.config))
    return generate_plan.plan_generate(cfg, generation._resolve_gc(m), **gp.shape(case), **gp.arguments(case, m))


def raised_at(name):
    """(the exception planning the case raises, the line of generate_plan.py that raised it)."""
    with pytest.raises(Exception) as e:
        plan(name)
    lines = [f.lineno for f in traceback.extract_tb(e.value.__traceback__)
             if os.path.basename(f.filename) == "generate_plan.py"]
    return e.value, lines[-1]


@pytest.mark.parametrize("name", [n for n in INVALID if n not in gp.LATE])
def test_the_planner_raises_generates_argument_errors(name):
    err, _ = raised_at(name)
    want = RECORDED["cases"][name]
    assert (type(err).__name__, str(err)) == (want["error"], want["message"])


# nothing was decoded and the languages came from a pass either way: the record cannot tell how the call would have
# detected (in the prefill without prompt_ids: <|startoftranscript|> at position 0)
NO_ROOM = {"short-no-room-auto-ret": generate_plan.PREFILL, "short-no-room-auto-prompt_ids-ret": generate_plan.OWN_PASS}


@pytest.mark.parametrize("name", PLANNED)
def test_request_says_what_the_recorded_call_did(name):
    case, rec = gp.CASES[name], RECORDED["cases"][name]
    rq = plan(name)
    kw = case["kw"]
    assert rq.long_form == (case["form"] == "long")
    built = [b["decoder"] for b in rec.get("built", [])]
    if "error" not in rec:
        assert rec["form"] == case["form"]
        if built:
            kind = (generate_plan.ASSISTED if "_SpecDecoder" in built else
                    generate_plan.BEAM if "_BeamDecoder" in built else generate_plan.GREEDY)
            assert rq.decoder == kind
    assert rq.num_beams == kw.get("num_beams", 1) and (rq.decoder == generate_plan.BEAM) == (rq.num_beams > 1)
    assert (rq.assistant is not None) == ("assist" in case) == (rq.decoder == generate_plan.ASSISTED)
    if rq.assistant is not None:
        assert rq.k == min(kw.get("num_assistant_tokens") or generate_plan.DEFAULT_ASSISTANT_TOKENS,
                           generate_plan.MAX_ASSISTANT_TOKENS)
    assert rq.prompt_ids == (tuple(kw["prompt_ids"]) if "prompt_ids" in kw else None)
    assert rq.timestamps == bool(kw.get("return_timestamps")) and rq.task == kw.get("task")
    assert rq.max_length == kw.get("max_length") and rq.max_new_tokens == kw.get("max_new_tokens")
    assert rq.use_graph == kw.get("use_graph", True) and rq.return_language == bool(kw.get("return_language"))
    assert (rq.repetition_penalty, rq.no_repeat_ngram_size) == (
        kw.get("repetition_penalty", case.get("gc", {}).get("repetition_penalty", 1.0)),
        kw.get("no_repeat_ngram_size", 0))
    # the languages and how "auto" is detected
    language = kw.get("language")
    if language == "auto":
        assert rq.languages == generate_plan.AUTO and rq.detected
        if name in NO_ROOM:
            assert rq.detection == NO_ROOM[name]
        elif "error" not in rec:
            fused = any("detect" in r for r in rec["runs"]) or not rec["detects"]
            assert rq.detection == (generate_plan.PREFILL if fused else generate_plan.OWN_PASS)
            assert fused or len(rec["detects"]) >= 1
        else:
            assert rq.detection == generate_plan.OWN_PASS          # beam search over detected languages
    else:
        assert rq.detection is None and not rq.detected
        if language is None or ("decoder_input_ids" in kw and not rq.long_form and not isinstance(language, list)):
            assert rq.languages is None
        else:
            assert len(rq.languages) == gp.shape(case)["rows"]
            if "error" not in rec and rec["languages"] is not None:
                assert list(rq.languages) == rec["languages"]
            if "error" not in rec and "decoder_input_ids" not in kw and not rq.long_form and rq.num_beams == 1:
                col = len(kw.get("prompt_ids", [])) + 1               # after <|startoftranscript|>
                assert all([row[col] for row in prompt] == list(rq.languages) for prompt in rec["prompts"])
    # the fallback settings
    t = kw.get("temperature", 0.0)
    assert rq.temps == (tuple(t) if isinstance(t, (list, tuple)) else (t,))
    assert rq.track == (len(rq.temps) > 1 or kw.get("logprob_threshold") is not None
                        or kw.get("no_speech_threshold") is not None)
    assert rq.condition_on_prev_tokens == bool(kw.get("condition_on_prev_tokens"))
    assert rq.seed == kw.get("seed", 0) and rq.fallback_batch == kw.get("fallback_batch", True)
    assert (rq.trace is not None) == bool(kw.get("_trace")) and (rq.keep is not None) == bool(kw.get("_keep"))
    with pytest.raises(dataclasses.FrozenInstanceError):
        rq.num_beams = 3


def test_precedence_of_the_argument_checks():
    """Of two adjacent steps violated together the earlier one's check raises: the raise statement that the case
    violating that step alone reaches."""
    alone = {step: raised_at(name)[1] for step, name in gp.ORDER.items()}
    assert len(set(alone.values())) == len(alone) == 13
    assert sorted(gp.PAIRS) == [(i, i + 1) for i in range(1, 13)]
    calls = {p: c for p, c in gp.PAIRS.items() if isinstance(c, dict)}          # the others say why no call has both
    assert len(calls) == 10
    for (i, j) in calls:
        assert raised_at(f"pair-{i}-{j}")[1] == alone[i], (i, j)


def test_every_argument_and_every_raise_is_in_the_table():
    named = set(inspect.signature(generation.generate).parameters) - {"model", "kw"}
    seen = set()
    for case in gp.CASES.values():
        seen |= set(case["kw"])
        seen.add("encoder_outputs" if case.get("input", "features") != "features" else "input_features")
        if case["form"] == "long":
            seen.add("attention_mask")
        if "assist" in case:
            seen.add("assistant_model")
    missing = (named | generate_plan.GENERATE_KEYWORDS) - seen
    assert not missing, sorted(missing)
    # every named parameter of generate but the inputs themselves is a parameter of the planner
    planner = set(inspect.signature(generate_plan.plan_generate).parameters)
    assert named - {"input_features", "encoder_outputs", "attention_mask"} <= planner
    with open(generate_plan.__file__) as f:
        tree = ast.parse(f.read())
    raises = [(n.lineno, n.end_lineno) for n in ast.walk(tree) if isinstance(n, ast.Raise)]
    hit = {raised_at(n)[1] for n in INVALID if n not in gp.LATE}
    unhit = [r for r in raises if not any(r[0] <= line <= r[1] for line in hit)]
    assert len(raises) >= 25 and not unhit, unhit
    # ... and generation.py keeps only the errors that need a device result, one site each
    with open(generation.__file__) as f:
        src = f.read()
    assert src.count("language_rows(") == 0 and src.count("were detected as") == 1
    assert src.count("return_language=True needs") == 0 and 'hasattr(gc, "get")' not in src
    assert src.count('hasattr(encoder_outputs, "last_hidden_state")') == 1              # _unwrap
    assert len(inspect.signature(generation._longform).parameters) <= 6


def test_longform_holds_the_request_and_what_it_derives():
    mine = {f.name for f in dataclasses.fields(generation._LongForm)}
    assert "rq" in mine and not mine & {f.name for f in dataclasses.fields(generate_plan.Request)}
