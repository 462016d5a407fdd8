"""The long-form seek loop (tw/generation.py _LongForm.run) against the commit before it became one loop
(tests/golden/longform_host.json, recorded there by tests/golden/make_golden_longform_host.py): with scripted decoders
the host logic is pure Python, so the output ids, every _trace record, the keyword names of every run() call and the
shape of every encode() input are compared exactly.  The one allowed difference: on the cases the recorded commit ran
through its sequential loop, the fallback batch of `len(rest)` rows is now rounded with _bucket."""
import json
import os

import pytest

from conftest import GOLDEN
from longform_host_cases import CASES, run_case
from tw import generation

with open(os.path.join(GOLDEN, "longform_host.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def results():
    return {name: json.loads(json.dumps(run_case(generation, case))) for name, case in CASES.items()}


def test_table_is_the_recorded_one():
    assert len(RECORDED["commit"]) == 40
    assert sorted(RECORDED["cases"]) == sorted(CASES)
    assert all(RECORDED["cases"][n]["sequential"] == c["sequential"] for n, c in CASES.items())


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_recorded(results, name):
    got, want = results[name], RECORDED["cases"][name]
    assert got["ids"] == want["ids"]
    assert got["runs"] == want["runs"]
    assert got["encodes"] == want["encodes"]
    assert len(got["trace"]) == len(want["trace"])
    for g, w in zip(got["trace"], want["trace"]):
        g, w = dict(g), dict(w)
        gb, wb = g.pop("batch"), w.pop("batch")
        assert g == w
        assert gb == (generation._bucket(wb) if want["sequential"] else wb), (g["seek"], g["T"])


def test_one_recording_conditioned_makes_the_plain_calls(results):
    for name in ("cond1_t0", "cond1_all_fail", "cond1_switches_off", "cond1_assisted", "cond1_repeat", "cond1_fp32"):
        assert all("pads" not in r["keywords"] for r in results[name]["runs"]), name
    tr = results["cond1_t0"]["trace"]
    init = tr[0]["prompt"]
    assert len(tr) == 3
    segs = []
    for t in tr:
        assert t["prompt"] == ([50361] + generation.previous_text(segs, 50364) + init if segs else init)
        segs.append(t["raw"][:-1])                               # not the last window: its eos is cut


def test_conditioning_switches_off_after_a_hot_accept(results):
    tr = results["cond1_switches_off"]["trace"]
    init = tr[0]["prompt"]
    by_seek = {}
    for t in tr:
        by_seek.setdefault(t["seek"], []).append(t)
    w0, w1, w2 = (by_seek[s] for s in sorted(by_seek))
    assert len(w0) == 1 and w1[0]["prompt"][0] == 50361 and w1[0]["prompt"][-len(init):] == init
    assert [t["T"] for t in w1] == [0.0, 0.4, 1.0] and all(t["needs_fallback"] for t in w1)
    assert all(t["prompt"] == init for t in w2)                  # window 1 kept its T = 1.0 attempt
    fail = results["cond1_all_fail"]["trace"]
    assert all(t["needs_fallback"] and t["prompt"] == fail[0]["prompt"] for t in fail)


def test_assisted_and_fp32(results):
    runs = results["cond1_assisted"]["runs"]
    assert [r["decoder"] for r in runs].count("spec") == 3       # the temperature-0 attempt of each window
    assert all(("enc_a" in r["keywords"]) == (r["decoder"] == "spec") for r in runs)
    assert all(("accepted" in t) == (t["T"] == 0.0) for t in results["cond1_assisted"]["trace"])
    tr = results["cond1_fp32"]["trace"]
    assert len(tr) > 3 and all(t["batch"] == 1 for t in tr)


def test_beam_search_one_recording_at_a_time(results):
    r = results["beam2_two_recordings"]
    assert all(shape[0] == 1 for shape in r["encodes"])
    assert [t["b"] for t in r["trace"]] == sorted(t["b"] for t in r["trace"])         # recording-major
    assert {t["b"] for t in r["trace"]} == {0, 1}
    assert [x["decoder"] for x in r["runs"]] == ["beam", "beam", "row", "beam"]
    failed = [t for t in r["trace"] if t["needs_fallback"]]
    assert len(failed) == 1 and failed[0]["T"] == 0.0 and failed[0]["seek"] == 3000
    assert all("avg_logprob" in t and "no_speech_prob" in t for t in r["trace"])
    z = results["beam2_zero_later"]
    assert all(t["batch"] == 1 for t in z["trace"])              # levels one at a time
    assert [x["decoder"] for x in z["runs"][:3]] == ["beam", "row", "beam"]


def test_several_recordings_conditioned_stay_one_batch(results):
    r = results["cond3_batched"]
    assert all("pads" in x["keywords"] for x in r["runs"])
    assert r["encodes"][0][0] == 3 and any(t["batch"] == 4 for t in r["trace"])
    assert any(t["skip"] for t in r["trace"])
