"""generate(return_token_logprobs=True), host side: the planner's keyword, the seek loop's slicing of an attempt's
log-probs beside its tokens, and the labelling driver's score columns and --min_avg_logprob filter (a stub transcriber
with fixed ids and log-probs)."""
import csv
import dataclasses
import types

import numpy as np
import pytest

from tw import generate_plan, pseudo_labelling as pl
from tw.config import GenerationConfig
from tw.generation import compression_ratio, retrieve_segment, segment_logprobs, trim_pads

EOS, TS = 50257, 50364


def _plan(**kw):
    cfg = types.SimpleNamespace(vocab_size=51865, max_source_positions=1500, max_target_positions=448)
    gc = GenerationConfig(decoder_start_token_id=50258, eos_token_id=EOS, pad_token_id=EOS,
                          no_timestamps_token_id=50363, lang_to_id={"<|zh|>": 50260, "<|en|>": 50259})
    return generate_plan.plan_generate(cfg, gc, rows=2, frames=3000, have_features=True, have_encoder_outputs=False,
                                       language="zh", **kw)


def test_plan_flag_sets_track_and_the_field():
    rq = _plan(return_token_logprobs=True)
    assert rq.return_token_logprobs is True and rq.track is True
    off = _plan()
    assert off.return_token_logprobs is False and off.track is False
    # the default Request is today's in every other field, and the flag changes only the two
    a, b = dataclasses.asdict(off), dataclasses.asdict(rq)
    assert {k for k in a if a[k] != b[k]} == {"return_token_logprobs", "track"}
    assert [f.name for f in dataclasses.fields(generate_plan.Request)][-1] == "return_token_logprobs"
    # long-form: the same, on top of a request that tracks anyway
    lf = _plan(return_token_logprobs=True, return_timestamps=True, temperature=(0.0, 0.4))
    assert lf.long_form and lf.track and lf.return_token_logprobs


def test_plan_flag_with_beam_search_is_not_implemented():
    with pytest.raises(NotImplementedError, match="return_token_logprobs with beam search"):
        _plan(return_token_logprobs=True, num_beams=2)
    with pytest.raises(NotImplementedError, match="repetition_penalty and return_token_logprobs with beam search"):
        _plan(return_token_logprobs=True, num_beams=2, repetition_penalty=1.2)
    assert _plan(num_beams=2).num_beams == 2
    # no other combination raises
    _plan(return_token_logprobs=True, repetition_penalty=1.2, no_repeat_ngram_size=3)
    _plan(return_token_logprobs=True, return_language=True, return_timestamps=True, condition_on_prev_tokens=True)


def test_slicing_keeps_ids_and_logprobs_aligned():
    """A window of two timestamp-delimited segments, a dangling token after the last pair and trailing pads."""
    seq = [TS, 11, 12, TS + 50, TS + 50, 13, TS + 90, TS + 90, 14, EOS, EOS, EOS]
    lps = [-(i + 1) / 8 for i in range(len(seq))]
    raw = seq[:seq.index(EOS) + 1]                      # row_tokens: up to and including the first eos
    cut = raw[:-1]                                      # not the last window: the eos is cut
    cut = trim_pads(cut, EOS, EOS)
    segs, off = retrieve_segment(cut, 3000)
    assert segs == [[TS, 11, 12, TS + 50], [TS + 50, 13, TS + 90, TS + 90]] and off == 180
    got = segment_logprobs(lps[:len(cut)], segs)
    assert [len(g) for g in got] == [len(s) for s in segs]
    flat_ids = [t for s in segs for t in s]
    flat_lps = [x for g in got for x in g]
    # token j of the window keeps value j; token 14 after the last pair belongs to no segment
    assert flat_ids == seq[:8] and flat_lps == lps[:8]
    # no timestamp pair: one segment, the whole window
    one, _ = retrieve_segment([TS, 11, 12, EOS], 3000)
    assert segment_logprobs([-1.0, -2.0, -3.0, -4.0], one) == [[-1.0, -2.0, -3.0, -4.0]]
    # pad == eos keeps one eos; its value stays with it
    kept = trim_pads([TS, 11, EOS, EOS, EOS], EOS, EOS)
    assert kept == [TS, 11, EOS] and [-1.0, -2.0, -3.0, 0.0, 0.0][:len(kept)] == [-1.0, -2.0, -3.0]


def _wavs(tmp_path, secs):
    paths = []
    for i, s in enumerate(secs):
        p = tmp_path / f"f{i}.wav"
        p.write_bytes(b"x")
        paths.append(str(p))
    audio = {p: np.full(int(s * pl.SR), i + 1, dtype=np.float32) for i, (p, s) in enumerate(zip(paths, secs))}
    return paths, lambda p: (audio[p], pl.SR)


# chunk k of the run (in order) decodes to ids [65 + k, 66 + k] with these log-probs (the last one is the eos's)
LPS = [[-0.5, -0.25, -0.125], [-2.0, -4.0, -0.5], [-0.0625, -0.125, -0.0625], [-3.0, -3.0, -3.0]]


def _stub(scores):
    seen = []

    def transcribe(chunks):
        out = []
        for _ in chunks:
            k = len(seen)
            seen.append(k)
            ids = [65 + k, 66 + k]
            out.append((ids, LPS[k]) if scores else ids)
        return out
    return transcribe


def _run(tmp_path, sub, scores, **kw):
    paths, read_audio = _wavs(tmp_path, (10.0, 8.0))          # 2 + 2 chunks of 5 s
    out = tmp_path / sub
    out.mkdir()
    stats = {}

    def write(p, rows):
        pl.save_transcription_to_csv(rows, str(out / (p.split("/")[-1][:-4] + ".csv")),
                                     **(dict(scores=True) if scores else {}))
    extra = dict(scores=True, vocab_size=51865, stats=stats, **kw) if scores else {}
    res = pl.transcribe_files(paths, _stub(scores), lambda ids: "".join(map(chr, ids)), 5, 3, read_audio,
                              num_workers=1, log=lambda s: None, on_done=write, **extra)
    assert all(r is not None for r in res.values())
    return out, stats


def test_driver_score_columns_and_default_csv(tmp_path):
    plain, _ = _run(tmp_path, "plain", False)
    assert (plain / "f0.csv").read_bytes() == b"start,end,text\r\n0.00,5.00,AB\r\n5.00,10.00,BC\r\n"
    assert (plain / "f1.csv").read_bytes() == b"start,end,text\r\n0.00,5.00,CD\r\n5.00,8.00,DE\r\n"
    scored, stats = _run(tmp_path, "scored", True)
    assert stats == dict(rows=4, dropped=0)
    rows = list(csv.reader(open(scored / "f0.csv", newline=""))) + list(csv.reader(open(scored / "f1.csv", newline="")))[1:]
    assert rows[0] == ["start", "end", "text", "avg_logprob", "min_logprob", "compression_ratio"]
    assert [r[:3] for r in rows[1:]] == [["0.00", "5.00", "AB"], ["5.00", "10.00", "BC"], ["0.00", "5.00", "CD"],
                                        ["5.00", "8.00", "DE"]]
    for k, r in enumerate(rows[1:]):
        assert r[3] == f"{sum(LPS[k]) / 3:.4f}" and r[4] == f"{min(LPS[k]):.4f}"
        assert r[5] == f"{compression_ratio([65 + k, 66 + k], 51865):.4f}"
    sc = pl.chunk_scores([65, 66], LPS[0], 51865)
    assert sc["avg_logprob"] == -0.875 / 3 and sc["min_logprob"] == -0.5
    assert pl.chunk_scores([], [], 51865) == dict(avg_logprob=0.0, min_logprob=0.0, compression_ratio=0.0)


def test_driver_min_avg_logprob_drops_and_counts(tmp_path):
    out, stats = _run(tmp_path, "cut", True, min_avg_logprob=-1.0)
    assert stats == dict(rows=2, dropped=2)                   # chunks 1 (avg -2.17) and 3 (avg -3.0)
    assert [r[2] for r in csv.reader(open(out / "f0.csv", newline=""))] == ["text", "AB"]
    assert [r[2] for r in csv.reader(open(out / "f1.csv", newline=""))] == ["text", "CD"]


def test_driver_flags():
    a = pl.parse_args([])
    assert a.write_scores is False and a.min_avg_logprob is None
    a = pl.parse_args(["--write_scores", "True", "--min_avg_logprob", "-1.5"])
    assert a.write_scores is True and a.min_avg_logprob == -1.5
    with pytest.raises(SystemExit):
        pl.parse_args(["--min_avg_logprob", "-1.5"])
