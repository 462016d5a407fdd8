"""generate(return_token_logprobs=True) on the GPU: the per-token log-probs the selection kernels store
(tw_select_sample[_ts]_lp, tw_spec_accept_lp in csrc/decode.hip) and their way up to generate and the labelling driver.

The oracle everywhere is the running sum the engine has always kept: the stored values, added in column order in fp32
from 0.0f, must give sum_logp bit for bit, and each value must be the log-softmax of the processed row at the token
(tests/select_cases.py restates the processing; the bar is that file's LOGP_ATOL, the one test_select_kernels_gpu.py
holds sum_logp to)."""
import csv
import functools
import os

import numpy as np
import pytest
import torch

import select_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 50257
F32_ATOL = 1e-4         # fp32 model against the fp32 CPU oracle: tests/test_fp32_gpu.py's bar for log-probs


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def f32_sum(vals):
    """The values added in order in fp32, from 0.0f."""
    return functools.reduce(lambda a, b: np.float32(a + np.float32(b)), vals, np.float32(0.0))


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the kernels

STEPS, B3, COL0, LD_LP = 6, 3, 2, 11          # columns 2 .. 7 of a [3, 9] id matrix; log-prob rows of 11 floats
_DT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


def step_rows(voc, ts):
    """fp32 logits [STEPS][3][V]: row 0 decodes on, row 1 is finished before the first call, row 2 reaches eos (plain:
    at the first step; with the timestamp rules, whose first step takes a timestamp, at the second)."""
    gen_ = torch.Generator().manual_seed(5 + int(ts))
    xs = []
    for s in range(STEPS):
        rows = []
        for b in range(B3):
            x = sc._base(voc, gen_, ts_shift=-5.0 if ts else 0.0)
            if ts:
                x[voc.no_ts] = 14.0
                x[sc.TEXT_BEST + s] = 12.0
                if b == 0 and s == 3:
                    x[voc.mid] = 13.0               # a timestamp in the middle of the decode: an open pair after it
            if b == 2 and s == (1 if ts else 0):
                x[voc.eos] = 20.0
            rows.append(x)
        xs.append(torch.stack(rows))
    return xs


def drive(F, voc, ts, dtype, xs, lp, slp=True):
    """STEPS consecutive columns through the tracking selector, the column from t_dev -> (ids, done, last_ts,
    sum_logp, tok_logp or None) on the host and the id matrix before every step."""
    T = COL0 + STEPS + 1
    ids = torch.zeros(B3, T, dtype=torch.int64, device=DEV)
    ids[:, :COL0] = torch.tensor([1, 2])
    done = torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV)
    last = torch.full((B3,), -1, dtype=torch.int32, device=DEV)
    nxt = torch.zeros(B3, dtype=torch.int64, device=DEV)
    sum_logp = torch.zeros(B3, dtype=torch.float32, device=DEV) if slp else None
    tok = torch.full((B3, LD_LP), float("nan"), dtype=torch.float32, device=DEV) if lp else None
    ctl = torch.zeros(3 * B3, dtype=torch.int32, device=DEV)
    sup, beg = F.token_bitmask(voc.sup, voc.V, DEV), F.token_bitmask(voc.beg, voc.V, DEV)
    t_dev = torch.tensor([COL0 - 1], dtype=torch.int32, device=DEV)
    before = []
    kw = dict(tok_logp=tok) if lp else {}
    for s in range(STEPS):
        logits = torch.full((B3, voc.ld), float("nan"), dtype=dtype, device=DEV)
        logits[:, :voc.V] = xs[s].to(dtype).to(DEV)
        before.append(ids.cpu().clone())
        if ts:
            F.select_sample_ts(logits, voc.ld, B3, voc.V, sup, beg, voc.eos, done, ids, 1, nxt, last, COL0, ctl,
                               sum_logp, ts_begin=voc.ts_begin, no_ts=voc.no_ts, max_initial=50, t_dev=t_dev, **kw)
        else:
            F.select_sample(logits, voc.ld, B3, voc.V, sup, beg, False, voc.eos, done, ids, 1, nxt, ctl, sum_logp,
                            t_dev=t_dev, begin_col=-1, **kw)
        F.step_advance(t_dev)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu()
    return dict(ids=host(ids), done=host(done), last=host(last), slp=host(sum_logp), tok=host(tok), before=before)


def restated_logp(voc, ts, dtype, x, ids_before, col, tok):
    """fp32 log_softmax of the processed row (tests/select_cases.py) at the kernel's token."""
    gen = ids_before[COL0:col].tolist()
    g = sc.Group("drive", voc, ts, COL0, col, 50 if ts else -1, ts, [])
    row = sc.Row("drive", x, gen=gen, prompt=(1, 2))
    r = sc.processed_row(g, row, dtype)
    if ts:
        assert sc.mass_margin(g, row, dtype) > sc.MASS_MARGIN          # the mass rule is not decided by rounding
    assert bool(torch.isfinite(r[tok]))
    return float(torch.log_softmax(r.float(), -1)[tok])


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=lambda d: _DT[d])
@pytest.mark.parametrize("ts", [False, True], ids=["plain", "ts"])
@pytest.mark.parametrize("vocab", ["small", "real"])
def test_kernels_store_what_they_add(vocab, ts, dtype):
    from tw import ops as F
    voc = sc.VOCABS[vocab]
    xs = step_rows(voc, ts)
    old = drive(F, voc, ts, dtype, xs, lp=False)
    new = drive(F, voc, ts, dtype, xs, lp=True)
    for k in ("ids", "done", "last", "slp"):
        assert torch.equal(old[k], new[k]), k
    assert old["done"].tolist() == [0, 1, 1]                      # row 2 reached eos on the way
    tok = new["tok"]
    cols = slice(COL0, COL0 + STEPS)
    written = torch.zeros(B3, LD_LP, dtype=torch.bool)
    written[:, cols] = True
    assert bool(torch.isnan(tok[~written]).all()) and not bool(torch.isnan(tok[written]).any())
    assert bits(tok[1, cols]).tolist() == [0] * STEPS             # the finished row: exact zeros
    e = new["ids"][2, cols].tolist().index(voc.eos)
    assert float(tok[2, COL0 + e]) < 0 and bits(tok[2, COL0 + e + 1:COL0 + STEPS]).tolist() == [0] * (STEPS - 1 - e)
    worst = 0.0
    for b in range(B3):
        assert bits(f32_sum(tok[b, cols].tolist())) == bits(new["slp"][b]), (b, tok[b, cols], new["slp"][b])
        live = STEPS if b == 0 else 0 if b == 1 else e + 1
        for s in range(live):
            col = COL0 + s
            want = restated_logp(voc, ts, dtype, xs[s][b], new["before"][s][b], col, int(new["ids"][b, col]))
            worst = max(worst, abs(float(tok[b, col]) - want))
    print(f"\n[token_logprobs] {vocab} {'ts' if ts else 'plain'} {_DT[dtype]}: max |stored - fp32 restatement| = "
          f"{worst:.3e}")
    assert worst <= sc.LOGP_ATOL
    # the per-token matrix alone: no running sum
    alone = drive(F, voc, ts, dtype, xs, lp=True, slp=False)
    assert torch.equal(alone["ids"], new["ids"]) and torch.equal(alone["done"], new["done"])
    assert torch.equal(alone["tok"][:, cols], tok[:, cols]) and bool(torch.isnan(alone["tok"][~written]).all())


def test_lp_entries_reject_nothing_to_track():
    from tw import _native, ops as F
    voc = sc.SMALL
    logits = torch.zeros(1, voc.ld, dtype=torch.float32, device=DEV)
    ids = torch.full((1, 4), 7, dtype=torch.int64, device=DEV)
    done = torch.zeros(1, dtype=torch.uint8, device=DEV)
    nxt = torch.zeros(1, dtype=torch.int64, device=DEV)
    ctl = torch.zeros(3, dtype=torch.int32, device=DEV)
    tok = torch.full((1, 2), 5.0, dtype=torch.float32, device=DEV)
    lib = _native.lib()
    args = (logits.data_ptr(), voc.ld, F._dt(logits), 1, voc.V, None, None, 0, voc.eos, done.data_ptr(), ids.data_ptr(),
            4, 2, nxt.data_ptr(), None, -1, ctl.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.tw_select_sample_lp(*args, None, None, 0, stream) == 1                 # neither output
    assert lib.tw_select_sample_lp(*args, None, tok.data_ptr(), 2, stream) == 1       # column 2 of a 2-column row
    torch.cuda.synchronize()
    assert ids.tolist() == [[7] * 4] and tok.tolist() == [[5.0, 5.0]]


# ------------------------------------------------------------------------------------------------ 2. acceptance

def _accept(F, lp, drafts, target, slots, t0=3, k=3, T=16, sum0=-0.75):
    """One tw_spec_accept[_lp] round on a row whose last accepted column is t0."""
    ids = torch.full((T + k + 1,), EOS, dtype=torch.int64, device=DEV)
    ids[:t0 + 1] = torch.tensor([50258, 11, 12, 13])
    ids[t0 + 1:t0 + 2 + k] = torch.tensor(target)
    st = dict(ids=ids, t=torch.tensor([t0], dtype=torch.int32, device=DEV),
              cur=torch.zeros(1, dtype=torch.int64, device=DEV), done=torch.zeros(1, dtype=torch.uint8, device=DEV),
              snap=torch.zeros(1, dtype=torch.uint8, device=DEV),
              slots=torch.tensor(slots, dtype=torch.float32, device=DEV),
              slp=torch.tensor([sum0], dtype=torch.float32, device=DEV),
              hist=torch.zeros(4, dtype=torch.int32, device=DEV))
    tok = torch.full((T + k + 1,), float("nan"), dtype=torch.float32, device=DEV) if lp else None
    F.spec_accept(torch.tensor(drafts, dtype=torch.int64, device=DEV), k, ids, T, EOS, st["t"], st["cur"], st["done"],
                  st["snap"], slots=st["slots"], sum_logp=st["slp"], hist=st["hist"],
                  **(dict(tok_logp=tok) if lp else {}))
    torch.cuda.synchronize()
    return {k_: v.cpu() for k_, v in st.items()}, None if tok is None else tok.cpu()


@pytest.mark.parametrize("name,drafts,target,adv", [
    ("accept_0", [21, 22, 23], [31, 32, 33, 34], 1),
    ("accept_all", [21, 22, 23], [21, 22, 23, 24], 4),
    ("eos_in_drafts", [21, EOS, 23], [21, EOS, EOS, EOS], 3)])
def test_spec_accept_lp(name, drafts, target, adv):
    from tw import ops as F
    t0, k = 3, 3
    slots = [-0.3, -1.7, -0.011, -2.5]
    if name == "eos_in_drafts":
        slots[2] = slots[3] = 0.0            # the launches after the eos saw a finished row: nothing added
    old, _ = _accept(F, False, drafts, target, slots)
    new, tok = _accept(F, True, drafts, target, slots)
    for key in old:
        assert torch.equal(old[key], new[key]), key
    assert int(new["t"]) == t0 + adv and new["slots"].tolist() == [0.0] * (k + 1)
    got = tok[t0 + 1:t0 + k + 2]
    assert bits(got[:adv]).tolist() == bits(slots[:adv]).tolist()
    assert bits(got[adv:]).tolist() == [0] * (k + 1 - adv)
    other = torch.ones_like(tok, dtype=torch.bool)
    other[t0 + 1:t0 + k + 2] = False
    assert bool(torch.isnan(tok[other]).all())
    assert bits(f32_sum([-0.75] + got.tolist())) == bits(new["slp"][0])


# ------------------------------------------------------------------------------------------------ 3. short form

_CACHE = {}


def _fp32_model():
    if "m" not in _CACHE:
        from test_decode_gpu import _ts_model
        mg, cfg, w, m = _ts_model()
        m.set_compute("fp32")
        _CACHE["m"] = (mg, cfg, w, m)
    return _CACHE["m"]


def _oracle():
    if "ref" not in _CACHE:
        from oracle.whisper_ref import Ref, to_torch
        mg, cfg, w, m = _fp32_model()
        _CACHE["ref"] = Ref(cfg, to_torch(w))
    return _CACHE["ref"]


def _restate(ref, feats1, prompt, toks, sup, ts):
    """fp32 log-probs of `toks` after `prompt` on one window: the CPU oracle teacher-forced along them, the suppress
    masks (and the begin ones at the first step), the timestamp rules when `ts`, log_softmax at the token."""
    from oracle.greedy_ref import timestamp_rules
    seq = torch.tensor([list(prompt) + list(toks)])
    with torch.no_grad():
        lg = ref.logits(ref.decoder(seq[:, :-1], ref.encoder(feats1))).float()[0]
    P, out = len(prompt), []
    for j, tok in enumerate(toks):
        row = lg[P - 1 + j].clone()
        row[sup] = -float("inf")
        if j == 0:
            row[[220, EOS]] = -float("inf")
        if ts:
            row = timestamp_rules(row, list(toks[:j]), j == 0, max_initial=50)
        out.append(float(torch.log_softmax(row, -1)[tok]))
    return out


@pytest.mark.parametrize("ts", [False, True], ids=["plain", "timestamps"])
def test_short_form(ts):
    from test_decode_gpu import _feats
    mg, cfg, w, m = _fp32_model()
    feats = _feats()
    kw = dict(language="zh", task="transcribe", max_new_tokens=12, return_timestamps=ts)
    want = m.generate(feats, **kw)
    trace = []
    ids, lps = m.generate(feats, return_token_logprobs=True, _trace=trace, **kw)
    assert torch.equal(ids, want)
    assert lps.shape == ids.shape and lps.dtype == torch.float32 and lps.device == ids.device
    ids, lps = ids.cpu(), lps.cpu()
    ref = _oracle()
    worst = 0.0
    if not ts:
        prompt = [50258, 50260, 50359, 50363]
        for b in range(3):
            row = ids[b].tolist()
            n = row.index(EOS) + 1 if EOS in row else len(row)
            assert bits(lps[b, n:]).tolist() == [0] * (len(row) - n)
            assert bool((lps[b, :n] < 0).all())
            got = lps[b, :n].tolist()
            worst = max(worst, max(abs(a - c) for a, c in zip(got, _restate(ref, feats[b:b + 1], prompt, row[:n],
                                                                            mg.SUPPRESS, False))))
    else:
        assert {t["b"] for t in trace} == {0, 1, 2}
        for t in trace:
            seg = torch.zeros(1, 80, 3000)
            seg[0, :, :t["n"]] = feats[t["b"], :, t["seek"]:t["seek"] + t["n"]]
            want_lp = _restate(ref, seg, t["prompt"], t["raw"], mg.SUPPRESS, True)
            assert len(t["token_logprobs"]) == len(t["raw"])
            worst = max(worst, max(abs(a - c) for a, c in zip(t["token_logprobs"], want_lp)))
        check_kept_segments(trace, ids, lps, 3000)
    print(f"\n[token_logprobs] short form ts={ts}: max |engine - fp32 oracle| = {worst:.3e}")
    assert worst <= F32_ATOL


def check_kept_segments(trace, ids, lps, frames):
    """Every recording's returned tokens are the concatenation of its kept attempts' segments, and the returned
    log-probs over those columns are the kept attempt's token_logprobs at the same indices; 0 in the padding after
    them.  frames: the recordings' length (a window that does not reach it loses its eos, as in the seek loop)."""
    from tw.generation import retrieve_segment, trim_pads
    for b in sorted({t["b"] for t in trace}):
        kept = {}
        for t in trace:
            if t["b"] == b:
                kept[t["seek"]] = t                   # the last attempt of a window is the one kept
        col = 0
        for seek in sorted(kept):
            t = kept[seek]
            seq = list(t["raw"])
            if seek + 3000 < frames and seq and seq[-1] == EOS:
                seq = seq[:-1]
            seq = trim_pads(seq, EOS, EOS)
            if t.get("skip") or not seq:
                continue
            segs, _ = retrieve_segment(seq, t["n"])
            n = sum(len(s) for s in segs)
            assert ids[b, col:col + n].tolist() == [x for s in segs for x in s], (b, seek)
            assert bits(lps[b, col:col + n]).tolist() == bits(t["token_logprobs"][:n]).tolist(), (b, seek)
            col += n
        assert bits(lps[b, col:]).tolist() == [0] * (ids.shape[1] - col)


# ------------------------------------------------------------------------------------------------ 4. assisted

@pytest.mark.parametrize("ts", [False, True], ids=["plain", "timestamps"])
def test_assisted_equals_unassisted(ts):
    from test_assisted_gpu import _assistant, _feat1, _kwargs, _target
    cfg, m, GC = _target("bf16")
    a = _assistant("bf16", "random")
    want_ids, want_lps = m.generate(_feat1(), return_token_logprobs=True, **_kwargs(ts))
    got_ids, got_lps = m.generate(_feat1(), assistant_model=a, num_assistant_tokens=3, return_token_logprobs=True,
                                  **_kwargs(ts))
    assert torch.equal(got_ids, want_ids) and got_ids.shape[1] >= 8
    assert torch.equal(got_lps.view(torch.int32), want_lps.view(torch.int32))
    assert bool((want_lps[0, 0] < 0))


# ------------------------------------------------------------------------------------------------ 5. long-form, fallback

def test_longform_fallback_keeps_the_kept_attempts_values():
    from test_fallback_gpu import _setup
    mg, cfg, w, m = _setup()
    lf = torch.from_numpy(mg.longform_features())
    kw = dict(attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True, language="zh",
              task="transcribe", temperature=(0.0, 0.4), compression_ratio_threshold=0.0, max_new_tokens=40, seed=11)
    want = m.generate(lf, **kw)
    trace = []
    ids, lps = m.generate(lf, return_token_logprobs=True, _trace=trace, **kw)
    assert torch.equal(ids, want) and lps.shape == ids.shape
    for s in {t["seek"] for t in trace}:
        assert [t["T"] for t in trace if t["seek"] == s] == [0.0, 0.4]        # every window fell back once
    check_kept_segments(trace, ids.cpu(), lps.cpu(), lf.shape[-1])
    for t in trace:
        n = len(t["token_logprobs"])
        assert n == len(t["raw"]) >= 1
        mean = float(f32_sum(t["token_logprobs"])) / n
        assert abs(mean - t["avg_logprob"]) <= 2 ** -23 * abs(mean), (mean, t["avg_logprob"])


# ------------------------------------------------------------------------------------------------ 6. the driver

def test_driver_writes_scores(tmp_path):
    import json
    from oracle import logmel
    from oracle.weights import CONFIGS, make_weights
    from test_pseudo_labelling_gpu import _wav
    from tw import pseudo_labelling as pl
    from tw.config import GenerationConfig, WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration
    cfg = CONFIGS["micro"]
    m = WhisperForConditionalGeneration.from_state_dict(
        WhisperConfig(**cfg), {k: torch.from_numpy(v) for k, v in make_weights(cfg, 2).items()}, dtype=torch.bfloat16)
    m.generation_config = GenerationConfig(suppress_tokens=[], begin_suppress_tokens=[220, 50257])
    ck = tmp_path / "ckpt"
    m.save_pretrained(str(ck))
    with open(ck / "generation_config.json", "w") as f:
        json.dump(dict(m.generation_config), f)
    files = []
    for i, secs in enumerate((12.0, 4.0, 9.5)):
        p = tmp_path / f"clip{i}.wav"
        _wav(p, logmel.synthetic_clip(10 + i, secs))
        files.append(str(p))
    man = tmp_path / "manifest.csv"
    man.write_text("audio_path\n" + "\n".join(files) + "\n")
    argv = ["--dataset_path", str(man), "--model_size_or_path", str(ck), "--chunk_length", "5", "--batch_size", "3",
            "--num_workers", "2", "--max_new_tokens", "24", "--byte_level_text_tokenizer", "True", "--log_progress",
            "False"]
    pl.main(argv + ["--output_dir", str(tmp_path / "plain")])
    pl.main(argv + ["--output_dir", str(tmp_path / "scored"), "--write_scores", "True"])
    nrows = 0
    for name in ("clip0.csv", "clip1.csv", "clip2.csv"):
        with open(tmp_path / "plain" / name, newline="", encoding="utf-8") as f:
            plain = list(csv.reader(f))
        with open(tmp_path / "scored" / name, newline="", encoding="utf-8") as f:
            scored = list(csv.reader(f))
        assert plain[0] == ["start", "end", "text"]
        assert scored[0] == ["start", "end", "text", "avg_logprob", "min_logprob", "compression_ratio"]
        assert [r[:3] for r in scored] == plain                     # the same labels
        for r in scored[1:]:
            avg, lo, cr = float(r[3]), float(r[4]), float(r[5])
            assert lo <= avg <= 0 and cr > 0, r
            nrows += 1
    assert nrows == 3 + 1 + 2
    # a threshold above every score drops every row and keeps the files
    pl.main(argv + ["--output_dir", str(tmp_path / "none"), "--write_scores", "True", "--min_avg_logprob", "0.5"])
    for name in ("clip0.csv", "clip1.csv", "clip2.csv"):
        with open(tmp_path / "none" / name, newline="", encoding="utf-8") as f:
            assert list(csv.reader(f)) == [["start", "end", "text", "avg_logprob", "min_logprob", "compression_ratio"]]
    assert sorted(os.listdir(tmp_path / "none")) == sorted(os.listdir(tmp_path / "plain"))
