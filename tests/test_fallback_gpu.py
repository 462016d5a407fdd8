"""Temperature fallback, thresholds and previous-text conditioning of long-form decoding on the GPU
(HF generate_with_fallback / _need_fallback / WhisperNoSpeechDetection /
_prepare_decoder_input_ids, restated in oracle/greedy_ref.longform and pinned there to HF fixtures
tests/golden/fallback.npz).

Parity bar (stated per test):
  * sampling kernel: 8192 Gumbel-max draws pass a Pearson chi-square goodness-of-fit test against
    softmax(x / T) at p > 1e-4 (the RNG is the engine's counter-based hash, not torch's stream: distributional,
    not bitwise); log-prob of each chosen token equal to log_softmax(x)[token] within 1e-4;
  * average log-probs and no-speech probabilities of each window vs the bf16-autocast oracle
    teacher-forced along the GPU's own tokens: 0.05 absolute (avg log-prob; bf16 logits) and
    0.15 in log space (no-speech probability);
  * conditioned prompts: exactly the oracle's rule applied to the GPU's own previous segments;
    every conditioned window obeys the timestamp rules vs the oracle;
  * threshold pairs that never / always fire: outputs identical to plain greedy / empty (as HF).
"""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _setup():
    from test_decode_gpu import _ts_model
    return _ts_model()


def _chi2_pvalue(obs, exp):
    """Pearson chi-square goodness of fit; bins expecting < 5 draws are pooled."""
    from scipy.stats import chi2
    big = exp >= 5
    o = torch.cat([obs[big], obs[~big].sum()[None]]) if (~big).any() else obs[big]
    e = torch.cat([exp[big], exp[~big].sum()[None]]) if (~big).any() else exp[big]
    keep = e > 0
    stat = float(((o[keep] - e[keep]) ** 2 / e[keep]).sum())
    return float(chi2.sf(stat, int(keep.sum()) - 1))


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_sampling_kernel_distribution_and_logprob(T):
    from tw import ops as F
    V, B = 200, 8192
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(V, generator=g) * 2.0).to(torch.bfloat16)
    sup = [3, 17, 150]
    logits = x[None].repeat(B, 1).contiguous().cuda()
    ids = torch.zeros(B, 4, dtype=torch.int64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    nxt = torch.zeros(B, dtype=torch.int64, device="cuda")
    # one control word per row (each row an independent attempt with its own seed)
    ctl = F.sample_ctl([T] * B, [1234 + 7919 * b for b in range(B)]).cuda()
    slp = torch.zeros(B, dtype=torch.float32, device="cuda")
    F.select_sample(logits, V, B, V, F.token_bitmask(sup, V, "cuda"), None, False, 50257 % V, done, ids, 1, nxt, ctl,
                    slp)
    torch.cuda.synchronize()
    tok = ids[:, 1].cpu()
    xf = x.float()
    xm = xf.clone()
    xm[sup] = -float("inf")
    p = torch.softmax(xm / T, -1)
    freq = torch.bincount(tok, minlength=V).float() / B
    assert float(freq[sup].sum()) == 0.0
    assert _chi2_pvalue(freq * B, p * B) > 1e-4
    lp = torch.log_softmax(xm, -1)
    np.testing.assert_allclose(slp.cpu().numpy(), lp[tok].numpy(), atol=1e-4)
    # greedy (1/T = 0) through the same kernel: argmax, same log-prob rule
    F.sample_ctl([0.0] * B, [0] * B, ctl)
    slp.zero_(); done.zero_()
    F.select_sample(logits, V, B, V, F.token_bitmask(sup, V, "cuda"), None, False, 50257 % V, done, ids, 2, nxt, ctl,
                    slp)
    torch.cuda.synchronize()
    assert bool((ids[:, 2].cpu() == int(xm.argmax())).all())
    np.testing.assert_allclose(slp.cpu().numpy(), float(lp.max()), atol=1e-4)
    # a different seed gives a different draw sequence
    F.sample_ctl([T] * B, [99 + 7919 * b for b in range(B)], ctl)
    F.select_sample(logits, V, B, V, None, None, False, 50257 % V, done.zero_(), ids, 3, nxt, ctl, slp)
    torch.cuda.synchronize()
    assert not torch.equal(ids[:, 3].cpu(), tok)


def test_sampling_respects_timestamp_rules():
    """Sampled tokens of the timestamp selector stay inside the rule-processed support: at the
    window's first step only timestamps <= ts_begin + max_initial; never <|notimestamps|>."""
    from tw import ops as F
    V, B = 51865, 2048
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(V, generator=g) * 0.5).to(torch.bfloat16)
    x[50364:50364 + 30] = 6.0                               # make timestamps likely
    logits = torch.zeros(B, 51904, dtype=torch.bfloat16)
    logits[:, :V] = x
    logits = logits.cuda()
    ids = torch.full((B, 8), 50258, dtype=torch.int64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    nxt = torch.zeros(B, dtype=torch.int64, device="cuda")
    last_ts = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ctl = F.sample_ctl([1.0] * B, [3 + 7919 * b for b in range(B)]).cuda()
    slp = torch.zeros(B, dtype=torch.float32, device="cuda")
    F.select_sample_ts(logits, 51904, B, V, None, None, 50257, done, ids, 3, nxt, last_ts, 3, ctl, slp,
                       max_initial=10)
    torch.cuda.synchronize()
    tok = ids[:, 3].cpu()
    assert bool(((tok >= 50364) & (tok <= 50374)).all())
    assert len(set(tok.tolist())) > 3                       # several timestamps drawn
    assert bool(torch.isfinite(slp).all()) and bool((slp < 0).all())


def test_thresholds_never_and_always_fire():
    mg, cfg, w, m = _setup()
    g = load_golden("fallback")
    lf = torch.from_numpy(mg.longform_features())
    kw = dict(attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True, language="zh",
              task="transcribe")
    plain = m.generate(lf, **kw).cpu()[0].tolist()
    none = m.generate(lf, temperature=(0.0,), logprob_threshold=-1e9, no_speech_threshold=1.0, **kw).cpu()[0].tolist()
    skip = m.generate(lf, temperature=(0.0,), logprob_threshold=1e9, no_speech_threshold=0.0, **kw).cpu()
    assert none == plain
    assert skip.shape[1] == 0 and g["fb_skipall_ids"].shape[1] == 0


def test_window_logprob_and_no_speech_vs_oracle():
    from oracle import greedy_ref
    from oracle.whisper_ref import Ref, to_torch
    mg, cfg, w, m = _setup()
    g = load_golden("fallback")
    lf = torch.from_numpy(mg.longform_features())
    trace = []
    m.generate(lf, attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True,
               language="zh", task="transcribe", temperature=(0.0,), logprob_threshold=-1e9,
               no_speech_threshold=1.0, _trace=trace)
    ref = Ref(cfg, to_torch(w), amp=True)
    prompt = [50258, 50260, 50359]
    T = lf.shape[-1]
    for k, tr in enumerate(trace):
        n = tr["n"]
        seg = torch.zeros(1, 80, 3000)
        seg[0, :, :n] = lf[0, :, tr["seek"]:tr["seek"] + n]
        toks = list(tr["raw"])
        while len(toks) > 1 and toks[-1] == 50257 and toks[-2] == 50257:
            toks = toks[:-1]
        seq = torch.tensor([prompt + toks])
        with torch.no_grad():
            h = ref.decoder(seq[:, :-1], ref.encoder(seg))
            lg = ref.logits(h).float()[0]
        scores = []
        for j in range(len(toks)):
            row = lg[len(prompt) - 1 + j].clone()
            row[mg.SUPPRESS] = -float("inf")
            if j == 0:
                row[[220, 50257]] = -float("inf")
            full = greedy_ref.timestamp_rules(row, toks[:j], j == 0, max_initial=50)
            if not torch.isfinite(full[toks[j]]):
                # the "timestamp mass beats the best text token" decision was a bf16 near-tie and the GPU
                # took the other branch (checked by test_decode_gpu): score that branch's row
                full = greedy_ref.timestamp_rules(row, toks[:j], j == 0, max_initial=50, apply_mass=False)
                if toks[j] >= 50364:
                    full[:50364] = -float("inf")
            scores.append(full)
        avg = greedy_ref.avg_logprob(scores, toks)
        nsp = float(torch.softmax(lg[0], -1)[50362])
        assert abs(tr["avg_logprob"] - avg) <= 0.05, (k, tr["avg_logprob"], avg)
        assert abs(math.log(tr["no_speech_prob"]) - math.log(nsp)) <= 0.15, (k, tr["no_speech_prob"], nsp)
    # and against HF fp32 where the windows' tokens agree (same inputs): same scale of values
    hf = g["fb_avg_logprobs"]
    assert abs(trace[0]["avg_logprob"] - hf[0]) <= 0.25


def test_condition_on_prev_tokens():
    """Conditioned long-form on the GPU: each window's prompt is the oracle rule applied to the GPU's
    own earlier segments; every window obeys the timestamp rules given that prompt; the host loop
    rebuilds the output."""
    from oracle import greedy_ref
    from oracle.whisper_ref import Ref, to_torch
    from test_decode_gpu import _check_ts_window
    mg, cfg, w, m = _setup()
    lf = torch.from_numpy(mg.longform_features())
    trace = []
    out = m.generate(lf, attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True,
                     language="zh", task="transcribe", condition_on_prev_tokens=True, _trace=trace).cpu()[0].tolist()
    ref = Ref(cfg, to_torch(w), amp=True)
    init = [50258, 50260, 50359]
    T = lf.shape[-1]
    seek, segments, rebuilt = 0, [], []
    for k, tr in enumerate(trace):
        assert tr["seek"] == seek
        exp_prompt = list(init)
        if segments:
            prev = []
            for st in segments:
                prev.extend(st[:-1] if len(st) > 2 and st[-2] >= 50364 else st)
            exp_prompt = [50361] + prev[-223:] + init
        assert tr["prompt"] == exp_prompt, k
        n = min(3000, T - seek)
        seg = torch.zeros(1, 80, 3000)
        seg[0, :, :n] = lf[0, :, seek:seek + n]
        _check_ts_window(ref, seg, exp_prompt, tr["raw"], mg.SUPPRESS)
        seq = list(tr["raw"])
        if seek + 3000 < T and seq and seq[-1] == 50257:
            seq = seq[:-1]
        segs, off = greedy_ref.retrieve_segment(seq, n)
        for sgm in segs:
            rebuilt.extend(sgm)
            segments.append(list(sgm))
        seek += off if off > 0 else n
    assert rebuilt == out and len(trace) >= 3 and trace[1]["prompt"][0] == 50361


def test_sampled_fallback_control_flow():
    """compression_ratio_threshold 0 fails every attempt: each window is tried at every temperature
    in order, the last (sampled) attempt is kept, conditioning switches off (T >= 0.5); the same seed
    reproduces the output, another seed changes it; sampled windows still obey the rule support."""
    mg, cfg, w, m = _setup()
    lf = torch.from_numpy(mg.longform_features())
    kw = dict(attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True, language="zh",
              task="transcribe", temperature=(0.0, 0.4, 1.0), compression_ratio_threshold=0.0,
              condition_on_prev_tokens=True, max_new_tokens=40)
    trace = []
    out1 = m.generate(lf, seed=11, _trace=trace, **kw).cpu()[0].tolist()
    out2 = m.generate(lf, seed=11, **kw).cpu()[0].tolist()
    out3 = m.generate(lf, seed=12, **kw).cpu()[0].tolist()
    assert out1 == out2 and out1 != out3
    seeks = sorted(set(t["seek"] for t in trace))
    for s in seeks:
        ts = [t["T"] for t in trace if t["seek"] == s]
        assert ts == [0.0, 0.4, 1.0]
        assert all(t["needs_fallback"] for t in trace if t["seek"] == s)
    # after a window accepted at T = 1.0 the next prompt is not conditioned
    for t in trace:
        if t["seek"] > 0:
            assert t["prompt"][0] == 50258
    for t in trace:
        toks = t["raw"]
        assert toks[0] >= 50364 and toks[0] <= 50364 + 50           # first step: a timestamp <= max_initial
        assert 50363 not in toks


def test_batched_fallback_equals_sequential():
    """The speculative fallback batch (after a window's first attempt fails, the remaining temperatures decode
    together as one batch, one row per temperature with its own seed) gives exactly the attempts of decoding
    them one at a time: the same sampled tokens, the same per-attempt average log-prob and no-speech
    probability, the same accepted attempt and output (tw/generation.py _LongForm.run)."""
    mg, cfg, w, m = _setup()
    lf = torch.from_numpy(mg.longform_features())
    kw = dict(attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True, language="zh",
              task="transcribe", temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold=1.35,
              logprob_threshold=-1.0, no_speech_threshold=0.6, max_new_tokens=40, seed=5)
    ta, tb = [], []
    a = m.generate(lf, _trace=ta, fallback_batch=True, **kw).cpu()[0].tolist()
    b = m.generate(lf, _trace=tb, fallback_batch=False, **kw).cpu()[0].tolist()
    assert a == b
    assert len(ta) == len(tb) and any(t["batch"] > 1 for t in ta)
    strip = lambda r: r[:next((i + 1 for i, x in enumerate(r) if x == 50257), len(r))]
    for x, y in zip(ta, tb):
        assert (x["seek"], x["T"], x["prompt"]) == (y["seek"], y["T"], y["prompt"])
        assert strip(x["raw"]) == strip(y["raw"])
        assert x["avg_logprob"] == y["avg_logprob"] and x["no_speech_prob"] == y["no_speech_prob"]
        assert (x["needs_fallback"], x["skip"]) == (y["needs_fallback"], y["skip"])


def test_one_conditioned_recording_bucketed_fallback_equals_sequential():
    """One recording under condition_on_prev_tokens goes through the same seek loop as a batch of them, so its
    fallback batch is rounded with _bucket: the five sampled temperatures decode as 8 rows (the three extra rows repeat
    the first attempt and are dropped).  compression_ratio_threshold 0 fails every attempt, so every row of that batch
    is compared with its own batch-1 decode (fallback_batch=False): the same output, per attempt the same seek,
    temperature and prompt, the same tokens up to eos, and bit-equal average log-prob and no-speech probability."""
    mg, cfg, w, m = _setup()
    lf = torch.from_numpy(mg.longform_features())
    kw = dict(attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True, language="zh",
              task="transcribe", condition_on_prev_tokens=True, temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
              compression_ratio_threshold=0.0, max_new_tokens=40)
    ta, tb = [], []
    a = m.generate(lf, _trace=ta, fallback_batch=True, **kw).cpu()[0].tolist()
    b = m.generate(lf, _trace=tb, fallback_batch=False, **kw).cpu()[0].tolist()
    assert a == b
    assert len(ta) == len(tb) and len(ta) % 6 == 0 and len(ta) >= 12
    assert [t["batch"] for t in ta[:6]] == [1, 8, 8, 8, 8, 8] and all(t["batch"] == 1 for t in tb)
    strip = lambda r: r[:next((i + 1 for i, x in enumerate(r) if x == 50257), len(r))]
    for x, y in zip(ta, tb):
        assert (x["seek"], x["T"], x["prompt"]) == (y["seek"], y["T"], y["prompt"])
        assert strip(x["raw"]) == strip(y["raw"])
        assert x["avg_logprob"] == y["avg_logprob"] and x["no_speech_prob"] == y["no_speech_prob"]
