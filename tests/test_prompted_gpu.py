"""Prompted decoding on the GPU: generate(prompt_ids=...) and batched condition_on_prev_tokens=True against HF's own
calls (tests/golden/prompted.npz, tests/golden/make_golden_prompted.py: HF Transformers 5.15 fp32 on the CPU), and
the left-padded decode session under them.

* pad invariance: a window decoded from a prompt left-padded by 5 columns of garbage ids (masked per row on the device:
  tw_decode_attn_ks / tw_embed_step_off) gives the ids of the unpadded decode -- fp32, bf16 and fp16, on the skinny-GEMM
  step (micro, d = 128) and the GEMV step (d = 256), graph and eager.  The padded row runs the same kernels' bodies
  over the same keys in the same order, so the 16-bit rows are held to identity as well (no tie allowance needed);
* fp32: the ids of fixtures (a) short-form greedy with and without timestamps, (b) num_beams 2, (c) long-form on 3
  recordings with prompt_ids; (d) the conditioned long-form on 3 recordings (micro dims) and on 2 recordings at the
  large-v2 dims: windows, seeks, prompts and tokens, every seek iteration's windows in ONE decode batch;
* bf16 / fp16: each row of the conditioned batched call decodes what its window decodes alone from its recorded prompt.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from prompted_inputs import PROMPT_IDS, conditioned_features

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g():
    return load_golden("prompted")


@pytest.fixture(scope="module")
def micro32():
    from test_batched_longform_gpu import _model
    return _model("micro", None)


def _rows(a, fill=-1):
    return [[int(x) for x in r if x != fill] for r in a]


def _levels(bs):
    """Indices of consecutive trace records grouped by seek iteration (a recording appears once per iteration)."""
    out, cur, seen = [], [], set()
    for i, b in enumerate(bs):
        if b in seen:
            out.append(cur)
            cur, seen = [], set()
        seen.add(b)
        cur.append(i)
    out.append(cur)
    return out


# ------------------------------------------------------------------------------------------ pad invariance
@pytest.mark.parametrize("name,compute", [("micro", "fp32"), ("micro", "bf16"), ("micro", "fp16"), ("d256", "bf16"),
                                          ("d256", "fp16")])
def test_left_padded_prompt_decodes_the_unpadded_ids(name, compute):
    import oracle.fixture_inputs as fx
    from oracle import logmel
    from test_decode_kstart_gpu import small_model
    from tw.config import GenerationConfig
    from tw.generation import _Decoder, row_tokens
    cfg, m = small_model(name, compute)
    gc = GenerationConfig({k: fx.TS_GENERATION[k] for k in fx.TW_GENERATION_KEYS})
    feats = torch.from_numpy(logmel.log_mel_batch([logmel.synthetic_clip(0), logmel.synthetic_clip(2, 9.0)]))
    enc16 = m.encode(m.conv_input(feats))
    Tk = cfg["max_source_positions"]
    prompt = [50361, 1000, 1037, 1074, 50258, 50260, 50359]
    P, new, npad = len(prompt), 40, 5
    for use_graph in (True, False):
        plain = _Decoder(m, gc, 2, Tk, P, P + new, True, use_graph)
        a = plain.run(enc16, torch.tensor([prompt] * 2, device=DEV)).cpu()
        padded = _Decoder(m, gc, 2, Tk, P + npad, P + npad + new, True, use_graph)
        garbage = [[7, 50257, 51000, 3, 50258], [50257] * npad]
        b = padded.run(enc16, torch.tensor([garbage[0] + prompt, garbage[1] + prompt], device=DEV),
                       pads=[npad, npad], shift_positions=True).cpu()
        assert torch.equal(a, b), (name, compute, use_graph)
        # rows with different pad counts in one batch, the decoder reused (its captured step survives)
        c = padded.run(enc16, torch.tensor([garbage[0] + prompt, [50257] * 2 + [50361, 1111, 1112] + prompt],
                                           device=DEV), pads=[npad, 2], shift_positions=True).cpu()
        assert row_tokens(c[0].tolist(), 50257) == row_tokens(a[0].tolist(), 50257)
        # all-zero counts take the per-row entries and give the plain decode; no counts: today's calls
        d = plain.run(enc16, torch.tensor([prompt] * 2, device=DEV), pads=[0, 0]).cpu()
        assert torch.equal(a, d) and plain.sess.padded is True
        d = plain.run(enc16, torch.tensor([prompt] * 2, device=DEV)).cpu()
        assert torch.equal(a, d) and plain.sess.padded is False and padded.sess.padded is True


# ------------------------------------------------------------------------------------------ generate(prompt_ids)
def _short_feats(n):
    from test_decode_gpu import _feats
    return _feats()[:n]


def test_prompt_ids_short_form_fp32_vs_hf(g, micro32):
    m = micro32
    pid = torch.tensor(PROMPT_IDS)
    assert g["prompt_ids"].tolist() == PROMPT_IDS
    got = m.generate(_short_feats(3), prompt_ids=pid, language="zh", task="transcribe", max_length=64).cpu().numpy()
    np.testing.assert_array_equal(got, g["pa_ids"])
    # not vacuous: the unprompted decode (greedy.npz) differs
    un = load_golden("greedy")["greedy_ids"]
    n = min(un.shape[1], got.shape[1])
    assert (un[:, :n] != got[:, :n]).any()
    got = m.generate(_short_feats(2), prompt_ids=pid, return_timestamps=True, language="zh", task="transcribe",
                     max_new_tokens=48).cpu().numpy()
    np.testing.assert_array_equal(got, g["pa_ts_ids"])
    un = load_golden("greedy_ts")["ts_short_ids"]
    n = min(un.shape[1], got.shape[1])
    assert (un[:, :n] != got[:, :n]).any()
    # a list works as the tensor does
    got = m.generate(_short_feats(3), prompt_ids=PROMPT_IDS, language="zh", task="transcribe", max_length=64)
    np.testing.assert_array_equal(got.cpu().numpy(), g["pa_ids"])


def test_prompt_ids_beam_fp32_vs_hf(g, micro32):
    got = micro32.generate(_short_feats(3), prompt_ids=torch.tensor(PROMPT_IDS), language="zh", task="transcribe",
                           max_length=64, num_beams=2).cpu().numpy()
    np.testing.assert_array_equal(got, g["pb_ids"])


def _check_longform(m, g, tag, feats, mask, **kw):
    trace = []
    out = m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), return_timestamps=True,
                     language="zh", task="transcribe", _trace=trace, **kw).cpu().numpy()
    want = list(zip(g[f"{tag}_win_b"].tolist(), g[f"{tag}_win_seek"].tolist()))
    assert [(t["b"], t["seek"]) for t in trace] == want
    assert [t["prompt"] for t in trace] == _rows(g[f"{tag}_win_prompt"])
    assert [[int(x) for x in t["raw"]] for t in trace] == _rows(g[f"{tag}_win_ids"])
    np.testing.assert_array_equal(out, g[f"{tag}_ids"])
    if f"{tag}_win_ns" in g:
        np.testing.assert_allclose([t["avg_logprob"] for t in trace], g[f"{tag}_win_avg"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose([t["no_speech_prob"] for t in trace], g[f"{tag}_win_ns"], rtol=1e-4, atol=1e-12)
    return trace


def test_prompt_ids_long_form_fp32_vs_hf(g, micro32):
    import oracle.fixture_inputs as fx
    feats, mask = fx.batched_longform_features()
    trace = _check_longform(micro32, g, "pl", feats, mask, prompt_ids=torch.tensor(PROMPT_IDS), temperature=(0.0,),
                            logprob_threshold=-1e9, no_speech_threshold=1.0)
    assert all(t["prompt"][:len(PROMPT_IDS)] == PROMPT_IDS for t in trace)
    assert all(t["batch"] >= 3 for t in trace[:3])


# ------------------------------------------------------------------------------------------ batched conditioning
def _assert_fixture_conditions(g, tag, cfg):
    """The fixture exercises what it is for (asserted from the recorded HF trace, so the test cannot pass vacuously)."""
    prompts = _rows(g[f"{tag}_win_prompt"])
    cut = cfg["max_target_positions"] // 2 - 1
    lv = _levels(g[f"{tag}_win_b"].tolist())
    assert any(len({len(prompts[i]) for i in ix}) > 1 for ix in lv if len(ix) > 1)     # rows that differ in length
    assert any(len(p) > 1 + 3 for p in prompts)                                         # previous text
    assert any(len(p) == 1 + cut + 3 for p in prompts)                                  # a prompt cut at the limit
    for ix in lv:                                                                       # HF's padded length
        assert {int(g[f"{tag}_win_plen"][i]) for i in ix} == {max(len(prompts[i]) for i in ix)}
    return lv


@pytest.mark.parametrize("tag,kw", [("cond0", dict(temperature=0.0)),
                                    ("condf", dict(temperature=(0.0,), logprob_threshold=-1e9,
                                                   no_speech_threshold=1.0))])
def test_batched_conditioned_long_form_fp32_vs_hf_micro(g, micro32, tag, kw):
    from oracle.weights import CONFIGS
    lv = _assert_fixture_conditions(g, tag, CONFIGS["micro"])
    feats, mask = conditioned_features()
    trace = _check_longform(micro32, g, tag, feats, mask, condition_on_prev_tokens=True, **kw)
    for ix in lv:                     # the windows of one seek iteration ran in one batch
        if len(ix) > 1:
            assert all(trace[i]["batch"] >= len(ix) for i in ix), [trace[i]["batch"] for i in ix]
    assert any(trace[i]["batch"] > 1 for i in range(len(trace)))


def test_batched_conditioned_long_form_fp32_vs_hf_lv2(g):
    """The large-v2 dims (d = 1280, 20 heads): batch-2 decode, rows padded by up to 191 columns."""
    from oracle.weights import CONFIGS
    from prompted_inputs import LV2_PICK, lv2_candidate_features
    from test_batched_longform_gpu import _model
    tag = "lv2_condf"
    assert f"{tag}_ids" in g, "tests/golden/prompted.npz has no large-v2 part"
    lv = _assert_fixture_conditions(g, tag, CONFIGS["large-v2"])
    m = _model("lv2", None)
    feats, mask = lv2_candidate_features(LV2_PICK)
    trace = _check_longform(m, g, tag, feats, mask, condition_on_prev_tokens=True, temperature=(0.0,),
                            logprob_threshold=-1e9, no_speech_threshold=1.0)
    for ix in lv:
        if len(ix) > 1:
            assert all(trace[i]["batch"] >= len(ix) for i in ix)
    assert any(t["batch"] > 1 for t in trace)


@pytest.mark.parametrize("compute", ["bf16", "fp16"])
def test_batched_conditioned_16bit_rows_follow_their_windows(compute):
    """Each row of the batched conditioned call is the decode of its window alone (batch 1) from the prompt the trace
    records, left-padded to the iteration's length as HF pads it (HF 5.15 embeds a padded row at its column index, so
    the padding is part of what the row computes): the windows of each seek iteration are encoded together as the call
    encodes them (the encoder sees the batch), then decoded one by one."""
    import oracle.fixture_inputs as fx
    from test_decode_kstart_gpu import small_model
    from tw.config import GenerationConfig
    from tw.generation import _Decoder, row_tokens, total_length
    cfg, m = small_model("micro", compute)
    m.generation_config = gc = GenerationConfig({k: fx.TS_GENERATION[k] for k in fx.TW_GENERATION_KEYS})
    feats, mask = conditioned_features()
    trace = []
    m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), return_timestamps=True, language="zh",
               task="transcribe", condition_on_prev_tokens=True, temperature=0.0, _trace=trace)
    lv = _levels([t["b"] for t in trace])
    assert any(len({len(trace[i]["prompt"]) for i in ix}) > 1 for ix in lv)       # the padded path ran
    assert any(trace[i]["batch"] > 1 for ix in lv for i in ix)
    fd = torch.from_numpy(feats).to(DEV)
    Tk, eos, pad = cfg["max_source_positions"], int(gc.eos_token_id), int(gc.pad_token_id)
    for ix in lv:
        segb = torch.zeros(len(ix), 80, 3000, device=DEV)
        for r, i in enumerate(ix):
            t = trace[i]
            segb[r, :, :t["n"]] = fd[t["b"], :, t["seek"]:t["seek"] + t["n"]]
        e = m.encode(m.conv_input(segb))
        Pl = max(len(trace[i]["prompt"]) for i in ix)
        ml = total_length(m.config, gc, Pl)
        for r, i in enumerate(ix):
            p = trace[i]["prompt"]
            npad = Pl - len(p)
            dec = _Decoder(m, gc, 1, Tk, Pl, ml, True, True)
            alone = dec.run(e[r * Tk:(r + 1) * Tk], torch.tensor([[pad] * npad + p], device=DEV),
                            pads=[npad])[0].tolist()
            assert row_tokens(alone, eos) == [int(x) for x in trace[i]["raw"]], (i, trace[i]["b"], trace[i]["seek"])


@pytest.mark.parametrize("compute", ["bf16", "fp16"])
def test_batched_conditioned_fallback_attempts_carry_their_rows_prompt(compute):
    """The conditioned batched call under a fallback schedule that fires (the temperatures and thresholds of
    test_batched_longform_16bit_rows_follow_their_windows): the speculative run, which decodes several temperature
    levels of the failing rows as one padded batch, and the level-by-level run, whose batches hold other rows, give the
    same output and the same attempts -- so every attempt of a row decodes from that row's prompt and pad count
    whichever batch it sits in -- and attempts above temperature 0 ran on rows that were left-padded."""
    import oracle.fixture_inputs as fx
    from test_decode_kstart_gpu import small_model
    from tw.config import GenerationConfig
    cfg, m = small_model("micro", compute)
    m.generation_config = GenerationConfig({k: fx.TS_GENERATION[k] for k in fx.TW_GENERATION_KEYS})
    feats, mask = conditioned_features()
    kw = dict(return_timestamps=True, language="zh", task="transcribe", temperature=(0.0, 0.2, 0.4),
              compression_ratio_threshold=1.35, logprob_threshold=-1.0, no_speech_threshold=0.6, seed=5,
              condition_on_prev_tokens=True)
    ta, tb = [], []
    a = m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), _trace=ta, fallback_batch=True,
                   **kw).cpu().numpy()
    b = m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), _trace=tb, fallback_batch=False,
                   **kw).cpu().numpy()
    np.testing.assert_array_equal(a, b)
    acc = lambda tr: sorted((t["b"], t["seek"], t["T"], tuple(t["prompt"]), tuple(t["raw"])) for t in tr)
    assert set(acc(tb)) <= set(acc(ta))
    # not vacuous: a seek iteration whose rows' prompts differ in length made attempts above temperature 0, one of them
    # on a row shorter than the iteration's longest prompt (a padded row), in a batch of several rows
    hit = 0
    for tr in (ta, tb):
        its = _iterations(tr)
        longest = {}
        for t, i in zip(tr, its):
            longest[i] = max(longest.get(i, 0), len(t["prompt"]))
        hit += sum(1 for t, i in zip(tr, its) if t["T"] and len(t["prompt"]) < longest[i] and t["batch"] > 1)
    print(f"{compute}: {len(ta)} / {len(tb)} attempts, {hit} fallback attempts on padded rows")
    assert hit > 0


def _iterations(trace):
    """The seek iteration of each trace record: a new one starts where a recording's temperature-0 attempt repeats."""
    out, seen, cur = [], set(), 0
    for r in trace:
        if not r["T"]:
            if r["b"] in seen:
                cur, seen = cur + 1, set()
            seen.add(r["b"])
        out.append(cur)
    return out
