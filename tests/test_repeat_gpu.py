"""generate(repetition_penalty=, no_repeat_ngram_size=) on the GPU.

* fp32 against HF's own calls (tests/golden/repeat.npz, tests/golden/make_golden_repeat.py: HF Transformers 5.15 fp32
  on the CPU): the ids of every fixture case; for the long-form cases also windows, seeks, prompts and, where HF's gate
  recorded them, the per-window avg_logprob / no-speech probability within the bar of tests/test_prompted_gpu.py.
* bf16 / fp16 against the engine's own logits (HF's 16-bit logits differ before any processor runs): every token of an
  eager decode equals tests/repeat_cases.py restate() followed by the selection oracle of tests/select_cases.py on
  that step's logits.
* graph against eager, a decoder reused across windows, batch rows against their batch-1 decode (one row sampled),
  and off means off.
"""
import numpy as np
import pytest
import torch

import repeat_cases as rc
import select_cases as sc
from conftest import load_golden
from prompted_inputs import PROMPT_IDS, conditioned_features
from repeat_inputs import BOTH, LONG, LONG_INPUTS, OPTION_KEYS, SHORT

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g():
    return load_golden("repeat")


@pytest.fixture(scope="module")
def micro32():
    from test_batched_longform_gpu import _model
    return _model("micro", None)


def _without(kw):
    return {k: v for k, v in kw.items() if k not in OPTION_KEYS}


def _differs(a, b):
    n = min(a.shape[1], b.shape[1])
    return a.shape != b.shape or bool((a[:, :n] != b[:, :n]).any())


# ------------------------------------------------------------------------------------------ fp32 against HF
@pytest.mark.parametrize("tag", list(SHORT))
def test_short_form_fp32_vs_hf(g, micro32, tag):
    from test_decode_gpu import _feats
    n, kw, prompted = SHORT[tag]
    extra = dict(prompt_ids=torch.tensor(PROMPT_IDS)) if prompted else {}
    got = micro32.generate(_feats()[:n], **kw, **extra).cpu().numpy()
    np.testing.assert_array_equal(got, g[f"{tag}_ids"])
    plain = micro32.generate(_feats()[:n], **_without(kw), **extra).cpu().numpy()
    assert _differs(got, plain)                                    # not vacuous: the options change the decode


@pytest.mark.parametrize("tag", list(LONG))
def test_long_form_fp32_vs_hf(g, micro32, tag):
    from test_prompted_gpu import _check_longform, _rows
    lens, seed = LONG_INPUTS[tag]
    feats, mask = conditioned_features(lens=lens, seed=seed)
    trace = _check_longform(micro32, g, tag, feats, mask, **LONG[tag])
    assert all(not t["T"] for t in trace)                          # no fallback: one attempt per window
    if tag == "cond3":                                             # rows left-padded in one decode batch
        prompts = _rows(g[f"{tag}_win_prompt"])
        assert any(len(p) < int(pl) for p, pl in zip(prompts, g[f"{tag}_win_plen"]))
        assert any(t["batch"] > 1 for t in trace)
    else:
        assert len(trace) >= 2 and f"{tag}_win_avg" in g and f"{tag}_win_ns" in g


# ------------------------------------------------------------------------------------------ 16-bit: own logits
def _stepwise(m, gc, enc16, Tk, prompt, new, ts, penalty, ngram):
    """An eager decode of `new` steps with the decoder's own calls -> (ids [B, P + new], per-step logits [B, V])."""
    from tw.generation import _Decoder
    B, P = prompt.shape
    dec = _Decoder(m, gc, B, Tk, P, P + new, ts, False, repetition_penalty=penalty, no_repeat_ngram_size=ngram)
    sel = dec.sel
    sess = dec.sess = dec._open(None, m, enc16, Tk)
    sess.set_pads(None, False)
    sel.reset(prompt.to(DEV))
    dec._prefill([sess], None)
    sess.cur.copy_(sel.ids[:, P - 1])
    V = m.config.vocab_size
    logits = []
    for _ in range(new):
        sess.step(sel)
        logits.append(sess.logits[:, :V].float().cpu())
    return sel.ids.cpu(), logits


@pytest.mark.parametrize("ts", [False, True], ids=["plain", "timestamps"])
@pytest.mark.parametrize("compute", ["bf16", "fp16"])
def test_16bit_tokens_follow_the_engines_own_logits(compute, ts):
    import oracle.fixture_inputs as fx
    from test_decode_gpu import _feats
    from test_decode_kstart_gpu import small_model
    from tw.config import GenerationConfig
    cfg, m = small_model("micro", compute)
    gc = GenerationConfig({k: fx.TS_GENERATION[k] for k in fx.TW_GENERATION_KEYS})
    enc16 = m.encode(m.conv_input(_feats()[:2]))
    no_ts = int(gc.no_timestamps_token_id)
    prompt = [50361, 1000, 1037, 50258, 50260, 50359] + ([] if ts else [no_ts])
    B, P, new = 2, len(prompt), 24
    penalty, ngram = BOTH["repetition_penalty"], BOTH["no_repeat_ngram_size"]
    ids, logits = _stepwise(m, gc, enc16, cfg["max_source_positions"], torch.tensor([prompt] * B), new, ts, penalty,
                            ngram)
    eos = int(gc.eos_token_id)
    voc = sc.Vocab("micro", cfg["vocab_size"], m.Vp, eos, no_ts, no_ts + 1, tuple(gc.suppress_tokens),
                   tuple(gc.begin_suppress_tokens), no_ts + 100)
    mi = gc.max_initial_timestamp_index if "max_initial_timestamp_index" in gc else None
    changed = 0
    for b in range(B):
        done = False
        for s in range(new):
            col = P + s
            hist = ids[b, :col].tolist()
            got = int(ids[b, col])
            if done:
                assert got == eos
                continue
            x = rc.restate(logits[s][b:b + 1], [hist], penalty, ngram)[0]
            changed += int(not rc.same_bits(x, logits[s][b]))
            grp = sc.Group("step", voc, ts, P, col, -1 if mi is None else int(mi), True, [])
            row = sc.Row("r", x, gen=hist[P:], prompt=tuple(hist[:P]))
            want = sc.reference(grp, row, torch.float32)["tok"]
            if got != want and ts and sc.mass_margin(grp, row, torch.float32) < sc.MASS_MARGIN:
                # the timestamp-mass decision within the selection tests' own margin: either branch
                want = sc.lowest_argmax(sc.processed_row(grp, row, torch.float32, apply_mass=False))
            assert got == want, (compute, ts, b, s, got, want)
            done = got == eos
    assert changed >= new                                           # the pre-pass changed the rows it was given


# ------------------------------------------------------------------------------------------ graph, reuse, batch, off
def test_graph_equals_eager_and_a_reused_decoder(micro32):
    from test_decode_gpu import _feats, _ts_model
    mg, cfg, w, m = _ts_model()
    for kw in (dict(language="zh", task="transcribe", max_length=48), ):
        a = m.generate(_feats(), use_graph=True, **BOTH, **kw).cpu()
        b = m.generate(_feats(), use_graph=False, **BOTH, **kw).cpu()
        assert torch.equal(a, b)
        assert _differs(a.numpy(), m.generate(_feats(), **kw).cpu().numpy())
    # long-form without conditioning: every window has the same prompt, so one decoder (one captured step, one
    # scratch) serves them all
    lf = torch.from_numpy(mg.longform_features())
    kw = dict(attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True, language="zh",
              task="transcribe", max_new_tokens=32)
    ta, tb = [], []
    a = m.generate(lf, use_graph=True, _trace=ta, **BOTH, **kw).cpu()
    b = m.generate(lf, use_graph=False, _trace=tb, **BOTH, **kw).cpu()
    assert torch.equal(a, b) and len(ta) >= 2 and [t["raw"] for t in ta] == [t["raw"] for t in tb]
    assert len({len(t["prompt"]) for t in ta}) == 1
    assert _differs(a.numpy(), m.generate(lf, **kw).cpu().numpy())


@pytest.mark.parametrize("compute", ["bf16", "fp16"])
def test_batch_rows_equal_their_batch1_decode(compute):
    """Rows of one batch (two greedy, one sampled at T = 0.7 with its own seed) decode what each decodes alone."""
    import oracle.fixture_inputs as fx
    from test_decode_gpu import _feats
    from test_decode_kstart_gpu import small_model
    from tw.config import GenerationConfig
    from tw.generation import _Decoder, batch_rows_independent, row_tokens
    cfg, m = small_model("micro", compute)
    assert batch_rows_independent(m)
    gc = GenerationConfig({k: fx.TS_GENERATION[k] for k in fx.TW_GENERATION_KEYS})
    Tk = cfg["max_source_positions"]
    enc = m.encode(m.conv_input(_feats()[:1]))                     # one window shared by the rows, as a fallback batch
    prompt = [50258, 50260, 50359]
    P, new = len(prompt), 32
    temps, seeds = [0.0, 0.0, 0.7, 0.0], [3, 4, 5, 6]
    eos = int(gc.eos_token_id)
    for use_graph in (True, False):
        batch = _Decoder(m, gc, 4, Tk, P, P + new, True, use_graph, True, **BOTH)
        rows = batch.run(enc, torch.tensor([prompt] * 4, device=DEV), temperature=temps, seed=seeds).cpu().tolist()
        slp = batch.sel.sum_logp.cpu().tolist()
        one = _Decoder(m, gc, 1, Tk, P, P + new, True, use_graph, True, **BOTH)
        for r in (0, 2):
            alone = one.run(enc, torch.tensor([prompt], device=DEV), temperature=temps[r], seed=seeds[r]).cpu().tolist()
            assert row_tokens(rows[r], eos) == row_tokens(alone[0], eos), (compute, use_graph, r)
            assert slp[r] == float(one.sel.sum_logp[0])
        assert row_tokens(rows[0], eos) != row_tokens(rows[2], eos)     # the sampled row is another decode


def test_off_means_off(micro32):
    from test_decode_gpu import _feats
    kw = dict(language="zh", task="transcribe", max_length=48)
    keep_a, keep_b, keep_c = [], [], []
    a = micro32.generate(_feats(), _keep=keep_a, **kw).cpu()
    b = micro32.generate(_feats(), repetition_penalty=1.0, no_repeat_ngram_size=0, _keep=keep_b, **kw).cpu()
    assert torch.equal(a, b)
    assert keep_a[0].sel.scratch is None and keep_b[0].sel.scratch is None and not keep_b[0].sel.repeat
    c = micro32.generate(_feats(), _keep=keep_c, **BOTH, **kw).cpu()
    sel = keep_c[0].sel
    assert sel.repeat and sel.scratch.dtype == torch.float32 and tuple(sel.scratch.shape) == (3, micro32.Vp)
    assert _differs(a.numpy(), c.numpy())
