"""detect_language and generate(language="auto" / [...]) on the GPU, micro model.

* fp32 against HF's own calls (tests/golden/langid.npz, tests/golden/make_golden_langid.py: HF Transformers 5.15 fp32
  on the CPU, language=None there): detect_language's ids, every short-form case, the per-row list, the long-form
  calls window by window, and return_language.
* every compute mode against the engine itself: "auto" equals language=[its own detected ids], graph equals eager,
  the prefill-fused detection equals detect_language on the same encoder rows, on 16-bit the detected ids equal the
  restatement (tests/langid_cases.py) on the step's own logits, mixed-language batch rows equal their batch-1
  decodes where rows are independent, assisted equals unassisted, beam search with one language equals the fixed
  call and raises on mixed ones."""
import numpy as np
import pytest
import torch

import langid_cases as lc
from conftest import load_golden
from langid_inputs import LANG_TO_ID, LIST_LANGUAGES, LONG, LONG_INPUTS, SHORT
from prompted_inputs import PROMPT_IDS, conditioned_features

pytestmark = pytest.mark.gpu
DEV = "cuda"
COMPUTES = ("fp32", "bf16", "fp16")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g():
    return load_golden("langid")


_models = {}


def _model(compute):
    """The micro model of the fixtures with the 99 language ids in its generation config, one per compute mode."""
    if compute not in _models:
        import oracle.fixture_inputs as fx
        from test_decode_kstart_gpu import small_model
        from tw.config import GenerationConfig
        cfg, m = small_model("micro", compute)
        gc = {k: fx.TS_GENERATION[k] for k in fx.TW_GENERATION_KEYS}
        gc["lang_to_id"] = dict(LANG_TO_ID)
        m.generation_config = GenerationConfig(gc)
        _models[compute] = m
    return _models[compute]


def _feats():
    from test_decode_gpu import _feats as f
    return f()


def _extra(prompted):
    return dict(prompt_ids=torch.tensor(PROMPT_IDS)) if prompted else {}


# ------------------------------------------------------------------------------------------ fp32 against HF
def test_detect_language_fp32_vs_hf(g):
    m = _model("fp32")
    ids = m.detect_language(_feats())
    assert ids.dtype == torch.int64 and ids.is_cuda
    np.testing.assert_array_equal(ids.cpu().numpy(), g["detect_ids"])
    assert len(set(g["detect_ids"].tolist())) > 1                      # not vacuous: the rows' languages differ
    ids2, probs, table = m.detect_language(_feats(), return_probs=True)
    assert torch.equal(ids, ids2) and table == sorted(LANG_TO_ID.values()) and tuple(probs.shape) == (3, 99)
    p = probs.cpu()
    assert torch.allclose(p.sum(1), torch.ones(3), atol=1e-5)
    assert [table[int(j)] for j in p.argmax(1)] == ids.tolist()
    enc = m.encode(m.conv_input(_feats())).view(3, -1, m.config.d_model)
    assert torch.equal(m.detect_language(encoder_outputs=(enc,)), ids)
    with pytest.raises(ValueError, match="either"):
        m.detect_language()
    with pytest.raises(ValueError, match="only one"):
        m.detect_language(_feats(), encoder_outputs=(enc,))


@pytest.mark.parametrize("tag", list(SHORT))
def test_short_form_fp32_vs_hf(g, tag):
    m = _model("fp32")
    kw, prompted = SHORT[tag]
    language = LIST_LANGUAGES if tag == "list" else "auto"
    got, lang = m.generate(_feats(), language=language, return_language=True, **kw, **_extra(prompted))
    np.testing.assert_array_equal(got.cpu().numpy(), g[f"{tag}_ids"])
    want = [LANG_TO_ID[f"<|{c}|>"] for c in LIST_LANGUAGES] if tag == "list" else g["detect_ids"].tolist()
    assert lang.dtype == torch.int64 and lang.tolist() == want
    zh = m.generate(_feats(), language="zh", **kw, **_extra(prompted)).cpu().numpy()
    n = min(zh.shape[1], got.shape[1])
    assert zh.shape != tuple(got.shape) or bool((zh[:, :n] != got.cpu().numpy()[:, :n]).any())


@pytest.mark.parametrize("tag", list(LONG))
def test_long_form_fp32_vs_hf(g, tag):
    from test_prompted_gpu import _rows
    m = _model("fp32")
    lens, seed = LONG_INPUTS
    feats, mask = conditioned_features(lens=lens, seed=seed)
    trace = []
    out, lang = m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), return_timestamps=True,
                           language="auto", return_language=True, _trace=trace, **LONG[tag])
    assert lang.tolist() == g["lf_lang_ids"].tolist() and len(set(lang.tolist())) > 1
    assert [(t["b"], t["seek"]) for t in trace] == list(zip(g[f"{tag}_win_b"].tolist(), g[f"{tag}_win_seek"].tolist()))
    assert [t["prompt"] for t in trace] == _rows(g[f"{tag}_win_prompt"])
    assert [[int(x) for x in t["raw"]] for t in trace] == _rows(g[f"{tag}_win_ids"])
    np.testing.assert_array_equal(out.cpu().numpy(), g[f"{tag}_ids"])


# ------------------------------------------------------------------------------------------ every compute mode
@pytest.mark.parametrize("compute", COMPUTES)
def test_auto_equals_its_own_languages_graph_equals_eager(compute):
    m = _model(compute)
    kw = dict(task="transcribe", max_length=40)
    a, lang = m.generate(_feats(), language="auto", return_language=True, use_graph=True, **kw)
    b = m.generate(_feats(), language="auto", use_graph=False, **kw)
    c, lang_c = m.generate(_feats(), language=lang.tolist(), return_language=True, **kw)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(lang, lang_c)
    # with prompt_ids the languages come from the separate pass: the same ids, and the same decode as the list form
    d, lang_d = m.generate(_feats(), language="auto", return_language=True, prompt_ids=torch.tensor(PROMPT_IDS), **kw)
    e = m.generate(_feats(), language=lang.tolist(), prompt_ids=torch.tensor(PROMPT_IDS), **kw)
    assert torch.equal(lang_d, lang) and torch.equal(d, e)


@pytest.mark.parametrize("compute", COMPUTES)
def test_fused_column_equals_detect_language_and_the_restatement(compute):
    """The prefill-fused detection writes into column 1 what detect_language gives on the same encoder rows; on every
    mode both equal the restatement applied to the detection step's own logits, read back."""
    from tw.generation import DecodeSession
    m = _model(compute)
    enc16 = m.encode(m.conv_input(_feats()))
    enc = enc16.view(3, -1, m.config.d_model)
    keep = []
    out = m.generate(encoder_outputs=(enc,), language="auto", task="transcribe", max_length=24, _keep=keep)
    col1 = keep[0].sel.ids[:, 1].clone()
    ids, probs, table = m.detect_language(encoder_outputs=(enc,), return_probs=True)
    assert torch.equal(col1, ids) and out.shape[0] == 3
    assert keep[0].sel.ids[:, 0].tolist() == [50258] * 3 and keep[0].sel.ids[:, 2].tolist() == [50359] * 3
    sess = DecodeSession(m, enc16, 3, enc.shape[1], 2)
    sess.cur.fill_(50258)
    sess.step()
    x = sess.logits[:, :m.config.vocab_size].float().cpu()
    want, p64 = lc.lang_detect_ref(x, table)
    assert ids.cpu().tolist() == want.tolist()
    assert bool(((probs.cpu().double() - p64).abs() <= lc.prob_bound(x, table, p64)).all())


@pytest.mark.parametrize("compute", ["bf16", "fp16"])
def test_mixed_language_rows_equal_their_batch1_decodes(compute):
    from tw.generation import batch_rows_independent, row_tokens
    m = _model(compute)
    assert batch_rows_independent(m)
    kw = dict(task="transcribe", max_length=40)
    eos = int(m.generation_config.eos_token_id)
    rows = m.generate(_feats(), language=LIST_LANGUAGES, **kw).cpu().tolist()
    for r, lang in enumerate(LIST_LANGUAGES):
        alone = m.generate(_feats()[r:r + 1], language=lang, **kw).cpu().tolist()[0]
        assert row_tokens(rows[r], eos) == row_tokens(alone, eos), (compute, r)
    assert row_tokens(rows[0], eos) != row_tokens(m.generate(_feats()[:1], language="en", **kw).cpu().tolist()[0], eos)


@pytest.mark.parametrize("compute", COMPUTES)
def test_assisted_auto_equals_unassisted(compute):
    """The unassisted call detects inside the prefill, the assisted one in the separate pass."""
    m = _model(compute)
    kw = dict(language="auto", task="transcribe", max_length=40, return_language=True)
    f1 = _feats()[1:2]
    a, la = m.generate(f1, **kw)
    b, lb = m.generate(f1, assistant_model=m, num_assistant_tokens=3, **kw)
    assert torch.equal(a, b) and torch.equal(la, lb)


@pytest.mark.parametrize("compute", COMPUTES)
def test_beam_search_one_language_and_mixed(compute):
    m = _model(compute)
    kw = dict(task="transcribe", max_length=32, num_beams=2)
    f = _feats()
    lang = m.detect_language(f).tolist()
    assert lang[0] == lang[2] != lang[1]
    same = torch.stack([f[0], f[2]])
    a, la = m.generate(same, language="auto", return_language=True, **kw)
    b = m.generate(same, language=lang[0], **kw)
    assert torch.equal(a, b) and la.tolist() == [lang[0], lang[0]]
    assert torch.equal(a, m.generate(same, language=[lang[0], lang[0]], **kw))
    with pytest.raises(NotImplementedError, match="different languages"):
        m.generate(f, language="auto", **kw)
    with pytest.raises(NotImplementedError, match="different languages"):
        m.generate(f, language=["zh", "en", "zh"], **kw)
