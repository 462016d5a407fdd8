"""generate(repetition_penalty=, no_repeat_ngram_size=) without a GPU: the oracle of the kernel parity tests against
HF's own processor classes, the argument checks of generate, the long-form plumbing with a scripted decoder, and the
pseudo-labelling flags."""
import types

import numpy as np
import pytest
import torch

import repeat_cases as rc
from tw import generation
from tw.config import GenerationConfig

EOS = 50257


# ------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("vocab", list(rc.VOCABS))
@pytest.mark.parametrize("dtype", rc.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_restatement_equals_hf_processors(vocab, dtype):
    """tests/repeat_cases.py restate() == RepetitionPenaltyLogitsProcessor then NoRepeatNGramLogitsProcessor
    (transformers logits_process.py), bit for bit, on the whole case table."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    V, eos = rc.VOCABS[vocab], rc.EOS[vocab]
    x = rc.score_table(V, dtype)
    changed = banned = 0
    for n, L, p in rc.combos():
        hists = rc.histories(L, V, eos)
        ids = torch.tensor(hists, dtype=torch.int64).reshape(rc.ROWS, L)
        want = x.clone()
        if p != 1.0:
            want = lp.RepetitionPenaltyLogitsProcessor(penalty=p)(ids, want)
        if n > 0:
            want = lp.NoRepeatNGramLogitsProcessor(n)(ids, want)
        got = rc.restate(x, hists, p, n)
        assert rc.same_bits(got, want), (vocab, dtype, n, L, p)
        changed += int(not rc.same_bits(got, x))
        banned += int((torch.isinf(got) & (got < 0) & ~(torch.isinf(x) & (x < 0))).sum())
    assert changed > len(rc.combos()) // 2 and banned > 0        # the table is not vacuous


def test_case_table_covers_what_it_claims():
    V, eos = rc.VOCABS["real"], rc.EOS["real"]
    assert rc.lengths(6) == [0, 1, 4, 5, 6, 447] and rc.lengths(0) == [0, 1, 447] and rc.lengths(2) == [0, 1, 2, 447]
    h = dict(zip(rc.KINDS, rc.histories(447, V, eos)))
    assert len(set(h["same"])) == 1 and len(set(h["norepeat"])) == 447
    assert eos in h["eos_mid"][200:240] and h["edges3_eos_end"][-2:] == [eos, eos]
    assert {0, V - 1} <= set(h["edges"]) and {0, V - 1} <= set(h["pool5"])
    trap = (V - rc.TRAP_OFFSET) % V
    assert all(trap not in r for r in h.values())
    for dt in rc.DTYPES:
        x = rc.score_table(V, dt)
        big = float(torch.finfo(dt).max)
        vals = torch.cat([x[r, [0, 5, V // 2 + 1, V - 7, V - 1, eos]] for r in range(rc.ROWS)])
        assert bool(torch.isnan(vals).any()) and bool((vals == big).any()) and bool((vals == float("-inf")).any())
        assert bool(((vals == 0) & torch.signbit(vals)).any()) and bool(((vals == 0) & ~torch.signbit(vals)).any())
        q = torch.tensor(0.7).to(dt).float()
        assert float((q / torch.tensor(1.3)).double()) != float(q.double()) / float(torch.tensor(1.3).double())


# ------------------------------------------------------------------------------------------ generate's argument checks
def _gc(**extra):
    return GenerationConfig(decoder_start_token_id=50258, eos_token_id=EOS, pad_token_id=EOS,
                            no_timestamps_token_id=50363, suppress_tokens=[], lang_to_id={"<|zh|>": 50260}, **extra)


def _model(**gc_extra):
    cfg = types.SimpleNamespace(max_source_positions=1500, max_target_positions=448, vocab_size=51865, d_model=128,
                                eos_token_id=EOS)
    return types.SimpleNamespace(config=cfg, device=torch.device("cpu"), compute="bf16",
                                 generation_config=_gc(**gc_extra))


FEATS = torch.zeros(1, 80, 3000)


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.3), dict(repetition_penalty=2),
                                dict(repetition_penalty="1.3"), dict(repetition_penalty=float("nan")),
                                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0),
                                dict(no_repeat_ngram_size="2"), dict(no_repeat_ngram_size=True)])
def test_bad_values_raise_value_error(kw):
    with pytest.raises(ValueError, match=list(kw)[0]):
        generation.generate(_model(), FEATS, language="zh", **kw)


def test_generation_config_supplies_the_defaults():
    """Named in generation_config and not passed: the config's value is taken (and checked) as HF takes it; the call's
    keyword wins over the config's."""
    with pytest.raises(ValueError, match="repetition_penalty"):
        generation.generate(_model(repetition_penalty=0.0), FEATS, language="zh")
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        generation.generate(_model(no_repeat_ngram_size=3), FEATS, language="zh", num_beams=2)
    assert generation.repeat_options(_gc(repetition_penalty=1.2, no_repeat_ngram_size=3), {}) == (1.2, 3)
    assert generation.repeat_options(_gc(repetition_penalty=1.2), dict(repetition_penalty=1.5)) == (1.5, 0)
    assert generation.repeat_options(_gc(), {}) == (1.0, 0)
    assert generation.repeat_options(_gc(), dict(repetition_penalty=1, no_repeat_ngram_size=0)) == (1.0, 0)


@pytest.mark.parametrize("kw,names", [(dict(repetition_penalty=1.3), ["repetition_penalty"]),
                                      (dict(no_repeat_ngram_size=2), ["no_repeat_ngram_size"]),
                                      (dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
                                       ["repetition_penalty", "no_repeat_ngram_size"])])
def test_beam_and_assistant_are_not_implemented(kw, names):
    with pytest.raises(NotImplementedError) as e:
        generation.generate(_model(), FEATS, language="zh", num_beams=2, **kw)
    assert all(n in str(e.value) for n in names) and "beam" in str(e.value)
    assistant = types.SimpleNamespace(config=_model().config, generation_config=None, decoder_only=False)
    with pytest.raises(NotImplementedError) as e:
        generation.generate(_model(), FEATS, language="zh", assistant_model=assistant, **kw)
    assert all(n in str(e.value) for n in names) and "assist" in str(e.value)


def test_unknown_keyword_still_raises_type_error():
    with pytest.raises(TypeError, match="repetition_penalti"):
        generation.generate(_model(), FEATS, language="zh", repetition_penalti=1.3)
    with pytest.raises(TypeError, match="encoder_repetition_penalty"):
        generation.generate(_model(), FEATS, language="zh", repetition_penalty=1.3, encoder_repetition_penalty=1.1)


# ------------------------------------------------------------------------------------------ long-form plumbing
def test_long_form_builds_its_decoders_with_the_options(monkeypatch):
    """Every decoder of a long-form call (the window's and the fallback batch's) is built with the two options, passed
    plainly; with both off they are (1.0, 0), the values with which _Select launches no pre-pass."""
    from test_generation_cpu import _ScriptedDecoder, _script
    from test_generation_cpu import _model as scripted_model
    built = []

    class _Recording(_ScriptedDecoder):
        def __init__(self, *a, **kw):
            built.append(dict(kw))
            super().__init__(*a)

    monkeypatch.setattr(generation, "_Decoder", _Recording)
    _ScriptedDecoder.script = _script()
    feats = torch.zeros(1, 80, 6000)
    feats[..., 3000:] = 1.0
    m = scripted_model()
    m.generation_config = _gc()
    common = dict(attention_mask=None, return_timestamps=True, language="zh", task="transcribe", max_new_tokens=40,
                  use_graph=False, temperature=(0.0, 0.2, 0.4, 0.6), compression_ratio_threshold=1.35)
    on = generation.generate(m, feats, repetition_penalty=1.3, no_repeat_ngram_size=2, **common)
    assert len(built) >= 2 and all(k == dict(repetition_penalty=1.3, no_repeat_ngram_size=2) for k in built)
    del built[:]
    off = generation.generate(m, feats, repetition_penalty=1.0, no_repeat_ngram_size=0, **common)
    assert len(built) >= 2 and all(k == dict(repetition_penalty=1.0, no_repeat_ngram_size=0) for k in built)
    assert torch.equal(on, off)                                   # the scripted decoder ignores the options


# ------------------------------------------------------------------------------------------ the labelling driver
def test_pseudo_labelling_flags_reach_generate():
    from tw import pseudo_labelling as pl
    a = pl.parse_args([])
    assert (a.repetition_penalty, a.no_repeat_ngram_size) == (1.0, 0)
    a = pl.parse_args(["--repetition_penalty", "1.3", "--no_repeat_ngram_size", "3"])
    assert (a.repetition_penalty, a.no_repeat_ngram_size) == (1.3, 3) and isinstance(a.repetition_penalty, float)
    seen = {}

    class _M:
        def generate(self, mel, **kw):
            seen.update(kw)
            return torch.tensor([[7, 8, EOS, EOS]])

    class _FE:
        def pad_waveforms(self, chunks):
            return chunks

        def extract(self, wav, want_conv_input=False):
            return torch.zeros(1, 80, 3000), None

    tr = pl.ChunkTranscriber.__new__(pl.ChunkTranscriber)
    tr.m, tr.fe, tr.eot, tr.language, tr.max_new_tokens = _M(), _FE(), EOS, "zh", 24
    tr.repetition_penalty, tr.no_repeat_ngram_size = a.repetition_penalty, a.no_repeat_ngram_size
    assert tr([np.zeros(16000, dtype=np.float32)]) == [[7, 8]]
    assert seen["repetition_penalty"] == 1.3 and seen["no_repeat_ngram_size"] == 3
    import inspect
    sig = inspect.signature(pl.ChunkTranscriber.__init__).parameters
    assert sig["repetition_penalty"].default == 1.0 and sig["no_repeat_ngram_size"].default == 0
