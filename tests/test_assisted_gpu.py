"""Assisted (speculative) decoding on the GPU: generate(assistant_model=...) returns exactly the ids of the same call
without an assistant (HF generate(assistant_model=...), run_eval.py:524-545,653-654) -- bf16, fp16 and fp32, with and
without timestamps, 1 / 4 / 7 drafted tokens a round, captured round and eager -- for three assistants: the target's
own weights (every draft must be accepted: each accepted position's logits are bit-identical to the plain decode's),
an unrelated random model (rounds that reject), and a 2-layer student as a decoder-only WhisperForCausalLM over the
target's encoder output.  Micro models, as tests/test_decode_gpu.py builds them."""
import math
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
EOS = 50257
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _target(mode):
    """mode: 'bf16' (fp32 master, bf16 autocast), 'fp16' (an fp16 model), 'fp32'."""
    if ("t", mode) not in _CACHE:
        import oracle.fixture_inputs as mg
        from test_decode_gpu import _micro
        cfg, w, m, GC = _micro(dtype=torch.float16 if mode == "fp16" else torch.float32)
        if mode == "fp32":
            m.set_compute("fp32")
        m.generation_config = GC({k: mg.TS_GENERATION[k] for k in mg.TW_GENERATION_KEYS})
        _CACHE[("t", mode)] = (cfg, m, GC)
    return _CACHE[("t", mode)]


def _assistant(mode, kind):
    if (kind, mode) in _CACHE:
        return _CACHE[(kind, mode)]
    from oracle.weights import make_weights
    from tw.config import WhisperConfig
    from tw.modeling import WhisperForCausalLM, WhisperForConditionalGeneration
    from tw.student import init_student_model_from_teacher
    cfg, m, GC = _target(mode)
    dt = torch.float16 if mode == "fp16" else torch.float32
    if kind == "self":
        a = m
    elif kind == "random":
        w = make_weights(cfg, 7, lin_std=0.2)
        a = WhisperForConditionalGeneration.from_state_dict(WhisperConfig(**cfg),
                                                            {k: torch.from_numpy(v) for k, v in w.items()}, dtype=dt)
        a.generation_config = GC(dict(m.generation_config))
    else:
        st = init_student_model_from_teacher(m, decoder_layers=2)
        a = WhisperForCausalLM.from_state_dict(st.config, st.state_dict(), dtype=dt)
        a.generation_config = GC(dict(m.generation_config))
    if a is not m and mode == "fp32":
        a.set_compute("fp32")
    _CACHE[(kind, mode)] = a
    return a


def _feat1():
    if "feat" not in _CACHE:
        from test_decode_gpu import _feats
        _CACHE["feat"] = _feats()[:1]
    return _CACHE["feat"]


def _kwargs(ts):
    if ts:
        return dict(return_timestamps=True, language="zh", task="transcribe", max_new_tokens=30)
    return dict(language="zh", task="transcribe", max_new_tokens=30)


def _plain(mode, ts):
    if ("plain", mode, ts) not in _CACHE:
        cfg, m, GC = _target(mode)
        trace = []
        out = m.generate(_feat1(), _trace=trace, **_kwargs(ts)).cpu()
        _CACHE[("plain", mode, ts)] = (out, trace)
    return _CACHE[("plain", mode, ts)]


def _check_full_acceptance(accepted, L, k, ended_on_eos):
    """The target's own weights as the assistant: every round accepts all k drafts and there are ceil(L / (k + 1))
    rounds.  The one exception is by the kernel's rule (the count stops at the first eos): the round that emits eos
    counts the drafts up to and including it."""
    R = math.ceil(L / (k + 1))
    assert len(accepted) == R, (accepted, L, k)
    assert all(n == k for n in accepted[:-1]), accepted
    rest = L - (R - 1) * (k + 1)
    assert accepted[-1] == (min(rest, k) if ended_on_eos else k), (accepted, L, k)


@pytest.mark.parametrize("kind", ["self", "random", "student"])
@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
def test_assisted_equals_plain(mode, ts, kind):
    cfg, m, GC = _target(mode)
    a = _assistant(mode, kind)
    want, want_trace = _plain(mode, ts)
    assert want.shape[1] >= 8                       # several rounds at every k
    some_rejected = False
    for k in (1, 4, 7):
        for use_graph in (True, False):
            trace = []
            got = m.generate(_feat1(), assistant_model=a, num_assistant_tokens=k, use_graph=use_graph, _trace=trace,
                             **_kwargs(ts)).cpu()
            assert torch.equal(got, want), (k, use_graph)
            rounds = [t for t in trace if "accepted" in t]
            assert rounds and all(0 <= n <= k for t in rounds for n in t["accepted"])
            if ts:                          # one traced entry per window, as without an assistant
                assert [(t["seek"], t["raw"]) for t in trace] == [(t["seek"], t["raw"]) for t in want_trace]
                raws = [t["raw"] for t in trace]
            else:
                raws = [got[0].tolist()]
            for t, raw in zip(rounds, raws):
                L = len(raw)
                if kind in ("self", "student"):     # the 2-layer student of a 2-layer teacher is the teacher's decoder
                    _check_full_acceptance(t["accepted"], L, k, raw[-1] == EOS)
                elif k > 1:
                    some_rejected = some_rejected or any(n < k for n in t["accepted"])
    if kind == "random":
        assert some_rejected


def test_fp32_matches_hf_fixtures():
    """On the fp32 path the assisted ids are also HF's: the fixtures the plain decode is pinned to."""
    from test_decode_gpu import _feats
    import oracle.fixture_inputs as mg
    from tw.generation import row_tokens
    cfg, m, GC = _target("fp32")
    a = _assistant("fp32", "random")
    keep = m.generation_config
    g = load_golden("greedy")
    try:
        m.generation_config = GC(suppress_tokens=g["suppress"].tolist(), begin_suppress_tokens=[220, 50257])
        a.generation_config = None
        gen = m.generate(_feats()[:1], decoder_input_ids=torch.tensor([g["greedy_prompt"].tolist()]), max_length=64,
                         assistant_model=a).cpu()[0].tolist()
        assert gen == row_tokens(g["greedy_ids"][0].tolist(), EOS)
    finally:
        m.generation_config = keep
        a.generation_config = GC(dict(keep))
    g = load_golden("greedy_ts")
    lf = torch.from_numpy(mg.longform_features())
    out = m.generate(lf, attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True,
                     language="zh", task="transcribe", assistant_model=a).cpu()
    np.testing.assert_array_equal(out.numpy(), g["ts_long_ids"])


@pytest.mark.parametrize("kind", ["self", "random"])
def test_max_length_mid_round(kind):
    cfg, m, GC = _target("bf16")
    a = _assistant("bf16", kind)
    for n in (1, 7, 11):
        kw = dict(language="zh", task="transcribe", max_new_tokens=n)
        want = m.generate(_feat1(), **kw).cpu()
        got = m.generate(_feat1(), assistant_model=a, num_assistant_tokens=4, **kw).cpu()
        assert torch.equal(got, want), n
    # the length cap at the end of the position table: the spare rows of a round clamp their positions
    kw = dict(language="zh", task="transcribe", max_length=448)
    want = m.generate(_feat1(), **kw).cpu()
    got = m.generate(_feat1(), assistant_model=a, num_assistant_tokens=7, **kw).cpu()
    assert torch.equal(got, want)


@pytest.mark.parametrize("cond", [False, True])
def test_longform_fallback_with_assistant(cond):
    """The long-form fixture call of tests/test_fallback_gpu.py (seek loop, temperature fallback, thresholds; and
    with conditioning on the previous text): the same ids, the same traced windows, seeks, temperatures and prompts,
    and equal average log-prob and no-speech probability per attempt."""
    import oracle.fixture_inputs as mg
    cfg, m, GC = _target("bf16")
    a = _assistant("bf16", "random")
    lf = torch.from_numpy(mg.longform_features())
    kw = dict(attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True, language="zh",
              task="transcribe", temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold=1.35,
              logprob_threshold=-1.0, no_speech_threshold=0.6, max_new_tokens=40, seed=5,
              condition_on_prev_tokens=cond)
    ta, tb = [], []
    want = m.generate(lf, _trace=tb, **kw).cpu()
    got = m.generate(lf, _trace=ta, assistant_model=a, **kw).cpu()
    assert torch.equal(got, want)
    assert len(ta) == len(tb) and any("accepted" in t for t in ta)
    for x, y in zip(ta, tb):
        assert (x["seek"], x["n"], x["T"], x["prompt"], x["raw"]) == (y["seek"], y["n"], y["T"], y["prompt"], y["raw"])
        assert x["avg_logprob"] == y["avg_logprob"] and x["no_speech_prob"] == y["no_speech_prob"]
        assert (x["needs_fallback"], x["skip"]) == (y["needs_fallback"], y["skip"])
        assert ("accepted" in x) == (not x["T"])           # the temperature-0 attempt is the assisted one


def test_decoder_only_assistant_casts_the_encoder_output():
    """A bf16 WhisperForCausalLM under an fp32 target: the target's encoder rows are cast to the assistant's dtype."""
    from tw.modeling import WhisperForCausalLM
    cfg, m, GC = _target("fp32")
    src = _assistant("fp32", "random")
    a = WhisperForCausalLM.from_state_dict(src.config, src.state_dict(), dtype=torch.bfloat16)
    kw = _kwargs(False)
    got = m.generate(_feat1(), assistant_model=a, **kw).cpu()
    assert torch.equal(got, _plain("fp32", False)[0])
    with pytest.raises(RuntimeError, match="no encoder"):
        a.encode(None)


@pytest.mark.parametrize("stream", ["bf16", "fp32"])
def test_gemv_verify_pass(stream):
    """d_model = 256: the decode step's Linears are GEMV launches (with the fused LayerNorm and KV append when the
    residual stream is 16-bit), so the verify pass runs them with M = Q rows and appends Q cache rows at once."""
    from oracle.weights import CONFIGS, make_weights
    from tw.config import GenerationConfig, WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration
    import oracle.fixture_inputs as mg
    cfg = dict(CONFIGS["micro"], d_model=256, encoder_attention_heads=4, decoder_attention_heads=4,
               encoder_ffn_dim=512, decoder_ffn_dim=512)
    dt = torch.bfloat16 if stream == "bf16" else torch.float32
    mk = lambda seed: WhisperForConditionalGeneration.from_state_dict(
        WhisperConfig(**cfg), {k: torch.from_numpy(v) for k, v in make_weights(cfg, seed, lin_std=0.15).items()}, dtype=dt)
    m, r = mk(3), mk(4)
    m.generation_config = GenerationConfig({k: mg.TS_GENERATION[k] for k in mg.TW_GENERATION_KEYS})
    for ts in (False, True):
        want = m.generate(_feat1(), **_kwargs(ts)).cpu()
        for a, k in ((m, 7), (m, 2), (r, 4)):
            trace = []
            got = m.generate(_feat1(), assistant_model=a, num_assistant_tokens=k, _trace=trace, **_kwargs(ts)).cpu()
            assert torch.equal(got, want), (ts, k)
            if a is m:
                assert all(n == k for t in trace if "accepted" in t for n in t["accepted"][:-1])


def test_argument_errors():
    cfg, m, GC = _target("bf16")
    a = _assistant("bf16", "random")
    from test_decode_gpu import _feats
    with pytest.raises(ValueError, match="batch size 1"):
        m.generate(_feats()[:2], assistant_model=a, language="zh", task="transcribe", max_new_tokens=4)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(_feat1(), assistant_model=a, num_beams=2, language="zh", task="transcribe", max_new_tokens=4)
    other = types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=51864, d_model=128), generation_config=None)
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(_feat1(), assistant_model=other, language="zh", task="transcribe", max_new_tokens=4)
