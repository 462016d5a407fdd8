"""cross_kv_dtype="fp8_e4m3" without a GPU: the format's restatement (tests/xkv_fp8_cases.py) checked against the
format's own statements, the model switch, the pseudo-labelling flag, and how far the quantisation alone moves the
oracle's greedy ids on the fixture the GPU test uses."""
import types

import numpy as np
import pytest
import torch

import xkv_fp8_cases as xc
from conftest import load_golden
from oracle.weights import CONFIGS, make_weights

DTYPES = (torch.bfloat16, torch.float16)


# ------------------------------------------------------------------------------------------ quantise_ref
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_scales_are_the_smallest_power_of_two_that_fits(dt):
    g = torch.Generator().manual_seed(3)
    mags = torch.tensor([2.0 ** e for e in range(-20, 14, 3)])
    x = (torch.randn(len(mags), 5, 64, generator=g) * mags[:, None, None]).to(dt)
    q, s = xc.quantise_ref(x)
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all())                                          # powers of two
    r = x.float().abs().amax((1, 2)) / s
    assert bool(((r > 224) & (r <= 448)).all()), r                         # one step smaller would overflow
    assert float(q.float().abs().max()) <= xc.E4M3_MAX and bool(torch.isfinite(q.float()).all())


def test_zero_block_subnormal_block_and_non_finite_block():
    x = torch.zeros(4, 3, 64, dtype=torch.bfloat16)
    x[1, 0, :4] = torch.tensor([0.0, -0.0, 0.0, -0.0], dtype=torch.bfloat16)
    x[2] = 2.0 ** -130                                                      # bf16 subnormals: e clamps at -100
    x[2, 1, 5] = -(2.0 ** -127)
    x[3, 2, 7] = float("inf")
    q, s = xc.quantise_ref(x)
    assert s[0] == 1.0 and s[1] == 1.0 and s[2] == 2.0 ** -100 and torch.isnan(s[3])
    assert bool((q[:3].float() == 0).all())                                 # 2^-27 in units of the scale rounds to 0
    assert q[1].view(torch.uint8)[0, :4].tolist() == [0, 0x80, 0, 0x80]     # the zeros keep their signs


def test_mantissa_boundary_at_seven_eighths():
    """absmax = m * 2^x: m = 0.875 is the last mantissa that fits with e = x - 9 (0.875 * 512 = 448)."""
    for dt in DTYPES:
        x = torch.zeros(3, 1, 64, dtype=dt)
        x[0, 0, 0], x[1, 0, 0], x[2, 0, 0] = 0.875 * 4, 0.875 * 4 + 2.0 ** -6, -0.5 * 4      # x = 2
        q, s = xc.quantise_ref(x)
        assert s.tolist() == [2.0 ** -7, 2.0 ** -6, 2.0 ** -7]
        assert q[:, 0, 0].float().tolist() == [448.0, 224.0, -256.0]       # 3.515625 / 2^-6 = 225 -> 224 (RNE)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_dequantise_then_requantise_is_the_identity(dt):
    x = xc.blocks(2, 3, 37, dt, seed=5)
    q, s = xc.quantise_ref(x)
    back = xc.dequantise_ref(q, s)
    assert torch.equal(back.to(dt).float(), back)                           # representable in the 16-bit dtype
    q2, s2 = xc.quantise_ref(back.to(dt))
    # a block whose largest value rounded down may take a smaller scale; the values it stands for are the same
    assert torch.equal(xc.dequantise_ref(q2, s2), back)
    same = s2 == s
    assert bool(same.any()) and torch.equal(q2.view(torch.uint8)[same], q.view(torch.uint8)[same])


def test_planted_ties_round_to_even():
    x = xc.blocks(1, 1, 2, torch.bfloat16, seed=1)
    q, s = xc.quantise_ref(x)
    assert float(s) == 0.125
    got = q.float().view(-1)[1:18].tolist()
    assert got == [16.0, 20.0, -20.0, 1.0, -1.25, 192.0, -256.0, 0.0, 2.0 ** -8, -(2.0 ** -8), 3 * 2.0 ** -8,
                   2.0 ** -6, 7 * 2.0 ** -9, 0.0, 0.0, -0.0, 30.0]


# ------------------------------------------------------------------------------------------ the switch
def _model(dtype=torch.float32, compute="bf16"):
    from tw.config import WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration
    cfg = CONFIGS["micro"]
    w = make_weights(cfg, 1)
    return WhisperForConditionalGeneration.from_state_dict(WhisperConfig(**cfg), {k: torch.from_numpy(v) for k, v in
                                                                                  w.items()},
                                                           dtype=dtype, device="cpu", compute=compute)


def test_setter_accepts_none_auto_and_fp8():
    m = _model()
    assert m.cross_kv_dtype is None
    for v, want in (("fp8_e4m3", "fp8_e4m3"), ("auto", None), ("fp8_e4m3", "fp8_e4m3"), (None, None)):
        m.cross_kv_dtype = v
        assert m.cross_kv_dtype == want


def test_setter_refuses_other_formats_and_the_fp32_path():
    m = _model()
    with pytest.raises(ValueError, match="cross_kv_dtype"):
        m.cross_kv_dtype = "int8"
    assert m.cross_kv_dtype is None
    m32 = _model(compute="fp32")
    with pytest.raises(ValueError, match="fp32"):
        m32.cross_kv_dtype = "fp8_e4m3"
    m32.cross_kv_dtype = "auto"
    assert m32.cross_kv_dtype is None
    m.cross_kv_dtype = "fp8_e4m3"
    with pytest.raises(ValueError, match="cross_kv_dtype"):
        m.set_compute("fp32")


def test_from_pretrained_passes_the_value_to_the_setter(tmp_path):
    from tw.modeling import WhisperForConditionalGeneration
    _model().save_pretrained(str(tmp_path))
    m = WhisperForConditionalGeneration.from_pretrained(str(tmp_path), device="cpu", cross_kv_dtype="fp8_e4m3")
    assert m.cross_kv_dtype == "fp8_e4m3"
    assert WhisperForConditionalGeneration.from_pretrained(str(tmp_path), device="cpu").cross_kv_dtype is None
    with pytest.raises(ValueError, match="cross_kv_dtype"):
        WhisperForConditionalGeneration.from_pretrained(str(tmp_path), device="cpu", cross_kv_dtype="int4")


# ------------------------------------------------------------------------------------------ the flag
def test_pseudo_labelling_flag_reaches_the_model(monkeypatch):
    import inspect
    from tw import modeling, pseudo_labelling as pl
    assert pl.parse_args([]).cross_kv_dtype == "auto"
    assert pl.parse_args(["--cross_kv_dtype", "fp8_e4m3"]).cross_kv_dtype == "fp8_e4m3"
    with pytest.raises(SystemExit):
        pl.parse_args(["--cross_kv_dtype", "int8"])
    seen = []

    class _M:
        cross_kv_dtype = "unset"

    def _load(path, **kw):
        assert "cross_kv_dtype" not in kw                  # set on the model after loading
        seen.append(_M())
        return seen[-1]

    monkeypatch.setattr(modeling.WhisperForConditionalGeneration, "from_pretrained", staticmethod(_load))
    monkeypatch.setattr(torch.cuda, "set_device", lambda i: None)
    monkeypatch.setattr(pl, "load_text_decoder", lambda a: (lambda ids: ""))
    monkeypatch.setattr(pl, "ChunkTranscriber", lambda model, *a, **k: types.SimpleNamespace(m=model))
    monkeypatch.setattr(pl, "load_dataset", lambda p: [])
    monkeypatch.setattr(pl, "transcribe_files", lambda *a, **k: [])
    for argv, want in (([], "auto"), (["--cross_kv_dtype", "fp8_e4m3"], "fp8_e4m3")):
        pl.main(argv + ["--output_dir", "."])
        assert seen[-1].cross_kv_dtype == want


def test_chunk_transcriber_signature_keeps_its_defaults():
    import inspect
    from tw import pseudo_labelling as pl
    sig = inspect.signature(pl.ChunkTranscriber.__init__).parameters
    assert list(sig) == ["self", "model", "language", "max_new_tokens", "device", "repetition_penalty",
                         "no_repeat_ngram_size"]


# ------------------------------------------------------------------------------------------ RefFp8 against Ref
def _feats():
    from oracle import logmel
    return torch.from_numpy(logmel.log_mel_batch([logmel.synthetic_clip(0), logmel.synthetic_clip(2, 9.0),
                                                  logmel.synthetic_clip(4, 25.0)]))


def test_quantisation_alone_stays_within_the_cap_on_the_greedy_fixture():
    """tests/golden/greedy.npz's inputs: the greedy ids of RefFp8 against those of Ref under the rule the GPU test
    applies to the engine (xkv_fp8_cases.agreement) -- at most half of the generated positions are left out, so the
    engine's fp8 run is judged against RefFp8 on a fixture where the format itself decides little."""
    from oracle import greedy_ref
    from oracle.whisper_ref import Ref, to_torch
    cfg = CONFIGS["micro"]
    w = make_weights(cfg, 1, lin_std=0.2)
    g = load_golden("greedy")
    sup, prompt = g["suppress"].tolist(), g["greedy_prompt"].tolist()
    feats = _feats()
    with torch.no_grad():
        ids8 = greedy_ref.greedy(xc.RefFp8(cfg, to_torch(w), amp=True), feats, prompt, max_length=64,
                                 suppress_tokens=sup)
        ids16, sc16 = greedy_ref.greedy(Ref(cfg, to_torch(w), amp=True), feats, prompt, max_length=64,
                                        suppress_tokens=sup, return_scores=True)
    left, total = xc.agreement(ids8, ids16, sc16, len(prompt), margin=None)
    print(f"RefFp8 vs Ref on greedy.npz: {left} of {total} generated positions left out")
    assert total >= 16 and 2 * left <= total
