"""decode_weight_dtype="fp8_e4m3" without a GPU: the format's restatement (tests/w8_cases.py) checked against the
format's own statements, the model switch, the pseudo-labelling flag, the trainer's refusal, and how far the
quantisation alone moves the oracle on the config the GPU test uses (printed, not a condition)."""
import types

import pytest
import torch

import w8_cases as wc
from conftest import load_golden

DTYPES = (torch.bfloat16, torch.float16)


# ------------------------------------------------------------------------------------------ quantise_rows_ref
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_scales_are_the_smallest_power_of_two_that_fits(dt):
    g = torch.Generator().manual_seed(3)
    mags = torch.tensor([2.0 ** e for e in range(-20, 14, 3)])
    W = (torch.randn(len(mags), 320, generator=g) * mags[:, None]).to(dt)
    q, s = wc.quantise_rows_ref(W)
    assert q.shape == W.shape and s.shape == (len(mags),)
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all())                                          # powers of two
    r = W.float().abs().amax(1) / s
    assert bool(((r > 224) & (r <= 448)).all()), r                         # one step smaller would overflow
    assert float(q.float().abs().max()) <= 448.0 and bool(torch.isfinite(q.float()).all())
    # a row's scale is its own: the rows quantised one at a time give the same bytes
    for n in range(W.shape[0]):
        q1, s1 = wc.quantise_rows_ref(W[n:n + 1])
        assert torch.equal(q1.view(torch.uint8)[0], q.view(torch.uint8)[n]) and s1[0] == s[n]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", [16, 256])
def test_zero_row_boundary_rows_and_non_finite_rows(dt, K):
    W, rows = wc.weight_cases(8, K, dt, seed=2)
    q, s = wc.quantise_rows_ref(W)
    z = rows["zero"]
    assert s[z] == 1.0 and bool((q[z].float() == 0).all())
    assert q[z].view(torch.uint8)[:3].tolist() == [0, 0x80, 0]              # the zeros keep their signs
    # absmax = m * 2^x with x = 2: m = 0.875 is the last mantissa that fits with e = x - 9 (0.875 * 512 = 448)
    a, b = rows["m0875"], rows["above"]
    assert s[a] == 2.0 ** -7 and s[b] == 2.0 ** -6
    assert float(q[a, K // 2]) == 448.0 and float(q[b, K // 2]) == 224.0    # 3.515625 / 2^-6 = 225 -> 224 (RNE)
    for kind in ("inf", "nan"):
        r = rows[kind]
        assert torch.isnan(s[r]) and bool(torch.isnan(q[r].float()).all())
    ok = wc.finite_rows(rows, 8)
    assert bool(torch.isfinite(s[ok]).all()) and bool(torch.isfinite(wc.dequantise_rows_ref(q, s)[ok]).all())


def test_planted_ties_round_to_even():
    W, rows = wc.weight_cases(8, 128, torch.bfloat16, seed=1)
    q, s = wc.quantise_rows_ref(W)
    r = rows["ties"]
    assert float(s[r]) == 0.125
    assert q[r].float()[1:18].tolist() == [16.0, 20.0, -20.0, 1.0, -1.25, 192.0, -256.0, 0.0, 2.0 ** -8,
                                           -(2.0 ** -8), 3 * 2.0 ** -8, 2.0 ** -6, 7 * 2.0 ** -9, 0.0, 0.0, -0.0, 30.0]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_dequantise_then_requantise_stands_for_the_same_values(dt):
    W, rows = wc.weight_cases(40, 320, dt, seed=5)
    ok = wc.finite_rows(rows, 40)
    q, s = wc.quantise_rows_ref(W)
    back = wc.dequantise_rows_ref(q, s)[ok]
    assert torch.equal(back.to(dt).float(), back)                           # representable in the 16-bit dtype
    q2, s2 = wc.quantise_rows_ref(back.to(dt))
    # a row whose largest value rounded down may take a smaller scale; the values it stands for are the same
    assert torch.equal(wc.dequantise_rows_ref(q2, s2), back)
    same = s2 == s[ok]
    assert bool(same.any()) and torch.equal(q2.view(torch.uint8)[same], q.view(torch.uint8)[ok][same])


# ------------------------------------------------------------------------------------------ the switch
def _model(dtype=torch.float32, compute="bf16"):
    from tw.config import WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration
    from oracle.weights import CONFIGS, make_weights
    cfg = CONFIGS["micro"]
    w = make_weights(cfg, 1)
    return WhisperForConditionalGeneration.from_state_dict(WhisperConfig(**cfg), {k: torch.from_numpy(v) for k, v in
                                                                                  w.items()},
                                                           dtype=dtype, device="cpu", compute=compute)


def test_setter_accepts_none_auto_and_fp8():
    m = _model()
    assert m.decode_weight_dtype is None
    for v, want in (("fp8_e4m3", "fp8_e4m3"), ("auto", None), ("fp8_e4m3", "fp8_e4m3"), (None, None)):
        m.decode_weight_dtype = v
        assert m.decode_weight_dtype == want
    assert m.cross_kv_dtype is None                        # the two settings are independent
    m.requantize_decode_weights()                          # a no-op with the setting off


def test_setter_refuses_other_formats_and_the_fp32_path():
    m = _model()
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        m.decode_weight_dtype = "int8"
    assert m.decode_weight_dtype is None
    m32 = _model(compute="fp32")
    with pytest.raises(ValueError, match="fp32"):
        m32.decode_weight_dtype = "fp8_e4m3"
    m32.decode_weight_dtype = "auto"
    assert m32.decode_weight_dtype is None
    m.decode_weight_dtype = "fp8_e4m3"
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        m.set_compute("fp32")
    assert m.compute == "bf16" and m.decode_weight_dtype == "fp8_e4m3"


def test_covered_weights_are_the_steps_linears_and_the_head():
    m = _model()
    keys = m.decode_weight_keys()
    d, f, L = m.config.d_model, m.config.decoder_ffn_dim, m.config.decoder_layers
    assert len(keys) == 6 * L + 1
    assert [k[3] for k in keys[:6]] == [(3 * d, d), (d, d), (d, d), (d, d), (f, d), (d, f)]
    assert keys[-1][0] == wc.HEAD and keys[-1][3] == (m.Vp, d)
    assert not any("k_proj" in k[0] or "v_proj" in k[0] or "encoder.layers" in k[0] for k in keys)


def test_from_pretrained_passes_the_value_to_the_setter(tmp_path):
    from tw.modeling import WhisperForConditionalGeneration
    _model().save_pretrained(str(tmp_path))
    m = WhisperForConditionalGeneration.from_pretrained(str(tmp_path), device="cpu", decode_weight_dtype="fp8_e4m3")
    assert m.decode_weight_dtype == "fp8_e4m3" and m.cross_kv_dtype is None
    assert WhisperForConditionalGeneration.from_pretrained(str(tmp_path), device="cpu").decode_weight_dtype is None
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        WhisperForConditionalGeneration.from_pretrained(str(tmp_path), device="cpu", decode_weight_dtype="int4")


def test_trainer_refuses_a_student_with_the_setting_on():
    from tw.distill import DistillationTrainer
    s, t = _model(), _model()
    s.decode_weight_dtype = "fp8_e4m3"
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        DistillationTrainer(s, t)


# ------------------------------------------------------------------------------------------ the flag
def test_pseudo_labelling_flag_reaches_the_model(monkeypatch):
    from tw import modeling, pseudo_labelling as pl
    assert pl.parse_args([]).decode_weight_dtype == "auto"
    assert pl.parse_args(["--decode_weight_dtype", "fp8_e4m3"]).decode_weight_dtype == "fp8_e4m3"
    with pytest.raises(SystemExit):
        pl.parse_args(["--decode_weight_dtype", "int8"])
    seen = []

    class _M:
        decode_weight_dtype = "unset"

    def _load(path, **kw):
        assert "decode_weight_dtype" not in kw             # set on the model after loading
        seen.append(_M())
        return seen[-1]

    monkeypatch.setattr(modeling.WhisperForConditionalGeneration, "from_pretrained", staticmethod(_load))
    monkeypatch.setattr(torch.cuda, "set_device", lambda i: None)
    monkeypatch.setattr(pl, "load_text_decoder", lambda a: (lambda ids: ""))
    monkeypatch.setattr(pl, "ChunkTranscriber", lambda model, *a, **k: types.SimpleNamespace(m=model))
    monkeypatch.setattr(pl, "load_dataset", lambda p: [])
    monkeypatch.setattr(pl, "transcribe_files", lambda *a, **k: [])
    for argv, want in (([], "auto"), (["--decode_weight_dtype", "fp8_e4m3"], "fp8_e4m3")):
        pl.main(argv + ["--output_dir", "."])
        assert seen[-1].decode_weight_dtype == want


# ------------------------------------------------------------------------------------------ RefW8 against Ref
def test_how_far_the_quantisation_alone_moves_the_oracle(record_property):
    """DECODE_CFG (the GPU test's config) on two clips and the greedy fixture prompt: the greedy ids of RefW8 against
    those of Ref, and the worst change of a logit along Ref's own sequence.  Recorded and printed, not a condition:
    the engine's fp8 run is judged against RefW8, and what the format costs in WER / MER needs a real checkpoint."""
    from oracle import greedy_ref, logmel
    g = load_golden("greedy")
    sup, prompt = g["suppress"].tolist(), g["greedy_prompt"].tolist()
    feats = torch.from_numpy(logmel.log_mel_batch([logmel.synthetic_clip(0), logmel.synthetic_clip(2, 9.0)]))
    r16, r8 = wc.decode_ref("bf16", False), wc.decode_ref("bf16", True)
    with torch.no_grad():
        ids8 = greedy_ref.greedy(r8, feats, prompt, max_length=32, suppress_tokens=sup)
        ids16, sc16 = greedy_ref.greedy(r16, feats, prompt, max_length=32, suppress_tokens=sup, return_scores=True)
        enc = r16.encoder(feats)
        seq = torch.as_tensor(ids16)[:, :-1]
        dl = (r8.logits(r8.decoder(seq, enc)) - r16.logits(r16.decoder(seq, enc))).abs().max()
    left, total = wc.xc.agreement(torch.as_tensor(ids8), torch.as_tensor(ids16), sc16, len(prompt), margin=None)
    print(f"RefW8 vs Ref on DECODE_CFG: {left} of {total} generated positions after a row's first difference; "
          f"worst logit change {float(dl):.4f}")
    record_property("positions_left_out", left)
    record_property("positions", total)
    record_property("worst_logit_change", float(dl))
    assert total >= 8 and bool(torch.isfinite(dl))
