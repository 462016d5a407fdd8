"""model.decode_weight_dtype = "fp8_e4m3" end to end on the GPU, on the smallest config whose decode step takes the
GEMV path (w8_cases.DECODE_CFG, d_model = 256), for a bf16 model, an fp16 model and (greedy only) bf16 autocast over
an fp32 master.

The reference is the CPU restatement RefW8 (tests/w8_cases.py: oracle.whisper_ref.Ref over the dequantised weights),
never the engine's own 16-bit run.  The margin rule is tests/test_decode_gpu.py::
test_generate_matches_autocast_oracle's: at every live position the engine's token is within the margin of the best
processed score of the oracle run along the engine's own sequence; no position is left out.  The margin comes from a
control in the same test -- the same rule with the setting off against plain Ref, the parent's code path: within
MARGIN (0.05) -> MARGIN, else twice the control's worst gap (the fp8 path adds no rounding the oracle does not
restate; only the accumulation order differs).
"""
import pytest
import torch

import w8_cases as wc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 50257
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _model(mode):
    """One engine model per mode for the module; every test leaves the setting off."""
    if mode not in _CACHE:
        from tw.config import GenerationConfig
        m = wc.decode_model(mode)
        g = load_golden("greedy")
        m.generation_config = GenerationConfig(suppress_tokens=g["suppress"].tolist(),
                                               begin_suppress_tokens=[220, EOS])
        _CACHE[mode] = m
    m = _CACHE[mode]
    m.decode_weight_dtype = None
    return m


def _fixture():
    if "fx" not in _CACHE:
        from test_decode_gpu import _feats
        g = load_golden("greedy")
        _CACHE["fx"] = (g["suppress"].tolist(), g["greedy_prompt"].tolist(), _feats())
    return _CACHE["fx"]


def _ref(mode, w8):
    if ("ref", mode, w8) not in _CACHE:
        _CACHE[("ref", mode, w8)] = wc.decode_ref(mode, w8)
    return _CACHE[("ref", mode, w8)]


def _enc(mode):
    """The oracle's encoder output on the fixture clips (the format leaves the encoder alone: Ref's and RefW8's)."""
    if ("enc", mode) not in _CACHE:
        with torch.no_grad():
            _CACHE[("enc", mode)] = _ref(mode, False).encoder(_fixture()[2])
    return _CACHE[("enc", mode)]


def _generate(m, feats, prompt, n=40, **kw):
    pr = torch.tensor([prompt] * feats.shape[0])
    gen = m.generate(feats, decoder_input_ids=pr, max_length=n, **kw).cpu()
    return torch.cat([pr, gen], 1)


def _margin(mode, control):
    """The rule of the module docstring: w8_cases.W8_MARGIN while the control stays within MARGIN."""
    return wc.W8_MARGIN if control <= wc.MARGIN else 2 * control


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_buffers_hold_the_restatement_of_the_engines_own_weights(mode):
    from tw.generation import DecodeSession
    m = _model(mode)
    ptr_before = None
    m.decode_weight_dtype = "fp8_e4m3"
    d = wc.DECODE_CFG["d_model"]
    p = "model.decoder.layers.0"
    for key, w16 in ((p + ".self_attn.q_proj.weight",
                      m.wspan(p + ".self_attn.q_proj.weight", p + ".self_attn.v_proj.weight", (3 * d, d))),
                     (p + ".fc2.weight", m._w16(p + ".fc2.weight")), (wc.HEAD, m._w16(wc.HEAD))):
        b, s = m.decode_weight_fp8(key)
        assert b.dtype == torch.uint8 and tuple(b.shape) == tuple(w16.shape) and s.dtype == torch.float32
        q, sr = wc.quantise_rows_ref(w16.cpu())
        assert torch.equal(b.cpu(), q.view(torch.uint8)) and torch.equal(s.cpu(), sr)
    b, s = m.decode_weight_fp8(wc.HEAD)
    V = wc.DECODE_CFG["vocab_size"]
    assert bool((s[V:] == 1).all()) and bool((b[V:] == 0).all())            # pad rows: zero, scale 1
    # one byte buffer, one scale buffer; the session records the setting
    assert m._w8_bytes.dtype == torch.uint8 and m._w8_scales.dtype == torch.float32
    sup, prompt, feats = _fixture()
    enc = m.encode(m.conv_input(feats[:1].to(DEV)))
    sess = DecodeSession(m, enc, 1, enc.shape[0], 8)
    assert sess.w8 and sess.gemv
    # requantize_decode_weights after writing a weight: the bytes change in place
    ptr_before = (m._w8_bytes.data_ptr(), m._w8_scales.data_ptr())
    w = m._w16(p + ".fc2.weight")
    keep = w.clone()
    w[3].mul_(4.0)
    old_b, old_s = (t.clone() for t in m.decode_weight_fp8(p + ".fc2.weight"))
    m.requantize_decode_weights()
    nb, ns = m.decode_weight_fp8(p + ".fc2.weight")
    assert (m._w8_bytes.data_ptr(), m._w8_scales.data_ptr()) == ptr_before
    assert float(ns[3]) == 4 * float(old_s[3]) and torch.equal(nb[3], old_b[3])     # x 4: the scale moves, exactly
    w.copy_(keep)
    m.requantize_decode_weights()
    assert torch.equal(m.decode_weight_fp8(p + ".fc2.weight")[1], old_s)
    m.decode_weight_dtype = None
    assert not DecodeSession(m, enc, 1, enc.shape[0], 8).w8


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_greedy_ids_against_the_w8_oracle(mode):
    sup, prompt, feats = _fixture()
    m = _model(mode)
    P = len(prompt)
    control = wc.worst_gap(_ref(mode, False), feats, 1, _generate(m, feats, prompt), P, sup, enc=_enc(mode))
    margin = _margin(mode, control)
    m.decode_weight_dtype = "fp8_e4m3"
    seq = _generate(m, feats, prompt)
    m.decode_weight_dtype = None
    gap = wc.worst_gap(_ref(mode, True), feats, 1, seq, P, sup, enc=_enc(mode))
    print(f"{mode}: control (setting off, Ref) worst gap {control:.4f} -> margin {margin:.4f}; fp8 against RefW8 "
          f"worst gap {gap:.4f}")
    assert seq.shape[1] - P >= 16
    assert gap <= margin, (gap, margin, control)


def test_autocast_over_an_fp32_master_against_the_w8_oracle():
    """bf16 autocast over an fp32 master: the GEMV path without the fused LayerNorm (LN kernel + plain w8 call, the
    head included) and an fp32 residual stream.  The same rule, with one allowance that is reasoned, not measured:
    this config's logits reach |x| in [16, 32), where one bf16 ulp is 0.125 > MARGIN, and the logits ARE bf16 values
    -- two fp32 sums that differ only by their accumulation order can round to neighbouring bf16 values, so a gap
    of at most one bf16 ulp of the best score (2^-7 |best|) is a tie at the logits' own resolution and counts as 0.
    The control (setting off, plain Ref) is held to the same."""
    sup, prompt, feats = _fixture()
    m = _model("amp")
    P = len(prompt)
    kw = dict(enc=_enc("amp"), tie_ulp=2.0 ** -7)
    control = wc.worst_gap(_ref("amp", False), feats, 1, _generate(m, feats, prompt), P, sup, **kw)
    m.decode_weight_dtype = "fp8_e4m3"
    a = _generate(m, feats, prompt, use_graph=True)
    b = _generate(m, feats, prompt, use_graph=False)
    m.decode_weight_dtype = None
    gap = wc.worst_gap(_ref("amp", True), feats, 1, a, P, sup, **kw)
    print(f"amp: control worst gap {control:.4f}; fp8 against RefW8 worst gap {gap:.4f} (gaps within one bf16 ulp of "
          f"the best score count as 0)")
    assert torch.equal(a, b)
    assert control <= wc.MARGIN and gap <= wc.MARGIN, (control, gap)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_batch_of_nine_reads_the_same_weight_values(mode):
    """B = 9 is off the GEMV path: the session reads the 16-bit copy of the dequantised weights through the GEMM, so it
    is judged against RefW8 under the same rule; rows 0..7 of a B = 8 call against the same rows of the B = 9 call
    differ only by the summation order of GEMV against GEMM (printed)."""
    from tw.generation import DecodeSession
    sup, prompt, feats = _fixture()
    m = _model(mode)
    P = len(prompt)
    f9 = feats.repeat(3, 1, 1)
    control = wc.worst_gap(_ref(mode, False), feats, 3, _generate(m, f9, prompt, 32), P, sup, enc=_enc(mode))
    margin = _margin(mode, control)
    m.decode_weight_dtype = "fp8_e4m3"
    enc = m.encode(m.conv_input(f9.to(DEV)))
    sess = DecodeSession(m, enc, 9, enc.shape[0] // 9, 8)
    assert sess.w8 and not sess.gemv
    del sess
    s9 = _generate(m, f9, prompt, 32)
    s8 = _generate(m, f9[:8], prompt, 32)
    assert m._w8_deq                                                       # the lazily built copy exists ...
    m.decode_weight_dtype = None
    assert not m._w8_deq                                                   # ... and is dropped with the setting
    gap = wc.worst_gap(_ref(mode, True), feats, 3, s9, P, sup, enc=_enc(mode))
    n = min(s8.shape[1], s9.shape[1])           # a call stops when its last row has finished: eos columns beyond
    agree = int((s8[:, :n] == s9[:8, :n]).all(1).sum())
    print(f"{mode}: B = 9 control worst gap {control:.4f} -> margin {margin:.4f}; fp8 B = 9 against RefW8 worst gap "
          f"{gap:.4f}; rows of B = 8 equal to the same rows of B = 9: {agree} of 8")
    assert gap <= margin, (gap, margin, control)


def test_timestamps_through_the_seek_loop_against_the_w8_oracle():
    import oracle.fixture_inputs as mg
    from test_decode_gpu import _check_ts_window
    from tw.config import GenerationConfig
    sup, prompt, feats = _fixture()
    m = _model("bf16")
    keep = m.generation_config
    m.generation_config = GenerationConfig({k: mg.TS_GENERATION[k] for k in mg.TW_GENERATION_KEYS})
    try:
        m.decode_weight_dtype = "fp8_e4m3"
        trace = []
        gen = m.generate(feats[:1], return_timestamps=True, language="zh", task="transcribe", max_new_tokens=40,
                         _trace=trace).cpu()
    finally:
        m.decode_weight_dtype = None
        m.generation_config = keep
    ref = _ref("bf16", True)
    assert trace
    for t in trace:
        n = 3000 - t["seek"]
        seg = torch.zeros(1, 80, 3000)
        seg[0, :, :n] = feats[0, :, t["seek"]:t["seek"] + n]
        _check_ts_window(ref, seg, [50258, 50260, 50359], t["raw"], mg.SUPPRESS)
    assert int(gen[0, 0]) >= 50364


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_assisted_equals_unassisted_with_the_setting_on_the_target(mode):
    import oracle.fixture_inputs as mg
    from tw.config import GenerationConfig
    sup, prompt, feats = _fixture()
    m = _model(mode)
    keep = m.generation_config
    m.generation_config = GenerationConfig({k: mg.TS_GENERATION[k] for k in mg.TW_GENERATION_KEYS})
    if ("other", mode) not in _CACHE:
        from oracle.weights import make_weights
        from tw.config import WhisperConfig
        from tw.modeling import WhisperForConditionalGeneration
        sd = {k: torch.from_numpy(v) for k, v in make_weights(wc.DECODE_CFG, 4, lin_std=wc.DECODE_LIN_STD).items()}
        _CACHE[("other", mode)] = WhisperForConditionalGeneration.from_state_dict(
            WhisperConfig(**wc.DECODE_CFG), sd, dtype=wc.MODES[mode][0])
    other = _CACHE[("other", mode)]
    other.generation_config = GenerationConfig(dict(m.generation_config))
    try:
        m.decode_weight_dtype = "fp8_e4m3"
        for ts in (False, True):
            kw = dict(language="zh", task="transcribe", max_new_tokens=24, **({"return_timestamps": True} if ts else {}))
            want = m.generate(feats[:1], **kw).cpu()
            for a, k in ((m, 7), (other, 4)):
                trace = []
                got = m.generate(feats[:1], assistant_model=a, num_assistant_tokens=k, _trace=trace, **kw).cpu()
                assert torch.equal(got, want), (ts, k)
                if a is m:          # the target's own bytes as the assistant: every draft of a full round stands
                    assert all(n == k for t in trace if "accepted" in t for n in t["accepted"][:-1])
    finally:
        m.decode_weight_dtype = None
        m.generation_config = keep


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_graph_equals_eager_and_the_switch_leaves_nothing_stale(mode):
    sup, prompt, feats = _fixture()
    m = _model(mode)
    before = _generate(m, feats, prompt)
    m.decode_weight_dtype = "fp8_e4m3"
    a = _generate(m, feats, prompt, use_graph=True)
    b = _generate(m, feats, prompt, use_graph=False)
    assert torch.equal(a, b)
    m.decode_weight_dtype = None
    assert torch.equal(_generate(m, feats, prompt), before)
    m.decode_weight_dtype = "fp8_e4m3"
    assert torch.equal(_generate(m, feats, prompt), a)
    m.decode_weight_dtype = "auto"
    assert torch.equal(_generate(m, feats, prompt), before)
