"""model.cross_kv_dtype = "fp8_e4m3" end to end on the GPU, micro fixture dimensions.

The reference is the CPU restatement RefFp8 (tests/xkv_fp8_cases.py: oracle.whisper_ref.Ref with the cross-attention
K/V through quantise_ref), never the engine's own 16-bit run:

* the session's buffers: bytes, today's element count, the scale tensors;
* greedy ids on the inputs of tests/golden/greedy.npz: RefFp8 teacher-forced along the emitted tokens holds each of
  them within MARGIN of its argmax (the rule and MARGIN of tests/test_decode_gpu.py), and against
  oracle.greedy_ref.greedy(RefFp8) the ids agree up to a near-tie per row, at most half of the generated positions
  left out (tests/test_xkv_fp8_cpu.py checks that RefFp8 against Ref stays within that cap by itself);
* with timestamps, through the seek loop, every window obeys the timestamp rules against RefFp8;
* engine-internal equalities: the shared-block batch == per-row copies, graph replay == eager, and after
  cross_kv_dtype = None the model returns exactly the ids it returned before the switch was set.
"""
import pytest
import torch

import xkv_fp8_cases as xc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _greedy_model():
    from test_decode_gpu import _feats, _micro
    cfg, w, m, GC = _micro()
    g = load_golden("greedy")
    sup = g["suppress"].tolist()
    m.generation_config = GC(suppress_tokens=sup, begin_suppress_tokens=[220, 50257])
    return cfg, w, m, sup, g["greedy_prompt"].tolist(), _feats()


def test_session_buffers_are_bytes_with_scales():
    from tw.generation import DecodeSession
    cfg, w, m, sup, prompt, feats = _greedy_model()
    m.cross_kv_dtype = "fp8_e4m3"
    enc = m.encode(m.conv_input(feats.to(DEV)))
    B, Tk = 3, enc.shape[0] // 3
    H, L = cfg["d_model"] // 64, cfg["decoder_layers"]
    sess = DecodeSession(m, enc, B, Tk, 8)
    assert len(sess.cross_kv) == L and len(sess.cross_scale) == L
    for kv, s in zip(sess.cross_kv, sess.cross_scale):
        assert kv.element_size() == 1 and kv.numel() == 2 * B * H * Tk * 64
        assert s.dtype == torch.float32 and s.numel() == 2 * B * H
        m2, _ = torch.frexp(s.cpu())
        assert bool((m2 == 0.5).all())                                # every scale a power of two
    # the bytes are the format's: layer 0 against quantise_ref of the engine's own 16-bit projection
    m.cross_kv_dtype = None
    s16 = DecodeSession(m, enc, B, Tk, 8)
    assert s16.cross_kv[0].element_size() == 2 and s16.cross_scale is None
    n = B * H * Tk * 64
    k16, v16 = s16.cross_kv[0][:n].view(B, H, Tk, 64).cpu(), s16.cross_kv[0][n:].view(B, H, Tk, 64).cpu()
    (qk, sk), (qv, sv) = xc.quantise_ref(k16), xc.quantise_ref(v16)
    assert torch.equal(sess.cross_kv[0][:n].cpu(), qk.view(torch.uint8).reshape(-1))
    assert torch.equal(sess.cross_kv[0][n:].cpu(), qv.view(torch.uint8).reshape(-1))
    assert torch.equal(sess.cross_scale[0].cpu(), torch.cat([sk.reshape(-1), sv.reshape(-1)]))


def test_greedy_ids_against_the_fp8_oracle():
    from oracle import greedy_ref
    from oracle.whisper_ref import to_torch
    from test_decode_gpu import MARGIN, _mask, _teacher_forced
    assert MARGIN == xc.MARGIN
    cfg, w, m, sup, prompt, feats = _greedy_model()
    m.cross_kv_dtype = "fp8_e4m3"
    P = len(prompt)
    gen = m.generate(feats, decoder_input_ids=torch.tensor([prompt] * 3), max_length=64).cpu()
    seq = torch.cat([torch.tensor([prompt] * 3), gen], 1)
    ref = xc.RefFp8(cfg, to_torch(w), amp=True)
    # the margin rule of tests/test_decode_gpu.py::test_generate_matches_autocast_oracle, RefFp8 for Ref
    lg = _teacher_forced(ref, feats, seq)
    worst = 0.0
    for j in range(gen.shape[1]):
        live = torch.ones(3, dtype=torch.bool) if j == 0 else (gen[:, :j] != 50257).all(1)
        ra = _mask(lg[:, P - 1 + j], j, sup)
        gap = ra.max(-1).values - ra.gather(1, gen[:, j:j + 1])[:, 0]
        worst = max(worst, float(gap[live].max()) if bool(live.any()) else 0.0)
        assert bool((gap[live] <= MARGIN).all()), (j, gap)
    # against the oracle's own greedy ids
    with torch.no_grad():
        ids_ref, sc = greedy_ref.greedy(ref, feats, prompt, max_length=64, suppress_tokens=sup, return_scores=True)
    left, total = xc.agreement(seq, ids_ref, sc, P)
    print(f"worst teacher-forced gap {worst:.4f} (MARGIN {MARGIN}); {left} of {total} positions left out")
    assert total >= 16 and 2 * left <= total


def test_timestamps_through_the_seek_loop_against_the_fp8_oracle():
    from oracle.whisper_ref import to_torch
    from test_decode_gpu import _check_ts_window, _feats, _ts_model
    mg, cfg, w, m = _ts_model()
    m.cross_kv_dtype = "fp8_e4m3"
    feats = _feats()[:2]
    trace = []
    gen = m.generate(feats, return_timestamps=True, language="zh", task="transcribe", max_new_tokens=48,
                     _trace=trace).cpu()
    prompt = [50258, 50260, 50359]
    ref = xc.RefFp8(cfg, to_torch(w), amp=True)
    assert trace and {t["b"] for t in trace} == {0, 1}
    for t in trace:
        n = 3000 - t["seek"]
        seg = torch.zeros(1, 80, 3000)
        seg[0, :, :n] = feats[t["b"], :, t["seek"]:t["seek"] + n]
        _check_ts_window(ref, seg, prompt, t["raw"], mg.SUPPRESS)
    assert bool((gen[:, 0] >= 50364).all())


def test_shared_block_batch_equals_per_row_copies():
    """One clip's quantised blocks and scales read by every row with batch stride 0 (the fallback batch of one
    window) == the rows over B quantised copies: the same logits, bit for bit, over several steps."""
    from tw.generation import DecodeSession
    cfg, w, m, sup, prompt, feats = _greedy_model()
    m.cross_kv_dtype = "fp8_e4m3"
    enc = m.encode(m.conv_input(feats[:1].to(DEV)))
    B, Tk = 4, enc.shape[0]
    a = DecodeSession(m, enc, B, Tk, 8)
    b = DecodeSession(m, enc.repeat(B, 1), B, Tk, 8)
    assert a.xkv_shared and not b.xkv_shared
    for tok in (50258, 50260, 50359, 1234):
        for s in (a, b):
            s.cur.copy_(torch.tensor([tok, tok + 1, tok + 2, tok + 3], device=DEV))
            s.step()
        assert torch.equal(a.logits, b.logits)
    assert bool(torch.isfinite(a.logits.float()).all())


def test_graph_equals_eager_and_the_switch_is_dropped_cleanly():
    cfg, w, m, sup, prompt, feats = _greedy_model()
    pr = torch.tensor([prompt] * 3)
    before = m.generate(feats, decoder_input_ids=pr, max_length=48).cpu()
    m.cross_kv_dtype = "fp8_e4m3"
    a = m.generate(feats, decoder_input_ids=pr, max_length=48, use_graph=True).cpu()
    b = m.generate(feats, decoder_input_ids=pr, max_length=48, use_graph=False).cpu()
    assert torch.equal(a, b)
    m.cross_kv_dtype = None
    after = m.generate(feats, decoder_input_ids=pr, max_length=48).cpu()
    assert torch.equal(before, after)
