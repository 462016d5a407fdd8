"""The large-v3 family on the GPU: the 128-bin log-mel kernel, and every kernel that sees the vocabulary at
V = 51866 (one column more than large-v2; the padded row length stays 51904) or the conv stem at 128 mel bins.

Bars are the existing ones for the same arithmetic:
  * log-mel: 1e-4 absolute against HF (tests/golden/v3.npz) and against a float64 restatement (test_kernels_gpu.py's
    bar at 80 bins); the conv input equals the rounded mel bit for bit; 80 bins through the new entry point are
    tw_logmel_len's bits;
  * fp32 path against HF fp32: losses 2e-5 relative, sampled tensors 1e-4 relative L2 (test_fp32_gpu.py); token ids,
    windows and seeks identical;
  * bf16 forward: the micro config's bar of test_distill_gpu.py (log-sum-exp 2^-7 relative at worst, 3e-4 on average;
    CE 1e-3);
  * selection kernels: ids exact, log-probs 1e-4 (test_select_kernels_gpu.py's harness on a 51866-id vocabulary);
  * decode GEMV: test_kernels_gpu.py::test_gemv_decode's bar; KL/CE: test_kl_ce_matches_oracle's.
"""
import json
import os

import numpy as np
import pytest
import torch

import select_cases as sc
import v3_inputs as X
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def bf(x):
    return x.to(torch.bfloat16)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ log-mel
def _log_mel64(wav, n, fb):
    """HF's _torch_extract_fbank_features in float64 with the filter bank `fb` [201, n_mels]: zero-pad / trim to n
    samples, reflect pad 200, periodic Hann frames of 400 every 160, |rfft|^2 without the last frame, mel, log10 with
    a 1e-10 floor, max(x, clip max - 8), (x + 4) / 4."""
    x = np.zeros(n, dtype=np.float64)
    w = np.asarray(wav, dtype=np.float64).reshape(-1)[:n]
    x[:len(w)] = w
    xp = np.pad(x, (200, 200), mode="reflect")
    idx = np.arange(400)[None, :] + 160 * np.arange(1 + (len(xp) - 400) // 160)[:, None]
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 400)
    spec = np.fft.rfft(xp[idx] * win[None, :], axis=1)
    power = (spec.real ** 2 + spec.imag ** 2)[:-1]
    ls = np.log10(np.maximum(power @ fb.astype(np.float64), 1e-10)).T
    return (np.maximum(ls, ls.max() - 8.0) + 4.0) / 4.0


def test_logmel_128_matches_hf_and_float64():
    from oracle import logmel as ol
    from tw import ops
    from tw.feature_extraction import mel_tables
    g = load_golden("v3")
    clips = [ol.synthetic_clip(0), ol.synthetic_clip(3, 12.0), np.zeros(16000, np.float32)]
    wav = torch.stack([torch.from_numpy(ol.pad_or_trim(c).astype(np.float32)) for c in clips]).to(DEV)
    basis, start, w = (t.to(DEV) for t in mel_tables(n_mels=128))
    mel = torch.full((3, 128, 3000), float("nan"), device=DEV)
    conv = torch.full((3, 3002, 128), 9.0, dtype=torch.bfloat16, device=DEV)
    ops.logmel(wav, basis, start, w, mel, conv)
    got = mel.cpu().numpy()
    ref = np.stack([_log_mel64(c, 480000, g["mel_filters"]) for c in clips])
    err, err_hf = np.abs(got - ref).max(), np.abs(got[:, :, ::10] - g["mel_sub"]).max()
    err_max = np.abs(got.reshape(3, -1).max(-1) - g["mel_max"]).max()
    print(f"128-bin log-mel max abs err vs float64 {err:.2e}, vs HF {err_hf:.2e}, clip max vs HF {err_max:.2e}")
    assert err < 1e-4 and err_hf < 1e-4 and err_max < 1e-4
    c = conv.float().cpu()
    assert (c[:, 0] == 0).all() and (c[:, 3001] == 0).all()
    assert (c[:, 1:3001].transpose(1, 2) - bf(mel.cpu()).float()).abs().max() == 0


def _longform_128():
    from oracle import logmel as ol
    from tw.feature_extraction import WhisperFeatureExtractor
    clips = [ol.synthetic_clip(6, 47.3), ol.synthetic_clip(7, 65.0)]
    fe = WhisperFeatureExtractor(feature_size=128, device=DEV)
    r = fe(clips, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True)
    return clips, fe, r


def test_logmel_128_longform_matches_hf_and_float64():
    """The 47.3 s + 65 s long-form pair at 128 bins, held to the 80-bin bar: 1e-4 absolute against HF and float64.
    With the DFT accumulated in fp32, as at 80 bins, this call measured 1.50e-4 / 1.76e-4: two values next to the clamp
    floor in one- and two-tap mel rows, where O(0.5) terms cancel to O(1e-3) (80 bins on the same clips: 8.5e-5).  The
    128-bin instantiation therefore accumulates the DFT on the f64 MFMA."""
    g = load_golden("v3")
    clips, fe, r = _longform_128()
    got = r.input_features.cpu().numpy()
    n = max(len(c) for c in clips)
    assert got.shape == tuple(g["long_shape"]) == (2, 128, n // 160)
    ref = np.stack([_log_mel64(c, n, g["mel_filters"]) for c in clips])
    err, err_hf = np.abs(got - ref).max(), np.abs(got[:, :, ::10] - g["long_sub"]).max()
    print(f"128-bin long-form log-mel max abs err vs float64 {err:.2e}, vs HF {err_hf:.2e}")
    assert err < 1e-4 and err_hf < 1e-4


def test_logmel_128_longform_conv_input_mask_and_odd_length():
    from oracle import logmel as ol
    g = load_golden("v3")
    clips, fe, r = _longform_128()
    n = max(len(c) for c in clips)
    assert (r["attention_mask"].cpu().numpy() == g["long_attention_mask"]).all()
    c = r.conv_input.float().cpu()
    T = n // 160
    assert c.shape == (2, T + 2, 128) and (c[:, 0] == 0).all() and (c[:, T + 1] == 0).all()
    assert (c[:, 1:T + 1].transpose(1, 2) - bf(r.input_features.cpu()).float()).abs().max() == 0
    # the custom op with n_mels=128 is the same kernel
    import tw.torch_ops  # noqa: F401
    wav = fe.pad_waveforms(clips, n).to(DEV)
    assert torch.equal(torch.ops.tw.log_mel(wav, 128), r.input_features)
    # a length the hop does not divide (the trailing 77 samples reach the last frames through the reflect pad only)
    odd = [ol.synthetic_clip(6, 37.2)[:16000 * 37 + 77], ol.synthetic_clip(1, 5.0)]
    n2 = 16000 * 37 + 77
    r2 = fe(odd, sampling_rate=16000, truncation=False, padding="longest")
    ref2 = np.stack([_log_mel64(c, n2, g["mel_filters"]) for c in odd])
    assert n2 % 160 and r2.input_features.shape == (2, 128, n2 // 160) == ref2.shape
    err2 = np.abs(r2.input_features.cpu().numpy() - ref2).max()
    print(f"128-bin log-mel at {n2} samples max abs err vs float64 {err2:.2e}")
    assert err2 < 1e-4


def test_logmel_80_through_the_mel_count_entry_is_bit_identical():
    from oracle import logmel as ol
    from tw._native import call
    from tw.feature_extraction import mel_tables
    basis, start, w = (t.to(DEV) for t in mel_tables())
    stream = torch.cuda.current_stream().cuda_stream
    for n, clips in ((480000, [ol.synthetic_clip(0), ol.synthetic_clip(3, 12.0)]),
                     (16000 * 37 + 77, [ol.synthetic_clip(6, 37.2), ol.synthetic_clip(1, 5.0)])):
        wav = torch.stack([torch.from_numpy(ol.pad_or_trim(c, n).astype(np.float32)) for c in clips]).to(DEV)
        nfr = n // 160
        out = []
        for name, extra in (("tw_logmel_len", ()), ("tw_logmel_mels", (80,))):
            mel = torch.full((2, 80, nfr), float("nan"), device=DEV)
            conv = torch.full((2, nfr + 2, 80), 9.0, dtype=torch.bfloat16, device=DEV)
            ws = torch.empty(2, dtype=torch.int32, device=DEV)
            call(name, wav.data_ptr(), 2, n, *extra, basis.data_ptr(), start.data_ptr(), w.data_ptr(), mel.data_ptr(),
                 conv.data_ptr(), ws.data_ptr(), stream)
            out.append((mel, conv))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        assert not bool(torch.isnan(out[1][0]).any())
    # any other mel count is refused before anything is launched
    with pytest.raises(RuntimeError):
        call("tw_logmel_mels", wav.data_ptr(), 2, n, 64, basis.data_ptr(), start.data_ptr(), w.data_ptr(),
             mel.data_ptr(), None, ws.data_ptr(), stream)


def test_mel_to_conv_input_at_128():
    from tw import ops
    mel = torch.from_numpy(X.features(2, seed=7, frames=301)).to(DEV)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        xt = torch.full((2, 303, 128), 9.0, dtype=dt, device=DEV)
        ops.mel_to_conv_input(mel, xt)
        assert (xt[:, 0] == 0).all() and (xt[:, 302] == 0).all()
        assert torch.equal(xt[:, 1:302], mel.transpose(1, 2).to(dt))


# ------------------------------------------------------------------------------------------------ model forward
def _model(seed, dtype=torch.float32, compute=None, lin_std=0.02):
    from oracle.weights import make_weights
    from tw.config import WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration
    w = make_weights(X.MICRO_V3, seed, lin_std=lin_std)
    kw = {} if compute is None else {"compute": compute}
    m = WhisperForConditionalGeneration.from_state_dict(WhisperConfig(**X.MICRO_V3),
                                                        {k: torch.from_numpy(v) for k, v in w.items()}, dtype=dtype, **kw)
    assert m.config.num_mel_bins == 128 and m.config.vocab_size == 51866 and m.Vp == 51904
    return m


def _batch(g):
    return dict(input_features=torch.from_numpy(X.features()).to(DEV),
                decoder_input_ids=torch.from_numpy(g["dec"]).to(DEV), labels=torch.from_numpy(g["lab"]).to(DEV))


def test_fp32_forward_logits_match_hf():
    g = load_golden("v3")
    from oracle import labels as L
    dec, lab = L.collate(X.label_lists(), decoder_start_token_id=X.V3["sot"], pad_token_id=X.V3["pad"])
    assert np.array_equal(dec, g["dec"]) and np.array_equal(lab, g["lab"]) and int(lab.max()) == X.LAST
    m = _model(1, compute="fp32")
    out = m(**_batch(g))
    lg = out.logits.float().cpu()
    assert lg.shape == (2, 447, 51866)
    rows = torch.cat([lg[:, X.ROWS, ::X.VSTRIDE], lg[:, X.ROWS, X.LAST:]], -1)
    want = np.concatenate([g["s_rows"], g["s_last"][..., None]], -1)
    e_rows, e_last = rel(rows, want), float((lg[:, X.ROWS, X.LAST] - torch.from_numpy(g["s_last"])).abs().max())
    e_lse = rel(torch.logsumexp(lg, -1), g["s_lse"])
    e_ce = abs(out.loss.item() - float(g["ce"])) / float(g["ce"])
    print(f"v3 fp32 forward: logit rows rel-L2 {e_rows:.2e}, last column max abs {e_last:.2e}, lse rel-L2 {e_lse:.2e}, "
          f"CE rel {e_ce:.2e}")
    assert e_rows < 1e-4 and e_lse < 1e-4 and e_ce < 2e-5
    assert e_last < 1e-4 * float(np.abs(g["s_rows"]).max())


def test_bf16_forward_matches_oracle_and_hf():
    """The micro config's bf16 forward bar (test_distill_gpu.py::test_forward_matches_oracle_and_hf): log-sum-exp
    against the bf16-autocast oracle within one bf16 ulp of the top logit (2^-7 relative) at worst and 3e-4 on average;
    CE 1e-3 against the oracle, HF's autocast run and HF's fp32 run."""
    from oracle.weights import make_weights
    from oracle.whisper_ref import Ref, to_torch
    g = load_golden("v3")
    m = _model(1)
    out = m(**_batch(g))
    ref = Ref(X.MICRO_V3, to_torch(make_weights(X.MICRO_V3, 1)), amp=True)
    with torch.no_grad():
        r = ref.forward(torch.from_numpy(X.features()), torch.from_numpy(g["dec"]), torch.from_numpy(g["lab"]))
    lse, rl = torch.logsumexp(out.logits.float(), -1).cpu(), torch.logsumexp(r["logits"], -1)
    e = (lse - rl).abs() / rl.abs()
    ce = {k: abs(out.loss.item() - v) / v for k, v in (("oracle", r["loss"].item()), ("HF amp", float(g["amp_ce"])),
                                                        ("HF fp32", float(g["ce"])))}
    print(f"v3 micro bf16 fwd: lse max rel {float(e.max()):.2e} mean {float(e.mean()):.2e}  CE rel {ce}")
    assert float(e.max()) <= 2 ** -7 and float(e.mean()) < 3e-4
    assert all(v < 1e-3 for v in ce.values()), ce


def test_fp32_train_step_matches_hf():
    from tw.distill import DistillationTrainer
    g = load_golden("v3")
    s, t = _model(1, compute="fp32"), _model(2, compute="fp32")
    tr = DistillationTrainer(s, t, learning_rate=1e-4, warmup_steps=0, freeze_encoder=True)
    assert tr.share
    m = tr.train_step(_batch(g))
    torch.cuda.synchronize()
    got = {k: float(v.item()) for k, v in m.items()}
    for k, fk in (("loss", "loss"), ("ce_loss", "ce"), ("kl_loss", "kl")):
        r = abs(got[k] - float(g[fk])) / abs(float(g[fk]))
        print(f"v3 fp32 step {k}: {got[k]:.7f} vs HF {float(g[fk]):.7f} (rel {r:.2e})")
        assert r < 2e-5, (k, got[k], float(g[fk]))


# ------------------------------------------------------------------------------------------------ generate
def _decode_model():
    from tw.config import GenerationConfig
    from oracle.fixture_inputs import TW_GENERATION_KEYS
    m = _model(1, lin_std=0.2).set_compute("fp32")
    gc = lambda d: GenerationConfig({k: d[k] for k in TW_GENERATION_KEYS})
    return m, gc


def test_fp32_greedy_and_timestamps_bit_exact_vs_hf():
    from tw.config import LARGE_V3_SUPPRESS
    g = load_golden("v3")
    m, gc = _decode_model()
    assert X.TS_GENERATION_V3["suppress_tokens"] == LARGE_V3_SUPPRESS
    feats = torch.from_numpy(X.features(3, seed=213))
    m.generation_config = gc(X.GREEDY_GENERATION_V3)
    for use_graph in (True, False):
        gen = m.generate(feats, decoder_input_ids=torch.tensor([X.GREEDY_PROMPT] * 3), max_length=64,
                         use_graph=use_graph).cpu().numpy()
        np.testing.assert_array_equal(gen, g["greedy_ids"])
    m.generation_config = gc(X.TS_GENERATION_V3)
    ts = m.generate(feats[:2], return_timestamps=True, language="zh", task="transcribe", max_new_tokens=48).cpu()
    np.testing.assert_array_equal(ts.numpy(), g["ts_ids"])
    assert bool((ts >= 50365).any())


def test_fp32_longform_two_windows_bit_exact_vs_hf():
    g = load_golden("v3")
    m, gc = _decode_model()
    m.generation_config = gc(X.TS_GENERATION_V3)
    lf = torch.from_numpy(X.longform_features())
    trace = []
    out = m.generate(lf, attention_mask=torch.ones(1, lf.shape[-1], dtype=torch.long), return_timestamps=True,
                     language="zh", task="transcribe", temperature=(0.0,), logprob_threshold=-1e9,
                     no_speech_threshold=1.0, _trace=trace).cpu().numpy()
    np.testing.assert_array_equal(out, g["lf_ids"])
    assert len(trace) == 2
    assert [(t["b"], t["seek"]) for t in trace] == list(zip(g["lf_win_b"].tolist(), g["lf_win_seek"].tolist()))
    rows = lambda a: [[int(x) for x in r if x >= 0] for r in a]
    assert [[int(x) for x in t["raw"]] for t in trace] == rows(g["lf_win_ids"])
    assert [t["prompt"] for t in trace] == rows(g["lf_win_prompt"])
    np.testing.assert_allclose([t["avg_logprob"] for t in trace], g["lf_win_avg"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose([t["no_speech_prob"] for t in trace], g["lf_win_ns"], rtol=1e-4, atol=1e-12)


# ------------------------------------------------------------------------------------------------ selection kernels
V3_VOCAB = sc.Vocab("v3", 51866, 51904, 50257, 50364, 50365, (3, 100, 5000, 51866 - 4), (220, 50257), 50365 + 700)
sc.VOCABS.setdefault("v3", V3_VOCAB)


def test_select_cases_reach_the_last_column():
    """The harness' own rows at V = 51866: a row whose maximum is column 51865 (<|30.00|>; a tail that stops at 51865
    misses it), timestamp prefixes ending at it, and padding columns 51866..51903 holding +inf / the largest finite
    value / NaN in every layout (test_select_kernels_gpu._layout)."""
    assert sc.VOCABS["v3"] == V3_VOCAB and V3_VOCAB.V % 8 == 2 and V3_VOCAB.ld - V3_VOCAB.V == 38
    gg = sc.groups("greedy", "v3")
    last = [r for r in gg[0].rows if r.name == "win_last"]
    assert len(last) == 1 and int(last[0].x.argmax()) == 51865
    for gi in (0, 1):
        i = [r.name for r in gg[gi].rows].index("win_last")
        assert sc.group_reference("greedy", "v3", gi, torch.bfloat16)[i]["tok"] == 51865
    assert any(r.gen and r.gen[-1] == 51865 for g in sc.groups("ts", "v3") for r in g.rows)


@pytest.mark.parametrize("kind", ["greedy", "ts"])
@pytest.mark.parametrize("dtype,B", [(torch.bfloat16, 1), (torch.bfloat16, 17), (torch.bfloat16, 100),
                                     (torch.bfloat16, 256), (torch.bfloat16, 257), (torch.float16, 17),
                                     (torch.float32, 17), (torch.float32, 257)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_select_matrix_at_v3(kind, dtype, B):
    from test_select_kernels_gpu import _matrix
    _matrix(kind, "v3", dtype, B)


# ------------------------------------------------------------------------------------------------ LM head and loss
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemv_lm_head_at_51866(M):
    """The decode GEMV at N = 51866, K = 1280 with the fused LayerNorm (the LM head of a large-v3 decode step): an fp64
    matmul of the bf16 operands within one bf16 ulp + 1e-5 (test_gemv_decode's bar), the fused LayerNorm equal to the
    LayerNorm kernel followed by the GEMV bit for bit, each row equal to the row decoded alone."""
    from tw import ops
    N, K = 51866, 1280
    g = torch.Generator().manual_seed(M * 7 + N + K)
    x = bf(torch.randn(M, K, generator=g) * 2 + 0.5)
    W = bf(torch.randn(N, K, generator=g) * 0.03)
    lw, lb = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.1
    xd, Wd, lwd, lbd = x.to(DEV), W.to(DEV), lw.to(DEV), lb.to(DEV)
    y = torch.empty_like(xd)
    ops.layernorm_fwd(xd, lwd, lbd, y)
    C1 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    C2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.gemv(xd, Wd, C1, ln_w=lwd, ln_b=lbd, flags=ops.GEMM_ROUND)
    ops.gemv(y, Wd, C2, flags=ops.GEMM_ROUND)
    assert torch.equal(C1, C2)
    ref = y.cpu().double() @ W.double().t()
    err = (C1.double().cpu() - ref).abs()
    assert (err <= 2 ** -8 * ref.abs() + 1e-5).all(), (float(err.max()), int(err.max(0).values.argmax()))
    assert (err[:, N - 1] <= 2 ** -8 * ref[:, N - 1].abs() + 1e-5).all()
    for i in range(M):
        one = torch.empty(1, N, dtype=torch.bfloat16, device=DEV)
        ops.gemv(xd[i:i + 1], Wd, one, ln_w=lwd, ln_b=lbd, flags=ops.GEMM_ROUND)
        assert torch.equal(one[0], C1[i]), i


def test_kl_ce_at_51866():
    from oracle import distill_ref
    from tw import ops
    g = torch.Generator().manual_seed(3)
    rows, V, ld = 5, 51866, 51904
    s = bf(torch.randn(rows, V, generator=g) * 3).float()
    t = bf(torch.randn(rows, V, generator=g) * 3).float()
    s[1, V - 1], t[3, V - 1] = 11.0, 11.0                  # mass at the column large-v2 does not have
    labels = torch.tensor([17, V - 1, -100, 50365, 4])      # one row masked; one label at the last column
    sl = s.clone().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(sl, labels, ignore_index=-100)
    loss, kl = distill_ref.distill_loss(sl.unsqueeze(0), t.unsqueeze(0), labels.unsqueeze(0), ce)
    loss.backward()
    sd = torch.zeros(rows, ld, dtype=torch.bfloat16, device=DEV); sd[:, :V] = bf(s).to(DEV)
    td = torch.zeros(rows, ld, dtype=torch.bfloat16, device=DEV); td[:, :V] = bf(t).to(DEV)
    lab = labels.to(DEV)
    nv = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.count_valid(lab, nv)
    dl = torch.full((rows, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    out3, _ = ops.kl_ce(sd, td, lab, V, nv, dlogits=dl)
    o = out3.cpu()
    assert int(nv.item()) == 4
    assert abs(o[1] - ce.item()) / ce.item() < 1e-4
    assert abs(o[2] - kl.item()) / kl.item() < 1e-4
    assert abs(o[0] - loss.item()) / loss.item() < 1e-4
    gd = dl.float().cpu()
    assert (gd[:, V:] == 0).all() and (gd[2] == 0).all()
    assert (gd[:, :V] - sl.grad).abs().max() <= 2 ** -7 * sl.grad.abs().max()
    assert float(gd[1, V - 1]) != 0 and float(gd[3, V - 1]) != 0
    out3b, _ = ops.kl_ce(sd, td, lab, V, nv, dlogits=sd)
    torch.cuda.synchronize()
    assert torch.equal(sd, dl) and torch.equal(out3b, out3)


# ------------------------------------------------------------------------------------------------ directories, drivers
def _save(m, d):
    from tw.config import large_v3_generation_config
    m.generation_config = large_v3_generation_config()
    m.save_pretrained(str(d))
    return str(d)


def test_student_from_v3_teacher_directory(tmp_path):
    from oracle.weights import make_weights
    from tw.config import WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration
    from tw.student import init_student_model_from_teacher
    cfg = dict(X.MICRO_V3, decoder_layers=3)
    t = WhisperForConditionalGeneration.from_state_dict(
        WhisperConfig(**cfg), {k: torch.from_numpy(v) for k, v in make_weights(cfg, 7).items()}, dtype=torch.float32)
    tdir, sdir = _save(t, tmp_path / "teacher"), str(tmp_path / "student")
    zh, en = (t.state_view("model.decoder.embed_tokens.weight")[i].clone() for i in (50260, 50259))
    st = init_student_model_from_teacher(tdir, decoder_layers=2, save_dir=sdir, mix_lang_emb=True)
    assert st.config.num_mel_bins == 128 and st.config.vocab_size == 51866 and st.config.decoder_layers == 2
    back = WhisperForConditionalGeneration.from_pretrained(sdir, device=DEV)
    assert back.config.num_mel_bins == 128 and back.config.vocab_size == 51866
    E, Eb = st.state_view("model.decoder.embed_tokens.weight"), back.state_view("model.decoder.embed_tokens.weight")
    assert E.shape[0] >= 51866 and torch.equal(E[:51866], Eb[:51866])
    assert torch.equal(E[50260], zh * 0.5 + en * 0.5) and torch.equal(E[51865], t.state_view(
        "model.decoder.embed_tokens.weight")[51865])
    assert back.generation_config.no_timestamps_token_id == 50364
    with open(os.path.join(sdir, "config.json")) as f:
        c = json.load(f)
    assert c["num_mel_bins"] == 128 and c["vocab_size"] == 51866


def test_drivers_on_a_v3_shaped_directory(tmp_path):
    """run_distillation's entry point (train + eval with generate) and the pseudo-labelling driver on large-v3 shaped
    micro directories: the front end and the label layout come from the directories, no id or mel count is passed."""
    from test_pseudo_labelling_gpu import _wav
    from test_run_distillation_gpu import _corpus
    from oracle import logmel
    from tw import dataset as D, pseudo_labelling as pl
    from tw.data import SpecialTokens
    from tw.feature_extraction import WhisperFeatureExtractor
    from tw.run_distillation import main
    teacher, student = _save(_model(2), tmp_path / "teacher"), _save(_model(1), tmp_path / "student")
    man = _corpus(str(tmp_path / "corpus"))
    # the feed the entry point builds: 128-bin conv input, <|notimestamps|> = 50364 where timestamps are dropped
    sp = SpecialTokens.for_vocab(51866)
    tok = D.WhisperTokenizerAdapter(lambda s: list(s.encode("utf-8")), language="zh", vocab_size=51866)
    feed = D.DataFeed(D.CoolDataset(man), tok, 2, device=DEV, shuffle=False, workers=2, timestamp_probability=0.0,
                      condition_on_prev_probability=0.0, specials=sp,
                      feature_extractor=WhisperFeatureExtractor.from_pretrained(student, device=DEV))
    batch = next(feed)
    assert batch["conv_input"].shape == (2, 3002, 128) and batch["input_features"].shape == (2, 128, 3000)
    lab = batch["labels"][0].cpu().tolist()
    assert lab[:3] == [50260, 50360, 50364] and max(lab) < 50365 and 50363 not in lab
    out = str(tmp_path / "out")
    res = main(["--model_name_or_path", student, "--teacher_model_name_or_path", teacher, "--output_dir", out,
                "--train_dataset_manifest", man, "--eval_dataset_manifest", man, "--per_device_train_batch_size", "2",
                "--per_device_eval_batch_size", "3", "--learning_rate", "1e-4", "--lr_scheduler_type",
                "constant_with_warmup", "--warmup_steps", "1", "--save_steps", "2", "--save_total_limit", "1",
                "--logging_steps", "1", "--freeze_encoder", "True", "--dtype", "bfloat16", "--language", "zh",
                "--timestamp_probability", "0.5", "--condition_on_prev_probability", "0.2", "--do_eval", "True",
                "--predict_with_generate", "True", "--max_label_length", "64", "--byte_level_text_tokenizer", "True",
                "--dataloader_num_workers", "2", "--streaming", "False", "--max_steps", "2", "--eval_steps", "2"])
    assert [h["step"] for h in res["train"]] == [1, 2]
    assert all(np.isfinite(h["loss"]) and h["loss"] > 0 for h in res["train"])
    assert len(res["eval"]) == 1 and np.isfinite(res["eval"][0]["loss"]) and 0 <= res["eval"][0]["wer"]
    with open(os.path.join(out, "config.json")) as f:
        c = json.load(f)
    assert c["num_mel_bins"] == 128 and c["vocab_size"] == 51866
    # pseudo-labelling on the trained directory
    files = []
    for i, secs in enumerate((7.0, 3.0)):
        p = tmp_path / f"clip{i}.wav"
        _wav(p, logmel.synthetic_clip(10 + i, secs))
        files.append(str(p))
    pm = tmp_path / "manifest.csv"
    pm.write_text("audio_path\n" + "\n".join(files) + "\n")
    pout = tmp_path / "pl"
    got = pl.main(["--dataset_path", str(pm), "--output_dir", str(pout), "--model_size_or_path", out,
                   "--chunk_length", "5", "--batch_size", "3", "--num_workers", "2", "--max_new_tokens", "16",
                   "--byte_level_text_tokenizer", "True", "--log_progress", "False"])
    assert sorted(os.listdir(pout)) == ["clip0.csv", "clip1.csv"]
    assert [len(got[f]) for f in files] == [2, 1]
