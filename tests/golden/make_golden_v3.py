"""Generate tests/golden/v3.npz: the large-v3 family's front end (128 mel bins) and vocabulary (51866 ids) on HF
Transformers 5.15, fp32 on the CPU.

Run in the build container (it needs HF Transformers):   python tests/golden/make_golden_v3.py

  mel    HF WhisperFeatureExtractor(feature_size=128) on the three 30 s-window clips of mel.npz that the 80-bin GPU test
         uses (synthetic_clip(0), synthetic_clip(3, 12.0), one second of zeros) and on mel_long.npz's two long-form
         clips (47.3 s; 65 s): every 10th frame, the row sums, the per-clip maximum, the [201, 128] filter bank and the
         long-form attention mask, as mel.npz / mel_long.npz store them.
  model  HF WhisperForConditionalGeneration at the micro dims with num_mel_bins=128, vocab_size=51866 and the
         oracle.weights recipe (inputs and ids: tests/v3_inputs.py):
           s_rows / s_last / s_lse / s_argmax   teacher-forced fp32 logits of two label rows (positions ROWS, every 97th
                                         column and the last one; log-sum-exp and argmax of every position)
           amp_s_lse / amp_ce            the same forward under bf16 autocast (the reference's own bf16 noise)
           ce / kl / loss                the distillation step's losses for a student (seed 1) / teacher (seed 2) pair
                                         with the frozen encoder shared (gen_micro's recipe in make_golden.py)
           greedy_ids / ts_ids           greedy generate without (GREEDY_GENERATION_V3, a decoder_input_ids prompt) and
                                         with return_timestamps (TS_GENERATION_V3): the large-v3 ids and suppress list
           lf_*                          one long-form call over 45 s: two windows (ids, windows, seeks, prompts)
Only token ids, a few logit rows and scalars are stored; weights and inputs are regenerated from seeds.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import hf_model, logmel, longform_clips, make_weights  # noqa: E402
from make_golden_prompted import run_longform, store  # noqa: E402

import v3_inputs as X  # noqa: E402
from oracle import labels as L  # noqa: E402


def gen_mel(out):
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=X.N_MELS)
    clips = [logmel.synthetic_clip(0), logmel.synthetic_clip(3, 12.0), np.zeros(16000, dtype=np.float32)]
    mel = fe(clips, sampling_rate=16000, return_tensors="np").input_features.astype(np.float32)
    assert mel.shape == (3, X.N_MELS, 3000)
    out["mel_sub"] = mel[:, :, ::10]
    out["mel_rowsum"] = mel.sum(-1)
    out["mel_max"] = mel.reshape(len(clips), -1).max(-1)
    out["mel_filters"] = fe.mel_filters.astype(np.float32)
    r = fe(longform_clips(), sampling_rate=16000, return_tensors="np", truncation=False, padding="longest",
           return_attention_mask=True)
    mel = r.input_features.astype(np.float32)
    out["long_sub"] = mel[:, :, ::10]
    out["long_rowsum"] = mel.sum(-1)
    out["long_max"] = mel.reshape(mel.shape[0], -1).max(-1)
    out["long_shape"] = np.array(mel.shape)
    out["long_attention_mask"] = np.asarray(r.attention_mask).astype(np.int8)
    print("mel", out["mel_sub"].shape, out["long_sub"].shape, flush=True)


def gen_step(out):
    from transformers.modeling_outputs import BaseModelOutput
    cfg = X.MICRO_V3
    S, Tm = hf_model(cfg, make_weights(cfg, 1)).eval(), hf_model(cfg, make_weights(cfg, 2)).eval()
    assert S.model.encoder.conv1.weight.shape[1] == X.N_MELS and S.proj_out.weight.shape[0] == X.VOCAB
    dec, lab = L.collate(X.label_lists(), decoder_start_token_id=X.V3["sot"], pad_token_id=X.V3["pad"])
    feats_t, dec_t, lab_t = torch.from_numpy(X.features()), torch.from_numpy(dec), torch.from_numpy(lab)
    assert int(lab.max()) == X.LAST, "no label at the vocabulary's last column"
    with torch.no_grad():
        so = S(input_features=feats_t, decoder_input_ids=dec_t, labels=lab_t)
        to = Tm(encoder_outputs=BaseModelOutput(so.encoder_last_hidden_state), labels=lab_t)
        T = 2.0
        p = torch.softmax(to.logits / T, -1)
        lq = torch.log_softmax(so.logits / T, -1)
        div = torch.nn.functional.kl_div(lq, p, reduction="none") * (lab_t >= 0).unsqueeze(-1)
        kl = div.sum() / (lab_t >= 0).sum() * T ** 2
        loss = 0.8 * so.loss + 1.0 * kl
        with torch.autocast("cpu", dtype=torch.bfloat16):
            so2 = S(input_features=feats_t, decoder_input_ids=dec_t, labels=lab_t)
    out["ce"], out["kl"], out["loss"] = (np.float64(x.item()) for x in (so.loss, kl, loss))
    out["dec"], out["lab"] = dec, lab
    out["s_lse"] = torch.logsumexp(so.logits, -1).numpy()
    out["s_argmax"] = so.logits.argmax(-1).numpy()
    out["s_rows"] = so.logits[:, X.ROWS, ::X.VSTRIDE].numpy()
    out["s_last"] = so.logits[:, X.ROWS, X.LAST].numpy()
    out["amp_ce"] = np.float64(so2.loss.float().item())
    out["amp_s_lse"] = torch.logsumexp(so2.logits.float(), -1).numpy()
    print("step", float(out["loss"]), float(out["ce"]), float(out["kl"]), flush=True)


def gen_decode(out):
    from transformers import GenerationConfig
    cfg = X.MICRO_V3
    m = hf_model(cfg, make_weights(cfg, 1, lin_std=0.2)).eval()
    feats = torch.from_numpy(X.features(3, seed=213))
    calls = {"n": 0}
    cls = type(m)
    orig = cls.generate_with_fallback

    def count(self, *a, **k):
        calls["n"] += 1
        return orig(self, *a, **k)
    cls.generate_with_fallback = count
    try:
        with torch.no_grad():
            m.generation_config = GenerationConfig(**X.GREEDY_GENERATION_V3)
            out["greedy_ids"] = m.generate(feats, decoder_input_ids=torch.tensor([X.GREEDY_PROMPT] * 3), max_length=64,
                                           num_beams=1, do_sample=False).numpy()
    finally:
        cls.generate_with_fallback = orig
    assert calls["n"] == 1, "the no-timestamp call decoded more than one window"
    with torch.no_grad():
        m.generation_config = GenerationConfig(**X.TS_GENERATION_V3)
        out["ts_ids"] = m.generate(feats[:2], return_timestamps=True, language="zh", task="transcribe",
                                   max_new_tokens=48).numpy()
    assert (out["ts_ids"] >= X.V3["timestamp_begin"]).any(), "the timestamp call emitted no timestamp"
    m.generation_config = GenerationConfig(**X.TS_GENERATION_V3)
    lf = X.longform_features()
    ids, rec = run_longform(m, lf, np.ones((1, lf.shape[-1]), dtype=np.int64), temperature=(0.0,),
                            logprob_threshold=-1e9, no_speech_threshold=1.0)
    assert len(rec["seek"]) == 2 and rec["seek"][0] == 0, ("not a two-window call", rec["seek"])
    store(out, "lf", ids, rec)
    del out["lf_win_margin"], out["lf_win_plen"]
    print("decode", out["greedy_ids"].shape, out["ts_ids"].shape, out["lf_ids"].shape, rec["seek"], flush=True)


def main():
    out = {}
    gen_mel(out)
    gen_step(out)
    gen_decode(out)
    path = os.path.join(HERE, "v3.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "micro_step.npz"))
    print("wrote", path, size, "bytes (micro_step.npz:", cap, ")")
    assert size <= cap


if __name__ == "__main__":
    main()
