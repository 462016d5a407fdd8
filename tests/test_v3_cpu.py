"""The large-v3 family on the host side: the 128-bin mel tables, the special-token layout of the 51866-id vocabulary,
the label path with that layout, and the config entries.  The large-v2 defaults are checked beside each, against the
module constants and oracle.labels, to show the default path is untouched."""
import json
import os
import re

import numpy as np
import pytest

import v3_inputs as X
from conftest import REPO, load_golden


# ------------------------------------------------------------------------------------------------ front end tables
def test_feature_extractor_sizes():
    from tw.feature_extraction import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=128, device="cpu")
    assert fe.feature_size == 128 and fe.mel_filters.shape == (201, 128)
    assert WhisperFeatureExtractor(device="cpu").mel_filters.shape == (201, 80)
    with pytest.raises(NotImplementedError):
        WhisperFeatureExtractor(feature_size=64, device="cpu")


def test_feature_extractor_from_pretrained(tmp_path):
    from tw.feature_extraction import WhisperFeatureExtractor
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
    (a / "preprocessor_config.json").write_text(json.dumps({"feature_size": 128, "hop_length": 160}))
    (a / "config.json").write_text(json.dumps({"num_mel_bins": 80}))       # the preprocessor file wins
    (b / "config.json").write_text(json.dumps({"num_mel_bins": 128}))
    (c / "config.json").write_text(json.dumps({"num_mel_bins": 80}))
    sizes = [WhisperFeatureExtractor.from_pretrained(str(d), device="cpu").feature_size for d in (a, b, c)]
    assert sizes == [128, 128, 80]


def test_mel_filters_128_match_hf():
    from tw.feature_extraction import mel_filters
    g = load_golden("v3")
    assert g["mel_filters"].shape == (201, 128)
    np.testing.assert_allclose(mel_filters(n_mels=128).astype(np.float32), g["mel_filters"], rtol=0, atol=1e-7)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_mel_tables_rebuild_the_dense_bank(n_mels):
    from tw.feature_extraction import MELW, mel_filters, mel_tables
    basis, start, w = (t.numpy() for t in mel_tables(n_mels=n_mels))
    assert basis.shape == (400, 416) and start.shape == (n_mels,) and w.shape == (n_mels, MELW)
    fb = mel_filters(n_mels=n_mels).astype(np.float32)
    dense = np.zeros_like(fb)
    for m in range(n_mels):
        taps = int(np.count_nonzero(fb[:, m]))
        assert 1 <= taps <= MELW, (m, taps)                     # no filter is empty or wider than the tap budget
        for j in range(MELW):
            if w[m, j] != 0:
                dense[start[m] + j, m] = w[m, j]
    assert np.array_equal(dense, fb)
    # the default call is still the 80-bin table, and the DFT basis does not depend on the count
    b0, s0, w0 = mel_tables()
    assert s0.shape == (80,) and np.array_equal(b0.numpy(), basis)


def test_log_mel_op_fake_follows_n_mels():
    import torch
    import tw.torch_ops  # noqa: F401
    wav = torch.empty(3, 480000, device="meta")
    assert torch.ops.tw.log_mel(wav).shape == (3, 80, 3000)
    assert torch.ops.tw.log_mel(wav, 128).shape == (3, 128, 3000)
    assert torch.ops.tw.log_mel(torch.empty(2, 756800, device="meta"), n_mels=128).shape == (2, 128, 4730)


# ------------------------------------------------------------------------------------------------ special tokens
def test_special_tokens_by_vocab():
    from tw import data as D
    v2 = D.SpecialTokens.for_vocab(51865)
    assert (v2.eot, v2.pad, v2.sot, v2.transcribe, v2.startofprev, v2.notimestamps, v2.timestamp_begin) == \
        (D.EOT, D.PAD, D.SOT, D.TRANSCRIBE, D.STARTOFPREV, D.NOTIMESTAMPS, D.TIMESTAMP_BEGIN)
    assert (v2.translate, v2.startoflm, v2.nospeech, v2.n_languages, v2.first_timestamp) == \
        (50358, 50360, 50362, 99, 50364)
    v3 = D.SpecialTokens.for_vocab(51866)
    assert (v3.eot, v3.sot, v3.translate, v3.transcribe, v3.startoflm, v3.startofprev, v3.nospeech, v3.notimestamps,
            v3.n_languages) == (50257, 50258, 50359, 50360, 50361, 50362, 50363, 50364, 100)
    # the label side's threshold is <|notimestamps|> (the reference's all_special_ids[-1]); <|0.00|> follows it
    assert v3.timestamp_begin == 50364 and v3.first_timestamp == 50365 and v3.first_timestamp + 1500 == 51865
    assert {k: getattr(v3, k) for k in ("eot", "sot", "translate", "transcribe", "startoflm", "startofprev",
                                        "nospeech", "notimestamps")} == {k: X.V3[k] for k in (
                                            "eot", "sot", "translate", "transcribe", "startoflm", "startofprev",
                                            "nospeech", "notimestamps")}
    for v in (51864, 51867, 1000):
        with pytest.raises(ValueError):
            D.SpecialTokens.for_vocab(v)


def test_special_tokens_from_tokenizer():
    from tw import data as D
    from tw.dataset import whisper_special_tokens

    class Tok:
        def __init__(self, n):
            self.tab = whisper_special_tokens(n)

        def convert_tokens_to_ids(self, t):
            return self.tab.get(t)
    assert D.SpecialTokens.from_tokenizer(Tok(99)) == D.SpecialTokens.for_vocab(51865)
    assert D.SpecialTokens.from_tokenizer(Tok(100)) == D.SpecialTokens.for_vocab(51866)


def test_special_token_tables():
    from tw.dataset import WhisperTokenizerAdapter, whisper_special_tokens
    v2, v3 = whisper_special_tokens(), whisper_special_tokens(100)
    assert v2["<|30.00|>"] == 51864 and v2["<|0.00|>"] == 50364 and "<|yue|>" not in v2 and v2 == whisper_special_tokens(99)
    assert v3["<|30.00|>"] == 51865 and v3["<|yue|>"] == 50358 and v3["<|su|>"] == 50357 == v2["<|su|>"]
    assert v3["<|translate|>"] == 50359 and v3["<|startofprev|>"] == 50362 and v3["<|notimestamps|>"] == 50364
    assert sorted(v3.values()) == list(range(50257, 51866))         # every id above the text range, once
    enc = lambda s: list(s.encode("utf-8"))
    a2 = WhisperTokenizerAdapter(enc, language="zh", predict_timestamps=False)
    a3 = WhisperTokenizerAdapter(enc, language="yue", predict_timestamps=False, vocab_size=51866)
    assert a2.timestamp_ids()[0] == 50364 and a2.prefix_tokens == [50258, 50260, 50359, 50363]
    assert a3.timestamp_ids()[0] == 50365 and a3.timestamp_ids()[-1] == 51865
    assert a3.prefix_tokens == [50258, 50358, 50360, 50364]
    ids = a3("<|0.00|>ab<|30.00|>", add_special_tokens=True).input_ids
    assert ids == [50258, 50358, 50360, 50364, 50365, 97, 98, 51865, 50257]
    assert a3.decode(ids, skip_special_tokens=False) == "<|startoftranscript|><|yue|><|transcribe|><|notimestamps|>" \
        "<|0.00|><|30.00|><|endoftext|>"


# ------------------------------------------------------------------------------------------------ labels
class _Draws:
    """rng.binomial(1, p) answering from a list."""

    def __init__(self, draws):
        self.draws = list(draws)

    def binomial(self, n, p):
        return self.draws.pop(0)


def _restated(rows, prevs, draws, notimestamps, startofprev, cutoff, max_len):
    """prepare_train_dataset's text targets (run_distillation.py:1221-1274) written out for the hand batch: every row
    has a previous-segment column of its own; ids above <|notimestamps|> are timestamps."""
    draws, out = list(draws), []
    for ids, prev in zip(rows, prevs):
        ids = list(ids)
        has_ts = any(t > notimestamps for t in ids)
        keep = True
        if has_ts:
            keep = bool(draws.pop(0))
            if not keep:
                ids = [t for t in ids if t < notimestamps]
                ids.insert(3, notimestamps)
        cond = bool(draws.pop(0))
        if cond and prev is not None:
            prev = list(prev)
            if has_ts and not keep:
                prev = [t if t < notimestamps else 220 for t in prev]
            if len(prev) > cutoff:
                prev = [startofprev] + prev[-cutoff + 1:]
            if len(prev) + len(ids) > max_len:
                prev = [startofprev] + prev[len(prev) + len(ids) - max_len + 1:]
            ids = prev + ids
        out.append(ids)
    return out


# draws in call order: row 0 (has timestamps) drop them, no prompt; row 1 prompt; row 2 no prompt
DRAWS = [0, 0, 1, 0]
MAXLEN = 64             # cut-off 32 < the 42-id previous segment of row 1


def test_prepare_labels_and_collator_v3_layout():
    from tw import data as D
    rows, prevs = X.hand_batch()
    sp = D.SpecialTokens.for_vocab(51866)
    got = D.prepare_labels(rows, prevs, _Draws(DRAWS), max_label_length=MAXLEN, specials=sp)
    want = _restated(rows, prevs, DRAWS, 50364, 50362, MAXLEN // 2, MAXLEN)
    assert got == want
    # row 0: timestamps dropped, <|notimestamps|> = 50364 at position 3, text kept
    assert got[0] == [50258, 50260, 50360, 50364, 900, 901, 902, 903, 50257]
    # row 1: <|startofprev|> = 50362 + the last 31 previous ids (its timestamps kept), then the row
    assert got[1][0] == 50362 and len(got[1]) == 32 + len(rows[1]) and got[1][31] == 50365 + 200
    assert got[1][32:] == rows[1] and got[2] == rows[2]
    dec, lab = D.DataCollatorSpeechSeq2SeqWithPadding(max_target_length=MAXLEN, specials=sp).collate_labels(got)
    dec, lab = dec.numpy(), lab.numpy()
    assert dec.shape == lab.shape == (3, MAXLEN - 1)
    for i, ids in enumerate(got):
        n = len(ids)
        assert dec[i, :n].tolist() == ids and (dec[i, n:] == 50257).all()
        sot = ids.index(50258)
        first = sot if sot > 0 else 0               # labels are shifted by one: a prompt and SOT are masked
        assert (lab[i, :first] == -100).all() and lab[i, first:n - 1].tolist() == ids[first + 1:]
        assert (lab[i, n - 1:] == -100).all()
    assert (lab[1, :32] == -100).all() and lab[1, 32] == 50260


def test_default_label_path_is_the_large_v2_one():
    """The same batch written with large-v2 ids through the default arguments equals oracle.labels."""
    from oracle import labels as L
    from tw import data as D
    rows, prevs = X.hand_batch()
    down = lambda ids: None if ids is None else [t - 1 if t >= 50359 else t for t in ids]      # v3 -> v2 ids
    rows2, prevs2 = [down([t for t in r if t != 50358] if 50358 in r else r) for r in rows], [down(p) for p in prevs]
    rows2[2] = [50258, 50260] + rows2[2][1:]                                                   # <|yue|> -> <|zh|>
    got = D.prepare_labels(rows2, prevs2, _Draws(DRAWS), max_label_length=MAXLEN)
    want = L.prepare_labels(rows2, prevs2, _Draws(DRAWS), max_label_length=MAXLEN)
    assert got == want and got[0][3] == 50363 and got[1][0] == 50361
    assert got == D.prepare_labels(rows2, prevs2, _Draws(DRAWS), max_label_length=MAXLEN,
                                   specials=D.SpecialTokens.for_vocab(51865))
    dec, lab = D.DataCollatorSpeechSeq2SeqWithPadding(max_target_length=MAXLEN).collate_labels(got)
    dec0, lab0 = L.collate(want, max_target_length=MAXLEN)
    assert np.array_equal(dec.numpy(), dec0) and np.array_equal(lab.numpy(), lab0)
    assert D.synthetic_label_lists(4, seed=3) == L.synthetic_label_lists(4, seed=3)
    v3 = D.synthetic_label_lists(4, seed=3, specials=D.SpecialTokens.for_vocab(51866))
    assert [r[r.index(50258):][:4] for r in v3] == [[50258, 50260, 50360, 50364]] * 4


# ------------------------------------------------------------------------------------------------ config
def test_model_dims_and_suppress_list():
    from tw import config as C
    v2 = C.MODEL_DIMS["large-v2"]
    assert "num_mel_bins" not in v2 and "vocab_size" not in v2
    for name, dec in (("large-v3", 32), ("large-v3-turbo", 4), ("distil-large-v3", 2)):
        d = C.MODEL_DIMS[name]
        assert d["num_mel_bins"] == 128 and d["vocab_size"] == 51866
        assert d["encoder_layers"] == 32 and d["decoder_layers"] == dec and d["d_model"] == 1280
        cfg = C.WhisperConfig(**d)
        assert cfg.num_mel_bins == 128 and cfg.vocab_size == 51866
    assert C.LARGE_V3_SUPPRESS == X.SUPPRESS_V3 and len(C.LARGE_V3_SUPPRESS) == len(C.LARGE_V2_SUPPRESS)
    assert C.LARGE_V3_SUPPRESS[-8:] == [49870, 50254, 50258, 50359, 50360, 50361, 50362, 50363]
    assert C.LARGE_V3_SUPPRESS[:-5] == C.LARGE_V2_SUPPRESS[:-5]
    # what tw.generation derives from the list and the config: <|startofprev|> and <|nospeech|>
    gc = C.GenerationConfig(C.large_v3_generation_config())
    assert gc.suppress_tokens[-2] == 50362 and gc.no_timestamps_token_id - 1 == 50363
    assert gc.task_to_id["transcribe"] == 50360 and gc.lang_to_id["<|yue|>"] == 50358


def test_header_declares_the_mel_count_entry():
    from tw import _native
    with open(os.path.join(REPO, "include", "tw_hip.h")) as f:
        m = re.search(r"int tw_logmel_mels\(([^;]*)\);", f.read())
    assert m and len(m.group(1).split(",")) == len(_native.SIGNATURES["tw_logmel_mels"]) == 11
