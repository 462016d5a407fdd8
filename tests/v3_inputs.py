"""Inputs and settings of the large-v3 family fixture (tests/golden/v3.npz) as plain data, shared by its generator
(tests/golden/make_golden_v3.py: HF Transformers on the CPU) and by test_v3_cpu.py / test_v3_gpu.py, which import
neither the generator nor Transformers.

The large-v3 vocabulary (51866 ids) has one more language token than large-v2's: <|yue|> = 50358, after <|su|>.  Every
special id from <|translate|> upward is therefore one higher than in oracle.weights.SPECIAL.
"""
import numpy as np

from oracle.fixture_inputs import SUPPRESS
from oracle.weights import CONFIGS

V3 = dict(eot=50257, pad=50257, sot=50258, en=50259, zh=50260, yue=50358, translate=50359, transcribe=50360,
          startoflm=50361, startofprev=50362, nospeech=50363, notimestamps=50364, timestamp_begin=50365)
VOCAB, N_MELS = 51866, 128
# the micro parity config with the two large-v3 fields
MICRO_V3 = dict(CONFIGS["micro"], num_mel_bins=N_MELS, vocab_size=VOCAB)
# large-v2's suppress list with every id from 50358 (where <|yue|> was inserted) raised by one
SUPPRESS_V3 = [t + 1 if t >= 50358 else t for t in SUPPRESS]
TS_GENERATION_V3 = dict(decoder_start_token_id=V3["sot"], eos_token_id=V3["eot"], pad_token_id=V3["pad"],
                        bos_token_id=V3["eot"], suppress_tokens=SUPPRESS_V3, begin_suppress_tokens=[220, V3["eot"]],
                        max_length=448, num_beams=1, do_sample=False, no_timestamps_token_id=V3["notimestamps"],
                        is_multilingual=True, lang_to_id={"<|en|>": V3["en"], "<|zh|>": V3["zh"], "<|yue|>": V3["yue"]},
                        task_to_id={"transcribe": V3["transcribe"], "translate": V3["translate"]},
                        max_initial_timestamp_index=50)
# greedy without timestamps (a decoder_input_ids prompt): the timestamp ids are suppressed too, as in
# oracle.fixture_inputs.LV2_GREEDY_SUPPRESS -- with random weights a row can emit a timestamp pair after
# <|notimestamps|>, and HF then decodes a second window for it, a path a trained checkpoint does not reach
GREEDY_PROMPT = [V3["sot"], V3["zh"], V3["transcribe"], V3["notimestamps"]]
GREEDY_GENERATION_V3 = dict(TS_GENERATION_V3, suppress_tokens=SUPPRESS_V3 + list(range(V3["timestamp_begin"], VOCAB)))
ROWS = [0, 3, 4, 57, 200, 446]          # decoder positions whose logit rows are stored
VSTRIDE = 97                             # vocabulary stride of the stored rows
LAST = VOCAB - 1                         # <|30.00|>, the column large-v2 does not have: stored beside the sampled ones
LONG_FRAMES = 4500                       # the long-form input: 45 s, two windows


def features(n=2, seed=211, frames=3000):
    """Deterministic log-mel-range features [n, 128, frames] (the front end itself is pinned by the mel fixture)."""
    return (np.random.default_rng(seed).standard_normal((n, N_MELS, frames)) * 0.5).astype(np.float32)


def longform_features():
    return features(1, seed=212, frames=LONG_FRAMES)


def label_lists():
    """Two label rows in the large-v3 layout: a plain <|notimestamps|> row, and a row with a <|startofprev|> prompt
    and timestamp pairs up to <|30.00|> (id 51865, the vocabulary's last column)."""
    rng = np.random.Generator(np.random.PCG64(5))
    ts = lambda sec: V3["timestamp_begin"] + int(round(sec / 0.02))
    body0 = rng.integers(0, V3["eot"], size=90).tolist()
    row0 = [V3["sot"], V3["zh"], V3["transcribe"], V3["notimestamps"]] + body0 + [V3["eot"]]
    a, b = rng.integers(0, V3["eot"], size=40).tolist(), rng.integers(0, V3["eot"], size=150).tolist()
    row1 = ([V3["startofprev"], 11, 12, 13] + [V3["sot"], V3["yue"], V3["transcribe"], ts(0.0)] + a + [ts(7.5), ts(7.5)]
            + b + [ts(30.0), V3["eot"]])
    assert ts(30.0) == LAST
    return [row0, row1]


def hand_batch():
    """The hand-written label batch of test_v3_cpu.py: (token id lists, previous-segment id lists).  Row 0 carries
    timestamps (dropped when the first draw says so), row 1 a previous segment longer than the cut-off, row 2 is plain."""
    ts = lambda sec: V3["timestamp_begin"] + int(round(sec / 0.02))
    r0 = [V3["sot"], V3["zh"], V3["transcribe"], ts(0.0), 900, 901, 902, ts(1.5), ts(1.5), 903, ts(30.0), V3["eot"]]
    r1 = [V3["sot"], V3["zh"], V3["transcribe"], V3["notimestamps"], 700, 701, 702, V3["eot"]]
    r2 = [V3["sot"], V3["yue"], V3["transcribe"], V3["notimestamps"], 800, 801, V3["eot"]]
    prev1 = [ts(0.0)] + list(range(1000, 1040)) + [ts(4.0)]
    return [r0, r1, r2], [None, prev1, None]
