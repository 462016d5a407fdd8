"""Inputs of the prompted-decoding fixtures (tests/golden/prompted.npz) as plain data, shared by the generator
(tests/golden/make_golden_prompted.py, HF Transformers) and the tests (which import neither the generator nor HF)."""
import numpy as np

# <|startofprev|> + nine text ids outside generation_config.suppress_tokens: what get_prompt_ids returns
PROMPT_IDS = [50361] + [1000 + 37 * i for i in range(9)]
COND_LENS = [6500, 4130, 1820]
COND_SEED = 3


# Candidate recordings for the large-v2-dims conditioned fixture: (kind, seed, frames, scale).  The generator decodes
# all of them in one HF call (tests/golden/make_golden_prompted.py search_lv2) and the fixture takes LV2_PICK.
LV2_CANDIDATES = [("noise", 3000, 6500, 0.5), ("noise", 3001, 4130, 0.5), ("noise", 7000, 6500, 2.0),
                  ("silence", 0, 6500, 0.0), ("tone", 0, 6000, 1.0), ("noise", 11000, 3500, 0.5)]
# The search's result at the large-v2 dims, (recording, seek, unpadded prompt length) per seek iteration:
#   2: (0, 2852, 200) (1, 2852, 200) (2, 2268, 9) (3, 2852, 200) (4, 2960, 39) (5, 2852, 135)
#   3: (0, 5064, 227) (2, 4924, 137) (3, 5704, 227) (4, 5414, 81)
# The default-scale Gaussian draws and silence all cut their first window at the same timestamp (prompts of 200, then
# the cut at 227); the louder draw and the tone do not.  Candidates 0 and 2 give rows of 200 / 9 and 227 (cut) / 137.
LV2_PICK = [0, 2]


def lv2_candidate_features(picks):
    """The picked LV2_CANDIDATES zero-padded to the longest -> (features [n, 80, max], attention mask): Gaussian
    features of another draw or scale, silence (all zero), or the log-mel of the synthetic tone clip tiled."""
    from oracle import logmel
    lens = [LV2_CANDIDATES[i][2] for i in picks]
    feats = np.zeros((len(picks), 80, max(lens)), dtype=np.float32)
    mask = np.zeros((len(picks), max(lens)), dtype=np.int64)
    for r, i in enumerate(picks):
        kind, seed, n, scale = LV2_CANDIDATES[i]
        if kind == "noise":
            feats[r, :, :n] = (np.random.default_rng(seed).standard_normal((80, n)) * scale).astype(np.float32)
        elif kind == "tone":
            clip = logmel.log_mel_batch([logmel.synthetic_clip(0)])[0]
            feats[r, :, :n] = np.tile(clip, (1, (n + clip.shape[1] - 1) // clip.shape[1]))[:, :n]
        mask[r, :n] = 1
    return feats, mask


def conditioned_features(lens=COND_LENS, seed=COND_SEED):
    """Recordings of 65 s, 41.3 s and 18.2 s for the condition_on_prev_tokens fixtures, zero-padded to the longest ->
    (features [n, 80, max], attention mask).  The draw (seed 3 of a search over 11) is one whose HF fp32 decode at the
    micro dims meets the fixture's conditions: an iteration whose rows' prompts differ in length, previous text, and a
    prompt cut at max_target_positions // 2 - 1, with no step's top-2 margin under 1e-3."""
    feats = np.zeros((len(lens), 80, max(lens)), dtype=np.float32)
    mask = np.zeros((len(lens), max(lens)), dtype=np.int64)
    for i, n in enumerate(lens):
        feats[i, :, :n] = (np.random.default_rng(1000 * seed + i).standard_normal((80, n)) * 0.5).astype(np.float32)
        mask[i, :n] = 1
    return feats, mask
