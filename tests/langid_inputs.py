"""Settings of the language-detection fixtures (tests/golden/langid.npz) as plain data, shared by the generator
(tests/golden/make_golden_langid.py, HF Transformers) and the tests (which import neither it nor HF).  The model and
clips are those of the repetition fixtures (tests/repeat_inputs.py: the micro model, weights seed 1; the three clips
of test_decode_gpu._feats; recordings drawn as prompted_inputs.conditioned_features draws them)."""

# Whisper large-v2's 99 languages in token order: <|en|> = 50259 .. <|su|> = 50357
LANGUAGE_CODES = (
    "en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la mi "
    "ml cy sk te fa lv bn sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be tg sd "
    "gu am yi lo uz fo ht ps tk nn mt sa lb my bo tl mg as tt haw ln ha ba jw su").split()
LANG_TO_ID = {f"<|{c}|>": 50259 + i for i, c in enumerate(LANGUAGE_CODES)}
assert len(LANG_TO_ID) == 99 and LANG_TO_ID["<|zh|>"] == 50260 and LANG_TO_ID["<|su|>"] == 50357

WEIGHT_SEED = 1
LIST_LANGUAGES = ["zh", "en", "zh"]
# short-form cases on the 3 clips: tag -> (generate keywords without `language`, prompt_ids or not).  HF's call has
# language=None (detection) where the engine's has language="auto"; "list" passes LIST_LANGUAGES to both.
SHORT = {
    "auto": (dict(max_length=64), False),                      # no task: HF then adds no task token either
    "auto_ts": (dict(return_timestamps=True, task="transcribe", max_new_tokens=48), False),
    "auto_prompt": (dict(task="transcribe", max_length=64), True),
    # the "en" row's step 14 leads by 6e-5 only in HF's fp32 decode: the case stops before it
    "list": (dict(task="transcribe", max_new_tokens=12), False),
}
# one long-form call of 3 recordings, without and with condition_on_prev_tokens
LONG = {
    "lf": dict(temperature=0.0, max_new_tokens=32, task="transcribe"),
    "lf_cond": dict(condition_on_prev_tokens=True, temperature=0.0, max_new_tokens=32, task="transcribe"),
}
# The recordings' lengths and draw (prompted_inputs.conditioned_features(lens, seed)).  The generator's conditions --
# (a) the detected languages of the clips, and of the recordings, not all equal; (b) every top-2 margin above
# repeat_inputs.TIE_MARGIN; (c) every case differs from its language="zh" call -- were searched over the draws
# LONG_SEEDS in order with the weights seed fixed; LONG_INPUTS holds the first draw that meets them
# (make_golden_langid.py prints the search when run with LANGID_SEARCH=1).
LONG_LENS = [6500, 4130, 1820]
LONG_SEEDS = tuple(range(12))
LONG_INPUTS = (LONG_LENS, 9)
