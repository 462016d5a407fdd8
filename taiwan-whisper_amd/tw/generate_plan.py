"""What one generate call asks for, decided on the host before any device work: plan_generate checks the arguments
(every error that does not depend on a device result, in one order) and returns a Request; tw/generation.py obeys it.
Nothing here touches a model method or a device tensor, so the decision is tested on the CPU
(tests/test_generate_plan_cpu.py).  The pure helpers the decision is made of live here too: the language forms and the
prompt they give, the repeat options, the checks of an assistant, the length cap."""
from __future__ import annotations

import dataclasses
import types

import torch

from .ops import LANG_MAX, MQ_MAX


def gc_get(gc, name):
    """A generation config's own value of `name` (None when it names none; not the Whisper default)."""
    if gc is None:
        return None
    return gc.get(name) if isinstance(gc, dict) else getattr(gc, name, None)


def _lang_id(gc, language):
    if language is None:
        return None
    if isinstance(language, int):
        return language
    l2i = dict(gc.lang_to_id or {})
    for key in (language, f"<|{language}|>"):
        if key in l2i:
            return l2i[key]
    builtin = {"en": 50259, "zh": 50260}
    lang = language.strip("<|>")
    if lang in builtin:
        return builtin[lang]
    raise ValueError(f"unknown language {language!r} (generation_config.lang_to_id has {sorted(l2i)[:5]}...)")


def build_prompt(gc, language=None, task=None, return_timestamps=False, detected=False):
    """HF Whisper prompt: [SOT, <|lang|>, <|task|>, (<|notimestamps|>)] (generation_whisper.py).  detected: the
    language comes from detection, not from the caller; HF then adds a task token only for a task that was passed
    (_retrieve_init_tokens defaults to <|transcribe|> only `elif language is not None`)."""
    ids = [gc.decoder_start_token_id]
    lid = _lang_id(gc, language)
    if lid is not None:
        ids.append(lid)
    if task is not None or (lid is not None and not detected):
        ids.append(dict(gc.task_to_id or {}).get(task or "transcribe", 50359))
    if not return_timestamps:
        ids.append(gc.no_timestamps_token_id)
    return ids


AUTO = "auto"          # generate(language="auto"): HF's language=None, detection per row


def language_table(gc, V):
    """The ids tw_lang_detect chooses among: sorted(generation_config.lang_to_id.values()), checked here because the
    kernel's C entry cannot look into device memory -- unique (ascending once sorted), inside [0, V), at most
    ops.LANG_MAX.  An empty or missing lang_to_id raises ValueError."""
    l2i = gc_get(gc, "lang_to_id")
    if not l2i:
        raise ValueError("tw: language detection needs generation_config.lang_to_id (the generation config names no "
                         "language tokens)")
    ids = sorted(int(v) for v in dict(l2i).values())
    if len(set(ids)) != len(ids) or ids[0] < 0 or ids[-1] >= V or len(ids) > LANG_MAX:
        raise ValueError(f"tw: generation_config.lang_to_id must hold 1..{LANG_MAX} distinct ids in [0, {V}); got "
                         f"{len(ids)} ids from {ids[0]} to {ids[-1]}")
    return ids


def language_rows(gc, language, B):
    """generate's `language` -> None (no language token), AUTO, or one language id per row.  A list or tuple names
    one language per row, each whatever a single `language` may be; HF's errors (_retrieve_init_tokens): TypeError
    for a None element, ValueError for a length other than the batch size."""
    if isinstance(language, (list, tuple)):
        if any(l is None for l in language):
            raise TypeError("Expected `language` to be `None`, a single string (e.g. `'en'`), or a list of strings "
                            "with length equal to the batch size (e.g. `('en', 'fr')` for a batch size of 2). Got a "
                            "list containing `None`.")
        if len(language) != B:
            raise ValueError("When passing a list of languages, the length of the list must match the batch size. "
                             f"Expected length of {B}, but got {len(language)} languages.")
        return [_lang_id(gc, l) for l in language]
    if isinstance(language, str) and language == AUTO:
        return AUTO
    lid = _lang_id(gc, language)
    return None if lid is None else [lid] * B


def total_length(cfg, gc, P, max_length=None, max_new_tokens=None):
    """Length cap of prompt + generated tokens, HF _set_max_new_tokens_and_length
    (generation_whisper.py:1919-1945): max_new_tokens counts after the P prompt tokens; a max_length
    (the call's, else generation_config's) is raised by the min(max_target_positions // 2 - 1, P)
    initial tokens; both capped at max_target_positions."""
    if max_new_tokens is not None:
        total = P + int(max_new_tokens)
    else:
        ml = max_length or gc.max_length or cfg.max_target_positions
        total = int(ml) + min(cfg.max_target_positions // 2 - 1, P)
    return min(total, cfg.max_target_positions)


# keywords generate implements beyond its named parameters (the fallback settings of HF's long-form generate, the
# engine's own switches and the tests' private hooks); anything else raises TypeError instead of being dropped
GENERATE_KEYWORDS = frozenset({"temperature", "compression_ratio_threshold", "logprob_threshold", "no_speech_threshold",
                               "condition_on_prev_tokens", "do_sample", "seed", "fallback_batch", "_trace", "_keep",
                               "repetition_penalty", "no_repeat_ngram_size"})


def repeat_options(gc, kw):
    """generate's repetition_penalty / no_repeat_ngram_size -> (penalty, n): the call's value, else the generation
    config's when it names one (as HF merges them), else off (1.0, 0).  HF's checks: the penalty a strictly positive
    float (RepetitionPenaltyLogitsProcessor; 1 adds no processor, so an int 1 passes), the size a non-negative int."""
    def pick(name):
        v = kw.get(name)
        return v if v is not None else gc_get(gc, name)
    p, n = pick("repetition_penalty"), pick("no_repeat_ngram_size")
    if p is None or (not isinstance(p, bool) and isinstance(p, (int, float)) and p == 1):
        p = 1.0
    elif not isinstance(p, float) or not p > 0:
        raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {p!r}")
    if n is None:
        n = 0
    elif isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"`no_repeat_ngram_size` has to be a non-negative integer, but is {n!r}")
    return float(p), int(n)


def _repeat_names(penalty, ngram):
    return " and ".join(nm for nm, on in (("repetition_penalty", penalty != 1.0), ("no_repeat_ngram_size", ngram > 0))
                        if on)


# Drafted tokens per round when generate(assistant_model=...) is given no num_assistant_tokens.  A guess from byte
# counts, not a measurement: a large-v2 verify pass reads the decoder's weights once whatever Q is, a distil-32-2
# draft step reads 1/16 of the layers plus the LM head, so a handful of drafts costs little beside one target step
# (tools/bench_spec.py times both; the end-to-end gain depends on the acceptance rate of real checkpoints, which is
# unmeasured).  HF's default (20 with a heuristic schedule) differs; for greedy decoding the output does not depend on it.
DEFAULT_ASSISTANT_TOKENS = 4
MAX_ASSISTANT_TOKENS = MQ_MAX - 1

_ASSIST_GC_KEYS = ("eos_token_id", "pad_token_id", "decoder_start_token_id", "suppress_tokens", "begin_suppress_tokens",
                   "no_timestamps_token_id", "max_initial_timestamp_index", "lang_to_id", "task_to_id")


def check_assistant(model, assistant, num_assistant_tokens, num_beams):
    """The argument checks of generate(assistant_model=...) -> None or (assistant, k).  Of `model` only config and
    generation_config are read.  ValueError: beam search with an assistant (as HF), a vocabulary or generation config
    that differs from the target's (the drafts are compared id by id and selected with the target's rules), a
    decoder-only assistant of another width."""
    if assistant is None:
        if num_assistant_tokens is not None:
            raise ValueError("tw generate: num_assistant_tokens needs an assistant_model")
        return None
    if num_beams > 1:
        raise ValueError("tw generate: assisted decoding is greedy (num_beams must be 1), as HF's is")
    k = DEFAULT_ASSISTANT_TOKENS if num_assistant_tokens is None else int(num_assistant_tokens)
    if k < 1:
        raise ValueError(f"num_assistant_tokens={num_assistant_tokens!r}: at least 1")
    k = min(k, MAX_ASSISTANT_TOKENS)
    cfg, ac = model.config, getattr(assistant, "config", None)
    if ac is None:
        raise ValueError("tw generate: assistant_model must be a tw WhisperForConditionalGeneration or WhisperForCausalLM")
    if ac.vocab_size != cfg.vocab_size:
        raise ValueError(f"tw generate: the assistant's vocabulary ({ac.vocab_size}) differs from the target's "
                         f"({cfg.vocab_size})")
    ga, gt = assistant.generation_config, model.generation_config
    for key in _ASSIST_GC_KEYS:
        va, vt = gc_get(ga, key), gc_get(gt, key)
        if va is not None and vt is not None and va != vt:
            raise ValueError(f"tw generate: the assistant's generation config differs from the target's in {key}")
    if getattr(assistant, "decoder_only", False) and ac.d_model != cfg.d_model:
        raise ValueError(f"tw generate: a decoder-only assistant decodes over the target's encoder output: d_model "
                         f"{ac.d_model} != {cfg.d_model}")
    return assistant, k


GREEDY, BEAM, ASSISTED = "greedy", "beam", "assisted"
PREFILL, OWN_PASS = "prefill", "own_pass"


@dataclasses.dataclass(frozen=True)
class Request:
    """One generate call, resolved: everything the call needs to know after its arguments were checked."""
    long_form: bool                 # the seek loop (_longform); else one decode of <= 30 s inputs
    decoder: str                    # GREEDY, BEAM or ASSISTED (long-form: of the temperature-0 attempt of a window)
    num_beams: int
    assistant: object               # ASSISTED: the assistant model and the drafted tokens per round
    k: int
    timestamps: bool
    use_graph: bool
    max_length: int                 # as given
    max_new_tokens: int             # as given
    prompt_ids: tuple               # ints in front of every task prompt, or None
    decoder_input_ids: object       # the caller's own prompt (short-form), or None
    languages: object               # None (no language token), AUTO, or one language id per row
    detection: str                  # AUTO: PREFILL (inside the decode's prefill, on the device) or OWN_PASS; else None
    task: str
    return_language: bool
    repetition_penalty: float
    no_repeat_ngram_size: int
    temps: tuple                    # the fallback settings (long-form)
    compression_ratio_threshold: float
    logprob_threshold: float
    no_speech_threshold: float
    condition_on_prev_tokens: bool
    seed: int
    fallback_batch: bool
    track: bool                     # the selection tracks log-probs / samples (a threshold or a temperature needs it)
    trace: list                     # the tests' private hooks _trace and _keep
    keep: list
    return_token_logprobs: bool = False     # the log-prob of every returned token beside the ids (forces track)

    @property
    def detected(self):
        """build_prompt's flag: the language token comes from detection."""
        return self.languages == AUTO


def plan_generate(cfg, gc, *, rows, frames, have_features, have_encoder_outputs, max_length=None, num_beams=1,
                  return_timestamps=False, language=None, task=None, decoder_input_ids=None, max_new_tokens=None,
                  use_graph=None, prompt_ids=None, prompt_condition_type=None, assistant_model=None,
                  num_assistant_tokens=None, return_language=False, return_token_logprobs=False, **kw) -> Request:
    """generate's arguments -> the Request, or the argument error generate raises; the checks in the order of their
    precedence.  return_token_logprobs reaches here through generate's **kw: the planner owns the keyword.  cfg, gc: the model's config and its resolved generation config.  rows: the batch size of the inputs
    (0 without any); frames: input_features.shape[-1] or None."""
    unknown = sorted(set(kw) - GENERATE_KEYWORDS)
    if unknown:
        raise TypeError(f"tw generate: unsupported keyword argument(s) {', '.join(unknown)}")
    if prompt_condition_type not in (None, "first-segment", "all-segments"):
        raise ValueError(f"prompt_condition_type={prompt_condition_type!r}: 'first-segment' or 'all-segments'")
    if prompt_condition_type == "all-segments":
        raise NotImplementedError("tw generate: prompt_condition_type='all-segments' is not implemented (the prompt "
                                  "conditions as 'first-segment', HF's default)")
    if prompt_ids is not None:
        prompt_ids = tuple(int(t) for t in torch.as_tensor(prompt_ids).reshape(-1).tolist())
        if decoder_input_ids is not None:
            raise ValueError("tw generate: pass prompt_ids or decoder_input_ids, not both")
        if kw.get("condition_on_prev_tokens"):
            raise NotImplementedError("tw generate: prompt_ids together with condition_on_prev_tokens is not "
                                      "implemented")
        prompt_ids = prompt_ids or None
    nb = max(1, int(num_beams or 1))
    assist = check_assistant(types.SimpleNamespace(config=cfg, generation_config=gc), assistant_model,
                             num_assistant_tokens, nb)
    if assist is not None and have_features and not have_encoder_outputs and rows != 1:
        raise ValueError("tw generate: assisted decoding takes a single input (batch size 1), as HF's does")
    temperature = kw.get("temperature") if kw.get("temperature") is not None else 0.0
    thresholds = [kw.get(n) for n in ("compression_ratio_threshold", "logprob_threshold", "no_speech_threshold")]
    seed = int(kw.get("seed", 0))
    penalty, ngram = repeat_options(gc, kw)
    # HF's beam search applies the two repeat processors to log-probabilities, and it scores its hypotheses in torch:
    # their per-token values are not kept.  The verify pass of assisted decoding would need a history per query row
    # for the repeat processors.  None of these is built
    beamless = " and ".join(n for n in (_repeat_names(penalty, ngram),
                                        "return_token_logprobs" if return_token_logprobs else "") if n)
    if nb > 1 and beamless:
        raise NotImplementedError(f"tw generate: {beamless} with beam search (num_beams > 1) is not implemented")
    if assist is not None and (penalty != 1.0 or ngram > 0):
        raise NotImplementedError(f"tw generate: {_repeat_names(penalty, ngram)} with assisted decoding "
                                  "(assistant_model) is not implemented")
    # a list and "auto" are resolved here; a single language after the other checks, where its error has always
    # come (with decoder_input_ids the caller owns the prompt and a single `language` is not looked at)
    per_row = isinstance(language, (list, tuple)) or (isinstance(language, str) and language == AUTO)
    langs = language_rows(gc, language, rows) if per_row else None
    if langs == AUTO:
        if decoder_input_ids is not None:
            raise ValueError("tw generate: language='auto' builds the prompt around the detected language; with "
                             "decoder_input_ids the caller owns the prompt")
        language_table(gc, cfg.vocab_size)
    if return_language and language is None:
        raise ValueError("tw generate: return_language=True needs a language (a name, a list, or 'auto')")
    if return_language and decoder_input_ids is not None:
        raise ValueError("tw generate: return_language=True with decoder_input_ids: the caller owns the prompt, and "
                         "`language` is not looked at")
    if nb > 1 and langs not in (None, AUTO) and len(set(langs)) > 1:
        raise NotImplementedError("tw generate: beam search decodes one prompt for every clip; the rows of this call "
                                  "name different languages")
    # HF (generation_whisper.py:785-898) runs the seek loop for every input when timestamps are predicted, a
    # <= 30 s one included: a window that ends on a timestamp pair before the end of the audio is followed by
    # another window from that timestamp (tests/test_lv2_decode_gpu.py pins it at large-v2 dims)
    seek_loop = bool(return_timestamps) and decoder_input_ids is None
    long_form = (have_features and not have_encoder_outputs
                 and (frames > 2 * cfg.max_source_positions or seek_loop))        # 3000 feature frames = 30 s
    if not long_form and (kw.get("do_sample") or temperature not in (0, 0.0) or any(t is not None for t in thresholds)):
        # the reference applies fallback / thresholds to long-form inputs only (run_eval.py:659-685)
        raise NotImplementedError("tw generate: temperature fallback and thresholds apply to long-form (> 30 s) "
                                  "inputs, as in the reference; short-form decoding is greedy")
    if not per_row and (long_form or decoder_input_ids is None):
        langs = language_rows(gc, language, rows)
    temps = tuple(temperature) if isinstance(temperature, (list, tuple)) else (temperature,)
    detection = None
    if langs == AUTO:
        # short-form greedy decoding whose <|startoftranscript|> is at position 0 detects in its own prefill; every
        # other form runs detect_language's step first and builds host prompts
        fused = not long_form and nb == 1 and assist is None and not prompt_ids
        detection = PREFILL if fused else OWN_PASS
    return Request(
        long_form=long_form, decoder=ASSISTED if assist is not None else BEAM if nb > 1 else GREEDY, num_beams=nb,
        assistant=assist and assist[0], k=assist and assist[1], timestamps=bool(return_timestamps),
        use_graph=True if use_graph is None else use_graph, max_length=max_length, max_new_tokens=max_new_tokens,
        prompt_ids=prompt_ids, decoder_input_ids=decoder_input_ids,
        languages=langs if langs in (None, AUTO) else tuple(langs), detection=detection, task=task,
        return_language=bool(return_language), repetition_penalty=penalty, no_repeat_ngram_size=ngram, temps=temps,
        compression_ratio_threshold=thresholds[0], logprob_threshold=thresholds[1], no_speech_threshold=thresholds[2],
        condition_on_prev_tokens=bool(kw.get("condition_on_prev_tokens") or False), seed=seed,
        fallback_batch=bool(kw.get("fallback_batch", True)),
        track=(thresholds[1] is not None or thresholds[2] is not None or any(t and t > 0 for t in temps)
               or len(temps) > 1 or bool(return_token_logprobs)),
        trace=kw.get("_trace"), keep=kw.get("_keep"), return_token_logprobs=bool(return_token_logprobs))
