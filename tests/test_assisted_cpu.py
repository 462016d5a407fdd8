"""The argument checks of generate(assistant_model=..., num_assistant_tokens=...) that need no GPU."""
import types

import pytest
import torch


class _Cfg:
    d_model, max_source_positions, max_target_positions, vocab_size, eos_token_id = 128, 1500, 448, 51865, 50257


class _Model:
    config, generation_config, device = _Cfg(), None, "cpu"


def _assistant(**over):
    cfg = types.SimpleNamespace(vocab_size=51865, d_model=128)
    a = types.SimpleNamespace(config=cfg, generation_config=None, decoder_only=False)
    for k, v in over.items():
        setattr(cfg if hasattr(cfg, k) else a, k, v)
    return a


def test_unknown_keyword_still_raises():
    from tw.generation import generate
    with pytest.raises(TypeError, match="no_such_option"):
        generate(_Model(), None, no_such_option=1)
    with pytest.raises(TypeError, match="no_such_option"):
        generate(_Model(), None, assistant_model=_assistant(), num_assistant_tokens=3, no_such_option=1)


def test_new_keywords_are_accepted():
    """assistant_model / num_assistant_tokens pass the keyword check and their own validation: the call goes on to
    the next argument check (here: all-segments prompts are not implemented)."""
    from tw.generation import generate
    with pytest.raises(NotImplementedError, match="all-segments"):
        generate(_Model(), None, assistant_model=_assistant(), num_assistant_tokens=3, prompt_ids=[50361, 5],
                 prompt_condition_type="all-segments")
    import inspect
    sig = inspect.signature(generate).parameters
    assert sig["assistant_model"].default is None and sig["num_assistant_tokens"].default is None


def test_batch_and_beams_raise():
    from tw.generation import generate
    with pytest.raises(ValueError, match="batch size 1"):
        generate(_Model(), torch.zeros(2, 80, 3000), assistant_model=_assistant())
    with pytest.raises(ValueError, match="num_beams"):
        generate(_Model(), torch.zeros(1, 80, 3000), assistant_model=_assistant(), num_beams=2)
    with pytest.raises(ValueError, match="needs an assistant_model"):
        generate(_Model(), torch.zeros(1, 80, 3000), num_assistant_tokens=4)
    with pytest.raises(ValueError, match="at least 1"):
        generate(_Model(), torch.zeros(1, 80, 3000), assistant_model=_assistant(), num_assistant_tokens=0)


def test_vocabulary_config_and_width_must_match():
    from tw.config import GenerationConfig
    from tw.generation import check_assistant
    m = _Model()
    with pytest.raises(ValueError, match="vocabulary"):
        check_assistant(m, _assistant(vocab_size=51864), None, 1)
    with pytest.raises(ValueError, match="d_model"):
        check_assistant(m, _assistant(d_model=256, decoder_only=True), None, 1)
    check_assistant(m, _assistant(d_model=256), None, 1)          # its own encoder: any width
    m2 = _Model()
    m2.generation_config = GenerationConfig(suppress_tokens=[1, 2], eos_token_id=50257)
    a = _assistant()
    a.generation_config = GenerationConfig(suppress_tokens=[1, 3], eos_token_id=50257)
    with pytest.raises(ValueError, match="suppress_tokens"):
        check_assistant(m2, a, None, 1)
    a.generation_config = GenerationConfig(suppress_tokens=[1, 2], eos_token_id=50257, forced_decoder_ids=None)
    assert check_assistant(m2, a, None, 1) == (a, 4)


def test_default_and_cap_of_num_assistant_tokens():
    from tw.generation import DEFAULT_ASSISTANT_TOKENS, MAX_ASSISTANT_TOKENS, check_assistant
    a = _assistant()
    assert DEFAULT_ASSISTANT_TOKENS == 4 and MAX_ASSISTANT_TOKENS == 7
    assert check_assistant(_Model(), a, None, 1) == (a, 4)
    assert check_assistant(_Model(), a, 20, 1) == (a, 7)
    assert check_assistant(_Model(), None, None, 1) is None


def test_signatures_of_the_new_entry_points():
    from tw import _native
    for name in ("tw_decode_attn_mq", "tw_spec_accept", "tw_embed_step_multi"):
        assert name in _native.SIGNATURES
