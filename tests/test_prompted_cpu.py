"""generate's keyword handling and the conditioned prompt assembly (no GPU)."""
import numpy as np
import pytest

from conftest import load_golden


class _Cfg:
    d_model, max_source_positions, max_target_positions, vocab_size, eos_token_id = 128, 1500, 448, 51865, 50257


class _Model:
    config, generation_config, device = _Cfg(), None, "cpu"


def test_generate_rejects_unknown_keywords():
    from tw.generation import GENERATE_KEYWORDS, generate
    with pytest.raises(TypeError, match="no_such_option"):
        generate(_Model(), None, no_such_option=1)
    with pytest.raises(TypeError, match="prompt_idz"):
        generate(_Model(), None, prompt_idz=[50361, 5])
    # what the callers in the package, the benchmark and the tests pass stays accepted
    assert {"temperature", "compression_ratio_threshold", "logprob_threshold", "no_speech_threshold",
            "condition_on_prev_tokens", "seed", "fallback_batch", "_trace", "_keep"} <= GENERATE_KEYWORDS


def test_all_segments_is_not_implemented():
    from tw.generation import generate
    with pytest.raises(NotImplementedError, match="all-segments"):
        generate(_Model(), None, prompt_ids=[50361, 5], prompt_condition_type="all-segments")
    with pytest.raises(ValueError):
        generate(_Model(), None, prompt_ids=[50361, 5], prompt_condition_type="some-segments")


def _rows(a):
    return [[int(x) for x in r if x != -1] for r in a]


@pytest.mark.parametrize("tag", ["cond0", "condf", "lv2_condf"])
def test_conditioned_prompts_match_hf(tag):
    """Replay HF's recorded windows through the prompt assembly: from each recording's accepted segments (rebuilt from
    the recorded window tokens with retrieve_segment, as the seek loop does) the unpadded prompts, the padded length
    and the pad counts of every seek iteration are HF's decoder_input_ids."""
    from tw.generation import conditioned_prompts, retrieve_segment
    g = load_golden("prompted")
    if f"{tag}_ids" not in g:
        pytest.fail(f"tests/golden/prompted.npz has no {tag} part")
    ts_begin, eos, cut, prev_sot, window = 50364, 50257, 448 // 2 - 1, 50361, 3000
    init = [50258, 50260, 50359]
    lens = [6500, 6500] if tag.startswith("lv2") else [6500, 4130, 1820]
    bs, seeks = g[f"{tag}_win_b"].tolist(), g[f"{tag}_win_seek"].tolist()
    prompts, ids, plen = _rows(g[f"{tag}_win_prompt"]), _rows(g[f"{tag}_win_ids"]), g[f"{tag}_win_plen"].tolist()
    segments = [[] for _ in lens]
    seen_cut = False
    i = 0
    while i < len(bs):
        j, level = i, []
        while j < len(bs) and bs[j] not in level:
            level.append(bs[j])
            j += 1
        got, P = conditioned_prompts(init, [segments[b] for b in level], [True] * len(level),
                                     len(segments[0]) > 0, prev_sot, cut, ts_begin)
        assert got == prompts[i:j]
        assert {P} == set(plen[i:j])
        assert [P - len(p) for p in got] == [plen[k] - len(prompts[k]) for k in range(i, j)]
        seen_cut |= any(len(p) == 1 + cut + len(init) for p in got)
        for k in range(i, j):
            b, seq = bs[k], list(ids[k])
            n = min(window, lens[b] - seeks[k])
            if seeks[k] + window < lens[b] and seq and seq[-1] == eos:
                seq = seq[:-1]
            while len(seq) > 1 and seq[-1] == eos and seq[-2] == eos:      # trailing pads (pad == eos keeps one)
                seq = seq[:-1]
            segs, _ = retrieve_segment(seq, n, ts_begin)
            segments[b].extend(list(s) for s in segs)
        i = j
    assert seen_cut


def test_conditioned_prompts_unconditioned_rows():
    from tw.generation import conditioned_prompts
    init = [50258, 50260, 50359, 50363]
    got, P = conditioned_prompts(init, [[[5, 6]], []], [True, True], False, 50361, 223, 50364)
    assert got == [init, init] and P == 4
    # conditioned: a row without previous text (or not conditioning) carries <|startofprev|> alone; a segment closing
    # on a timestamp pair loses its last timestamp; the text is cut to its last cut_off tokens
    segs = [[50364, 7, 8, 50370, 50370], [9]]
    got, P = conditioned_prompts(init, [segs, [], segs], [True, True, False], True, 50361, 3, 50364)
    assert got == [[50361, 8, 50370, 9] + init, [50361] + init, [50361] + init] and P == 8
