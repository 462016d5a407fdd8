"""The planted cases of tests/select_cases.py can see the bugs they are meant for (no GPU needed): every rule state
is reached, every rule-drop mutant of the timestamp rules changes the pick of some case, and the mass-rule comparison
of every case but (d) is at least 1e-3 away from a tie, so the kernels' fp32 / fast-exp evaluation cannot
legitimately take the other branch."""
import pytest
import torch

import select_cases as sc

NEG = sc.NEG


def mutant_rules(drop, before=()):
    """timestamp_rules restated with one rule removed (drop=None: the full rules).  before: ids ahead of begin_col
    that the pair state wrongly looks at (the window's own last timestamp still comes from gen, as last_ts[b])."""
    def rules(lg, gen, first, ts_begin, no_ts, eos, max_initial, apply_mass=True):
        lg = lg.clone()
        if drop != "no_ts":
            lg[no_ts] = NEG
        seq = list(before) + list(gen)
        last = len(seq) >= 1 and seq[-1] >= ts_begin
        pen = len(seq) < 2 or seq[-2] >= ts_begin
        if last and pen and drop != "closed_pair":
            lg[ts_begin:] = NEG
        if last and not pen and drop != "open_pair":
            lg[:eos] = NEG
        stamps = [t for t in gen if t >= ts_begin]
        if stamps and drop != "monotonic":
            closing = last and not pen
            if drop == "lim_always_last":
                closing = True
            if drop == "lim_always_next":
                closing = False
            lg[ts_begin:(stamps[-1] if closing else stamps[-1] + 1)] = NEG
        if first and drop != "first_text":
            lg[:ts_begin] = NEG
        if first and max_initial is not None and drop != "max_initial":
            lg[ts_begin + max_initial + 1:] = NEG
        if apply_mass and drop != "mass":
            lp = torch.log_softmax(lg.float(), -1)
            if lp[ts_begin:].logsumexp(-1) > lp[:ts_begin].max():
                lg[:ts_begin] = NEG
        if apply_mass and drop == "mass_ge":                 # >= where HF has >
            lp = torch.log_softmax(lg.float(), -1)
            if lp[ts_begin:].logsumexp(-1) >= lp[:ts_begin].max():
                lg[:ts_begin] = NEG
        return lg
    return rules


MUTANTS = ("no_ts", "closed_pair", "open_pair", "monotonic", "lim_always_last", "lim_always_next", "first_text",
           "max_initial", "mass", "mass_ge")


def _pick(g, row, rules):
    return sc.lowest_argmax(sc.processed_row(g, row, torch.float32, rules=rules))


@pytest.mark.parametrize("vocab", ["small", "real"])
def test_restated_rules_equal_the_oracle(vocab):
    full = mutant_rules(None)
    for g in sc.groups("ts", vocab):
        for r in g.rows:
            a = sc.processed_row(g, r, torch.float32)
            b = sc.processed_row(g, r, torch.float32, rules=full)
            assert torch.equal(a, b), (g.name, r.name)


@pytest.mark.parametrize("vocab", ["small", "real"])
def test_every_prefix_state_reached(vocab):
    voc = sc.VOCABS[vocab]
    for bc in (0, 5):
        gs = [g for g in sc.groups("ts", vocab) if g.begin_col == bc]
        seen = {r.state for g in gs for r in g.rows}
        assert seen == set(sc.PREFIXES), (bc, seen)
        lasts = {sc.row_last_ts(voc, r) for g in gs for r in g.rows}
        assert lasts == {-1, voc.ts_begin, voc.mid, voc.V - 1}
        assert {(g.max_initial, g.begin_on) for g in gs if g.first} == {(m, b) for m in (-1, 0, 50) for b in (False, True)}
        for g in gs:
            for r in g.rows:
                assert len(r.prompt) == bc and len(r.prompt) + len(r.gen) == g.col
                if bc:
                    assert sum(t >= voc.ts_begin for t in r.prompt) >= 2      # a conditioned prompt holds timestamps
        kinds = {r.kind for g in gs for r in g.rows}
        assert {"mass_a", "mass_b", "mass_d", "forbid:ts_below_lim", "forbid:text_in_open_pair",
                "forbid:ts_in_closed_pair", "forbid:text_at_first", "forbid:ts_above_max_initial", "done"} <= kinds


@pytest.mark.parametrize("vocab", ["small", "real"])
def test_no_ts_is_the_maximum_of_every_row(vocab):
    voc = sc.VOCABS[vocab]
    for g in sc.groups("ts", vocab):
        for r in g.rows:
            assert int(torch.argmax(r.x)) == voc.no_ts and float(r.x.abs()[torch.isfinite(r.x)].max()) <= 14.0


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=str)
@pytest.mark.parametrize("vocab", ["small", "real"])
def test_mass_margin_of_every_case(vocab, dtype):
    n = 0
    for g in sc.groups("ts", vocab):
        for r in g.rows:
            if r.kind == "mass_d":
                continue
            n += 1
            assert sc.mass_margin(g, r, dtype) >= sc.MASS_MARGIN, (g.name, r.name)
    assert n == sum(r.kind != "mass_d" for g in sc.groups("ts", vocab) for r in g.rows) and n > 100


@pytest.mark.parametrize("vocab", ["small", "real"])
def test_mass_cases_take_the_branch_they_are_named_for(vocab):
    voc = sc.VOCABS[vocab]
    fired_with_text = 0
    for g in sc.groups("ts", vocab):
        for r in g.rows:
            if not r.kind.startswith("mass_"):
                continue
            pre = sc.processed_row(g, r, torch.float32, apply_mass=False)
            post = sc.processed_row(g, r, torch.float32)
            text_alive = bool(torch.isfinite(pre[:voc.ts_begin]).any())
            fired = text_alive and not bool(torch.isfinite(post[:voc.ts_begin]).any())
            pick = sc.lowest_argmax(post)
            if r.kind == "mass_a":
                assert fired or not text_alive, (g.name, r.name)
                ts = pre[voc.ts_begin:]
                assert pick == voc.ts_begin + int(torch.nonzero(ts == ts.max())[0])      # lowest id on ties
                fired_with_text += fired
            elif text_alive or r.kind == "mass_d":          # (b) and (d): text wins wherever text is eligible at all
                assert text_alive and not fired and pick < voc.ts_begin, (g.name, r.name)
            if r.kind == "mass_d":                          # exactly one eligible timestamp, equal to the best text
                ts = pre[voc.ts_begin:]
                assert int(torch.isfinite(ts).sum()) == 1 and float(ts.max()) == float(pre[:voc.ts_begin].max())
    assert fired_with_text >= 10


def test_small_vocabulary_timestamps_straddle_slices():
    """(c): the ~30 planted timestamps of a mass case fall into at least four slices at G = 16 and 32.  At G = 4 a
    slice is 256 ids and the timestamps (631 .. 1002) touch only the last two of the four: both must be hit."""
    voc = sc.SMALL
    assert [sc.slices(B, voc.V)[0] for B in sc.BATCHES] == list(sc.SLICES)
    assert [sc.slices(B, sc.REAL.V)[0] for B in sc.BATCHES] == list(sc.SLICES)
    assert sc.slices(1, voc.V) == (32, 32) and voc.V % 8 != 0
    n = 0
    for g in sc.groups("ts", "small"):
        for r in g.rows:
            if r.kind != "mass_a" or sc.row_last_ts(voc, r) not in (-1, voc.ts_begin) or (g.first and g.max_initial >= 0):
                continue
            if r.gen and r.gen[-1] >= voc.ts_begin and (len(r.gen) < 2 or r.gen[-2] >= voc.ts_begin):
                continue                                    # closed pair: no timestamp eligible
            level = float(r.x[voc.ts_begin:].max())
            planted = (torch.nonzero(r.x[voc.ts_begin:] == level).flatten() + voc.ts_begin).tolist()
            assert len(planted) >= 25
            for B, need in ((1, 4), (17, 4), (100, 2)):
                w = sc.slices(B, voc.V)[1]
                assert len({t // w for t in planted}) >= need, (g.name, r.name, B)
            n += 1
    assert n >= 4


@pytest.mark.parametrize("drop", MUTANTS)
@pytest.mark.parametrize("vocab", ["small", "real"])
def test_rule_drop_mutant_changes_a_pick(vocab, drop):
    rules = mutant_rules(drop)
    hits = [(g.name, r.name) for g in sc.groups("ts", vocab) for r in g.rows
            if _pick(g, r, rules) != _pick(g, r, sc.timestamp_rules)]
    assert hits, drop


@pytest.mark.parametrize("vocab", ["small", "real"])
def test_looking_before_begin_col_changes_a_pick(vocab):
    """A selector that read ids[col-1] / ids[col-2] without the begin_col bound would take the conditioned prompt's
    timestamps for generated ones."""
    hits = 0
    for g in sc.groups("ts", vocab):
        for r in g.rows:
            if r.prompt and _pick(g, r, mutant_rules(None, r.prompt)) != _pick(g, r, sc.timestamp_rules):
                hits += 1
    assert hits > 0


def test_greedy_cases_plant_what_they_say():
    for vocab in ("small", "real"):
        voc = sc.VOCABS[vocab]
        off, on = sc.groups("greedy", vocab)
        ref = {r.name: sc.reference(off, r, torch.float32) for r in off.rows}
        ron = {r.name: sc.reference(on, r, torch.float32) for r in on.rows}
        assert ref["win_first"]["tok"] == 0 and ref["win_last"]["tok"] == voc.V - 1
        assert ref["tie_same_chunk"]["tok"] == 16 and ref["tie_slices"]["tok"] == 45
        assert ref["tie_three"]["tok"] == voc.V // 3
        assert ref["sup_winner"]["tok"] == 300 and ref["sup_first_word"]["tok"] != voc.sup[0]
        assert ref["beg_winner"]["tok"] == voc.beg[0] and ron["beg_winner"]["tok"] == 301
        assert ref["eos_winner"]["tok"] == voc.eos and ref["eos_winner"]["done"] == 1 and ron["eos_winner"]["tok"] == 302
        assert ref["done_row"]["tok"] == voc.eos and ref["done_row"]["logp"] is None
        assert ref["all_neg_inf"]["tok"] == 0 and ref["only_suppressed_finite"]["tok"] == 0
        assert not ref["all_neg_inf"]["any_finite"] and ref["one_finite"]["tok"] == voc.V - 2
        for B in sc.BATCHES:
            G, w = sc.slices(B, voc.V)
            for k in ({1, G // 2, G - 1} - {0}) if G > 1 else ():
                assert ref[f"win_slice_end_G{G}_k{k}"]["tok"] == k * w - 1
                assert ref[f"win_slice_start_G{G}_k{k}"]["tok"] == k * w
                assert ref[f"tie_across_slice_G{G}_k{k}"]["tok"] == k * w - 1
        if voc.V > 2048:
            assert ref["tie_across_pass"]["tok"] == 2047 and ref["tie_same_thread_two_passes"]["tok"] == 13
            later = 0
            for B in sc.BATCHES:
                G, w = sc.slices(B, voc.V)
                if G > 1 and w > 2048:                      # the pass boundary counted from slice 1's first id
                    assert w + 2048 < min(voc.V, 2 * w)
                    assert ref[f"win_pass_end_G{G}_k1"]["tok"] == w + 2047
                    assert ref[f"win_pass_start_G{G}_k1"]["tok"] == w + 2048
                    assert ref[f"tie_across_pass_G{G}_k1"]["tok"] == w + 2047
                    later += 1
            assert later == 3                               # G = 16, 4 and 2
