"""The long-form host logic (tw/generation.py generate -> _longform) as a table of cases over scripted stand-ins: with
the device decoders scripted the seek loop is pure Python, so its outputs can be compared exactly between two commits.
tests/golden/make_golden_longform_host.py records the table on one commit (longform_host.json);
tests/test_longform_host_cpu.py runs it on the working tree and compares.

Recording r of a case carries the window id 10 * r + k in its k-th 3000-frame stretch; the stand-in model's encoder
returns that id (one row a window), and the scripted decoders decode SCRIPT[(window id, temperature)]."""
import math
import types

import torch

from tw.config import GenerationConfig

EOS = 50257
TS0 = 50364            # <|0.00|>
PREV = 50361           # <|startofprev|>: the second-last suppress token
LOG = dict(runs=[], encodes=[])


def _tokens(base, n, end):
    """<|0.00|>, n text tokens from `base`, a closing timestamp, eos: accepted as one segment ending on a single
    timestamp (the seek advances by the whole window)."""
    return [TS0] + list(range(base, base + n)) + [TS0 + end, EOS]


def _loop(a):
    return [TS0] + [a, a + 1] * 20 + [EOS]       # compression ratio >> 1.35


class _Sel:
    def __init__(self, nb):
        self.sum_logp = torch.zeros(nb)


class ScriptedDecoder:
    """generation._Decoder: row r of a run decodes script[(window, temperature)]; the batch is cut where its longest
    row emits eos, the rows that finished earlier padded with eos.  logp[(window, temperature)] overrides the
    summed log-prob (-0.1 a token); ns[window] is the no-speech probability (default 0.1)."""
    script, logp, ns, kind = {}, {}, {}, "row"

    def __init__(self, model, gc, nb, Tk, P, ml, timestamps, use_graph, track=False, **kw):
        self.nb = nb
        self.sel = _Sel(nb)
        self.ns_logp = torch.zeros(nb)

    def run(self, enc16, prompt, **kw):
        LOG["runs"].append(dict(decoder=self.kind, keywords=sorted(kw)))
        assert prompt.shape[0] == self.nb
        ids = enc16.flatten()
        wins = [int(ids[r].item()) if ids.numel() == self.nb else int(ids[0].item()) for r in range(self.nb)]
        t = kw.get("temperature", 0.0)
        temps = list(t) if isinstance(t, (list, tuple)) else [t]
        assert len(temps) == self.nb
        keys = [(w, round(t, 1)) for w, t in zip(wins, temps)]
        rows = [list(self.script[k]) for k in keys]
        L = max(len(r) for r in rows)
        for i, (k, r) in enumerate(zip(keys, rows)):
            self.sel.sum_logp[i] = self.logp.get(k, -0.1 * len(r))
            self.ns_logp[i] = math.log(self.ns.get(k[0], 0.1))
        return torch.tensor([r + [EOS] * (L - len(r)) for r in rows], dtype=torch.int64)


class ScriptedSpecDecoder(ScriptedDecoder):
    """generation._SpecDecoder: one row; `accepted` as the device decoder exposes it after a run."""
    kind = "spec"

    def __init__(self, model, assistant, gc, Tk, P, ml, timestamps, use_graph, track=False, k=None, **kw):
        super().__init__(model, gc, 1, Tk, P, ml, timestamps, use_graph, track)
        self.k, self.accepted = k, []

    def run(self, enc16, prompt, **kw):
        out = super().run(enc16, prompt, **kw)
        assert tuple(kw["enc_a"].shape) == tuple(enc16.shape)
        self.accepted = [self.k, 1, 0][:max(1, out.shape[1] // 4)]
        return out


class ScriptedBeamDecoder:
    """generation._BeamDecoder for one window: decodes script[(window, "beam")]; sum_logp / ns_prob as its run
    leaves them."""
    script, logp, ns = {}, {}, {}

    def __init__(self, model, gc, B, nb, Tk, P, max_length, timestamps=None):
        assert B == 1 and nb > 1 and timestamps is not None
        self.sum_logp = self.ns_prob = None

    def run(self, enc16, prompt, **kw):
        LOG["runs"].append(dict(decoder="beam", keywords=sorted(kw)))
        key = (int(enc16.flatten()[0].item()), "beam")
        row = list(self.script[key])
        self.sum_logp = torch.tensor([self.logp.get(key, -0.1 * len(row))])
        self.ns_prob = torch.tensor([self.ns.get(key[0], 0.1)])
        return torch.tensor([row], dtype=torch.int64)


def model(compute="bf16"):
    cfg = types.SimpleNamespace(max_source_positions=1500, max_target_positions=448, vocab_size=51865, d_model=128)
    m = types.SimpleNamespace(config=cfg, device=torch.device("cpu"), compute=compute, act_dtype=torch.float32,
                              generation_config=_gc())
    m.conv_input = lambda feats: feats

    def encode(x):
        LOG["encodes"].append(list(x.shape))
        return x[:, :1, :1].reshape(-1, 1).clone()
    m.encode = encode
    return m


def features(frames):
    """One recording per entry of `frames` (its length in feature frames) -> (features, attention mask)."""
    T = max(frames)
    T = (T + 2999) // 3000 * 3000
    feats = torch.zeros(len(frames), 80, T)
    mask = torch.zeros(len(frames), T, dtype=torch.long)
    for r, n in enumerate(frames):
        for k in range(T // 3000):
            feats[r, :, 3000 * k:3000 * (k + 1)] = 10 * r + k
        mask[r, :n] = 1
    return feats, mask


def _gc():
    return GenerationConfig(decoder_start_token_id=50258, eos_token_id=EOS, pad_token_id=EOS,
                            no_timestamps_token_id=50363, suppress_tokens=[1, PREV, 50362],
                            lang_to_id={"<|zh|>": 50260})


def _greedy_script(wins):
    return {(w, 0.0): _tokens(100 + 10 * w, 3 + w % 4, 100 + w) for w in wins}


def _cases():
    c = {}
    # sequential on the parent (one recording conditioned, or beam search): `batch` follows _bucket there
    c["cond1_t0"] = dict(frames=[9000], kw=dict(condition_on_prev_tokens=True, temperature=0.0), sequential=True,
                         script=_greedy_script([0, 1, 2]))
    s = {(w, t): _loop(200 + 10 * w + int(10 * t)) for w in (0, 1) for t in (0.0, 0.4, 1.0)}
    c["cond1_all_fail"] = dict(frames=[6000], sequential=True, script=s,
                               kw=dict(condition_on_prev_tokens=True, temperature=(0.0, 0.4, 1.0),
                                       compression_ratio_threshold=0.0))
    # window 0 accepted at T = 0 (window 1 conditioned on it), window 1 fails at every temperature and keeps its
    # T = 1.0 attempt (window 2 unconditioned), window 2 accepted at T = 0.4
    s = _greedy_script([0])
    s.update({(1, t): _loop(300 + int(10 * t)) for t in (0.0, 0.4, 1.0)})
    s.update({(2, 0.0): _loop(400), (2, 0.4): _tokens(410, 4, 60), (2, 1.0): _tokens(420, 9, 70)})
    c["cond1_switches_off"] = dict(frames=[8500], sequential=True, script=s,
                                   kw=dict(condition_on_prev_tokens=True, temperature=(0.0, 0.4, 1.0),
                                           compression_ratio_threshold=1.35))
    s = _greedy_script([0, 2])
    s.update({(1, 0.0): _loop(500), (1, 0.2): _tokens(510, 2, 40), (1, 0.4): _tokens(520, 8, 50),
              (1, 0.6): _tokens(530, 5, 55)})
    c["cond1_assisted"] = dict(frames=[9000], sequential=True, script=s, assist=3,
                               kw=dict(condition_on_prev_tokens=True, temperature=(0.0, 0.2, 0.4),
                                       compression_ratio_threshold=1.35, logprob_threshold=-1.0))
    c["cond1_repeat"] = dict(frames=[6000], sequential=True, script=dict(s),
                             kw=dict(condition_on_prev_tokens=True, temperature=(0.0, 0.2, 0.4, 0.6),
                                     compression_ratio_threshold=1.35, repetition_penalty=1.3,
                                     no_repeat_ngram_size=2))
    # beam search, two recordings (windows 0, 1 and 10): the beam attempt of window 1 fails its log-prob gate
    s = {(0, "beam"): _tokens(600, 4, 120), (1, "beam"): _tokens(610, 5, 80), (1, 0.4): _tokens(620, 3, 90),
         (10, "beam"): _tokens(630, 6, 30)}
    c["beam2_two_recordings"] = dict(frames=[6000, 2500], sequential=True, script=s, logp={(1, "beam"): -20.0},
                                     kw=dict(num_beams=2, temperature=(0.0, 0.4), logprob_threshold=-1.0,
                                             no_speech_threshold=0.6))
    s = {(0, "beam"): _loop(700), (0, 0.4): _loop(710), (1, "beam"): _tokens(720, 3, 20), (2, "beam"): _loop(730),
         (2, 0.4): _tokens(740, 5, 25)}
    c["beam2_zero_later"] = dict(frames=[9000], sequential=True, script=s,
                                 kw=dict(num_beams=2, temperature=(0.0, 0.4, 0.0), compression_ratio_threshold=1.35,
                                         condition_on_prev_tokens=True))
    # the batched loop on the parent: three recordings conditioned; window 11 is skipped as silence
    s = _greedy_script([0, 1, 10, 20, 21, 22])
    s.update({(1, 0.0): _loop(800), (1, 0.2): _loop(810), (1, 0.4): _tokens(820, 4, 33), (1, 0.6): _tokens(830, 2, 34),
              (11, 0.0): _tokens(840, 3, 35), (20, 0.0): _loop(850), (20, 0.2): _tokens(860, 12, 36),
              (20, 0.4): _tokens(870, 3, 37), (20, 0.6): _tokens(880, 3, 38)})
    c["cond3_batched"] = dict(frames=[6000, 4000, 9000], sequential=False, script=s, logp={(11, 0.0): -30.0},
                              ns={11: 0.9},
                              kw=dict(condition_on_prev_tokens=True, temperature=(0.0, 0.2, 0.4, 0.6),
                                      compression_ratio_threshold=1.35, logprob_threshold=-1.0,
                                      no_speech_threshold=0.6))
    s = _greedy_script([0])
    s.update({(1, 0.0): _loop(900), (1, 0.2): _loop(910), (1, 0.4): _tokens(920, 4, 44), (1, 0.6): _tokens(930, 2, 45)})
    c["cond1_fp32"] = dict(frames=[6000], sequential=True, script=s, compute="fp32",
                           kw=dict(condition_on_prev_tokens=True, temperature=(0.0, 0.2, 0.4, 0.6),
                                   compression_ratio_threshold=1.35))
    return c


CASES = _cases()


def run_case(generation, case):
    """One case on the module `generation` -> dict(ids, trace (without gate_ms), runs, encodes)."""
    names = dict(_Decoder=ScriptedDecoder, _SpecDecoder=ScriptedSpecDecoder, _BeamDecoder=ScriptedBeamDecoder)
    saved = {n: getattr(generation, n) for n in names}
    for cls in (ScriptedDecoder, ScriptedBeamDecoder):
        cls.script, cls.logp, cls.ns = case["script"], case.get("logp", {}), case.get("ns", {})
    LOG["runs"], LOG["encodes"] = [], []
    m = model(case.get("compute", "bf16"))
    assist = None
    if case.get("assist"):          # an assistant with an encoder of its own (its calls are recorded with the target's)
        assist = types.SimpleNamespace(decoder_only=False, conv_input=m.conv_input, encode=m.encode, config=m.config,
                                       generation_config=None)
    feats, mask = features(case["frames"])
    trace = []
    try:
        for n, cls in names.items():
            setattr(generation, n, cls)
        out = generation.generate(m, feats, attention_mask=mask, language="zh", task="transcribe", max_new_tokens=40,
                                  use_graph=False, return_timestamps=True, _trace=trace, assistant_model=assist,
                                  num_assistant_tokens=case.get("assist"), **case["kw"])
    finally:
        for n, cls in saved.items():
            setattr(generation, n, cls)
    trace = [{k: v for k, v in t.items() if k != "gate_ms"} for t in trace]
    return dict(ids=out.tolist(), trace=trace, runs=list(LOG["runs"]), encodes=list(LOG["encodes"]))
