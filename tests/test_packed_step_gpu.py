"""One distillation step with packed decoder rows (TW_PACK_ROWS=1, the default) against the same step on padded rows
(TW_PACK_ROWS=0), from identical initial state, at the c1 dims (tests/golden/cfg_c1.npz: tiny <- tiny).

The two paths compute the same rows with the same kernels; they differ only by fp32 regrouping (split-K chunking of the
weight-gradient products at another M, the loss reduction over another row count).  Every packed-vs-padded distance
must stay below the fixture's own 16-bit noise for that quantity, dist(autocast ref, fp32 ref) as _within_noise of
tests/test_configs_gpu.py computes it: packing then moves the result by less than two correct evaluations of the
reference differ.  Measured on MI355X (printed by the tests): see DESIGN.md §4, "Packed decoder rows".

Two batches: the fixture's own (the packed run must also pass the fixture checks the padded run passes), and one whose
labels hold a full-length row (n_b = T, nothing dropped), a short row and a row with a <|startofprev|> prompt (leading
masked rows, which stay).
"""
import numpy as np
import pytest
import torch

from test_configs_gpu import _build, _maxrel, _rl2, _within_noise

pytestmark = pytest.mark.gpu

P0 = "model.decoder.layers.0.fc1.weight"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _three_row_batch(batch):
    """c1 features (the first clip twice) with a full-length, a short and a prompted label row."""
    from oracle import labels as L
    from oracle.weights import SPECIAL
    rng = np.random.Generator(np.random.PCG64(21))
    head = [SPECIAL["sot"], SPECIAL["zh"], SPECIAL["transcribe"], SPECIAL["notimestamps"]]
    body = lambda n: rng.integers(0, SPECIAL["eot"], size=n).tolist()
    full = head + body(448 - 5) + [SPECIAL["eot"]]
    short = head + body(30) + [SPECIAL["eot"]]
    prompted = [SPECIAL["startofprev"]] + body(24) + head + body(90) + [SPECIAL["eot"]]
    dec, lab = L.collate([full, short, prompted])
    n = [int(np.nonzero(r >= 0)[0][-1]) + 1 for r in lab]
    assert n[0] == lab.shape[1] and n[1] < 64 and int(np.nonzero(lab[2] >= 0)[0][0]) > 20
    f = batch["input_features"]
    dev = f.device
    return dict(input_features=torch.cat([f, f[:1]]), decoder_input_ids=torch.from_numpy(dec).to(dev),
                labels=torch.from_numpy(lab).to(dev))


def _run(monkeypatch, pack, three_rows):
    """-> (fixture, names, losses, flat gradient before the update, model) of one train_step from the c1 state."""
    from tw.distill import DistillationTrainer
    monkeypatch.setenv("TW_PACK_ROWS", "1" if pack else "0")
    g, s, t, batch, c = _build("c1")
    if three_rows:
        batch = _three_row_batch(batch)
    tr = DistillationTrainer(s, t, learning_rate=1e-4, warmup_steps=0, freeze_encoder=c["freeze_encoder"],
                             freeze_embed_positions=c["freeze_embed_positions"])
    assert tr.pack_rows == pack
    cap = {}
    orig = tr.optimizer_step

    def hook():
        cap["grad"] = s.grad.clone()
        return orig()
    tr.optimizer_step = hook
    m = tr.train_step(batch)
    torch.cuda.synchronize()
    return g, s, {k: m[k].item() for k in ("loss", "ce_loss", "kl_loss")}, cap["grad"]


def _norms(s, names, grad):
    from tw.modeling import to_hf
    out = []
    for n in names:
        o = s.store.offset[n]
        out.append(to_hf(n, grad[o: o + s.store.numel(n)].view(s.store.segs[n]), s.config).double().norm().item())
    return np.array(out)


def _fc1_block(s, grad):
    o = s.store.offset[P0]
    return grad[o: o + s.store.numel(P0)].view(s.store.segs[P0])[::37, ::29].double().cpu()


@pytest.mark.parametrize("three_rows", [False, True], ids=["fixture_batch", "full_short_prompt_rows"])
def test_packed_step_within_16bit_noise_of_padded_step(monkeypatch, three_rows):
    g, s, loss_p, grad_p = _run(monkeypatch, True, three_rows)
    _, s0, loss_0, grad_0 = _run(monkeypatch, False, three_rows)
    names = [str(n) for n in g["grad_names"]]
    # the fixture's 16-bit noise per quantity: the bars
    bars = {k: abs(float(g[f"amp|{fk}"]) - float(g[f"f32|{fk}"])) / abs(float(g[f"f32|{fk}"]))
            for k, fk in (("loss", "loss"), ("ce_loss", "ce"), ("kl_loss", "kl"))}
    bars["grad_norms"] = _maxrel(g["amp|grad_norms"], g["f32|grad_norms"])
    bars["fc1_block"] = _rl2(g["amp|grad_dec0_fc1_sub"], g["f32|grad_dec0_fc1_sub"])
    dist = {k: abs(loss_p[k] - loss_0[k]) / abs(loss_0[k]) for k in ("loss", "ce_loss", "kl_loss")}
    dist["grad_norms"] = _maxrel(_norms(s, names, grad_p), _norms(s0, names, grad_0))
    dist["fc1_block"] = _rl2(_fc1_block(s, grad_p), _fc1_block(s0, grad_0))
    for k in dist:
        print(f"  packed vs padded, {k}: {dist[k]:.3e}  (bar: reference 16-bit noise {bars[k]:.3e})")
    for k in dist:
        assert dist[k] < bars[k], (k, dist[k], bars[k])
    if three_rows:
        return
    # the packed run against the fixture, as tests/test_configs_gpu.py holds the padded run
    for k, fk in (("loss", "loss"), ("ce_loss", "ce"), ("kl_loss", "kl")):
        for mode in ("amp", "f32"):
            ref = float(g[f"{mode}|{fk}"])
            assert abs(loss_p[k] - ref) / abs(ref) < 1e-3, (k, mode)
    _within_noise("c1 packed per-tensor grad norms", _norms(s, names, grad_p), g, "grad_norms", _maxrel, floor=1e-2)
    tot = grad_p.double().norm().item()
    _within_noise("c1 packed total grad norm", np.array([tot]), {k: np.array([g[k]]) for k in
                  ("amp|grad_total_norm", "f32|grad_total_norm")}, "grad_total_norm", _maxrel, floor=2e-3)
    _within_noise("c1 packed dec0.fc1 grad block", _fc1_block(s, grad_p), g, "grad_dec0_fc1_sub", _rl2)
