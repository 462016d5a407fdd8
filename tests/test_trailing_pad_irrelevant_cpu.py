"""The premise of the trainer's packed decoder rows, on the CPU oracle (tiny config, B = 2, T = 447): the rows after
a clip's last label take no part in the step.  Replacing the decoder inputs at those positions (>= n_b = 1 + the last
index with a label) with random tokens leaves distill_ref.train_step's three losses and every trainable gradient
exactly unchanged: the loss masks them, the decoder is causal and the reference passes no decoder attention mask, so
no kept row reads them.  A LEADING masked position (inside a <|startofprev|> prompt) is different -- later rows attend
to it -- and changing one does move the result: those rows must never be dropped."""
import numpy as np
import torch

from oracle import distill_ref, labels as L
from oracle.weights import CONFIGS, SPECIAL, make_weights
from oracle.whisper_ref import Ref, to_torch


def _step(cfg, ws, wt, feats, dec, lab):
    ps = to_torch(ws)
    names = [n for n in ps if n.startswith("model.decoder.")]
    for n in names:
        ps[n].requires_grad_(True)
    o = distill_ref.train_step(Ref(cfg, ps, amp=True), Ref(cfg, to_torch(wt, torch.bfloat16), amp=True,
                                                           stream_bf16=True),
                               feats, torch.from_numpy(dec), torch.from_numpy(lab))
    return {k: float(o[k]) for k in ("loss", "ce_loss", "kl_loss")}, {n: ps[n].grad.clone() for n in names}


def test_trailing_pad_rows_do_not_reach_losses_or_gradients():
    cfg = CONFIGS["tiny"]
    ws, wt = make_weights(cfg, 1), make_weights(cfg, 2)
    rng = np.random.Generator(np.random.PCG64(9))
    lists = L.synthetic_label_lists(2, seed=7, prompt_fraction=0.0, min_len=40, max_len=120)
    lists[1] = [SPECIAL["startofprev"]] + rng.integers(0, SPECIAL["eot"], size=20).tolist() + lists[1]
    dec, lab = L.collate(lists)
    B, T = lab.shape
    assert T == 447
    n = [int(np.nonzero(lab[b] >= 0)[0][-1]) + 1 for b in range(B)]
    lead = int(np.nonzero(lab[1] >= 0)[0][0])
    assert all(0 < nb < T for nb in n) and lead > 5, "the batch needs trailing padding and a masked prompt"
    feats = torch.from_numpy(rng.standard_normal((B, cfg["num_mel_bins"], 3000)).astype(np.float32) * 0.5)
    base_loss, base_grad = _step(cfg, ws, wt, feats, dec, lab)
    gmax = max(float(g.abs().max()) for g in base_grad.values())
    assert gmax > 0

    # trailing pad positions: random tokens in place of <pad>
    dec_t = dec.copy()
    for b in range(B):
        dec_t[b, n[b]:] = rng.integers(0, SPECIAL["eot"], size=T - n[b])
    assert (dec_t != dec).any()
    loss, grad = _step(cfg, ws, wt, feats, dec_t, lab)
    assert loss == base_loss
    for k in base_grad:
        assert torch.equal(grad[k], base_grad[k]), k

    # a leading masked position (inside the prompt): later rows attend to it
    dec_l = dec.copy()
    dec_l[1, 3] = (dec[1, 3] + 1) % SPECIAL["eot"]
    assert lab[1, 3] < 0 and 3 < lead
    loss, grad = _step(cfg, ws, wt, feats, dec_l, lab)
    assert loss != base_loss
    assert any(not torch.equal(grad[k], base_grad[k]) for k in base_grad)
