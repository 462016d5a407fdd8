"""The decode step's per-row entries for left-padded prompts (include/tw_hip.h):

* tw_decode_attn_ks: row b attends keys [k_start[b], Tk) -- vs an fp64 reference over that range at test_decode_gpu's
  bar (2**-7 * max|ref| + 1e-3 for the 16-bit types; the fp32 attention bar of test_fp32_gpu, 2e-5 relative, for fp32),
  on the one-workgroup-per-pair kernels (fixed and device Tk) and the split + combine path (a start inside the first
  chunk of DA_SPLIT keys, and one past it so a whole chunk is masked), row-interleaved and head-major; the masked
  K / V rows hold NaN, so any read of them shows; a start at or past Tk is clamped to the last key; on the
  one-workgroup path each row equals, bit for bit, the plain entry run on that row alone from its start;
* tw_embed_step_off: tok[ids] + pos[max(t - off, 0)], exact;
* a captured step replayed after the arrays' contents changed equals the eager step with the new contents.
"""
import os
import re

import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda"
# keys per workgroup of the split path, read from the kernel's header so the cases stay on its chunk boundary
with open(os.path.join(PKG, "csrc", "decode_impl.h")) as _f:
    DA_SPLIT = int(re.search(r"constexpr int DA_SPLIT = (\d+);", _f.read()).group(1))
assert 32 <= DA_SPLIT < 220           # the (2, 20, 230) cases below need two chunks and starts inside each


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bar(dt, ref):
    return 2e-5 * ref.abs().max() if dt == torch.float32 else 2 ** -7 * ref.abs().max() + 1e-3


def _ref(q, k, v, starts, Tk):
    """q [B, H, 64], k / v [B, H, T, 64] (any dtype) -> fp64 attention of row b over keys [starts[b], Tk)."""
    out = []
    for b, s0 in enumerate(starts):
        s0 = max(min(s0, Tk - 1), 0)
        kk, vv = k[b, :, s0:Tk].double(), v[b, :, s0:Tk].double()
        s = torch.einsum("he,hke->hk", q[b].double(), kk) * 0.125
        out.append(torch.einsum("hk,hke->he", torch.softmax(s, -1), vv).reshape(-1))
    return torch.stack(out)


CASES = [  # B, H, Tk, starts, device Tk, dtype
    (3, 2, 5, [0, 1, 4], False, torch.bfloat16),                      # one workgroup; a single-key range
    (3, 2, 5, [0, 1, 4], False, torch.float32),
    (3, 2, 5, [7, 5, -2], False, torch.float16),                      # starts at / past Tk and below 0: clamped
    (2, 20, 230, [DA_SPLIT + 9, 17], False, torch.bfloat16),          # split: chunk 0 wholly masked / a start inside it
    (2, 20, 230, [DA_SPLIT, 229], False, torch.float32),              # split: a start on the boundary, the last key
    (40, 20, 200, [(7 * b) % 199 for b in range(40)], True, torch.float16),    # one workgroup under device Tk
    (40, 20, 200, [(11 * b) % 200 for b in range(40)], True, torch.bfloat16),
]


@pytest.mark.parametrize("B,H,Tk,starts,dev,dt", CASES)
def test_decode_attn_k_start(B, H, Tk, starts, dev, dt):
    from tw import ops
    g = torch.Generator().manual_seed(B * 131 + Tk)
    d = H * 64
    Tmax = Tk + 3
    cache = torch.randn(B, Tmax, 3 * d, generator=g).to(dt)           # [q | k | v] rows like the self cache
    t = Tk - 1
    for b, s0 in enumerate(starts):                                    # the masked rows' K and V: NaN
        cache[b, :max(min(s0, Tk - 1), 0), d:] = float("nan")
    cd = cache.to(DEV)
    flat = cd.view(-1)
    sb = Tmax * 3 * d
    ks = torch.tensor(starts, dtype=torch.int32, device=DEV)
    o = torch.empty(B, d, dtype=dt, device=DEV)
    qv = flat[t * 3 * d:]
    if dev:
        t_dev = torch.tensor([Tk - 1], dtype=torch.int32, device=DEV)
        ops.decode_attn(qv, sb, flat[d:], 3 * d, sb, flat[2 * d:], 3 * d, sb, o, d, B, H, 1, 0.125, tk_dev=t_dev,
                        tk_max=Tmax, k_start=ks)
    else:
        ops.decode_attn(qv, sb, flat[d:], 3 * d, sb, flat[2 * d:], 3 * d, sb, o, d, B, H, Tk, 0.125, k_start=ks)
    assert bool(torch.isfinite(o).all())
    q = cache[:, t, :d].view(B, H, 64)
    k = cache[:, :, d:2 * d].view(B, Tmax, H, 64).transpose(1, 2)
    v = cache[:, :, 2 * d:].view(B, Tmax, H, 64).transpose(1, 2)
    ref = _ref(q, k, v, starts, Tk)
    err = (o.double().cpu() - ref).abs().max()
    print(f"B {B} H {H} Tk {Tk} {dt}: max err {float(err):.3e} (bar {float(_bar(dt, ref)):.3e})")
    assert err <= _bar(dt, ref)
    split = not dev and B * H < 640 and Tk > DA_SPLIT
    if not split:
        # the body walks from its first key: row b == the plain entry on that row alone, K / V advanced to its start
        for b in range(0, B, max(1, B // 5)):
            s0 = max(min(starts[b], Tk - 1), 0)
            row = flat[b * sb:]
            o1 = torch.empty(1, d, dtype=dt, device=DEV)
            if dev:               # device Tk: the plain entry never splits, whatever the key count
                n_dev = torch.tensor([Tk - s0 - 1], dtype=torch.int32, device=DEV)
                ops.decode_attn(row[t * 3 * d:], sb, row[s0 * 3 * d + d:], 3 * d, sb, row[s0 * 3 * d + 2 * d:], 3 * d,
                                sb, o1, d, 1, H, 1, 0.125, tk_dev=n_dev, tk_max=Tmax - s0)
            else:
                assert Tk - s0 <= DA_SPLIT
                ops.decode_attn(row[t * 3 * d:], sb, row[s0 * 3 * d + d:], 3 * d, sb, row[s0 * 3 * d + 2 * d:], 3 * d,
                                sb, o1, d, 1, H, Tk - s0, 0.125)
            assert torch.equal(o1[0], o[b]), b


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_decode_attn_k_start_head_major(dt):
    """The head-stride form ([H][Tk][64] blocks per clip, the cross-attention layout), split path, 12 chunks."""
    from tw import ops
    B, H, Tk = 5, 20, 1500
    starts = [0, 3, DA_SPLIT * 4 + 1, 1499, 700]
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, H * 64, generator=g).to(dt)
    k = torch.randn(B, H, Tk, 64, generator=g).to(dt)
    v = torch.randn(B, H, Tk, 64, generator=g).to(dt)
    for b, s0 in enumerate(starts):
        k[b, :, :s0] = float("nan")
        v[b, :, :s0] = float("nan")
    qd, kd, vd = q.to(DEV), k.to(DEV).reshape(-1), v.to(DEV).reshape(-1)
    o = torch.empty(B, H * 64, dtype=dt, device=DEV)
    ks = torch.tensor(starts, dtype=torch.int32, device=DEV)
    ops.decode_attn(qd, H * 64, kd, 64, H * Tk * 64, vd, 64, H * Tk * 64, o, H * 64, B, H, Tk, 0.125, hsk=Tk * 64,
                    hsv=Tk * 64, k_start=ks)
    assert bool(torch.isfinite(o).all())
    ref = _ref(q.view(B, H, 64), k, v, starts, Tk)
    err = (o.double().cpu() - ref).abs().max()
    print(f"head-major {dt}: max err {float(err):.3e} (bar {float(_bar(dt, ref)):.3e})")
    assert err <= _bar(dt, ref)


def test_decode_attn_k_start_zero_is_the_plain_entry():
    """Every start 0: the same result as tw_decode_attn, bit for bit, on both paths."""
    from tw import ops
    for B, H, Tk in ((2, 20, 230), (3, 2, 77)):
        d = H * 64
        g = torch.Generator().manual_seed(Tk)
        q = torch.randn(B, d, generator=g).bfloat16().to(DEV)
        kv = torch.randn(B, Tk, 2 * d, generator=g).bfloat16().to(DEV)
        o0, o1 = torch.empty_like(q), torch.empty_like(q)
        ops.decode_attn(q, d, kv, 2 * d, Tk * 2 * d, kv.view(-1)[d:], 2 * d, Tk * 2 * d, o0, d, B, H, Tk, 0.125)
        ops.decode_attn(q, d, kv, 2 * d, Tk * 2 * d, kv.view(-1)[d:], 2 * d, Tk * 2 * d, o1, d, B, H, Tk, 0.125,
                        k_start=torch.zeros(B, dtype=torch.int32, device=DEV))
        assert torch.equal(o0, o1)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_embed_step_off(dt):
    from tw import ops
    B, D, V, T = 5, 384, 100, 32
    g = torch.Generator().manual_seed(3)
    tok = torch.randn(V, D, generator=g).to(dt).to(DEV)
    pos = torch.randn(T, D, generator=g).to(dt).to(DEV)
    ids = torch.tensor([3, 99, 0, 17, 42], device=DEV)
    off = [0, 4, 7, 9, 30]                                   # t = 7: t > off, t == off and t < off rows
    offd = torch.tensor(off, dtype=torch.int32, device=DEV)
    for t in (0, 7, 31):
        t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
        out = torch.empty(B, D, dtype=dt, device=DEV)
        ops.embed_step(ids, tok, pos, out, t_dev, T, pos_off=offd)
        p = torch.tensor([max(t - o_, 0) for o_ in off], device=DEV)
        want = tok[ids] + pos[p]                              # the sum in the operands' own dtype
        assert torch.equal(out, want), t
    # no offsets: the plain entry
    out0, out1 = torch.empty(B, D, dtype=dt, device=DEV), torch.empty(B, D, dtype=dt, device=DEV)
    ops.embed_step(ids, tok, pos, out0, t_dev, T)
    ops.embed_step(ids, tok, pos, out1, t_dev, T, pos_off=torch.zeros(B, dtype=torch.int32, device=DEV))
    assert torch.equal(out0, out1)


def small_model(name, compute):
    """micro (d = 128: the skinny-GEMM decode step with tw_kv_append) or a d = 256 model (d % 256 == 0: the GEMV step,
    whose QKV GEMV appends K / V to the cache itself)."""
    from oracle.weights import CONFIGS, _base, make_weights
    from tw.config import WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration
    cfg = CONFIGS["micro"] if name == "micro" else _base(256, 1, 2, 4, 512)
    w = make_weights(cfg, 1, lin_std=0.2)
    m = WhisperForConditionalGeneration.from_state_dict(WhisperConfig(**cfg), {k: torch.from_numpy(v) for k, v in
                                                                               w.items()}, dtype=torch.float32)
    m.set_compute(compute)
    return cfg, m


@pytest.mark.parametrize("name", ["micro", "d256"])
def test_captured_step_follows_k_start_and_pos_off(name):
    """One decode step captured with one set of pad counts, replayed after the device arrays changed: the same logits
    as an eager step with the new contents (and not those of the old contents)."""
    from tw.generation import DecodeSession
    cfg, m = small_model(name, "bf16")
    B, Tk, T_max, t0 = 3, cfg["max_source_positions"], 16, 9
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(B * Tk, cfg["d_model"], generator=g).to(m.act_dtype).to(DEV)
    sess = DecodeSession(m, enc, B, Tk, T_max)
    for c in sess.self_kv:                                    # a filled cache (rows 0 .. t0 - 1 of every layer)
        c.copy_(torch.randn(c.shape, generator=g).to(c.dtype))
    saved = [c.clone() for c in sess.self_kv]
    ids = torch.tensor([5, 900, 77], device=DEV)

    def prepare(pads):
        sess.set_pads(pads, shift_positions=True)
        for c, s_ in zip(sess.self_kv, saved):
            c.copy_(s_)
        sess.t_dev.fill_(t0)
        sess.cur.copy_(ids)

    prepare([1, 0, 4])
    sess.step()                                               # warm up outside capture (workspace allocation)
    prepare([1, 0, 4])
    sess.capture(None)
    graph = sess.graph
    prepare([1, 0, 4])
    graph.replay()
    old = sess.logits.clone()
    prepare([6, 2, 0])
    assert sess.graph is graph                                # the contents changed, not the mode: no recapture
    graph.replay()
    got = sess.logits.clone()
    assert int(sess.t_dev) == t0 + 1
    prepare([6, 2, 0])
    sess.step()
    torch.cuda.synchronize()
    assert torch.equal(got, sess.logits)
    assert not torch.equal(got, old)
