"""Greedy generation with a KV cache.

Reference calls: `generate_step` (training/run_distillation.py:1580-1584), pseudo-labelling
`generate(num_beams=1, language, task)` (training/run_pseudo_labelling.py:917-922); semantics of
HF WhisperForConditionalGeneration.generate greedy path (HF generation_whisper.py): prompt
[<|startoftranscript|>, <|lang|>, <|task|>, <|notimestamps|>], SuppressTokens every step,
SuppressTokensAtBegin at the first generated step (HF logits_process.py), argmax, finished rows
padded with pad (= eos), stop when every row emitted eos or max_length is reached; the return
value is the generated ids only (transformers >= 5 behaviour, the version in this image).

Device layout (one DecodeSession per batch of clips):
  * self-attention cache per decoder layer: bf16 [B][T_max][2d] (k | v); the fused QKV projection
    of a step goes to a [B][3d] staging buffer and tw_kv_append copies k, v to row t; keys /
    values 0..t are read in place by tw_decode_attn (tw_decode_attn_ks from each row's first real
    column when the prompts are left-padded; tw_decode_attn_mq for the Q rows of a verify pass);
  * cross-attention K/V per decoder layer: bf16, head-major (K [B][H][1500][64] then V), projected
    once from the encoder output (k has no bias: the zero-bias segment of the fused KV bias) and
    transposed by tw_kv_head_major; with model.cross_kv_dtype == "fp8_e4m3" the same blocks as e4m3 bytes plus
    one fp32 power-of-two scale per (clip, head) block of K and of V (tw_kv_head_major_fp8), read by
    tw_decode_attn_fp8 / tw_decode_attn_mq_fp8;
  * logits bf16 [B][Vp]; tw_greedy_select applies the suppress masks, takes the argmax, writes
    the token into the id matrix and the next step's input vector, and tracks finished rows.
Everything runs on the HIP library.  The step index lives in device memory (t_dev: embedding
position, cache row, self-attention length, output column, begin-suppress test), so one step —
~14 launches per decoder layer + head + select + advance — is captured once into a HIP graph and
replayed per token; the host reads the finished flags every 8 steps to stop early.
"""
from __future__ import annotations

import dataclasses
import time
import types

import torch

from . import ops as F
# the request planner and the pure host helpers; imported by name so that they stay reachable as generation.<name>
from .generate_plan import (ASSISTED, AUTO, BEAM, DEFAULT_ASSISTANT_TOKENS, GENERATE_KEYWORDS,  # noqa: F401
                            MAX_ASSISTANT_TOKENS, OWN_PASS, PREFILL, Request, _ASSIST_GC_KEYS, _lang_id, _repeat_names,
                            build_prompt, check_assistant, gc_get, language_rows, language_table, plan_generate,
                            repeat_options, total_length)


class _StepBufs:
    """Activation buffers of M rows on their way through the decoder layers and the head."""

    def __init__(self, model, M):
        cfg, d, dev, act = model.config, model.config.d_model, model.device, model.act_dtype
        self.M = M
        self.x = torch.empty(M, d, dtype=model.stream_dtype, device=dev)
        self.y = torch.empty(M, d, dtype=act, device=dev)
        self.qkv = torch.empty(M, 3 * d, dtype=act, device=dev)
        self.o = torch.empty(M, d, dtype=act, device=dev)
        self.q = torch.empty(M, d, dtype=act, device=dev)
        self.h = torch.empty(M, cfg.decoder_ffn_dim, dtype=act, device=dev)
        self.logits = torch.empty(M, model.Vp, dtype=act, device=dev)


class DecodeSession:
    """Device state of one greedy decode over a batch; every step is position-independent (the step
    index lives in `t_dev`), so the whole step is captured once into a HIP graph and replayed."""

    def __init__(self, model, enc16: torch.Tensor, B: int, Tk: int, T_max: int, spare: int = 0):
        """spare: cache rows past T_max for the rounds of assisted decoding (step_multi writes Q rows at once, so a
        round that starts at the last position stays inside the caches); the positions then clamp to the table."""
        cfg = model.config
        T_max = T_max + spare
        self.m, self.B, self.Tk, self.T_max = model, B, Tk, T_max
        self.clamp_pos = spare > 0
        self.d = cfg.d_model
        self.H = self.d // 64
        dev = model.device
        d = self.d
        act = model.act_dtype            # bf16 (autocast) or fp32 (fp32 path): caches, operands, logits
        self.self_kv = [torch.empty(B, T_max, 2 * d, dtype=act, device=dev)
                        for _ in range(cfg.decoder_layers)]
        # cross-attention K/V head-major (K [B][H][Tk][64] then V): each (clip, head) of the per-step
        # cross-attention reads two contiguous runs instead of 128-B rows 2d apart (tw_kv_head_major; the
        # projection goes through one scratch [B*Tk][2d] block)
        # model.cross_kv_dtype == "fp8_e4m3": the same blocks as e4m3 bytes, half the size, with one fp32 power-of-two
        # scale per (clip, head) block of K and of V (tw_kv_head_major_fp8; the format: include/tw_hip.h).  The scale
        # tensors (2*B*H floats per layer, K's then V's) are allocated once, so a captured step survives set_encoder
        self.xkv_dtype = getattr(model, "cross_kv_dtype", None)
        self.xkv_fp8 = self.xkv_dtype == "fp8_e4m3"
        self.cross_kv = [torch.empty(2 * B * self.H * Tk * 64, dtype=torch.uint8 if self.xkv_fp8 else act, device=dev)
                         for _ in range(cfg.decoder_layers)]
        self.cross_scale = [torch.ones(2 * B * self.H, dtype=torch.float32, device=dev)
                            for _ in range(cfg.decoder_layers)] if self.xkv_fp8 else None
        self.graph = None
        self.xkv_shared = False
        self.set_encoder(enc16)
        self.t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.cur = torch.zeros(B, dtype=torch.int64, device=dev)       # this step's input ids
        self.buf = _StepBufs(model, B)   # the B rows of step
        self.mq = None                   # the Q rows of step_multi (alloc_multi)
        # batch <= 8 on the bf16 / fp16 paths: every Linear is one GEMV launch, with the LayerNorm in front of it
        # fused when the residual stream is 16-bit (bit-identical A); larger batches use the skinny GEMM with a
        # separate LayerNorm
        self.gemv = B <= 8 and model.compute in ("bf16", "fp16") and d % 256 == 0
        self.gemv_ln = self.gemv and model.stream_dtype == act
        # model.decode_weight_dtype == "fp8_e4m3": the step's Linears and the head read e4m3 bytes with one fp32 scale
        # per weight row (tw_gemv_w8_*; the model's buffers, allocated once, so a captured step survives a
        # requantisation); off the GEMV path the session reads a 16-bit copy of the dequantised weights, so a
        # recording's values do not depend on its batch's size
        self.w8 = getattr(model, "decode_weight_dtype", None) == "fp8_e4m3"
        # left-padded prompts (rows of one batch whose prompts differ in length: HF's decoder attention mask and
        # position ids): per row the first real cache row and the position offset, read on the device by
        # tw_decode_attn_ks / tw_embed_step_off.  Allocated once, refilled per window (set_pads), so a captured step
        # survives; without pad counts the step makes the plain calls
        self.k_start = torch.zeros(B, dtype=torch.int32, device=dev)
        self.pos_off = torch.zeros(B, dtype=torch.int32, device=dev)
        self.padded = False
        self.shifted = False

    @property
    def logits(self):
        """[B][Vp] logits of the last step."""
        return self.buf.logits

    def set_encoder(self, enc16):
        """(Re)project the cross-attention K/V of every decoder layer in place (graph-safe).  enc16 holds B*Tk
        rows, or Tk rows shared by every row of the batch (the speculative fallback batch of one window: each row
        sees exactly the K/V of a batch-1 decode)."""
        m, d = self.m, self.d
        shared = enc16.shape[0] == self.Tk and self.B > 1
        nb = 1 if shared else self.B
        # shared: ONE clip's K/V blocks ([H][Tk][64] K then V, at the front of each layer's buffer),
        # read by every row with batch stride 0 (tw_decode_attn_hs) instead of B copies: the fallback batch's
        # cross-attention reads 1/B of the bytes and each row still sees exactly its batch-1 K/V.  The captured step
        # bakes the call's strides in, so a change of mode drops the graph (recaptured on the next run)
        if self.graph is not None and shared != self.xkv_shared:
            self.graph = None
        self.xkv_shared = shared
        # the projection goes through one [nb*Tk][2d] scratch block that lives only for this call
        # (3.9 GB at the 512-clip large-v2 batch; the caching allocator reuses it for the next window)
        proj = torch.empty(nb * self.Tk, 2 * d, dtype=m.act_dtype, device=m.device)
        for i, kv in enumerate(self.cross_kv):
            p = f"model.decoder.layers.{i}.encoder_attn"
            wkv = m.wspan(p + ".k_proj.weight", p + ".v_proj.weight", (2 * d, d))
            bkv = m.wspan(p + ".k_proj.zero_bias", p + ".v_proj.bias", (2 * d,))
            m._lin(enc16, wkv, bkv, proj)
            if self.xkv_fp8:        # the same 16-bit projection, then quantised per (clip, head) block
                F.kv_head_major_fp8(proj, 2 * d, kv, self.cross_scale[i], nb, self.Tk, self.H)
            else:
                F.kv_head_major(proj, 2 * d, kv, nb, self.Tk, self.H)
        del proj

    def set_pads(self, pads, shift_positions=False):
        """pads: per-row count of left pad columns of this window's prompt; the pad columns are masked from the
        row's self-attention.  None: the plain entry points, today's calls.  A list, all zeros included, takes the
        per-row entries (with every start 0 tw_decode_attn_ks computes the plain entry's result bit for bit), so a
        caller whose windows alternate between equal and unequal prompt lengths keeps one captured step.
        shift_positions False (the default): every row embeds at its column index, which is what transformers 5.15
        computes for Whisper (generate derives position ids from the mask for decoder-only models only,
        generation/utils.py _prepare_position_ids_for_generation).  True: the row's positions count from its first
        real token, and the row then decodes exactly what its unpadded prompt decodes.  The captured step bakes in
        which entry points it calls, so a change of mode drops the graph (recaptured on the next run); the counts
        themselves are device data."""
        padded = pads is not None
        pads = [int(p) for p in pads] if padded else []
        shifted = padded and bool(shift_positions)
        if self.graph is not None and (padded != self.padded or shifted != self.shifted):
            self.graph = None
        self.padded, self.shifted = padded, shifted
        if padded:
            assert len(pads) == self.B and min(pads) >= 0
            v = torch.tensor(pads, dtype=torch.int32)
            self.k_start.copy_(v)
            self.pos_off.copy_(v)

    def _ln(self, x, name, y):
        m = self.m
        F.layernorm_fwd(x, m.ln_param(name + ".weight"), m.ln_param(name + ".bias"), y)
        return y

    def _ln_lin(self, x, ln, w, b, out, y, flags=F.GEMM_ROUND, kv=None):
        """out = Linear(LayerNorm(x)): one GEMV launch (batch <= 4, bf16 stream) or LN (into y) + GEMM.  kv: the
        GEMV also appends columns >= kv[3] to the self-attention cache row (only on the GEMV path)."""
        m = self.m
        if self.gemv_ln:
            self._gemv(x, w, out, ln_w=m.ln_param(ln + ".weight"), ln_b=m.ln_param(ln + ".bias"), bias=b, flags=flags,
                       kv=kv)
        else:
            y = self._ln(x, ln, y)
            if self.gemv:
                self._gemv(y, w, out, bias=b, flags=flags)
            else:
                m._lin(y, w, b, out, flags=flags)
        return out

    def _gemv(self, a, w, out, **kw):
        """One GEMV launch; w is a 16-bit weight, or (bytes, row scales) with decode_weight_dtype on (_weight)."""
        if isinstance(w, tuple):
            F.gemv_w8(a, w[0], w[1], out, **kw)
        else:
            F.gemv(a, w, out, **kw)

    def _weight(self, first, last=None, shape=None):
        """The weight of one of the step's Linears as this session reads it: the model's 16-bit view (first .. last: a
        fused span), or with decode_weight_dtype on its e4m3 bytes and row scales (GEMV path) / the 16-bit copy of
        its dequantised values (GEMM path)."""
        m = self.m
        if self.w8:
            return m.decode_weight_fp8(first) if self.gemv else m.decode_weight_dequantised(first)
        return m._w16(first) if last is None else m.wspan(first, last, shape)

    def _lin(self, a, w, b, out, res=None, flags=F.GEMM_ROUND):
        if self.gemv:
            self._gemv(a, w, out, bias=b, res=res, flags=flags)
        else:
            self.m._lin(a, w, b, out, res=res, flags=flags)
        return out

    def _embed_tables(self):
        m = self.m
        if m.store.p32 is not None:
            return m.store.v32("model.decoder.embed_tokens.weight"), m.store.v32("model.decoder.embed_positions.weight")
        return m.store.v16("model.decoder.embed_tokens.weight"), m.store.v16("model.decoder.embed_positions.weight")

    def _layers(self, b, sb, rows, self_attn, cross_attn, head=True):
        """The decoder layers and the head on the b.M rows embedded in b.x: per layer the fused QKV, k and v to the
        cache (row m of b to cache row *t_dev of the block m * sb elements in; `rows` bounds that row), self_attn(b,
        cache) into b.o, out-proj, cross-q, cross_attn(b, layer index) into b.o, out-proj, MLP.  head=False stops
        after the last layer."""
        m, d, t_dev = self.m, self.d, self.t_dev
        x, o, y = b.x, b.o, b.y
        for i in range(m.config.decoder_layers):
            p = f"model.decoder.layers.{i}"
            # self attention: fused QKV -> staging; k, v appended to the cache
            wqkv = self._weight(p + ".self_attn.q_proj.weight", p + ".self_attn.v_proj.weight", (3 * d, d))
            bqkv = m.wspan(p + ".self_attn.q_proj.bias", p + ".self_attn.v_proj.bias", (3 * d,))
            cache = self.self_kv[i]
            if self.gemv_ln:        # k, v written to the cache by the QKV GEMV itself
                self._ln_lin(x, p + ".self_attn_layer_norm", wqkv, bqkv, b.qkv, y, kv=(cache, sb, 2 * d, d, t_dev, rows))
            else:
                self._ln_lin(x, p + ".self_attn_layer_norm", wqkv, bqkv, b.qkv, y)
                F.kv_append(b.qkv[:, d:], 3 * d, cache, 2 * d, sb, b.M, 2 * d, t_dev, rows)
            self_attn(b, cache)
            self._lin(o, self._weight(p + ".self_attn.out_proj.weight"), m._w16(p + ".self_attn.out_proj.bias"), x,
                      res=x)
            # cross attention over the encoder frames
            self._ln_lin(x, p + ".encoder_attn_layer_norm", self._weight(p + ".encoder_attn.q_proj.weight"),
                         m._w16(p + ".encoder_attn.q_proj.bias"), b.q, y)
            cross_attn(b, i)
            self._lin(o, self._weight(p + ".encoder_attn.out_proj.weight"), m._w16(p + ".encoder_attn.out_proj.bias"),
                      x, res=x)
            # MLP
            self._ln_lin(x, p + ".final_layer_norm", self._weight(p + ".fc1.weight"), m._w16(p + ".fc1.bias"), b.h, y,
                         flags=F.GEMM_ROUND | F.GEMM_GELU)
            self._lin(b.h, self._weight(p + ".fc2.weight"), m._w16(p + ".fc2.bias"), x, res=x)
        if head and (self.gemv_ln or (self.w8 and self.gemv)):    # the bytes have no GEMM: every GEMV session's head
            self._ln_lin(x, "model.decoder.layer_norm", self._weight("model.decoder.embed_tokens.weight"), None,
                         b.logits, y)
        elif head:
            m.lm_head(self._ln(x, "model.decoder.layer_norm", y), out=b.logits,
                      E=self._weight("model.decoder.embed_tokens.weight") if self.w8 else None)

    def alloc_multi(self, Q):
        """Activation buffers of step_multi: Q rows each (one row of the batch, Q consecutive positions)."""
        assert self.B == 1 and 1 <= Q <= F.MQ_MAX
        if self.mq is None or self.mq.M != Q:
            self.mq = _StepBufs(self.m, Q)
        return self.mq

    def _self_attn_mq(self, b, cache):
        d, Q = self.d, b.M
        F.decode_attn_mq(b.qkv, Q * 3 * d, 3 * d, cache, 2 * d, 0, cache.view(-1)[d:], 2 * d, 0, b.o, Q * d, d,
                         1, self.H, Q, 1, 0.125, tk_dev=self.t_dev, tk_max=self.T_max, causal=True)

    def _cross_attn_mq(self, b, i):         # the clip's [H][Tk][64] K then V blocks of layer i
        d, Q, n1, kv = self.d, b.M, self.H * self.Tk * 64, self.cross_kv[i]
        if self.xkv_fp8:
            s = self.cross_scale[i]
            F.decode_attn_mq_fp8(b.q, Q * d, d, kv, 64, 0, kv[n1:], 64, 0, s, s[self.H:], 0, b.o, Q * d, d, 1, self.H,
                                 Q, self.Tk, 0.125, hsk=self.Tk * 64, hsv=self.Tk * 64)
            return
        F.decode_attn_mq(b.q, Q * d, d, kv, 64, 0, kv[n1:], 64, 0, b.o, Q * d, d, 1, self.H, Q, self.Tk, 0.125,
                         hsk=self.Tk * 64, hsv=self.Tk * 64)

    def step_multi(self, Q, ids, select=None):
        """The forward of ONE row for the Q tokens ids[0..Q) at positions *t_dev .. *t_dev + Q - 1 (the verify pass
        of assisted decoding): the step's launches (_layers) with M = Q rows -- the Linears read each weight once for
        the Q rows (the GEMV at d % 256 == 0 on the 16-bit paths, else the GEMM; a row of either does not depend on M)
        -- K/V of the Q positions to cache rows t .. t+Q-1 (row j of the buffers to cache row t + j: batch stride =
        row stride), self-attention causal among the Q rows and cross-attention through tw_decode_attn_mq (each K / V
        row loaded once for the Q queries; per query the single-query arithmetic), Q logit rows.
        Position-independent (t read on the device); t_dev is NOT advanced: the caller decides how many positions
        stand (tw_spec_accept).  select(self, logits) runs after the head."""
        assert self.B == 1 and not self.padded and self.spare_ok(Q)
        b = self.alloc_multi(Q)
        E, Pe = self._embed_tables()
        F.embed_step_multi(ids, E, Pe, b.x, self.t_dev, Q)
        # the first of the Q cache rows written is below T_max - (Q - 1)
        self._layers(b, 2 * self.d, self.T_max - (Q - 1), self._self_attn_mq, self._cross_attn_mq)
        if select is not None:
            select(self, b.logits)

    def spare_ok(self, Q):
        return self.clamp_pos and Q <= F.MQ_MAX

    def _self_attn(self, b, cache):
        d, sb = self.d, self.T_max * 2 * self.d
        F.decode_attn(b.qkv, 3 * d, cache, 2 * d, sb, cache.view(-1)[d:], 2 * d, sb, b.o, d, self.B, self.H, 1, 0.125,
                      tk_dev=self.t_dev, tk_max=self.T_max, k_start=self.k_start if self.padded else None)

    def _cross_attn(self, b, i):
        B, H, Tk, d, kv = self.B, self.H, self.Tk, self.d, self.cross_kv[i]
        if self.xkv_fp8:        # the same two calls over bytes, with the blocks' scales (K's, then V's)
            s = self.cross_scale[i]
            if self.xkv_shared:
                F.decode_attn_fp8(b.q, d, kv, 64, 0, kv[H * Tk * 64:], 64, 0, s, s[H:], 0, b.o, d, B, H, Tk, 0.125,
                                  hsk=Tk * 64, hsv=Tk * 64)
            else:
                F.decode_attn_fp8(b.q, 64, kv, 64, Tk * 64, kv[B * H * Tk * 64:], 64, Tk * 64, s, s[B * H:], 1, b.o,
                                  64, B * H, 1, Tk, 0.125)
        elif self.xkv_shared:   # every row over the one clip's [H][Tk][64] blocks (batch stride 0)
            F.decode_attn(b.q, d, kv, 64, 0, kv[H * Tk * 64:], 64, 0, b.o, d, B, H, Tk, 0.125, hsk=Tk * 64,
                          hsv=Tk * 64)
        else:                   # B*H one-head clips over contiguous [Tk][64] runs
            F.decode_attn(b.q, 64, kv, 64, Tk * 64, kv[B * H * Tk * 64:], 64, Tk * 64, b.o, 64, B * H, 1, Tk, 0.125)

    def step(self, select=None, cur=None, head=True):
        """One decoder step at position *t_dev for input ids `cur` (default: self.cur); then t_dev += 1.
        select = (sup, beg, eos, done, ids, P) runs greedy selection into ids[:, t+1] and cur.  head=False stops
        after the last layer (a step that only fills the caches)."""
        b, t_dev, T_max = self.buf, self.t_dev, self.T_max
        cur = self.cur if cur is None else cur
        E, Pe = self._embed_tables()
        if self.clamp_pos:           # spare rows past the length cap: their positions clamp to the table
            assert self.B == 1 and not self.shifted
            F.embed_step_multi(cur, E, Pe, b.x, t_dev, 1)
        else:
            F.embed_step(cur, E, Pe, b.x, t_dev, T_max, pos_off=self.pos_off if self.shifted else None)
        self._layers(b, T_max * 2 * self.d, T_max, self._self_attn, self._cross_attn, head)
        if select is not None:
            select(self)
        F.step_advance(t_dev)

    def capture(self, select):
        """Record one selecting step into a HIP graph (nothing executes during capture)."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.step(select)
        self.graph = g


def _detect(model, gc, enc16, B, Tk, want_probs=False):
    """HF detect_language's decoder part on B clips' encoder rows: one step at position 0 on <|startoftranscript|>
    through a DecodeSession, then tw_lang_detect over the language ids -> (ids int64 [B], probs fp32 [B, L] or None,
    the id table)."""
    table = language_table(gc, model.config.vocab_size)
    dev = model.device
    sess = DecodeSession(model, enc16, B, Tk, 2)          # position 0 and a spare cache row
    sess.cur.fill_(int(gc.decoder_start_token_id))
    sess.step()
    ids = torch.empty(B, dtype=torch.int64, device=dev)
    probs = torch.empty(B, len(table), dtype=torch.float32, device=dev) if want_probs else None
    F.lang_detect(sess.logits, model.Vp, B, model.config.vocab_size, torch.tensor(table, dtype=torch.int32, device=dev),
                  ids, probs)
    return ids, probs, table


def _first_window(model, input_features):
    """HF's input_features[:, :, :3000]: the first 30 s of every input, zero-padded on the right when shorter."""
    window = 2 * model.config.max_source_positions
    f = input_features[:, :, :window]
    if f.shape[-1] < window:
        f = torch.nn.functional.pad(f, (0, window - f.shape[-1]))
    return f


def _resolve_gc(model):
    from .config import GenerationConfig
    gc = model.generation_config if model.generation_config is not None else GenerationConfig()
    if not isinstance(gc, GenerationConfig):
        gc = GenerationConfig(gc)
    if gc.eos_token_id is None:
        gc.eos_token_id = model.config.eos_token_id
    return gc


def _unwrap(encoder_outputs):
    """The encoder's last hidden state [B, Tk, d] out of what a caller passes as encoder_outputs (HF's ModelOutput or
    a tuple); None stays None."""
    if encoder_outputs is None:
        return None
    return encoder_outputs.last_hidden_state if hasattr(encoder_outputs, "last_hidden_state") else encoder_outputs[0]


def _encoder_rows(model, features, hidden):
    """The encoder rows a decode reads -> (enc16 [B * Tk, d] on the device, B, Tk): the caller's own encoder output
    `hidden` (_unwrap) when there is one, else `features` through the model's encoder."""
    if hidden is not None:
        B, Tk = hidden.shape[0], hidden.shape[1]
        return hidden.reshape(-1, model.config.d_model).to(model.device, model.act_dtype).contiguous(), B, Tk
    conv_in = model.conv_input(features)
    enc16 = model.encode(conv_in)
    B = conv_in.shape[0]
    return enc16, B, enc16.shape[0] // B


@torch.no_grad()
def detect_language(model, input_features=None, encoder_outputs=None, return_probs=False):
    """HF WhisperGenerationMixin.detect_language (transformers 5.15 generation_whisper.py:1610-1673): the language
    token id of each input, int64 [B] on the device -- the largest of the language logits at the position after
    <|startoftranscript|>.  Exactly one of input_features (cut to the first 3000 frames, zero-padded when shorter)
    and encoder_outputs.  return_probs=True: (ids, probs fp32 [B, L], ids_table) with probs[b, j] the softmax over
    the L = len(lang_to_id) language logits alone of language ids_table[j] (sorted ids); HF has no such output,
    faster-whisper's language_probability is this number.  Ties go to the lowest id, as torch.argmax; a row whose
    language logits are all -inf gives the lowest language id where HF gives token 0 (unreachable: logits are
    finite)."""
    if input_features is None and encoder_outputs is None:
        raise ValueError("You have to specify either `input_features` or `encoder_outputs`")
    if input_features is not None and encoder_outputs is not None:
        raise ValueError("Make sure to specify only one of `input_features` or `encoder_outputs` - not both!")
    gc = _resolve_gc(model)
    language_table(gc, model.config.vocab_size)
    feats = _first_window(model, input_features) if input_features is not None else None
    enc16, B, Tk = _encoder_rows(model, feats, _unwrap(encoder_outputs))
    ids, probs, table = _detect(model, gc, enc16, B, Tk, return_probs)
    return (ids, probs, table) if return_probs else ids


class _Select:
    """Per-step token selection into ids[:, t+1] (t read on the device): HF SuppressTokens,
    SuppressTokensAtBegin and, with timestamps, WhisperTimeStampLogitsProcessor + argmax."""

    def __init__(self, gc, B, V, T_max, P, dev, timestamps, track=False, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, Vp=None, logp=False):
        track = track or logp            # the per-token values come from the tracking kernels (1/T = 0: argmax)
        self.V, self.P, self.ts, self.track = V, P, timestamps, track
        # HF RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor: launch-time scalars of the pre-pass
        # (baked into a captured step) and its fp32 output rows [B][Vp]; neither active: no scratch, today's calls
        self.penalty, self.ngram = float(repetition_penalty), int(no_repeat_ngram_size)
        self.repeat = self.penalty != 1.0 or self.ngram > 0
        self.scratch = torch.empty(B, Vp, dtype=torch.float32, device=dev) if self.repeat else None
        self.eos = int(gc.eos_token_id)
        self.sup = F.token_bitmask(gc.suppress_tokens or [], V, dev)
        self.beg = F.token_bitmask(gc.begin_suppress_tokens or [], V, dev)
        self.ids = torch.full((B, T_max), self.eos, dtype=torch.int64, device=dev)
        self.done = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.last_ts = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.no_ts = int(gc.no_timestamps_token_id)
        mi = gc.max_initial_timestamp_index if "max_initial_timestamp_index" in gc else None
        self.max_initial = -1 if mi is None else int(mi)
        # temperature fallback: one sampling control word (1/T, seed) per row, read on the device, so a captured
        # graph serves every temperature and the rows of a batch can be different fallback attempts; running
        # log-prob of the chosen tokens
        self.B = B
        self.ctl = torch.zeros(3 * B, dtype=torch.int32, device=dev) if track else None
        self.sum_logp = torch.zeros(B, dtype=torch.float32, device=dev) if track else None
        # logp (generate(return_token_logprobs=True)): the log-prob of every selected token at its column of the id
        # matrix, written by the _lp kernels (baked into a captured step); off: nothing allocated, today's calls
        self.tok_logp = torch.zeros(B, T_max, dtype=torch.float32, device=dev) if logp else None

    def reset(self, prompt, temperature=0.0, seed=0):
        """temperature / seed: one value for every row, or one per row."""
        self.ids.fill_(self.eos)
        self.ids[:, :self.P] = prompt
        self.done.zero_()
        self.last_ts.fill_(-1)
        temps = list(temperature) if isinstance(temperature, (list, tuple)) else [temperature] * self.B
        seeds = list(seed) if isinstance(seed, (list, tuple)) else [seed] * self.B
        if self.tok_logp is not None:
            self.tok_logp.zero_()
        if self.track:
            self.sum_logp.zero_()
            F.sample_ctl(temps, seeds, self.ctl)
        elif any(temps):
            raise ValueError("sampling needs a tracking selector (track=True)")

    def __call__(self, sess):
        self.launch(sess.logits, sess.t_dev, sess.cur, B=sess.B)

    def launch(self, logits, t_dev, next_ids, col=1, sum_logp=None, B=1):
        """The selection kernel this selector's mode takes (plain, timestamps, or the tracking forms with their
        per-row control word) on `logits` ([B][Vp] rows) into ids[:, *t_dev + col] and next_ids.  sum_logp: where the
        tracking forms accumulate (default: the selector's running sum, and with it the selector's per-token matrix
        when it keeps one; a caller that redirects the sum -- the verify pass's slots -- stores the per-token values
        itself, tw_spec_accept_lp).  With a repetition penalty or a no-repeat
        n-gram size, tw_repeat_process first writes the rows, processed for the history ids[:, :*t_dev + col], to the
        selector's fp32 scratch, and the selection kernel reads that instead (HF runs the two processors first)."""
        Vp = logits.stride(0)
        if self.repeat:
            assert B <= self.scratch.shape[0] and Vp == self.scratch.shape[1]
            logits = F.repeat_process(logits, Vp, B, self.V, self.ids, col, self.scratch[:B], self.penalty,
                                      self.ngram, t_dev=t_dev)
        if self.track:
            slp = self.sum_logp if sum_logp is None else sum_logp
            lp = dict(tok_logp=self.tok_logp) if sum_logp is None and self.tok_logp is not None else {}
            if self.ts:
                F.select_sample_ts(logits, Vp, B, self.V, self.sup, self.beg, self.eos, self.done, self.ids,
                                   col, next_ids, self.last_ts, self.P, self.ctl, slp, ts_begin=self.no_ts + 1,
                                   no_ts=self.no_ts, max_initial=self.max_initial, t_dev=t_dev, **lp)
            else:
                F.select_sample(logits, Vp, B, self.V, self.sup, self.beg, False, self.eos, self.done,
                                self.ids, col, next_ids, self.ctl, slp, t_dev=t_dev, begin_col=self.P, **lp)
        elif self.ts:
            F.greedy_select_ts(logits, Vp, B, self.V, self.sup, self.beg, self.eos, self.done, self.ids, col,
                               next_ids, self.last_ts, self.P, ts_begin=self.no_ts + 1, no_ts=self.no_ts,
                               max_initial=self.max_initial, t_dev=t_dev)
        else:
            F.greedy_select(logits, Vp, B, self.V, self.sup, self.beg, False, self.eos, self.done, self.ids,
                            col, next_ids, t_dev=t_dev, begin_col=self.P)


class _PromptedDecode:
    """What a plain and an assisted decode of one window share: the session set-up, the prompt prefill with the
    no-speech probe, and HF's trimming of the result.  Subclasses hold m, B, P, T_max, sel and ns_logp."""

    def _open(self, sess, model, enc, Tk, spare=0):
        """The session of `model` over this window's encoder rows: built on first use, re-projected in place after."""
        # the K/V format and the weight format are the session's for life
        if (sess is None or sess.xkv_dtype != getattr(model, "cross_kv_dtype", None)
                or sess.w8 != (getattr(model, "decode_weight_dtype", None) == "fp8_e4m3")):
            return DecodeSession(model, enc, self.B, Tk, self.T_max, spare=spare)
        sess.set_encoder(enc)
        return sess

    def _probe(self, logits, no_speech):
        """log-softmax of the raw logits at no_speech's token -> ns_logp (WhisperNoSpeechDetection)."""
        F.token_logprob(logits, self.m.Vp, self.B, self.m.config.vocab_size, no_speech[1], self.ns_logp)

    def _prefill(self, sessions, no_speech, detect=None):
        """Prompt columns 0 .. P - 2 through every session, from position 0; the first session is the one whose
        logits at the <|startoftranscript|> position the no-speech probe reads.
        detect (a device int32 table of language ids, language_table): the step at column 0 is HF's detection step,
        so tw_lang_detect writes each row's language id from the first session's logits into column 1 of the id
        matrix, on the device, before the prefill reads that column (the prompt holds a placeholder there; column 0
        must be <|startoftranscript|>, i.e. no prompt_ids)."""
        for sess in sessions:
            sess.t_dev.zero_()
        for t in range(self.P - 1):
            for sess in sessions:
                sess.cur.copy_(self.sel.ids[:, t])
                sess.step()
                if sess is sessions[0] and no_speech is not None and t == no_speech[0]:
                    self._probe(sess.logits, no_speech)
                if sess is sessions[0] and detect is not None and t == 0:
                    F.lang_detect(sess.logits, self.m.Vp, self.B, self.m.config.vocab_size, detect,
                                  self.sel.ids[:, 1])

    def _trim(self, t):
        """The generated columns up to t without the trailing ones in which every row had already finished (HF stops
        at the step where the last row emits eos)."""
        gen = self.sel.ids[:, self.P:t + 1]
        is_eos = (gen == self.sel.eos).cpu()
        B = gen.shape[0]
        first = torch.where(is_eos.any(1), is_eos.int().argmax(1), torch.full((B,), gen.shape[1]))
        L = int(min(gen.shape[1], int(first.max()) + 1)) if B else 0
        if self.sel.tok_logp is not None:       # the same columns of the per-token log-probs, beside the ids
            return gen[:, :L], self.sel.tok_logp[:, self.P:self.P + L]
        return gen[:, :L]


class _Decoder(_PromptedDecode):
    """One greedy decode of B windows with a fixed prompt; reusable across windows (long-form):
    the captured step graph stays valid because every buffer it touches is reused in place."""

    def __init__(self, model, gc, B, Tk, P, max_length, timestamps, use_graph, track=False, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, logp=False):
        self.m, self.P, self.T_max, self.use_graph = model, P, max_length, use_graph
        self.sess = None
        self.sel = _Select(gc, B, model.config.vocab_size, max_length, P, model.device, timestamps, track,
                           repetition_penalty, no_repeat_ngram_size, Vp=model.Vp, logp=logp)
        self.B, self.Tk = B, Tk
        self.ns_logp = torch.zeros(B, dtype=torch.float32, device=model.device) if track else None

    def run(self, enc16, prompt, temperature=0.0, seed=0, no_speech=None, pads=None, shift_positions=False,
            detect=None):
        """prompt: int64 [B, P] (device) -> generated ids [B, L] (device), HF trimming; a decoder built with
        logp=True -> (ids, per-token log-probs fp32 [B, L]: 0 after a row's eos).
        detect: the device table of language ids -> the languages are detected inside the prefill (_prefill) and
        sel.ids[:, 1] holds them afterwards; `prompt` carries any valid language id there.
        pads: per-row count of leading pad columns of `prompt` (rows left-padded to the longest prompt of the batch,
        as HF pads them): those columns are masked from the row's self-attention; every row embeds at its column
        index, as HF does.  shift_positions=True instead counts a row's positions from its first real token, so that
        it decodes what its unpadded prompt decodes (DecodeSession.set_pads).
        no_speech = (sot_position, token): log-softmax of the raw logits at the <|startoftranscript|>
        position for that token goes to self.ns_logp (WhisperNoSpeechDetection)."""
        sel, P = self.sel, self.P
        sess = self.sess = self._open(self.sess, self.m, enc16, self.Tk)
        sess.set_pads(pads, shift_positions)
        sel.reset(prompt, temperature, seed)
        assert detect is None or (P >= 2 and pads is None)
        self._prefill([sess], no_speech, detect)
        sess.cur.copy_(sel.ids[:, P - 1])
        if self.use_graph and sess.graph is None:
            sess.capture(sel)
        t = P - 1
        while t + 1 < self.T_max:
            if self.use_graph:
                sess.graph.replay()
            else:
                sess.step(sel)
            if no_speech is not None and t == P - 1 and no_speech[0] == P - 1:
                self._probe(sess.logits, no_speech)
            t += 1
            if (t - P) % 8 == 7 and bool(sel.done.all()):
                break
        return self._trim(t)


class _SpecDecoder(_PromptedDecode):
    """Assisted (speculative) greedy decode of ONE window: _Decoder.run's signature and result.  A round: the
    assistant drafts k tokens with its own DecodeSession (k + 1 steps: the last one only puts the last draft's K/V
    into the assistant's cache, without the LM head, so that a fully accepted round leaves the assistant caught up),
    the target scores the k + 1 positions in one pass (DecodeSession.step_multi), k + 1 launches of the selection
    kernel the plain decode would have used pick the target's token of each position -- launch j + 1 sees the right
    context exactly when draft j was accepted -- and tw_spec_accept keeps the accepted prefix and rolls the rest
    back, all on the device.  The round is position-independent, so it is captured once as one HIP graph; the host
    reads the step counter and the finished flag every 4 rounds.
    Both models write one id matrix: the drafts go to columns t+1 .. t+k, where the assistant's timestamp rules and
    then the target's selection read them, and the target's tokens overwrite them in place.  Every accepted
    position's logits are those of the plain decode (a row of the step's Linears does not depend on how many rows
    run with it; tw_decode_attn_mq computes each query as the single-query kernel does), so the ids, the summed
    log-prob and the no-speech probability equal the plain decode's."""

    def __init__(self, model, assistant, gc, Tk, P, max_length, timestamps, use_graph, track=False, k=None,
                 logp=False):
        track = track or logp
        self.m, self.a, self.P, self.T_max, self.use_graph = model, assistant, P, max_length, use_graph
        self.k = DEFAULT_ASSISTANT_TOKENS if k is None else int(k)
        assert 1 <= self.k <= MAX_ASSISTANT_TOKENS
        Q = self.k + 1
        dev = model.device
        V = model.config.vocab_size
        self.sel = _Select(gc, 1, V, max_length + Q, P, dev, timestamps, track, logp=logp)
        self.sel_a = _Select(gc, 1, V, 1, P, dev, timestamps, False)     # the assistant: plain greedy, own flags
        self.sel_a.ids = self.sel.ids
        self.B, self.Tk = 1, Tk
        self.ns_logp = torch.zeros(1, dtype=torch.float32, device=dev) if track else None
        self.vin = torch.zeros(Q, dtype=torch.int64, device=dev)         # [current token, draft 0 .. draft k-1]
        self.sink = torch.zeros(1, dtype=torch.int64, device=dev)
        self.slots = torch.zeros(Q, dtype=torch.float32, device=dev) if track else None
        self.done_snap = torch.zeros(1, dtype=torch.uint8, device=dev)
        self.hist = torch.zeros(1 + max(1, max_length - P), dtype=torch.int32, device=dev)
        self.sess = self.sess_a = self.graph = None
        self.accepted = []               # per round of the last run: the number of drafts accepted

    def _verify_select(self, sess, logits):
        for j in range(self.k + 1):
            self.sel.launch(logits[j:j + 1], sess.t_dev, self.sink, col=1 + j,
                            sum_logp=self.slots[j:j + 1] if self.slots is not None else None)

    def _round(self):
        k, sel, sel_a, sa, st, vin = self.k, self.sel, self.sel_a, self.sess_a, self.sess, self.vin
        for i in range(k + 1):
            if i < k:
                sa.step(lambda s, i=i: sel_a.launch(s.logits, s.t_dev, vin[i + 1:i + 2]), cur=vin[i:i + 1])
            else:
                sa.step(cur=vin[i:i + 1], head=False)
        st.step_multi(k + 1, vin, self._verify_select)
        F.spec_accept(vin[1:], k, sel.ids[0], self.T_max, sel.eos, st.t_dev, vin[:1], sel.done, self.done_snap,
                      t_dev_a=sa.t_dev, done_a=sel_a.done, last_ts=sel.last_ts if sel.ts else None,
                      last_ts_a=sel_a.last_ts if sel.ts else None, begin_col=self.P, ts_begin=sel.no_ts + 1,
                      slots=self.slots, sum_logp=sel.sum_logp if self.slots is not None else None, hist=self.hist,
                      tok_logp=sel.tok_logp[0] if sel.tok_logp is not None else None)

    def run(self, enc16, prompt, temperature=0.0, seed=0, no_speech=None, pads=None, shift_positions=False,
            enc_a=None):
        """enc_a: the assistant's encoder rows for this window (its own encoder's output, or the target's cast to the
        assistant's dtype for a decoder-only assistant)."""
        if pads is not None and any(int(p) for p in pads):
            raise NotImplementedError("tw generate: assisted decoding takes unpadded prompts")
        if isinstance(temperature, (list, tuple)):
            temperature = temperature[0]
        if temperature:
            raise NotImplementedError("tw generate: assisted decoding is greedy (temperature 0)")
        sel, sel_a, P, Q = self.sel, self.sel_a, self.P, self.k + 1
        enc_a = enc16 if enc_a is None else enc_a
        st = self.sess = self._open(self.sess, self.m, enc16, self.Tk, spare=Q)
        sa = self.sess_a = self._open(self.sess_a, self.a, enc_a, enc_a.shape[0], spare=Q)
        sel.reset(prompt, 0.0, seed if not isinstance(seed, (list, tuple)) else seed[0])
        sel_a.done.zero_()
        sel_a.last_ts.fill_(-1)
        self.done_snap.zero_()
        self.hist.zero_()
        if self.slots is not None:
            self.slots.zero_()
        self._prefill([st, sa], no_speech)
        self.vin[:1].copy_(sel.ids[0, P - 1:P])
        if self.use_graph and self.graph is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._round()
            self.graph = g
        r, t = 0, P - 1
        while r < self.T_max - P:                                # every live round accepts at least one token
            if self.use_graph:
                self.graph.replay()
            else:
                self._round()
            if r == 0 and no_speech is not None and no_speech[0] == P - 1:
                self._probe(st.mq.logits, no_speech)
            r += 1
            if r % 4 == 0:
                t = int(st.t_dev)
                if t + 1 >= self.T_max or bool(sel.done.all()):
                    break
        t = int(st.t_dev)
        h = self.hist.tolist()
        self.accepted = h[1:1 + h[0]]
        return self._trim(t)


class _BeamDecoder:
    """Beam search over B clips x k beams with the same prompt (with `timestamps`, one window of the seek loop): HF
    GenerationMixin._beam_search (transformers 5.15 generation/utils.py:3208-3560), the search behind
    `training/run_eval.py:144-147` (--num_beams) and `run_distillation.py:1476-1484` (generation_num_beams).
    The B*k rows decode as one batch on the engine's step (DecodeSession, every clip's encoder rows repeated k
    times); per step, on the device: fp32 log-softmax of the logits, the suppress processors on the log-probs,
    plus the running scores, the top 2k of k*V candidates, the k best unfinished continue (the self-attention
    caches gathered by their source beams), finished candidates among the top k enter the per-clip set of k
    hypotheses with score sum(log p) / generated_length ** length_penalty; the search stops when no running beam
    can beat the worst kept hypothesis (early_stopping False: the heuristic at the current length) or every
    candidate hits max_length."""

    def __init__(self, model, gc, B, nb, Tk, P, max_length, timestamps=None):
        self.m, self.gc, self.B, self.nb, self.Tk, self.P, self.T_max = model, gc, B, nb, Tk, P, max_length
        # timestamps: (ts_begin, no_ts, max_initial) -> HF WhisperTimeStampLogitsProcessor on the log-probs after the
        # suppress processors (generation_whisper.py _retrieve_logit_processors order), begin_index = P; with it the
        # decoder also tracks, per hypothesis, the sum over its steps of log_softmax(processed row)[token] -- what HF's
        # _retrieve_avg_logprobs sums over the chosen beam's scores (beam_indices) for the fallback gate
        self.ts = timestamps
        self.sum_logp = None      # [B] after run(): that sum for each clip's best hypothesis
        self.ns_prob = None       # [B] after run(no_speech=...): no-speech probability (_ns)
        dev = model.device
        self.V = model.config.vocab_size
        self.eos = int(gc.eos_token_id)
        pad = getattr(gc, "pad_token_id", None)
        self.fill = int(pad) if pad is not None else self.eos
        self.sup = torch.tensor(sorted(set(gc.suppress_tokens or [])), dtype=torch.int64, device=dev)
        self.beg = torch.tensor(sorted(set(gc.begin_suppress_tokens or [])), dtype=torch.int64, device=dev)
        self.length_penalty = float(getattr(gc, "length_penalty", 1.0) if getattr(gc, "length_penalty", None)
                                    is not None else 1.0)
        es = getattr(gc, "early_stopping", False)
        self.early_stopping = False if es is None else es

    def _ns(self, sess, token):
        """WhisperNoSpeechDetection under beam search (is_scores_logprobs): exp of the fp32 log-softmax of the raw
        logits at <|startoftranscript|>, the first beam row of each clip (every beam row holds the prompt there)."""
        lg = sess.logits.view(self.B, self.nb, -1)[:, 0, :self.V].float()
        return torch.log_softmax(lg, dim=-1)[:, token].exp()

    @staticmethod
    def _gather(t, idx):
        """HF _gather_beams: t [B, K, ...] rows picked per clip by idx [B, k]."""
        while idx.dim() < t.dim():
            idx = idx.unsqueeze(-1)
        return torch.gather(t, 1, idx.expand(*idx.shape[:2], *t.shape[2:]))

    def _ts_rules(self, logp, run_seq, run_last_ts, cur):
        """HF WhisperTimeStampLogitsProcessor (transformers generation/logits_process.py) on the B*k processed
        log-prob rows, vectorised: <|notimestamps|> masked; timestamps in pairs (after a pair no timestamp, after a single
        one no text); timestamps never decrease (nor repeat <|0.00|>); the first step a timestamp <= max_initial; then
        text masked where the timestamps' summed probability beats every text token."""
        tb, no_ts, max_initial = self.ts
        eos = self.eos
        BN, V = logp.shape
        logp[:, no_ts] = -float("inf")
        ngen = cur - self.P
        cols = torch.arange(V, device=logp.device)
        if ngen >= 1:
            last = run_seq[:, :, cur - 1].reshape(-1)
            last_is = last >= tb
            pen_is = (run_seq[:, :, cur - 2].reshape(-1) >= tb) if ngen >= 2 else torch.ones_like(last_is)
            kill_ts = last_is & pen_is
            kill_text = last_is & ~pen_is
            logp.masked_fill_(kill_ts[:, None] & (cols >= tb)[None, :], -float("inf"))
            logp.masked_fill_(kill_text[:, None] & (cols < eos)[None, :], -float("inf"))
            lts = run_last_ts.reshape(-1)
            lim = torch.where(kill_text, lts, lts + 1)
            logp.masked_fill_((lts >= 0)[:, None] & (cols >= tb)[None, :] & (cols[None, :] < lim[:, None]),
                              -float("inf"))
        else:
            logp[:, :tb] = -float("inf")
            if max_initial is not None:
                logp[:, tb + max_initial + 1:] = -float("inf")
        lp2 = torch.log_softmax(logp.float(), dim=-1)
        ts_mass = torch.logsumexp(lp2[:, tb:], dim=-1)
        text_max = lp2[:, :tb].max(dim=-1).values
        logp.masked_fill_((ts_mass > text_max)[:, None] & (cols < tb)[None, :], -float("inf"))
        return logp

    def run(self, enc16, prompt, no_speech=None):
        """enc16: [B*Tk, d] encoder rows; prompt: int64 [P] (device or host) -> generated ids [B, L] (device).
        no_speech = (sot_position, token): softmax of the raw logits at that prompt position for that token goes to
        self.ns_prob (WhisperNoSpeechDetection)."""
        m, B, nb, P, T_max, V = self.m, self.B, self.nb, self.P, self.T_max, self.V
        dev = m.device
        d = m.config.d_model
        BN = B * nb
        prompt = torch.as_tensor(prompt, dtype=torch.int64, device=dev)
        enc_rep = enc16.view(B, self.Tk, d).repeat_interleave(nb, 0).reshape(BN * self.Tk, d).contiguous()
        sess = DecodeSession(m, enc_rep, BN, self.Tk, T_max)
        del enc_rep
        sess.t_dev.zero_()
        pl = prompt.tolist()                                     # one host read for the whole prompt
        for t in range(P - 1):                                   # prompt prefill (identical on every row)
            sess.cur.fill_(pl[t])
            sess.step()
            if no_speech is not None and t == no_speech[0]:
                self.ns_prob = self._ns(sess, no_speech[1])
        sess.cur.fill_(pl[P - 1])
        K = max(2, 2) * nb                                       # beams_to_keep: (1 eos token + 1) * k
        top_mask = torch.zeros(K, dtype=torch.bool, device=dev)
        top_mask[:nb] = True
        run_seq = torch.full((B, nb, T_max), self.fill, dtype=torch.int64, device=dev)
        run_seq[:, :, :P] = prompt
        seqs = run_seq.clone()
        run_scores = torch.zeros(B, nb, dtype=torch.float32, device=dev)
        run_scores[:, 1:] = -1e9
        scores = torch.full((B, nb), -1e9, dtype=torch.float32, device=dev)
        finished = torch.zeros(B, nb, dtype=torch.bool, device=dev)
        heur_unsat = torch.ones(B, 1, dtype=torch.bool, device=dev)
        run_bidx = torch.full((B, nb, T_max - P), -1, dtype=torch.int32, device=dev)
        bidx = run_bidx.clone()
        lp, es = self.length_penalty, self.early_stopping
        rows_ident = torch.arange(BN, dtype=torch.int64, device=dev)
        ts = self.ts is not None
        run_last_ts = torch.full((B, nb), -1, dtype=torch.int64, device=dev)     # last timestamp token per beam
        run_sum = torch.zeros(B, nb, dtype=torch.float32, device=dev)            # sum of renormalised log-probs
        fin_sum = torch.zeros(B, nb, dtype=torch.float32, device=dev)
        cur = P
        while True:
            sess.step()                                          # logits of position cur - 1 on every row
            if no_speech is not None and cur == P and no_speech[0] == P - 1:
                self.ns_prob = self._ns(sess, no_speech[1])
            logp = torch.log_softmax(sess.logits[:, :V].float(), dim=-1)
            if self.sup.numel():
                logp[:, self.sup] = -float("inf")
            if cur == P and self.beg.numel():                    # SuppressTokensAtBegin (begin_index = P)
                logp[:, self.beg] = -float("inf")
            if ts:
                logp = self._ts_rules(logp, run_seq, run_last_ts, cur)
            acc = (logp.view(B, nb, V) + run_scores[:, :, None]).reshape(B, nb * V)
            # _get_top_k_continuations
            top_lp, top_i = torch.topk(acc, k=K)
            src = top_i // V
            tok = top_i % V
            if ts:
                # HF's gate sums log_softmax(processed row)[token] along the chosen beam: processed - lse(processed)
                lse = torch.logsumexp(logp, dim=-1).view(B, nb)
                contrib = torch.gather(logp.view(B, nb * V), 1, top_i) - torch.gather(lse, 1, src)
                top_sum = torch.gather(run_sum, 1, src) + contrib
                top_last_ts = torch.where(tok >= self.ts[0], tok, torch.gather(run_last_ts, 1, src))
            top_bidx = self._gather(run_bidx, src)
            top_seq = self._gather(run_seq, src)
            top_seq[:, :, cur] = tok
            top_bidx[:, :, cur - P] = (src + torch.arange(B, device=dev).view(-1, 1) * nb).to(torch.int32)
            # stopping criteria on each candidate: eos, or the sequence reaching max_length
            hits = (tok == self.eos) | (cur + 1 >= T_max)
            # _get_running_beams_for_next_iteration
            run_lp = top_lp + hits.to(torch.float32) * -1.0e9
            nxt = torch.topk(run_lp, k=nb)[1]
            run_seq = self._gather(top_seq, nxt)
            run_scores = self._gather(run_lp, nxt)
            run_bidx = self._gather(top_bidx, nxt)
            if ts:
                run_sum = self._gather(top_sum, nxt)
                run_last_ts = self._gather(top_last_ts, nxt)
            # _update_finished_beams
            just = hits & top_mask[None, :]
            fin_lp = top_lp / ((cur + 1 - P) ** lp)
            full = torch.all(finished, dim=-1, keepdim=True) & (es is True)
            fin_lp = fin_lp + full.to(torch.float32) * -1.0e9
            fin_lp = fin_lp + (~heur_unsat).to(torch.float32) * -1.0e9
            fin_lp = fin_lp + (~just).to(torch.float32) * -1.0e9
            m_seq = torch.cat((seqs, top_seq), 1)
            m_sc = torch.cat((scores, fin_lp), 1)
            m_bi = torch.cat((bidx, top_bidx), 1)
            m_fin = torch.cat((finished, just), 1)
            keep = torch.topk(m_sc, k=nb)[1]
            seqs, scores = self._gather(m_seq, keep), self._gather(m_sc, keep)
            bidx, finished = self._gather(m_bi, keep), self._gather(m_fin, keep)
            if ts:
                fin_sum = self._gather(torch.cat((fin_sum, top_sum), 1), keep)
            # the next step's inputs: each running beam's new token, its source row's caches
            src_rows = run_bidx[:, :, cur - P].reshape(-1).to(torch.int64)
            sess.cur.copy_(run_seq[:, :, cur].reshape(-1))
            cur += 1
            # _check_early_stop_heuristic / _beam_search_has_unfinished_sequences
            if es == "never" and lp > 0.0:
                best_len = T_max - P
            else:
                best_len = cur - P
            best_run = run_scores[:, :1] / (best_len ** lp)
            worst_fin = torch.where(finished, torch.min(scores, dim=1, keepdim=True)[0], torch.full_like(scores, -1e9))
            heur_unsat = heur_unsat & torch.any(best_run > worst_fin, dim=-1, keepdim=True)
            # one host read per step for every decision: continue?  and is the beam reorder the identity (every
            # running beam continues its own row), in which case the cache gather is skipped
            flags = torch.stack([torch.any(heur_unsat), torch.all(finished), torch.all(hits),
                                 (src_rows == rows_ident).all()]).tolist()
            go = flags[0] and not (flags[1] and es is True) and not flags[2]
            if not go or cur >= T_max:
                break
            if not flags[3]:
                for c in sess.self_kv:
                    c[:, :cur - 1].copy_(c[:, :cur - 1].index_select(0, src_rows))
        best = seqs[:, 0]
        gen_len = int(((bidx[:, 0] + 1) != 0).sum(dim=1).max())
        if ts:
            self.sum_logp = fin_sum[:, 0]
        return best[:, P:P + gen_len]


def retrieve_segment(seq, seek_num_frames, ts_begin=50364, input_stride=2):
    """HF `_retrieve_segment` (generation_whisper.py), token part: split a window's tokens at
    consecutive timestamp pairs -> (segments, seek offset in feature frames)."""
    is_ts = [t >= ts_begin for t in seq]
    single_end = is_ts[-2:] == [False, True]
    cut = [i + 1 for i in range(len(seq) - 1) if is_ts[i] and is_ts[i + 1]]
    if not cut:
        return [list(seq)], seek_num_frames
    slices = list(cut)
    if single_end:
        slices.append(len(seq))
    else:
        slices[-1] += 1
    segs, last = [], 0
    for c in slices:
        segs.append(list(seq[last:c]))
        last = c
    off = seek_num_frames if single_end else (seq[last - 2] - ts_begin) * input_stride
    return segs, off


def segment_logprobs(lps, segs):
    """The per-token values `lps` of a window's tokens cut as retrieve_segment cut the tokens into `segs`: the
    segments are consecutive slices from the window's first token (tokens after the last cut belong to none)."""
    out, last = [], 0
    for sg in segs:
        out.append(list(lps[last:last + len(sg)]))
        last += len(sg)
    assert last <= len(lps)
    return out


def _language_ids(model, gc, rq, chunks):
    """The request's languages as one id per row, or None (no language token): the named ids as they are; "auto" with
    a pass of its own (OWN_PASS) runs _detect on every (enc16, B, Tk) of `chunks` -- short-form: the call's encoder
    rows; long-form: each recording's raw first window -- and reads the ids back, one readback a chunk.  Beam search
    decodes one prompt, so rows detected as different languages raise NotImplementedError."""
    if rq.languages != AUTO:
        return rq.languages
    assert rq.detection == OWN_PASS
    langs = []
    for enc16, B, Tk in chunks:
        langs += _detect(model, gc, enc16, B, Tk)[0].tolist()
        del enc16
    if rq.num_beams > 1 and len(set(langs)) > 1:
        what = "recordings of this call have" if rq.long_form else "rows of this call were detected as"
        raise NotImplementedError(f"tw generate: beam search decodes one prompt for every clip; the {what} different "
                                  f"languages ({langs})")
    return langs


@torch.no_grad()
def generate(model, input_features=None, max_length=None, num_beams=1, return_timestamps=False, language=None,
             task=None, decoder_input_ids=None, max_new_tokens=None, encoder_outputs=None, attention_mask=None,
             use_graph=None, prompt_ids=None, prompt_condition_type=None, assistant_model=None,
             num_assistant_tokens=None, return_language=False, **kw):
    """HF WhisperGenerationMixin.generate (transformers 5.15 generation_whisper.py), the calls the reference makes.
    prompt_ids (run_eval.py:656-657 --prompt_text): 1-D ids from get_prompt_ids (<|startofprev|> + text), placed in
    front of the task prompt of every decoded window (_prepare_decoder_input_ids; with the default
    prompt_condition_type "first-segment" and no conditioning on previous text, HF puts it in front of each window of a
    long-form input, not only the first); the begin indices of the suppress / timestamp processors and the length cap
    count it; the returned ids do not contain it.
    assistant_model (run_eval.py:524-545 --assistant_model_name_or_path, passed at :653-654): assisted (speculative)
    greedy decoding of a single input -- a tw WhisperForConditionalGeneration with its own encoder, or a
    WhisperForCausalLM decoding over this model's encoder output (the distilled student with the shared frozen
    encoder); it drafts num_assistant_tokens tokens a round (default DEFAULT_ASSISTANT_TOKENS, at most
    MAX_ASSISTANT_TOKENS; HF's default and schedule differ) and this model verifies them in one pass (_SpecDecoder).
    The ids are those of the same call without an assistant.
    repetition_penalty / no_repeat_ngram_size (HF generate's, faster-whisper transcribe's): HF's
    RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor on the raw fp32 scores of every generated step,
    before the suppress / timestamp rules, the log-prob of the fallback gate and sampling; the history is the whole
    decoder row (left padding, <|startofprev|> text and task prompt included).  Defaults come from generation_config
    when it names them.  Greedy and long-form (fallback, condition_on_prev_tokens) decoding take them; beam search and
    assisted decoding raise NotImplementedError.  Any keyword that is not implemented raises TypeError.
    language: None -- no language token in the prompt (NOT HF's meaning: HF's language=None detects; here that is
    language="auto"); a name, code, token or id for every row; a list / tuple with one of those per row (HF's
    language=[...]; a length other than the batch size is HF's ValueError, a None element HF's TypeError);
    "auto" -- every row's language is detected as HF detect_language does (the largest language logit after
    <|startoftranscript|> on the first 30 s) and, as in HF, no task token follows unless `task` is passed.
    "auto" needs generation_config.lang_to_id and excludes decoder_input_ids (ValueError).  Short-form greedy
    decoding without prompt_ids detects inside the prompt prefill, on the device (_PromptedDecode._prefill: no
    second pass, no host read); every other form -- prompt_ids, beam search, assisted and long-form decoding, the
    latter once per call on each recording's first 3000 raw frames -- runs detect_language's step first and reads
    the B ids back.  Beam search decodes one prompt, so rows of different languages raise NotImplementedError.
    return_language=True returns (ids, language ids int64 [B] on the device) for any language form but None (there is
    no language to return: ValueError).  With decoder_input_ids the caller owns the prompt: `language` is not looked
    at, as before, and return_language raises ValueError.
    return_token_logprobs=True (a keyword of the planner, through **kw): returns (ids, logprobs), or (ids, languages,
    logprobs) with return_language.  logprobs: fp32 on the ids' device, the ids' shape; element [b, j] is the log-prob
    of ids[b, j] under the log-softmax of the processed scores of its step -- after the repeat processors, the
    suppress masks and the timestamp rules, at temperature 1 (HF's _retrieve_avg_logprobs convention: what
    compute_transition_scores gives on the processed scores) -- as the selection kernel computed it, and 0.0 where the
    engine selected nothing: after a row's eos and in the padding between rows.  Long-form: a token carries the
    value of the attempt that was kept.  It forces the tracking selection kernels (argmax at 1/T = 0: the ids do not
    change); with num_beams > 1 it raises NotImplementedError."""
    gc = _resolve_gc(model)
    hidden = _unwrap(encoder_outputs)
    given = hidden if hidden is not None else input_features
    rq = plan_generate(model.config, gc, rows=given.shape[0] if given is not None else 0,
                       frames=input_features.shape[-1] if input_features is not None else None,
                       have_features=input_features is not None, have_encoder_outputs=encoder_outputs is not None,
                       max_length=max_length, num_beams=num_beams, return_timestamps=return_timestamps,
                       language=language, task=task, decoder_input_ids=decoder_input_ids, max_new_tokens=max_new_tokens,
                       use_graph=use_graph, prompt_ids=prompt_ids, prompt_condition_type=prompt_condition_type,
                       assistant_model=assistant_model, num_assistant_tokens=num_assistant_tokens,
                       return_language=return_language, **kw)
    if rq.long_form:
        return _longform(model, gc, rq, input_features, attention_mask)
    cfg, dev = model.config, model.device
    enc16, B, Tk = _encoder_rows(model, input_features, hidden)
    # detection fused into the decode (PREFILL): the prefill's step at column 0 is the detection step, so column 1 of
    # the prompt holds a placeholder language until the device writes the detected one there; the decoder is handed
    # the id table and its id matrix is read afterwards
    fused = rq.detection == PREFILL
    detect = lang_out = None
    if rq.decoder_input_ids is not None:
        prompt = torch.as_tensor(rq.decoder_input_ids, dtype=torch.int64)
        if prompt.dim() == 1:
            prompt = prompt[None].repeat(B, 1)
    else:
        if fused:
            table = language_table(gc, cfg.vocab_size)
            detect = torch.tensor(table, dtype=torch.int32, device=dev)
            langs = [table[0]] * B
        else:
            langs = _language_ids(model, gc, rq, [(enc16, B, Tk)])
        prompt = torch.tensor([list(rq.prompt_ids or ()) + build_prompt(gc, lid, rq.task, rq.timestamps,
                                                                         detected=rq.detected)
                               for lid in (langs if langs is not None else [None] * B)], dtype=torch.int64)
        if rq.return_language and not fused:
            lang_out = torch.tensor(langs, dtype=torch.int64, device=dev)
    P = prompt.shape[1]
    ml = total_length(cfg, gc, P, rq.max_length, rq.max_new_tokens)
    want_lp = rq.return_token_logprobs
    lpkw = dict(logp=True) if want_lp else {}        # off: the decoders are built and run as before
    if P >= ml:
        # nothing is decoded, so there is no prefill to detect in: the languages, when asked for, take their own pass
        if fused and rq.return_language:
            lang_out = _detect(model, gc, enc16, B, Tk)[0]
        out = torch.empty(B, 0, dtype=torch.int64, device=dev)
    elif rq.decoder == ASSISTED:
        if B != 1:
            raise ValueError("tw generate: assisted decoding takes a single input (batch size 1), as HF's does")
        enc_a = assistant_encoder(rq.assistant, model, enc16, input_features)
        dec = _SpecDecoder(model, rq.assistant, gc, Tk, P, ml, rq.timestamps, rq.use_graph, k=rq.k, **lpkw)
        if rq.keep is not None:
            rq.keep.append(dec)
        out = dec.run(enc16, prompt.to(dev), enc_a=enc_a)
        if rq.trace is not None:
            rq.trace.append(dict(accepted=list(dec.accepted), num_assistant_tokens=dec.k))
    elif rq.decoder == BEAM:
        if not bool((prompt == prompt[:1]).all()):
            raise NotImplementedError("tw generate: beam search takes one prompt for every clip")
        out = _BeamDecoder(model, gc, B, rq.num_beams, Tk, P, ml).run(enc16, prompt[0])
    else:
        dec = _Decoder(model, gc, B, Tk, P, ml, rq.timestamps, rq.use_graph, repetition_penalty=rq.repetition_penalty,
                       no_repeat_ngram_size=rq.no_repeat_ngram_size, **lpkw)
        if rq.keep is not None:              # tests: the decoder (and its device caches) outlive the call
            rq.keep.append(dec)
        out = dec.run(enc16, prompt.to(dev), **(dict(detect=detect) if fused else {}))
        if fused and rq.return_language:
            lang_out = dec.sel.ids[:, 1].clone()
    if want_lp:        # a decoder built with logp returns (ids, log-probs); nothing decoded: no columns
        out, lps = out if isinstance(out, tuple) else (out, torch.zeros(B, 0, dtype=torch.float32, device=dev))
        return (out, lang_out, lps.clone()) if rq.return_language else (out, lps.clone())
    return (out, lang_out) if rq.return_language else out


def assistant_encoder(assistant, model, enc16, input_features):
    """The assistant's encoder rows for one window: a decoder-only assistant (WhisperForCausalLM) takes the
    target's, cast to its own activation dtype; any other runs its own encoder on the same features."""
    if getattr(assistant, "decoder_only", False):
        return enc16 if enc16.dtype == assistant.act_dtype else enc16.to(assistant.act_dtype)
    if input_features is None:
        raise ValueError("tw generate: an assistant with its own encoder needs input_features (encoder_outputs are "
                         "the target's)")
    return assistant.encode(assistant.conv_input(input_features))


def batch_rows_independent(model):
    """True where each row of a decode batch of <= 8 rows is bit-identical to its batch-1 decode: on the 16-bit
    compute paths every decode-step Linear is a per-row GEMV (d % 256 == 0) or the skinny GEMM, whose K order per
    output does not depend on the batch (no split-K at <= 32 rows); tests/test_fallback_gpu.py runs the skinny
    form (micro, d = 128).  The fp32 path's GEMMs are not shown row-independent, so it decodes one at a time."""
    return model.compute in ("bf16", "fp16")


def row_tokens(raw, eos):
    """One row of a decoded batch as its own batch-1 decode returns it: up to and including its first eos."""
    raw = list(raw)
    return raw[:raw.index(eos) + 1] if eos in raw else raw


def compression_ratio(tokens, vocab_size):
    """HF _retrieve_compression_ratio (generation_whisper.py:1949-1956): raw token bytes (little-endian,
    int(log2(V)/8)+1 bytes each) over their zlib-compressed length."""
    import math
    import zlib
    n = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(n, "little") for t in tokens)
    return len(raw) / len(zlib.compress(raw))


def need_fallback(tokens, avg_logprob, no_speech_prob, vocab_size, compression_ratio_threshold=None,
                  logprob_threshold=None, no_speech_threshold=None):
    """HF _need_fallback (generation_whisper.py:1243-1290) -> (needs_fallback, should_skip)."""
    needs, skip = False, False
    if compression_ratio_threshold is not None and compression_ratio(tokens, vocab_size) > compression_ratio_threshold:
        needs = True
    if logprob_threshold is not None and avg_logprob < logprob_threshold:
        needs = True
    if no_speech_threshold is not None and logprob_threshold is not None:
        if avg_logprob < logprob_threshold and no_speech_prob > no_speech_threshold:
            needs, skip = False, True
    return needs, skip


def _bucket(n):
    """Decode-batch size for n rows: the next power of two up to 8 (the GEMV regime: one launch per Linear whatever the
    rows), then the next multiple of 8; the extra rows repeat the first one and are dropped.  A shrinking batch --
    recordings finishing, fewer rows falling back -- then reuses a captured step."""
    if n > 8:
        return (n + 7) // 8 * 8
    b = 1
    while b < n:
        b *= 2
    return b


def previous_text(segments, ts_begin):
    """The tokens of a recording's accepted segments as HF conditions on them (_pad_to_max_length with
    skip_ending_double_timestamps): a segment that closes on a timestamp pair loses its last timestamp."""
    prev = []
    for st in segments:
        prev.extend(st[:-1] if len(st) > 2 and st[-2] >= ts_begin else st)
    return prev


def conditioned_prompts(init, segments, cond_on, conditioned, prev_sot, cut_off, ts_begin, inits=None):
    """The decoder prompts of one seek iteration of the batched long-form loop (HF _prepare_decoder_input_ids):
    segments / cond_on hold, per active row, its accepted segments and whether it conditions on them.  Not
    `conditioned`: every row takes init.  Otherwise row r takes <|startofprev|> (prev_sot, when the model has one) +
    the last cut_off tokens of its previous text (only when cond_on[r] and it has segments) + init.
    inits: one init per row in place of `init` (rows of different languages: equal lengths, another language token).
    -> (unpadded prompts, the length they are left-padded to)."""
    inits = [init] * len(segments) if inits is None else inits
    assert len(inits) == len(segments) and len({len(i) for i in inits}) <= 1
    if not conditioned:
        return [list(i) for i in inits], len(inits[0]) if inits else len(init)
    head = [int(prev_sot)] if prev_sot is not None else []
    out = []
    for sg, on, ini in zip(segments, cond_on, inits):
        prev = previous_text(sg, ts_begin)[-cut_off:] if on and sg else []
        out.append(head + prev + list(ini))
    return out, max(len(p) for p in out)


def trim_pads(seq, pad, eos):
    """seq without its trailing pads, as HF removes them (pad == eos keeps one eos)."""
    seq = list(seq)
    if seq and seq[-1] == pad:
        k = len(seq)
        while k > 1 and seq[k - 2] == pad:
            k -= 1
        seq = seq[:k] if pad == eos else seq[:k - 1]
    return seq


@dataclasses.dataclass
class _LongForm:
    """The constants of one long-form call, its decoder cache and the seek loop (`run`, once per group of recordings):
    HF's batched sequential long-form (generation_whisper.py:785-898 with generate_with_fallback :970-1117).  The
    recordings of a group stay in ONE batch window after window: each seek iteration cuts the current 30 s window of
    every unfinished recording at its own seek (_get_input_segment, zero-padded), encodes and decodes them together,
    and a recording whose seek reaches its length leaves the batch (_maybe_reduce_batch).  The rows whose attempt
    fails HF's gate (compression ratio of the token bytes, average log-prob of the processed scores; no-speech
    probability at <|startoftranscript|> -> the window is skipped) are decoded again at the next temperature,
    together; a row is accepted at its first passing attempt (or keeps its last one).  HF's own rows are not
    batch-invariant either, so parity is with HF's batched call (tests/test_batched_longform_gpu.py).
    Speculative fallback (fallback_batch, where batch_rows_independent): while the failing rows are few, several
    temperature levels of them decode as one batch of at most 8 rows (<= 8 rows is one GEMV launch per Linear,
    latency-bound: extra rows are nearly free); a row's attempt decodes the same tokens whichever batch it sits in
    (per-row temperature and seed, tw_select_sample_ts), so the result is the level-by-level one.
    cond (condition_on_prev_tokens): every active row builds its own prompt -- <|startofprev|> + the last cut_off
    tokens of its accepted segments + the task prompt, conditioned only after a window accepted at temperature < 0.5
    -- and the rows are left-padded with pad to the longest prompt of the iteration (HF _prepare_decoder_input_ids /
    _pad_to_max_length; HF's length cap counts the padded length); every row embeds at its column index, as
    transformers 5.15 does, so a padded row is HF's row, not the decode of its unpadded prompt.  As in HF, the
    conditioned form starts once the group's first recording has a segment, and from then on a row without previous
    text carries <|startofprev|> alone (no <|startofprev|> id: the rows condition without it).
    init: per recording of the call, prompt_ids + task prompt, the unconditioned prompt (the recordings' language
    tokens may differ, the lengths do not); n_task: the length of its task part.  An assisted request (one recording):
    the temperature-0 attempt of each window is assisted (_SpecDecoder).  The fields are the request and what is
    derived from it once per call; the request's own settings are read from rq."""
    model: object
    gc: object
    rq: Request
    eos: int
    pad: int
    ts_begin: int
    ns_token: int
    prev_sot: int
    cut_off: int
    init: list
    n_task: int
    enc_rows: int = 32              # windows per encoder call (bounds the encoder's activations)
    decoders: dict = dataclasses.field(default_factory=dict)

    def decoder(self, P, ml, nb=1, spec=False):
        # the two repeat options and the models' cross-attention K/V and decode weight formats are baked into a
        # captured step
        key = (P, ml, nb, spec, self.rq.repetition_penalty, self.rq.no_repeat_ngram_size,
               getattr(self.model, "cross_kv_dtype", None), getattr(self.rq.assistant, "cross_kv_dtype", None),
               getattr(self.model, "decode_weight_dtype", None),
               getattr(self.rq.assistant, "decode_weight_dtype", None),
               self.rq.return_token_logprobs)
        if key in self.decoders:
            self.decoders[key] = self.decoders.pop(key)      # most recently used last
        else:
            # each decoder holds a captured step and the cross-attention K/V of its rows (246 MB per row at
            # large-v2): keep the three most recently used
            while len(self.decoders) >= 3:
                self.decoders.pop(next(iter(self.decoders)))
            m, Tk = self.model, self.model.config.max_source_positions
            lpkw = dict(logp=True) if self.rq.return_token_logprobs else {}
            if spec:
                self.decoders[key] = _SpecDecoder(m, self.rq.assistant, self.gc, Tk, P, ml, True, self.rq.use_graph,
                                                  self.rq.track, k=self.rq.k, **lpkw)
            else:
                self.decoders[key] = _Decoder(m, self.gc, nb, Tk, P, ml, True, self.rq.use_graph, self.rq.track,
                                              repetition_penalty=self.rq.repetition_penalty,
                                              no_repeat_ngram_size=self.rq.no_repeat_ngram_size, **lpkw)
        return self.decoders[key]

    def seeds(self, b, nwin):
        """One seed per temperature level for window nwin of recording b (its index in the call)."""
        return [(self.rq.seed * 1000003 + b * 7919 + nwin * 131 + fi) & ((1 << 63) - 1)
                for fi in range(len(self.rq.temps))]

    # One attempt of the fallback ladder on the window state w (enc, enc_a, prompts, P, ml, ns, seeds, padded) ->
    # (raw tokens per attempt, gate(r, n) -> (avg_logprob over n tokens, no_speech_prob) of row r, read back only when
    # the row is gated, decode batch, accepted drafts per round or None, the log-prob of every raw token per attempt
    # or None without return_token_logprobs)
    def decode_rows(self, w, attempts):
        """`attempts` [(recording, level)] as one batch of _bucket rows, each with its own temperature and seed; rows
        of one window share its encoder rows (K/V projected once).  A group of several conditioned recordings passes
        the rows' pad counts in every iteration, all zeros included, so a decoder's captured step is not dropped when
        equal and unequal prompt lengths alternate; a group of one has no padding and makes the plain calls."""
        nb = _bucket(len(attempts))
        rows = attempts + [attempts[0]] * (nb - len(attempts))
        b0 = rows[0][0]
        e16 = w.enc[b0] if len({b for b, _ in rows}) == 1 else torch.cat([w.enc[b] for b, _ in rows])
        tl = [self.rq.temps[f] or 0.0 for _, f in rows]
        sl = [w.seeds[b][f] for b, f in rows]
        assisted = self.rq.decoder == ASSISTED and nb == 1 and not tl[0]
        dec = self.decoder(w.P, w.ml, nb, spec=assisted)
        pads = [w.P - len(w.prompts[b]) for b, _ in rows]
        prompt = torch.tensor([[self.pad] * n + w.prompts[b] for n, (b, _) in zip(pads, rows)], dtype=torch.int64,
                              device=self.model.device)
        kw = dict(temperature=tl if nb > 1 else tl[0], seed=sl if nb > 1 else sl[0], no_speech=w.ns)
        if w.padded:
            kw["pads"] = pads
        if assisted:
            kw["enc_a"] = w.enc_a[b0]
        # a batch is cut at its LAST row's first eos: each row is cut at its own first eos, what its own decode returns
        out = dec.run(e16, prompt, **kw)
        ids, lpm = out if self.rq.return_token_logprobs else (out, None)
        raws = [row_tokens(r, self.eos) for r in ids.tolist()[:len(attempts)]]
        lps = None if lpm is None else [lp[:len(raw)] for lp, raw in zip(lpm.tolist(), raws)]

        def gate(r, n):
            return (float(dec.sel.sum_logp[r]) / n if self.rq.track else 0.0,
                    float(torch.exp(dec.ns_logp[r])) if w.ns is not None else 0.0)
        return raws, gate, nb, list(dec.accepted) if assisted else None, lps

    def decode_beam(self, w, b):
        """HF generate_with_fallback at temperature 0 with num_beams > 1: a beam search over recording b's window
        (_BeamDecoder with the timestamp rules; its gate values from the chosen hypothesis's per-step processed
        scores).  One row, always gated."""
        gc = self.gc
        beam_ts = (self.ts_begin, int(gc.no_timestamps_token_id),
                   gc.max_initial_timestamp_index if "max_initial_timestamp_index" in gc else None)
        bd = _BeamDecoder(self.model, gc, 1, self.rq.num_beams, self.model.config.max_source_positions, w.P, w.ml,
                          timestamps=beam_ts)
        raw = row_tokens(bd.run(w.enc[b], w.prompts[b], no_speech=w.ns)[0].tolist(), self.eos)

        def gate(r, n):
            return float(bd.sum_logp[0]) / n, float(bd.ns_prob[0]) if w.ns is not None else 0.0
        return [raw], gate, 1, None, None

    def run(self, feats, lens, recs):
        """The seek loop over the recordings `recs` (their indices in the call) -> ({recording: its tokens},
        {recording: their log-probs} -- with return_token_logprobs; every cut of an attempt's tokens below cuts its
        log-probs at the same indices, so a token keeps the value of the attempt that was kept)."""
        model, rq, eos, pad = self.model, self.rq, self.eos, self.pad
        temps, trace, cond = rq.temps, rq.trace, rq.condition_on_prev_tokens
        window = 2 * model.config.max_source_positions            # 3000 feature frames = 30 s
        dev, nmel, V = model.device, feats.shape[1], model.config.vocab_size
        spec = rq.fallback_batch and batch_rows_independent(model)
        # a beam search at temperature 0 later in the schedule decodes alone: the levels are taken one at a time
        one_level = rq.num_beams > 1 and any(not t for t in temps[1:])
        assert rq.num_beams == 1 or len(recs) == 1
        seek = {b: 0 for b in recs}
        nwin = {b: 0 for b in recs}
        outs = {b: [] for b in recs}
        out_lps = {b: [] for b in recs}
        segments = {b: [] for b in recs}         # accepted segments per recording (the previous text)
        cond_on = {b: cond for b in recs}
        while True:
            active = [b for b in recs if seek[b] < int(lens[b])]          # _maybe_reduce_batch
            if not active:
                break
            nfr = {b: min(window, int(lens[b]) - seek[b]) for b in active}
            prompts, P = conditioned_prompts(None, [segments[b] for b in active], [cond_on[b] for b in active],
                                             any(cond_on.values()) and len(segments[recs[0]]) > 0, self.prev_sot,
                                             self.cut_off, self.ts_begin, inits=[self.init[b] for b in active])
            ml = total_length(model.config, self.gc, P, rq.max_length, rq.max_new_tokens)
            if P >= ml:
                raise ValueError(f"prompt of {P} tokens leaves no room below max_length {ml}")
            w = types.SimpleNamespace(enc={}, enc_a={}, prompts=dict(zip(active, prompts)), P=P, ml=ml,
                                      ns=(P - self.n_task, self.ns_token) if rq.no_speech_threshold is not None
                                      else None, seeds={b: self.seeds(b, nwin[b]) for b in active},
                                      padded=cond and len(recs) > 1)
            # encode the current windows together (chunks of enc_rows)
            for c0 in range(0, len(active), self.enc_rows):
                rows = active[c0:c0 + self.enc_rows]
                segb = torch.zeros(len(rows), nmel, window, dtype=torch.float32, device=dev)
                for i, b in enumerate(rows):
                    segb[i, :, :nfr[b]] = feats[b, :, seek[b]:seek[b] + nfr[b]]
                e = model.encode(model.conv_input(segb))
                tk = e.shape[0] // len(rows)
                for i, b in enumerate(rows):
                    w.enc[b] = e[i * tk:(i + 1) * tk]
                if rq.decoder == ASSISTED:          # one recording: the assistant's rows for the same window
                    w.enc_a[rows[0]] = assistant_encoder(rq.assistant, model, w.enc[rows[0]], segb)
                del segb
            result = {}                       # b -> (last attempt's tokens, skip, its temperature)
            pending = list(active)
            level = 0
            while pending and level < len(temps):
                per = max(1, 8 // len(pending)) if spec and level > 0 and not one_level else 1
                levels = list(range(level, min(len(temps), level + per)))
                attempts = [(b, f) for f in levels for b in pending]
                beam = rq.num_beams > 1 and len(levels) == 1 and not temps[level]
                raws, gate, batch, accepted, lps = (self.decode_beam(w, pending[0]) if beam
                                                    else self.decode_rows(w, attempts))
                decided = set()
                for r, (b, f) in enumerate(attempts):
                    if b in decided:
                        continue                                  # accepted at a lower temperature of this batch
                    raw = raws[r]
                    needs, skip = False, False
                    rec = dict(b=b, seek=seek[b], n=nfr[b], T=temps[f], prompt=list(w.prompts[b]), raw=list(raw))
                    if rq.track or rq.compression_ratio_threshold is not None or beam:
                        tg = time.perf_counter()      # gate cost: log-prob / no-speech readback + compression ratio
                        cand = trim_pads(raw, pad, eos)
                        avg, nsp = gate(r, max(len(cand), 1))
                        needs, skip = need_fallback(cand, avg, nsp, V, rq.compression_ratio_threshold,
                                                    rq.logprob_threshold, rq.no_speech_threshold)
                        rec.update(avg_logprob=avg, no_speech_prob=nsp, needs_fallback=needs, skip=skip, batch=batch,
                                   gate_ms=(time.perf_counter() - tg) * 1e3)
                    else:
                        rec["batch"] = batch
                    if accepted is not None:
                        rec["accepted"] = accepted
                    if lps is not None:
                        rec["token_logprobs"] = list(lps[r])          # one per token of `raw`
                    if trace is not None:
                        trace.append(rec)
                    result[b] = (raw, skip, temps[f], lps[r] if lps is not None else None)
                    if not needs:
                        decided.add(b)
                pending = [b for b in pending if b not in decided]
                level = levels[-1] + 1
            del w
            for b in active:
                seq, skip, t_acc, lp = result[b]
                n = nfr[b]
                nwin[b] += 1
                cond_on[b] = cond and (t_acc is None or t_acc < 0.5)
                if not skip:
                    if seek[b] + window < int(lens[b]) and seq and seq[-1] == eos:    # not the last window: cut its eos
                        seq = seq[:-1]
                    seq = trim_pads(seq, pad, eos)
                if skip or not seq:
                    seek[b] += n
                    continue
                segs, off = retrieve_segment(seq, n, self.ts_begin)
                for sgm in segs:
                    outs[b].extend(sgm)
                    if cond:
                        segments[b].append(list(sgm))
                if lp is not None:                        # seq is a prefix of the attempt's tokens
                    for sl in segment_logprobs(lp[:len(seq)], segs):
                        out_lps[b].extend(sl)
                seek[b] += off if off > 0 else n          # a closing <|0.00|> pair would not advance: take the window
        return outs, out_lps


def _longform(model, gc, rq, feats, attention_mask):
    """HF sequential long-form generate (generation_whisper.py step 6): per input, 30 s windows from `seek`, decoded
    with the timestamp rules and HF's temperature fallback; trailing eos/pad trimmed, segments split at consecutive
    timestamps, seek advanced by the last timestamp (or the whole window on a single-timestamp ending).  Returns the
    concatenated segment tokens, right-padded with pad.  Sampled attempts draw from softmax(x / T) with the engine's
    counter-based RNG (seeded by `seed`, the recording, the window and the fallback index), not torch's RNG stream.
    One seek loop (_LongForm.run) serves every form.  num_beams == 1: the recordings of the call are one group and
    decode as one batch.  num_beams > 1 (run_eval.py --num_beams with timestamps / long-form): every recording is a
    group of its own, in recording order, so each window is encoded alone (the encoder's output depends on the batch
    it runs in); a temperature-0 attempt is a beam search over the window, a sampled attempt keeps one beam.
    rq: the call's Request.  Its languages give every recording its own task prompt for all of its windows; "auto"
    detects once per call, as HF does, on the first 3000 raw frames of every recording (HF's
    input_features[:, :, :3000], not the zero-filled window the seek loop cuts), enc_rows recordings at a time.
    rq.return_language: -> (ids, language ids int64 [B]); rq.return_token_logprobs: the ids' log-probs last."""
    cfg = model.config
    feats = feats.to(model.device, torch.float32)
    B, _, T = feats.shape
    lens = attention_mask.sum(-1).tolist() if attention_mask is not None else [T] * B

    def first_windows():
        for c0 in range(0, B, _LongForm.enc_rows):
            e = model.encode(model.conv_input(_first_window(model, feats[c0:c0 + _LongForm.enc_rows])))
            n = min(B, c0 + _LongForm.enc_rows) - c0
            yield e, n, e.shape[0] // n
            del e                             # before the next chunk is encoded
    langs = _language_ids(model, gc, rq, first_windows())
    task_inits = [build_prompt(gc, lid, rq.task, True, detected=rq.detected)
                  for lid in (langs if langs is not None else [None] * B)]
    eos, pad = int(gc.eos_token_id), int(gc.pad_token_id if gc.pad_token_id is not None else gc.eos_token_id)
    prev_sot = gc_get(gc, "prev_sot_token_id")
    if prev_sot is None:
        sup = list(gc.suppress_tokens or [])
        prev_sot = sup[-2] if len(sup) >= 2 else None
    lf = _LongForm(model=model, gc=gc, rq=rq, eos=eos, pad=pad, ts_begin=int(gc.no_timestamps_token_id) + 1,
                   ns_token=int(gc.no_timestamps_token_id) - 1, prev_sot=prev_sot,
                   cut_off=cfg.max_target_positions // 2 - 1,
                   # prompt_ids: in front of every window's task prompt
                   init=[list(rq.prompt_ids or ()) + t for t in task_inits],
                   n_task=len(task_inits[0]) if task_inits else 0)
    outs, out_lps = {}, {}
    for recs in ([list(range(B))] if rq.num_beams == 1 else [[b] for b in range(B)]):
        o, l = lf.run(feats, lens, recs)
        outs.update(o)
        out_lps.update(l)
    L = max((len(o) for o in outs.values()), default=0)
    res = torch.full((B, L), pad, dtype=torch.int64)
    for b, o in outs.items():
        res[b, :len(o)] = torch.tensor(o, dtype=torch.int64)
    ret = [res.to(model.device)]
    if rq.return_language:
        ret.append(torch.tensor(langs, dtype=torch.int64, device=model.device))
    if rq.return_token_logprobs:            # the ids' shape; 0 in the padding between rows
        lps = torch.zeros(B, L, dtype=torch.float32)
        for b, l in out_lps.items():
            lps[b, :len(l)] = torch.tensor(l, dtype=torch.float32)
        ret.append(lps.to(model.device))
    return tuple(ret) if len(ret) > 1 else ret[0]
