"""The 8-bit decoder weight format (include/tw_hip.h, decode_weight_dtype="fp8_e4m3") restated in torch on the CPU,
and what the tests of it share.

quantise_rows_ref: the K/V format's restatement (xkv_fp8_cases.quantise_ref) with "block" = one weight row: per row
of K 16-bit values, scale = 2^e with e the smallest integer such that absmax * 2^-e <= 448 (clamped to [-100, 100]; 1
for an all-zero row; NaN for a row with a non-finite value), bytes = RNE_e4m3fn(x * 2^-e).  RefW8: the oracle model
whose decoder-layer Linear weights (fused self-attention q/k/v, self out-proj, cross q-proj, cross out-proj, fc1, fc2)
and LM head are replaced by their dequantised values; embedding lookups stay on the original table.
"""
import torch

import xkv_fp8_cases as xc
from oracle.weights import CONFIGS, make_weights
from oracle.whisper_ref import Ref, to_torch

MARGIN = xc.MARGIN          # 0.05, tests/test_decode_gpu.py's margin of the 16-bit engine against Ref
# The margin of the fp8 engine against RefW8 on DECODE_CFG (tests/test_w8_decode_gpu.py).  The rule: the same
# teacher-forced check with the setting OFF against plain Ref on this config is the control; if its worst gap is
# within MARGIN the fp8 margin is MARGIN, else twice the control's worst gap.  Measured control gaps on an MI355X
# (the parent's code path; the test recomputes them every run): 0.0000 for the bf16 model and for the fp16 model, at
# B = 3 and at B = 9 -- within MARGIN, so the fp8 margin is:
W8_MARGIN = MARGIN
CONTROL_GAPS = {"bf16": 0.0, "fp16": 0.0}

# the smallest config whose decode step takes the GEMV path (d_model % 256 == 0), as
# tests/test_assisted_gpu.py::test_gemv_verify_pass builds it
DECODE_CFG = dict(CONFIGS["micro"], d_model=256, encoder_attention_heads=4, decoder_attention_heads=4,
                  encoder_ffn_dim=512, decoder_ffn_dim=512)
DECODE_SEED, DECODE_LIN_STD = 3, 0.15

# the decoder-layer Linear weights the format covers, by their suffix under model.decoder.layers.<i>
LAYER_WEIGHTS = (".self_attn.q_proj.weight", ".self_attn.k_proj.weight", ".self_attn.v_proj.weight",
                 ".self_attn.out_proj.weight", ".encoder_attn.q_proj.weight", ".encoder_attn.out_proj.weight",
                 ".fc1.weight", ".fc2.weight")
HEAD = "model.decoder.embed_tokens.weight"


def quantise_rows_ref(W16):
    """W16 [N, K] bf16 / fp16 -> (e4m3fn values [N, K], fp32 scales [N])."""
    N, K = W16.shape
    blk = W16.reshape(N, K // 64, 64) if K % 64 == 0 else W16.reshape(N, 1, K)
    q, s = xc.quantise_ref(blk)
    return q.reshape(N, K), s


def dequantise_rows_ref(q, scale):
    """fp32 values of quantised rows (exact)."""
    return q.float() * scale[:, None]


def requantised(W, half):
    """A weight as the fp8 engine reads it: rounded to the 16-bit dtype, quantised per row, dequantised (fp32)."""
    return dequantise_rows_ref(*quantise_rows_ref(W.to(half)))


def weight_cases(N, K, dtype, seed):
    """A random [N, K] weight matrix of a 16-bit dtype with the format's edge cases planted in rows 1, 2, ... as far
    as N reaches (row 0 stays random): an all-zero row, a row whose absmax sits at mantissa 0.875 (the last that takes
    the smaller exponent), one just above it, a row with an inf, a row with a NaN, and (K >= 64) a row of
    xkv_fp8_cases.blocks: +-0, values on e4m3 ties after scaling, e4m3 subnormals.
    -> (W, rows) with rows = {kind: row index} of what was planted."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * 0.03
    rows = {}
    kinds = ["zero", "m0875", "above", "inf", "nan"] + (["ties"] if K >= 64 else [])
    for i, kind in enumerate(kinds):
        r = i + 1
        if r >= N:
            break
        rows[kind] = r
        if kind == "zero":
            W[r] = 0.0
            W[r, 1] = -0.0
        elif kind in ("m0875", "above"):
            W[r].clamp_(-1.0, 1.0)
            W[r, K // 2] = 3.5 if kind == "m0875" else 3.5 + 2.0 ** -6
        elif kind == "inf":
            W[r, K - 1] = float("-inf")
        elif kind == "nan":
            W[r, 0] = float("nan")
        else:
            n = K // 64 * 64
            W[r, :n] = xc.blocks(1, 1, n // 64, dtype, seed).float().reshape(-1)
            W[r, n:].clamp_(-1.0, 1.0)
    return W.to(dtype), rows


def finite_rows(rows, N):
    """Boolean mask [N] of the rows weight_cases left finite."""
    ok = torch.ones(N, dtype=torch.bool)
    for kind in ("inf", "nan"):
        if kind in rows:
            ok[rows[kind]] = False
    return ok


class RefW8(Ref):
    """oracle.whisper_ref.Ref over parameters whose covered decoder weights are replaced by their dequantised values;
    logits() uses the dequantised head, the embedding lookups the original table."""

    def __init__(self, cfg, params, half=torch.bfloat16, **kw):
        p = dict(params)
        for i in range(cfg["decoder_layers"]):
            for n in LAYER_WEIGHTS:
                key = f"model.decoder.layers.{i}{n}"
                p[key] = requantised(p[key], half)
        super().__init__(cfg, p, half=half, **kw)
        self.head = requantised(params[HEAD], half)

    def logits(self, hdec):
        return self.lin(hdec, self.head).float()


# ---------------------------------------------------------------------------------------------- the decode models
MODES = {            # engine parameter dtype, oracle parameter dtype, Ref keywords
    "bf16": (torch.bfloat16, torch.bfloat16, dict(amp=True, stream_bf16=True)),
    "fp16": (torch.float16, torch.float16, dict(amp=True, stream_bf16=True, half=torch.float16)),
    "amp": (torch.float32, torch.float32, dict(amp=True)),          # fp32 master under bf16 autocast: no fused LN
}


def decode_weights():
    return make_weights(DECODE_CFG, DECODE_SEED, lin_std=DECODE_LIN_STD)


def decode_model(mode, device="cuda"):
    """The DECODE_CFG engine model of one of MODES."""
    from tw.config import WhisperConfig
    from tw.modeling import WhisperForConditionalGeneration
    sd = {k: torch.from_numpy(v) for k, v in decode_weights().items()}
    return WhisperForConditionalGeneration.from_state_dict(WhisperConfig(**DECODE_CFG), sd, dtype=MODES[mode][0],
                                                           device=device)


def decode_ref(mode, w8):
    """The oracle of decode_model(mode): RefW8 (the setting on) or Ref (off)."""
    _, pdt, kw = MODES[mode]
    return (RefW8 if w8 else Ref)(DECODE_CFG, to_torch(decode_weights(), pdt), **kw)


def worst_gap(ref, feats, reps, seq, P, sup, eos=50257, enc=None, tie_ulp=0.0):
    """The teacher-forced margin rule of tests/test_decode_gpu.py::test_generate_matches_autocast_oracle as a number:
    `ref` run along the engine's own sequences seq [B, P + L] (B = reps x the clips of feats, clip-major tiling as
    feats.repeat(reps, 1, 1)); at every live position (the row has not emitted eos before it) the gap between the
    best processed score and the engine's token's.  enc: ref.encoder(feats) when the caller has it already.
    tie_ulp: a gap of at most tie_ulp * |best score| counts as 0 (a tie at the logits' own resolution).
    -> the worst gap over all live positions (none is left out)."""
    gen = seq[:, P:]
    with torch.no_grad():
        enc = (ref.encoder(feats) if enc is None else enc).repeat(reps, 1, 1)
        lg = ref.logits(ref.decoder(seq[:, :-1], enc)).float()
    worst = 0.0
    for j in range(gen.shape[1]):
        live = torch.ones(seq.shape[0], dtype=torch.bool) if j == 0 else (gen[:, :j] != eos).all(1)
        row = lg[:, P - 1 + j].clone()
        row[:, sup] = -float("inf")
        if j == 0:
            row[:, [220, eos]] = -float("inf")
        gap = row.max(-1).values - row.gather(1, gen[:, j:j + 1])[:, 0]
        gap = torch.where(gap <= tie_ulp * row.max(-1).values.abs(), torch.zeros_like(gap), gap)
        if bool(live.any()):
            worst = max(worst, float(gap[live].max()))
    return worst
