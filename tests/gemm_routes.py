"""The host routing of tw_gemm_bf16 / tw_gemm_f16 restated in plain Python, and the shapes it is checked over.

`parent_route()` follows the routing as gemm_run() was written before plan_gemm() existed (csrc/gemm.hip at the commit
"LayerNorm, KL/CE, helper kernels: per-element parity tests"): one walk that mutates an integer tile code (128, 256,
2561 = 256x128 3-stage ring, 2562 = persistent, 2563 = 256x128 2-stage ring, 2564 = persistent + fp16 edge strips,
1284 = 128x128 4-stage ring) and leaves at the first route whose workspace it gets.  It is written from that function,
statement by statement, not from the planner, so tests/test_gemm_routes_cpu.py compares two independent texts.
Every operand is taken as 16-byte aligned (the tests plan with aligned stand-ins), so only the leading dimensions
decide the alignment conditions.
"""
import collections

F_BIAS, F_ROUND, F_GELU, F_RES, F_ACCUM, F_AUX_OUT, F_DGELU, F_CLAMP16 = 1, 2, 4, 8, 16, 32, 64, 128
TILE128, TILE256, TILE256x128, TILE256PP, NOSPLIT, TILE256x128_S2 = 256, 512, 1024, 2048, 16384, 262144
FORCED = TILE128 | TILE256 | TILE256x128 | TILE256PP

ROUTES = ("skinny", "skinny_splitk", "splitk_dw", "rounds_sk_tail", "rounds_dp_tail", "persistent",
          "persistent_edges", "t128", "t128_ring4", "t256", "t256x128_s3", "t256x128_s2")
EPI = ("generic", "store_bf16", "store_f32", "gelu", "gelu_aux", "res_bf16", "res_f32", "dgelu")

Call = collections.namedtuple("Call", "M N K a_trans b_trans H c16 flags res16 res_mod batch ldc ldr ldaux sC sR sAux")
Plan = collections.namedtuple("Plan", "route S m_dp split_tile group_m epi")


def call(M, N, K, *, a_trans=False, b_trans=False, H=False, c16=True, flags=0, res16=None, res_mod=0, batch=1,
         ldc=None, ldr=None, ldaux=None):
    """A call description: c16 = C in the 16-bit operand type (else fp32); res16 = None (no residual) / True / False;
    ld* default to N, batch strides to the dense M x N."""
    if res16 is not None:
        flags |= F_RES
    return Call(M, N, K, bool(a_trans), bool(b_trans), bool(H), bool(c16), flags, res16, res_mod, batch,
                N if ldc is None else ldc, N if ldr is None else ldr, N if ldaux is None else ldaux, M * N, M * N, M * N)


def pick_epilogue(c, batch=None):
    batch = c.batch if batch is None else batch
    f = c.flags & 0xff
    c8 = c.ldc % 8 == 0 and (batch == 1 or c.sC % 8 == 0)
    c4 = c.ldc % 4 == 0 and (batch == 1 or c.sC % 4 == 0)
    if (f & ~(F_BIAS | F_ROUND)) == 0:
        if c.c16 and c8:
            return "store_bf16"
        if not c.c16 and c4:
            return "store_f32"
        return "generic"
    x8 = c.ldaux % 8 == 0 and (batch == 1 or c.sAux % 8 == 0)
    if (f & ~(F_BIAS | F_AUX_OUT)) == (F_ROUND | F_GELU) and c.c16 and c8:
        if not f & F_AUX_OUT:
            return "gelu"
        return "gelu_aux" if x8 else "generic"
    if f == (F_ROUND | F_DGELU) and c.c16 and c8 and x8:
        return "dgelu"
    if (f & ~(F_BIAS | F_ROUND | F_CLAMP16)) == F_RES and c.res_mod == 0 and bool(c.res16) == c.c16:
        if c.c16 and c8 and c.ldr % 8 == 0 and (batch == 1 or c.sR % 8 == 0):
            return "res_bf16"
        if f & F_CLAMP16:
            return "generic"
        if not c.c16 and c4 and c.ldr % 4 == 0 and (batch == 1 or c.sR % 4 == 0):
            return "res_f32"
    return "generic"


def _cdiv(a, b):
    return (a + b - 1) // b


def splitk_factor(c, G, R=1.4):
    """-> (S, tile); S = 0: no split"""
    if not c.a_trans or not c.b_trans or c.batch != 1 or c.c16:
        return 0, 128
    if c.flags & ~(F_ROUND | F_ACCUM) & 0xff:
        return 0, 128
    if c.N & 3 or c.ldc & 3:
        return 0, 128
    tiles = _cdiv(c.M, 128) * _cdiv(c.N, 128)
    if tiles >= 512:
        return 0, 128
    slots = 2 * G
    tiles256 = _cdiv(c.M, 256) * _cdiv(c.N, 256)
    best_cost, best, tile = float(_cdiv(tiles, slots)) * 2.0 * c.K, 0, 128
    for S in range(2, 17):
        if c.K % S or c.K // S < 512:
            continue
        kc = float(c.K // S)
        c128 = float(_cdiv(tiles * S, slots)) * 2.0 * kc
        if c128 < best_cost:
            best_cost, best, tile = c128, S, 128
        if R > 0:
            c256 = float(_cdiv(tiles256 * S, G)) * 4.0 * kc / R
            if c256 < best_cost:
                best_cost, best, tile = c256, S, 256
    return best, tile


def sk_tail_plan(c, G):
    """-> (S, m_dp)"""
    if c.batch != 1 or c.res_mod != 0 or c.N & 3 or c.ldc & 3:
        return 0, 0
    tn, tm = _cdiv(c.N, 256), _cdiv(c.M, 256)
    T = tn * tm
    if T < G and c.M >= 256:
        best = 0
        for S in range(2, 17):
            if c.K % (64 * S) == 0 and T * S <= G and c.K // S >= 256:
                best = S
        return best, 0
    if T < G or T >= 4 * G:
        return 0, 0
    m_dp = (T // G) * G // tn
    tail = (tm - m_dp) * tn
    if tail <= 0 or m_dp <= 0:
        return 0, m_dp
    best = 0
    for S in range(2, 9):
        if c.K % (64 * S) == 0 and tail * S <= G and c.K // S >= 256:
            best = S
    return best, m_dp


def dp_tail_plan(c, G):
    """-> (ok, m_dp)"""
    if c.batch != 1 or c.res_mod != 0:
        return False, 0
    tn, tm = _cdiv(c.N, 256), _cdiv(c.M, 256)
    T = tn * tm
    if T < G or T >= 8 * G:
        return False, 0
    rest = T % G
    if rest == 0 or rest * 10 > G * 6:
        return False, 0
    m_dp = (T // G) * G // tn
    rows = c.M - m_dp * 256
    t128 = _cdiv(rows, 128) * _cdiv(c.N, 128)
    return (m_dp > 0 and rows > 0 and t128 <= G), m_dp


def skinny_row_blocks(M):
    return _cdiv(M, 64) if M > 64 else 1


def parent_route(c, cus=256, have_ws=True):
    """The route of call `c` on `cus` CUs; have_ws = False: splitk_workspace() returns null at every request."""
    M, N, K, batch, flags, H = c.M, c.N, c.K, c.batch, c.flags, c.H
    at, bt = c.a_trans, c.b_trans
    cus = max(cus, 8)
    G = cus & ~7                                            # pp_grid_cus()
    grouped = not at and not bt and batch == 1 and M >= 65536 and K <= 2048
    group_m = 8 if grouped else 1
    if (flags >> 24) & 15:
        group_m = (flags >> 24) & 15
    epi = pick_epilogue(c)

    def plan(route, S=0, m_dp=0, split_tile=0):
        return Plan(route, S, m_dp, split_tile, group_m, epi)

    t256 = _cdiv(M, 256) * _cdiv(N, 256) * batch
    tile = 256 if (t256 >= 1000 and K >= 256) else 128
    if not at and not bt and K >= 8192 and t256 >= G:
        tile = 256
    if not at and bt and K >= 8192 and t256 >= G // 2:
        tile = 256
    if not at and not bt and tile == 128 and K >= 1024:
        if t256 >= G and t256 * 100 >= _cdiv(t256, G) * G * 85:
            tile = 256
    if tile == 256 and not at and not bt:
        tile = 2562
    if flags & TILE128:
        tile = 128
    if flags & TILE256:
        tile = 256
    if flags & TILE256x128:
        tile = 2561
    if flags & TILE256PP:
        tile = 2562
    if H and tile == 2562 and (M % 256 or N % 256):
        edges = K % 64 == 0 and epi != "generic" and batch == 1 and c.res_mod == 0 and M >= 256 and N >= 256
        tile = 2564 if edges else 128
    if H and tile == 2562 and (K % 64 or epi == "generic"):
        tile = 128
    skinny = (not at and not bt and batch == 1 and M <= 128 and (N <= 4096 or (M <= 64 and N <= 8192))
              and not flags & FORCED)
    if skinny:
        nwg, nk = _cdiv(N, 16) * skinny_row_blocks(M), _cdiv(K, 32)
        S = min(_cdiv(512, nwg), nk // 4)
        if flags & NOSPLIT or M <= 32:
            S = 1
        if S > 1 and have_ws:
            return plan("skinny_splitk", S)
        return plan("skinny", 1)
    if not flags & (NOSPLIT | FORCED):
        S, sk_tile = splitk_factor(c, G)
        nbytes = S * M * N * 4
        if S > 0 and nbytes <= 1 << 30 and have_ws:
            return plan("splitk_dw", S, 0, sk_tile)
    if flags & TILE256x128_S2:
        tile = 2563
    no_plan = NOSPLIT | FORCED | TILE256x128_S2
    if not at and not bt and tile == 128 and K >= 3072 and not flags & no_plan:
        S, m_dp = sk_tail_plan(c, G)
        full = not H or (N % 256 == 0 and (M - m_dp * 256) % 256 == 0 and epi != "generic")
        if S > 0 and full and have_ws:
            return plan("rounds_sk_tail", S, m_dp)
    if not at and not bt and not flags & no_plan:
        ok, m_dp = dp_tail_plan(c, G)
        if ok and (not H or (N % 256 == 0 and K % 64 == 0 and epi != "generic")):
            return plan("rounds_dp_tail", 0, m_dp)
    if tile == 128 and not at and not bt and not flags & TILE128 and _cdiv(M, 128) * _cdiv(N, 128) * batch <= G:
        tile = 1284
    if tile == 2564:
        return plan("persistent_edges")
    # dispatch<H, AT, BT>
    if H and (at or bt):
        return plan("t256" if tile == 256 else "t128")
    if tile == 2562 and not at and not bt:
        return plan("persistent")
    return plan({1284: "t128_ring4", 256: "t256", 2561: "t256x128_s3", 2563: "t256x128_s2"}.get(tile, "t128"))


# ----------------------------------------------------------------------------- the shapes
def _model_shapes(d, ffn, vp, tokens):
    """(M, N, K) of every Linear / conv-as-GEMM forward product of a Whisper model at `tokens` rows."""
    out = set()
    for M in tokens:
        out |= {(M, 3 * d, d), (M, d, d), (M, 2 * d, d), (M, ffn, d), (M, d, ffn), (M, vp, d)}
    return out


def config_shapes():
    """Forward shapes of configurations c1..c5: c1 tiny <- tiny (B = 16), c2 small <- large-v2 (B = 32),
    c3 large-v2 with 2 decoder layers <- large-v2 (B = 64), c4 large-v2 batched greedy decode (512 clips), c5 large-v2
    long-form (one recording).  Encoder rows B x 1500, decoder rows B x 447, the conv stem as GEMMs (K = 3 x 80 and
    3 d), decode steps of B rows.  The other three layouts (dX, dW) are the same triples with operands transposed."""
    s = set()
    s |= _model_shapes(384, 1536, 51904, (16 * 1500, 16 * 447)) | {(16 * 3000, 384, 240), (16 * 1500, 384, 1152)}
    s |= _model_shapes(768, 3072, 51904, (32 * 1500, 32 * 447)) | {(32 * 3000, 768, 240), (32 * 1500, 768, 2304)}
    s |= _model_shapes(1280, 5120, 51904, (32 * 1500, 32 * 447, 64 * 1500, 64 * 447))
    s |= {(64 * 3000, 1280, 240), (64 * 1500, 1280, 3840), (32 * 3000, 1280, 240), (32 * 1500, 1280, 3840)}
    s |= _model_shapes(1280, 5120, 51904, (512 * 1500, 512, 128, 64, 16, 1500, 1, 4, 8))
    s |= {(512 * 3000, 1280, 240), (512 * 1500, 1280, 3840), (3000, 1280, 240), (1500, 1280, 3840)}
    return sorted(s)


PARITY_SHAPES = {
    (1, 1, 8), (1, 17, 40), (1, 128, 200), (1, 129, 192), (5, 15, 40), (5, 51, 72), (5, 264, 72), (8, 128, 200),
    (8, 129, 256), (8, 136, 256), (8, 255, 200), (16, 129, 256), (16, 136, 256), (32, 16, 72), (32, 16, 1280),
    (32, 264, 1280), (33, 1, 8), (33, 17, 1280), (64, 15, 40), (64, 51, 8), (65, 16, 72), (65, 40, 264),
    (65, 264, 40), (120, 248, 320), (120, 255, 320), (127, 248, 320), (127, 255, 320), (127, 256, 256),
    (128, 1, 72), (128, 17, 1280), (128, 200, 1280), (128, 256, 8), (128, 257, 320), (129, 1, 8), (129, 136, 72),
    (129, 257, 64), (129, 264, 64), (136, 129, 8), (136, 136, 1024), (136, 257, 64), (136, 264, 64), (136, 264, 72),
    (200, 264, 2048), (248, 1, 72), (248, 8, 72), (255, 1, 72), (255, 8, 64), (255, 8, 72), (256, 8, 128),
    (256, 16, 128), (256, 127, 72), (256, 129, 5120), (256, 136, 5120), (256, 136, 5128), (256, 256, 3072),
    (256, 264, 3072), (256, 512, 128), (257, 120, 192), (257, 127, 192), (257, 128, 128), (257, 257, 128),
    (257, 264, 128), (257, 264, 200), (264, 120, 192), (264, 127, 192), (264, 136, 5056), (264, 257, 128),
    (264, 264, 72), (264, 264, 128), (300, 520, 3072), (512, 256, 128), (512, 256, 192), (512, 768, 3072),
    (520, 392, 72), (520, 520, 72), (520, 520, 192), (776, 3080, 6144), (1280, 768, 64), (4096, 4096, 1024),
    (4352, 4096, 64), (4352, 4096, 3072), (32868, 512, 64),
}

# every (M, N, K) of tests/test_kernels_gpu.py and tests/test_fp16_train_gpu.py (the dW tests' N, K, M as the product's
# M, N, K = output rows, output columns, tokens)
TEST_SHAPES = sorted({
    (200, 136, 72), (128, 128, 64), (257, 520, 1280), (96, 51, 240), (300, 264, 128), (48000, 3072, 768),
    (1000, 768, 3072), (300, 200, 256), (300, 264, 200), (520, 600, 1344), (1000, 784, 1280), (256, 256, 64),
    (28608, 1280, 1280), (14000, 2560, 640), (8200, 2056, 320), (8200, 2056, 128), (4104, 4096, 1344), (520, 264, 64),
    (2312, 1288, 5128), (8200, 4104, 1344), (16400, 2056, 256), (66000, 1280, 1280), (28608, 1280, 5120),
    (11000, 1288, 4096), (512, 1280, 5120), (14000, 1280, 51904), (1280, 1280, 28608), (2560, 1280, 8192),
    (264, 136, 4096), (1280, 1280, 1000), (1, 16, 8), (5, 1000, 1280), (64, 1280, 5120), (100, 3840, 1280),
    (128, 200, 64), (128, 1280, 5120), (65, 520, 1280), (512, 1280, 1280), (300, 3840, 1280), (4096, 768, 768),
    (1024, 3072, 768), (28608, 5120, 1280), (28608, 51904, 1280), (1000, 2560, 1280), (1000, 1280, 256),
    (768, 768, 14304), (768, 3072, 48000), (520, 520, 128)}
    # ... and of the parity suite's case table (tests/gemm_cases.py; tests/test_gemm_cases_cpu.py checks the inclusion)
    | PARITY_SHAPES)

ROUTE_FLAGS = (0, TILE128, TILE256, TILE256x128, TILE256PP, TILE256x128_S2, NOSPLIT)


def table():
    """Every call of the comparison: shapes x the four layouts x bf16 / fp16 x the routing flags, with the epilogues
    the step uses on that layout.  The forced persistent kernel is asked for K-major operands only (its domain)."""
    calls = []
    for M, N, K in sorted(set(config_shapes()) | set(TEST_SHAPES)):
        for at, bt in ((0, 0), (0, 1), (1, 0), (1, 1)):
            if (at and M % 8) or (bt and N % 8) or (not (at and bt) and K % 8):
                continue
            for H in (False, True):
                for rf in ROUTE_FLAGS:
                    if rf == TILE256PP and (at or bt):
                        continue
                    if not at and not bt:      # forward: bias + round, + GELU (+ aux), residual in the stream type
                        epis = ((True, F_BIAS | F_ROUND, None), (True, F_BIAS | F_ROUND | F_GELU | F_AUX_OUT, None),
                                (False, F_BIAS | F_ROUND, False), (False, 0, None))
                    elif at and bt:            # dW: fp32 accumulate
                        epis = ((False, F_ROUND | F_ACCUM, None), (False, 0, None))
                    else:                      # dX: round, GELU backward
                        epis = ((True, F_ROUND, None), (True, F_ROUND | F_DGELU, None), (False, 0, None))
                    for c16, f, r16 in epis:
                        calls.append(call(M, N, K, a_trans=at, b_trans=bt, H=H, c16=c16, flags=f | rf, res16=r16))
    return calls
