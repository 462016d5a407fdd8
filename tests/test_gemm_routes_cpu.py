"""The GEMM route planner (csrc/gemm.hip plan_gemm, asked through ops.gemm_route / tw_gemm_route with a given CU count:
no GPU, nothing launched) against tests/gemm_routes.py, the plain-Python restatement of the routing as it stood before
the planner existed; against anchors derived by hand from that code for 256 CUs; and the table's coverage of every
route the library instantiates."""
import pytest
import torch

import gemm_routes as gr


def _ask(c, cus, have_ws=True):
    from tw import ops
    h = torch.float16 if c.H else torch.bfloat16
    f = c.flags
    return ops.gemm_route(
        h, h, h if c.c16 else torch.float32, c.M, c.N, c.K, lda=c.M if c.a_trans else c.K,
        ldb=c.N if c.b_trans else c.K, ldc=c.ldc, a_trans=c.a_trans, b_trans=c.b_trans,
        bias=h if f & gr.F_BIAS else None, res=None if c.res16 is None else (h if c.res16 else torch.float32),
        ldr=c.ldr, res_mod=c.res_mod, aux=h if f & (gr.F_AUX_OUT | gr.F_DGELU) else None, ldaux=c.ldaux,
        flags=f & ~(gr.F_BIAS | gr.F_RES), batch=c.batch, sC=c.sC, sR=c.sR, sAux=c.sAux, cus=cus, have_ws=have_ws)


@pytest.fixture(scope="module")
def table():
    return gr.table()


def test_route_names_match_the_library():
    from tw import ops
    assert ops.GEMM_ROUTES == gr.ROUTES and ops.GEMM_EPILOGUES == gr.EPI
    assert (ops.GEMM_TILE128, ops.GEMM_TILE256, ops.GEMM_TILE256x128, ops.GEMM_TILE256PP, ops.GEMM_NOSPLIT,
            ops.GEMM_TILE256x128_S2) == (gr.TILE128, gr.TILE256, gr.TILE256x128, gr.TILE256PP, gr.NOSPLIT,
                                         gr.TILE256x128_S2)
    assert ops.GEMM_GROUP_M(8) == 8 << 24


@pytest.mark.parametrize("cus", [256, 8])     # the MI355X, and what the library assumes without a device
@pytest.mark.parametrize("have_ws", [True, False])
def test_planner_equals_the_restated_routing(table, cus, have_ws):
    bad = []
    for c in table:
        got, want = tuple(_ask(c, cus, have_ws)), tuple(gr.parent_route(c, cus, have_ws))
        if got != want:
            bad.append((c, got, want))
    assert not bad, (len(bad), bad[:5])


BR = gr.F_BIAS | gr.F_ROUND
# (call, route, S, m_dp, split_tile, group_m) on 256 CUs, derived by hand from the routing
ANCHORS = [
    (gr.call(28608, 1280, 1280, flags=BR), "rounds_dp_tail", 0, 102, 0, 1),
    (gr.call(28608, 1280, 5120, flags=BR), "rounds_sk_tail", 5, 102, 0, 1),
    (gr.call(512, 1280, 5120, flags=BR), "rounds_sk_tail", 16, 0, 0, 1),
    (gr.call(512, 1280, 1280, flags=BR), "t128_ring4", 0, 0, 0, 1),
    (gr.call(66000, 1280, 1280, flags=BR), "rounds_dp_tail", 0, 256, 0, 8),
    (gr.call(14000, 1280, 51904, flags=BR), "rounds_dp_tail", 0, 51, 0, 1),
    (gr.call(5, 1000, 1280, flags=BR), "skinny", 1, 0, 0, 1),
    (gr.call(100, 3840, 1280, flags=BR), "skinny_splitk", 2, 0, 0, 1),
    # dW, both operands transposed, fp32 C, round + accumulate, output 768 x 3072 over K = 48000 tokens
    (gr.call(768, 3072, 48000, a_trans=True, b_trans=True, c16=False, flags=gr.F_ROUND | gr.F_ACCUM),
     "splitk_dw", 6, 0, 256, 1),
]
# the same calls when the split-K workspace cannot be had: what follows the route in the routing
FALLBACK = {1: ("rounds_dp_tail", 0, 102, 0, 1), 2: ("t128_ring4", 0, 0, 0, 1), 7: ("skinny", 1, 0, 0, 1),
            8: ("t128", 0, 0, 0, 1)}


@pytest.mark.parametrize("i", range(len(ANCHORS)))
def test_hand_derived_anchors(i):
    c, *want = ANCHORS[i]
    assert tuple(_ask(c, 256))[:5] == tuple(want)
    assert tuple(gr.parent_route(c, 256))[:5] == tuple(want)
    no_ws = tuple(_ask(c, 256, have_ws=False))[:5]
    assert no_ws == tuple(gr.parent_route(c, 256, have_ws=False))[:5]
    assert no_ws == FALLBACK.get(i, tuple(want))


def test_table_reaches_every_route_the_library_instantiates(table):
    seen, split_tiles = set(), set()
    for c in table:
        p = gr.parent_route(c, 256)
        seen.add((p.route, c.H))
        if p.route == "splitk_dw":
            split_tiles.add((p.split_tile, c.H))
    # every route in both operand types, but the edge-strip route: only the fp16 persistent kernel lacks ragged tiles
    want = {(r, H) for r in gr.ROUTES for H in (False, True)} - {("persistent_edges", False)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    assert split_tiles == {(128, False), (256, False), (128, True), (256, True)}
    assert len(table) < 40000


def test_invalid_and_empty_calls():
    from tw import ops
    bf = torch.bfloat16
    assert ops.gemm_route(bf, bf, bf, 0, 128, 64, lda=64, ldb=64, ldc=128, cus=256).route is None
    with pytest.raises(RuntimeError):      # K-major operands need K % 8 == 0, as the GEMM itself answers
        ops.gemm_route(bf, bf, bf, 128, 128, 60, lda=64, ldb=64, ldc=128, cus=256)
