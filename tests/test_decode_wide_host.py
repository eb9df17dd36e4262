"""CPU checks behind tests/test_decode_wide_gpu.py: the float64 gate of the wide decode product
(tests/decode_refs.py gemv_gate: K 2^-24 |X||W|^T per element, rel-L2 1e-5) passes an honest f32
restatement of gemv_wide_k's summation order on every case the GPU test runs and fails one-line
mutants of it, and the pure-Python predicate that routes a decode step to the wide product takes
exactly the one-token bf16 steps at 17 .. 64 sequences with the switch on.
"""
import pytest
import torch

from tests import decode_refs as R
from tests import decode_wide_refs as WR

BF = torch.bfloat16


@pytest.mark.parametrize("M,N,K", WR.WIDE_CASES, ids=["x".join(map(str, c)) for c in WR.WIDE_CASES])
def test_gate_passes_honest_and_fails_mutants(M, N, K):
    X, W, _, _, _ = WR.wide_inputs(M, N, K)
    ref, absprod = R.gemv_ref(X, W)
    w, rel = R.gemv_gate(WR.wide_honest(X, W), ref, absprod, K)
    print(f"wide {M}x{N}x{K}: honest err/gate {w:.3f}, rel-L2 {rel:.2e}")
    assert R.gemv_gate_ok(WR.wide_honest(X, W), ref, absprod, K)
    nk = -(-K // 32)
    mutants = {"tail8": dict(drop_tail8=True), "drop_step": dict(drop_step=nk // 2),
               "double_step": dict(double_step=nk // 2), "row": dict(row_last_as_0=True),
               "rows16": dict(rows16_as_0=True)}
    if N > 8:  # at N = 8 there is no row N-9
        mutants["n_clamp"] = dict(clamp_n_tail=True)
    for name, kw in mutants.items():
        assert not R.gemv_gate_ok(WR.wide_honest(X, W, **kw), ref, absprod, K), f"mutant {name} passes the gate"


def test_honest_rows_do_not_depend_on_the_other_rows():
    """the restated order splits K only: 17 rows alone or among 64 give the same bits"""
    X, W, _, _, _ = WR.wide_inputs(64, 264, 4096)
    assert torch.equal(WR.wide_honest(X[:17], W), WR.wide_honest(X, W)[:17])


@pytest.mark.parametrize("M,N,K", WR.WIDE_SWIGLU_CASES)
def test_swiglu_honest_within_the_decode_gate(M, N, K):
    """transform 3's arithmetic is cullavo_decode_linear's: the same derived bound holds at these rows"""
    X, W2, _, _, _ = WR.wide_inputs(M, 2 * N, K)
    ref, absprod = R.gemv_ref(X, W2)
    bound = K * 2.0 ** -24 * absprod
    w = R.swiglu_gate(WR.wide_swiglu_honest(X, W2), ref[:, :N], ref[:, N:], bound[:, :N], bound[:, N:])
    assert w <= 1.0, w


def test_routing_predicate():
    from cullavo_amd import generation as G
    f32 = torch.float32
    for B in range(1, 80):
        want = 17 <= B <= 64
        assert G.wide_route(B, 1, BF, True) is want, B
        assert G.wide_route(B, 1, BF, False) is False
        assert G.wide_route(B, 2, BF, True) is False      # follow-up turns, chunked prefill
        assert G.wide_route(B, 1, f32, True) is False     # the f32 parity model
    assert G.wide_route(32, 576, BF, True) is False
    # switch None: the module's DECODE_WIDE, read per call
    old = G.DECODE_WIDE
    try:
        G.DECODE_WIDE = True
        assert G.wide_route(17, 1, BF) and G.wide_route(64, 1, BF) and not G.wide_route(16, 1, BF)
        G.DECODE_WIDE = False
        assert not G.wide_route(17, 1, BF)
    finally:
        G.DECODE_WIDE = old


def test_measured_losers_stay_on_the_tiles():
    """ops.WIDE_TILES_FASTER holds (weight rows, K) -> M ranges inside 17 .. 64; anything else is wide"""
    from cullavo_amd import ops
    for (rows, K), ranges in ops.WIDE_TILES_FASTER.items():
        for lo, hi in ranges:
            assert ops.WIDE_M_MIN <= lo <= hi <= ops.WIDE_M_MAX
            assert ops.wide_prefers_tiles(rows, K, lo) and ops.wide_prefers_tiles(rows, K, hi)
    assert not ops.wide_prefers_tiles(768, 256, 17)  # the small test models: unmeasured, wide
