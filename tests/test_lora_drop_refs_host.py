"""The gates of tests/lora_drop_refs.py on the CPU, for the very inputs of the GPU cases: an honest f32
restatement of the three dropout modes of the bf16 GEMM and of lora_dx_k passes every gate (D1-D3, L1's
host stand-in, L2), each listed one-line mutant fails the gate named beside it, the ambiguous shares stay
within their cap for the contracted and the uncontracted f32 form, the case table's routes are what the
library plans, and the layout the bf16 mode 1 cannot run is refused before any launch. No GPU."""
import ctypes

import pytest
import torch

from tests import gemm_refs as G
from tests import lora_drop_refs as R

BF = torch.bfloat16
F32 = torch.float32
BY_NAME = {c["name"]: c for c in R.CASES}
OPERAND_CASES = [c for c in R.CASES if c["mode"] in (1, 2)]
OUTPUT_SHAPES = list({c["inputs"]: c for c in R.CASES if c["mode"] == 3}.values())  # one per shape: the tiles share inputs


def _opts(d, v):
    o = G.VARIANTS[v]
    beta = o.get("beta", 0.0)
    dt = F32 if o.get("f32") else BF
    return dict(alpha=o.get("alpha", 1.0), bias=d["bias"] if o.get("bias") else None,
                addend=d["addend"] if o.get("addend") else None, residual=d["residual"] if o.get("residual") else None,
                want_preact=bool(o.get("preact")), beta=beta, old=d["old"].to(dt) if beta else None, out_dtype=dt)


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
def test_threshold_elements():
    """every (F, p) of parity_refs.DROP_CASES still has an element whose hash equals the threshold under
    DROP_SEED; p = 0.1 (the issue's third value) has none, which is why D1 runs the union"""
    for F, p in {(F, p) for _, _, _, F, p in R.DROP_CASES}:
        assert F in R.D1_F and p in R.D1_P
        assert R.threshold_hits(F, p) >= 1, (F, p)
    assert all(R.threshold_hits(F, 0.1) == 0 for F in R.D1_F)
    assert {0.05, 0.1, 0.5} <= set(R.D1_P)


def test_case_table_routes():
    from cullavo_amd import _lib, ops
    L = _lib.lib()
    bad = []
    for c in R.CASES:
        prev = L.cullavo_gemm_set_tile(c["tile"])
        try:
            plan = L.cullavo_gemm_plan(c["M"], c["N"], c["K"], c["al"], c["bl"], None)
            dsc = ops.GemmDesc(c["al"], c["bl"], c["M"], c["N"], c["K"], None, 8, None, 8, None, c["N"], 1, 1.0)
            dsc.drop_operand, dsc.drop_p = c["mode"], R.P_PROD
            ws = L.cullavo_gemm_workspace(ctypes.addressof(dsc))
        finally:
            L.cullavo_gemm_set_tile(prev)
        if plan != c["plan"]:
            bad.append((c["name"], "plan", plan))
        splits = -(-(-(-c["K"] // 64)) // c["kt_per"]) if c["kt_per"] else 0
        if ws != splits * c["M"] * c["N"] * 4:
            bad.append((c["name"], "workspace", ws))
    assert not bad, bad
    names = " ".join(c["route"] for c in R.CASES)
    for word in ("drop_tile<0>", "drop_tile<1>", "launch<1,1,CT,2>", "store4", "192,256> LDS epilogue", "288,256> LDS epilogue",
                 "256,256> LDS epilogue", "256,256> partials", "launch<0,1> partials"):
        assert word in names, word


def test_layout_mode1_refused_before_launch():
    """drop_operand 1 with b_layout 1 (B stored [K, N]) returns CULLAVO_EUNSUPPORTED naming b_layout and
    leaves C alone; the f32 parity kernel, which takes both layouts, is not reached by the check"""
    from cullavo_amd import _lib, ops
    L = _lib.lib()
    M, N, K = 72, 40, 96
    d = G.gemm_inputs("drop1-layout", M, N, K, 0, 1, need=())
    assert d["B"].shape == (K, N) and d["B"].stride(0) == N + 24
    buf, C = G.framed(M, N, BF, "cpu")
    dsc = ops.GemmDesc(0, 1, M, N, K, d["A"].data_ptr(), d["A"].stride(0), d["B"].data_ptr(), d["B"].stride(0),
                       C.data_ptr(), C.stride(0), 1, 1.0)
    dsc.drop_operand, dsc.drop_p, dsc.drop_seed = 1, 0.05, R.DROP_SEED
    rc = L.cullavo_gemm_ex(ctypes.addressof(dsc), None)
    assert rc == 2 and "b_layout" in L.cullavo_last_error().decode()
    assert bool((buf == G.SENT).all())


# ---------------------------------------------------------------------------------------------
# D1, D2
# ---------------------------------------------------------------------------------------------
def _d1_fails(mask_mutant=None, stage_mutant=None):
    """the D1 sets (mode, F, al, p) whose restated output is not the expected one"""
    out = []
    for mode, al in ((1, 0), (2, 0), (2, 1)):
        for F in R.D1_F:
            c, d = R.d1_inputs(mode, F, al)
            c = dict(c, mode=mode, kt_per=None)
            d["Amk"] = d["A"] if c["al"] == 0 else d["A"].T
            d["Bnk"] = d["B"] if c["bl"] == 0 else d["B"].T
            for p in R.D1_P:
                ds = R.staged_inputs(c, d, p, mask_mutant=mask_mutant, stage_mutant=stage_mutant)
                got = G.product_honest(ds, c["M"], c["N"], c["K"])
                want, _ = R.d1_expected(F, p)
                if G.ndiff(got, want):
                    out.append((mode, F, al, p))
    return out


def test_honest_passes_d1():
    assert not _d1_fails()


def _d2_g1(c, d, p, **mut):
    ds = R.staged_inputs(c, d, p, **mut)
    c32 = G.product_honest(ds, c["M"], c["N"], c["K"], kt_per=c["kt_per"])
    exact = R.staged_inputs(c, d, p)
    ref, absprod = G.product_ref(exact["Amk"], exact["Bnk"])
    return G.g1_ok(c32, ref, absprod, c["K"]), c32


@pytest.mark.parametrize("c", OPERAND_CASES, ids=lambda c: c["name"])
def test_honest_passes_d2(c):
    d = R.case_inputs(c)
    plain = G.product_honest(d, c["M"], c["N"], c["K"], kt_per=c["kt_per"])
    ok0, c0 = _d2_g1(c, d, 0.0)
    assert ok0 and G.ndiff(c0, plain) == 0  # drop_p = 0: the plain product
    for p in (R.P_PROD, 0.5):
        ok, c32 = _d2_g1(c, d, p)
        assert ok, (c["name"], p)
        assert G.ndiff(c32, plain) > 0.3 * c32.numel()
        for v in R.D2_VARIANTS:
            kw = _opts(d, v)
            assert G.ndiff(G.chain_honest(c32, **kw)[0], G.chain_replay(c32, **kw)[0]) == 0, v


MASK_MUTANTS = ("drop_swapped", "drop_thr_off_by_one", "halves_swapped", "slab_relative_k", "tile_relative")
STAGE_MUTANTS = ("no_scale_ktail", "not_rounded")


@pytest.fixture(scope="module")
def operand_inputs():
    return {c["name"]: R.case_inputs(c) for c in OPERAND_CASES}


@pytest.mark.parametrize("mutant", MASK_MUTANTS + STAGE_MUTANTS)
def test_operand_mutants_fail(operand_inputs, mutant):
    kw = {"mask_mutant": mutant} if mutant in MASK_MUTANTS else {"stage_mutant": mutant}
    d2 = {(c["name"], p) for c in OPERAND_CASES for p in (R.P_PROD, 0.5)
          if not _d2_g1(c, operand_inputs[c["name"]], p, **kw)[0]}
    d1 = _d1_fails(**kw)
    assert d1 or d2, mutant
    split = {c["name"] for c in OPERAND_CASES if c["kt_per"]}
    if mutant == "slab_relative_k":  # only a second split can show it, and every split case does, in both modes
        assert {n for n, _ in d2} == split and not d1
    if mutant == "tile_relative":  # a second M-tile (mode 1) or N-tile (mode 2)
        assert {n for n, _ in d2} == {c["name"] for c in OPERAND_CASES if (c["M"] if c["mode"] == 1 else c["N"]) > R.TILE}
        assert {(m, F) for m, F, _, _ in d1} == {(1, 96), (1, 264), (2, 264)}  # D1: T = 136 tokens, F = 264 features
    if mutant == "drop_thr_off_by_one":  # one element in 65536: the D1 sets chosen to hold one
        assert {(F, p) for _, F, _, p in d1} == {(F, p) for F in R.D1_F for p in (0.05, 0.25, 0.5)}
    if mutant == "not_rounded":  # s = 2 is exact: p = 0.5 cannot show it
        assert d2 == {(c["name"], R.P_PROD) for c in OPERAND_CASES} and all(p != 0.5 for *_, p in d1)
    if mutant in ("drop_swapped", "halves_swapped", "no_scale_ktail"):
        assert {n for n, _ in d2} == {c["name"] for c in OPERAND_CASES}


# ---------------------------------------------------------------------------------------------
# D3
# ---------------------------------------------------------------------------------------------
def _d3_setup(c):
    d = R.case_inputs(c)
    c32 = G.product_honest(d, c["M"], c["N"], c["K"], kt_per=c["kt_per"])
    return d, c32


@pytest.mark.parametrize("c", OUTPUT_SHAPES, ids=lambda c: c["inputs"])
def test_honest_passes_d3(c):
    d, c32 = _d3_setup(c)
    M, N = c["M"], c["N"]
    keep = R.keep_mask(R.DROP_SEED, M, N, 0.5)
    for v in R.D3_VARIANTS:
        kw = _opts(d, v)
        want, wpre = G.chain_replay(c32, keep=keep, drop_scale=2.0, **kw)
        for contracted in (False, True):
            out, pre = R.drop_chain_honest(c32, keep, 0.5, contracted=contracted, **kw)
            assert G.ndiff(out, want) == 0, (v, contracted)
            assert pre is None or G.ndiff(pre, wpre) == 0
        beta = kw["beta"]
        if not (kw["bias"] is not None or kw["addend"] is not None or kw["residual"] is not None):
            exp = (beta * kw["old"].float()).to(kw["out_dtype"]) if beta else torch.zeros((), dtype=kw["out_dtype"])
            assert bool((want[~keep] == (exp[~keep] if beta else exp)).all())
    for p in R.D3_P_RON:
        keep = R.keep_mask(R.DROP_SEED, M, N, p)
        y32, _ = R.drop_chain_honest(c32, keep, p, out_dtype=F32)
        w, nz = R.d3_f32(y32, c32, keep, p)
        assert w <= 1.0 and nz == 0, (p, w, nz)
        for contracted in (False, True):
            y, _ = R.drop_chain_honest(c32, keep, p, beta=1.0, old=d["old"], contracted=contracted)
            bad, amb = R.d3_ron(y, c32, keep, p, d["old"])
            assert bad == 0 and amb <= G.AMBIGUOUS_CAP, (p, contracted, bad, amb)
            assert G.ndiff(y[~keep], d["old"][~keep]) == 0


def test_output_mutants_fail_d3():
    c = BY_NAME["m3-136x264-t-1"]
    d, c32 = _d3_setup(c)
    keep = R.keep_mask(R.DROP_SEED, c["M"], c["N"], 0.5)
    kw = _opts(d, "alpha2_bias")
    want = G.chain_replay(c32, keep=keep, drop_scale=2.0, **kw)[0]
    assert G.ndiff(R.drop_chain_honest(c32, keep, 0.5, **kw)[0], want) == 0
    assert G.ndiff(R.drop_chain_honest(c32, keep, 0.5, mutant="drop_after_bias", **kw)[0], want) > 0.9 * want.numel()
    for v in ("beta1_bf16", "beta1_f32", "beta05_bf16"):
        kw = _opts(d, v)
        want = G.chain_replay(c32, keep=keep, drop_scale=2.0, **kw)[0]
        assert G.ndiff(R.drop_chain_honest(c32, keep, 0.5, mutant="beta_before_drop", **kw)[0], want) > 0.9 * want.numel()
    for p in R.D3_P_RON:  # the production call: dropped elements lose their old value, kept ones gain s * old
        keep = R.keep_mask(R.DROP_SEED, c["M"], c["N"], p)
        y, _ = R.drop_chain_honest(c32, keep, p, beta=1.0, old=d["old"], mutant="beta_before_drop")
        bad, _ = R.d3_ron(y, c32, keep, p, d["old"])
        assert bad > 0.9 * y.numel()
    # the mask mutants through mode 3: the wrong elements are zero / scaled
    want = G.chain_replay(c32, keep=R.keep_mask(R.DROP_SEED, c["M"], c["N"], 0.5), drop_scale=2.0)[0]
    for mutant in ("drop_swapped", "halves_swapped"):
        km = R.mask(R.DROP_SEED, c["M"], c["N"], 0.5, mutant=mutant)
        assert G.ndiff(G.chain_replay(c32, keep=km, drop_scale=2.0)[0], want) > 0.3 * c32.numel()


# ---------------------------------------------------------------------------------------------
# lora_dx
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mod,M,N,p", R.lora_runs(), ids=lambda x: str(x))
def test_lora_dx_honest_passes(n_mod, M, N, p):
    d = R.lora_inputs(n_mod, M, N)
    assert d["du"].stride(0) == 64 * n_mod + 8 and d["a"].stride(0) == N + 24 and d["a"].shape == (64 * n_mod, N)
    seeds = R.lora_seeds(n_mod)
    assert len(set(seeds)) == n_mod
    for contracted in (False, True):
        buf, view = R.lora_dx_honest(d, n_mod, p, seeds, contracted=contracted)
        assert view.stride(0) == N + 4 and G.frame_untouched(buf, M, N)
        bad, amb, w = R.lora_dx_check(view, d, n_mod, p, seeds)
        assert bad == 0, (contracted, bad, w)
        assert amb is None or amb <= G.AMBIGUOUS_CAP, amb
    # L1's host stand-in: the per-module mode-3 chain (alpha 1, beta 1, bf16) applied in order gives the same bits
    run = d["dx0"]
    for m in range(n_mod):
        acc = d["du"][:, 64 * m:64 * m + 64].float() @ d["a"][64 * m:64 * m + 64].float()
        run, _ = R.drop_chain_honest(acc, R.keep_mask(seeds[m], M, N, p), p, beta=1.0, old=run)
    assert G.ndiff(run, R.lora_dx_honest(d, n_mod, p, seeds)[1]) == 0


@pytest.mark.parametrize("mutant", ["seed_m0", "old_from_dx0", "rows_past_M"])
def test_lora_dx_mutants_fail(mutant):
    hit = []
    for n_mod, M, N, p in R.lora_runs():
        d = R.lora_inputs(n_mod, M, N)
        seeds = R.lora_seeds(n_mod)
        buf, view = R.lora_dx_honest(d, n_mod, p, seeds, mutant=mutant)
        bad, _, w = R.lora_dx_check(view, d, n_mod, p, seeds)
        if bad or not G.frame_untouched(buf, M, N):
            hit.append((n_mod, M, N, p))
            if mutant != "rows_past_M":
                assert w > 100.0, (mutant, w)  # whole products, not a near miss
    if mutant == "seed_m0":  # needs a second module and a mask
        assert hit == [r for r in R.lora_runs() if r[0] >= 2 and r[3] > 0]
    elif mutant == "old_from_dx0":
        assert hit == [r for r in R.lora_runs() if r[0] >= 2]
    else:
        assert hit == R.lora_runs()


def test_cancelling_inputs_break_the_cap():
    """N(0, 1) operands, whose 64 terms cancel: the honest lora_dx passes L2, but more of it is ambiguous than
    the cap allows (see lora_inputs)"""
    n_mod, M, N, p = 1, 65, 264, R.P_PROD
    d = R.lora_inputs(n_mod, M, N, cancelling=True)
    seeds = R.lora_seeds(n_mod)
    bad, amb, _ = R.lora_dx_check(R.lora_dx_honest(d, n_mod, p, seeds)[1], d, n_mod, p, seeds)
    assert bad == 0 and amb > 2 * G.AMBIGUOUS_CAP
