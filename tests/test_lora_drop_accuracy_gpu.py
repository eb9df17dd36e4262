"""The three dropout modes of the bf16 MFMA GEMM (gemm_k with drop_tile on A and on B; store4 / store8 and
splitk_reduce_k with the output mask) and lora_dx_k, per element.

The case tables, the references, the gates D1-D3 / L1 / L2 with their derivations and the NaN-framed
inputs are tests/lora_drop_refs.py; tests/test_lora_drop_refs_host.py shows on the CPU, for these very
inputs, that an honest restatement passes every gate and that each listed mutant fails. Each case asserts
its route (cullavo_gemm_plan under the case's forced tile; cullavo_gemm_workspace > 0 exactly where a
split is meant) before it runs. C and dx are views into sentinel frames, the operands views into NaN
frames. One JSON line per case goes to the stats file of tests/test_accuracy_gpu.py.
"""
import ctypes
import json

import pytest
import torch

from tests import gemm_refs as G
from tests import lora_drop_refs as R
from tests.test_accuracy_gpu import _log as _append_stats
from tests.test_gemm_accuracy_gpu import _options, _replay_kw, _Runner

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def _lib():
    from cullavo_amd import _lib as L
    return L.lib()


def _log(rec):
    print(json.dumps(rec))
    _append_stats(rec)


def _route(c, L):
    """asserts the case's plan and split; call under the case's forced tile"""
    plan = L.cullavo_gemm_plan(c["M"], c["N"], c["K"], c["al"], c["bl"], None)
    assert plan == c["plan"], f"{c['name']}: plan {plan}, the table says {c['plan']} ({c['route']})"
    dsc = ops().GemmDesc(c["al"], c["bl"], c["M"], c["N"], c["K"], None, 8, None, 8, None, c["N"], 1, 1.0)
    dsc.drop_operand, dsc.drop_p = c["mode"], R.P_PROD
    ws = L.cullavo_gemm_workspace(ctypes.addressof(dsc))
    assert bool(ws) == c["workspace"], f"{c['name']}: split-K workspace {ws}"
    return plan, ws


def _finish(r, stats):
    stats["failures"] = r.fails
    _log(stats)
    assert not r.fails, f"{stats['case']} ({r.c.get('route', '')}): " + "; ".join(r.fails)


def _bitwise_variants(r, variants, c32, stats, tag, drop_kw, keep=None, drop_scale=1.0):
    """G2 under dropout: each variant's launch against chain_replay of c32 (with the output drop step when
    keep is given); mismatch counts into stats, failures into r.fails"""
    d = r.d
    for v in variants:
        o = G.VARIANTS[v]
        kw = _options(d, o)
        dt = F32 if o.get("f32") else BF
        beta = o.get("beta", 0.0)
        fill = d["old"].to(dt) if beta else None
        pre_on = bool(o.get("preact"))
        y, pre = r.run(f"{tag}/{v}", dtype=dt, fill=fill, want_preact=pre_on, beta=beta, **kw, **drop_kw)
        want, wpre = G.chain_replay(c32, want_preact=pre_on, beta=beta, old=fill, out_dtype=dt, keep=keep,
                                    drop_scale=drop_scale, **_replay_kw(kw))
        nd = {"g2": G.ndiff(y, want)}
        if pre_on:
            nd["g2_preact"] = G.ndiff(pre, wpre)
        stats["bits_differing"][f"{tag}/{v}"] = nd
        r.fails += [f"{tag}/{v}: {k}: {n} elements differ" for k, n in nd.items() if n]


# ---------------------------------------------------------------------------------------------
# the layout mode 1 cannot run
# ---------------------------------------------------------------------------------------------
def test_mode1_refuses_b_layout_1():
    """M = 72, N = 40, K = 96, B stored [K, N] with row stride N + 24: N < K, so even a library without the
    check would read inside B's allocation"""
    L = _lib()
    M, N, K = 72, 40, 96
    d = G.gemm_inputs("drop1-layout", M, N, K, 0, 1, DEV, need=())
    assert d["B"].shape == (K, N) and d["B"].stride(0) == N + 24
    buf, C = G.framed(M, N, BF, DEV)
    dsc = ops().GemmDesc(0, 1, M, N, K, d["A"].data_ptr(), d["A"].stride(0), d["B"].data_ptr(), d["B"].stride(0),
                         C.data_ptr(), C.stride(0), 1, 1.0)
    dsc.drop_operand, dsc.drop_p, dsc.drop_seed = ops().DROP_A, R.P_PROD, R.DROP_SEED
    rc = L.cullavo_gemm_ex(ctypes.addressof(dsc), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and "b_layout" in L.cullavo_last_error().decode()
    assert bool((buf == G.SENT).all())


# ---------------------------------------------------------------------------------------------
# D1
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,al", [(1, 0), (2, 0), (2, 1)], ids=["mode1-00", "mode2-01", "mode2-11"])
@pytest.mark.parametrize("F", R.D1_F)
def test_d1_mask_bit_for_bit(mode, al, F):
    c, d = R.d1_inputs(mode, F, al, DEV)
    r = _Runner(dict(c, route=f"D1 mode {mode}"), d)
    stats = {"test": "lora_drop_d1", "case": f"d1-mode{mode}-{c['al']}{c['bl']}-F{F}", "shape": [c["M"], c["N"], c["K"]],
             "route": f"gemm_k<{c['al']},{c['bl']},f32,{mode}> unsplit", "mismatches": {}, "kept_share": {}}
    for p in R.D1_P:
        y, _ = r.run(f"p{p}", dtype=F32, drop_operand=mode, drop_p=p, drop_seed=R.DROP_SEED)
        want, keep = R.d1_expected(F, p, DEV)
        n = G.ndiff(y, want)
        stats["mismatches"][str(p)] = n
        stats["kept_share"][str(p)] = keep.double().mean().item()
        if n:
            wrong_mask = int(((y != 0) != keep).sum())
            r.fails.append(f"p {p}: {n} elements differ ({wrong_mask} of them kept / dropped wrongly)")
    _finish(r, stats)


# ---------------------------------------------------------------------------------------------
# D2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in R.CASES if c["mode"] in (1, 2)], ids=lambda c: c["name"])
def test_d2_dropped_operand_product(c):
    L = _lib()
    M, N, K = c["M"], c["N"], c["K"]
    plan, ws = _route(c, L)
    d = R.case_inputs(c, DEV)
    r = _Runner(c, d)
    stats = {"test": "lora_drop_d2", "case": c["name"], "shape": [M, N, K], "layouts": [c["al"], c["bl"]], "route": c["route"],
             "plan": plan, "workspace": ws, "err_over_f32_bound": {}, "rel_l2_f32": {}, "bits_differing": {}}
    # drop_p = 0 with the operand named: the plain call
    plain32, _ = r.run("plain f32", dtype=F32)
    plain16, _ = r.run("plain bf16")
    z32, _ = r.run("p0 f32", dtype=F32, drop_operand=c["mode"], drop_p=0.0, drop_seed=R.DROP_SEED)
    z16, _ = r.run("p0 bf16", drop_operand=c["mode"], drop_p=0.0, drop_seed=R.DROP_SEED)
    nd = {"f32": G.ndiff(z32, plain32), "bf16": G.ndiff(z16, plain16)}
    stats["bits_differing"]["p0_vs_plain"] = nd
    r.fails += [f"drop_p 0 against the plain call, {k}: {n} elements differ" for k, n in nd.items() if n]
    for p in (R.P_PROD, 0.5):
        drop_kw = dict(drop_operand=c["mode"], drop_p=p, drop_seed=R.DROP_SEED)
        ds = R.staged_inputs(c, d, p)
        ref, absprod = G.product_ref(ds["Amk"], ds["Bnk"])
        c32, _ = r.run(f"p{p} f32", dtype=F32, **drop_kw)
        w, rel, fin = G.g1(c32, ref, absprod, K)
        stats["err_over_f32_bound"][str(p)], stats["rel_l2_f32"][str(p)] = w, rel
        if not (w <= 1.0 and rel <= 1e-5 and fin):
            r.fails.append(f"p {p} f32 output: err / (K 2^-24 |A_d||B|^T) {w:.3f}, rel-L2 {rel:.2e}, finite {fin}")
        _bitwise_variants(r, R.D2_VARIANTS, c32, stats, f"p{p}", drop_kw)
    _finish(r, stats)


# ---------------------------------------------------------------------------------------------
# D3
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in R.CASES if c["mode"] == 3], ids=lambda c: c["name"])
def test_d3_output_dropout(c):
    L = _lib()
    M, N, K = c["M"], c["N"], c["K"]
    prev_tile = L.cullavo_gemm_set_tile(c["tile"])
    prev_epi = L.cullavo_gemm_set_epilogue(1)
    try:
        plan, ws = _route(c, L)
        d = R.case_inputs(c, DEV)
        r = _Runner(c, d)
        stats = {"test": "lora_drop_d3", "case": c["name"], "shape": [M, N, K], "layouts": [c["al"], c["bl"]], "tile": c["tile"],
                 "route": c["route"], "plan": plan, "workspace": ws, "bits_differing": {}, "f32_err_over_gate": {},
                 "ambiguous_share": {}, "mismatches": {}}
        # the kernel's own plain f32 product of the same route, itself under G1
        c32, _ = r.run("plain f32", dtype=F32)
        ref, absprod = G.product_ref(d["Amk"], d["Bnk"])
        w, rel, fin = G.g1(c32, ref, absprod, K)
        stats["err_over_f32_bound"], stats["rel_l2_f32"] = w, rel
        if not (w <= 1.0 and rel <= 1e-5 and fin):
            r.fails.append(f"plain f32 output: G1 {w:.3f}, rel-L2 {rel:.2e}, finite {fin}")
        # p = 0.5: the scale is exact, every variant bitwise
        keep = R.keep_mask(R.DROP_SEED, M, N, 0.5, DEV)
        drop_kw = dict(drop_operand=3, drop_p=0.5, drop_seed=R.DROP_SEED)
        y32, _ = r.run("p0.5 f32", dtype=F32, **drop_kw)
        n = G.ndiff(y32, G.chain_replay(c32, out_dtype=F32, keep=keep, drop_scale=2.0)[0])
        stats["bits_differing"]["p0.5/f32"] = n
        if n:
            r.fails.append(f"p 0.5 f32 output: {n} elements differ")
        _bitwise_variants(r, R.D3_SPLIT_VARIANTS if c["workspace"] else R.D3_VARIANTS, c32, stats, "p0.5", drop_kw,
                          keep=keep, drop_scale=2.0)
        # scales that are no power of two
        for p in R.D3_P_RON:
            keep = R.keep_mask(R.DROP_SEED, M, N, p, DEV)
            drop_kw = dict(drop_operand=3, drop_p=p, drop_seed=R.DROP_SEED)
            y32, _ = r.run(f"p{p} f32", dtype=F32, **drop_kw)
            w, nz = R.d3_f32(y32, c32, keep, p)
            stats["f32_err_over_gate"][str(p)] = w
            old = d["old"]
            y, _ = r.run(f"p{p} bf16 beta 1", fill=old, beta=1.0, **drop_kw)
            bad, amb = R.d3_ron(y, c32, keep, p, old)
            nold = G.ndiff(y[~keep], old[~keep])
            stats["ambiguous_share"][str(p)] = amb
            stats["mismatches"][str(p)] = {"f32_dropped_nonzero": nz, "bf16_outside_neighbours": bad, "bf16_dropped_not_old": nold}
            if not w <= 1.0:
                r.fails.append(f"p {p} f32 output: |y - c s| / (E |c s|) {w:.3f} on a kept element")
            if nz:
                r.fails.append(f"p {p} f32 output: {nz} dropped elements are not 0")
            if bad:
                r.fails.append(f"p {p} bf16 beta 1: {bad} elements are neither the rounded f64 value nor its neighbour")
            if nold:
                r.fails.append(f"p {p} bf16 beta 1: {nold} dropped elements are not the old value")
            if amb > G.AMBIGUOUS_CAP:
                r.fails.append(f"p {p}: ambiguous share {amb:.4f} over the cap")
    finally:
        L.cullavo_gemm_set_tile(prev_tile)
        L.cullavo_gemm_set_epilogue(prev_epi)
    _finish(r, stats)


# ---------------------------------------------------------------------------------------------
# lora_dx
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mod,M,N,p", R.lora_runs(), ids=lambda x: str(x))
def test_lora_dx(n_mod, M, N, p):
    d = R.lora_inputs(n_mod, M, N, DEV)
    seeds = R.lora_seeds(n_mod)
    du, a = d["du"], d["a"]
    assert du.stride(0) == 64 * n_mod + 8 and a.stride(0) == N + 24
    fails = []
    buf, dx = R.dx_frame(d)
    assert dx.stride(0) == N + 4
    ops().lora_dx(du, a, dx, n_mod=n_mod, drop_p=p, seeds=seeds)
    # L1: the per-module launches D3 pins (ldc a multiple of 8: a frame of their own)
    rbuf, ref = G.framed(M, N, BF, DEV, fill=d["dx0"])
    for m in range(n_mod):
        dum, am = du[:, 64 * m:64 * m + 64], a[64 * m:64 * m + 64]
        ops().gemm_ex(0, 1, M, N, 64, dum, dum.stride(0), am, am.stride(0), ref, ref.stride(0), beta=1.0,
                      drop_operand=ops().DROP_OUT, drop_p=p, drop_seed=seeds[m])
    torch.cuda.synchronize()
    if not G.frame_untouched(buf, M, N):
        fails.append("lora_dx wrote outside its [M, N] view")
    if not G.frame_untouched(rbuf, M, N):
        fails.append("gemm_ex wrote outside its [M, N] view")
    l1 = G.ndiff(dx, ref)
    if l1:
        fails.append(f"L1: {l1} elements differ from the per-module launches")
    bad, amb, w = R.lora_dx_check(dx, d, n_mod, p, seeds)
    if bad:
        fails.append(f"L2: {bad} elements outside the gate (worst err / bound {w})")
    if amb is not None and amb > G.AMBIGUOUS_CAP:
        fails.append(f"L2: ambiguous share {amb:.4f} over the cap")
    _log({"test": "lora_dx", "case": f"n{n_mod}-{M}x{N}-p{p}", "shape": [M, N, 64 * n_mod],
          "route": f"lora_dx_k<{n_mod}>: {-(-M // 64) * -(-N // 256)} workgroups", "l1_bits_differing": l1,
          "l2_outside_gate": bad, "l2_err_over_bound": w, "ambiguous_share": amb, "failures": fails})
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("what", ["n_mod 0", "n_mod 4", "N % 8", "ld_dx < N", "p = 1"])
def test_lora_dx_argument_errors(what):
    """each returns a code before any launch and leaves dx and its frame untouched"""
    L = _lib()
    n_mod, M, N = 2, 63, 256
    d = R.lora_inputs(n_mod, M, N, DEV)
    buf, dx = R.dx_frame(d)
    before = buf.clone()
    n, Nn, ld_dx, p = {"n_mod 0": (0, N, N + 4, 0.05), "n_mod 4": (4, N, N + 4, 0.05), "N % 8": (2, N - 4, N + 4, 0.05),
                       "ld_dx < N": (2, N, N - 4, 0.05), "p = 1": (2, N, N + 4, 1.0)}[what]
    s = R.lora_seeds(2)
    rc = L.cullavo_lora_dx(n, M, Nn, d["du"].data_ptr(), d["du"].stride(0), d["a"].data_ptr(), d["a"].stride(0),
                           dx.data_ptr(), ld_dx, p, s[0], s[1], 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and "lora_dx" in L.cullavo_last_error().decode()
    assert G.ndiff(buf, before) == 0
