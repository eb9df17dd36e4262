"""The gates of tests/parity_refs.py discriminate, shown on the CPU before any GPU time is spent.

For every case of tests/test_parity_accuracy_gpu.py (same seeds, shapes and frames) an honest restatement
of the kernel's order stays at or below 1.0 of every tolerance gate and shows 0 differing bits under every
bitwise gate; each listed one-line mutant exceeds 2.0, or differs in bits, or breaks an exact-zero /
finiteness check, on at least one case. For every mutant the output (pytest -s) names a case on which it
fails and the cases on which it computes what the honest form computes. The exact emulation of fmaf that
the bitwise product gate P0 rests on is proven against rational arithmetic first.
"""
import random
from fractions import Fraction

import numpy as np
import torch

from tests import parity_refs as R

F32, BF = R.F32, R.BF


# ---------------------------------------------------------------------------------------------
# fmaf, exactly
# ---------------------------------------------------------------------------------------------
def _rne_f32(x):
    """Fraction -> the nearest f32 (ties to even), normal range, as a Fraction"""
    if x == 0:
        return Fraction(0)
    s, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (e - 23)
    n, rem = divmod(x, ulp)
    if rem * 2 > ulp or (rem * 2 == ulp and n % 2 == 1):
        n += 1
    return s * n * ulp


def _fma_check(triples, fma):
    a, b, c = (np.array([t[i] for t in triples], dtype=np.float32).astype(np.float64) for i in range(3))
    got = fma(a, b, c)
    bad = 0
    for i in range(len(triples)):
        want = _rne_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        bad += Fraction(float(got[i])) != want
    return bad


def _double_rounding_triples():
    """a b + acc just below the midpoint of acc (odd last bit) and its successor, by 2^-46 of the product:
    the f64 sum is the midpoint itself and the cast to f32 then ties to even, away from the exact result"""
    out = []
    for e in range(-20, 21, 2):
        for i in range(0, 7):
            for sg in (1.0, -1.0):
                a = sg * (1.0 + 2.0 ** -23) * 2.0 ** i
                b = (1.0 - 2.0 ** -23) * 2.0 ** (6 - i + e)
                out.append((a, b, sg * (2.0 ** 30 + 2.0 ** 7) * 2.0 ** e))
    return out


def test_fma_emulation_is_exact():
    rnd = random.Random(7)
    triples = []
    for n in range(12000):
        a, b = np.float32(rnd.gauss(0, 1)), np.float32(rnd.gauss(0, 1))
        kind = n % 3
        if kind == 0:
            c = np.float32(rnd.gauss(0, 1) * 2.0 ** rnd.randint(-6, 10))
        elif kind == 1:
            c = np.float32(-float(a) * float(b) * (1.0 + rnd.gauss(0, 1) * 2.0 ** -rnd.randint(1, 24)))   # cancelling
        else:
            c = np.float32(float(a) * float(b) * 2.0 ** rnd.randint(20, 30))                           # product below acc's ulp
        triples.append((a, b, c))
    assert _fma_check(triples, R.fma_f64) == 0
    hard = _double_rounding_triples()
    assert _fma_check(hard, R.fma_f64) == 0
    wrong = _fma_check(hard, R.fma_double_rounded)
    print(f"fmaf emulation: 0 of {len(triples) + len(hard)} triples differ from Fraction; the plain f64 sum cast to f32 "
          f"is wrong on {wrong} of the {len(hard)} constructed triples")
    assert wrong == len(hard)  # the mutant `plain double-rounded fma` fails here, not under P0


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
def _report(label, mutants):
    for name, (fails, equals) in sorted(mutants.items()):
        print(f"{label} mutant {name}: fails on {fails[0] if fails else '-'} ({len(fails)} cases); equal to the honest "
              f"form on: {', '.join(equals) if equals else 'none'}")
        assert fails, f"{label}: mutant {name} passes every case"


def test_gemm_case_table_serves_its_purposes():
    by = {c["name"]: c for c in R.GEMM_CASES}
    M, N, K = R.E_SHAPES[(1, 1)]
    assert K % R.FK == 11 and K % 4 and R.E_SHAPE[0] % 4 and R.E_SHAPE[2] % R.FK == 8
    assert (-(-M // R.FB), -(-N // R.FB)) == (3, 2) and N % R.FB == 8
    groups = {c["M"]: (-(-c["M"] // R.FB)) for c in R.GEMM_CASES if c["name"].startswith("grp")}
    assert groups == {1030: 9, 1400: 11, 2100: 17} and [t % 8 for t in groups.values()] == [1, 3, 1]
    assert sorted({-(-c["N"] // R.FB) for c in R.GEMM_CASES if c["beta1"]}) == [1, 2, 3]
    assert {c["K"] for c in R.GEMM_CASES if c["name"].startswith("K") and c["al"]} == {1, 3, 15, 16, 17, 32, 33}
    assert by["one-11"]["K"] == 5 and by["tile+1"]["M"] == 129
    for c in R.GEMM_CASES:  # every case is one the library accepts (gemm_impl's shared checks)
        assert c["N"] % 8 == 0 and (c["al"] == 0 or c["M"] % 8 == 0) and ((c["al"], c["bl"]) == (1, 1) or c["K"] % 8 == 0)
    # every tile exactly once in the grouped order
    for tm in (1, 3, 8, 9, 11, 17):
        for tn in (1, 2, 3):
            order = R.tile_order(tm, tn)
            assert sorted(order) == [(r, c) for r in range(tm) for c in range(tn)]


def test_gemm_product_gates_pass_honest_and_fail_mutants():
    mutants = {m: ([], []) for m in R.GEMM_PRODUCT_MUTANTS}
    worst_p1 = 0.0
    for c in R.GEMM_CASES:
        M, N, K = c["M"], c["N"], c["K"]
        d = R.gemm_inputs(c["name"], M, N, K, c["al"], c["bl"])
        chain = R.fma_chain(d["Amk"], d["Bnk"])
        honest, visits = R.product_honest(d, M, N, K)
        assert R.ndiff(honest, chain) == 0 and bool((visits == 1).all()), c["name"]          # P0
        ref, absprod = R.product_ref(d["Amk"], d["Bnk"])
        w, rel, fin = R.g1(honest, ref, absprod, K)                                        # P1
        worst_p1 = max(worst_p1, w)
        assert w <= 1.0 and rel <= 1e-5 and fin, (c["name"], w, rel)
        grouped = c["name"].startswith("grp")
        if grouped:
            want = R.epilogue_replay(chain, beta=1.0, old=d["old"])[0]
            assert R.ndiff(R.beta_in_place(honest, visits, d["old"], 1.0), want) == 0
        for m in R.GEMM_PRODUCT_MUTANTS:
            if grouped != (m in ("gsize_8", "tile_swapped")):
                continue  # the order mutants on the grouped cases, the K mutants on the small ones
            got, vis = R.product_honest(d, M, N, K, mutant=m)
            differs = R.ndiff(got, chain) > 0
            if grouped:  # and under beta = 1: a tile visited twice or never
                differs = differs or R.ndiff(R.beta_in_place(got, vis, d["old"], 1.0), want) > 0
            p1_fails = not R.g1_ok(got, ref, absprod, K)
            if m == "pairwise":
                # another summation order is inside P1 by construction (the bound of ANY order): only P0 sees it
                assert not p1_fails or K < 2
            mutants[m][0 if differs else 1].append(c["name"])
    print(f"gemm_f32 honest: P0 0 differing bits on {len(R.GEMM_CASES)} cases, P1 worst err/gate {worst_p1:.3f}")
    _report("gemm_f32 product", mutants)
    # where the K mutants are the honest form: no tail (K a multiple of 16), or a single term (pairwise)
    assert set(mutants["tail_dropped"][1]) == set(mutants["tail_unguarded"][1]) == \
        {c["name"] for c in R.GEMM_CASES if c["K"] % R.FK == 0 and not c["name"].startswith("grp")}
    assert mutants["pairwise"][1] == ["K1-11"]
    assert all(n.endswith("x40") for n in mutants["gsize_8"][1])  # tiles_n = 1: (x % 8, x // 8) = (0, 0) either way


def _epi_kw(d, o, M, N, keep):
    kw = dict(alpha=o.get("alpha", 1.0), beta=o.get("beta", 0.0))
    if o.get("drop"):
        kw.update(keep=keep, p=o["drop"])
    for k in ("bias", "addend", "residual"):
        if o.get(k):
            kw[k] = d[k]
    if kw["beta"]:
        kw["old"] = d["old"]
    return kw


def test_gemm_epilogue_gates_pass_honest_and_fail_mutants():
    M, N, K = R.E_SHAPE
    d = R.gemm_inputs("E-00", M, N, K, 0, 0)
    c32 = R.fma_chain(d["Amk"], d["Bnk"])
    keep = R.keep_mask(R.DROP_SEED, M, N, 0.5)
    ldc = N + 8
    mutants = {m: ([], []) for m in R.GEMM_EPI_MUTANTS}
    worst_p3 = {}

    def outcome(name, o, mutant=None):
        """True if the launch restated with `mutant` fails a gate of variant `name`"""
        kw = _epi_kw(d, o, M, N, keep)
        act = o.get("act", R.ACT_NONE)
        out, pre, cbuf, pbuf = R.epilogue_honest(c32, N, ldc, want_preact=bool(o.get("preact")), act=act, mutant=mutant,
                                                 **kw)
        bad = not R.frame_untouched(cbuf, M, N) or (pbuf is not None and not R.frame_untouched(pbuf, M, N))
        if act == R.ACT_NONE:
            want, wpre = R.epilogue_replay(c32, **kw)
            bad = bad or R.ndiff(out, want) > 0 or (pre is not None and R.ndiff(pre, wpre) > 0)
            return bad, 0.0
        res = kw.pop("residual")
        _, wpre = R.epilogue_replay(c32, **kw)
        bad = bad or R.ndiff(pre, wpre) > 0
        w = R.p3_act(out, wpre, act, res)
        return bad or w > 2.0, w

    for name, o in list(R.EPI_P2.items()) + list(R.EPI_P3.items()):
        bad, w = outcome(name, o)
        assert not bad and w <= 1.0, (name, w)
        if name in R.EPI_P3:
            worst_p3[name] = w
        for m in R.GEMM_EPI_MUTANTS:
            mutants[m][0 if outcome(name, o, m)[0] else 1].append(name)
    print("gemm_f32 epilogue honest: 0 differing bits under P2; P3 worst err/gate " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst_p3.items()))
    _report("gemm_f32 epilogue", mutants)
    assert set(mutants["preact_ld_n"][0]) == {n for n, o in {**R.EPI_P2, **R.EPI_P3}.items() if o.get("preact")}
    assert "beta1" in mutants["beta_on_new"][1] and "beta025" in mutants["beta_on_new"][0]  # 1 * v + old = v + 1 * old


def test_gemm_dropout_gates_pass_honest_and_fail_mutants():
    mutants = {m: ([], []) for m in R.GEMM_DROP_MUTANTS}
    worst_p3 = 0.0
    for name, mode, T, F, p in R.DROP_CASES:
        M, N, K, al, bl = R.drop_dims(mode, T, F)
        d = R.gemm_inputs(name, M, N, K, al, bl)
        keep = R.keep_mask(R.DROP_SEED, T, F, p)
        share = keep.float().mean().item()
        assert abs(share - (1 - p)) < 0.02, (name, share)
        plain = R.fma_chain(d["Amk"], d["Bnk"])

        def result(kp):
            if mode == 1:
                return R.product_honest(d, M, N, K, a_drop=(kp, p))[0]
            if mode == 2:
                return R.product_honest(d, M, N, K, b_drop=(kp.T, p))[0]
            return R.epilogue_honest(plain, N, N + 8, keep=kp, p=p)[0]
        got = result(keep)
        if mode == 1:
            assert R.ndiff(got, R.fma_chain(R.dropped_operand(d["Amk"], keep, p), d["Bnk"])) == 0      # P4
        elif mode == 2:
            assert R.ndiff(got, R.fma_chain(d["Amk"], R.dropped_operand(d["Bnk"], keep.T, p))) == 0
        elif p == 0.5:
            assert R.ndiff(got, R.epilogue_replay(plain, keep=keep, p=p)[0]) == 0                      # P2
        else:
            w, nz = R.p3_drop(got, plain, keep, p)                                                     # P3
            worst_p3 = max(worst_p3, w)
            assert w <= 1.0 and nz == 0, (name, w, nz)
        for m in R.GEMM_DROP_MUTANTS:
            km = R.keep_mask(R.DROP_SEED, T, F, p, mutant=m)
            differs = not torch.equal(km, keep) and R.ndiff(result(km), got) > 0
            mutants[m][0 if differs else 1].append(name)
    print(f"gemm_f32 dropout honest: P4 0 differing bits, P3 (p = 0.25, 0.05) worst err/gate {worst_p3:.3f}")
    _report("gemm_f32 dropout", mutants)
    assert not mutants["drop_swapped"][1]


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
def _fwd_figures(c, r, o, lse):
    """{gate: err / gate}; exact-zero, +inf and finiteness failures count as inf"""
    f = {"O": R.worst(o.double() - r["O"], R.o_gate(r, c))}
    err, bad_inf = R.lse_check(lse, r)
    f["LSE"] = float("inf") if bad_inf else (0.0 if err is None else err / 1e-5)
    f["lse_err"] = err
    zeros = R.zero_checks(c, r, o=o)
    f["zeros"] = float("inf") if any(zeros.values()) or not bool(torch.isfinite(o.float()).all()) else 0.0
    return f


def _bwd_figures(c, r, bw, dq, dk, dv):
    f = {k: R.worst(t.double() - bw[k], bw[k + "_gate"]) for k, t in (("dQ", dq), ("dK", dk), ("dV", dv))}
    zeros = R.zero_checks(c, r, dq=dq, dk=dk, dv=dv)
    fin = all(bool(torch.isfinite(t.float()).all()) for t in (dq, dk, dv))
    f["zeros"] = float("inf") if any(zeros.values()) or not fin else 0.0
    return f


def _fails(f):
    return any(v is not None and v > 2.0 for k, v in f.items() if k != "lse_err")


def test_attention_case_table_serves_its_purposes():
    names = [c["name"] for c in R.ATTN_CASES]
    assert len(set(names)) == len(names)
    full = [c for c in R.ATTN_CASES if (c["D"], c["dtype"]) == (32, F32)]
    # a wholly masked first key block, a sequence with nothing live, causal queries below kv_start
    c = next(x for x in full if x["name"].startswith("ks65-129c"))
    vis = R.visibility(c)
    assert not vis[1, :, :R.KB].any() and vis[1].any() and not vis[1, :129].any(-1).any()
    c = next(x for x in full if x["name"].startswith("ks130-131-"))
    assert not R.visibility(c)[1].any() and R.visibility(c)[0, :, 130].all()
    # cached: the first queries of sequence 1 see nothing; ragged: the early-out block, kv_len >= Lq - q_pad
    c = next(x for x in full if x["name"].startswith("cached-33-63"))
    live = R.visibility(c).any(-1)
    assert live[0].all() and not live[1, :4].any() and live[1, 4:].all()  # 63 + i >= 67
    for c in full:
        if c["kind"] == "ragged":
            assert all(kl >= c["Lq"] - qp for kl, qp in zip(c["kv_len"], c["q_pad"])), c["name"]
            assert not R.visibility(c).any(-1)[1, :c["q_pad"][1]].any()
    # rising: the row maximum rises in every block for most rows (every block rescales)
    c = next(x for x in full if x["name"].startswith("rising-"))
    q, k, v, do = R.attn_inputs(c)
    r = R.attn_ref(q, R.kv_rows(c, k), R.kv_rows(c, v), c, R.visibility(c))
    bm = torch.stack([r["S"][..., k0:k0 + R.KB].max(-1).values for k0 in range(0, c["Lk"], R.KB)], -1)
    assert (bm.diff(dim=-1) > 0).all(-1).double().mean() > 0.6
    c = next(x for x in full if x["name"].startswith("planted-"))
    q, k, v, do = R.attn_inputs(c)
    r = R.attn_ref(q, R.kv_rows(c, k), R.kv_rows(c, v), c, R.visibility(c))
    assert (r["S"].argmax(-1) == c["Lk"] - 1).double().mean() > 0.95


def test_attention_gates_pass_honest_and_fail_mutants():
    honest = {}
    fwd_m = {m: ([], []) for m in R.FWD_MUTANTS}
    bwd_m = {m: ([], []) for m in R.BWD_MUTANTS}
    lse_errs = []
    for c in R.ATTN_CASES:
        full = (c["D"], c["dtype"]) in ((32, F32), (16, BF))
        q, k, v, do = R.attn_inputs(c)
        kk, vv = R.kv_rows(c, k), R.kv_rows(c, v)
        r = R.attn_ref(q, kk, vv, c, R.visibility(c))
        o, lse = R.fwd_honest(q, kk, vv, c)
        f = _fwd_figures(c, r, o, lse)
        if f["lse_err"] is not None:
            lse_errs.append(f["lse_err"])
        for g in ("O", "LSE", "zeros"):
            honest[g] = max(honest.get(g, 0.0), f[g])
            assert f[g] <= 1.0, (c["name"], g, f[g])
        if full:
            for m in R.FWD_MUTANTS:
                fm = _fwd_figures(c, r, *R.fwd_honest(q, kk, vv, c, mutant=m))
                fwd_m[m][0 if _fails(fm) else 1].append(c["name"])
        if c["kind"] != "packed":
            continue
        o_st, lse32 = r["O"].to(c["dtype"]), r["LSE"].float()
        bw = R.bwd_ref(r, c, do, o_st, lse32)
        f = _bwd_figures(c, r, bw, *R.bwd_honest(q, kk, vv, o_st, do, lse32, c))
        for g, w in f.items():
            honest[g] = max(honest.get(g, 0.0), w)
            assert w <= 1.0, (c["name"], g, w)
        if full:
            for m in R.BWD_MUTANTS:
                fm = _bwd_figures(c, r, bw, *R.bwd_honest(q, kk, vv, o_st, do, lse32, c, mutant=m))
                bwd_m[m][0 if _fails(fm) else 1].append(c["name"])
    assert 0.0 < max(lse_errs) <= 1e-5
    print("attention honest, worst err/gate: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(honest.items())) +
          f"; LSE max|err| {max(lse_errs):.2e}")

    def short(m):  # the equal lists are long: name the count and the first few
        return {k: (f, e[:6] + ([f"... {len(e)} in all"] if len(e) > 6 else [])) for k, (f, e) in m.items()}
    _report("attention forward", short(fwd_m))
    _report("attention backward", short(bwd_m))
    # where the mask mutants must be the honest form
    assert all("cached" in n or "ragged" in n for n in fwd_m["past_omitted"][0] + fwd_m["v_below_start_read"][0])
    assert all("ragged" in n for n in fwd_m["qpad_unmasked"][0] + fwd_m["early_out_far"][0])
