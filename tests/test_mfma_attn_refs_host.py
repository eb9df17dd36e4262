"""The gates of tests/mfma_attn_refs.py discriminate, shown on the CPU before any GPU time is spent.

For every case of tests/test_mfma_attn_accuracy_gpu.py (same seeds, shapes, frames and poison) the honest
restatement of attn_fwd_pipe_body.h stays at or below 1.0 of every gate; each mutant of R.MUTANTS exceeds 2.0,
or breaks an exact-zero / +inf / finiteness check, on at least one case. Run with -s for the per-case honest
ratios and, per mutant, a case on which it fails.
"""
import json

import torch

from tests import mfma_attn_refs as R
from tests.test_parity_refs_host import _report

_cache = {}


def _setup(c):
    """(inputs, f64 reference) of a case, built once"""
    if c["name"] not in _cache:
        d = R.inputs(c)
        _cache[c["name"]] = (d, R.ref(d["q"], d["kc"], d["vc"], c))
    return _cache[c["name"]]


def _fails(f):
    return any(v is not None and v > 2.0 for k, v in f.items() if k != "lse_err")


def test_case_table_serves_its_purposes():
    names = [c["name"] for c in R.CASES + R.PACKED]
    assert len(set(names)) == len(names) and set(names) == set(R.COUNTS)
    for c in R.CASES + R.PACKED:
        assert R.counts(c) == R.COUNTS[c["name"]], (c["name"], R.counts(c))
        assert c["cap"] <= 400 and c["B"] * c["Lq"] <= 400
    for D in (128, 64):
        cs = [c for c in R.CASES if c["D"] == D]
        for Lq in (2, 33, 130):  # every kv_start value of the issue, per Lq, relative to the case's own past
            kinds = set()
            for c in cs:
                if c["kind"] == "cached" and c["struct"] == "random" and c["Lq"] == Lq:
                    past = c["kv_len"][0] - Lq
                    assert c["name"].startswith(f"cached-{Lq}-{past}-")
                    vals = R._ks_values(past, Lq)
                    kinds |= {i for i, v in enumerate(vals) for k in c["ks"] if k == min(max(v, 0), past + Lq)}
            assert kinds == set(range(10)), (D, Lq, kinds)
        assert {c["kv_len"][0] - c["Lq"] for c in cs if c["kind"] == "cached" and c["struct"] == "random"} == set(R.PASTS)
        rag = [c for c in cs if c["kind"] == "ragged" and c["struct"] == "random"]
        assert {p for c in rag for p in c["q_pad"]} >= {0, 1, 63, 64, 70, 127, 128, 129, 130}
        offs = {kl - c["Lq"] for c in rag for kl in c["kv_len"]}
        assert offs >= {-5, 0, 63, 64, 65} and any(0 in c["kv_len"] for c in rag)
        assert any(kl > c["cap"] for c in rag for kl in c["kv_len"])            # the clamp
        assert any(kl - c["Lq"] < -c["q_pad"][b] for c in rag for b, kl in enumerate(c["kv_len"]) if kl)
        # a sequence with nothing live, queries with no live key beside live ones, whole padding query tiles
        assert any(not R.live_mask(c)[b].any() for c in cs for b in range(c["B"]) if c["kind"] == "cached")
        assert any(c["Lq"] > 128 and min(c["q_pad"]) < 128 <= max(c["q_pad"]) for c in rag)
    # the four kinds of poison stand together in one case
    c = next(x for x in R.CASES if x["name"] == "ragged-130-p64-D128")
    d = R.inputs(c)
    b = next(b for b in range(c["B"]) if c["q_pad"][b] and c["ks"][b] and R.eff_len(c, b) < c["cap"])
    assert torch.isnan(d["q"][b * c["Lq"]].float()).all() and torch.isnan(d["kslab"][..., -R.PAD_COLS:].float()).all()
    assert torch.isnan(d["vc"][b, c["ks"][b] - 1].float()).all() and torch.isnan(d["vc"][b, R.eff_len(c, b)].float()).all()
    assert torch.isfinite(d["vc"][b, c["ks"][b]:R.eff_len(c, b)].float()).all()
    # planted: the key holds p within (0.3, 0.7) for a tenth or more of the queries that see it (the earliest
    # queries of a sequence see few keys beside it, so p nears 1 there); a masked plant is seen by none
    for c in R.CASES:
        if c["struct"] != "planted":
            continue
        d, r = _setup(c)
        for b in range(c["B"]):
            pos = R.plant_pos(c, b)
            seen = r["vis"][b, :, pos]
            assert bool(seen.any()) == (c["plant"] != "ks-1"), (c["name"], b)
            assert torch.isfinite(d["kc"][b, pos].float()).all()
            if seen.any():
                p = r["P"][b, :, seen, pos]
                assert ((p > 0.3) & (p < 0.7)).double().mean() > 0.1 and p.median() > 0.2, (c["name"], b, p.median().item())
            if c["plant"] in ("mid+1", "edge+1"):  # the query on the diagonal's other side exists
                assert not seen.all() and pos % R.KT == (31 if c["plant"] == "mid+1" else 0)
    # rising: the tile maximum climbs by more than the rescale threshold from tile to tile
    c = next(x for x in R.CASES if x["name"] == "cached-rising-D128")
    d, r = _setup(c)
    S = r["S"].masked_fill(~r["vis"][:, None], float("-inf"))[0, :, -1] * R.LOG2E   # the last query of sequence 0
    tm = torch.stack([S[:, k0:k0 + R.KT].max(-1).values for k0 in range(128, 320, R.KT)], -1)
    assert (tm.diff(dim=-1) > R.THR).all()


def test_gates_pass_honest_and_fail_mutants():
    honest, lse_errs, worst_shrink = {}, [], 0.0
    mut = {m: ([], []) for m in R.MUTANTS}
    for c in R.CASES:
        d, r = _setup(c)
        o, lse = R.fwd_honest(d["q"], d["kc"], d["vc"], c)
        f = R.figures(c, r, o, lse)
        honest[c["name"]] = round(f["O"], 4)
        if f["lse_err"] is not None:
            lse_errs.append(f["lse_err"])
        for g in ("O", "LSE", "zeros", "finite", "shrink"):
            assert f[g] <= 1.0, (c["name"], g, f[g])
        worst_shrink = max(worst_shrink, f["shrink"])
        for m in R.EQUIVALENT:
            om, lm = R.fwd_honest(d["q"], d["kc"], d["vc"], c, mutant=m)
            assert torch.equal(om.view(torch.int16), o.view(torch.int16)) and torch.equal(lm, lse), (c["name"], m)
        for m in R.MUTANTS:
            fm = R.figures(c, r, *R.fwd_honest(d["q"], d["kc"], d["vc"], c, mutant=m))
            mut[m][0 if _fails(fm) else 1].append(c["name"])
    assert 0.0 < max(lse_errs) <= 1e-5
    print("mfma attention honest, O worst err/gate per case: " + json.dumps(honest))
    print(f"mfma attention honest: worst O err/gate {max(honest.values()):.3f} ({max(honest, key=honest.get)}), "
          f"LSE max|err| {max(lse_errs):.2e}, worst |shrink| / gate {worst_shrink:.3f}")

    def short(m):
        return {k: (f, e[:4] + ([f"... {len(e)} in all"] if len(e) > 4 else [])) for k, (f, e) in m.items()}
    _report("mfma attention", short(mut))
    assert len(R.MUTANTS) >= 14
    by = {c["name"]: c for c in R.CASES}
    # the parent's 0 x V: it fails on, and only on, cases whose kv_start sits inside a tile
    z = mut["zero_times_v"][0]
    assert len(z) >= 40 and all(any(k % R.KT for k in by[n]["ks"]) for n in z)
    # each mask edge is caught by a planted key at that edge, by the size of the leak and not by a NaN
    assert any("plant-ks-1" in n for n in mut["ks_m1"][0])
    assert any("plant-mid+1" in n for n in mut["diag_p1"][0]) and any("plant-edge+1" in n for n in mut["diag_p1"][0])
    assert any("plant-last" in n for n in mut["kvlen_m1"][0])
    assert len(mut["p_truncated"][0]) >= 20   # the shrink gate (the mean loss varies with the mantissas met)
    assert all(by[n]["kind"] == "ragged" for n in mut["qpad_m1"][0] + mut["kvlen_unclamped"][0])


def test_packed_cases_pass_honest():
    """the packed cases of the GPU test under the same gates: the restatement with past = 0 (causal); the
    non-causal ones are held by the f64 reference alone"""
    for c in R.PACKED:
        d = R.inputs(c)
        r = R.ref(d["q"], d["kc"], d["vc"], c)
        assert R.counts(c) == R.COUNTS[c["name"]]
        if c["causal"]:
            f = R.figures(c, r, *R.fwd_honest(d["q"], d["kc"], d["vc"], c, fixed=False))
            assert all(f[g] <= 1.0 for g in ("O", "LSE", "zeros", "finite")), (c["name"], f)
