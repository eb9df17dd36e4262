"""The gates of tests/cycle_refs.py discriminate, shown on the CPU before any GPU time is spent: the
honest accumulation of the bf16-faithful oracle's gradients over the micro-batch sequences, and the
honest teacher-forced AdamW cycle over them, stay within 1.0 of every gate on every parameter; each
one-line mutant exceeds 2.0 on at least one parameter of at least one sequence. A sequence on which a
mutant coincides with the honest form is named, not skipped. The inputs are checked for the edges they
were chosen for. Run with -s for the figures."""
import functools

import torch

from tests import cycle_refs as C
from tests.test_train_refs_host import _assert_mutants, _record

BF, F32 = torch.bfloat16, torch.float32
HOST_SEQUENCES = dict(C.SEQUENCES, C=("C",))   # the C-only cycle: every projector key unreached


@functools.lru_cache(maxsize=None)
def _singles():
    """{batch: {key: bf16 oracle gradient or None}} over the full recipe's trainable keys"""
    batches = C.make_batches()
    out = {}
    for name, b in batches.items():
        g = C.oracle_grads(b)
        out[name] = {k: v for k, v in g.items() if k.startswith(C.TRAINABLE_PREFIXES["full"])}
    return out


def _terms(name):
    g = _singles()[name]
    return {k: (v if v is not None and C.reaches(k, name) else None) for k, v in g.items()}


def _unrounded(name):
    """a t_k that rounds to g_k: g_k (1 + 0.49 U r), r uniform in [-1, 1] (within half a bf16 ulp)"""
    gen = torch.Generator().manual_seed(7)
    return {k: v.float() * (1 + 0.49 * C.U * (2 * torch.rand(v.shape, generator=gen) - 1))
            for k, v in _terms(name).items() if v is not None}


@functools.lru_cache(maxsize=None)
def _stale():
    """what a completed (A, B) cycle leaves in the buffers"""
    return C.accumulate_honest([_terms("A"), _terms("B")], {k: torch.zeros(v.shape) for k, v in _singles()["A"].items()})[0][-1]


def _gate_sequence(seq, mutant=None, unrounded=False, scale=1.0):
    """worst over the keys of (first-write, total) for one sequence"""
    terms = [_terms(n) for n in seq]
    snaps, skipped = C.accumulate_honest(terms, _stale(), mutant, [_unrounded(n) for n in seq] if unrounded else None,
                                         scale)
    worst = 0.0
    for k in snaps[-1]:
        g = [(t[k].float() if t[k] is not None else torch.zeros_like(snaps[-1][k])) for t in terms]
        if all(t[k] is None for t in terms):
            ok = C.unreached_ok(snaps[-1][k], k in skipped)
            worst = max(worst, 0.0 if ok else float("inf"))
            continue
        first, total = C.accum_gates([s[k] for s in snaps], g, scale)
        worst = max(worst, first, total)
    return worst


def test_inputs_hold_their_edges():
    s = _singles()
    for k, g in s["C"].items():
        if k.startswith("multi_modal_projector."):
            assert g is None or float(g.float().abs().max()) == 0.0, k
            assert not C.reaches(k, "C")
    for name in ("A", "B"):
        for recipe, pre in C.TRAINABLE_PREFIXES.items():
            for k, g in s[name].items():
                if k.startswith(pre):
                    assert g is not None and float(g.float().abs().max()) > 0.0, (recipe, name, k)
    for k, g in s["C"].items():   # the text-only batch reaches every language-model key
        if k.startswith("language_model."):
            assert g is not None and float(g.float().abs().max()) > 0.0, k
    b = C.make_batches()
    assert b["B"][1][1, -9:].sum() == 0 and b["B"][1][0].all() and b["C"][2] is None
    assert (b["C"][0] != 1000).all()


def test_accumulation_gate_passes_honest_and_fails_mutants():
    honest, mutants, coincide = {}, {}, []
    for sname, seq in HOST_SEQUENCES.items():
        _record(honest, "rounded terms", _gate_sequence(seq))
        _record(honest, "unrounded terms", _gate_sequence(seq, unrounded=True))
        _record(honest, "mean of the cycle", _gate_sequence(seq, scale=1.0 / len(seq)) if len(seq) in (1, 2) else 0.0)
        for mu in C.ACCUM_MUTANTS:
            if mu == "sum_not_mean":
                if len(seq) != 2:
                    continue
                w = _gate_sequence(seq, mu, scale=0.5)
            else:
                w = _gate_sequence(seq, mu)
            _record(mutants, mu, w)
            if w <= 2.0:
                coincide.append((mu, sname, w))
    for mu, sname, w in coincide:
        print(f"accumulate: mutant {mu} coincides with the honest form on sequence {sname} ({w:.3f})")
    _assert_mutants(honest, mutants, "accumulate")
    # the sequences each mutant was chosen for
    assert _gate_sequence(HOST_SEQUENCES["C"], "stale_kept") > 2.0
    assert _gate_sequence(HOST_SEQUENCES["CA"], "first_write_adds") > 2.0


@functools.lru_cache(maxsize=None)
def _cycle_grads():
    """six accumulated gradients: the honest accumulation of UPDATE_CYCLES, scaled by a power of two per
    cycle (exact) so that the norms differ as they do once the weights move"""
    out = []
    for i, seq in enumerate(C.UPDATE_CYCLES):
        snaps, skipped = C.accumulate_honest([_terms(n) for n in seq], _stale())
        s = 2.0 ** (0, 1, -1, 0, 1, -1)[i]
        out.append(({k: (v * s).to(BF) for k, v in snaps[-1].items()}, set(snaps[-1]) - skipped))
    return out


def _max_norm():
    return C.median([C.norm64(list(g.values())) for g, _ in _cycle_grads()])


def test_reference_norms_straddle_max_norm():
    norms = [C.norm64(list(g.values())) for g, _ in _cycle_grads()]
    mx = _max_norm()
    assert any(n > mx * 1.01 for n in norms) and any(n < mx * 0.99 for n in norms), (norms, mx)
    assert not set(_cycle_grads()[2][1]) & {k for k in _singles()["A"] if k.startswith("multi_modal_projector.")}


def _run_cycles(pdt, sdt, mutant=None):
    W = {k: v.to(BF).to(pdt) for k, v in C.O.make_weights(C.O.config_small_gpu(), C.WEIGHT_SEED).items()
         if k in _singles()["A"]}
    state = {k: dict(p=v.clone(), m=torch.zeros(v.shape, dtype=sdt), v=torch.zeros(v.shape, dtype=sdt), step=0)
             for k, v in W.items()}
    mx = _max_norm()
    w, fails = {"m": 0.0, "v": 0.0, "p": 0.0}, []
    for i, (grads, reached) in enumerate(_cycle_grads()):
        recs, lr, coef, norm, sumsq = C.update_cycle_honest(state, grads, reached, i, i + 1, mx, sdt, mutant)
        own = {k: sum(1 for _, r in _cycle_grads()[:i + 1] if k in r) for k in recs}
        for k, r in recs.items():
            r["step"] = own[k]
        wi, fi = C.update_gates(recs, i, lr, coef, norm, sumsq, mx)
        w = {n: max(w[n], wi[n]) for n in w}
        fails += [f"cycle {i + 1}: {f}" for f in fi]
    return w, fails


# (parameter, moment) types: the two the GPU test runs, and f32 parameters, where a decay of
# lr wd = 1e-4 is visible (a bf16 parameter times 1 - 1e-4 rounds back to itself: under half an ulp)
UPDATE_TYPES = [(BF, BF), (BF, F32), (F32, F32)]


def test_update_gates_pass_honest_and_fail_mutants():
    honest, mutants = {}, {}
    for pdt, sdt in UPDATE_TYPES:
        label = f"{pdt}/{sdt}".replace("torch.", "")
        w, fails = _run_cycles(pdt, sdt)
        assert not fails, (label, fails)
        for n, x in w.items():
            _record(honest, f"{n} [{label}]", x)
        for mu in C.UPDATE_MUTANTS:
            w, fails = _run_cycles(pdt, sdt, mu)
            x = float("inf") if fails else max(w.values())
            _record(mutants, mu, x)
            print(f"update {label}: mutant {mu}: worst m/v/p {w['m']:.3g}/{w['v']:.3g}/{w['p']:.3g}, "
                  f"{len(fails)} exact checks failed" + (f" (first: {fails[0]})" if fails else ""))
            if x <= 2.0:
                print(f"update {label}: mutant {mu} coincides with the honest form at these types ({x:.3f})")
    _assert_mutants(honest, mutants, "update")
