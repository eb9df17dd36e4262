"""The bf16 MFMA attention forward per element against float64: attn_fwd_cached_k and attn_fwd_ragged_k
(csrc/attn_fwd_pipe_body.h) through ops.attn_fwd_cached / ops.attn_fwd_ragged on every case of
tests/mfma_attn_refs.py, and the packed instantiations (attn_fwd_pipe_k, stage 7; attn_fwd_k, stage 4) on a
handful of cases under the same gates. tests/test_mfma_attn_refs_host.py shows on the CPU, for these very
inputs, that an honest restatement passes every gate and that each listed mutant fails.

The caches hold NaN in every row at or above kv_len[b], in every row below kv_start[b] and in the slab's
padding columns; q rows below q_pad[b] are NaN. NaN in a cache row is data: nothing here can fault. Stats of
every case are appended to the stats file of tests/test_accuracy_gpu.py.
"""
import hashlib
import json
import os

import pytest
import torch

from tests import mfma_attn_refs as R
from tests.test_accuracy_gpu import _log as _append_stats

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mfma_attn_parent_bits.json")


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def _i32(x):
    return None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)


def _run(c, d, out=None):
    B, H, D, Lq = c["B"], c["H"], c["D"], c["Lq"]
    kw = dict(B=B, H=H, Lq=Lq, D=D, scale=c["scale"], kv_start=_i32(c["ks"]), out=out)
    if c["kind"] == "cached":
        return ops().attn_fwd_cached(d["q"], d["kc"], d["vc"], past=c["kv_len"][0] - Lq, **kw)
    if c["kind"] == "ragged":
        return ops().attn_fwd_ragged(d["q"], d["kc"], d["vc"], _i32(c["kv_len"]), q_pad=_i32(c["q_pad"]), **kw)
    return ops().attn_fwd(d["q"], d["k"], d["v"], Lk=c["cap"], causal=c["causal"], **kw)


def _check(c, test, extra=None):
    d = R.inputs(c, DEV)
    r = R.ref(d["q"], d["kc"], d["vc"], c)
    buf, out = R.out_block(c, DEV) if c["layout"] else (None, None)
    o, lse = _run(c, d, out)
    torch.cuda.synchronize()
    f = R.figures(c, r, o, lse)
    dead, masked = int((~r["live"]).sum()), int(R.poisoned_rows(c).sum())
    fails = []
    if (dead, masked) != R.COUNTS[c["name"]]:
        fails.append(f"dead queries / NaN key rows {(dead, masked)}, the table says {R.COUNTS[c['name']]}")
    if f["finite"]:
        fails.append("O is not finite: a masked (NaN) row reached the output")
    if f["zeros"]:
        fails.append("a dead query's O row is not exactly zero")
    if f["LSE"] > 1.0:
        fails.append(f"lse: max|err| {f['lse_err']}, or a dead row that is not +inf")
    if not f["O"] <= 1.0:
        fails.append(f"O err / gate {f['O']:.3f}")
    if not f["shrink"] <= 1.0:
        fails.append(f"O shrinks against the reference: |slope| / gate {f['shrink']:.3f}")
    if buf is not None and not R.frame_untouched(buf):
        fails.append("O written outside its column block")
    stats = {"test": test, "case": c["name"], "kind": c["kind"], "shape": [c["B"], c["H"], c["Lq"], c["cap"], c["D"]],
             "dead_query_rows": dead, "nan_key_rows": masked, "O": f["O"], "lse_max_err": f["lse_err"],
             "shrink": f["shrink"], "failures": fails}
    stats.update(extra or {})
    print(json.dumps(stats))
    _append_stats(stats)
    assert not fails, f"{c['name']} ({c['why']}): " + "; ".join(fails)
    return d, o, lse


@pytest.mark.parametrize("c", R.CASES, ids=[c["name"] for c in R.CASES])
def test_mfma_attention(c):
    d, o, lse = _check(c, "attn_mfma")
    if c["name"].startswith("ragged-uniform"):  # all rows uniform: bitwise the cached call
        oc, lc = _run(dict(c, kind="cached"), d)
        assert torch.equal(oc.view(torch.int16), o.view(torch.int16)) and torch.equal(lc, lse)


@pytest.fixture
def stage():
    from cullavo_amd import _lib
    prev = []

    def set_stage(s):
        prev.append(_lib.lib().cullavo_attn_set_stage(s))
    yield set_stage
    if prev:
        _lib.lib().cullavo_attn_set_stage(prev[0])


@pytest.mark.parametrize("st", (7, 4))
@pytest.mark.parametrize("c", R.PACKED, ids=[c["name"] for c in R.PACKED])
def test_mfma_attention_packed(c, st, stage):
    stage(st)
    _check(c, "attn_mfma_packed", {"stage": st})


def _finite(d):
    """the case's inputs with every NaN replaced by 1.25: a cache whose unpromised rows are finite"""
    for k in ("qbuf", "kslab", "vslab", "q"):
        if k in d:
            d[k].copy_(torch.nan_to_num(d[k].float(), nan=1.25).to(R.BF))
    return d


def bits(c):
    """sha256 of the bytes of O and LSE of case c on a finite cache"""
    d = _finite(R.inputs(c, DEV))
    o, lse = _run(c, d)
    torch.cuda.synchronize()
    return hashlib.sha256(o.contiguous().view(torch.int16).cpu().numpy().tobytes() + lse.cpu().numpy().tobytes()).hexdigest()


def test_finite_cache_bitwise_the_parent():
    """Zeroing the V rows below kv_start changes no bit where those rows were finite: they met P = 0 before and
    zeros now. tests/golden/mfma_attn_parent_bits.json holds the digests of O and LSE that the kernels of the
    commit before the fix returned for every case (finite fill 1.25 where the poison was), on an MI355X."""
    with open(GOLDEN) as f:
        want = json.load(f)
    assert set(want) == {c["name"] for c in R.CASES}
    diff = [c["name"] for c in R.CASES if bits(c) != want[c["name"]]]
    assert not diff, f"outputs differ in bits from the parent's on a finite cache: {diff}"
