"""Every dispatch path and epilogue option of the bf16 GEMM (csrc/gemm.hip, csrc/gemm_common.h) per
element, at the smallest shapes at which each can still go wrong.

The case table, the references, the gates G1-G5 (with their derivations) and the NaN-framed inputs
are tests/gemm_refs.py; tests/test_gemm_refs_host.py shows on the CPU, for these very inputs, that an
honest restatement passes every gate and that each listed mutant fails. Each case asserts its route
(cullavo_gemm_plan under the case's forced tile, the split-K workspace), runs the f32 output once
against f64 (G1), then every epilogue variant of the case against the bit-exact replay of the
documented chain on that f32 product (G2), the activations by round-or-neighbour (G3), the
SwiGLU-backward epilogue against ops.swiglu_bwd (G4) and the fused LoRA against the unfused addend
(G5). C, the pre-activation and the f32 C are views into sentinel frames; the operands are views
into NaN frames. Stats of every case are appended to the stats file of tests/test_accuracy_gpu.py.
"""
import ctypes
import json

import pytest
import torch

from tests import gemm_refs as R
from tests.test_accuracy_gpu import _log as _append_stats

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


class _Runner:
    """one case's launches: framed outputs, the frame checks collected in `fails`"""

    def __init__(self, c, d):
        self.c, self.d, self.fails = c, d, []

    def run(self, tag, dtype=BF, off=0, ncols=None, fill=None, want_preact=False, split_k=True, via_gemm=False, **kw):
        c, d = self.c, self.d
        M, N, K = c["M"], c["N"], c["K"]
        W = ncols or N
        buf, C = R.framed(M, W, dtype, DEV, off, fill)
        pbuf = pre = None
        if want_preact:
            pbuf, pre = R.framed(M, W, BF, DEV, off)
            kw["preact"] = pre
        if kw.get("residual") is not None:
            kw["ldr"] = kw["residual"].stride(0)
        if kw.get("addend") is not None:
            kw["ld_addend"] = kw["addend"].stride(0)
        A, B = d["A"], d["B"]
        if via_gemm:
            ops().gemm(c["al"], c["bl"], M, N, K, A, A.stride(0), B, B.stride(0), C, C.stride(0), **kw)
        else:
            ops().gemm_ex(c["al"], c["bl"], M, N, K, A, A.stride(0), B, B.stride(0), C, C.stride(0), split_k=split_k,
                          **kw)
        torch.cuda.synchronize()
        if not R.frame_untouched(buf, M, W, off):
            self.fails.append(f"{tag}: C written outside its [M, N] view")
        if pbuf is not None and not R.frame_untouched(pbuf, M, W, off):
            self.fails.append(f"{tag}: pre-activation written outside its [M, N] view")
        return C, pre


def _options(d, o, off=0):
    kw = {}
    if o.get("alpha"):
        kw["alpha"] = o["alpha"]
    if o.get("bias"):
        kw["bias"] = d["bias"]
    if o.get("addend"):
        kw["addend"] = d["addend"]
    if o.get("residual"):
        kw["residual"] = d["residual4"] if off else d["residual"]
    return kw


def _replay_kw(kw):
    return {k: v for k, v in kw.items() if k in ("alpha", "bias", "addend", "residual")}


def _variant(r, v, c32, stats):
    """runs variant v of r's case; mismatch counts into stats, failures into r.fails"""
    c, d = r.c, r.d
    M, N, K = c["M"], c["N"], c["K"]
    o = R.VARIANTS[v]
    act = o.get("act", R.ACT_NONE)
    nd = {}
    if act == R.ACT_SWIGLU_BWD:  # G4
        gu = d["gu"]
        y, _ = r.run(v, ncols=2 * N, act=act, residual=gu)
        want = ops().swiglu_bwd(c32.to(BF), gu.contiguous())
        nd["g4"] = R.ndiff(y, want)
    elif o.get("lora"):  # G5
        width, n_mod = c["width"], c["n_mod"]
        u, bst = d["u"], d["bst"]
        t = torch.empty((M, N), dtype=BF, device=DEV)
        t32 = torch.empty((M, width), dtype=F32, device=DEV)
        worst_t = 0.0
        for m in range(n_mod):
            um, bm = u[:, m * R.LORA_R:(m + 1) * R.LORA_R], bst[m * width:(m + 1) * width]
            tm = t[:, m * width:(m + 1) * width]
            ops().gemm_ex(0, 0, M, width, R.LORA_R, um, um.stride(0), bm, R.LORA_R, tm, N, alpha=R.LORA_SCALE, split_k=False)
            ops().gemm_ex(0, 0, M, width, R.LORA_R, um, um.stride(0), bm, R.LORA_R, t32, width, alpha=R.LORA_SCALE,
                          split_k=False)
            ref, absprod = R.product_ref(um, bm)
            w, rel, fin = R.g1(t32, ref, absprod, R.LORA_R, R.LORA_SCALE)
            worst_t = max(worst_t, w)
            if not (w <= 1.0 and rel <= 1e-5 and fin):
                r.fails.append(f"{v}: addend product of module {m}: G1 {w:.3f}, rel-L2 {rel:.2e}")
            nd[f"t{m}"] = R.ndiff(tm, t32.to(BF))
        stats["lora_addend_err_over_gate"] = worst_t
        kw = _options(d, o)
        pre_on = bool(o.get("preact"))
        y, pre = r.run(v, want_preact=pre_on, act=act, lora=(u, bst, width, R.LORA_SCALE), **kw)
        y2, pre2 = r.run(v + "/unfused", want_preact=pre_on, act=act, addend=t, split_k=False, **kw)
        nd["g5"] = R.ndiff(y, y2)
        if pre_on:
            nd["g5_preact"] = R.ndiff(pre, pre2)
    elif act == R.ACT_NONE:  # G2
        off = o.get("off", 0)
        kw = _options(d, o, off)
        dt = F32 if o.get("f32") else BF
        beta = o.get("beta", 0.0)
        fill = d["old"].to(dt) if beta else None
        pre_on = bool(o.get("preact"))
        # the plain product through ops.gemm, which hands a workspace to plan 9 and the plan's splits only:
        # the 128x128 split-K cases (plan 0) stay on gemm_ex, the route of their f32 product
        via_gemm = v == "plain" and not (c.get("workspace") and c["plan"] == 0)
        y, pre = r.run(v, dtype=dt, off=off, fill=fill, want_preact=pre_on, beta=beta, via_gemm=via_gemm, **kw)
        want, wpre = R.chain_replay(c32, want_preact=pre_on, beta=beta, old=fill, out_dtype=dt, **_replay_kw(kw))
        nd["g2"] = R.ndiff(y, want)
        if pre_on:
            nd["g2_preact"] = R.ndiff(pre, wpre)
        if off:  # the same options with every operand 16-byte aligned: the same bits
            y0, pre0 = r.run(v + "/aligned", want_preact=pre_on, **_options(d, o))
            nd["aligned"] = R.ndiff(y, y0) + R.ndiff(pre, pre0)
    else:  # G3
        kw = _options(d, o)
        res = kw.pop("residual", None)
        pre_on = bool(o.get("preact"))
        y_act, pre = r.run(v, want_preact=pre_on, act=act, **kw)
        _, wpre = R.chain_replay(c32, rounds=True, **_replay_kw(kw))
        if pre_on:
            nd["g2_preact"] = R.ndiff(pre, wpre)
        nd["g3"], amb = R.act_check(y_act, wpre, act)
        stats.setdefault("ambiguous_share", {})[v] = amb
        if amb > R.AMBIGUOUS_CAP:
            r.fails.append(f"{v}: ambiguous share {amb:.4f} over the cap")
        if res is not None:
            y, pre = r.run(v + "/residual", want_preact=pre_on, act=act, residual=res, **kw)
            nd["g3_residual"] = R.ndiff(y, (y_act.float() + res.float()).to(BF))
            nd["g2_preact_residual"] = R.ndiff(pre, wpre)
    stats["bits_differing"][v] = nd
    r.fails += [f"{v}: {k}: {n} elements differ" for k, n in nd.items() if n]


@pytest.mark.parametrize("c", R.CASES, ids=[c["name"] for c in R.CASES])
def test_gemm_path(c):
    L = _lib()
    M, N, K, al, bl = c["M"], c["N"], c["K"], c["al"], c["bl"]
    prev_tile = L.cullavo_gemm_set_tile(c["tile"])
    prev_epi = L.cullavo_gemm_set_epilogue(1)
    try:
        # the route
        grid = ctypes.c_int64(0)
        plan = L.cullavo_gemm_plan(M, N, K, al, bl, ctypes.byref(grid))
        assert plan == c["plan"], f"{c['name']}: plan {plan}, the table says {c['plan']} ({c['route']})"
        dsc = ops().GemmDesc(al, bl, M, N, K, None, 8, None, 8, None, N, 1, 1.0)
        ws = L.cullavo_gemm_workspace(ctypes.addressof(dsc))
        assert bool(ws) == bool(c.get("workspace")), f"{c['name']}: split-K workspace {ws}"
        if "tiles" in c:
            assert grid.value == c["tiles"] > torch.cuda.get_device_properties(0).multi_processor_count
        d = R.case_inputs(c, DEV)
        ref, absprod = R.product_ref(d["Amk"], d["Bnk"])
        r = _Runner(c, d)
        c32, _ = r.run("f32", dtype=F32)
        w, rel, fin = R.g1(c32, ref, absprod, K)
        stats = {"test": "gemm_paths", "case": c["name"], "shape": [M, N, K], "layouts": [al, bl], "tile": c["tile"],
                 "plan": plan, "err_over_f32_bound": w, "rel_l2_f32": rel, "bits_differing": {}}
        if not (w <= 1.0 and rel <= 1e-5 and fin):
            r.fails.append(f"f32 output: err / (K 2^-24 |A||B|^T) {w:.3f}, rel-L2 {rel:.2e}, finite {fin}")
        for v in c["variants"]:
            _variant(r, v, c32, stats)
    finally:
        L.cullavo_gemm_set_tile(prev_tile)
        L.cullavo_gemm_set_epilogue(prev_epi)
    stats["failures"] = r.fails
    _log(stats)
    assert not r.fails, f"{c['name']} (tile {c['tile']}, {c['route']}): " + "; ".join(r.fails)
