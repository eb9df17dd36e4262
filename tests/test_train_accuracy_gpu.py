"""The training step's norm, loss and SwiGLU / activation kernels per element against float64:
RMSNorm and LayerNorm forward and backward (norms.hip), the shifted cross entropy (loss.hip),
SwiGLU forward / backward and the activation backward (elementwise.hip).

References, gates (with their derivations), input sets and the purpose of every shape are
tests/train_refs.py; tests/test_train_refs_host.py shows on the CPU, for these very inputs, that an
honest restatement of each kernel passes its gate and that every listed mutant fails it. Everything
goes through ops.*; the f64 references run on the GPU. Stats of every case are appended to the stats
file of tests/test_accuracy_gpu.py, by its own writer.
"""
import json

import pytest
import torch

from tests import train_refs as T
from tests.test_accuracy_gpu import _log as _append_stats

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = T.BF, T.F32


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def _log(rec):
    print(json.dumps(rec))
    _append_stats(rec)


def _dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def _finish(test, case, figures, fails):
    """log the figures, fail on every figure above 1.0 and on every other failure"""
    _log({"test": test, "case": case, **figures})
    fails = fails + [f"{k}: err / gate {v:.3f}" for k, v in figures.items() if not v <= 1.0]
    assert not fails, f"{test} {case}: " + "; ".join(fails)


class _rms_bwd_mode:
    """cullavo_rmsnorm_set_bwd(mode) for a block; the default (1) is restored whatever happens"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from cullavo_amd import _lib
        self.L = _lib.lib()
        self.L.cullavo_rmsnorm_set_bwd(self.mode)

    def __exit__(self, *exc):
        self.L.cullavo_rmsnorm_set_bwd(1)


# ---------------------------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,dt", T.RMS_FWD_CASES, ids=[T.case_id(c) for c in T.RMS_FWD_CASES])
def test_rmsnorm_fwd_against_f64(rows, cols, dt):
    d = _dev(T.norm_inputs(rows, cols, dt))
    y, rstd = ops().rmsnorm_fwd(d["x"], d["w"], T.EPS)
    torch.cuda.synchronize()
    wr, wy = T.rms_fwd_gate(y, rstd, d["x"], d["w"])
    _finish("train_rmsnorm_fwd", T.case_id((rows, cols, dt)), {"rstd": wr, "y": wy}, [])


def _rms_bwd_run(d, rstd, mode, want, dres, dw_dtype=F32, beta=0.0):
    """one launch; returns {figure: worst err / gate}"""
    x, dy, w = d["x"], d["dy"], d["w"]
    dw = None
    if want:
        # beta 0 must overwrite whatever dw held: NaN
        dw = d["dw_old"].to(dw_dtype).clone() if beta != 0.0 else torch.full((x.shape[1],), float("nan"), dtype=dw_dtype, device=DEV)
    with _rms_bwd_mode(mode):
        dx = ops().rmsnorm_bwd(dy, x, w, rstd, dres=dres, dw=dw, beta=beta)
        torch.cuda.synchronize()
    tag = f"dw{int(want)}_dres{int(dres is not None)}"
    out = {f"dx_{tag}": T.rms_dx_gate(dx, dy, x, w, rstd, dres)}
    if want:
        out[f"dw_{tag}"] = T.rms_dw_gate(dw, dy, x, rstd, d["dw_old"].to(dw_dtype), beta)
    return out


@pytest.mark.parametrize("kind", T.NORM_KINDS)
@pytest.mark.parametrize("rows,cols", T.RMS_BWD_CASES, ids=[T.case_id(c) for c in T.RMS_BWD_CASES])
def test_rmsnorm_bwd_against_f64(rows, cols, kind):
    """backward mode 1 with and without dw and dres: rmsnorm_bwd8p_k with dw or beyond 4096 columns,
    rmsnorm_bwd8_k otherwise"""
    d = _dev(T.norm_inputs(rows, cols, BF, kind))
    rstd = T.rms_stats(d["x"])
    figures = {}
    for want in (False, True):
        for dres in (None, d["dres"]):
            figures.update(_rms_bwd_run(d, rstd, 1, want, dres))
    _finish("train_rmsnorm_bwd", f"{rows}x{cols}-{kind}", figures, [])


@pytest.mark.parametrize("kind", T.NORM_KINDS)
@pytest.mark.parametrize("rows,cols,want", T.RMS_BWD_MODE0_CASES, ids=[T.case_id(c) for c in T.RMS_BWD_MODE0_CASES])
def test_rmsnorm_bwd_mode0_against_f64(rows, cols, want, kind):
    """backward mode 0: rmsnorm_bwd_k beyond 4096 columns, rmsnorm_bwd8_k with dw at 4096"""
    assert T.rms_bwd_plan(rows, cols, 0, want)[0] == ("rmsnorm_bwd_k" if cols > 4096 else "rmsnorm_bwd8_k")
    d = _dev(T.norm_inputs(rows, cols, BF, kind))
    rstd = T.rms_stats(d["x"])
    figures = {}
    for dres in (None, d["dres"]):
        figures.update(_rms_bwd_run(d, rstd, 0, want, dres))
    _finish("train_rmsnorm_bwd_mode0", f"{rows}x{cols}-{kind}", figures, [])


@pytest.mark.parametrize("kind", T.NORM_KINDS)
def test_rmsnorm_bwd_f32_beta_and_chained(kind):
    figures = {}
    rows, cols = T.RMS_BWD_F32_CASE  # the f32 instantiation
    d = _dev(T.norm_inputs(rows, cols, F32, kind))
    for k, v in _rms_bwd_run(d, T.rms_stats(d["x"]), 1, True, d["dres"]).items():
        figures["f32_" + k] = v
    rows, cols = T.RMS_BWD_BETA_CASE  # dw bf16, accumulated onto its old value
    d = _dev(T.norm_inputs(rows, cols, BF, kind))
    for k, v in _rms_bwd_run(d, T.rms_stats(d["x"]), 1, True, d["dres"], dw_dtype=BF, beta=1.0).items():
        figures["beta_" + k] = v
    # chained: the forward kernel's own rstd into the backward and into its f64 reference
    d = _dev(T.norm_inputs(37, 4096, BF, kind))
    _, rstd = ops().rmsnorm_fwd(d["x"], d["w"], T.EPS)
    for k, v in _rms_bwd_run(d, rstd, 1, True, d["dres"]).items():
        figures["chained_" + k] = v
    _finish("train_rmsnorm_bwd_variants", kind, figures, [])


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
def _ln_case(rows, cols, dt, kind):
    d = _dev(T.norm_inputs(rows, cols, dt, kind, name="ln"))
    x, dy, w, b = d["x"], d["dy"], d["w"], d["b"]
    y, mean_k, rstd_k = ops().layernorm_fwd(x, w, b, T.EPS)
    torch.cuda.synchronize()
    wm, wr, wy = T.ln_fwd_gate(y, mean_k, rstd_k, x, w, b)
    figures = {"fwd_mean": wm, "fwd_rstd": wr, "fwd_y": wy}
    mean, rstd = T.ln_stats(x)

    def bwd(tag, mean, rstd, dres, want):
        dw = torch.full((cols,), float("nan"), dtype=F32, device=DEV) if want else None
        db = torch.full((cols,), float("nan"), dtype=F32, device=DEV) if want else None
        dx = ops().layernorm_bwd(dy, x, w, mean, rstd, dres=dres, dw=dw, db=db)
        torch.cuda.synchronize()
        for k, v in zip(("dx", "dw", "db"), T.ln_bwd_gate(dx, dw, db, dy, x, w, mean, rstd, dres)):
            if v is not None:
                figures[f"{k}_{tag}"] = v

    for want in (False, True):
        for dres in (None, d["dres"]):
            bwd(f"dw{int(want)}_dres{int(dres is not None)}", mean, rstd, dres, want)
    bwd("chained", mean_k, rstd_k, d["dres"], True)  # the forward kernel's own mean and rstd
    _finish("train_layernorm", f"{rows}x{cols}-{T.case_id((dt,))}-{kind}", figures, [])


@pytest.mark.parametrize("kind", T.NORM_KINDS)
@pytest.mark.parametrize("rows,cols", T.LN_CASES, ids=[T.case_id(c) for c in T.LN_CASES])
def test_layernorm_against_f64(rows, cols, kind):
    _ln_case(rows, cols, BF, kind)


@pytest.mark.parametrize("kind", T.NORM_KINDS)
def test_layernorm_f32_against_f64(kind):
    _ln_case(*T.LN_F32_CASE, F32, kind)


# ---------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------
def _grad_loss(gl):
    return None if gl is None else torch.tensor([gl], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("rows,V,dt,kind", T.CE_CASES, ids=[T.case_id(c) for c in T.CE_CASES])
def test_cross_entropy_against_f64(rows, V, dt, kind):
    xc, tc = T.ce_inputs(rows, V, dt, kind)
    ldl = xc.stride(0)
    buf = torch.empty(rows, ldl, dtype=dt, device=DEV)
    buf.copy_(xc.as_strided((rows, ldl), (ldl, 1)))  # with the CE_PAD columns
    x, t = buf[:, :V], tc.to(DEV)
    fails, figures = [], {}
    row_loss, row_lse = ops().ce_fwd(x, t)
    torch.cuda.synchronize()
    figures["lse"], figures["row_loss"], zero_ok = T.ce_fwd_gate(row_loss, row_lse, x, t)
    if not zero_ok:
        fails.append("the loss of an ignored row is not exactly 0.0")
    lse, loss, out = T.ce_stats(x, t)
    # ce_reduce on the reference's f32 row losses, on the kernel's own, and with nothing selected
    fails += T.ce_reduce_check(ops().ce_reduce(loss, t), loss, t)
    out_k = ops().ce_reduce(row_loss, t)
    fails += T.ce_reduce_check(out_k, row_loss, t)
    none = torch.full_like(t, T.IGNORE)
    fails += T.ce_reduce_check(ops().ce_reduce(loss, none), loss, none)

    def bwd(tag, lse, out, gl):
        dbuf = torch.full((rows, ldl), T.CE_SENT, dtype=dt, device=DEV)
        d = ops().ce_bwd(x, t, lse, out, _grad_loss(gl), out=dbuf[:, :V])
        torch.cuda.synchronize()
        figures[tag], zero_ok = T.ce_bwd_gate(d, x, t, lse, out, _grad_loss(gl))
        if not zero_ok:
            fails.append(f"{tag}: an ignored row is not zero over all V columns")
        if not bool((dbuf[:, V:] == T.CE_SENT).all()):
            fails.append(f"{tag}: columns V .. ldl-1 of the gradient buffer were written")

    for gl in T.CE_GRAD_LOSS:
        bwd(f"dlogits_gl_{gl if gl is None else round(gl, 3)}", lse, out, gl)
    bwd("dlogits_chained", row_lse, out_k, 0.5)  # the forward kernels' own lse and 1 / count
    _finish("train_cross_entropy", T.case_id((rows, V, dt, kind)), figures, fails)


@pytest.mark.parametrize("B,L,masked", [(3, 7, True), (3, 7, False), (4, 1, True), (4, 1, False), (300, 5, True)])
def test_shift_targets_bitwise(B, L, masked):
    g = T._gen(f"shift-{B}-{L}")
    labels = torch.randint(0, 32000, (B, L), generator=g)
    labels[torch.rand(B, L, generator=g) < 0.2] = T.IGNORE
    mask = (torch.rand(B, L, generator=g) < 0.7).long() if masked else None
    got = ops().shift_targets(labels.to(DEV), mask.to(DEV) if masked else None)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), T.shift_targets_ref(labels, mask))


# ---------------------------------------------------------------------------------------------
# SwiGLU and activation backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,F,dt", T.SWIGLU_CASES, ids=[T.case_id(c) for c in T.SWIGLU_CASES])
def test_swiglu_against_f64(rows, F, dt):
    gu, d = (t.to(DEV) for t in T.swiglu_inputs(rows, F, dt))
    o = ops().swiglu_fwd(gu)
    dgu = ops().swiglu_bwd(d, gu)
    torch.cuda.synchronize()
    wg, wu = T.swiglu_bwd_gate(dgu, d, gu)
    _finish("train_swiglu", T.case_id((rows, F, dt)), {"fwd": T.swiglu_fwd_gate(o, gu), "dgate": wg, "dup": wu}, [])


@pytest.mark.parametrize("act", T.ACTS)
@pytest.mark.parametrize("n,dt", T.ACT_CASES, ids=[T.case_id(c) for c in T.ACT_CASES])
def test_act_bwd_against_f64(n, dt, act):
    dy, v = (t.to(DEV) for t in T.act_inputs(n, dt))
    code = ops().ACT_GELU if act == "gelu" else ops().ACT_QUICK_GELU
    dx = ops().act_bwd(code, dy, v)
    torch.cuda.synchronize()
    _finish("train_act_bwd", f"{act}-{T.case_id((n, dt))}", {"dx": T.act_bwd_gate(dx, dy, v, act)}, [])
