"""The kernels that turn gradients into new weights and that move rows into and out of the model,
per element against float64: fused AdamW, the gradient sum of squares, the clip coefficient, the
in-place scale, the bias-gradient column sums (elementwise.hip); the embedding scatter-add and
gather, the two-source row gather, the CLIP patch unfold and the CLS / position / pre-LayerNorm
kernel (embed.hip).

References, gates (with their derivations), input sets and the purpose of every shape are
tests/update_refs.py; tests/test_update_refs_host.py shows on the CPU, for these very inputs, that an
honest restatement of each kernel passes its gate and that every listed mutant fails it. Everything
goes through ops.* (ops.call where the output buffer has to be the test's own, filled with a
sentinel); the f64 references run on the GPU. Stats of every case are appended to the stats file of
tests/test_accuracy_gpu.py, by its own writer.
"""
import json
import math

import pytest
import torch

from tests import update_refs as R
from tests.test_accuracy_gpu import _log as _append_stats

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = R.BF, R.F32


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def _log(rec):
    print(json.dumps(rec))
    _append_stats(rec)


def _finish(test, case, figures, fails):
    """log the figures, fail on every figure above 1.0 and on every other failure"""
    _log({"test": test, "case": case, **figures})
    fails = fails + [f"{k}: err / gate {v:.3f}" for k, v in figures.items() if not v <= 1.0]
    assert not fails, f"{test} {case}: " + "; ".join(fails)


def _scalar(v):
    return torch.tensor([v], dtype=F32, device=DEV)


# ---------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdt,sdt", R.ADAM_DTYPES, ids=[R.case_id(c) for c in R.ADAM_DTYPES])
def test_adamw_one_step_against_f64(pdt, sdt):
    """one step from a stored state, every case of update_refs.ADAM_CASES; one record per case"""
    failures = []
    for n, step, wd, gs, off in R.ADAM_CASES:
        p0, g, m0, v0 = R.adamw_inputs(n, pdt, sdt, step, wd, gs)
        p, gd, m, v = (R.at_offset(t, off, DEV) for t in (p0, g, m0, v0))
        assert all((t.data_ptr() - off * t.element_size()) % 16 == 0 for t in (p, gd, m, v))
        ops().adamw(p, gd, m, v, lr=R.ADAM_LR, beta1=R.ADAM_B1, beta2=R.ADAM_B2, eps=R.ADAM_EPS, weight_decay=wd,
                    step=step, grad_scale=None if gs is None else _scalar(gs))
        torch.cuda.synchronize()
        c = R.AdamConsts(step, wd)
        wm, wv, wp = R.adamw_gates(p, m, v, p0.to(DEV), gd, m0.to(DEV), v0.to(DEV), c, gs)
        case = f"{R.case_id((pdt, sdt))}-n{n}-step{step}-wd{wd}-gs{gs}-off{off}"
        fails = [] if torch.equal(gd.cpu(), g) else ["the gradient was written"]
        try:
            _finish("update_adamw", case, {"m": wm, "v": wv, "p": wp}, fails)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------
# sumsq, clip_coef, scale_inplace
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.SUMSQ_DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("n,kind", R.SUMSQ_CASES, ids=[R.case_id(c) for c in R.SUMSQ_CASES])
def test_sumsq_against_f64(n, kind, dt):
    x = R.sumsq_inputs(n, dt, kind).to(DEV)
    outs = []
    for _ in range(2):
        out = _scalar(R.SUMSQ_OUT0)
        ops().sumsq(x, out)
        torch.cuda.synchronize()
        outs.append(out)
    fails = [] if torch.equal(outs[0], outs[1]) else ["two runs differ bitwise"]
    _finish("update_sumsq", f"{n}-{kind}-{R.case_id((dt,))}", {"out": R.sumsq_gate(outs[0], x)}, fails)


@pytest.mark.parametrize("s,mn", R.CLIP_CASES, ids=[f"{s}-{mn}" for s, mn in R.CLIP_CASES])
def test_clip_coef_every_branch(s, mn):
    sumsq = _scalar(s)
    coef, norm = _scalar(-7.0), _scalar(-7.0)
    ops().clip_coef(sumsq, mn, coef, norm)
    coef2 = _scalar(-7.0)
    ops().clip_coef(sumsq, mn, coef2, None)   # norm_out not given
    torch.cuda.synchronize()
    fails = R.clip_coef_check(s, mn, coef.item(), norm.item()) + R.clip_coef_check(s, mn, coef2.item(), None)
    if not torch.equal(coef, coef2):
        fails.append("coef differs without norm_out")
    _log({"test": "update_clip_coef", "case": f"{s}-{mn}", "coef": coef.item(), "norm": norm.item()})
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("n,dt,s", R.SCALE_CASES, ids=[R.case_id(c) for c in R.SCALE_CASES])
def test_scale_inplace_against_f64(n, dt, s):
    x0 = R.scale_inputs(n, dt).to(DEV)
    buf = torch.full((n + 8,), -7.0, dtype=dt, device=DEV)   # the elements behind x must stay
    x = buf[:n]
    x.copy_(x0)
    ops().scale_inplace(x, _scalar(s))
    torch.cuda.synchronize()
    fails = [] if bool((buf[n:] == -7.0).all()) else ["elements past n were written"]
    if s == 1.0 and not torch.equal(x, x0):
        fails.append("the scale 1.0 changed bits")
    _finish("update_scale_inplace", R.case_id((n, dt, s)), {"y": R.scale_gate(x, x0, s)}, fails)


# ---------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,idt,odt,beta,kind", R.COLSUM_CASES, ids=[R.case_id(c) for c in R.COLSUM_CASES])
def test_colsum_against_f64(rows, cols, idt, odt, beta, kind):
    x, old = R.colsum_inputs(rows, cols, idt, kind)
    x, old = x.to(DEV), old.to(DEV)
    # beta 0 must overwrite whatever out held: NaN
    out = old.to(odt).clone() if beta != 0.0 else torch.full((cols,), float("nan"), dtype=odt, device=DEV)
    ops().colsum(x, out, beta=beta)
    torch.cuda.synchronize()
    _finish("update_colsum", R.case_id((rows, cols, idt, odt, beta, kind)), {"out": R.colsum_gate(out, x, old, beta)}, [])


# ---------------------------------------------------------------------------------------------
# embedding backward, forward, row gather
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n,tt,td,beta", R.EMB_BWD_CASES, ids=[R.case_id(c) for c in R.EMB_BWD_CASES])
def test_embedding_bwd_against_f64(dim, n, tt, td, beta):
    ids, dout, old = (t.to(DEV) for t in R.emb_bwd_inputs(dim, n, tt, td))
    runs = []
    for _ in range(2):
        dtable = old.clone()
        ops().embedding_bwd(ids, dout, dtable, beta=beta)
        torch.cuda.synchronize()
        runs.append(dtable)
    w, same = R.emb_bwd_gate(runs[0], ids, dout, old, beta)
    fails = [] if same else ["a row that no id in range addresses was written"]
    if not torch.equal(runs[0], runs[1]):
        fails.append("two runs differ bitwise")
    _finish("update_embedding_bwd", R.case_id((dim, n, tt, td, beta)), {"dtable": w}, fails)


@pytest.mark.parametrize("dim,dt", R.GATHER_CASES, ids=[R.case_id(c) for c in R.GATHER_CASES])
def test_embedding_fwd_and_row_gather2_exact(dim, dt):
    o = ops()
    a, b, ids, src = (t.to(DEV) for t in R.gather_inputs(dim, dt))
    code = o.DT_BF16 if dt == BF else o.DT_F32
    stream = torch.cuda.current_stream().cuda_stream
    ref = R.embedding_fwd_ref(ids, a)
    assert torch.equal(o.embedding_fwd(ids, a), ref)
    out = torch.full((ids.numel() + 1, dim), R.GATHER_SENTINEL, dtype=dt, device=DEV)   # one row more: must stay
    o.call("embedding_fwd", ids.data_ptr(), ids.numel(), a.data_ptr(), a.shape[0], dim, out.data_ptr(), code, stream)
    torch.cuda.synchronize()
    assert torch.equal(out[:-1], ref) and bool((out[-1] == R.GATHER_SENTINEL).all())

    ref2 = R.row_gather2_ref(src, a, b)
    assert torch.equal(o.row_gather2(src, a, b), ref2)
    out = torch.full((src.numel() + 1, dim), R.GATHER_SENTINEL, dtype=dt, device=DEV)
    o.call("row_gather2", src.data_ptr(), src.numel(), a.data_ptr(), a.shape[0], b.data_ptr(), dim, out.data_ptr(), code, stream)
    torch.cuda.synchronize()
    assert torch.equal(out[:-1], ref2) and bool((out[-1] == R.GATHER_SENTINEL).all())
    # b = None: every source row lies in a
    sa = src.clamp_max(a.shape[0] - 1)
    assert torch.equal(o.row_gather2(sa, a, None), R.row_gather2_ref(sa, a, None))


# ---------------------------------------------------------------------------------------------
# CLIP front end
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,dim,dt", R.VIS_CASES, ids=[R.case_id(c) for c in R.VIS_CASES])
def test_vision_embed_ln_against_f64(B, T, dim, dt):
    x, cls, pos, w, b = (t.to(DEV) for t in R.vis_inputs(B, T, dim, dt))
    y = ops().vision_embed_ln(x, cls, pos, w, b, B=B, T=T, eps=R.VIS_EPS)
    torch.cuda.synchronize()
    _finish("update_vision_embed_ln", R.case_id((B, T, dim, dt)), {"y": R.vis_gate(y, x, cls, pos, w, b, T)}, [])


@pytest.mark.parametrize("pdt,odt", R.IM2COL_DTYPES, ids=[R.case_id(c) for c in R.IM2COL_DTYPES])
def test_im2col_exact(pdt, odt):
    o = ops()
    s = R.IM2COL_SHAPE
    B, C, H, W, patch, kpad = (s[k] for k in ("B", "C", "H", "W", "patch", "kpad"))
    pix = R.im2col_inputs(pdt).to(DEV)
    ref = R.im2col_ref(pix, patch, kpad, odt)
    got = o.im2col_patches(pix, patch, kpad, dtype=odt)
    torch.cuda.synchronize()
    assert got.dtype == odt and torch.equal(got, ref)
    # the same launch into a buffer of the test's own: CLS rows and the padding columns are written as zeros
    # over the sentinel, the row behind the last stays
    rows = B * (1 + (H // patch) * (W // patch))
    out = torch.full((rows + 1, kpad), R.IM2COL_SENTINEL, dtype=odt, device=DEV)
    code = {BF: o.DT_BF16, F32: o.DT_F32}
    o.call("im2col_patches", pix.data_ptr(), code[pdt], B, C, H, W, patch, out.data_ptr(), kpad, code[odt],
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out[:-1], ref) and bool((out[-1] == R.IM2COL_SENTINEL).all())
    grid = out[:-1].view(B, -1, kpad)
    assert not grid[:, 0].any() and not grid[:, :, C * patch * patch:].any()
    if odt == BF:
        assert torch.equal(grid[0, 1, :patch], pix[0, 0, 0, :patch].to(BF))   # one RNE conversion of the pixel
    assert math.prod(ref.shape) == rows * kpad
