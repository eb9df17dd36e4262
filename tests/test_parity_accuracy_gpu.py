"""The f32 parity mode's kernels per element: gemm_f32_k (csrc/gemm_f32.hip) and the generic attention
kernels (csrc/attn_generic.hip, attn_gen_fwd_body.h), through ops, at the smallest shapes at which each
path can still go wrong.

The case tables, references, gates P0-P4 and the attention gates (with their derivations) and the
NaN-framed inputs are tests/parity_refs.py; tests/test_parity_refs_host.py shows on the CPU, for these
very inputs, that an honest restatement passes every gate and that each listed mutant fails. Operands sit
in NaN frames, outputs in sentinel frames; the caches of the cached and ragged attention hold NaN in every
row at or above kv_len and in every row below kv_start. Stats of every case are appended to the stats file
of tests/test_accuracy_gpu.py.
"""
import json

import pytest
import torch

from tests import parity_refs as R
from tests.test_accuracy_gpu import _log as _append_stats

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF = R.F32, R.BF


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def _log(rec):
    print(json.dumps(rec))
    _append_stats(rec)


def _i32(x):
    return None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------
# gemm_f32_k
# ---------------------------------------------------------------------------------------------
class _Gemm:
    """the launches of one shape: framed outputs, the frame checks collected in `fails`"""

    def __init__(self, d, M, N, K, al, bl):
        self.d, self.dims, self.fails = d, (M, N, K, al, bl), []

    def run(self, tag, fill=None, want_preact=False, **kw):
        M, N, K, al, bl = self.dims
        d = self.d
        buf, C = R.framed(M, N, F32, DEV, 0, fill)
        pbuf = pre = None
        if want_preact:
            pbuf, pre = R.framed(M, N, F32, DEV)
            kw["preact"] = pre
        if kw.get("residual") is not None:
            kw["ldr"] = kw["residual"].stride(0)
        if kw.get("addend") is not None:
            kw["ld_addend"] = kw["addend"].stride(0)
        A, B = d["A"], d["B"]
        ops().gemm_ex(al, bl, M, N, K, A, A.stride(0), B, B.stride(0), C, C.stride(0), split_k=False, **kw)
        torch.cuda.synchronize()
        if not R.frame_untouched(buf, M, N):
            self.fails.append(f"{tag}: C written outside its [M, N] view")
        if pbuf is not None and not R.frame_untouched(pbuf, M, N):
            self.fails.append(f"{tag}: pre-activation written outside its [M, N] view")
        return C, pre


def _product_figures(g, c32, stats):
    """P0 and P1 of a plain product into stats; failures into g.fails"""
    M, N, K, al, bl = g.dims
    d = g.d
    chain = R.fma_chain(d["Amk"], d["Bnk"])
    nd = R.ndiff(c32, chain)
    ulp = torch.finfo(F32).eps * chain.abs().clamp_min(2.0 ** -126)
    stats["p0_bits_differing"] = nd
    stats["p0_max_ulp"] = ((c32 - chain).abs() / ulp).max().item() if nd else 0.0
    ref, absprod = R.product_ref(d["Amk"], d["Bnk"])
    w, rel, fin = R.g1(c32, ref, absprod, K)
    stats["p1_err_over_gate"], stats["p1_rel_l2"] = w, rel
    if not (w <= 1.0 and rel <= 1e-5 and fin):
        g.fails.append(f"P1: err / (K 2^-24 |A||B|^T) {w:.3f}, rel-L2 {rel:.2e}, finite {fin}")
    if nd:
        g.fails.append(f"P0: {nd} elements differ from the k-ordered fmaf chain (largest {stats['p0_max_ulp']:.2f} ulp)")


def _epi_kw(d, o, keep):
    kw, rk = {}, {}
    if o.get("alpha"):
        kw["alpha"] = rk["alpha"] = o["alpha"]
    if o.get("drop"):
        kw.update(drop_operand=3, drop_p=o["drop"], drop_seed=R.DROP_SEED)
        rk.update(keep=keep, p=o["drop"])
    for k in ("bias", "addend", "residual"):
        if o.get(k):
            kw[k] = rk[k] = d[k]
    if o.get("beta"):
        kw["beta"] = rk["beta"] = o["beta"]
        rk["old"] = d["old"]
    return kw, rk


@pytest.mark.parametrize("c", R.GEMM_CASES, ids=[c["name"] for c in R.GEMM_CASES])
def test_gemm_f32(c):
    M, N, K, al, bl = c["M"], c["N"], c["K"], c["al"], c["bl"]
    d = R.gemm_inputs(c["name"], M, N, K, al, bl, DEV)
    g = _Gemm(d, M, N, K, al, bl)
    stats = {"test": "gemm_f32", "case": c["name"], "shape": [M, N, K], "layouts": [al, bl], "bits_differing": {},
             "p3_err_over_gate": {}}
    c32, _ = g.run("plain")
    _product_figures(g, c32, stats)
    nd = stats["bits_differing"]
    if c["beta1"]:  # a tile visited twice or never differs from the replay
        y, _ = g.run("beta1", fill=d["old"], beta=1.0)
        nd["beta1"] = R.ndiff(y, R.epilogue_replay(c32, beta=1.0, old=d["old"])[0])
    keep = R.keep_mask(R.DROP_SEED, M, N, 0.5, DEV) if c["epi"] else None
    for v in c["epi"]:
        o = R.EPI_P2.get(v) or R.EPI_P3[v]
        kw, rk = _epi_kw(d, o, keep)
        pre_on = bool(o.get("preact"))
        fill = d["old"] if o.get("beta") else None
        if v in R.EPI_P2:
            y, pre = g.run(v, fill=fill, want_preact=pre_on, **kw)
            want, wpre = R.epilogue_replay(c32, **rk)
            nd[v] = R.ndiff(y, want)
            if pre_on:
                nd[v + "/preact"] = R.ndiff(pre, wpre)
            if v == "drop3" and int((y[~keep] != 0).sum()):
                g.fails.append(f"{v}: a dropped element is not == 0")
        else:
            y, pre = g.run(v, want_preact=True, act=o["act"], **kw)
            res = rk.pop("residual")
            nd[v + "/preact"] = R.ndiff(pre, R.epilogue_replay(c32, **rk)[1])
            w = R.p3_act(y, pre, o["act"], res)
            stats["p3_err_over_gate"][v] = w
            if not w <= 1.0:
                g.fails.append(f"{v}: P3 err / gate {w:.3f}")
    g.fails += [f"{k}: {n} elements differ from the replay" for k, n in nd.items() if n]
    stats["failures"] = g.fails
    _log(stats)
    assert not g.fails, f"{c['name']} ({c['why']}): " + "; ".join(g.fails)


@pytest.mark.parametrize("case", R.DROP_CASES, ids=[x[0] for x in R.DROP_CASES])
def test_gemm_f32_dropout(case):
    name, mode, T, F, p = case
    M, N, K, al, bl = R.drop_dims(mode, T, F)
    d = R.gemm_inputs(name, M, N, K, al, bl, DEV)
    g = _Gemm(d, M, N, K, al, bl)
    keep = R.keep_mask(R.DROP_SEED, T, F, p, DEV)
    stats = {"test": "gemm_f32_dropout", "case": name, "shape": [M, N, K], "mode": mode, "p": p}
    plain, _ = g.run("plain")
    _product_figures(g, plain, stats)
    y0, _ = g.run("p0", drop_operand=mode, drop_p=0.0, drop_seed=R.DROP_SEED)
    stats["p0_mode_bits_differing"] = R.ndiff(y0, plain)                       # drop_p = 0 drops nothing
    y, _ = g.run("drop", drop_operand=mode, drop_p=p, drop_seed=R.DROP_SEED)
    if mode == 3:
        if p == 0.5:
            stats["bits_differing"] = R.ndiff(y, R.epilogue_replay(plain, keep=keep, p=p)[0])           # P2
        else:
            stats["p3_err_over_gate"], _ = R.p3_drop(y, plain, keep, p)                                # P3
        stats["mask_mismatches"] = int(((y != 0) != keep).sum())                                       # P4
        # and with ldc, ldr and ld_addend all in play around the dropout
        y2, _ = g.run("drop+bias+res", drop_operand=3, drop_p=p, drop_seed=R.DROP_SEED, bias=d["bias"],
                      residual=d["residual"])
        want = torch.where(keep, y, torch.zeros_like(y)) + d["bias"] + d["residual"]
        if p == 0.5:
            stats["bits_differing_bias_res"] = R.ndiff(y2, want)
        else:  # two more f32 roundings (or one, contracted) on the f64 chain
            cs = torch.where(keep, plain.double() * R.drop_scale(p), torch.zeros_like(plain, dtype=torch.float64))
            ref = cs + d["bias"].double() + d["residual"].double()
            gate = R.E * (cs.abs() + (cs + d["bias"].double()).abs() + ref.abs()) + R.FLOOR
            stats["p3_err_over_gate"] = max(stats["p3_err_over_gate"], R.worst(y2.double() - ref, gate))
    else:
        # the mask itself, read through an identity operand: C = the dropped x
        if mode == 1:
            di = R.gemm_inputs(name, T, F, F, 0, 0, DEV, identity="B")
            gi, x = _Gemm(di, T, F, F, 0, 0), di["Amk"]
        else:
            di = R.gemm_inputs(name, T, F, T, 1, 1, DEV, identity="A")
            gi, x = _Gemm(di, T, F, T, 1, 1), di["Bnk"].T
        yi, _ = gi.run("identity", drop_operand=mode, drop_p=p, drop_seed=R.DROP_SEED)
        g.fails += gi.fails
        stats["mask_mismatches"] = int(((yi != 0) != keep).sum()) + int((x == 0).sum())                # P4
        stats["identity_bits_differing"] = R.ndiff(yi, R.dropped_operand(x, keep, p))
        if mode == 1:
            want = R.fma_chain(R.dropped_operand(d["Amk"], keep, p), d["Bnk"])
        else:
            want = R.fma_chain(d["Amk"], R.dropped_operand(d["Bnk"], keep.T, p))
        stats["bits_differing"] = R.ndiff(y, want)                                                     # P4
    for k, v in stats.items():
        if k.endswith("bits_differing") or k.startswith("bits_differing") or k == "mask_mismatches":
            if v and k != "p0_bits_differing":
                g.fails.append(f"{k}: {v}")
    if not stats.get("p3_err_over_gate", 0.0) <= 1.0:
        g.fails.append(f"P3 err / gate {stats['p3_err_over_gate']:.3f}")
    stats["failures"] = g.fails
    _log(stats)
    assert not g.fails, f"{name}: " + "; ".join(g.fails)


def test_gemm_f32_shapes_the_library_rejects():
    """the shared argument checks of the bf16 GEMM hold for f32 operands: the shapes whose place the case table's
    nearest accepted shapes take (tests/parity_refs.py, E_SHAPES) are argument errors, nothing is launched"""
    for M, N, K, al, bl in ((261, 137, 203, 0, 0), (261, 136, 203, 0, 0), (261, 136, 203, 1, 1), (1, 1, 5, 0, 0),
                            (70, 40, 1, 0, 0), (1030, 260, 24, 0, 0)):
        # buffers large enough for every shape at ld 512, should a check ever let one through
        a, b, cc = (torch.zeros((1100, 512), dtype=F32, device=DEV) for _ in range(3))
        with pytest.raises(ValueError):
            ops().gemm_ex(al, bl, M, N, K, a, 512, b, 512, cc, 512, split_k=False)


def test_gemm_f32_dropout_unsupported_layouts():
    """operand dropout needs the token-major operand: the documented unsupported error, nothing launched"""
    from cullavo_amd._lib import CullavoError
    d = R.gemm_inputs("unsupported", 72, 40, 24, 1, 0, DEV)
    C = torch.full((72, 40), R.SENT, dtype=F32, device=DEV)
    A, B = d["A"], d["B"]
    with pytest.raises(CullavoError, match="dropout on A needs a_layout 0"):
        ops().gemm_ex(1, 0, 72, 40, 24, A, A.stride(0), B, B.stride(0), C, 40, drop_operand=1, drop_p=0.5, split_k=False)
    with pytest.raises(CullavoError, match="dropout on B needs b_layout 1"):
        ops().gemm_ex(1, 0, 72, 40, 24, A, A.stride(0), B, B.stride(0), C, 40, drop_operand=2, drop_p=0.5, split_k=False)
    torch.cuda.synchronize()
    assert bool((C == R.SENT).all())


# ---------------------------------------------------------------------------------------------
# generic attention
# ---------------------------------------------------------------------------------------------
def _sentinel_cols(rows, widths, dtype, gap=8):
    """column blocks of `widths` in one sentinel buffer, `gap` sentinel columns after each; (buffer, views)"""
    buf = torch.full((rows, sum(widths) + gap * len(widths)), R.SENT, dtype=dtype, device=DEV)
    views, c0 = [], 0
    for w in widths:
        views.append(buf[:, c0:c0 + w])
        c0 += w + gap
    return buf, views


def _gaps_untouched(buf, widths, gap=8):
    c0, ok = 0, True
    for w in widths:
        ok = ok and bool((buf[:, c0 + w:c0 + w + gap] == R.SENT).all())
        c0 += w + gap
    return ok


@pytest.mark.parametrize("c", R.ATTN_CASES, ids=[c["name"] for c in R.ATTN_CASES])
def test_attention_generic(c):
    B, Lq, Lk, D, dt, scale = c["B"], c["Lq"], c["Lk"], c["D"], c["dtype"], c["scale"]
    hd = R.H * D
    q, k, v, do = R.attn_inputs(c, DEV)
    fails, stats = [], {"test": "attn_generic", "case": c["name"], "kind": c["kind"], "shape": [B, R.H, Lq, Lk, D]}
    obuf = dbuf = None
    if c["layout"]:  # q | k | v column blocks of one buffer (Lq = Lk)
        qkv = torch.cat([q, k, v], 1)
        q, k, v = qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:]
        obuf, (out,) = _sentinel_cols(B * Lq, [hd], dt)
    else:
        out = None
    vis = R.visibility(c, device=DEV)
    r = R.attn_ref(q, R.kv_rows(c, k), R.kv_rows(c, v), c, vis)
    ks = _i32(c["ks"])
    if c["kind"] == "packed":
        o, lse = ops().attn_fwd(q, k, v, B=B, H=R.H, Lq=Lq, Lk=Lk, D=D, scale=scale, causal=c["causal"], kv_start=ks,
                                out=out)
    elif c["kind"] == "cached":
        o, lse = ops().attn_fwd_cached(q, k, v, B=B, H=R.H, Lq=Lq, past=c["past"], D=D, scale=scale, kv_start=ks)
    else:
        o, lse = ops().attn_fwd_ragged(q, k, v, _i32(c["kv_len"]), B=B, H=R.H, Lq=Lq, D=D, scale=scale,
                                       q_pad=_i32(c["q_pad"]), kv_start=ks)
    torch.cuda.synchronize()
    if not bool(torch.isfinite(o.float()).all()):
        fails.append("O is not finite: a masked (NaN) cache row reached the output")
    stats["dead_query_rows"] = int((~r["live"]).sum())
    stats["O"] = R.worst(o.double() - r["O"], R.o_gate(r, c))
    err, bad_inf = R.lse_check(lse, r)
    stats["lse_max_err"] = err
    if bad_inf:
        fails.append(f"lse: {bad_inf} dead rows are not +inf")
    # > 0: the comparison is not empty. With a single key lse = s, which bf16 operands at D = 16 give exactly
    if err is not None and not ((0.0 < err or Lk == 1) and err <= 1e-5):
        fails.append(f"lse max|err| {err:.2e}")
    zeros = R.zero_checks(c, r, o=o)
    if obuf is not None and not _gaps_untouched(obuf, [hd]):
        fails.append("O written outside its column block")
    if c["kind"] == "packed":
        if c["chain"]:
            o_in, lse_in = o, lse
        else:
            o_in, lse_in = r["O"].to(dt), r["LSE"].float()
        bw = R.bwd_ref(r, c, do, o_in, lse_in)
        kw = {}
        if c["layout"]:
            dbuf, (dq, dk, dv) = _sentinel_cols(B * Lq, [hd] * 3, dt)
            kw = dict(dq=dq, dk=dk, dv=dv)
        dq, dk, dv = ops().attn_bwd(q, k, v, o_in, do, lse_in, B=B, H=R.H, Lq=Lq, Lk=Lk, D=D, scale=scale,
                                    causal=c["causal"], kv_start=ks, **kw)
        torch.cuda.synchronize()
        for name, t in (("dQ", dq), ("dK", dk), ("dV", dv)):
            stats[name] = R.worst(t.double() - bw[name], bw[name + "_gate"])
            if not bool(torch.isfinite(t.float()).all()):
                fails.append(f"{name} is not finite")
        zeros.update(R.zero_checks(c, r, dq=dq, dk=dk, dv=dv))
        if dbuf is not None and not _gaps_untouched(dbuf, [hd] * 3):
            fails.append("dQ / dK / dV written outside their column blocks")
    fails += [f"{k}: {n} rows are not exactly zero" for k, n in zeros.items() if n]
    fails += [f"{k}: err / gate {stats[k]:.3f}" for k in ("O", "dQ", "dK", "dV") if k in stats and not stats[k] <= 1.0]
    stats["failures"] = fails
    _log(stats)
    assert not fails, f"{c['name']} ({c['why']}): " + "; ".join(fails)


def test_attention_causal_needs_equal_lengths():
    """the packed entry points take causal attention at Lq == Lk only: an argument error, nothing launched"""
    c = next(x for x in R.ATTN_CASES if x["name"] == "Lq70Lk33-D32f32")
    q, k, v, do = R.attn_inputs(c, DEV)
    with pytest.raises(ValueError, match="causal attention needs Lq == Lk"):
        ops().attn_fwd(q, k, v, B=2, H=R.H, Lq=70, Lk=33, D=32, scale=c["scale"], causal=True)
