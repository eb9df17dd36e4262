"""float64 references, gates, input sets and the case table for the bf16 GEMM family (csrc/gemm.hip,
csrc/gemm_common.h): every terminal launch of gemm_impl and every epilogue option, at the smallest
shapes at which each path can still go wrong. Plain torch on whatever device the tensors live on:
tests/test_gemm_refs_host.py proves on the CPU that every gate passes an honest f32 restatement and
fails a set of one-line mutants, tests/test_gemm_accuracy_gpu.py then holds the kernels to the same
gates on the same inputs (same seeds, same shapes, same NaN frames).

The gates:
 G1  the f32-output product against f64: |c - alpha A B^T| <= K 2^-24 |alpha| (|A| |B|^T) + FLOOR per
     element (bf16 x bf16 products are exact in f32, so the only error is the f32 summation of K terms,
     (K - 1) 2^-24 sum|a_k b_k| for ANY order: the bound of tests/test_accuracy_gpu.py) and rel-L2 <= 1e-5.
     At K = 200 the bound is ~1e-3 of a value of size ~2: one dropped 8-wide chunk misses it a
     thousandfold.
 G2  the epilogue chain replayed bit for bit (chain_replay) on the kernel's own f32 plain product.
 G3  the activations: the f64 value rounded to bf16, or its neighbour where the f64 value lies within a
     derived slack of a rounding boundary (act_check).
 G4  the SwiGLU-backward epilogue against ops.swiglu_bwd of the rounded product, bitwise.
 G5  the fused LoRA up-projection against the unfused addend path, bitwise.
No number here was taken from a kernel's output.
"""
import math

import torch

from tests.decode_refs import U, _gen, bf, worst  # noqa: F401 (U: re-exported for the tests)
from tests.train_refs import E, FLOOR

BF = torch.bfloat16
F32 = torch.float32
SENT = -7.0  # exact in bf16 and f32; no honest output of these inputs is a run of -7.0
ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_SWIGLU_BWD = 0, 1, 2, 3
AMBIGUOUS_CAP = 0.005
LORA_R = 64
LORA_SCALE = 2.0  # a power of two, as alpha (chain_replay)
# B ~ N(0, 1) * K^-0.5 * B_SCALE and bias ~ N(0, 1) * BIAS_SCALE: see gemm_inputs
B_SCALE = 1.0
BIAS_SCALE = 0.25
ADD_SCALE = 0.25


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _nan_framed(vals, layout, device):
    """the operand of logical shape [R, K] (rows = M or N) in its storage layout, as a view into a
    NaN-filled buffer. Layout 0: [R, K] K-contiguous, row stride K + 72 (NaN columns after K), one NaN
    row before and after. Layout 1: [K, R], row stride R + 24 (NaN columns after R), one NaN row before
    K and one after. The view starts one buffer row in: a non-zero multiple of 16 bytes for every
    shape the library accepts (K % 8 == 0 for layout 0, R % 8 == 0 for layout 1).
    Returns (buffer, storage view)."""
    R, K = vals.shape
    if layout == 0:
        buf = torch.full((R + 2, K + 72), float("nan"), dtype=BF)
        buf[1:R + 1, :K] = vals
        buf = buf.to(device)
        return buf, buf[1:R + 1, :K]
    buf = torch.full((K + 2, R + 24), float("nan"), dtype=BF)
    buf[1:K + 1, :R] = vals.T
    buf = buf.to(device)
    return buf, buf[1:K + 1, :R]


def _strided(vals, pad, device, off=0):
    """vals [M, N] as a view at column `off` of rows `pad` wider (zeros around: an epilogue operand
    read out of place shows as a wrong value, not as a NaN the gates would also catch)"""
    M, N = vals.shape
    buf = torch.zeros((M, N + pad), dtype=vals.dtype)
    buf[:, off:off + N] = vals
    buf = buf.to(device)
    return buf[:, off:off + N]


def gemm_inputs(name, M, N, K, al, bl, device="cpu", n_mod=0, need=("addend", "old", "gu"), b_scale=B_SCALE,
                bias_scale=BIAS_SCALE, add_scale=ADD_SCALE):
    """The inputs of one case, seeded from its name, generated on the CPU and moved as whole buffers
    so that the views keep their frames on the device. A dict of
      A, B        bf16 operands in their storage layouts (views into NaN frames, _nan_framed)
      Amk, Bnk    the same memory as logical [M, K] and [N, K] views
      bias [N], addend [M, N] (row stride N + 24), residual [M, N] (row stride N + 16), old [M, N],
      gu [M, 2N] (row stride 2N + 8) for the SwiGLU-backward epilogue,
      residual4: the residual's values in a view 4 elements into a row (8-byte aligned),
      u [M, n_mod * 64] (row stride + 8) and bst [N, 64] for the fused LoRA when n_mod > 0;
    addend, old and gu only when named in `need` (the large cases leave them out).
    A ~ N(0, 1); B ~ N(0, 1) K^-0.5 b_scale; bias and addend ~ N(0, 1) / 4: the pre-activation is
    N(0, ~1.06), and over the >= 78 000 elements of the edge shape it spans about [-4.5, 4.5], both
    tails of GELU and quick_gelu. The issue asked for B scaled by 2 K^-0.5 ([-6, 6] at three sigma);
    with N(0, 1) bias and addend that puts 7 % of a case's elements below -3.3, where 1 + erf cancels
    and the GELU slack of act_check spans several bf16 steps: 8.5 % ambiguous elements against the cap
    of 0.5 % (test_gemm_refs_host.py::test_issue_scale_breaks_the_cap), 0.23 % at these scales. So the
    inputs were changed, as the issue directs, not the cap."""
    g = _gen("gemm-" + name)
    Av = torch.randn(M, K, generator=g).to(BF)
    Bv = (torch.randn(N, K, generator=g) * (K ** -0.5 * b_scale)).to(BF)
    d = {}
    d["A_buf"], d["A"] = _nan_framed(Av, al, device)
    d["B_buf"], d["B"] = _nan_framed(Bv, bl, device)
    d["Amk"] = d["A"] if al == 0 else d["A"].T
    d["Bnk"] = d["B"] if bl == 0 else d["B"].T
    d["bias"] = (torch.randn(N, generator=g) * bias_scale).to(BF).to(device)
    res = torch.randn(M, N, generator=g).to(BF)
    d["residual"] = _strided(res, 16, device)
    d["residual4"] = _strided(res, 16, device, off=4)
    if "addend" in need:
        d["addend"] = _strided((torch.randn(M, N, generator=g) * add_scale).to(BF), 24, device)
    if "old" in need:
        d["old"] = torch.randn(M, N, generator=g).to(BF).to(device)
    if "gu" in need:
        d["gu"] = _strided(torch.randn(M, 2 * N, generator=g).to(BF), 8, device)
    if n_mod:
        d["u"] = _strided(torch.randn(M, n_mod * LORA_R, generator=g).to(BF), 8, device)
        d["bst"] = (torch.randn(N, LORA_R, generator=g) * LORA_R ** -0.5).to(BF).to(device)
    return d


def framed(M, N, dtype, device, off=0, fill=None):
    """C [M, N]: a view into a [M + 2, N + 8] buffer of sentinels (ldc = N + 8, a spare row either
    side), starting `off` (0 or 4) elements into its row. fill [M, N]: the old C of a beta case."""
    buf = torch.full((M + 2, N + 8), SENT, dtype=dtype, device=device)
    view = buf[1:M + 1, off:off + N]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def frame_untouched(buf, M, N, off=0):
    ok = (buf[0] == SENT).all() & (buf[M + 1] == SENT).all() & (buf[:, off + N:] == SENT).all()
    if off:
        ok = ok & (buf[:, :off] == SENT).all()
    return bool(ok)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def ndiff(a, b):
    """elements whose bits differ"""
    return int((bits(a) != bits(b)).sum())


# ---------------------------------------------------------------------------------------------
# G1
# ---------------------------------------------------------------------------------------------
def product_ref(Amk, Bnk):
    """(f64 product A B^T, |A| |B|^T in f64)"""
    Ad, Bd = Amk.double(), Bnk.double()
    return Ad @ Bd.T, Ad.abs() @ Bd.abs().T


def g1(c32, ref, absprod, K, alpha=1.0):
    """(worst err / gate, rel-L2, every element finite) of an f32-output product"""
    err = c32.double() - alpha * ref
    gate = K * E * abs(alpha) * absprod + FLOOR
    nrm = (alpha * ref).norm()
    rel = (err.norm() / nrm).item() if nrm > 0 else float(err.norm() > 0)
    return worst(err, gate), rel, bool(torch.isfinite(c32).all())


def g1_ok(c32, ref, absprod, K, alpha=1.0):
    w, rel, fin = g1(c32, ref, absprod, K, alpha)
    return w <= 1.0 and rel <= 1e-5 and fin


# ---------------------------------------------------------------------------------------------
# G2
# ---------------------------------------------------------------------------------------------
def chain_replay(c32, alpha=1.0, bias=None, addend=None, want_preact=False, rounds=False, residual=None,
                 beta=0.0, old=None, out_dtype=BF, keep=None, drop_scale=1.0):
    """store4 / store8 (gemm_common.h) on the kernel's own f32 plain product, in torch f32:
      v = alpha * c; with output dropout (drop_operand 3: `keep` bool [M, N], `drop_scale` 1 / (1 - p))
      v = keep ? v * drop_scale : 0; v += bias; v = bf16(v) + addend; with a pre-activation output or
      an activation (`rounds`) v = bf16(v), stored as the pre-activation; v = bf16(v) + residual;
      v += beta * old; stored as bf16 or f32.
    Every step is one f32 multiply or add or one bf16 rounding, so this is bit for bit what the
    kernel stores PROVIDED alpha, beta and the dropout scale are powers of two (the cases use alpha in
    {1, 2, 0.5}, beta in {1, 0.5} and p = 0.5 only): alpha * c, v * drop_scale and beta * old are then
    exact, and the replay is the same whether or not the compiler contracts acc * alpha + bias,
    v * drop_scale + bias or v + beta * old into one fma.
    Returns (out, pre-activation or None), the value after the `rounds` step left in f32 when an
    activation follows (the caller applies it)."""
    for s in (alpha, beta, drop_scale):
        assert s == 0.0 or math.frexp(abs(s))[0] == 0.5, "powers of two only"
    v = c32.float() * alpha
    if keep is not None:
        v = torch.where(keep, v * drop_scale, torch.zeros_like(v))
    if bias is not None:
        v = v + bias.float()
    if addend is not None:
        v = bf(v) + addend.float()
    pre = None
    if want_preact or rounds:
        v = bf(v)
        pre = v.to(BF)
    if residual is not None:
        v = bf(v) + residual.float()
    if beta != 0.0:
        v = v + beta * old.float()
    return v.to(out_dtype), pre


# ---------------------------------------------------------------------------------------------
# G3
# ---------------------------------------------------------------------------------------------
def _bf64(y):
    """f64 -> bf16 (through f32: the double rounding moves a value by 2^-24 relative at most, inside
    every slack below), back in f64"""
    return y.float().to(BF).double()


def act_check(out, pre, act):
    """The activation output of a launch against the f64 chain with the documented roundings, on the
    launch's own pre-activation `pre` (bf16, exactly the activation's input x).

    GELU: ref = 0.5 x (1 + erf64(x / sqrt 2)), out = bf16(ref). The kernel evaluates it in f32 with
    erff: the absolute error of erff (~2^-24, where 1 + erf cancels it is all that is left), times
    0.5 |x|, plus three f32 roundings of the value: slack = 2^-21 |x| + 2^-22 |ref|.
    quick_gelu: t = bf16(f32(1.702f * x)) (replayed exactly in torch f32), sg = bf16(sigmoid64(t)),
    out = bf16(sg * x) (8 x 8 significant bits: exact in f32). The kernel's sigmoid is
    v_rcp_f32(1 + v_exp_f32(-t log2 e)), about 1 ulp each: slack = 2^-21 sg on sg.
    An element passes if it lies between the roundings of ref - slack and ref + slack (bf16
    rounding is monotonic): where these two agree the element must equal the rounded f64 value;
    where they differ (the f64 value lies within slack of a rounding boundary) the element is
    AMBIGUOUS and may be either neighbour. First-order share 2 slack / ulp ~ 2^-12; the real shares
    are measured on the CPU (test_gemm_refs_host.py) and must stay <= AMBIGUOUS_CAP.
    Returns (number of failing elements, ambiguous share)."""
    x = pre.double()
    o = out.double()
    if act == ACT_GELU:
        ref = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
        slack = 2.0 ** -21 * x.abs() + 2.0 ** -22 * ref.abs()
        lo, hi = _bf64(ref - slack), _bf64(ref + slack)
    elif act == ACT_QUICK_GELU:
        t = bf(pre.float() * torch.tensor(1.702, dtype=F32, device=pre.device)).double()
        sg = torch.sigmoid(t)
        slack = 2.0 ** -21 * sg
        s_lo, s_hi = _bf64(sg - slack), _bf64(sg + slack)
        a, b = _bf64(s_lo * x), _bf64(s_hi * x)
        lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    else:
        raise ValueError(act)
    bad = ~((o >= lo) & (o <= hi))  # a NaN output fails both comparisons
    amb = (lo != hi)
    return int(bad.sum()), amb.double().mean().item()


def act_f32(x, act, tanh=False, no_t_round=False, plain_sigmoid=False):
    """act_apply restated in torch f32 on the rounded pre-activation x (f32 holding bf16 values);
    the keyword arguments are the mutants of test_gemm_refs_host.py"""
    if act == ACT_GELU:
        if tanh:
            return torch.nn.functional.gelu(x, approximate="tanh")
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))
    if act == ACT_QUICK_GELU:
        t = x if plain_sigmoid else x * torch.tensor(1.702, dtype=F32)
        if not (no_t_round or plain_sigmoid):
            t = bf(t)
        return bf(torch.sigmoid(t)) * x
    return x


# ---------------------------------------------------------------------------------------------
# honest restatements (CPU)
# ---------------------------------------------------------------------------------------------
SLAB = 64  # BK of every kernel in gemm.hip


def product_honest(d, M, N, K, kt_per=None, mutant=None, bm=128):
    """The product restated in torch f32 from the case's framed buffers: 64-deep K slabs summed in
    order; with kt_per, partials of kt_per slabs each, added in split order (splitk_reduce_k).
    The keyword `mutant` names one of the product mutants of test_gemm_refs_host.py."""
    A, B = d["Amk"].float(), d["Bnk"].float()
    if mutant == "pad_cols":  # the K tail's slab read to its end: the NaN columns / rows after K
        Kp = -(-K // SLAB) * SLAB
        A = torch.full((M, Kp), float("nan"))
        A[:, :K] = d["Amk"].float()
        B = torch.cat([B, torch.zeros(N, Kp - K)], 1)
        K = Kp
    if mutant == "row_last_as_0":
        A = A.clone()
        A[M - 1] = A[0]
    if mutant == "chunk_last_mtile":  # one 8-wide chunk of K lost in the last M-tile only
        A = A.clone()
        A[(M - 1) // bm * bm:, 8:16] = 0
    nk = -(-K // SLAB)
    weight = [1.0] * nk  # exact factors: a slab counted 0, 1 or 2 times
    if mutant == "drop_tail":
        weight[-1] = 0.0
    if mutant == "double_slab":
        weight[0] = 2.0
    per = kt_per or nk
    acc = None
    for s0 in range(0, nk, per):
        part = torch.zeros(M, N)
        for s in range(s0, min(nk, s0 + per)):
            lo, hi = s * SLAB, min(K, (s + 1) * SLAB)
            part = part + weight[s] * (A[:, lo:hi] @ B[:, lo:hi].T)
        acc = part if acc is None else acc + part
    return acc


def chain_honest(c, alpha=1.0, bias=None, addend=None, want_preact=False, act=ACT_NONE, residual=None, beta=0.0,
                 old=None, out_dtype=BF, mutant=None, N_tile=256, act_kw=None):
    """store8 restated step by step in torch f32 (activations in torch f32: G3 is what absorbs their
    difference from the kernel's erff / v_exp / v_rcp). Returns (out, pre-activation or None).
    `mutant` names one of the chain mutants of test_gemm_refs_host.py."""
    M, N = c.shape
    v = c.float() * alpha
    if bias is not None:
        b = bias.float()
        if mutant == "bias_shift4":  # the bias group of the last N-tile read 4 columns early
            b = b.clone()
            n0 = (N - 1) // N_tile * N_tile
            b[n0 + 4:] = bias.float()[n0:N - 4]
        if mutant == "bias_after_round":
            v = bf(v) + b
        elif mutant == "alpha_after_bias":
            v = (c.float() + b) * alpha
        else:
            v = v + b
    if addend is not None:
        v = (v if mutant == "addend_no_round" else bf(v)) + addend.float()
    pre = None
    if want_preact or act != ACT_NONE:
        v = bf(v)
        if want_preact:
            pre = v.to(BF)
        v = act_f32(v, act, **(act_kw or {}))
        if mutant == "preact_after_act" and want_preact:
            pre = v.to(BF)
    if residual is not None:
        v = (v if mutant == "residual_before_round" else bf(v)) + residual.float()
    if beta != 0.0:
        v = (bf(v) if mutant == "beta_on_rounded" else v) + beta * old.float()
    return v.to(out_dtype), pre


def lora_addend(d, N, width, scale=LORA_SCALE, swap_module=False):
    """t [M, N] = bf16(scale * u_m B_m^T) per module m = n // width, in torch f32 (K = 64: one slab).
    swap_module: module 1's term from module 0's u (a mutant)"""
    u, bst = d["u"].float(), d["bst"].float()
    cols = []
    for m in range(N // width):
        mu = 0 if (swap_module and m == 1) else m
        cols.append((u[:, mu * LORA_R:(mu + 1) * LORA_R] @ bst[m * width:(m + 1) * width].T) * scale)
    return torch.cat(cols, 1).to(BF)


# ---------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------
# Epilogue variants (name -> options). Every bf16 variant is held to G2's replay of the case's f32
# plain product, the activations to G3 (their pre-activation output to G2), `swiglu` to G4, `lora_*`
# to G5. `c4`: C, residual and pre-activation views start 4 elements into a row (8-byte aligned: epi_lds
# off), bitwise equal to the aligned run as well.
VARIANTS = {
    "plain": dict(),
    "bias_res": dict(bias=True, residual=True),
    "qgelu": dict(bias=True, act=ACT_QUICK_GELU),
    "qgelu_pre": dict(bias=True, act=ACT_QUICK_GELU, preact=True),
    "gelu_full": dict(bias=True, addend=True, preact=True, act=ACT_GELU, residual=True),
    "addend": dict(addend=True),
    "preact": dict(preact=True),
    "beta1_f32": dict(beta=1.0, f32=True),
    "beta05_f32": dict(beta=0.5, f32=True),
    "beta1_bf16": dict(beta=1.0),
    "beta05_bf16": dict(beta=0.5),
    "alpha2_bias": dict(alpha=2.0, bias=True),
    "alpha05_res": dict(alpha=0.5, residual=True),
    "c4": dict(bias=True, residual=True, preact=True, off=4),
    "swiglu": dict(act=ACT_SWIGLU_BWD),
    "lora_none": dict(lora=True),
    "lora_bias": dict(lora=True, bias=True),
    "lora_res": dict(lora=True, residual=True),
    "lora_qgelu_pre": dict(lora=True, bias=True, act=ACT_QUICK_GELU, preact=True),
}
LEAN = ("plain", "bias_res", "qgelu")
GENERAL = ("gelu_full", "addend", "preact", "beta1_f32", "beta05_f32", "beta1_bf16", "beta05_bf16", "alpha2_bias",
           "alpha05_res", "qgelu_pre")
SPLIT = ("plain", "bias_res", "beta1_f32", "beta1_bf16", "qgelu_pre")
KEDGE = ("plain", "bias_res", "gelu_full")
# K <= 8: a sum of so few products is heavy-tailed (K = 1: a product of two normals), 1 % of it lies where
# GELU's slack is ambiguous, over the cap; quick_gelu's slack is relative and stays at ~2^-12
KEDGE_SHORT = ("plain", "bias_res", "qgelu_pre")
LORA = ("lora_none", "lora_bias", "lora_res", "lora_qgelu_pre")
E_SHAPE = (296, 264, 200)  # 2 M-tiles of 288 / 256 / 192 and 3 of 128, 2 N-tiles of 256 and 3 of 128 (8 columns
#                            into the last), 4 K-tiles with an 8-deep tail


def _case(name, M, N, K, al, bl, tile, plan, variants, route, **kw):
    return dict(name=name, M=M, N=N, K=K, al=al, bl=bl, tile=tile, plan=plan, variants=tuple(variants), route=route, **kw)


def _build_cases():
    """`plan` is what cullavo_gemm_plan returns for the shape under the case's forced tile (-1: the
    automatic plan; on the host and on the MI355X alike the plan counts 256 CUs); `route` names the
    terminal launch(es) of gemm_impl the case's variants reach and why. Checked by
    tests/test_gemm_refs_host.py::test_case_table_plans on the host and asserted again on the GPU.
    In the 8-wave kernels the lean variants (LEAN) take the direct epilogue, every other variant the
    LDS-staged general one (lean_case() == -1); the f32 output of every case takes the general one."""
    M, N, K = E_SHAPE
    cs = []
    for al in (0, 1):
        for bl in (0, 1):
            L = f"{al}{bl}"
            # tile 0 / -1: E's automatic plan is the 128x128 tile too (9 tiles; nk = 4 < 8: no split)
            cs.append(_case(f"E-{L}-t0", M, N, K, al, bl, 0, 0, LEAN + GENERAL + ("c4",),
                            f"launch<{al},{bl}> unsplit (gemm_k, store4), bf16 and f32"))
            cs.append(_case(f"E-{L}-auto", M, N, K, al, bl, -1, 0, ("plain", "bias_res"),
                            f"choose_tile -> kT128: launch<{al},{bl}> unsplit"))
            # tile 2, plain and bias_res: at (0,0) launch256p needs dma_pre (K % 64 == 0; the K64-00 and
            # walk64 cases), so K = 200 takes launch256_lean<0,0,256> EPI 1 / 2, as (0,1) and (1,1) do;
            # (1,0) has no lean kernel: launch256 general. qgelu (lean case 2) has a direct kernel only in
            # launch256p / launch288pd, so here it is launch256 general as well
            cs.append(_case(f"E-{L}-t2", M, N, K, al, bl, 2, 2, LEAN + GENERAL + ("c4",),
                            f"launch256<{al},{bl},256,256> general bf16 / f32; plain, bias_res: "
                            + ("launch256 general (no lean kernel at (1,0))" if (al, bl) == (1, 0) else
                               f"launch256_lean<{al},{bl},256> EPI 1 / 2")))
            for t, bm in ((3, 192), (10, 288)):
                if al == 0:
                    lean = (f"launch256_lean<0,{bl},288> EPI 1 / 2 (launch288pd needs dma_pre: K % 64 == 0)"
                            if t == 10 else "launch256 general (192 rows have no lean kernel)")
                    cs.append(_case(f"E-{L}-t{t}", M, N, K, al, bl, t, t, LEAN + GENERAL + ("c4",),
                                    f"launch256<0,{bl},{bm},256> general bf16 / f32; plain, bias_res: {lean}"))
                else:  # 192 / 288 rows need a K-contiguous A: the plan and gemm_impl fall back to 256 rows
                    cs.append(_case(f"E-{L}-t{t}", M, N, K, al, bl, t, 2, ("plain", "bias_res", "gelu_full"),
                                    f"tile {t} with a_layout 1 falls back to kT256x256: as E-{L}-t2"))
    # K edges at E's M and N: one K-tile (no loop), one partial tile, tile + 8, two tiles + 8
    for Ke in (64, 8, 72, 136):
        for al, bl in ((0, 0), (0, 1), (1, 0), (1, 1)):
            for t in (0, 2) + ((10,) if al == 0 else ()):
                cs.append(_case(f"K{Ke}-{al}{bl}-t{t}", M, N, Ke, al, bl, t, t, KEDGE if Ke > 8 else KEDGE_SHORT,
                                "K % 64 == 0 and (0,0): dma_pre = 1, so tile 2 lean -> launch256p "
                                "(gemm256pd_k<0 / 1, 256>) and tile 10 lean -> launch288pd (gemm256pd_k<0 / 1, 288>)"
                                if Ke == 64 and (al, bl) == (0, 0) else "as the E case of this layout and tile"))
    for Ke in (203, 1):  # any K when both operands are K-strided (the header)
        for t in (0, 2):
            cs.append(_case(f"K{Ke}-11-t{t}", M, N, Ke, 1, 1, t, t, KEDGE if Ke > 8 else KEDGE_SHORT,
                            "launch<1,1> / launch256_lean<1,1,256> + launch256<1,1,256,256> at a K that is no "
                            "multiple of 8"))
    # persistent walk: 18 x 17 = 306 tiles of 256 rows, 16 x 17 = 272 of 288 rows over 256 workgroups
    for t, tiles in ((2, 306), (10, 272)):
        cs.append(_case(f"walk-00-t{t}", 4360, 4104, 136, 0, 0, t, t, LEAN,
                        "K = 136: dma_pre = 0, so the lean variants take launch256_lean (one tile per "
                        "workgroup); the walk itself is walk64-*", tiles=tiles))
        cs.append(_case(f"walk64-00-t{t}", 4360, 4104, 128, 0, 0, t, t, LEAN,
                        f"launch256p / launch288pd: gemm256pd_k<0 / 1 / 2, {256 if t == 2 else 288}> walks "
                        f"{tiles} tiles on min(tiles, CUs) workgroups (K % 64 == 0: dma_pre = 1); f32: launch256 general",
                        tiles=tiles))
    # split-K on the 8-wave kernel: splitk256_plan = min(256 / 4, 33 / 8) = 4 splits of 9 K-tiles (the last
    # split 6 and the 8-deep tail)
    for al, bl in ((0, 0), (0, 1), (1, 1)):
        cs.append(_case(f"split256-{al}{bl}", 264, 264, 2056, al, bl, -1, 9, SPLIT,
                        f"launch256<{al},{bl},256,256> with p.part (gemm256_k partials) + splitk_reduce_k<bf16 / f32>",
                        kt_per=9, workspace=True))
    # split-K on the 128x128 kernel: M < 256 so splitk256_plan = 1; splitk_plan: 2 tiles, nk = 9 -> 2 splits
    # of 5 K-tiles. Route checked by cullavo_gemm_workspace > 0 and plan != 9
    for al, bl in ((0, 0), (1, 1)):
        cs.append(_case(f"split128-{al}{bl}", 72, 136, 520, al, bl, -1, 0, SPLIT,
                        f"launch<{al},{bl}> with p.part (gemm_k partials) + splitk_reduce_k", kt_per=5,
                        workspace=True))
    # the plan's splits: the lowest-FLOP shapes (ragged N, K tail of 8) at which cullavo_gemm_plan returns
    # 100 + tile, found by a host search over M in steps of 8, N = 256 j + 8, K in {136 .. 4104}
    cs.append(_case("msplit-110", 10385, 1544, 1032, 0, 0, -1, 110, ("plain", "bias_res"),
                    "M-tail split: head 36 x 288 = 10368 rows -> launch256_lean<0,0,288> (K % 64 != 0), tail 17 "
                    "rows -> rows_from -> launch<0,0> split over K (4 x 5 K-tiles) + splitk_reduce_k", mm=10368,
                    workspace=True))
    cs.append(_case("msplit-110-lora", 10385, 1792, 1032, 0, 0, -1, 110, ("lora_res",),
                    "the same split with the fused LoRA (N a multiple of the module width 256): head "
                    "launch256<0,0,256,256,LORA> (K < 2048), tail rows_from (lora_u + mm ld) -> the same, 17 rows",
                    mm=10368, n_mod=7, width=256, workspace=True))
    cs.append(_case("rsplit-102-00", 9217, 1800, 2056, 0, 0, -1, 102, ("plain", "bias_res"),
                    "round split: head 32 x 256 = 8192 rows -> launch256_lean<0,0,256>, tail 1025 rows -> "
                    "split-256 (4 x 9 K-tiles) + splitk_reduce_k", mm=8192, workspace=True))
    cs.append(_case("rsplit-102-11", 4824, 3336, 1032, 1, 1, -1, 102, ("plain", "bias_res"),
                    "round split at (1,1): head 18 x 256 = 4608 rows -> launch256_lean<1,1,256>, tail 216 rows "
                    "(A + mm elements: a column offset) -> launch<1,1> split over K", mm=4608, workspace=True))
    # SwiGLU backward (G4): C and gu are 2N wide
    for bl in (0, 1):
        for t in (0, 2, 3, 10):
            cs.append(_case(f"swiglu-0{bl}-t{t}", M, N, K, 0, bl, t, t, ("swiglu",),
                            {0: f"launch<0,{bl}>: store4 -> swiglu_bwd_store<4>",
                             2: f"launch256<0,{bl},256,256,SWG> (lds_epilogue_swiglu)",
                             3: f"launch256<0,{bl},192,256> general: store8 -> swiglu_bwd_store<8>",
                             10: f"launch256<0,{bl},288,256,SWG>"}[t]))
    # fused LoRA (G5): two modules of 256 columns
    for t, plan in ((2, 2), (10, 10), (-1, 0)):
        cs.append(_case(f"lora-00-t{t}", 296, 512, 200, 0, 0, t, plan, LORA,
                        "launch256<0,0,288,256,LORA> (tile 10 forced)" if t == 10 else
                        "launch256<0,0,256,256,LORA> (every other plan)", n_mod=2, width=256))
    # decode-row boundary: 16 rows stream through gemv.hip (plan 14, pinned in the decode tests), 17 are tiled
    cs.append(_case("rows16-00", 16, N, K, 0, 0, -1, 14, ("plain", "bias_res"), "cvgemm_launch_gemv"))
    cs.append(_case("rows17-00", 17, N, K, 0, 0, -1, 0, ("plain", "bias_res"), "launch<0,0> unsplit: one M-tile"))
    return cs


CASES = _build_cases()
# cases whose host checks run on a subset (the honest restatement of rows [0, 136) and the last 136
# rows): everything else runs whole
LARGE = tuple(c["name"] for c in CASES if c["M"] * c["N"] * c["K"] > 1 << 28)


def case_inputs(c, device="cpu", **kw):
    """gemm_inputs of a case of the table: only the operands its variants read"""
    opts = [VARIANTS[v] for v in c["variants"]]
    need = tuple(k for k, on in (("addend", any(o.get("addend") for o in opts)),
                                 ("old", any(o.get("beta") for o in opts)),
                                 ("gu", any(o.get("act") == ACT_SWIGLU_BWD for o in opts))) if on)
    return gemm_inputs(c["name"], c["M"], c["N"], c["K"], c["al"], c["bl"], device, c.get("n_mod", 0), need, **kw)
