"""References, gates, case tables, input builders and honest restatements for the f32 parity mode:
csrc/gemm_f32.hip (gemm_f32_k) and csrc/attn_generic.hip with attn_gen_fwd_body.h (attn_gen_fwd_k
plain and cached, attn_gen_fwd_ragged_k, attn_gen_delta_k, attn_gen_bwd_kv_k, attn_gen_bwd_q_k).
tests/test_parity_refs_host.py proves on the CPU that every gate passes an honest restatement of the
kernel's order on every case and fails each listed one-line mutant on at least one;
tests/test_parity_accuracy_gpu.py holds the kernels to the same gates on the same inputs.

E = 2^-24 is the largest relative error of one f32 round-to-nearest, U = 2^-8 that of bf16; Ust is the
stored type's. No number here was taken from a kernel's output.

GEMM gates
 P0  the f32 output without an epilogue is BITWISE fma_chain(A, B): acc = 0; acc = fmaf(a_k, b_k, acc)
     for k = 0 .. K-1, the contract the kernel's header states. fma_chain emulates fmaf exactly in f64:
     the product of two f32 values is exact in f64 (48 bits), the sum p + acc is rounded TO ODD (the f64
     round-to-nearest sum, moved one f64 step towards the TwoSum error term when that term is not zero
     and the sum's last bit is even), and a round-to-odd value of 53 >= 2 * 24 + 2 bits rounds to f32 as
     the exact sum does. tests/test_parity_refs_host.py proves it against fractions.Fraction. A zero
     padded K tail adds fmaf(0, 0, acc) = acc (acc is never -0: an exact zero sum is +0).
 P1  |c - A B^T| <= K 2^-24 (|A| |B|^T) + FLOOR per element and rel-L2 <= 1e-5 (gemm_refs.g1).
 P2  the epilogue (alpha, output dropout, bias, addend, pre-activation store, residual, beta) BITWISE
     epilogue_replay on the kernel's own plain product: alpha, beta and the dropout scale powers of two,
     so each product is exact and the replay is the same whether or not a multiply-add is contracted.
 P3  what cannot be bitwise, against f64 on the kernel's own pre-activation x (f32, exactly the
     activation's input) or plain product:
       GELU        |y - 0.5 x (1 + erf(x / sqrt 2))| <= 2^-21 |x| + 2^-22 |ref|: gemm_refs.act_check's slack
                   (erff's absolute error where 1 + erf cancels, times 0.5 |x|, with margin; three f32
                   roundings of the value) -- the f32 store's own rounding is one of the three;
       quick_gelu  |y - x sigmoid(z)| <= (|z| + 6) 2^-23 |ref|, z = 1.702f x: train_refs' SwiGLU form
                   ((|g| + 6) 2^-23: the product's and v_exp's argument roundings grow with |z|, plus exp,
                   add, divide and the constant) without its two bf16 roundings;
       + residual  one more f32 rounding: + E |ref + residual|;
       dropout scale 1 / (1 - p) not a power of two (mode 3): |y - c s| <= E |c s|, s the f32 scale: one
                   rounding; dropped elements exactly 0.
 P4  the kept set is oracle.lora_keep_mask exactly (== 0 where dropped; for modes 1 and 2 read through an
     identity operand), modes 1 and 2 BITWISE fma_chain on f32(x * scale), drop_p = 0 BITWISE the plain
     product.

Attention gates: see the section below.
"""
import math

import numpy as np
import torch

from oracle import cullavo_oracle as O
from tests.decode_refs import U, _gen, worst
from tests.gemm_refs import SENT, bits, frame_untouched, framed, g1, g1_ok, ndiff, product_ref  # noqa: F401
from tests.train_refs import E, FLOOR

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
ACT_NONE, ACT_GELU, ACT_QUICK_GELU = 0, 1, 2
FB, FK, GROUP = 128, 16, 8   # gemm_f32_k: tile edge, K step, M-tiles per group
NAN = float("nan")


def ust(dtype):
    return U if dtype == BF else E


# =============================================================================================
# A. gemm_f32_k
# =============================================================================================
def fma_f64(a, b, acc):
    """fmaf(a, b, acc) of f32 values held in float64 numpy arrays, exactly (P0 above)"""
    p = a * b                                # exact
    s = p + acc
    bb = s - p
    err = (p - (s - bb)) + (acc - bb)        # TwoSum: s + err = p + acc exactly
    odd = (s.view(np.int64) & 1).astype(bool)
    fix = (err != 0) & ~odd
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32).astype(np.float64)


def fma_double_rounded(a, b, acc):
    """the mutant of fma_f64: the f64 sum cast to f32 (two roundings)"""
    return (a * b + acc).astype(np.float32).astype(np.float64)


def fma_chain(Amk, Bnk, fma=fma_f64, pairwise=False):
    """f32 [M, N]: the k-ordered chain from zero of P0. Amk [M, K], Bnk [N, K] f32 tensors (any device).
    pairwise (a mutant): even and odd k on two chains, added at the end."""
    A = Amk.detach().cpu().double().numpy()
    B = Bnk.detach().cpu().double().numpy()
    M, K = A.shape
    acc = [np.zeros((M, B.shape[0])), np.zeros((M, B.shape[0]))]
    for k in range(K):
        w = k & 1 if pairwise else 0
        acc[w] = fma(A[:, k:k + 1], B[None, :, k], acc[w])
    out = acc[0]
    if pairwise:
        out = (acc[0] + acc[1]).astype(np.float32)
    return torch.from_numpy(out.astype(np.float32)).to(Amk.device)


# ---- inputs ---------------------------------------------------------------------------------
def _nan_framed32(vals, layout, device):
    """the f32 operand of logical shape [R, K] in its storage layout, a view into a NaN buffer.
    Layout 0: [R, K], row stride K + 24, a NaN row before and after. Layout 1: [K, R], row stride R + 8,
    a NaN row before and 17 after (a whole 16-deep K step of NaN behind the operand in either layout).
    Returns (buffer, storage view, padded logical [R, ceil16(K)] view whose columns >= K are the margin)."""
    R, K = vals.shape
    Kp = -(-K // FK) * FK
    if layout == 0:
        buf = torch.full((R + 2, K + 24), NAN, dtype=F32)
        buf[1:R + 1, :K] = vals
        buf = buf.to(device)
        return buf, buf[1:R + 1, :K], buf[1:R + 1, :Kp]
    buf = torch.full((K + 18, R + 8), NAN, dtype=F32)
    buf[1:K + 1, :R] = vals.T
    buf = buf.to(device)
    return buf, buf[1:K + 1, :R], buf[1:Kp + 1, :R].T


def _strided(vals, pad, device):
    M, N = vals.shape
    buf = torch.zeros((M, N + pad), dtype=vals.dtype)
    buf[:, :N] = vals
    return buf.to(device)[:, :N]


def gemm_inputs(name, M, N, K, al, bl, device="cpu", identity=None):
    """Seeded from the name, built on the CPU, moved as whole buffers. A, B ~ N(0, 1) (unit scale, no
    subnormals: A / B follow the denorm mode); bias, addend ~ N(0, 1) / 4, residual, old ~ N(0, 1).
    ldr = N + 16, ld_addend = N + 24, ldc = N + 8 (gemm_refs.framed): all different.
    identity 'A' / 'B': that operand is the identity (K = M resp. K = N), to read a dropout mask."""
    g = _gen("parity-gemm-" + name)
    Av, Bv = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    if identity == "A":
        Av = torch.eye(M, K)
    if identity == "B":
        Bv = torch.eye(N, K)
    d = {}
    d["A_buf"], d["A"], d["Apad"] = _nan_framed32(Av, al, device)
    d["B_buf"], d["B"], d["Bpad"] = _nan_framed32(Bv, bl, device)
    d["Amk"] = d["A"] if al == 0 else d["A"].T
    d["Bnk"] = d["B"] if bl == 0 else d["B"].T
    d["bias"] = (torch.randn(N, generator=g) * 0.25).to(device)
    d["residual"] = _strided(torch.randn(M, N, generator=g), 16, device)
    d["addend"] = _strided(torch.randn(M, N, generator=g) * 0.25, 24, device)
    d["old"] = torch.randn(M, N, generator=g).to(device)
    return d


# ---- dropout --------------------------------------------------------------------------------
def drop_scale(p):
    """the host's f32 1.f / (1.f - p) (cullavo_gemm_f32_impl)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed, rows, cols, p, device="cpu", mutant=None):
    """bool [rows = tokens, cols = features]"""
    if mutant == "drop_swapped":          # token and feature swapped in the hash
        m = O.lora_keep_mask(seed, cols, rows, p).T
    elif mutant == "drop_thr_off_by_one":  # u16 > thr: the threshold one higher
        m = O.lora_keep_mask(seed, rows, cols, p + 2.0 ** -16)
    else:
        m = O.lora_keep_mask(seed, rows, cols, p)
    return torch.from_numpy(np.ascontiguousarray(m)).to(device)


def dropped_operand(x, keep, p):
    """f32(x * scale) where kept, 0 where dropped: what f32_drop stages"""
    return torch.where(keep, x * torch.tensor(drop_scale(p), dtype=F32, device=x.device), torch.zeros_like(x))


# ---- P2 / P3 --------------------------------------------------------------------------------
def epilogue_replay(c32, alpha=1.0, keep=None, p=0.0, bias=None, addend=None, residual=None, beta=0.0, old=None):
    """f32_epilogue with act none on the kernel's own plain product, torch f32 (P2). Returns (out, the
    value at the pre-activation store)."""
    for s in (alpha, beta, drop_scale(p)):
        assert s == 0.0 or math.frexp(abs(s))[0] == 0.5, "powers of two only"
    v = c32 * alpha
    if keep is not None:
        v = torch.where(keep, v * drop_scale(p), torch.zeros_like(v))
    if bias is not None:
        v = v + bias
    if addend is not None:
        v = v + addend
    pre = v
    if residual is not None:
        v = v + residual
    if beta != 0.0:
        v = v + beta * old
    return v, pre


def act_ref(x, act):
    """(f64 activation of the f32 pre-activation x, its P3 gate)"""
    xd = x.double()
    if act == ACT_GELU:
        ref = 0.5 * xd * (1.0 + torch.erf(xd / math.sqrt(2.0)))
        return ref, 2.0 ** -21 * xd.abs() + 2.0 ** -22 * ref.abs() + FLOOR
    z = float(np.float32(1.702)) * xd
    ref = xd * torch.sigmoid(z)
    return ref, (z.abs() + 6.0) * 2.0 ** -23 * ref.abs() + FLOOR


def p3_act(out, pre, act, residual=None):
    """worst err / gate of an activation output (P3)"""
    ref, gate = act_ref(pre, act)
    if residual is not None:
        ref = ref + residual.double()
        gate = gate + E * ref.abs()
    return worst(out.double() - ref, gate)


def p3_drop(out, c32, keep, p):
    """(worst err / gate over the kept elements, dropped elements that are not == 0) of mode 3"""
    ref = c32.double() * drop_scale(p)
    w = worst((out.double() - ref)[keep], (E * ref.abs() + FLOOR)[keep])
    return w, int((out[~keep] != 0).sum())


# ---- the honest restatement -----------------------------------------------------------------
def tile_order(tiles_m, tiles_n, mutant=None):
    """[(tile row, tile column)] in workgroup order: gemm_f32_k's grouped order"""
    out = []
    per_group = GROUP * tiles_n
    for lid in range(tiles_m * tiles_n):
        first_m = (lid // per_group) * GROUP
        gsize = GROUP if mutant == "gsize_8" else min(tiles_m - first_m, GROUP)
        r, c = first_m + (lid % per_group) % gsize, (lid % per_group) // gsize
        if mutant == "tile_swapped":
            r, c = first_m + (lid % per_group) // gsize, (lid % per_group) % gsize
        out.append((r, c))
    return out


def product_honest(d, M, N, K, mutant=None, a_drop=None, b_drop=None):
    """The plain product as gemm_f32_k forms it: per tile in workgroup order, K in 16-deep steps read from
    the padded storage (the NaN margin behind K guarded to zero), each element an fma_f64 chain. Returns
    (C [M, N] f32, NaN where no workgroup stored; visits [tiles_m, tiles_n]).
    a_drop / b_drop: (keep [R, K] in the operand's logical shape, p) of dropout modes 1 / 2."""
    A, B = d["Apad"].cpu().clone(), d["Bpad"].cpu().clone()
    Kp = A.shape[1]
    if mutant == "tail_dropped":
        Kp = K // FK * FK
    elif mutant != "tail_unguarded":
        A[:, K:] = 0.0
        B[:, K:] = 0.0
    for X, dr in ((A, a_drop), (B, b_drop)):
        if dr is not None:
            X[:, :K] = dropped_operand(X[:, :K], dr[0], dr[1])
    tm, tn = -(-M // FB), -(-N // FB)
    C = torch.full((M, N), NAN, dtype=F32)
    visits = torch.zeros((tm, tn), dtype=torch.int32)
    fma = fma_double_rounded if mutant == "fma_double_rounded" else fma_f64
    for r, c in tile_order(tm, tn, mutant):
        if r >= tm or c >= tn:
            continue  # every element of such a tile fails the m < M / n < N guard
        visits[r, c] += 1
        m0, n0 = r * FB, c * FB
        C[m0:m0 + FB, n0:n0 + FB] = fma_chain(A[m0:m0 + FB, :Kp], B[n0:n0 + FB, :Kp], fma, mutant == "pairwise")
    return C, visits


def beta_in_place(prod, visits, old, beta):
    """C = prod + beta * C applied once per visit of a tile (a tile visited twice reads its own output, one
    never visited keeps the old C): what the grouped-order cases with beta = 1 see"""
    C = old.clone()
    for r in range(visits.shape[0]):
        for c in range(visits.shape[1]):
            sl = (slice(r * FB, (r + 1) * FB), slice(c * FB, (c + 1) * FB))
            for _ in range(int(visits[r, c])):
                C[sl] = torch.nan_to_num(prod[sl], nan=0.0) + beta * C[sl]
    return C


def act_f32(x, act):
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))
    if act == ACT_QUICK_GELU:
        return x / (1.0 + torch.exp(torch.tensor(-1.702, dtype=F32) * x))
    return x


def epilogue_honest(c, N, ldc, alpha=1.0, keep=None, p=0.0, bias=None, addend=None, want_preact=False, act=ACT_NONE,
                    residual=None, beta=0.0, old=None, mutant=None):
    """f32_epilogue step by step in numpy / torch f32 on flat [M * ldc] output buffers (so that a wrong
    leading dimension lands where the kernel's would). Returns (C view [M, N], pre-activation view or
    None, C buffer, pre-activation buffer), the buffers [M + 2, ldc] sentinel frames."""
    M = c.shape[0]
    s = torch.tensor(drop_scale(p), dtype=F32)
    v = c * torch.tensor(alpha, dtype=F32)
    b = bias if bias is not None else None
    if keep is not None and mutant != "drop_after_bias":
        v = torch.where(keep, v * s, torch.zeros_like(v))
    if b is not None and mutant != "bias_after_act":
        v = v + b
    if keep is not None and mutant == "drop_after_bias":
        v = torch.where(keep, v * s, torch.zeros_like(v))
    if addend is not None:
        v = v + addend
    if residual is not None and mutant == "residual_before_act":
        v = v + residual
    pre = v
    v = act_f32(v, act)
    if b is not None and mutant == "bias_after_act":
        v = v + b
    if residual is not None and mutant != "residual_before_act":
        v = v + residual
    if beta != 0.0:
        v = (v * beta + old) if mutant == "beta_on_new" else (v + beta * old)
    cbuf = torch.full((M + 2, ldc), SENT, dtype=F32)
    cbuf[1:M + 1, :N] = v
    pbuf = pview = None
    if want_preact:
        pbuf = torch.full((M + 2, ldc), SENT, dtype=F32)
        ld = N if mutant == "preact_ld_n" else ldc
        flat = pbuf.view(-1)
        idx = (ldc + torch.arange(M)[:, None] * ld + torch.arange(N)[None, :]).reshape(-1)
        flat[idx] = pre.reshape(-1)
        pview = pbuf[1:M + 1, :N]
    return cbuf[1:M + 1, :N], pview, cbuf, pbuf


# ---- the case table -------------------------------------------------------------------------
# The library's shared argument checks (gemm_impl) hold for f32 operands too: N, lda, ldb, ldc, ldr % 8 == 0,
# K % 8 == 0 unless both layouts are 1, M % 8 == 0 for a_layout 1. Shapes outside them (261 x 137 x 203 at every
# layout, 1 x 1 x 5, N = 260, K = 20 or 1 at (0,0)) return CULLAVO_EINVAL before gemm_f32_k is reached, so the
# table holds the nearest shapes the library accepts; layout 1's per-element `i0 + i4 + j < imax` guards can
# therefore never decide within a group of 4 (test_parity_accuracy_gpu.py asserts the rejection).
E_SHAPES = {(0, 0): (261, 136, 200), (0, 1): (261, 136, 200), (1, 0): (264, 136, 200), (1, 1): (264, 136, 203)}
E_SHAPE = E_SHAPES[(0, 0)]  # 3 x 2 tiles, ragged M and N; K ends 8 into a 16-step (11 at (1,1), no multiple of 4)
# epilogue variants under P2 (act none; alpha, beta, the dropout scale powers of two)
EPI_P2 = {
    "alpha": dict(alpha=0.5),
    "drop3": dict(drop=0.5),
    "bias": dict(bias=True),
    "addend": dict(addend=True),
    "preact": dict(preact=True),
    "residual": dict(residual=True),
    "beta025": dict(beta=0.25),
    "beta1": dict(beta=1.0),
    "all": dict(alpha=0.5, drop=0.5, bias=True, addend=True, preact=True, residual=True, beta=0.25),
    "all_beta1": dict(alpha=0.5, drop=0.5, bias=True, addend=True, preact=True, residual=True, beta=1.0),
}
# activations under P3
EPI_P3 = {
    "gelu": dict(act=ACT_GELU, bias=True, preact=True, residual=True),
    "qgelu": dict(act=ACT_QUICK_GELU, bias=True, preact=True, residual=True),
}
# chosen on the CPU from oracle.lora_keep_mask alone (a search over 0xC0FFEE << 32 | n, n < 400) so that at every
# (features, p) of DROP_CASES at least one element's 16-bit hash EQUALS the threshold: with a random seed one
# element in 65536 does, and a `>` in place of `>=` would show on none of these small masks
DROP_SEED = 0xC0FFEE_0000_0076


def _g(name, M, N, K, al, bl, why, epi=(), beta1=False):
    return dict(name=name, M=M, N=N, K=K, al=al, bl=bl, why=why, epi=tuple(epi), beta1=beta1)


def _gemm_cases():
    cs = []
    for al in (0, 1):
        for bl in (0, 1):
            M, N, K = E_SHAPES[(al, bl)]
            full = (al, bl) in ((0, 0), (1, 1))
            cs.append(_g(f"E-{al}{bl}", M, N, K, al, bl, "the edge shape: ragged M / N / K at every layout; the "
                         "epilogue variants at (0,0) and (1,1)", tuple(EPI_P2) + tuple(EPI_P3) if full else ("all",)))
    for Kk in (1, 3, 15, 16, 17, 32, 33):
        cs.append(_g(f"K{Kk}-11", 72, 40, Kk, 1, 1, "nk = 1 (K <= 16), K < 4, one step and one over, two steps and "
                     "one over"))
    for Kk in (8, 16, 24, 32, 40):
        cs.append(_g(f"K{Kk}-00", 70, 40, Kk, 0, 0, "the multiples of 8 around one and two K steps"))
    cs.append(_g("one-00", 1, 8, 8, 0, 0, "a single row of the narrowest N"))
    cs.append(_g("one-11", 8, 8, 5, 1, 1, "the smallest (1,1) shape, K = 5"))
    cs.append(_g("tile", 128, 128, 16, 0, 0, "exact tiles, one K step"))
    cs.append(_g("tile+1", 129, 136, 16, 0, 0, "one row and 8 columns into a second tile"))
    for Mg, tm in ((1030, 9), (1400, 11), (2100, 17)):
        for Ng in (40, 136, 264):
            cs.append(_g(f"grp-{Mg}x{Ng}", Mg, Ng, 24, 0, 0, f"grouped order: tiles_m {tm} (last group of {tm % 8}), "
                         f"tiles_n {-(-Ng // FB)}; plain under P0 and beta = 1 onto a random C", beta1=True))
    return cs


GEMM_CASES = _gemm_cases()
# dropout: (name, mode, tokens, features, p). Mode 1: A = x [tokens, features] at (0,0), N = 40; mode 2:
# B = x [tokens, features] at (1,1) (K = tokens), M = 40; mode 3: C [tokens, features], K = 24
DROP_CASES = [(f"drop{mode}-f{F}-p{p}", mode, 136, F, p) for mode in (1, 2, 3) for F in (96, 264)
              for p in (0.5, 0.25, 0.05)]
GEMM_PRODUCT_MUTANTS = ("tail_dropped", "tail_unguarded", "pairwise", "gsize_8", "tile_swapped")
GEMM_EPI_MUTANTS = ("preact_ld_n", "bias_after_act", "residual_before_act", "beta_on_new", "drop_after_bias")
GEMM_DROP_MUTANTS = ("drop_swapped", "drop_thr_off_by_one")


def drop_dims(mode, T, F):
    """(M, N, K, al, bl) of a dropout case"""
    return {1: (T, 40, F, 0, 0), 2: (40, F, T, 1, 1), 3: (T, F, 24, 0, 0)}[mode]


# =============================================================================================
# B. generic attention
# =============================================================================================
"""Gates (first order, from the kernels' rounding points). For a query row i with n live keys, scores
s_ij = scale q_i . k_j, lse_i, p_ij = exp(s_ij - lse_i):

 rho_ij = (|s| + |lse| + |s - lse| + 2) 2^-23 + (D + 2) E scale sum_d |q_d k_d|
     the relative error of one probability: train_refs' ce_bwd form (the argument s - lse carries the
     roundings of s * scale, lse and the subtraction, each relative 2^-24 of its operand and doubled for
     __expf's own argument product; + 2 for v_exp and the final scaling) plus the score's own D-term fma
     chain, (D + 2) E sum |q_d k_d| absolute in s and so relative in p.
 LSE  live rows within 1e-5 absolute (the project's gate), the largest error finite and > 0; dead rows
     exactly +inf.
 O    Ust |ref| + sum_j p_j (2 rho_j + (n + 2 blocks + 8) E) |v_j|: the forward's p is exp(s - m) / l: both
     numerator and l (a sum of such terms: n E for its additions, 2 E per block for alpha and the rescale)
     carry rho, hence 2 rho; the n-term fma chain of the output adds n E; the division, inv and the store
     the rest.
 dV   Ust |ref| + sum_i p_ij (rho_ij + (rows + 8) E) |dO_i|, rows = Lq: the backward's p = exp(s - lse)
     carries rho once; an fma chain over the query rows.
 dQ   Ust |ref| + scale sum_j [ p (rho |dp - delta| + (D + 2) E sum_d |dO v| + (D + 2) E sum_d |dO o|)
                                + (terms + 8) E |dS| ] |k_j|, terms = Lk: dS = p (dp - delta) carries p's rho on
     the difference, the absolute errors of the two D-term sums dp and delta (which do not shrink when
     dp - delta cancels), and the fma chain over the keys.
 dK   the same with |q_i| and terms = Lq.
Exact zeros (== 0): O and dQ rows of queries with no live key, dK and dV rows of keys below kv_start[b],
every tensor of a batch row with kv_start == Lk. Everything finite. The backward reference takes the lse
it is given (P = exp(S - lse)) and delta from the o it is given, as FA2 defines both.
"""
H = 3
KB, QF, QB = 64, 64, 32


def _heads(x, B, L, D, dt=F64):
    return x.to(dt).reshape(B, L, -1, D).transpose(1, 2)  # [B, h, L, D]


def _flat(x):
    B, h, L, D = x.shape
    return x.transpose(1, 2).reshape(B * L, h * D)


def visibility(c, mutant=None, device="cpu"):
    """bool [B, Lq, Lk]: the keys each query attends in case c (kind packed / cached / ragged); the mask
    mutants of the host test change it here"""
    B, Lq, Lk = c["B"], c["Lq"], c["Lk"]
    i = torch.arange(Lq, device=device)[None, :, None]
    j = torch.arange(Lk, device=device)[None, None, :]
    ks = torch.tensor(c["ks"] if c["ks"] is not None else [0] * B, device=device)[:, None, None]
    vis = (j > ks) if mutant == "ks_gt" else (j >= ks)
    if c["kind"] == "packed":
        if c["causal"]:
            vis = vis & ((j < i) if mutant == "causal_lt" else (j <= i))
        kl = torch.full((B, 1, 1), Lk, device=device)
        past = torch.zeros((B, 1, 1), dtype=torch.long, device=device)
        qp = torch.zeros((B, 1, 1), dtype=torch.long, device=device)
    else:
        kl = torch.tensor(c["kv_len"], device=device)[:, None, None]
        qp = torch.tensor(c["q_pad"], device=device)[:, None, None]
        past = kl - Lq
        if mutant == "past_omitted":
            past = torch.zeros_like(past)
        vis = vis & ((j < past + i) if mutant == "causal_lt" else (j <= past + i)) & (j < kl)
        if mutant != "qpad_unmasked":
            vis = vis & (i >= qp)
    vis = vis.expand(B, Lq, Lk).clone()
    # the key loop's end per 64-row query block, and the ragged early-out (blocks the kernel never stages)
    for b in range(B):
        for q0 in range(0, Lq, QF):
            kend = int(kl[b]) if not (c["causal"] or c["kind"] != "packed") else min(int(kl[b]), int(past[b]) + q0 + QF)
            if mutant == "kend_short":
                kend = max(0, -(-kend // KB) * KB - KB)
            out = q0 + QF <= int(qp[b]) + (QF if mutant == "early_out_far" else 0)
            if c["kind"] == "ragged" and out:
                kend = 0
            vis[b, q0:q0 + QF, -(-kend // KB) * KB:] = False
    return vis


def attn_ref(q, k, v, c, vis):
    """f64 softmax attention over the live keys. q [B*Lq, H*D]; k, v [B, Lk, H*D] (packed: the [B*Lk] rows
    viewed so; non-finite rows are masked ones and count as 0). Returns a dict of O [B*Lq, H*D], LSE
    [B, H, Lq] (+inf on dead rows), S, P [B, H, Lq, Lk], live [B, Lq], n [B, Lq]."""
    B, Lq, Lk, D = c["B"], c["Lq"], c["Lk"], c["D"]
    Q = _heads(q, B, Lq, D)
    K = _heads(torch.nan_to_num(k.double(), nan=0.0), B, Lk, D)
    V = _heads(torch.nan_to_num(v.double(), nan=0.0), B, Lk, D)
    S = (Q @ K.transpose(-1, -2)) * c["scale"]
    Sm = S.masked_fill(~vis[:, None], float("-inf"))
    live = vis.any(-1)
    lse = torch.logsumexp(Sm, -1)
    P = torch.exp(Sm - lse.masked_fill(~live[:, None], 0.0)[..., None])
    lse = lse.masked_fill(~live[:, None], float("inf"))
    return dict(O=_flat(P @ V), LSE=lse, S=S, P=P, live=live, n=vis.sum(-1), Q=Q, K=K, V=V, vis=vis)


def _rho(r, c, P=None):
    S, lse = r["S"], torch.where(torch.isinf(r["LSE"]), torch.zeros_like(r["LSE"]), r["LSE"])[..., None]
    qk = (r["Q"].abs() @ r["K"].abs().transpose(-1, -2)) * c["scale"]
    return (S.abs() + lse.abs() + (S - lse).abs() + 2.0) * 2.0 ** -23 + (c["D"] + 2) * E * qk


def o_gate(r, c):
    blocks = -(-c["Lk"] // KB)
    per_row = ((r["n"] + 2 * blocks + 8) * E)[:, None, :, None].double()
    w = r["P"] * (2.0 * _rho(r, c) + per_row)
    return ust(c["dtype"]) * r["O"].abs() + _flat(w @ r["V"].abs()) + FLOOR


def bwd_ref(r, c, do, o_given, lse_given):
    """f64 backward from the given (stored) o and lse. Returns dict dQ, dK, dV [.., H*D] and their gates."""
    B, Lq, Lk, D, scale = c["B"], c["Lq"], c["Lk"], c["D"], c["scale"]
    dO, Og = _heads(do, B, Lq, D), _heads(o_given, B, Lq, D)
    lse = lse_given.double()
    dead = torch.isinf(lse)
    P = torch.exp(r["S"] - lse.masked_fill(dead, 0.0)[..., None]).masked_fill(~r["vis"][:, None], 0.0)
    P = P.masked_fill(dead[..., None], 0.0)
    dP = dO @ r["V"].transpose(-1, -2)
    delta = (dO * Og).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    out = dict(dQ=_flat(dS @ r["K"]) * scale, dK=_flat(dS.transpose(-1, -2) @ r["Q"]) * scale,
               dV=_flat(P.transpose(-1, -2) @ dO))
    us = ust(c["dtype"])
    rr = dict(r, LSE=lse)
    rho = _rho(rr, c)
    gv = P * (rho + (Lq + 8) * E)
    out["dV_gate"] = us * out["dV"].abs() + _flat(gv.transpose(-1, -2) @ dO.abs()) + FLOOR
    abs_dp = dO.abs() @ r["V"].abs().transpose(-1, -2)
    abs_dl = (dO.abs() * Og.abs()).sum(-1, keepdim=True)
    core = P * (rho * (dP - delta).abs() + (D + 2) * E * (abs_dp + abs_dl))
    gq = core + (Lk + 8) * E * dS.abs()
    gk = core + (Lq + 8) * E * dS.abs()
    out["dQ_gate"] = us * out["dQ"].abs() + scale * _flat(gq @ r["K"].abs()) + FLOOR
    out["dK_gate"] = us * out["dK"].abs() + scale * _flat(gk.transpose(-1, -2) @ r["Q"].abs()) + FLOOR
    return out


def lse_check(lse, r):
    """(max |err| over live rows, dead rows that are not +inf)"""
    live = r["live"][:, None].expand_as(r["LSE"])
    err = (lse.double() - r["LSE"])[live].abs()
    bad = int((lse[~live] != float("inf")).sum())
    return (err.max().item() if err.numel() else None), bad


def zero_checks(c, r, o=None, dq=None, dk=None, dv=None):
    """{name: rows that must be == 0 and are not}"""
    B, Lq, Lk = c["B"], c["Lq"], c["Lk"]
    dead_q = (~r["live"]).reshape(B * Lq)
    out = {}
    if o is not None:
        out["O_dead_rows"] = int((o[dead_q] != 0).any(-1).sum())
    if dq is not None:
        out["dQ_dead_rows"] = int((dq[dead_q] != 0).any(-1).sum())
    if dk is not None:
        ks = torch.tensor(c["ks"] if c["ks"] is not None else [0] * B, device=dk.device)
        below = (torch.arange(Lk, device=dk.device)[None] < ks[:, None]).reshape(B * Lk)
        out["dK_below_start"] = int((dk[below] != 0).any(-1).sum())
        out["dV_below_start"] = int((dv[below] != 0).any(-1).sum())
    return out


# ---- honest restatements --------------------------------------------------------------------
def fwd_honest(q, k, v, c, mutant=None):
    """attn_gen_fwd_body.h in torch f32: 64-key blocks, the running maximum, alpha, l and o rescaled per
    block, o * (1 / l) stored in the storage type. K / V rows the kernel stages as zeros (rows >= Lk; V rows
    below kv_start in the cached kernels) are zeros here. Returns (o [B*Lq, H*D] storage type, lse f32)."""
    B, Lq, Lk, D, scale = c["B"], c["Lq"], c["Lk"], c["D"], c["scale"]
    vis = visibility(c, mutant)
    Q, K, V = _heads(q, B, Lq, D, F32), _heads(k, B, Lk, D, F32), _heads(v, B, Lk, D, F32)
    if mutant == "v_head0":
        V = V[:, :1].expand_as(V)
    ks = c["ks"] if c["ks"] is not None else [0] * B
    if c["kind"] != "packed":
        V = V.clone()
        for b in range(B):
            if mutant != "v_below_start_read":
                V[b, :, :ks[b]] = 0.0
            V[b, :, c["kv_len"][b]:] = 0.0
    m = torch.full((B, Q.shape[1], Lq), float("-inf"))
    l = torch.zeros_like(m)
    o = torch.zeros((B, Q.shape[1], Lq, D))
    sc = torch.tensor(scale, dtype=F32)
    for k0 in range(0, Lk, KB):
        s = (Q @ K[:, :, k0:k0 + KB].transpose(-1, -2)) * sc
        s = torch.where(vis[:, None, :, k0:k0 + KB], s, torch.full_like(s, float("-inf")))
        mnew = torch.maximum(m, s.max(-1).values)
        alpha = torch.where(mnew == float("-inf"), torch.ones_like(m), torch.exp(m - mnew))
        p = torch.where(s == float("-inf"), torch.zeros_like(s), torch.exp(s - mnew[..., None]))
        l = (l if mutant == "l_not_rescaled" else l * alpha) + p.sum(-1)
        m = mnew
        if mutant != "o_not_rescaled":
            o = o * alpha[..., None]
        o = o + p @ V[:, :, k0:k0 + KB]
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    lse = torch.where(l > 0, m + (0.0 if mutant == "lse_no_log" else torch.log(l)), torch.full_like(l, float("inf")))
    return _flat(o * inv[..., None]).to(c["dtype"]), lse


def bwd_honest(q, k, v, o, do, lse, c, mutant=None):
    """attn_gen_delta_k, attn_gen_bwd_kv_k and attn_gen_bwd_q_k in torch f32 (packed kernels). Returns
    (dq, dk, dv) in the storage type."""
    B, Lq, Lk, D, scale = c["B"], c["Lq"], c["Lk"], c["D"], c["scale"]
    vis = visibility(c, mutant if mutant in ("causal_lt", "ks_gt") else None)
    vis_q = visibility(c, "kend_short") if mutant == "kend_short" else vis
    vis_kv = vis
    if mutant == "qstart_late" and c["causal"]:
        vis_kv = vis.clone()
        for k0 in range(0, Lk, KB):
            vis_kv[:, :k0 // QB * QB + QB, k0:k0 + KB] = False
    Q, K, V = _heads(q, B, Lq, D, F32), _heads(k, B, Lk, D, F32), _heads(v, B, Lk, D, F32)
    dO, Og = _heads(do, B, Lq, D, F32), _heads(o, B, Lq, D, F32)
    if mutant == "v_head0":
        V = V[:, :1].expand_as(V)
    delta = (dO * Og).sum(-1, keepdim=True)
    if mutant == "delta_wrong_head":
        delta = delta.roll(1, 1)
    if mutant == "ds_no_delta":
        delta = torch.zeros_like(delta)
    sc = torch.tensor(scale, dtype=F32)
    dead = torch.isinf(lse)[..., None]
    arg = (Q @ K.transpose(-1, -2)) * sc - torch.where(dead, torch.zeros_like(lse[..., None]), lse[..., None])
    dP = dO @ V.transpose(-1, -2)

    def p_ds(vv):
        p = torch.where(vv[:, None] & ~dead, torch.exp(arg), torch.zeros_like(arg))
        return p, p * (dP - delta)
    p_kv, ds_kv = p_ds(vis_kv)
    _, ds_q = p_ds(vis_q)
    dv = p_kv.transpose(-1, -2) @ dO
    dk = ((p_kv if mutant == "dk_with_p" else ds_kv).transpose(-1, -2) @ Q) * sc
    dq = ds_q @ K
    if mutant != "dq_no_scale":
        dq = dq * sc
    return tuple(_flat(t).to(c["dtype"]) for t in (dq, dk, dv))


FWD_MUTANTS = ("causal_lt", "ks_gt", "kend_short", "o_not_rescaled", "l_not_rescaled", "lse_no_log", "past_omitted",
               "qpad_unmasked", "early_out_far", "v_head0", "v_below_start_read")
BWD_MUTANTS = ("causal_lt", "ks_gt", "kend_short", "qstart_late", "ds_no_delta", "dq_no_scale", "dk_with_p", "v_head0",
               "delta_wrong_head")


# ---- cases ----------------------------------------------------------------------------------
def _a(name, kind, D, dtype, Lq, Lk, causal=False, ks=None, why="", **kw):
    c = dict(name=f"{name}-D{D}{'bf' if dtype == BF else 'f32'}", kind=kind, B=2, D=D, dtype=dtype, Lq=Lq, Lk=Lk,
             causal=bool(causal), ks=ks, scale=D ** -0.5, why=why, struct=None, layout=False, chain=False,
             kv_len=None, q_pad=None, past=None)
    c.update(kw)
    return c


def _attn_cases():
    cs = []
    for D, dt in ((32, F32), (16, BF), (16, F32), (64, F32), (128, F32), (32, BF)):
        full = (D, dt) in ((32, F32), (16, BF))
        for L in (1, 63, 64, 65, 131):
            for causal in (0, 1):
                cs.append(_a(f"L{L}{'c' if causal else ''}", "packed", D, dt, L, L, causal, (0, min(3, L - 1)),
                             "one row; one under, on and one over a 64-key / 64-query block; three blocks"))
        # (causal with Lq != Lk, e.g. (130, 70), is an argument error of cullavo_attn_fwd / _bwd: "causal attention
        # needs Lq == Lk", asserted in test_parity_accuracy_gpu.py; the cached entry points are its causal form)
        for Lq, Lk, causal in ((70, 33, 0), (33, 130, 0)):
            cs.append(_a(f"Lq{Lq}Lk{Lk}{'c' if causal else ''}", "packed", D, dt, Lq, Lk, causal, (0, 5),
                         "Lq != Lk: fewer and more keys than queries, a partial and a third key block"))
        for ks in ((0, 1), (63, 64), (65, 129), (130, 131)):
            for causal in (0, 1):
                cs.append(_a(f"ks{ks[0]}-{ks[1]}{'c' if causal else ''}", "packed", D, dt, 131, 131, causal, ks,
                             "kv_start either side of a block edge: a wholly masked first key block, causal queries "
                             "below kv_start, Lk - 1 and Lk (a sequence with nothing live)"))
        if not full:
            continue
        for st in ("rising", "planted", "cancel"):
            for causal in (0, 1):
                cs.append(_a(f"{st}{'c' if causal else ''}", "packed", D, dt, 200, 200, causal, (0, 7),
                             "score structure: every block raises the row maximum / the largest score on the last "
                             "key / dO = 0.5 O + noise so dp - delta cancels", struct=st))
        cs.append(_a("layout", "packed", D, dt, 131, 131, 1, (0, 9), "q | k | v and dq | dk | dv column blocks of one "
                     "buffer each, O through out= into a wider buffer, sentinels around every output", layout=True))
        cs.append(_a("chain", "packed", D, dt, 131, 131, 1, (0, 9), "the backward fed the forward kernel's own o and lse",
                     chain=True))
        for Lq, past in ((2, 1), (33, 63), (70, 100), (130, 200), (5, 64)):
            cs.append(_a(f"cached-{Lq}-{past}", "cached", D, dt, Lq, past + Lq, 1, (0, 67), "cached prefill: the first "
                         "queries of sequence 1 see nothing (kv_start 67)", kv_len=(past + Lq,) * 2, q_pad=(0, 0),
                         past=past))
        # ragged: kv_len[b] >= Lq - q_pad[b] always (ops.attn_fwd_ragged documents kv_len as counting this call's
        # Lq - q_pad new rows, so a smaller kv_len is not a documented input). Of the crossing of Lq {70, 130},
        # kv_len {(200, 45), (130, 3)} and q_pad {(0, 64), (0, 67)} that leaves the Lq = 70 combinations below; at
        # Lq = 130 sequence 1 needs kv_len >= 66, so (200, 70) and (130, 66) stand in for (200, 45) and (130, 3)
        rag = [(70, (200, 45), (0, 64)), (70, (200, 45), (0, 67)), (70, (130, 3), (0, 67)),
               (130, (200, 70), (0, 64)), (130, (200, 70), (0, 67)), (130, (130, 66), (0, 64)), (130, (130, 66), (0, 67))]
        for Lq, kl, qp in rag:
            for ks in (None, (0, 2)):
                cs.append(_a(f"ragged-{Lq}-{kl[0]}-{kl[1]}-p{qp[1]}{'ks' if ks else ''}", "ragged", D, dt, Lq, max(kl), 1,
                             ks, "ragged: a padding block ending on a query-block edge (64) and just past it (67), the "
                             "early-out, several key blocks", kv_len=kl, q_pad=qp))
    return cs


ATTN_CASES = _attn_cases()
CACHE_SPARE = 37  # NaN rows behind the longest sequence


def attn_inputs(c, device="cpu"):
    """q, do [B*Lq, H*D]; packed: k, v [B*Lk, H*D]; cached / ragged: k, v caches [B, Lk + 37, H*D] whose rows
    >= kv_len[b] and rows < kv_start[b] are NaN. Seeded from the case name, CPU, then moved."""
    B, Lq, Lk, D, dt = c["B"], c["Lq"], c["Lk"], c["D"], c["dtype"]
    g = _gen("parity-attn-" + c["name"])
    hd = H * D
    q = torch.randn(B * Lq, hd, generator=g)
    rows = Lk if c["kind"] == "packed" else Lk + CACHE_SPARE
    k = torch.randn(B, rows, hd, generator=g)
    v = torch.randn(B, rows, hd, generator=g)
    do = torch.randn(B * Lq, hd, generator=g)
    if c["struct"] in ("rising", "planted"):  # every query shares a component along u: s_ij gains 2 k_j . u
        u = torch.zeros(D)
        u[0] = 1.0
        q = (q.view(B * Lq, H, D) + 2.0 * D ** 0.5 * u).view(B * Lq, hd)
    if c["struct"] == "rising":   # + 4 per 64-key block on scores of unit spread (the last block has 8 keys)
        k = (k.view(B, rows, H, D) + 2.0 * (torch.arange(rows) // KB).float()[None, :, None, None] * u).view(B, rows, hd)
    if c["struct"] == "planted":  # s = 12 +- 1.5 on the last key against a largest other score of ~6
        k[:, Lk - 1] = (6.0 * u).repeat(H)
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    if c["struct"] == "cancel":
        r = attn_ref(q, k, v, c, visibility(c))
        do = 0.5 * r["O"].float() + 0.1 * do
    do = do.to(dt)
    if c["kind"] != "packed":
        ks = c["ks"] if c["ks"] is not None else [0] * B
        for b in range(B):
            for t in (k, v):
                t[b, c["kv_len"][b]:] = NAN
                t[b, :ks[b]] = NAN
    else:
        k, v = k.view(B * Lk, hd), v.view(B * Lk, hd)
    return tuple(t.to(device) for t in (q, k, v, do))


def kv_rows(c, k):
    """k or v as [B, Lk, H*D] for attn_ref / the honest forms"""
    return k.view(c["B"], c["Lk"], -1) if c["kind"] == "packed" else k[:, :c["Lk"]]
