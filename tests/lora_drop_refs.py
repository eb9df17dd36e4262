"""References, gates, inputs and the case table for the bf16 GEMM's three dropout modes (csrc/gemm.hip
gemm_k<.., DROP> with drop_tile, store4 / store8 / splitk_reduce_k with drop_mode 3, csrc/gemm_common.h)
and for lora_dx_k (csrc/lora.hip): every adapter product of a LoRA training step with dropout.
tests/test_lora_drop_refs_host.py proves on the CPU, for these very inputs, that an honest f32
restatement passes every gate and that each listed one-line mutant fails at least one;
tests/test_lora_drop_accuracy_gpu.py holds the kernels to the same gates. Operands are views into NaN
frames with padded row strides, outputs views into sentinel frames (gemm_refs). The mask is
oracle.lora_keep_mask (parity_refs.keep_mask), the scale s = f32(1 / (1 - p)) (parity_refs.drop_scale).
E = 2^-24, U = 2^-8 (one f32 / bf16 round-to-nearest, relative). No number here was taken from a
kernel's output.

The arithmetic, from the code:
 modes 1, 2  the staged operand element is bf16(f32(x) * s) where kept and +0 where dropped (drop_tile):
             one f32 multiply and one round-to-nearest-even cast, restated exactly by `staged`. Products of
             bf16 values are exact in f32, so the only error left is the f32 summation.
 mode 3      v = alpha * acc; v = keep ? v * s : 0; then the documented chain (bias, addend, pre-activation,
             residual, beta, store): gemm_refs.chain_replay with keep / drop_scale.
 lora_dx_k   for m = 0 .. n-1 in order dx = bf16((keep_m ? acc_m * s : 0) + dx), acc_m the 64-deep f32 product
             of du[:, 64 m : 64 m + 64] and a_stack[64 m : 64 m + 64]; rounded after every module.

The gates:
 D1  the mask bit for bit: ones through the dropped operand against an identity, f32 output: exactly
     float(bf16(s)) where the oracle keeps, exactly 0 where it drops. T = 136, F in (96, 264), seed
     parity_refs.DROP_SEED, p in D1_P. The issue names p in (0.05, 0.1, 0.5) as "the (F, p) sets of
     parity_refs.DROP_CASES, where a hash equals the threshold"; DROP_CASES holds p in (0.5, 0.25, 0.05), and
     at p = 0.1 no element of these masks has a hash equal to the threshold (counted from the oracle alone,
     threshold_hits). D1_P is therefore the union (0.05, 0.1, 0.25, 0.5): the issue's three run, and every
     (F, p) of DROP_CASES keeps its threshold element (asserted on the CPU).
 D2  the dropped-operand product. f32 output against f64 of the exactly staged operand under gemm_refs' G1:
     |c - alpha A_d B^T| <= K 2^-24 |alpha| (|A_d| |B|^T) + FLOOR per element ((K - 1) 2^-24 sum |a_k b_k| bounds
     the f32 summation of K exact products in ANY order) and rel-L2 <= 1e-5; the bf16 output and the epilogue
     variants bit for bit chain_replay of the kernel's own f32 product of the same launch (G2); drop_p = 0
     with drop_operand set bitwise the plain call.
 D3  mode 3. p = 0.5 (s = 2): every variant bitwise chain_replay with the drop step, on the kernel's own plain
     f32 product of the same route. p in (0.05, 0.1): s is not a power of two, so v * s rounds and the
     compiler may contract v * s + (next addend) into one fma:
       f32 output, no other option: |y - c s| <= E |c s| + FLOOR on kept elements (one rounding; parity_refs P3),
       dropped elements exactly 0;
       bf16 output with beta = 1 (the production call): y must lie between bf16(ref - slack) and
       bf16(ref + slack), ref = c s + old in f64. The kernel forms either t = fl(c s), y32 = fl(t + old):
       |y32 - ref| <= E |c s| (1 + E) + E |ref|, or y32 = fl(fma(c, s, old)): <= E |ref|. slack is the larger,
       the first. Where the two roundings of ref -+ slack agree the element must equal the rounded f64
       value; where they differ it is AMBIGUOUS and may be either neighbour. First-order share
       2 slack / (bf16 spacing) ~ 2^-14; measured on the CPU for both f32 forms and held <= AMBIGUOUS_CAP.
       Dropped elements: slack 0, so exactly bf16(beta * old) = old.
 L1  lora_dx_k bitwise the per-module gemm_ex(0, 1, K = 64, drop_operand 3, beta 1) launches, which D3 pins.
 L2  lora_dx_k against f64, r_m = r_(m-1) + (keep_m ? c_m s : 0) in f64 from r_(-1) = dx, c_m the f64 product:
       n_mod = 1: round-or-neighbour as D3 with slack = keep ? s 64 E (|du| |A|) + E |c s| (1 + E) + E |r| : 0:
         the 64-term f32 sum (any order), the scaling, the addition;
       n_mod = 2, 3: |dx - r_(n-1)| <= (1 + 4 U) sum_m [ U |r_m| + E |r_m| + keep_m (s 64 E (|du_m| |A_m|) + E |c_m s|) ]
         + FLOOR: each module's stored value is one bf16 rounding (U |r_m|) of one f32 addition (E |r_m|) of
         the scaled 64-term sum; an earlier module's error enters the later ones unchanged (the additions
         are of exact values), and the factor 1 + 4 U covers |r_m| being the kernel's value, not the
         reference's, to second order. A module applied with another's mask, or onto the original dx, is
         off by whole products c s ~ 1: hundreds of times the bound.
     Rows and columns outside [M, N] keep the sentinel.
"""
import torch

from cullavo_amd.lora import module_seed
from tests import gemm_refs as G
from tests.decode_refs import U, _gen, bf, worst
from tests.parity_refs import DROP_CASES, DROP_SEED, drop_scale, keep_mask  # noqa: F401 (DROP_CASES: for the tests)
from tests.train_refs import E, FLOOR

BF = torch.bfloat16
F32 = torch.float32
SLAB = G.SLAB
TILE = 128  # BM = BN of gemm_k
D1_T = 136
D1_F = (96, 264)
D1_P = (0.05, 0.1, 0.25, 0.5)
P_PROD = 0.05          # the training recipe's lora_dropout
LORA_STEP_SEED, LORA_UID = 20240521, 7  # module_seed(step seed, group uid, m): distinct per module


# ---------------------------------------------------------------------------------------------
# the mask and the staged operand
# ---------------------------------------------------------------------------------------------
def threshold_hits(F, p, T=D1_T, seed=DROP_SEED):
    """elements whose 16-bit hash EQUALS the threshold, from the oracle alone: kept at thr, dropped at thr + 1"""
    return int((keep_mask(seed, T, F, p) & ~keep_mask(seed, T, F, p, mutant="drop_thr_off_by_one")).sum())


def scale_t(p, device="cpu"):
    return torch.tensor(drop_scale(p), dtype=F32, device=device)


def mask(seed, T, F, p, device="cpu", mutant=None, k_axis=None, k0=0, i_axis=None):
    """keep [tokens, features] and the mask mutants of the host test.
    halves_swapped: the odd / even 16-bit halves of a pair's hash exchanged;
    slab_relative_k: from k0 on along `k_axis` (the axis K runs over: 1 = features in mode 1, 0 = tokens in
      mode 2) the mask of k - k0, the second split hashing its slab-relative k;
    tile_relative: along `i_axis` (the M / N index of the operand) the mask of i % 128 (t - m0)."""
    if mutant in ("drop_swapped", "drop_thr_off_by_one"):
        return keep_mask(seed, T, F, p, device, mutant)
    k = keep_mask(seed, T, F, p, device)
    if mutant == "halves_swapped":
        k = k.view(T, F // 2, 2).flip(2).reshape(T, F)
    if mutant == "slab_relative_k" and k0:
        k = k.clone()
        if k_axis == 1:
            k[:, k0:] = k[:, :F - k0].clone()
        else:
            k[k0:] = k[:T - k0].clone()
    if mutant == "tile_relative":
        idx = torch.arange(k.shape[i_axis], device=k.device) % TILE
        k = k.index_select(i_axis, idx)
    return k


def staged(x, keep, p, mutant=None, k_axis=1, K=None):
    """drop_tile exactly: bf16(f32(x) * s) where kept, +0 where dropped; x bf16 [tokens, features]. Returns f32
    holding the staged values.
    no_scale_ktail: the elements of the last, partial K-tile (k >= K // 64 * 64 along k_axis) kept unscaled;
    not_rounded: scaled but left in f32."""
    xs = x.float() * scale_t(p, x.device)
    if mutant != "not_rounded":
        xs = bf(xs)
    if mutant == "no_scale_ktail":
        k0 = K // SLAB * SLAB
        xs = xs.clone()
        if k_axis == 1:
            xs[:, k0:] = x.float()[:, k0:]
        else:
            xs[k0:] = x.float()[k0:]
    return torch.where(keep, xs, torch.zeros_like(xs))


# ---------------------------------------------------------------------------------------------
# round-or-neighbour (gemm_refs.act_check's mechanism)
# ---------------------------------------------------------------------------------------------
def ron(out, ref, slack):
    """(elements outside [bf16(ref - slack), bf16(ref + slack)], ambiguous share); a NaN fails"""
    lo, hi = G._bf64(ref - slack), G._bf64(ref + slack)
    o = out.double()
    bad = ~((o >= lo) & (o <= hi))
    return int(bad.sum()), (lo != hi).double().mean().item()


def d3_ron(out, c32, keep, p, old):
    """D3: the bf16 output with beta = 1 at a scale that is no power of two"""
    cs = torch.where(keep, c32.double() * drop_scale(p), torch.zeros_like(c32, dtype=torch.float64))
    ref = cs + old.double()
    slack = torch.where(keep, E * cs.abs() * (1 + E) + E * ref.abs(), torch.zeros_like(ref))
    return ron(out, ref, slack)


def d3_f32(out, c32, keep, p):
    """D3: (worst err / gate over the kept elements, dropped elements that are not == 0) of the f32 output"""
    ref = c32.double() * drop_scale(p)
    w = worst((out.double() - ref)[keep], (E * ref.abs() + FLOOR)[keep])
    return w, int((out[~keep] != 0).sum())


# ---------------------------------------------------------------------------------------------
# mode 3 restated (host)
# ---------------------------------------------------------------------------------------------
def drop_chain_honest(c, keep, p, alpha=1.0, bias=None, addend=None, want_preact=False, residual=None, beta=0.0,
                      old=None, out_dtype=BF, mutant=None, contracted=False):
    """store4 / store8 with drop_mode 3, step by step in torch f32. contracted: v * s + (the operand added
    next: the bias, or beta * old where nothing else lies between) as one fma, emulated in f64: the product of
    two f32 values is exact there, so only the sum rounds, and the cast to f32 rounds again -- a double
    rounding that differs from fmaf on ~2^-29 of all values and stays inside every slack. Mutants:
    drop_after_bias, beta_before_drop. Returns (out, pre-activation or None)."""
    s = scale_t(p)
    v = c.float() * alpha
    z = torch.zeros_like(v)
    b = bias.float() if bias is not None else None
    if mutant == "beta_before_drop":
        v = torch.where(keep, (v + beta * old.float()) * s, z)
        beta = 0.0
        if b is not None:
            v = v + b
    elif mutant == "drop_after_bias":
        v = torch.where(keep, (v + b) * s, z)
    else:
        nxt = b
        if nxt is None and beta != 0.0 and addend is None and not want_preact and residual is None:
            nxt = beta * old.float()
        if contracted and nxt is not None:
            v = torch.where(keep, (v.double() * s.double() + nxt.double()).float(), z + nxt)
            if b is None:
                beta = 0.0
        else:
            v = torch.where(keep, v * s, z)
            if b is not None:
                v = v + b
    if addend is not None:
        v = bf(v) + addend.float()
    pre = None
    if want_preact:
        v = bf(v)
        pre = v.to(BF)
    if residual is not None:
        v = bf(v) + residual.float()
    if beta != 0.0:
        v = v + beta * old.float()
    return v.to(out_dtype), pre


# ---------------------------------------------------------------------------------------------
# lora_dx
# ---------------------------------------------------------------------------------------------
def _nan_rows(vals, ld, device):
    """vals [R, C] bf16 as a view into a NaN buffer [R + 2, ld]"""
    R, C = vals.shape
    buf = torch.full((R + 2, ld), float("nan"), dtype=BF)
    buf[1:R + 1, :C] = vals
    buf = buf.to(device)
    return buf, buf[1:R + 1, :C]


def dx_frame(d, device=None):
    """a fresh dx: (sentinel buffer [M + 2, N + 4], view [M, N] holding dx0), ld_dx = N + 4"""
    M, N = d["dx0"].shape
    buf = torch.full((M + 2, N + 4), G.SENT, dtype=BF, device=device or d["dx0"].device)
    view = buf[1:M + 1, :N]
    view.copy_(d["dx0"])
    return buf, view


def lora_seeds(n_mod):
    return [module_seed(LORA_STEP_SEED, LORA_UID, m) for m in range(n_mod)]


def lora_inputs(n_mod, M, N, device="cpu", cancelling=False):
    """du [M, 64 n] (ld 64 n + 8) and a_stack [64 n, N] (ld N + 24), views into NaN frames; dx0 [M, N] ~ N(0, 1) / 4.
    du = (row sign) |N(0, 1)| / 2 and a_stack = (column sign) |N(0, 1)| 2^-(3 + column % 3): the 64 terms of one
    element share a sign, so |c| = |du| |A| ~ 2.5, 1.3 or 0.64 (both signs) and dx rarely cancels it: L2's
    n_mod = 1 slack, s 64 E |du| |A|, is ~4e-6 of the value, an ambiguous share of ~0.1-0.2 % against the cap of
    0.5 %. With N(0, 1) / 2 and N(0, 1) / 8 operands and dx ~ N(0, 1) the terms cancel, |du| |A| ~ 5 |c|, and
    1.3-1.8 % of the honest restatement's elements are ambiguous
    (test_lora_drop_refs_host.py::test_cancelling_inputs_break_the_cap): the inputs were chosen, as the issue
    directs, not the cap."""
    g = _gen(f"lora-dx-{n_mod}-{M}-{N}")
    R = G.LORA_R
    d = {}
    rs = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
    cs = torch.where(torch.rand(1, N, generator=g) < 0.5, -1.0, 1.0) * 2.0 ** -(3 + torch.arange(N) % 3).float()
    du = torch.randn(M, R * n_mod, generator=g)
    a = torch.randn(R * n_mod, N, generator=g)
    if cancelling:
        du, a = du * 0.5, a * R ** -0.5
    else:
        du, a = du.abs() * 0.5 * rs, a.abs() * cs
    d["du_buf"], d["du"] = _nan_rows(du.to(BF), R * n_mod + 8, device)
    d["a_buf"], d["a"] = G._nan_framed(a.to(BF).T, 1, device)  # [64 n, N], row stride N + 24
    d["dx0"] = (torch.randn(M, N, generator=g) * (1.0 if cancelling else 0.25)).to(BF).to(device)
    return d


def lora_dx_honest(d, n_mod, p, seeds, mutant=None, contracted=False):
    """lora_dx_k restated in torch f32 on a sentinel-framed dx. Returns (buffer, view). Mutants: seed_m0 (module 1
    hashes with module 0's seed), old_from_dx0 (every module adds onto the original dx), rows_past_M (the row
    after the last is stored too: a zero product onto a zero `old`)."""
    M, N = d["dx0"].shape
    R = G.LORA_R
    s = scale_t(p)
    buf, view = dx_frame(d)
    dx0 = d["dx0"].float()
    run = dx0
    for m in range(n_mod):
        acc = d["du"][:, R * m:R * (m + 1)].float() @ d["a"][R * m:R * (m + 1)].float()
        keep = keep_mask(seeds[0] if (mutant == "seed_m0" and m == 1) else seeds[m], M, N, p)
        old = dx0 if mutant == "old_from_dx0" else run
        if contracted:
            v = torch.where(keep, (acc.double() * s.double() + old.double()).float(), old)
        else:
            v = torch.where(keep, acc * s, torch.zeros_like(acc)) + old
        run = bf(v)
    view.copy_(run)
    if mutant == "rows_past_M":
        buf[M + 1, :N] = 0.0
    return buf, view


def lora_dx_ref(d, n_mod, p, seeds):
    """(r_(n-1) in f64, the L2 bound for n_mod >= 2, the L2 slack for n_mod = 1)"""
    M, N = d["dx0"].shape
    R = G.LORA_R
    s = drop_scale(p)
    r = d["dx0"].double()
    bound = torch.zeros_like(r)
    slack = None
    for m in range(n_mod):
        du, a = d["du"][:, R * m:R * (m + 1)].double(), d["a"][R * m:R * (m + 1)].double()
        c, ab = du @ a, du.abs() @ a.abs()
        keep = keep_mask(seeds[m], M, N, p, device=r.device)
        z = torch.zeros_like(r)
        r = r + torch.where(keep, c * s, z)
        prod = torch.where(keep, s * R * E * ab + E * (c * s).abs() * (1 + E), z)
        slack = torch.where(keep, prod + E * r.abs(), z)
        bound = bound + prod + (E + U) * r.abs()
    return r, (1 + 4 * U) * bound + FLOOR, slack


def lora_dx_check(view, d, n_mod, p, seeds):
    """L2 of a dx view: (failing elements, ambiguous share or None, worst err / bound or None)"""
    r, bound, slack = lora_dx_ref(d, n_mod, p, seeds)
    if n_mod == 1:
        bad, amb = ron(view, r, slack)
        return bad, amb, None
    err = view.double() - r
    bad = int((~(err.abs() <= bound)).sum())  # a NaN fails
    return bad, None, worst(err, bound)


# ---------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------
# epilogue variants (gemm_refs.VARIANTS, activation-free: the bitwise ones)
D2_VARIANTS = ("plain", "bias_res", "addend", "beta1_f32", "beta1_bf16", "alpha2_bias")
D3_VARIANTS = ("plain", "bias_res", "addend", "preact", "beta1_f32", "beta05_f32", "beta1_bf16", "beta05_bf16",
               "alpha2_bias", "alpha05_res")
D3_SPLIT_VARIANTS = ("plain", "bias_res", "preact", "beta1_f32", "beta1_bf16")
D3_P_RON = (0.05, 0.1)


def _case(name, mode, M, N, K, al, bl, tile=-1, plan=0, kt_per=None, route=""):
    return dict(name=name, mode=mode, M=M, N=N, K=K, al=al, bl=bl, tile=tile, plan=plan, kt_per=kt_per,
                workspace=kt_per is not None, route=route, inputs=f"drop{mode}-{M}x{N}x{K}-{al}{bl}")


def _cases():
    """`plan`: cullavo_gemm_plan under the forced tile; `kt_per`: K-tiles per split where the library splits
    (cullavo_gemm_workspace > 0 exactly there), from splitk_plan / splitk256_plan; both checked on the host
    (test_lora_drop_refs_host.py::test_case_table_routes) and asserted again on the GPU."""
    cs = []
    for M, N, K, kt, why in ((136, 40, 96, None, "one K-tile and a 32-wide tail, a ragged second M-tile"),
                             (136, 64, 200, None, "a K tail of 8"),
                             (72, 64, 520, 5, "2 splits of 5 K-tiles: the second slab's mask needs the absolute k"),
                             (264, 64, 520, 5, "three M-tiles (m0 > 0), split")):
        cs.append(_case(f"m1-{M}x{N}x{K}", 1, M, N, K, 0, 0, kt_per=kt,
                        route=f"launch<0,0,CT,1>: gemm_k drop_tile<0> on A{' + splitk_reduce_k' if kt else ''}; {why}"))
    for al in (0, 1):
        for M, N, K, kt, why in ((64, 96, 136, None, "M = r, N = features, K = tokens: a K tail of 8"),
                                 (64, 264, 136, None, "N crosses two 128-column tiles (n0 > 0)"),
                                 (64, 264, 520, 5, "split over K: tokens along K")):
            cs.append(_case(f"m2-{al}1-{M}x{N}x{K}", 2, M, N, K, al, 1, kt_per=kt,
                            route=f"launch<{al},1,CT,2>: gemm_k drop_tile<1> on B{' + splitk_reduce_k' if kt else ''}; {why}"))
    for M, N in ((136, 264), (300, 520)):
        for tile, plan, r in ((-1, 0, "choose_tile -> kT128: launch<0,1> store4"), (0, 0, "launch<0,1> store4"),
                              (2, 2, "launch256_lean declines (lean_case -1) -> launch256<0,1,256,256> LDS epilogue, store8"),
                              (3, 3, "launch256<0,1,192,256> LDS epilogue, store8"),
                              (10, 10, "launch256_lean<0,1,288> declines -> launch256<0,1,288,256> LDS epilogue, store8")):
            cs.append(_case(f"m3-{M}x{N}-t{tile}", 3, M, N, 64, 0, 1, tile=tile, plan=plan, route=r))
    for bl in (0, 1):
        cs.append(_case(f"m3-split256-0{bl}", 3, 264, 264, 2056, 0, bl, plan=9, kt_per=9,
                        route=f"launch256<0,{bl},256,256> partials (4 x 9 K-tiles) + splitk_reduce_k: the mask in the "
                              "reduction's store4"))
    cs.append(_case("m3-split128-01", 3, 72, 136, 520, 0, 1, kt_per=5,
                    route="launch<0,1> partials (2 x 5 K-tiles) + splitk_reduce_k"))
    return cs


CASES = _cases()
LORA_CASES = [(1, 1, 8), (1, 65, 264), (2, 63, 256), (2, 130, 520), (3, 64, 264), (3, 129, 8)]  # (n_mod, M, N)
LORA_P = (0.05, 0.5)
LORA_P0_CASE = (3, 64, 264)  # p = 0 once


def lora_runs():
    return [(n, M, N, p) for n, M, N in LORA_CASES for p in LORA_P] + [LORA_P0_CASE + (0.0,)]


def case_inputs(c, device="cpu"):
    return G.gemm_inputs(c["inputs"], c["M"], c["N"], c["K"], c["al"], c["bl"], device, need=("addend", "old"))


def operand_mask_dims(c):
    """(tokens, features, the operand's key in the inputs, k_axis, i_axis) of a mode 1 / 2 case: mode 1 drops
    A [M = tokens, K = features], mode 2 B^T [K = tokens, N = features]"""
    if c["mode"] == 1:
        return c["M"], c["K"], "Amk", 1, 0
    return c["K"], c["N"], "Bnk", 0, 1


def staged_inputs(c, d, p, seed=DROP_SEED, mask_mutant=None, stage_mutant=None):
    """the inputs with the dropped operand replaced by its staged values (f32 holding bf16 values), as logical
    [M, K] / [N, K]"""
    T, F, key, k_axis, i_axis = operand_mask_dims(c)
    dev = d[key].device
    k0 = (c["kt_per"] or 0) * SLAB
    keep = mask(seed, T, F, p, dev, mask_mutant, k_axis=k_axis, k0=k0, i_axis=i_axis)
    x = d[key] if c["mode"] == 1 else d[key].T  # [tokens, features]
    xs = staged(x, keep, p, stage_mutant, k_axis=k_axis, K=c["K"])
    return dict(d, **{key: xs if c["mode"] == 1 else xs.T})


def d1_inputs(mode, F, al, device="cpu"):
    """ones [T, F] through the dropped operand against an identity. Mode 1 at (0,0): A = ones [T, F], B = I_F
    (N = K = F); mode 2 at (al,1): A = I_T (M = K = T), B = ones stored [K = T, N = F]. C [T, F] either way."""
    T = D1_T
    ones = torch.ones(T, F, dtype=BF)
    d = {}
    if mode == 1:
        c = dict(M=T, N=F, K=F, al=0, bl=0)
        d["A_buf"], d["A"] = G._nan_framed(ones, 0, device)
        d["B_buf"], d["B"] = G._nan_framed(torch.eye(F, dtype=BF), 0, device)
    else:
        c = dict(M=T, N=F, K=T, al=al, bl=1)
        d["A_buf"], d["A"] = G._nan_framed(torch.eye(T, dtype=BF), al, device)
        d["B_buf"], d["B"] = G._nan_framed(ones.T, 1, device)  # logical [N = F, K = T], stored [T, F]
    return c, d


def d1_expected(F, p, device="cpu"):
    keep = keep_mask(DROP_SEED, D1_T, F, p, device)
    sb = bf(scale_t(p, device))
    return torch.where(keep, sb, torch.zeros((), device=device)), keep
