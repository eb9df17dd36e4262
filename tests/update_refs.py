"""float64 references, gates and input sets for the kernels that turn gradients into new weights and
that move rows into and out of the model: fused AdamW, the gradient sum of squares, the clip
coefficient, the in-place scale and the bias-gradient column sums (csrc/elementwise.hip); the
embedding gather and scatter-add, the two-source row gather, the CLIP patch unfold and the fused
CLS / position / pre-LayerNorm kernel (csrc/embed.hip).
Plain torch on whatever device the tensors live on: tests/test_update_refs_host.py proves on the CPU
that every gate passes an honest f32 restatement of the kernel and fails a set of one-line mutants,
tests/test_update_accuracy_gpu.py then holds the kernels to the same gates on the same inputs (same
seeds, same shapes).

U, E, FLOOR and ust are those of tests/train_refs.py. Every gate is first order, per element, carries
the 2^-126 floor and is reported as the worst err / gate. The build passes no fast-math flag
(build.py: -O3 alone), so the f32 divide and sqrtf are correctly rounded: each counts one E.
No number here was taken from a kernel's output.
"""
import math

import torch

from tests.decode_refs import U, _gen, bf, worst
from tests.train_refs import BF, E, F32, FLOOR, _butterfly, case_id, ln_fwd_gate, ln_fwd_honest, ln_stats, ust

F64 = torch.float64


def f32(x):
    """one value as a float argument of the C ABI receives it"""
    return torch.tensor(float(x), dtype=F32)


def _rnd(t, dtype):
    """an f32 tensor after one store as `dtype`, back in f32"""
    return bf(t) if dtype == BF else t


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# fused AdamW (adamw_k, cullavo_adamw)
# ---------------------------------------------------------------------------------------------
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 0.01, 0.9, 0.999, 1e-8   # lr: the update is ~64 bf16 ulps of p ~ 0.02
ADAM_N_TRIPS = 18789    # 2348 vectors + a tail of 5: see adamw_plan
ADAM_DTYPES = [(BF, BF), (BF, F32), (F32, F32)]   # (parameter, state): the three instantiations

# (n, step, weight_decay, grad_scale, element offset of every buffer from a 16-B boundary)
ADAM_CASES = (
    # steps 1 (zero state, bc1 = 0.1) and 1000 (stored state, bc1 = 1.0f, bc2_sqrt = 0.795), with and
    # without decay, without a scale pointer, with the scale 1.0 and with a clipping 0.37
    [(ADAM_N_TRIPS, step, wd, gs, 0) for step in (1, 1000) for wd in (0.0, 0.1) for gs in (None, 1.0, 0.37)]
    + [(ADAM_N_TRIPS, 1000, 0.1, 0.37, 1),   # 2 B (4 B) off: the scalar loop serves every element
       (ADAM_N_TRIPS, 1000, 0.1, 0.37, 4),   # bf16: 8 B but not 16 B aligned, scalar; f32 buffers: 16 B, vector
       (5, 1000, 0.1, 0.37, 0),              # the tail alone (nvec = 0)
       (5, 1, 0.0, None, 1),                 # the tail alone, unaligned, zero state
       (8, 1000, 0.1, 0.37, 0),              # one vector, no tail
       (8, 1, 0.1, 1.0, 4),
       # lr wd = 0.05, several bf16 ulps: at wd = 0.1 the decayed bf16 parameter rounds back to p itself
       # (lr wd = 0.001 is under half an ulp), and where the decay is applied cannot show
       (ADAM_N_TRIPS, 1000, 5.0, 0.37, 0)]
)


def adamw_plan(n, vec):
    """(workgroups, trips of thread 0, threads with a last trip whose first half is live, of those
    the threads whose second half is live too, threads in all): the restated launch of cullavo_adamw
    and the two-steps-per-trip loop of adamw_k. Without vec the vector loop does not run (trips 0)."""
    nv = n // 8 if vec else n
    g = max(1, _cdiv(nv, 256 * 4))
    stride = g * 256
    nvec = n // 8 if vec else 0
    trips = _cdiv(nvec, 2 * stride)
    if trips == 0:
        return g, 0, 0, 0, stride
    last = (trips - 1) * 2 * stride
    first_live = max(0, min(stride, nvec - last))
    second_live = max(0, min(stride, nvec - last - stride))
    return g, trips, first_live, second_live, stride


def adamw_vec(offset, pdt, sdt):
    """whether cullavo_adamw takes the 8-wide path: all four buffers 16-B aligned"""
    return (offset * pdt.itemsize) % 16 == 0 and (offset * sdt.itemsize) % 16 == 0


class AdamConsts:
    """What cullavo_adamw and adamw_k derive from their float arguments, restated bit for bit (f32
    tensors; .d(name) gives the same value in f64): bc1 = 1.f - (float)pow(b1, step) and
    bc2_sqrt = (float)sqrt(1 - pow(b2, step)) from f64 pow as the host does, step_size = lr / bc1,
    decay = 1.f - lr * wd, c1 = 1.f - b1 and c2 = 1.f - b2 (exact: Sterbenz, both betas in [0.5, 1])."""

    def __init__(self, step, wd, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
        self.lr, self.wd, self.b1, self.b2, self.eps = f32(lr), f32(wd), f32(b1), f32(b2), f32(eps)
        self.bc1 = f32(1.0) - f32(math.pow(self.b1.item(), step))
        self.bc2s = f32(math.sqrt(1.0 - math.pow(self.b2.item(), step)))
        self.step_size = self.lr / self.bc1
        self.decay = f32(1.0) - self.lr * self.wd
        self.c1, self.c2 = f32(1.0) - self.b1, f32(1.0) - self.b2
        self.step = step

    def d(self, name):
        return getattr(self, name).double().item()


def adamw_state_ref(g, m, v, c, gs):
    """(g', m', v') in f64: g' = g gs (not rounded to the parameter type), m' = m + (g' - m)(1 - b1),
    v' = b2 v + (1 - b2) g'^2"""
    G = g.double() * (1.0 if gs is None else f32(gs).double().item())
    M, V = m.double(), v.double()
    return G, M + (G - M) * c.d("c1"), V * c.d("b2") + c.d("c2") * G * G


def adamw_inputs(n, pdt, sdt, step, wd, gs):
    """(p, g, m, v) on the CPU, p and g of pdt, m and v of sdt. g = 0.01 n; step 1: zero state; later
    steps: m = 0.005 n, v = 0.0001 (0.5 + u); p = 0.02 n. Planted:
      element 0: g = m = v = 0 (an embedding row that saw no token: the denominator is eps alone);
      element 1: g = 2^-33, m = 2^-32, v = 2^-80 (about 1e-10, 2e-10, 1e-24): sqrt(v') is far below eps;
      element 2: g = 0 with the live state;
      element 3 and every 16th from 19 on: p such that the decayed p is within a few percent of the update
        (taken from the f64 reference): there p' cancels to ~2^-5 of the update, U |p'| no longer hides
        an error of the update itself."""
    gen = _gen(f"adamw-{n}-{pdt}-{sdt}-{step}")
    g = 0.01 * torch.randn(n, generator=gen)
    m = 0.005 * torch.randn(n, generator=gen)
    v = 0.0001 * (0.5 + torch.rand(n, generator=gen))
    p = 0.02 * torch.randn(n, generator=gen)
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    g[0], m[0], v[0] = 0.0, 0.0, 0.0
    g[1] = 2.0 ** -33
    if step > 1:
        m[1], v[1] = 2.0 ** -32, 2.0 ** -80
    g[2] = 0.0
    g, m, v = g.to(pdt), m.to(sdt), v.to(sdt)
    c = AdamConsts(step, wd)
    _, M1, V1 = adamw_state_ref(g, m, v, c, gs)
    upd = c.d("step_size") * M1 / (V1.sqrt() / c.d("bc2s") + c.d("eps"))
    idx = torch.tensor([i for i in range(n) if i == 3 or (i >= 19 and i % 16 == 3)], dtype=torch.int64)
    if idx.numel():
        jit = 1.0 + 2.0 ** -5 * torch.randn(idx.numel(), generator=gen).double()
        p[idx] = (upd[idx] / c.d("decay") * jit).float()
    return p.to(pdt), g, m, v


def at_offset(t, offset, device=None):
    """a copy of t that starts `offset` elements past a 16-B boundary (allocations are at least 64-B aligned)"""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=device or t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + t.numel()]
    out.copy_(t)
    return out


def adamw_p_decayed(p0, c):
    """the kernel's first rounding point of p, bit for bit: round_T(f32(p) * decay), one IEEE f32 product
    with the f32 constant 1.f - lr * wd and one round-to-nearest-even to the parameter type"""
    return (p0.float() * c.decay.to(p0.device)).to(p0.dtype)


def adamw_gates(p1, m1, v1, p0, g, m0, v0, c, gs):
    """One step from (p0, g, m0, v0) to (p1, m1, v1). Returns (worst of m, worst of v, worst of p).
    m: ref = m + (g' - m) c1. In f32: g' rounds once, the difference once, its product with c1 once,
       the sum once, each within E (|g'| + |m|): gate Ust |ref| + 4 E (|g'| + |m|).
    v: ref = b2 v + c2 g'^2. v b2 rounds once; c2 g' g' is two products of a g' that itself rounded
       (its error doubled by the square): 4 E; the sum once more: gate Ust |ref| + 6 E (b2 v + c2 g'^2).
    p: the decayed parameter is restated bit for bit (adamw_p_decayed) and the moments the kernel stored
       (m1, v1, held by the two gates above) are what its update reads, so
       ref = p_dec - step_size m1 / (sqrt(v1) / bc2_sqrt + eps) in f64 over the restated f32 constants.
       sqrtf, the divide by bc2_sqrt and the add of eps leave the denominator within 3 E, the product
       step_size m1 and the quotient add two: the update is within 5 E, gated at 6 E |update|; the
       subtraction rounds the result once in f32 and the store once more: (Ust + E) |ref|.
       Nothing of the size of U |update| is allowed: where p_dec and the update cancel, the gate is
       far below one bf16 ulp of the update."""
    G, Mr, Vr = adamw_state_ref(g, m0, v0, c, gs)
    sdt, pdt = m1.dtype, p1.dtype
    wm = worst(m1.double() - Mr, ust(sdt) * Mr.abs() + 4 * E * (G.abs() + m0.double().abs()) + FLOOR)
    wv = worst(v1.double() - Vr, ust(sdt) * Vr.abs() + 6 * E * Vr.abs() + FLOOR)
    upd = c.d("step_size") * m1.double() / (v1.double().sqrt() / c.d("bc2s") + c.d("eps"))
    ref = adamw_p_decayed(p0, c).double() - upd
    wp = worst(p1.double() - ref, (ust(pdt) + E) * ref.abs() + 6 * E * upd.abs() + FLOOR)
    return wm, wv, wp


ADAM_MUTANTS = ("gs_ignored", "gs_not_in_square", "b1_for_c1", "no_bc1", "v_over_bc2", "eps_in_root",
                "decay_after", "unrounded_moments")


def adamw_honest(p, g, m, v, c, gs, mutant=None):
    """adamw_elem restated in torch f32, operation by operation (no fused multiply-add: the kernel
    turns contraction off). Returns (p1, m1, v1) in the stored types. `mutant` names one of ADAM_MUTANTS."""
    pdt, sdt = p.dtype, m.dtype
    s = f32(1.0) if (gs is None or mutant == "gs_ignored") else f32(gs)
    g0 = g.float()
    gv = g0 * s
    pv = p.float() if mutant == "decay_after" else _rnd(p.float() * c.decay, pdt)
    mf = m.float() + (gv - m.float()) * (c.b1 if mutant == "b1_for_c1" else c.c1)
    vf = v.float() * c.b2 + c.c2 * gv * (g0 if mutant == "gs_not_in_square" else gv)
    mv, vv = _rnd(mf, sdt), _rnd(vf, sdt)
    mu, vu = (mf, vf) if mutant == "unrounded_moments" else (mv, vv)
    if mutant == "v_over_bc2":
        denom = torch.sqrt(vu) / (c.bc2s * c.bc2s) + c.eps
    elif mutant == "eps_in_root":
        denom = torch.sqrt(vu / (c.bc2s * c.bc2s) + c.eps)
    else:
        denom = torch.sqrt(vu) / c.bc2s + c.eps
    ss = c.lr if mutant == "no_bc1" else c.step_size
    pv = pv - ss * mu / denom
    if mutant == "decay_after":
        pv = pv * c.decay
    return pv.to(pdt), mv.to(sdt), vv.to(sdt)


# ---------------------------------------------------------------------------------------------
# sum of squares (sumsq_k, sumsq_final_k)
# ---------------------------------------------------------------------------------------------
SUMSQ_PARTIALS = 1024                      # CULLAVO_SUMSQ_PARTIALS: the grid's cap
SUMSQ_PASS = SUMSQ_PARTIALS * 256 * 8      # elements one pass of the capped grid covers (1024 x 2048)
SUMSQ_N_BIG = 2 * SUMSQ_PASS + 8 * 300 + 3  # two full passes, 300 vectors of a third, a tail of 3
SUMSQ_OUT0 = 1.5                           # out[0] before the call
# (n, kind)
SUMSQ_CASES = [
    (5, "normal"),            # n < 8: nvec = 0, the tail loop alone
    (8, "normal"),            # one vector, no tail
    (2051, "normal"),         # 256 vectors (one workgroup, every thread one) and a tail of 3
    (2051, "spike"),          # one element 2^10 times the rest: the sum is that square
    (SUMSQ_N_BIG, "normal"),  # the grid capped at 1024: every thread strides on to a second vector, 300 to a third
]
SUMSQ_DTYPES = (BF, F32)


def sumsq_plan(n):
    """(workgroups, grid-stride passes = the most vectors one thread adds, tail elements) of cullavo_sumsq"""
    nvec = n // 8
    g = min(SUMSQ_PARTIALS, max(1, _cdiv(nvec, 256)))
    return g, _cdiv(nvec, g * 256), n - nvec * 8


def sumsq_inputs(n, dtype, kind):
    x = torch.randn(n, generator=_gen(f"sumsq-{n}-{dtype}-{kind}"))
    if kind == "spike":
        x[n // 2] = 2.0 ** 10 * x.abs().max()
    return x.to(dtype)


def sumsq_gate(out, x, out0=SUMSQ_OUT0):
    """ref = out0 + S, S = sum x^2 in f64. Every f32 add along the way is within E of a running sum of
    non-negative terms, so within E S: a lane's chain of 8 squares per vector it owns and one tail
    element (8 passes + 1 adds, and each square's own rounding, counted once more), the 6 butterfly
    levels, the 3 adds over the workgroup's waves; in sumsq_final_k a thread's chain over its
    cdiv(workgroups, 256) partials, 6 levels and 3 adds again. The += rounds out0 + S once: E |ref|."""
    g, passes, _ = sumsq_plan(x.numel())
    S = (x.double() ** 2).sum()
    ref = out0 + S
    count = (8 * passes + 1) + 1 + 6 + 3 + _cdiv(g, 256) + 6 + 3
    return worst(out.double().reshape(-1)[:1] - ref, (count * E * S + E * ref.abs() + FLOOR).reshape(1))


def _wg_sum(acc):
    """acc [..., 256] -> [...]: wave_sum per wave, then (red[0] + red[1]) + (red[2] + red[3])"""
    w = _butterfly(acc.reshape(*acc.shape[:-1], 4, 64))[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


SUMSQ_MUTANTS = ("no_tail", "no_second_pass", "assign")


def sumsq_honest(x, out0=SUMSQ_OUT0, mutant=None):
    """sumsq_k and sumsq_final_k restated in torch f32, in the kernels' order. Lanes without a vector
    add 0.0, which is exact. Returns the f32 out[0]."""
    n = x.numel()
    g, passes, tail = sumsq_plan(n)
    xf = x.float()
    nvec = n // 8
    T = g * 256
    pad = torch.zeros(max(passes, 1) * T, 8)
    pad[:nvec] = xf[:nvec * 8].view(nvec, 8)
    pad = pad.view(max(passes, 1), T, 8)
    acc = torch.zeros(T)
    for ps in range(passes):
        if mutant == "no_second_pass" and ps == 1:
            continue
        for j in range(8):
            acc = acc + pad[ps, :, j] * pad[ps, :, j]
    if tail and mutant != "no_tail":
        t = xf[nvec * 8:]
        acc[:tail] = acc[:tail] + t * t
    partials = _wg_sum(acc.view(g, 256))
    pp = torch.zeros(_cdiv(g, 256) * 256)
    pp[:g] = partials
    a2 = torch.zeros(256)
    for k in range(_cdiv(g, 256)):
        a2 = a2 + pp[k * 256:(k + 1) * 256]
    total = _wg_sum(a2)
    return total if mutant == "assign" else f32(out0) + total


# ---------------------------------------------------------------------------------------------
# clip coefficient (clip_coef_k) and in-place scale (scale_k)
# ---------------------------------------------------------------------------------------------
# (sumsq, max_norm)
CLIP_CASES = [
    (7.3, 1.0),              # the clipping branch
    (3.0e9, 0.5),            # a large norm: coef ~ 1e-5
    (0.25, 1.0),             # norm below max_norm: coef exactly 1.0
    (0.0, 1.0),              # no gradient at all: 1 / 1e-6 clamps to exactly 1.0
    (float("nan"), 1.0),     # a NaN gradient: see clip_coef_check
]
CLIP_TINY = 1e-6   # the kernel's own 1e-6f


def clip_coef_check(sumsq, max_norm, coef, norm):
    """sumsq is the f32 value given to the kernel. norm (None when norm_out was not given) within 2 E of
    sqrt(sumsq) (one correctly rounded sqrtf); coef within 4 E of min(1, max_norm / (norm + 1e-6)) (the
    root, the add and the divide: 3 roundings) and exactly 1.0 where that quotient is >= 1 + 8 E, sumsq = 0
    included. A NaN sumsq gives norm NaN and coef exactly 1.0: fminf returns its non-NaN argument. torch's
    clip_grad_norm_ would give a NaN coefficient there; the difference is harmless, the gradients that
    coef multiplies are NaN already. Returns the failures."""
    s = f32(sumsq).double().item()
    mn = f32(max_norm).double().item()
    fails = []
    if math.isnan(s):
        if norm is not None and not math.isnan(norm):
            fails.append(f"norm {norm!r} of a NaN sumsq")
        if coef != 1.0:
            fails.append(f"coef {coef!r} of a NaN sumsq")
        return fails
    nref = math.sqrt(s)
    q = mn / (nref + f32(CLIP_TINY).double().item())
    cref = min(1.0, q)
    if norm is not None and not abs(norm - nref) <= 2 * E * nref + FLOOR:
        fails.append(f"norm {norm!r} vs {nref!r}")
    if not abs(coef - cref) <= 4 * E * cref + FLOOR:
        fails.append(f"coef {coef!r} vs {cref!r}")
    if q >= 1.0 + 8 * E and coef != 1.0:
        fails.append(f"coef {coef!r} instead of exactly 1.0")
    return fails


def clip_coef_honest(sumsq, max_norm):
    """clip_coef_k restated in torch f32: (coef, norm) as Python floats"""
    norm = torch.sqrt(f32(sumsq))
    coef = torch.fmin(f32(1.0), f32(max_norm) / (norm + f32(CLIP_TINY)))
    return coef.item(), norm.item()


SCALE_CASES = [(n, dt, s) for n in (1, 257, 2051) for dt in (BF, F32) for s in (0.37, 1.0)]
# n = 1: one live thread; 257: a second workgroup with one element; 2051: nine workgroups, the last partial


def scale_inputs(n, dtype):
    return torch.randn(n, generator=_gen(f"scale-{n}-{dtype}")).to(dtype)


def scale_gate(y, x, s):
    """ref = x s with the f32 s. f32: one product, E |ref|. bf16: the f32 product and the store round in
    turn; the first moves the value by E |ref|, which can push the second past half a bf16 ulp only next to
    a rounding midpoint, and there |ref| exceeds its power of two by 2^-8 at least, so that U |ref| is
    half an ulp and 2^-16 of |ref| more: Ust |ref| holds for both. s = 1.0 must leave every bit alone
    (checked by the tests, not here)."""
    ref = x.double() * f32(s).double().item()
    return worst(y.double() - ref, ust(y.dtype) * ref.abs() + FLOOR)


def scale_honest(x, s, mutant=None):
    return (x.float() * (f32(s) * f32(s) if mutant == "twice" else f32(s))).to(x.dtype)


# ---------------------------------------------------------------------------------------------
# column sums (colsum_k, colsum_final_k)
# ---------------------------------------------------------------------------------------------
K_COLSUM_SPLIT = 32                    # kColsumSplit: grid.y
COLSUM_SLOTS = 8 * K_COLSUM_SPLIT      # row slots: 8 row lanes per workgroup x 32 workgroups down the rows
# (rows, cols, input type, output type, beta, kind)
COLSUM_CASES = [
    (1, 8, BF, F32, 0.0, "normal"),         # one row, one column group: 255 row slots and 31 of 32 lanes idle
    (255, 264, BF, F32, 0.0, "normal"),     # fewer rows than row slots (slot 255 stays empty); the second
    (255, 264, BF, F32, 0.0, "cancel"),     # column workgroup holds 8 columns
    (255, 264, F32, F32, 1.0, "normal"),    # f32 input
    (1000, 520, BF, F32, 1.0, "cancel"),    # f32 output accumulated onto its old value (functions.py)
    (1000, 520, BF, BF, 0.0, "normal"),     # bf16 output; 4 rows per slot (3 for slots 232 on)
    (1000, 520, BF, BF, 1.0, "cancel"),     # bf16 output accumulated
]


def colsum_rows_per_lane(rows):
    """the longest chain of the loop r = rl + 8 blockIdx.y; r < rows; r += 8 gridDim.y"""
    return _cdiv(rows, COLSUM_SLOTS)


def colsum_inputs(rows, cols, dtype, kind):
    """(x [rows, cols], old [cols] f32 values). "cancel": rows 2k and 2k + 1 are n and -n + 2^-8 n', so a
    column sums to ~2^-8 sqrt(rows / 2) while sum |x| is ~0.8 rows: the gate is far below the
    max-magnitude tolerance of the older test."""
    g = _gen(f"colsum-{rows}-{cols}-{dtype}-{kind}")
    x = torch.randn(rows, cols, generator=g)
    if kind == "cancel":
        x[1::2] = -x[0:2 * (rows // 2):2] + 2.0 ** -8 * torch.randn(rows // 2, cols, generator=g)
    old = torch.randn(cols, generator=g)
    return x.to(dtype), old


def colsum_gate(out, x, old, beta):
    """ref = sum_rows x (+ beta old). A lane adds its rows_per_lane rows, the workgroup its 8 row lanes
    (8 adds from zero), colsum_final_k the 32 partials (32 adds from zero), then the product with beta
    and its add: each within E of the running sum of magnitudes, (rows_per_lane + 8 + 32 + 2) E sum |x|;
    the product beta old itself E |beta old|; the store Ust |ref|."""
    X = x.double()
    ref, gate = X.sum(0), (colsum_rows_per_lane(X.shape[0]) + 8 + 32 + 2) * E * X.abs().sum(0)
    if beta != 0.0:
        bo = beta * old.to(out.dtype).double()
        ref, gate = ref + bo, gate + E * bo.abs()
    return worst(out.double() - ref, gate + ust(out.dtype) * ref.abs() + FLOOR)


COLSUM_MUTANTS = ("no_last_slot", "no_beta", "no_p31")


def colsum_honest(x, old, beta, out_dtype, mutant=None):
    """colsum_k and colsum_final_k restated in torch f32, in the kernels' order"""
    xf = x.float()
    rows, cols = xf.shape
    acc = torch.zeros(COLSUM_SLOTS, cols)   # slot of row r: r % 256 = 8 blockIdx.y + row lane
    for r in range(rows):
        acc[r % COLSUM_SLOTS] = acc[r % COLSUM_SLOTS] + xf[r]
    acc = acc.view(K_COLSUM_SPLIT, 8, cols)
    s = torch.zeros(cols)
    for p in range(K_COLSUM_SPLIT):
        if mutant == "no_p31" and p == 31:
            continue
        part = torch.zeros(cols)
        for k in range(8):
            if not (mutant == "no_last_slot" and k == 7):
                part = part + acc[p, k]
        s = s + part
    if beta != 0.0 and mutant != "no_beta":
        s = s + f32(beta) * old.to(out_dtype).float()
    return s.to(out_dtype)


# ---------------------------------------------------------------------------------------------
# embedding backward (embedding_bwd_k)
# ---------------------------------------------------------------------------------------------
EMB_VOCAB = 50
EMB_LONE = EMB_VOCAB - 1    # the id whose only occurrence is position n - 1
EMB_MANY = 7                # the id with the most occurrences
# (dim, n, table type, dout type, beta)
EMB_BWD_CASES = [
    (8, 1, F32, BF, 0.0),        # one position, one live thread
    (8, 300, F32, BF, 1.0),      # two windows of positions at the narrowest row
    (256, 300, F32, BF, 1.0),    # the training step's pair and beta
    (256, 700, BF, BF, 0.0),     # three windows
    (2056, 300, F32, BF, 1.0),   # register chunk c = 1 served by thread 0 alone; the four type pairs:
    (2056, 300, BF, BF, 1.0),
    (2056, 300, F32, F32, 0.0),
    (2056, 300, BF, F32, 0.0),
    (2056, 700, F32, BF, 0.0),   # three windows and two chunks
    (8192, 1, BF, BF, 0.0),      # the widest row from one position
    (8192, 700, F32, BF, 1.0),   # all four chunks full, three windows (dout is 11 MB)
]


def emb_chunks(dim):
    """register chunks of 256 threads x 8 columns in use (kMaxC = 4)"""
    return _cdiv(dim // 8, 256)


def emb_ids(n):
    """ids [n] int64, drawn from 1 .. 39: id 0 and ids 40 .. 48 never occur, their rows stay untouched.
    For n >= 300: EMB_MANY stands at every odd position from 3 on when n = 700 (349 occurrences over three
    windows of 256 positions from the first) and at every third position when n = 300 (two windows);
    position 1 holds -100 and position 2 holds vocab, both skipped (a clamp would send -100 to row 0, which
    nothing else writes). Position n - 1 holds EMB_LONE, its only occurrence: a first occurrence in the last
    window."""
    g = _gen(f"emb-ids-{n}")
    ids = torch.randint(1, 40, (n,), generator=g)
    if n >= 300:
        ids[ids == EMB_MANY] = 8
        if n >= 700:
            ids[3::2] = EMB_MANY
        else:
            ids[3::3] = EMB_MANY
        ids[1], ids[2] = -100, EMB_VOCAB
    ids[n - 1] = EMB_LONE
    return ids


def emb_bwd_inputs(dim, n, tt, td):
    """(ids [n], dout [n, dim] of td, old table [vocab, dim] of tt: the sentinel of the untouched rows)"""
    g = _gen(f"emb-bwd-{dim}-{n}-{tt}-{td}")
    return emb_ids(n), torch.randn(n, dim, generator=g).to(td), torch.randn(EMB_VOCAB, dim, generator=g).to(tt)


def emb_bwd_gate(dtable, ids, dout, old, beta):
    """The contract: the kernel writes only the rows that are hit. Row id of dtable, for every id in range
    that occurs k >= 1 times: ref = sum of its dout rows (+ beta old), f64. The k adds from zero and the
    product and add of beta old are each within E of the running sum of magnitudes: (k + 2) E sum |dout
    rows of id|, plus E |beta old| for that product and Ust |ref| for the store. Every other row (ids that
    do not occur, rows only an id out of range would reach by a clamp) keeps the bits of `old`, at any
    beta. Returns (worst over the hit rows, untouched rows bitwise equal)."""
    vocab, dim = old.shape
    ok = (ids >= 0) & (ids < vocab)
    idx = ids[ok]
    D = dout.double()[ok]
    ref = torch.zeros(vocab, dim, dtype=F64, device=old.device).index_add_(0, idx, D)
    mag = torch.zeros(vocab, dim, dtype=F64, device=old.device).index_add_(0, idx, D.abs())
    k = torch.bincount(idx, minlength=vocab).double()[:, None]
    bo = beta * old.double()
    ref = ref + bo
    gate = (k + 2) * E * mag + E * bo.abs() + ust(dtable.dtype) * ref.abs() + FLOOR
    hit = k[:, 0] > 0
    same = bool(torch.equal(dtable[~hit], old[~hit]))
    return worst(dtable.double()[hit] - ref[hit], gate[hit]), same


EMB_MUTANTS = ("first_window_only", "chunk0_only", "clamp_ids", "beta_everywhere")


def emb_bwd_honest(ids, dout, old, beta, mutant=None):
    """embedding_bwd_k restated in torch f32: per id, its dout rows added in increasing position order"""
    vocab, dim = old.shape
    out = old.clone()
    use = ids.clamp(0, vocab - 1) if mutant == "clamp_ids" else ids
    df = dout.float()
    if mutant == "beta_everywhere":
        out = (f32(beta) * old.float()).to(old.dtype)
    for i in sorted(set(use.tolist())):
        if i < 0 or i >= vocab:
            continue
        pos = (use == i).nonzero()[:, 0].tolist()
        if mutant == "first_window_only":
            pos = [q for q in pos if q < pos[0] + 256]
        acc = torch.zeros(dim)
        for q in pos:
            acc = acc + df[q]
        if beta != 0.0:
            acc = acc + f32(beta) * old[i].float()
        cols = min(dim, 2048) if mutant == "chunk0_only" else dim
        out[i, :cols] = acc[:cols].to(old.dtype)
    return out


# ---------------------------------------------------------------------------------------------
# embedding forward and the two-source row gather (embedding_fwd_k, row_gather2_k): exact copies
# ---------------------------------------------------------------------------------------------
GATHER_CASES = [(dim, dt) for dim in (8, 2056) for dt in (BF, F32)]
# dim 8: one 16-B unit per bf16 row, two per f32 row (rows move as twice as many 16-bit units);
# 2056: 257 units, thread 0 takes a second one (f32: 514, threads 0 and 1 a third)
GATHER_SENTINEL = -7.0


def gather_inputs(dim, dtype):
    """(table a [50, dim], second source b [6, dim], ids [12] with -1, -100 and vocab among them,
    src [12] for row_gather2: rows of a, rows of b (index 50 + j) and -1 / -5 for zero rows)"""
    g = _gen(f"gather-{dim}-{dtype}")
    a = torch.randn(EMB_VOCAB, dim, generator=g).to(dtype)
    b = torch.randn(6, dim, generator=g).to(dtype)
    ids = torch.tensor([0, 49, -1, 17, EMB_VOCAB, 17, -100, 3, 48, EMB_VOCAB + 7, 1, 0])
    src = torch.tensor([0, 50, -1, 49, 55, 17, -5, 52, 3, 50, -1, 49])
    return a, b, ids, src


def embedding_fwd_ref(ids, table):
    """table[ids], an all-zero row for an id out of range"""
    ok = (ids >= 0) & (ids < table.shape[0])
    out = table[ids.clamp(0, table.shape[0] - 1)].clone()
    out[~ok] = 0
    return out


def row_gather2_ref(src, a, b):
    """row r = a[src] for 0 <= src < n_a, b[src - n_a] from there on (b None: a serves as both), zeros for src < 0"""
    both = torch.cat([a, a if b is None else b], 0)
    out = both[src.clamp_min(0)].clone()
    out[src < 0] = 0
    return out


# ---------------------------------------------------------------------------------------------
# CLIP front end: patch unfold (im2col_k) and CLS / position / pre-LayerNorm (vision_embed_ln_k)
# ---------------------------------------------------------------------------------------------
VIS_EPS = 1e-5
# (B, T, dim, dtype): B T rows, four to a workgroup
VIS_CASES = [
    (3, 5, 8, BF),       # 15 rows (the last workgroup holds 3), one lane live, NCH 1
    (3, 5, 520, BF),     # a row that ends 8 columns into its second chunk, NCH 2
    (2, 3, 1024, BF),    # 6 rows; the padded width is the width, NCH 2
    (1, 5, 2056, BF),    # 5 rows; NCH 8 with five chunks live
    (1, 3, 4104, BF),    # 3 rows, one workgroup not full; NCH 16 with nine chunks live
    (3, 5, 520, F32),    # the f32 instantiation
]
VIS_X_CLS = 1e4   # in the rows t == 0 of x, which the kernel must not read into the result


def vis_nch(dim):
    """chunks of 512 columns vision_embed_ln_k is unrolled to (cullavo_vision_embed_ln)"""
    for lim, n in ((512, 1), (1024, 2), (2048, 4), (4096, 8)):
        if dim <= lim:
            return n
    return 16


def vis_inputs(B, T, dim, dtype):
    """x [B T, dim] = n + 2 (rows t == 0: VIS_X_CLS), cls [dim] = n + 2, pos [T, dim] = 0.5 n, w, b [dim].
    The mean of 2 stands well above the deviations: a rounding of x + pos left out moves the
    normalised value by several times U of it."""
    g = _gen(f"vis-{B}-{T}-{dim}-{dtype}")
    x = torch.randn(B * T, dim, generator=g) + 2.0
    x[::T] = VIS_X_CLS
    cls = torch.randn(dim, generator=g) + 2.0
    pos = 0.5 * torch.randn(T, dim, generator=g)
    w = 1.0 + 0.1 * torch.randn(dim, generator=g)
    b = 0.1 * torch.randn(dim, generator=g)
    return tuple(t.to(dtype) for t in (x, cls, pos, w, b))


def vis_v(x, cls, pos, T):
    """the kernel's rounding point, bit for bit: v = round(f32(x) + f32(pos[row % T])), rows t == 0
    round(f32(cls) + f32(pos[0])): one IEEE f32 add and one round-to-nearest-even to the stored type"""
    rows = x.shape[0]
    v = x.float() + pos.float().repeat(rows // T, 1)
    v[::T] = cls.float() + pos[0].float()
    return v.to(x.dtype)


def vis_gate(y, x, cls, pos, w, b, T, eps=VIS_EPS):
    """y against the f64 LayerNorm of the restated v: the y part of train_refs.ln_fwd_gate (the kernel's
    arithmetic after v is layernorm_fwd_k's)"""
    v = vis_v(x, cls, pos, T)
    mean, rstd = ln_stats(v, eps)
    return ln_fwd_gate(y, mean, rstd, v, w, b, eps)[2]


VIS_MUTANTS = ("cls_takes_x", "pos_by_row", "padded_div", "v_not_rounded")


def vis_honest(x, cls, pos, w, b, T, eps=VIS_EPS, mutant=None):
    """vision_embed_ln_k restated in torch f32 (sums in lane order by train_refs.ln_fwd_honest).
    pos_by_row reads pos[row]; past the table (undefined in a kernel) it is restated as the last row."""
    rows, dim = x.shape
    xf = x.float()
    pf = pos.float()[torch.arange(rows).clamp_max(T - 1)] if mutant == "pos_by_row" else pos.float().repeat(rows // T, 1)
    v = xf + pf
    if mutant != "cls_takes_x":
        v[::T] = cls.float() + pf[::T]
    if mutant != "v_not_rounded":
        v = _rnd(v, x.dtype)
    if mutant == "padded_div":
        pad = torch.zeros(rows, 512 * vis_nch(dim))   # dividing by the padded width = zero columns in the mean
        pad[:, :dim] = v
        cols = torch.tensor(float(pad.shape[1]))
        mean = (pad.sum(1) / cols)[:, None]
        d = v - mean
        r = torch.rsqrt((d * d).sum(1) / cols + torch.tensor(eps))[:, None]
        return (d * r * w.float() + b.float()).to(x.dtype)
    return ln_fwd_honest(v, w, b, eps)[0].to(x.dtype)


IM2COL_SHAPE = dict(B=2, C=3, H=8, W=12, patch=4, kpad=56)   # gw = 3, gh = 2: H != W; kreal = 48 < kpad
IM2COL_DTYPES = [(pd, od) for pd in (F32, BF) for od in (BF, F32)]   # (pixels, output)
IM2COL_SENTINEL = -7.0


def im2col_inputs(pdt):
    s = IM2COL_SHAPE
    return torch.randn(s["B"], s["C"], s["H"], s["W"], generator=_gen(f"im2col-{pdt}")).to(pdt)


def im2col_index(B, C, H, W, patch, kpad, mutant=None):
    """(flat pixel index [B (1 + P), kpad], live mask) in the CLIP convolution's unfold order: row
    b (1 + P) + 1 + py gw + px (row b (1 + P) is the CLS slot), column (ch patch + i) patch + j reads pixel
    [b, ch, py patch + i, px patch + j]. Mutants: "py_by_gh" (py = p / gh) and "swap_ch" (channel and
    in-patch index swapped: ch = c % C, i j from c / C); an index past the image wraps (a kernel would
    read whatever lies there)."""
    gh, gw = H // patch, W // patch
    P = gh * gw
    r = torch.arange(B * (1 + P))[:, None]
    c = torch.arange(kpad)[None, :]
    b, t = r // (1 + P), r % (1 + P)
    p = (t - 1).clamp_min(0)
    py, px = p // (gh if mutant == "py_by_gh" else gw), p % gw
    if mutant == "swap_ch":
        ch, rem = c % C, c // C
    else:
        ch, rem = c // (patch * patch), c % (patch * patch)
    i, j = rem // patch, rem % patch
    idx = ((b * C + ch) * H + py * patch + i) * W + px * patch + j
    live = (t > 0) & (c < C * patch * patch)
    return (idx % (B * C * H * W)).expand(B * (1 + P), kpad), live.expand(B * (1 + P), kpad)


def im2col_ref(pix, patch, kpad, odt, mutant=None):
    """exact: the pixels converted once to the output type, gathered; CLS rows and columns kreal .. kpad-1 zero"""
    B, C, H, W = pix.shape
    idx, live = im2col_index(B, C, H, W, patch, kpad, mutant)
    idx, live = idx.to(pix.device), live.to(pix.device)
    out = pix.to(odt).reshape(-1)[idx]
    return torch.where(live, out, torch.zeros((), dtype=odt, device=pix.device))
