"""float64 references, gates and input sets for the training step's norm, loss and SwiGLU / activation
kernels (csrc/norms.hip, csrc/loss.hip, the SwiGLU and act_bwd kernels of csrc/elementwise.hip).
Plain torch on whatever device the tensors live on: tests/test_train_refs_host.py proves on the CPU
that every gate passes an honest f32 restatement of the kernel and fails a set of one-line mutants,
tests/test_train_accuracy_gpu.py then holds the kernels to the same gates on the same inputs (same
seeds, same shapes).

U = 2^-8 is the largest relative error of one bf16 round-to-nearest, E = 2^-24 the same for f32;
ust(dtype) is the one of the stored type. Every gate is first order, per element, carries a floor
of 2^-126 (an output may flush to zero) and is reported as the worst err / gate. The statistics a
backward kernel takes as input (rstd, mean, row_lse, loss_out) are computed here in f64, rounded
once to f32 and given to the kernel and to the f64 reference alike. No number here was taken from
a kernel's output.
"""
import math

import torch

from tests.decode_refs import U, _gen, bf, worst

BF = torch.bfloat16
F32 = torch.float32
E = 2.0 ** -24
FLOOR = 2.0 ** -126
EPS = 1e-5
IGNORE = -100


def ust(dtype):
    return U if dtype == BF else E


# ---------------------------------------------------------------------------------------------
# the kernels' launch geometry (csrc/norms.hip), restated
# ---------------------------------------------------------------------------------------------
K_ROWS_PER_BLOCK = 4    # kRowsPerBlock: one wave per row in the forward and one-wave backward kernels
K_BWD_BLOCKS = 256      # kBwdBlocks
K_BWD8_BLOCKS = 512     # kBwd8Blocks: rmsnorm_bwd8_k, 2 waves per row, 4 rows per iteration
K_BWD8P_BLOCKS = 256    # kBwd8pBlocks: rmsnorm_bwd8p_k, kWpr = 4 waves per row, kSlots = 2 rows per iteration
K_WPR = 4
K_SLOTS = 8 // K_WPR


def nch_for(cols):
    """512-column chunks a row is unrolled to (norms.hip nch_for)"""
    for lim, n in ((512, 1), (1024, 2), (2048, 4), (4096, 8), (6144, 12)):
        if cols <= lim:
            return n
    return 16


def rms_fwd_prew(rows, cols, dtype):
    """whether rmsnorm_fwd runs the PREW instantiation"""
    return dtype == BF and rows <= 64 and nch_for(cols) <= 8


def rms_bwd_plan(rows, cols, mode, want_dw):
    """(kernel, waves per row, workgroups, rows per workgroup, rows per iteration) of rmsnorm_bwd_impl.
    rmsnorm_bwd_k walks rows with a stride, its 'rows per workgroup' is given as all rows."""
    nch = nch_for(cols)
    wide = nch > 8 and mode == 0
    pipe = (not wide) and mode == 1 and (want_dw or nch > 8)
    if wide:
        return "rmsnorm_bwd_k", 1, min(K_BWD_BLOCKS, -(-rows // K_ROWS_PER_BLOCK)), rows, 1
    nb = min(K_BWD8P_BLOCKS if pipe else K_BWD8_BLOCKS, -(-rows // 4))
    rpb = -(-rows // nb)
    return ("rmsnorm_bwd8p_k", K_WPR, nb, rpb, K_SLOTS) if pipe else ("rmsnorm_bwd8_k", 2, nb, rpb, 4)


# ---------------------------------------------------------------------------------------------
# cases: every purpose stands next to its case
# ---------------------------------------------------------------------------------------------
# (rows, cols, dtype). Column counts: 8 (one lane), 520 (ends inside chunk 2), 2056 (ends inside chunk 5 of
# NCH 8), 4096, 5120 (NCH 12) and 8192 (NCH 16).
RMS_FWD_CASES = [
    (1, 8, BF),       # one row, one lane live (PREW)
    (5, 520, BF),     # a partial workgroup, a row that ends 8 columns into its second chunk (PREW)
    (1, 4096, BF),    # the decode step's launch: one row, PREW at its widest (NCH 8)
    (65, 2056, BF),   # 65 rows at NCH 8: the first row count on the non-PREW path at a width PREW serves
    (3, 5120, BF),    # a few rows without PREW (NCH 12 has no PREW form)
    (5, 8192, BF),    # the widest row
    (5, 520, F32),    # the f32 instantiation
]

# (rows, cols): each runs with and without dw and dres, in backward mode 1
RMS_BWD_CASES = [
    (1, 8),        # a single row: one workgroup, the second row slot idle
    (7, 8192),     # NCH 16: four chunks per wave part; workgroups of 4 and 3 rows
    (9, 5120),     # NCH 12: three chunks per wave part (pipelined also without dw); 3 rows per workgroup
    (37, 4096),    # NCH 8; ten workgroups, the last with one row
    (300, 2056),   # a row that ends 8 columns into chunk 5: wave part 0 owns a short second chunk
    (2100, 520),   # with dw: 9 rows per workgroup = 5 iterations (odd: the double-buffered loop leaves in
                   # its middle, the last iteration has one row), workgroup 233 has 3 rows, 234..255 none
]
# (rows, cols, want_dw) in backward mode 0
RMS_BWD_MODE0_CASES = [
    (9, 5120, True), (7, 8192, True),   # rmsnorm_bwd_k (NCH 16, one wave per row)
    (37, 4096, True),                   # rmsnorm_bwd8_k with dw
]
RMS_BWD_F32_CASE = (37, 2056)           # the f32 instantiation (x, dy, w, dres, dx f32; dw f32)
RMS_BWD_BETA_CASE = (300, 2056)         # bf16 dw with beta = 1

# (rows, cols): with and without dres
LN_CASES = [(3, 64), (577, 128), (64, 1024), (5, 520)]
LN_F32_CASE = (5, 520)
NORM_KINDS = ("normal", "corr")

# (rows, V, dtype, kind)
CE_CASES = [
    (70, 5, BF, "normal"),          # V < 8: the column tail alone
    (70, 1000, BF, "normal"),       # no tail, one pass of the 2048-column loop
    (70, 1003, BF, "normal"),       # tail of 3, ldl 1008
    (70, 1003, BF, "planted_last"),  # the row's largest logit in the tail's last column
    (70, 2056, BF, "ascending"),    # two loop passes, every step raises the running maximum
    (70, 4099, BF, "normal"),       # two full passes and a tail, ldl 4104
    (70, 4099, BF, "planted_last"),
    (1030, 1003, BF, "normal"),     # more rows than ce_reduce has threads: its stride loop
    (70, 1003, F32, "ascending"),   # the f32 instantiation
]
CE_GRAD_LOSS = (None, 0.5, 1.0 / 3.0)

SWIGLU_CASES = [(3, 8, BF), (70, 688, BF), (70, 688, F32)]   # (rows, F, dtype)
ACT_CASES = [(8, BF), (33 * 264, BF), (33 * 264, F32)]       # (n, dtype)
ACTS = ("gelu", "quick_gelu")


def case_id(c):
    return "-".join({BF: "bf16", F32: "f32"}.get(v, str(v)) for v in c)


# ---------------------------------------------------------------------------------------------
# lane-order sums (one wave per row or several: wave part p owns the 512-column chunks p, p + parts, ...)
# ---------------------------------------------------------------------------------------------
_LANE = torch.arange(64)


def _butterfly(v):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1, on [..., 64]"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    return v


def wave_part_sums(t, parts=1):
    """f32 row sums of t [rows, cols] as the norm kernels form them: a lane adds its 8 columns of
    each of its wave part's chunks in turn, the 64 lanes combine in a butterfly. Returns one [rows]
    partial per wave part."""
    rows, cols = t.shape
    nch = -(-cols // 512)
    pad = torch.zeros(rows, nch * 512)
    pad[:, :cols] = t
    ch = pad.view(rows, nch, 64, 8)
    out = []
    for p in range(parts):
        seq = ch[:, p::parts].permute(0, 2, 1, 3).reshape(rows, 64, -1)
        acc = torch.zeros(rows, 64)
        for k in range(seq.shape[2]):
            acc = acc + seq[:, :, k]
        out.append(_butterfly(acc)[:, 0])
    return out


def _drop_last_chunk(t):
    """t with the columns of the last live 512-column chunk zeroed (adding 0.0 is exact)"""
    t = t.clone()
    t[:, (t.shape[1] - 1) // 512 * 512:] = 0
    return t


# ---------------------------------------------------------------------------------------------
# norm inputs
# ---------------------------------------------------------------------------------------------
def norm_inputs(rows, cols, dtype=BF, kind="normal", name="rms"):
    """x, dy, dres [rows, cols], w, b [cols], dw_old [cols] of `dtype` (CPU). kind "corr":
    dy = round(0.5 x + 0.5 n), so the projection terms of the backward are as large as g itself.
    With two rows or more, row rows // 2 of x is scaled by 2^-10 (exactly), where eps matters.
    LayerNorm's x is 2 n + 0.25."""
    g = _gen(f"{name}-{rows}-{cols}-{dtype}-{kind}")
    x = torch.randn(rows, cols, generator=g)
    if name == "ln":
        x = 2.0 * x + 0.25
    x = x.to(dtype)
    if rows >= 2:
        x[rows // 2] = (x[rows // 2].float() * 2.0 ** -10).to(dtype)
    n = torch.randn(rows, cols, generator=g)
    dy = (0.5 * x.float() + 0.5 * n).to(dtype) if kind == "corr" else n.to(dtype)
    w = (1.0 + 0.1 * torch.randn(cols, generator=g)).to(dtype)
    b = (0.1 * torch.randn(cols, generator=g)).to(dtype)
    dres = torch.randn(rows, cols, generator=g).to(dtype)
    dw_old = torch.randn(cols, generator=g).to(dtype)
    return dict(x=x, dy=dy, w=w, b=b, dres=dres, dw_old=dw_old)


def rms_stats(x, eps=EPS):
    """rstd in f64, rounded once to f32"""
    return ((x.double() ** 2).mean(1) + eps).rsqrt().float()


def ln_stats(x, eps=EPS):
    """(mean, rstd) in f64, each rounded once to f32"""
    X = x.double()
    mean = X.mean(1)
    var = ((X - mean[:, None]) ** 2).mean(1)
    return mean.float(), (var + eps).rsqrt().float()


# ---------------------------------------------------------------------------------------------
# RMSNorm forward (rmsnorm_fwd_k, with and without PREW: the same arithmetic)
# ---------------------------------------------------------------------------------------------
def rms_fwd_gate(y, rstd, x, w, eps=EPS):
    """rstd: |rstd - ref| <= (cols + 8) E ref: an f32 sum of cols non-negative terms in any order
    (cols E with the products' own roundings), one divide, one add, one rsqrtf.
    y = round(w * round(x r)), w * q exact in f32 for bf16: two roundings of the value, 2 U (1 + U),
    and the relative error of r and of the product x r, within 2 (cols + 8) E; all times |w x r_ref|.
    For f32 the two roundings are the two f32 products: 4 E.
    Returns (worst of rstd, worst of y)."""
    X = x.double()
    cols = X.shape[1]
    r = ((X ** 2).mean(1) + eps).rsqrt()
    ref = w.double() * X * r[:, None]
    two = 2 * U * (1 + U) if y.dtype == BF else 4 * E
    return (worst(rstd.double() - r, (cols + 8) * E * r + FLOOR),
            worst(y.double() - ref, (two + 2 * (cols + 8) * E) * ref.abs() + FLOOR))


def rms_fwd_honest(x, w, eps=EPS, drop_last_chunk=False, padded_div=False, no_eps=False, w_off8=False):
    """rmsnorm_fwd_k restated in torch f32. The keyword arguments are the mutants."""
    xf, wf = x.float(), w.float()
    cols = xf.shape[1]
    sq = xf * xf
    ss = wave_part_sums(_drop_last_chunk(sq) if drop_last_chunk else sq)[0]
    div = torch.tensor(float(512 * nch_for(cols) if padded_div else cols))
    ms = ss / div
    r = torch.rsqrt(ms if no_eps else ms + torch.tensor(eps))
    if w_off8:
        wf = wf.roll(-8)
    q = xf * r[:, None]
    q = bf(q) if x.dtype == BF else q
    return (wf * q).to(x.dtype), r


# ---------------------------------------------------------------------------------------------
# RMSNorm backward (rmsnorm_bwd8p_k, rmsnorm_bwd8_k, rmsnorm_bwd_k; reduce_partials_k)
# ---------------------------------------------------------------------------------------------
def rms_dx_gate(dx, dy, x, w, rstd, dres=None):
    """ref = r (g - x r dot) + dres with g = dy w, dot = mean_c g x r, r the f32 rstd given.
    |dx - ref| <= Ust |ref| + E [6 (|r g| + |x r^2 dot| + |dres|) + (cols + 4) |x| r^2 A], A = mean_c |g x r|.
    The store rounds the value once (Ust |ref|). Before it, in f32: g (one product), the
    subtraction, the product with r and the residual add round r g at most 4 times; x r, its product
    with dot, the subtraction, the product with r and the add round x r^2 dot at most 5 times; dres is
    rounded by its add alone: 6 E covers each. dot is a sum of cols products of three rounded factors,
    in any order of lanes, wave parts and chunks, divided once: (cols - 1 + 3 + 1) E A at most, carried
    to dx by |x| r^2: the last term, at cols + 4."""
    X, W, r = x.double(), w.double(), rstd.double()[:, None]
    cols = X.shape[1]
    g = dy.double() * W
    gxr = g * X * r
    A, dot = gxr.abs().mean(1, keepdim=True), gxr.mean(1, keepdim=True)
    D = dres.double() if dres is not None else torch.zeros((), dtype=torch.float64, device=X.device)
    ref = r * (g - X * r * dot) + D
    gate = ust(dx.dtype) * ref.abs() + E * (6 * ((r * g).abs() + (X * r * r * dot).abs() + D.abs())
                                             + (cols + 4) * X.abs() * r * r * A) + FLOOR
    return worst(dx.double() - ref, gate)


def rms_q(x, rstd):
    """the kernel's one rounding point of dw, bit for bit: q = round(f32(x) * f32(rstd)), one IEEE f32
    product and (for bf16) one round-to-nearest-even"""
    q = x.float() * rstd.float()[:, None]
    return bf(q) if x.dtype == BF else q


def rms_dw_gate(dw, dy, x, rstd, dw_old=None, beta=0.0):
    """ref = sum_rows dy q (+ beta dw_old) in f64 over the restated q: the products dy q round once
    and their f32 sum over rows (row slots, workgroup partials, 16 reduce groups: any order, and the
    empty slots add exact zeros) is within (rows - 1) E of sum |dy q|: gated at (rows + 16) E sum |dy q|,
    plus E |beta dw_old| for that product and U |ref| when dw is stored as bf16."""
    q = rms_q(x, rstd).double()
    prod = dy.double() * q
    rows = prod.shape[0]
    ref, gate = prod.sum(0), (rows + 16) * E * prod.abs().sum(0) + FLOOR
    if beta != 0.0:
        ref = ref + beta * dw_old.double()
        gate = gate + E * (beta * dw_old.double()).abs()
    if dw.dtype == BF:
        gate = gate + U * ref.abs()
    return worst(dw.double() - ref, gate)


def rms_bwd_honest(dy, x, w, rstd, dres=None, parts=K_WPR, rpb=None, slots=K_SLOTS, want_dw=False, dw_dtype=F32,
                   dw_old=None, beta=0.0, miss_part3=False, miss_last_chunk=False, padded_div=False,
                   drop_dres=False, dres_twice=False, rstd_next_row=False, dw_miss_last_row=False):
    """The RMSNorm backward kernels restated in torch f32: `parts` waves per row (4: rmsnorm_bwd8p_k,
    2: rmsnorm_bwd8_k, 1: rmsnorm_bwd_k), their partial dot products added in order; dw summed per
    workgroup of rpb rows (per row slot, slots folded in order), the workgroups' partial rows in
    reduce_partials_k's 16 groups. Returns (dx, dw or None). The keyword arguments from miss_part3 on
    are the mutants."""
    T = x.dtype
    xf, df, wf, r = x.float(), dy.float(), w.float(), rstd.float()[:, None]
    rows, cols = xf.shape
    if rstd_next_row:
        r = r.roll(-1, 0)
    xh = xf * r
    g = df * wf
    t = g * xh
    if miss_last_chunk:
        t = _drop_last_chunk(t)
    ps = wave_part_sums(t, parts)
    dot = torch.zeros(rows)
    for p, s in enumerate(ps):
        if not (miss_part3 and p == 3):
            dot = dot + s
    dot = (dot / torch.tensor(float(512 * nch_for(cols) if padded_div else cols)))[:, None]
    o = r * (g - xh * dot)
    if dres is not None and not drop_dres:
        o = o + dres.float()
        if dres_twice:
            o = o + dres.float()
    dx = o.to(T)
    if not want_dw:
        return dx, None
    prod = df * (bf(xh) if T == BF else xh)
    rpb = rows if rpb is None else rpb
    partials = []
    for r0 in range(0, rows, rpb):
        r1 = min(rows, r0 + rpb) - (1 if dw_miss_last_row else 0)
        acc = [torch.zeros(cols) for _ in range(slots)]
        for i in range(r0, r1):
            acc[(i - r0) % slots] = acc[(i - r0) % slots] + prod[i]
        fold = acc[0]
        for a in acc[1:]:
            fold = fold + a
        partials.append(fold)
    groups = [torch.zeros(cols) for _ in range(16)]
    for p, part in enumerate(partials):
        groups[p % 16] = groups[p % 16] + part
    s = torch.zeros(cols)
    for gsum in groups:
        s = s + gsum
    if beta != 0.0:
        s = s + torch.tensor(beta) * dw_old.float()
    return dx, s.to(dw_dtype)


# ---------------------------------------------------------------------------------------------
# LayerNorm (layernorm_fwd_k, layernorm_bwd_k)
# ---------------------------------------------------------------------------------------------
def ln_fwd_gate(y, mean, rstd, x, w, b, eps=EPS):
    """With a = mean_c |x| and xh = (x - mean) r:
    mean: an f32 sum of cols terms in any order and one divide, (cols + 2) E a.
    rstd: the f32 mean moves sum (x - mean)^2 only to second order (the deviations sum to zero);
    each square carries the rounding of its difference twice and its own, the sum cols more, then a
    divide, an add and rsqrtf, halved by the root: (cols + 16) E ref.
    y = xh w + b: the mean's error enters as (cols + 2) E a r |w|, rstd's and the three products' /
    differences' as (cols + 16) E |w xh|, the add of b rounds the result and leaves b's share within
    4 E |b|; the store is Ust |ref|.
    Returns (worst of mean, worst of rstd, worst of y)."""
    X, W, B = x.double(), w.double(), b.double()
    cols = X.shape[1]
    m = X.mean(1, keepdim=True)
    r = (((X - m) ** 2).mean(1, keepdim=True) + eps).rsqrt()
    a = X.abs().mean(1, keepdim=True)
    xh = (X - m) * r
    ref = xh * W + B
    gate = ust(y.dtype) * ref.abs() + E * ((cols + 16) * a * r * W.abs() + (cols + 16) * (W * xh).abs()
                                            + 4 * B.abs()) + FLOOR
    return (worst(mean.double()[:, None] - m, (cols + 2) * E * a + FLOOR),
            worst(rstd.double()[:, None] - r, (cols + 16) * E * r + FLOOR),
            worst(y.double() - ref, gate))


def ln_fwd_honest(x, w, b, eps=EPS):
    """layernorm_fwd_k restated in torch f32: (y, mean, rstd)"""
    xf = x.float()
    cols = torch.tensor(float(xf.shape[1]))
    mean = (wave_part_sums(xf)[0] / cols)[:, None]
    d = xf - mean
    r = torch.rsqrt(wave_part_sums(d * d)[0] / cols + torch.tensor(eps))[:, None]
    y = d * r * w.float() + b.float()
    return y.to(x.dtype), mean[:, 0], r[:, 0]


def ln_bwd_gate(dx, dw, db, dy, x, w, mean, rstd, dres=None):
    """With the f32 mean and rstd given, xh = (x - mean) r, g = dy w, sg = mean_c g, sgx = mean_c g xh:
    dx: ref = r (g - sg - xh sgx) + dres, gate Ust |ref| + E r [(cols + 2) mean|g| + (cols + 6) |xh| mean|g xh|
        + 8 (|g| + |sg| + |xh sgx|)] + 2 E |dres|: the two f32 row sums in any order (sg's terms round
        once, sgx's carry xh's two roundings and their own), each term of the bracket rounded a few
        times on its way through the two subtractions, the product with r and the residual add.
    dw: ref = sum_rows dy xh, gate (rows + 8) E sum |dy xh|; db: ref = sum_rows dy, gate (rows + 8) E sum |dy|
        (f32 sums over rows in any order; xh rounds twice, the product once).
    Returns (worst of dx, worst of dw or None, worst of db or None)."""
    X, W, DY = x.double(), w.double(), dy.double()
    rows, cols = X.shape
    r = rstd.double()[:, None]
    xh = (X - mean.double()[:, None]) * r
    g = DY * W
    sg, sgx = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    D = dres.double() if dres is not None else torch.zeros((), dtype=torch.float64, device=X.device)
    ref = r * (g - sg - xh * sgx) + D
    gate = ust(dx.dtype) * ref.abs() + E * r * ((cols + 2) * g.abs().mean(1, keepdim=True)
                                                 + (cols + 6) * xh.abs() * (g * xh).abs().mean(1, keepdim=True)
                                                 + 8 * (g.abs() + sg.abs() + (xh * sgx).abs())) + 2 * E * D.abs() + FLOOR
    wdx = worst(dx.double() - ref, gate)
    if dw is None:
        return wdx, None, None
    pw = DY * xh
    return (wdx, worst(dw.double() - pw.sum(0), (rows + 8) * E * pw.abs().sum(0) + FLOOR),
            worst(db.double() - DY.sum(0), (rows + 8) * E * DY.abs().sum(0) + FLOOR))


def ln_bwd_honest(dy, x, w, mean, rstd, dres=None, no_sg=False, no_sgx=False, db_miss_row=False):
    """layernorm_bwd_k restated in torch f32: (dx, dw, db), dw and db f32. The keyword arguments are the
    mutants."""
    xf, df, wf = x.float(), dy.float(), w.float()
    rows, cols = xf.shape
    r = rstd.float()[:, None]
    xh = (xf - mean.float()[:, None]) * r
    g = df * wf
    c = torch.tensor(float(cols))
    sg = (wave_part_sums(g)[0] / c)[:, None]
    sgx = (wave_part_sums(g * xh)[0] / c)[:, None]
    if no_sg:
        sg = torch.zeros_like(sg)
    if no_sgx:
        sgx = torch.zeros_like(sgx)
    o = r * (g - sg - xh * sgx)
    if dres is not None:
        o = o + dres.float()
    pw = df * xh
    dw, db = torch.zeros(cols), torch.zeros(cols)
    for i in range(rows):
        dw = dw + pw[i]
        if not (db_miss_row and i == rows - 1):
            db = db + df[i]
    return o.to(x.dtype), dw, db


# ---------------------------------------------------------------------------------------------
# cross entropy (loss.hip)
# ---------------------------------------------------------------------------------------------
CE_PAD = 30.0   # in the columns V .. ldl-1 of the logits buffer: a kernel that read them would move lse by > 14
CE_SENT = -7.0  # in the whole gradient buffer before ce_bwd


def ce_inputs(rows, V, dtype=BF, kind="normal"):
    """(logits [rows, V]: a view of a [rows, ldl] buffer, ldl = V rounded up to 8, whose other columns
    hold CE_PAD; targets [rows] int64). Logits are 2 n (|lse| < 16: lse is about log V + 2).
    "planted_last": column V-1 holds 12.0, the row's largest; "ascending": every row sorted, so every
    step of the online maximum rescales. Targets: row 0 column 0, row 1 column V-1, row 2 column V-2
    (inside the tail when V % 8 >= 2), row 3 ignored, the rest random with a quarter ignored."""
    g = _gen(f"ce-{rows}-{V}-{dtype}-{kind}")
    ldl = -(-V // 8) * 8
    buf = 2.0 * torch.randn(rows, ldl, generator=g)
    if kind == "planted_last":
        buf[:, V - 1] = 12.0
    if kind == "ascending":
        buf[:, :V] = buf[:, :V].sort(1).values
    buf[:, V:] = CE_PAD
    buf = buf.to(dtype)
    t = torch.randint(0, V, (rows,), generator=g)
    t[torch.rand(rows, generator=g) < 0.25] = IGNORE
    t[0], t[1], t[2], t[3] = 0, V - 1, V - 2, IGNORE
    return buf[:, :V], t


def ce_ref(logits, targets, ignore=IGNORE):
    """(lse, row loss, x_t, valid) in f64; the loss of an ignored row is 0"""
    X = logits.double()
    valid = targets != ignore
    lse = torch.logsumexp(X, 1)
    xt = X.gather(1, targets.clamp_min(0)[:, None])[:, 0]
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    return lse, torch.where(valid, lse - xt, zero), torch.where(valid, xt, zero), valid


def ce_stats(logits, targets, ignore=IGNORE):
    """what ce_bwd takes from the forward, built from the f64 reference and rounded once to f32:
    (row_lse [rows], row_loss [rows], loss_out [3] = mean loss, count, 1 / count)"""
    lse, loss, _, valid = ce_ref(logits, targets, ignore)
    cnt = valid.sum().double()
    out = torch.stack([loss[valid].sum() / cnt, cnt, 1.0 / cnt]).float()
    return lse.float(), loss.float(), out


def ce_fwd_gate(row_loss, row_lse, logits, targets, ignore=IGNORE):
    """row_lse: |lse - ref| <= 1e-5, the project's LSE gate of the attention kernels (|lse| < 16, where
    one f32 rounding of lse is 1e-6). row_loss = lse - x_t: 1e-5 + 2 E (|lse| + |x_t|); rows with an
    ignored target exactly 0.0. Returns (worst of lse, worst of loss, ignored rows exactly zero)."""
    lse, loss, xt, valid = ce_ref(logits, targets, ignore)
    zero_ok = bool((row_loss[~valid] == 0).all().item())
    return (worst(row_lse.double() - lse, torch.full_like(lse, 1e-5)),
            worst(row_loss.double() - loss, 1e-5 + 2 * E * (lse.abs() + xt.abs()) + FLOOR), zero_ok)


def ce_reduce_check(out, row_loss, targets, ignore=IGNORE):
    """out[0] within 2 E |ref| of the f64 mean of the selected f32 row losses (a double sum, one
    rounding to f32), out[1] exactly the count, out[2] exactly float(1 / count); nothing selected:
    NaN, 0, inf. Returns the failures."""
    valid = targets != ignore
    cnt = int(valid.sum())
    o = out.double().cpu()
    fails = []
    if cnt == 0:
        if not (math.isnan(o[0]) and o[1] == 0 and o[2] == float("inf")):
            fails.append(f"nothing selected: {o.tolist()} instead of nan, 0, inf")
        return fails
    ref = (row_loss.double()[valid].sum() / cnt).item()
    if not abs(o[0].item() - ref) <= 2 * E * abs(ref) + FLOOR:
        fails.append(f"mean {o[0].item()!r} vs {ref!r}")
    if o[1].item() != cnt:
        fails.append(f"count {o[1].item()} vs {cnt}")
    if o[2].item() != torch.tensor(1.0 / cnt, dtype=torch.float64).float().item():
        fails.append(f"1 / count {o[2].item()!r}")
    return fails


def ce_bwd_gate(d, logits, targets, row_lse, loss_out, grad_loss=None, ignore=IGNORE):
    """Given the f32 lse: p = exp(x - lse), ref = (p - [col == t]) scale, scale = grad_loss / count
    (the two f32 values given, multiplied exactly here, rounded once in the kernel), 0 on ignored rows.
    |d - ref| <= Ust |ref| + |scale| (p rho + 2 E (p + [col == t])), rho = (|x| + |lse| + |x - lse| + 2) 2^-23:
    the fast exponential's argument x - lse rounds once and once more against log2(e), which moves p by
    about |x - lse| 2^-23, the exp2 itself by an ulp; the subtraction and the product with scale round
    the result, scale's own rounding is one E of either term. Holds where p - 1 cancels at the target.
    Returns (worst, ignored rows exactly zero over all V columns)."""
    X = logits.double()
    valid = targets != ignore
    l = row_lse.double()[:, None]
    p = torch.exp(X - l)
    hot = torch.zeros_like(X)
    hot.scatter_(1, targets.clamp_min(0)[:, None], 1.0)
    hot = hot * valid[:, None]
    gl = 1.0 if grad_loss is None else grad_loss.double().reshape(-1)[0]
    scale = (valid.double() * gl * loss_out.double()[2])[:, None]
    ref = (p - hot) * scale
    rho = (X.abs() + l.abs() + (X - l).abs() + 2) * 2.0 ** -23
    gate = ust(d.dtype) * ref.abs() + scale.abs() * (p * rho + 2 * E * (p + hot)) + FLOOR
    zero_ok = bool((d[~valid].float() == 0).all().item())
    return worst(d.double() - ref, gate), zero_ok


def ce_fwd_honest(logits, targets, ignore=IGNORE, skip_tail=False, no_rescale=False):
    """ce_fwd_k restated in torch f32: 256 threads each run the online (max, sum) over their 8-wide
    vectors (2048 columns a pass) and then over the tail, a butterfly combines the 64 lanes of a wave,
    thread 0 the four waves. Returns (row_loss, row_lse). skip_tail / no_rescale are mutants."""
    x = logits.float()
    rows, V = x.shape
    nv = V // 8
    ninf = float("-inf")
    m, s = torch.full((rows, 256), ninf), torch.zeros(rows, 256)
    body = x[:, :nv * 8].reshape(rows, nv, 8)
    for lo in range(0, nv, 256):
        n = min(nv, lo + 256) - lo
        v = body[:, lo:lo + n]
        mo, so = m[:, :n].clone(), s[:, :n].clone()
        nm = torch.maximum(mo, v.amax(-1))
        acc = torch.zeros(rows, n)
        for j in range(8):
            acc = acc + torch.exp(v[:, :, j] - nm)
        s[:, :n] = (so if no_rescale else so * torch.exp(mo - nm)) + acc
        m[:, :n] = nm
    n = V - nv * 8
    if n and not skip_tail:
        v = x[:, nv * 8:]
        mo, so = m[:, :n].clone(), s[:, :n].clone()
        nm = torch.maximum(mo, v)
        s[:, :n] = so * torch.exp(mo - nm) + torch.exp(v - nm)
        m[:, :n] = nm

    def combine(m, s, om, os):
        nm = torch.maximum(m, om)
        dead = nm == ninf
        nz = torch.where(dead, torch.zeros_like(nm), nm)
        return nm, torch.where(dead, torch.zeros_like(s), s * torch.exp(m - nz) + os * torch.exp(om - nz))

    m, s = m.view(rows, 4, 64), s.view(rows, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        m, s = combine(m, s, m[..., _LANE ^ o], s[..., _LANE ^ o])
    M, S = m[:, 0, 0], s[:, 0, 0]
    for wv in range(1, 4):
        M, S = combine(M, S, m[:, wv, 0], s[:, wv, 0])
    lse = M + torch.log(S)
    valid = targets != ignore
    xt = x.gather(1, targets.clamp_min(0)[:, None])[:, 0]
    return torch.where(valid, lse - xt, torch.zeros(())), lse


def ce_bwd_honest(logits, targets, row_lse, loss_out, grad_loss=None, ignore=IGNORE, no_onehot_in_tail=False,
                  ignore_grad_loss=False, keep_ignored=False):
    """ce_bwd_k restated in torch f32. The last three keyword arguments are the mutants."""
    x = logits.float()
    rows, V = x.shape
    valid = targets != ignore
    gl = torch.ones(()) if (grad_loss is None or ignore_grad_loss) else grad_loss.float().reshape(-1)[0]
    sc = gl * loss_out.float()[2]
    scale = (sc * torch.ones(rows) if keep_ignored else torch.where(valid, sc, torch.zeros(())))[:, None]
    hot = torch.zeros_like(x)
    hot.scatter_(1, targets.clamp_min(0)[:, None], 1.0)
    hot = hot * valid[:, None]
    if no_onehot_in_tail:
        hot[:, V // 8 * 8:] = 0
    return ((torch.exp(x - row_lse.float()[:, None]) - hot) * scale).to(logits.dtype)


def shift_targets_ref(labels, mask, ignore=IGNORE):
    """targets[b, t] = labels[b, t + 1] where t + 1 < L and mask[b, t + 1] != 0 (mask None: everywhere),
    else ignore; flattened"""
    B, L = labels.shape
    t = torch.full((B, L), ignore, dtype=torch.int64, device=labels.device)
    nxt = labels[:, 1:].to(torch.int64)
    t[:, :L - 1] = nxt if mask is None else torch.where(mask[:, 1:] != 0, nxt, torch.full_like(nxt, ignore))
    return t.reshape(-1)


# ---------------------------------------------------------------------------------------------
# SwiGLU and activation backward (elementwise.hip)
# ---------------------------------------------------------------------------------------------
def act_values(n, dtype, name):
    """n values within +-16: 4 n clamped, the first ones replaced by 0, +-16, the zeros of the two
    slopes (silu' at g = -1.278, gelu' and quick_gelu' at v = -0.75) and a dense band around each
    (steps below bf16's spacing there)"""
    g = _gen(f"act-{name}-{n}-{dtype}")
    v = (4.0 * torch.randn(n, generator=g)).clamp(-16.0, 16.0)
    special = torch.cat([torch.tensor([0.0, 16.0, -16.0, -1.278, -0.75, -1.2785, -0.7518, -0.0]),
                         torch.linspace(-1.40, -1.15, 56), torch.linspace(-0.85, -0.65, 56)])
    k = min(n, special.numel())
    v[:k] = special[:k]
    return v.to(dtype)


def swiglu_inputs(rows, F, dtype=BF):
    """gu [rows, 2F] = gate | up, dout [rows, F] (CPU). The up half and dout end in 0, 16, -16."""
    g = _gen(f"swiglu-train-{rows}-{F}-{dtype}")
    gate = act_values(rows * F, dtype, "swiglu").view(rows, F)
    up = (2.0 * torch.randn(rows, F, generator=g)).clamp(-16.0, 16.0)
    d = torch.randn(rows, F, generator=g)
    for t in (up, d):
        t[-1, -3:] = torch.tensor([0.0, 16.0, -16.0])
    return torch.cat([gate, up.to(dtype)], 1).contiguous(), d.to(dtype)


def act_inputs(n, dtype=BF):
    """(dy [n], preact [n])"""
    g = _gen(f"act-bwd-{n}-{dtype}")
    return torch.randn(n, generator=g).to(dtype), act_values(n, dtype, "preact")


def _two(dtype):
    return 2 * U * (1 + U) if dtype == BF else 4 * E


def swiglu_fwd_gate(o, gu):
    """ref = silu(g) u; o = round(round(silu(g)) * u): two roundings of the value, 2 U (1 + U) (4 E for
    f32: the quotient and the product); the f32 silu = g / (1 + exp(-g)) adds the fast exponential's
    |g| 2^-23 and a few roundings: (|g| + 6) 2^-23. Both times |ref|."""
    F = gu.shape[1] // 2
    g, u = gu[:, :F].double(), gu[:, F:].double()
    ref = g * torch.sigmoid(g) * u
    return worst(o.double() - ref, (_two(o.dtype) + (g.abs() + 6) * 2.0 ** -23) * ref.abs() + FLOOR)


def swiglu_bwd_gate(dgu, dout, gu):
    """dup = round(d * round(silu(g))): the forward's gate on ref = d silu(g).
    dgate: ref = d u s (1 + g (1 - s)), s = sigmoid(g). The slope 1 + g (1 - s) vanishes at g = -1.278, so
    its f32 error is absolute: s carries (|g| + 6) 2^-24 relative, which 1 - s, its product with g and
    the sum turn into at most (|g| + 6)(1 + |g|) 2^-24 of the slope's scale 1 + |g|; the products with
    d u s add their roundings relative to the same scale: gated at Ust |ref| + 2^-21 (|g| + 6)(1 + |g|) s |d u|.
    Returns (worst of dgate, worst of dup)."""
    F = gu.shape[1] // 2
    g, u, d = gu[:, :F].double(), gu[:, F:].double(), dout.double()
    s = torch.sigmoid(g)
    ref_g = d * u * s * (1 + g * (1 - s))
    gate_g = ust(dgu.dtype) * ref_g.abs() + 2.0 ** -21 * (g.abs() + 6) * (1 + g.abs()) * s * (d * u).abs() + FLOOR
    ref_u = d * g * s
    gate_u = (_two(dgu.dtype) + (g.abs() + 6) * 2.0 ** -23) * ref_u.abs() + FLOOR
    return worst(dgu[:, :F].double() - ref_g, gate_g), worst(dgu[:, F:].double() - ref_u, gate_u)


def _rnd(t, dtype):
    return bf(t) if dtype == BF else t


def swiglu_fwd_honest(gu, swap_halves=False):
    F = gu.shape[1] // 2
    g, u = gu[:, :F].float(), gu[:, F:].float()
    if swap_halves:
        g, u = u, g
    return (_rnd(g / (1.0 + torch.exp(-g)), gu.dtype) * u).to(gu.dtype)


def swiglu_bwd_honest(dout, gu, slope_no_s=False, swap_halves=False):
    """swiglu_bwd_k restated in torch f32; slope_no_s (1 + g (1 - s) -> 1 + g) and swap_halves are mutants"""
    F = gu.shape[1] // 2
    g, u, d = gu[:, :F].float(), gu[:, F:].float(), dout.float()
    if swap_halves:
        g, u = u, g
    s = 1.0 / (1.0 + torch.exp(-g))
    b = d * _rnd(g * s, gu.dtype)
    a = d * u * s * (1.0 + (g if slope_no_s else g * (1.0 - s)))
    return torch.cat([a, b], 1).to(gu.dtype)


def act_bwd_gate(dx, dy, v, act):
    """quick_gelu: with z = 1.702 v and s = sigmoid(z), ref = dy s (1 + z (1 - s)): swiglu's dgate form,
    Ust |ref| + 2^-21 (|z| + 6)(1 + |z|) s |dy|.
    gelu: ref = dy (Phi(v) + v phi(v)); Phi = 0.5 (1 + erf) and v phi each carry an absolute f32 error of a
    few E where they cancel (v = -0.75): Ust |ref| + 2^-20 |dy|."""
    V, D = v.double(), dy.double()
    if act == "gelu":
        ref = D * (0.5 * (1 + torch.erf(V / math.sqrt(2.0))) + V * torch.exp(-0.5 * V * V) / math.sqrt(2 * math.pi))
        gate = ust(dx.dtype) * ref.abs() + 2.0 ** -20 * D.abs() + FLOOR
    else:
        z = 1.702 * V
        s = torch.sigmoid(z)
        ref = D * s * (1 + z * (1 - s))
        gate = ust(dx.dtype) * ref.abs() + 2.0 ** -21 * (z.abs() + 6) * (1 + z.abs()) * s * D.abs() + FLOOR
    return worst(dx.double() - ref, gate)


def act_bwd_honest(dy, v, act, no_vpdf=False, lose_1702=False):
    """act_bwd_k restated in torch f32; no_vpdf (gelu) and lose_1702 (quick_gelu's second term) are mutants"""
    x, d = v.float(), dy.float()
    if act == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
        pdf = 0.39894228040143268 * torch.exp(-0.5 * x * x)
        dg = cdf if no_vpdf else cdf + x * pdf
    else:
        s = 1.0 / (1.0 + torch.exp(-(1.702 * x)))
        dg = s + (x if lose_1702 else 1.702 * x) * s * (1.0 - s)
    return (d * dg).to(dy.dtype)
