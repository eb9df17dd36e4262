"""float64 references, gates and input sets for the decode step's kernels (csrc/gemv.hip,
csrc/decode.hip, the RoPE kernels of csrc/elementwise.hip). Plain torch on whatever device the
tensors live on: tests/test_decode_refs_host.py proves on the CPU that every gate passes an honest
f32 restatement of the kernel and fails a set of one-line mutants, tests/test_decode_accuracy_gpu.py
then holds the kernels to the same gates on the same inputs (same seeds, same shapes).

U = 2^-8 is the largest relative error of one bf16 round-to-nearest (8 significant bits);
2^-24 the same for f32. No number here was taken from a kernel's output.
"""
import zlib

import torch

BF = torch.bfloat16
U = 2.0 ** -8
D_HEAD = 128
CHUNK = 64  # keys per workgroup of attn_decode_k


def bf(x):
    """one bf16 round-to-nearest of an f32 tensor, back in f32"""
    return x.to(BF).float()


def worst(err, gate):
    """max err / gate over the elements; 0 / 0 counts as 0 and x / 0 as inf"""
    err, gate = err.double().abs(), gate.double()
    r = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(err))
    r = torch.where(torch.isnan(err), torch.full_like(r, float("inf")), r)
    return r.max().item() if r.numel() else 0.0


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------------------------
# GEMV (gemv.hip): Y[M, N] = X[M, K] W[N, K]^T
# ---------------------------------------------------------------------------------------------
# (M, N, K): every case is plan tile 14
GEMV_CASES = [(1, 16, 32), (5, 24, 72), (2, 8, 64), (16, 776, 1000), (7, 264, 4096), (8, 4096, 4096),
              (3, 40, 8200), (2, 16392, 136), (15, 16400, 72)]
# (M, N, K) of decode_linear transform 3 (w holds 2N rows: the kernel variant is chosen on 2N)
SWIGLU_CASES = [(3, 8, 72), (16, 8200, 136)]


def gemv_waves(N, K):
    """waves per workgroup = contiguous K ranges of the variant gemv.hip picks for (N, K)"""
    return 16 if (K < 8192 and N > 16384) else 8


def gemv_inputs(M, N, K, name="gemv"):
    """bf16 X [M, K], W [N, K], bias [N], addend [M, N], residual [M, N] (CPU)"""
    g = _gen(f"{name}-{M}-{N}-{K}")
    X = torch.randn(M, K, generator=g).to(BF)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
    bias = torch.randn(N, generator=g).to(BF)
    add = torch.randn(M, N, generator=g).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    return X, W, bias, add, res


def gemv_ref(X, W):
    """(f64 product X W^T, absprod = |X| |W|^T in f64)"""
    Xd, Wd = X.double(), W.double()
    return Xd @ Wd.T, Xd.abs() @ Wd.abs().T


def gemv_gate(c32, ref, absprod, K):
    """The f32 output of the product against f64 (the gates of test_accuracy_gpu.py):
    bf16 x bf16 products are exact in f32, so the only error is the f32 summation of K terms, and
    for ANY order of that sum |c - ref| <= (K - 1) 2^-24 sum|x_k w_k| to first order: gated at
    K 2^-24 absprod per element, and rel-L2 <= 1e-5 over the tensor.
    Returns (worst err / bound, rel-L2)."""
    err = c32.double() - ref
    return worst(err, K * 2.0 ** -24 * absprod), (err.norm() / ref.norm()).item()


def gemv_gate_ok(c32, ref, absprod, K):
    w, rel = gemv_gate(c32, ref, absprod, K)
    return w <= 1.0 and rel <= 1e-5


def epilogue_replay(c32, bias=None, addend=None, residual=None):
    """store4's chain (gemm_common.h) on the kernel's own f32 product, in torch f32: v = c32;
    v += bias; v = bf16(v) + addend; v = bf16(v) + residual; bf16(v). Every step is one f32 add or
    one bf16 rounding, so this is bit for bit what the kernel stores."""
    v = c32.float()
    if bias is not None:
        v = v + bias.float()
    if addend is not None:
        v = bf(v) + addend.float()
    if residual is not None:
        v = bf(v) + residual.float()
    return v.to(BF)


def gemv_honest(X, W, waves=8, drop_tail8=False, drop_step=None, double_step=None, row_last_as_0=False,
                clamp_n_tail=False):
    """gemv_k restated in torch f32: `waves` contiguous K ranges of cdiv(cdiv(K, 32), waves) 32-deep
    k-steps, each summed in f32, the partials added in wave order. The keyword arguments are the
    mutants of test_decode_refs_host.py."""
    Xf, Wf = X.float(), W.float()
    M, K = Xf.shape
    N = Wf.shape[0]
    if row_last_as_0:  # row M-1 of X read as row 0
        Xf = Xf.clone()
        Xf[M - 1] = Xf[0]
    if clamp_n_tail:  # the last 8 weight rows clamped to row N-9
        Wf = Wf.clone()
        Wf[N - 8:] = Wf[N - 9]
    keep = torch.ones(K)
    if drop_tail8:
        keep[K - 8:] = 0
    if drop_step is not None:
        keep[32 * drop_step:32 * drop_step + 32] = 0
    if double_step is not None:
        keep[32 * double_step:32 * double_step + 32] = 2
    Xf = Xf * keep  # exact in f32 (x0, x1, x2)
    nk = -(-K // 32)
    per = -(-nk // waves) * 32
    acc = None
    for w in range(waves):
        lo, hi = w * per, min(K, (w + 1) * per)
        part = Xf[:, lo:hi] @ Wf[:, lo:hi].T if lo < hi else torch.zeros(M, N)
        acc = part if acc is None else acc + part
    return acc


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def swiglu_gate(y, g, up, dg, dup):
    """decode_linear transform 3: y = bf16(bf16(silu(bf16(g32))) * bf16(up32)) against silu(g) * up of
    the f64 products g, up; dg, dup = K 2^-24 absprod, the f32 summation bounds of g32 and up32.

    Three roundings act on the value itself (bf16 of silu, bf16 of up32, bf16 of the product):
    3 U |silu(g) up|. The gate product is perturbed before silu, by its f32 sum (dg) and its own bf16
    rounding (U |g|), and silu carries that into the output with slope |silu'| (silu' = s (1 + g (1 - s)),
    s = sigmoid(g); at most 1.0999): |silu'(g)| (U |g| + dg) |up|. The up product's f32 sum adds
    |silu(g)| dup. First order in U; the second-order terms are below 4 U^2 of the first term.

    The issue stated the last bracket as U (|dg up| + |silu(g) dup|), which leaves no term for the
    bf16 rounding of g32: an honest f32 restatement exceeds that form by several times at negative g,
    where silu is small but its slope times |g| is not (test_swiglu_issue_form_rejects_honest), so the
    derivation above replaces it, as the issue directs for a derivation an honest restatement breaks.
    Returns worst err / gate."""
    g, up = g.double(), up.double()
    s = torch.sigmoid(g)
    slope = (s * (1.0 + g * (1.0 - s))).abs()
    ref = silu64(g) * up
    gate = 3 * U * ref.abs() + slope * (U * g.abs() + dg) * up.abs() + silu64(g).abs() * dup
    return worst(y.double() - ref, gate)


def swiglu_gate_issue_form(y, g, up, dg, dup):
    """the bound as the issue wrote it (see swiglu_gate): kept to show that an honest restatement
    does not meet it"""
    g, up = g.double(), up.double()
    ref = silu64(g) * up
    gate = 3 * U * ref.abs() + U * ((dg * up).abs() + (silu64(g) * dup).abs())
    return worst(y.double() - ref, gate)


def swiglu_honest(X, W2, waves=8):
    """the kernel's OT = 1 epilogue on the honest f32 products: W2 [2N, K] = gate rows | up rows"""
    N = W2.shape[0] // 2
    z = gemv_honest(X, W2, waves)
    g, up = bf(z[:, :N]), bf(z[:, N:])
    return bf(bf(g / (1.0 + torch.exp(-g))) * up).to(BF)


# ---------------------------------------------------------------------------------------------
# decode attention (decode.hip)
# ---------------------------------------------------------------------------------------------
ATTN_H = 3
# name -> (max_len, [(kv_start, kv_len), ...]): one launch each, the pairs are the batch rows
ATTN_CASES = {
    "edges192": (192, [(0, 1), (0, 63), (0, 64), (0, 65), (0, 128), (0, 129)]),
    "starts576": (576, [(17, 513), (63, 64), (64, 65), (65, 200), (130, 131), (1, 3), (200, 200), (5, 0)]),
    "regs2048": (2048, [(0, 2048), (1999, 2048)]),
    "loop2112": (2112, [(0, 2112), (0, 2049), (2050, 2112), (0, 70)]),
}
# the planted key: the pairs of the first two cases with at least two keys
PLANT_MAX_LEN = 576
PLANT_PAIRS = [p for c in ("edges192", "starts576") for p in ATTN_CASES[c][1] if p[1] - p[0] >= 2]
PLANT_LOCS = ("first", "last", "below", "above")


def attn_inputs(name, max_len, B, H=ATTN_H, D=D_HEAD):
    """q: a column block [B, H*D] of a [B, 3*H*D] row; caches [B, max_len, H*D] inside rows of
    H*D + 64 (CPU, bf16, N(0, 1))"""
    g = _gen("attn-" + name)
    qrow = torch.randn(B, 3 * H * D, generator=g).to(BF)
    kbuf = torch.randn(B, max_len, H * D + 64, generator=g).to(BF)
    vbuf = torch.randn(B, max_len, H * D + 64, generator=g).to(BF)
    return qrow[:, H * D:2 * H * D], kbuf[:, :, :H * D], vbuf[:, :, :H * D]


def plant_location(loc, lo, hi, max_len):
    """cache row of the planted key, or None where the pair has no such row"""
    r = {"first": lo, "last": hi - 1, "below": lo - 1, "above": hi}[loc]
    return r if 0 <= r < max_len else None


def plant(q, kc, vc, pairs, loc, H=ATTN_H, D=D_HEAD):
    """k* = 4 q_h (exact in bf16; score 4 |q_h|^2 / sqrt(D), about 45, against N(0, 1) scores) and
    v* = 8.0 at the location's row of every batch row. Returns the planted rows (None: no row)."""
    rows = []
    for b, (lo, hi) in enumerate(pairs):
        r = plant_location(loc, lo, hi, kc.shape[1])
        rows.append(r)
        if r is not None:
            kc[b, r] = (4.0 * q[b].float()).to(BF)
            vc[b, r] = 8.0
    return rows


def window(kv_start, kv_len, L):
    """bool [B, L]: key j of batch row b is visible"""
    j = torch.arange(L, device=kv_len.device)[None, :]
    return (j >= kv_start[:, None]) & (j < kv_len[:, None])


def fill_outside(kc, vc, vis, value, keep_rows=None):
    """copies of the caches with every row outside the window set to `value` (keep_rows [B]: one
    row per batch row left as it is, None entries ignored)"""
    out = ~vis
    if keep_rows is not None:
        out = out.clone()
        for b, r in enumerate(keep_rows):
            if r is not None:
                out[b, r] = False
    kc2, vc2 = kc.clone(), vc.clone()
    kc2[out] = value
    vc2[out] = value
    return kc2, vc2


def decode_attn_ref(q, kc, vc, kv_start, kv_len, scale, D=D_HEAD):
    """f64 softmax attention of one query row per (b, h) over keys [kv_start[b], kv_len[b]).
    q [B, H*D], caches [B, L, H*D] (views). Returns (o [B, H*D], pv_abs = sum_j p_j |v_j| [B, H*D],
    n = kv_len - kv_start [B]); rows with an empty window are zero. Cache rows outside the window are
    never multiplied in (they may hold NaN)."""
    B, L = kc.shape[0], kc.shape[1]
    H = q.shape[1] // D
    vis = window(kv_start, kv_len, L)
    zero = torch.zeros((), dtype=torch.float64, device=q.device)
    K = torch.where(vis[:, :, None], kc.double(), zero).view(B, L, H, D)
    V = torch.where(vis[:, :, None], vc.double(), zero).view(B, L, H, D)
    S = torch.einsum("bhd,blhd->bhl", q.double().reshape(B, H, D), K) * scale
    S = S.masked_fill(~vis[:, None, :], float("-inf"))
    m = S.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(S - m)
    l = p.sum(-1, keepdim=True)
    p = p / torch.where(l > 0, l, torch.ones_like(l))
    o = torch.einsum("bhl,blhd->bhd", p, V).reshape(B, H * D)
    pv_abs = torch.einsum("bhl,blhd->bhd", p, V.abs()).reshape(B, H * D)
    return o, pv_abs, (kv_len - kv_start).clamp_min(0)


def attn_gate(o, ref, pv_abs, n):
    """|o - ref| <= U |ref| + (n + 8) 2^-23 pv_abs per element; rows with an empty window exactly 0.

    The kernel rounds to bf16 once, at the output: U |ref|. Everything before it is f32: the
    probabilities p_j = exp2(s_j - m) (exp2f and the subtraction, a couple of 2^-24 each), the sums
    sum_j p_j v_j and sum_j p_j over n terms in some order ((n - 1) 2^-24 of sum_j p_j |v_j| each,
    whatever the order: 16 key groups, 64-key chunks, chunk order), the chunk rescale exp2(m_c - M),
    its products and the division (one 2^-24 each): (2 (n - 1) + ~8) 2^-24 pv_abs, gated at
    (n + 8) 2^-23 pv_abs. The f32 score itself (a 128-term dot, absolute error ~1e-6, the same
    relative error on p_j) sits inside the + 8 for two keys and far below n 2^-23 beyond; with one
    key p = 1 exactly. Returns (worst err / gate, every empty row exactly zero)."""
    nn = n.double()[:, None]
    gate = U * ref.abs() + (nn + 8) * 2.0 ** -23 * pv_abs
    empty = (n == 0)
    zero_ok = bool((o[empty].float() == 0).all().item()) if bool(empty.any()) else True
    return worst(o.double() - ref, gate), zero_ok


def attn_gate_rows(o, ref, pv_abs, n):
    """worst err / gate per batch row"""
    return [attn_gate(o[b:b + 1], ref[b:b + 1], pv_abs[b:b + 1], n[b:b + 1])[0] for b in range(o.shape[0])]


def attn_honest(q, kc, vc, kv_start, kv_len, scale, D=D_HEAD, drop_chunk=None, no_rescale=False,
                swap_heads=False):
    """attn_decode_k + attn_decode_combine_k restated in torch f32: q * scale * log2(e), scores, per
    64-key chunk the max, p = exp2(s - m_c), l_c = sum p, o_c = p V; then M = max m_c,
    w_c = exp2(m_c - M), o = bf16(sum w_c o_c / sum w_c l_c). drop_chunk [B] (one chunk index per batch
    row, -1 none), no_rescale and swap_heads are the mutants."""
    B, L = kc.shape[0], kc.shape[1]
    H = q.shape[1] // D
    nc = -(-L // CHUNK)
    Lp = nc * CHUNK
    vis = window(kv_start, kv_len, L)
    if drop_chunk is not None:
        ch = torch.arange(L)[None, :] // CHUNK
        vis = vis & (ch != drop_chunk[:, None])
    visp = torch.zeros(B, Lp, dtype=torch.bool)
    visp[:, :L] = vis
    K = torch.zeros(B, Lp, H, D)
    V = torch.zeros(B, Lp, H, D)
    K[:, :L] = torch.where(vis[:, :, None], kc.float(), torch.zeros(())).view(B, L, H, D)
    V[:, :L] = torch.where(vis[:, :, None], vc.float(), torch.zeros(())).view(B, L, H, D)
    qs = q.float().reshape(B, H, D) * torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    S = torch.einsum("bhd,blhd->bhl", qs, K).masked_fill(~visp[:, None, :], float("-inf"))
    S = S.view(B, H, nc, CHUNK)
    mc = S.amax(-1)  # [B, H, nc]
    mfin = torch.where(torch.isinf(mc), torch.zeros_like(mc), mc)
    P = torch.exp2(S - mfin[..., None])
    lc = P.sum(-1)
    oc = torch.einsum("bhck,bckhd->bhcd", P, V.view(B, nc, CHUNK, H, D))
    Mx = mc.amax(-1, keepdim=True)
    Mfin = torch.where(torch.isinf(Mx), torch.zeros_like(Mx), Mx)
    w = torch.where(torch.isinf(mc), torch.zeros_like(mc), torch.exp2(mc - Mfin))
    if no_rescale:
        w = (w > 0).float()
    Lsum = torch.zeros(B, H)
    acc = torch.zeros(B, H, D)
    for c in range(nc):  # chunk order, as the combine kernel
        Lsum = Lsum + w[:, :, c] * lc[:, :, c]
        acc = acc + w[:, :, c, None] * oc[:, :, c]
    o = torch.where(Lsum[..., None] > 0, acc / Lsum.clamp_min(1e-37)[..., None], torch.zeros(()))
    if swap_heads:
        o = o.roll(1, dims=1)
    return o.reshape(B, H * D).to(BF)


# ---------------------------------------------------------------------------------------------
# RoPE (elementwise.hip rope8_k / rope_append8_k, the ROPE branch of attn_decode_k)
# ---------------------------------------------------------------------------------------------
THETA = 10000.0
ROPE_CASES = [(128, 4, 4), (128, 4, 2), (64, 3, 3)]  # (D, hq, hk)
ROPE_T = 40
# (start rows of the new token per batch row, kv_start per batch row): position = start - kv_start,
# as generate() numbers a left-padded batch
DECODE_ROPE_SETS = {
    "slots64": ((0, 63, 64), (0, 5, 3)),
    "slots2060": ((127, 2047, 2060), (0, 100, 2059)),
}


def rope_positions():
    """40 positions with 0 (twice), 1, 1087 and 4095 among them; neighbours differ"""
    g = _gen("rope-pos")
    pos = torch.randint(2, 4095, (ROPE_T,), generator=g)
    pos[0], pos[1], pos[2], pos[3], pos[20] = 0, 1, 1087, 4095, 0
    return pos


def rope_inputs(D, hq, hk):
    """q [T, hq*D] and k [T, hk*D]: column blocks of wider rows (CPU, bf16)"""
    g = _gen(f"rope-{D}-{hq}-{hk}")
    row = torch.randn(ROPE_T, (hq + 2 * hk) * D + 16, generator=g).to(BF)
    return row[:, :hq * D], row[:, hq * D:(hq + hk) * D], rope_positions()


def decode_rope_inputs(name, Lnew, H=ATTN_H, D=D_HEAD):
    """q | k | v column blocks of [B*Lnew, 3*H*D] rows, caches of max_len = max start + 70 rows of
    H*D + 64, start / kv_start int32 [B], position_ids int64 [B*Lnew] (CPU)"""
    starts, kvs = DECODE_ROPE_SETS[name]
    B = len(starts)
    max_len = max(starts) + 70
    g = _gen(f"decode-rope-{name}-{Lnew}")
    qkv = torch.randn(B * Lnew, 3 * H * D, generator=g).to(BF)
    kbuf = torch.randn(B, max_len, H * D + 64, generator=g).to(BF)
    vbuf = torch.randn(B, max_len, H * D + 64, generator=g).to(BF)
    start = torch.tensor(starts, dtype=torch.int32)
    kv_start = torch.tensor(kvs, dtype=torch.int32)
    pos = ((start - kv_start).long()[:, None] + torch.arange(Lnew)[None, :]).reshape(-1)
    return qkv, kbuf[:, :, :H * D], vbuf[:, :, :H * D], start, kv_start, pos, max_len


def _halves(x, D):
    xh = x.reshape(x.shape[0], -1, D)
    return xh[..., :D // 2], xh[..., D // 2:]


def rope_ref(x, pos, D, theta=THETA):
    """the exact half-split rotation in f64: pair (i, i + D/2) of every head turns by
    pos * theta^(-2i/D), cos and sin unrounded. x [T, nh*D], pos [T]."""
    x1, x2 = _halves(x.double(), D)
    i = torch.arange(D // 2, dtype=torch.float64, device=x.device)
    ang = pos.double()[:, None, None] * torch.pow(torch.tensor(theta, dtype=torch.float64), -2.0 * i / D)
    c, s = torch.cos(ang), torch.sin(ang)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(x.shape)


def rope_pair_abs(x, D):
    """|x1| + |x2| of each element's pair, in x's shape (f64)"""
    x1, x2 = _halves(x.double().abs(), D)
    return torch.cat([x1 + x2, x1 + x2], -1).reshape(x.shape)


def rope_gate(o, x, pos, D, theta=THETA, factor=4.0):
    """|o - ref| <= 4 U (|x1| + |x2|) per element of a pair (x1, x2) = x[i], x[i + D/2].

    o1 = bf16(bf16(x1 c') + bf16(-x2 s')) with c', s' = bf16(cosf / sinf(f32 angle)). With
    a = |x1| |c| + |x2| |s|: the rounded cos / sin move the exact result by at most U a, the two product
    roundings by U a, the rounding of the sum by U |o1| <= U a: 3 U a to first order, and
    a <= sqrt(x1^2 + x2^2) <= |x1| + |x2| since c^2 + s^2 = 1. The f32 angle is off by at most
    ~position * 2^-22 (the roundings of inv_freq and of the product: 1e-3 rad at position 4095), which
    turns the pair by 0.25 U (|x1| + |x2|). Together 3.25 U (|x1| + |x2|), gated at 4 U (|x1| + |x2|).
    At position 0 the angle is 0 exactly, c = 1, s = 0, and the output is the input bitwise.
    `factor` 8 gates the inverse of the forward against the input (the forward's error through a
    rotation, + the inverse's single rounding and (c^2 + s^2 - 1) |x| <= 2 U |x|).
    Returns worst err / gate."""
    return worst(o.double() - rope_ref(x, pos, D, theta), factor * U * rope_pair_abs(x, D))


def rope_honest(x, pos, D, theta=THETA, interleaved=False, flip_sin=False):
    """rope8_k restated in torch f32 at its rounding points. interleaved / flip_sin are mutants; the
    position mutants pass another pos."""
    xf = x.float()
    T = xf.shape[0]
    i = torch.arange(D // 2, dtype=torch.float32)
    inv_freq = 1.0 / torch.pow(torch.tensor(theta, dtype=torch.float32), (2 * i) / D)
    ang = pos.float()[:, None, None] * inv_freq
    c, s = bf(torch.cos(ang)), bf(torch.sin(ang))
    if flip_sin:
        s = -s
    xh = xf.reshape(T, -1, D)
    if interleaved:
        x1, x2 = xh[..., 0::2], xh[..., 1::2]
    else:
        x1, x2 = xh[..., :D // 2], xh[..., D // 2:]
    o1 = bf(bf(x1 * c) + bf(-x2 * s))
    o2 = bf(bf(x2 * c) + bf(x1 * s))
    if interleaved:
        o = torch.stack([o1, o2], -1).reshape(T, -1, D)
    else:
        o = torch.cat([o1, o2], -1)
    return o.reshape(x.shape).to(BF)


def rope_inverse_honest(y, pos, D, theta=THETA):
    """the inverse (transpose) rotation as rope8_k runs it: f32 products and sum, one bf16 rounding"""
    yf = y.float()
    T = yf.shape[0]
    i = torch.arange(D // 2, dtype=torch.float32)
    ang = pos.float()[:, None, None] * (1.0 / torch.pow(torch.tensor(theta, dtype=torch.float32), (2 * i) / D))
    c, s = bf(torch.cos(ang)), bf(torch.sin(ang))
    yh = yf.reshape(T, -1, D)
    y1, y2 = yh[..., :D // 2], yh[..., D // 2:]
    return torch.cat([y1 * c + y2 * s, y2 * c - y1 * s], -1).reshape(y.shape).to(BF)
