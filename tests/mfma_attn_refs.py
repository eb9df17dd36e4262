"""Case table, NaN-framed inputs, f64 reference, gates and honest restatement for the bf16 MFMA attention
forward that serving runs: attn_fwd_cached_k<128|64> and attn_fwd_ragged_k<128|64> (csrc/attention.hip, both
text includes of csrc/attn_fwd_pipe_body.h), and a handful of packed cases for attn_fwd_pipe_k / attn_fwd_k.
tests/test_mfma_attn_refs_host.py proves on the CPU that the gates pass an honest restatement of the kernel's
order on every case and fail each listed one-line mutant; tests/test_mfma_attn_accuracy_gpu.py holds the
kernels to the same gates on the same inputs. The f64 softmax-attention reference, rho and the LSE / zero
checks are tests/parity_refs.py's (attn_ref, _rho, lse_check); only the mask is this module's, because the
generic kernels' visibility() also restates their own 64-query block loop.

Reference: softmax over the live keys kv_start[b] <= j < kv_len[b], j <= past_b + i (past_b = kv_len[b] - Lq,
kv_len clamped to [0, rows of the slab]), for queries i >= q_pad[b]; a query without a live key has O = 0 and
LSE = +inf.

Gates (first order, from the rounding points of attn_fwd_pipe_body.h; U = 2^-8 one bf16 rounding, E = 2^-24
one f32 rounding; nothing here was taken from a kernel's output). For a query row with n live keys, scores
s_j, probabilities p_j = exp(s_j - lse):
 LSE  live rows within 1e-5 absolute (the project's gate); dead rows exactly +inf.
 O    U |ref| + sum_j p_j (U + 2 rho_j + (n + 2 tiles + 8) E) |v_j|, per element, no element excluded:
        U |ref|          the one bf16 rounding of o / l at the store;
        U p_j |v_j|      P is rounded to bf16 (round to nearest even, pack_frag's (__bf16) cast) before the
                         P V MFMA: each term of the numerator carries a relative error of at most U, while l
                         is summed from the unrounded P and carries none of it. A worst-case sum: random
                         roundings cancel, so an honest kernel sits well under 1 on random data (the host
                         test records where). The planted cases keep the gate honest: one key holds p near
                         1/2 with |v| = 3, so a mask edge off by one moves O by ~1.5, tens of times the gate;
        2 rho_j          parity_refs._rho, the relative error of one f32 probability (the exponent's argument
                         roundings and the D-term score chain), once for the numerator and once for l. The
                         kernel's exponent is exp2(fma(s, c, -m)) with c = scale log2 e and m the (possibly
                         stale, deferred-rescale) row maximum in log2 units: |m| exceeds |lse| log2 e by at
                         most thr + log2 n = 8 + 9 at these shapes, 17 E < 2^-19 more per probability, four
                         orders below the U term and inside rho's factor-2 slack on |s| and |lse| (log2 e <
                         2); the constants are therefore the issue's;
        (n + 2 tiles + 8) E   the f32 accumulation of P V over n keys, alpha and the fused l = fma(l, alpha,
                         rs) per tile, 1 / l, the product and slack.
 Shrink  |slope of (O - ref) on ref| <= U / 4 over a case's elements (see shrink()): rounding P to nearest is
      unbiased, truncating it is not, and no per-element bound can tell the two apart.
 Exact: O == 0 on dead queries (no live key, or i < q_pad[b]); every output element finite.
"""
import math

import torch

from tests import parity_refs as P
from tests.decode_refs import U, _gen, worst  # noqa: F401
from tests.train_refs import E, FLOOR

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
KT, QT, WAVE = 64, 128, 32       # keys per tile, queries per workgroup, queries per wave
THR = 8.0                        # g_rescale_thr as shipped (log2 units)
PAD_COLS = 16                    # NaN columns behind H * D in every cache slab
SPARE = 37                       # NaN rows behind the longest sequence
SENT = 777.0                     # the out= buffer's fill (exact in bf16)
PLANT_V = 3.0
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
HEADS = {128: 2, 64: 3}


# ---- cases ----------------------------------------------------------------------------------
def _case(name, kind, D, Lq, kv_len, ks, q_pad=None, cap=None, struct="random", plant=None, layout=False, why=""):
    B = len(kv_len)
    cap = cap if cap is not None else max(kv_len) + SPARE
    return dict(name=f"{name}-D{D}", kind=kind, D=D, H=HEADS[D], B=B, Lq=Lq, kv_len=tuple(kv_len),
                ks=None if ks is None else tuple(ks), q_pad=tuple(q_pad) if q_pad is not None else (0,) * B, cap=cap,
                Lk=cap, scale=D ** -0.5, struct=struct, plant=plant, layout=layout, why=why, dtype=BF)


def eff_len(c, b):
    """kv_len[b] as attn_fwd_ragged_k clamps it"""
    return min(max(c["kv_len"][b], 0), c["cap"])


PASTS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
PLANTS = ("ks", "ks-1", "mid", "mid+1", "edge", "edge+1", "last")


def _ks_values(past, Lq):
    return (0, 1, 63, 64, 65, past - 1, past, past + 1, past + Lq - 1, past + Lq)


def _cases(D):
    cs = []
    # cached: every (Lq, past); the B = 3 rows walk the ten kv_start values, so each Lq meets each value at least
    # twice over its nine cases (27 cases of 3 rows per head dim stand for the issue's ~40 of 2)
    for Lq in (2, 33, 130):
        for pi, past in enumerate(PASTS):
            vals = _ks_values(past, Lq)
            ks = [min(max(vals[(3 * pi + r) % 10], 0), past + Lq) for r in range(3)]
            cs.append(_case(f"cached-{Lq}-{past}", "cached", D, Lq, (past + Lq,) * 3, ks, layout=pi % 2 == 0,
                            why="kv_start, past and past + Lq either side of the 64-key tile edges; kv_start > past: "
                            "queries with no live key; kv_start = past + Lq: a sequence with nothing live"))
    # ragged: q_pad x (kv_len - Lq) x kv_start, three rows a case
    for Lq in (70, 130):
        pads = sorted({min(p, Lq) for p in (0, 1, 63, 64, 127, 128, 129, Lq)})
        offs = (-5, 0, 63, 64, 65, "zero", "over")
        starts = (0, 63, 64, 65, 1)
        cap = Lq + 65 + SPARE
        for n, pad in enumerate(pads):
            kl, ks, qp = [], [], []
            for r in range(3):
                off = offs[(3 * n + r) % len(offs)]
                kl.append(0 if off == "zero" else cap + 9 if off == "over" else Lq + off)
                # kv_len = 0 is a sequence of padding alone; otherwise the row keeps the case's q_pad, raised to
                # -past where the cache is shorter than the block (the documented kv_len >= Lq - q_pad)
                qp.append(Lq if off == "zero" else max(pad, 5 if off == -5 else 0))
                ks.append(starts[(2 * n + r) % len(starts)])
            cs.append(_case(f"ragged-{Lq}-p{pad}", "ragged", D, Lq, kl, ks, qp, cap=cap, layout=n % 2 == 1,
                            why="q_pad on the 64 / 128 edges and = Lq (whole query tiles that run no key tile), "
                            "kv_len - Lq negative, zero and around a tile edge, kv_len = 0 and above the slab (the "
                            "clamp), kv_start either side of the first tile's edge"))
        cs.append(_case(f"ragged-{Lq}-short", "ragged", D, Lq, (Lq - 5, Lq - 64, 3), (0, 1, 2), (0, 0, 0), cap=cap,
                        why="kv_len < Lq with no padding declared (outside the documented input): queries below "
                        "-past have no key at or below them and are dead rows"))
    cs.append(_case("ragged-uniform", "ragged", D, 130, (330, 330), (70, 129), (0, 0),
                    why="all rows uniform: bitwise the cached call"))
    # score structure at one cached and one ragged shape
    shapes = (("cached", dict(Lq=130, kv_len=(330, 330), ks=(70, 129))),
              ("ragged", dict(Lq=130, kv_len=(200, 150), ks=(70, 3), q_pad=(0, 64))))
    for kind, kw in shapes:
        cs.append(_case(f"{kind}-rising", kind, D, struct="rising", layout=True,
                        why="the row maximum rises by ~14 log2 units per tile: every tile rescales", **kw))
        for pl in PLANTS:
            cs.append(_case(f"{kind}-plant-{pl}", kind, D, struct="planted", plant=pl,
                            why="one key with p ~ 1/2 and v = 3 at a mask edge: a leaked or lost key moves O by ~1.5",
                            **kw))
    return cs


CASES = _cases(128) + _cases(64)
# packed cases for ops.attn_fwd at forward stages 7 and 4: kv_len = Lk, past = Lk - Lq = 0 when causal
PACKED = [dict(_case(f"packed-{L}{'c' if causal else ''}", "packed", D, L, (L, L), ks, cap=L), causal=causal)
          for D in (128, 64) for L, ks in ((65, (0, 3)), (131, (63, 65)), (200, (0, 129)))
          for causal in (True, False)]

# (dead queries, NaN key rows of the slabs) per case, written out from live_mask / poisoned_rows when the table
# was made: a typo that empties a case changes its counts
COUNTS = {
    "cached-2-0-D128": (3, 114), "cached-2-1-D128": (4, 117), "cached-2-63-D128": (2, 302),
    "cached-2-64-D128": (2, 178), "cached-2-65-D128": (0, 303), "cached-2-127-D128": (1, 492),
    "cached-2-128-D128": (3, 370), "cached-2-129-D128": (0, 239), "cached-2-200-D128": (0, 575),
    "cached-33-0-D128": (34, 145), "cached-33-1-D128": (66, 179), "cached-33-63-D128": (33, 333),
    "cached-33-64-D128": (33, 209), "cached-33-65-D128": (0, 303), "cached-33-127-D128": (1, 492),
    "cached-33-128-D128": (65, 432), "cached-33-129-D128": (0, 239), "cached-33-200-D128": (0, 575),
    "cached-130-0-D128": (64, 175), "cached-130-1-D128": (127, 240), "cached-130-63-D128": (130, 430),
    "cached-130-64-D128": (130, 306), "cached-130-65-D128": (0, 303), "cached-130-127-D128": (1, 492),
    "cached-130-128-D128": (259, 626), "cached-130-129-D128": (0, 239), "cached-130-200-D128": (0, 575),
    "ragged-70-p0-D128": (69, 375), "ragged-70-p1-D128": (72, 376), "ragged-70-p63-D128": (189, 273),
    "ragged-70-p64-D128": (192, 306), "ragged-70-p70-D128": (210, 280), "ragged-70-short-D128": (139, 445),
    "ragged-130-p0-D128": (69, 375), "ragged-130-p1-D128": (132, 436), "ragged-130-p63-D128": (189, 273),
    "ragged-130-p64-D128": (192, 306), "ragged-130-p127-D128": (384, 340), "ragged-130-p128-D128": (384, 306),
    "ragged-130-p129-D128": (388, 334), "ragged-130-p130-D128": (390, 312), "ragged-130-short-D128": (199, 505),
    "ragged-uniform-D128": (0, 273), "cached-rising-D128": (0, 273), "cached-plant-ks-D128": (0, 273),
    "cached-plant-ks-1-D128": (0, 273), "cached-plant-mid-D128": (0, 273), "cached-plant-mid+1-D128": (0, 273),
    "cached-plant-edge-D128": (0, 273), "cached-plant-edge+1-D128": (0, 273), "cached-plant-last-D128": (0, 273),
    "ragged-rising-D128": (64, 197), "ragged-plant-ks-D128": (64, 197), "ragged-plant-ks-1-D128": (64, 197),
    "ragged-plant-mid-D128": (64, 197), "ragged-plant-mid+1-D128": (64, 197), "ragged-plant-edge-D128": (64, 197),
    "ragged-plant-edge+1-D128": (64, 197), "ragged-plant-last-D128": (64, 197), "cached-2-0-D64": (3, 114),
    "cached-2-1-D64": (4, 117), "cached-2-63-D64": (2, 302), "cached-2-64-D64": (2, 178),
    "cached-2-65-D64": (0, 303), "cached-2-127-D64": (1, 492), "cached-2-128-D64": (3, 370),
    "cached-2-129-D64": (0, 239), "cached-2-200-D64": (0, 575), "cached-33-0-D64": (34, 145),
    "cached-33-1-D64": (66, 179), "cached-33-63-D64": (33, 333), "cached-33-64-D64": (33, 209),
    "cached-33-65-D64": (0, 303), "cached-33-127-D64": (1, 492), "cached-33-128-D64": (65, 432),
    "cached-33-129-D64": (0, 239), "cached-33-200-D64": (0, 575), "cached-130-0-D64": (64, 175),
    "cached-130-1-D64": (127, 240), "cached-130-63-D64": (130, 430), "cached-130-64-D64": (130, 306),
    "cached-130-65-D64": (0, 303), "cached-130-127-D64": (1, 492), "cached-130-128-D64": (259, 626),
    "cached-130-129-D64": (0, 239), "cached-130-200-D64": (0, 575), "ragged-70-p0-D64": (69, 375),
    "ragged-70-p1-D64": (72, 376), "ragged-70-p63-D64": (189, 273), "ragged-70-p64-D64": (192, 306),
    "ragged-70-p70-D64": (210, 280), "ragged-70-short-D64": (139, 445), "ragged-130-p0-D64": (69, 375),
    "ragged-130-p1-D64": (132, 436), "ragged-130-p63-D64": (189, 273), "ragged-130-p64-D64": (192, 306),
    "ragged-130-p127-D64": (384, 340), "ragged-130-p128-D64": (384, 306), "ragged-130-p129-D64": (388, 334),
    "ragged-130-p130-D64": (390, 312), "ragged-130-short-D64": (199, 505), "ragged-uniform-D64": (0, 273),
    "cached-rising-D64": (0, 273), "cached-plant-ks-D64": (0, 273), "cached-plant-ks-1-D64": (0, 273),
    "cached-plant-mid-D64": (0, 273), "cached-plant-mid+1-D64": (0, 273), "cached-plant-edge-D64": (0, 273),
    "cached-plant-edge+1-D64": (0, 273), "cached-plant-last-D64": (0, 273), "ragged-rising-D64": (64, 197),
    "ragged-plant-ks-D64": (64, 197), "ragged-plant-ks-1-D64": (64, 197), "ragged-plant-mid-D64": (64, 197),
    "ragged-plant-mid+1-D64": (64, 197), "ragged-plant-edge-D64": (64, 197), "ragged-plant-edge+1-D64": (64, 197),
    "ragged-plant-last-D64": (64, 197), "packed-65c-D128": (3, 3), "packed-65-D128": (0, 3),
    "packed-131c-D128": (128, 128), "packed-131-D128": (0, 128), "packed-200c-D128": (129, 129),
    "packed-200-D128": (0, 129), "packed-65c-D64": (3, 3), "packed-65-D64": (0, 3), "packed-131c-D64": (128, 128),
    "packed-131-D64": (0, 128), "packed-200c-D64": (129, 129), "packed-200-D64": (0, 129),
}


def plant_pos(c, b):
    kl, ks = eff_len(c, b), (c["ks"][b] if c["ks"] else 0)
    past, pl = kl - c["Lq"], c["plant"]
    if pl in ("ks", "ks-1"):
        return ks - (pl == "ks-1")
    if pl == "last":
        return kl - 1
    lo = past + max(c["q_pad"][b], 1)
    want = 30 if pl.startswith("mid") else 63
    p = next(x for x in range(lo, kl) if x % KT == want)
    return p + pl.endswith("+1")


# ---- reference ------------------------------------------------------------------------------
def live_mask(c, device="cpu"):
    """bool [B, Lq, cap]: the keys each query attends"""
    B, Lq, cap = c["B"], c["Lq"], c["cap"]
    i = torch.arange(Lq, device=device)[None, :, None]
    j = torch.arange(cap, device=device)[None, None, :]
    ks = torch.tensor(c["ks"] if c["ks"] else [0] * B, device=device)[:, None, None]
    kl = torch.tensor([eff_len(c, b) for b in range(B)], device=device)[:, None, None]
    qp = torch.tensor(c["q_pad"], device=device)[:, None, None]
    vis = (j >= ks) & (j < kl) & (i >= qp)
    if c["kind"] != "packed" or c["causal"]:
        vis = vis & (j <= kl - Lq + i)
    return vis.expand(B, Lq, cap).clone()


def poisoned_rows(c):
    """bool [B, cap]: the cache rows that hold NaN (below kv_start, at or above kv_len)"""
    j = torch.arange(c["cap"])[None]
    ks = torch.tensor(c["ks"] if c["ks"] else [0] * c["B"])[:, None]
    kl = torch.tensor([eff_len(c, b) for b in range(c["B"])])[:, None]
    return (j < ks) | (j >= kl)


def counts(c):
    return int((~live_mask(c).any(-1)).sum()), int(poisoned_rows(c).sum())


def ref(q, kc, vc, c):
    """parity_refs.attn_ref on the slabs (NaN rows are masked ones and count as 0)"""
    return P.attn_ref(torch.nan_to_num(q.double(), nan=0.0), kc, vc, c, live_mask(c, q.device))


def o_gate(r, c):
    tiles = -(-c["cap"] // KT)
    per_row = ((r["n"] + 2 * tiles + 8) * E)[:, None, :, None].double()
    w = r["P"] * (U + 2.0 * P._rho(r, c) + per_row)
    return U * r["O"].abs() + P._flat(w @ r["V"].abs()) + FLOOR


def figures(c, r, o, lse):
    """{gate: err / gate}; exact-zero, +inf and finiteness failures count as inf"""
    f = {"O": worst(o.double() - r["O"], o_gate(r, c))}
    err, bad_inf = P.lse_check(lse, r)
    f["LSE"] = float("inf") if bad_inf else (0.0 if err is None else err / 1e-5)
    f["lse_err"] = err
    dead = (~r["live"]).reshape(-1)
    f["zeros"] = float("inf") if bool((o[dead] != 0).any()) else 0.0
    f["finite"] = 0.0 if bool(torch.isfinite(o.float()).all()) else float("inf")
    f["shrink"] = abs(shrink(o, r)) / SHRINK_GATE
    return f


SHRINK_GATE = U / 4


def shrink(o, r):
    """the least-squares slope of o - ref on ref over all elements. A bound no per-element gate can give: P
    rounded to nearest carries zero-mean errors (and so does the store), so an honest o neither shrinks nor
    grows against ref beyond |slope| ~ U / sqrt(elements) < 2^-14 at the smallest case (1536 elements); P
    TRUNCATED to bf16 loses 0 .. 2^-7 of every probability, 0.72 * 2^-8 on average over a binade, while l is
    summed unrounded: o shrinks by that factor, three times the gate of U / 4."""
    ref = r["O"]
    den = float((ref * ref).sum())
    return float(((torch.nan_to_num(o.double()) - ref) * ref).sum()) / den if den > 0 else 0.0


# ---- inputs ---------------------------------------------------------------------------------
def inputs(c, device="cpu"):
    """dict q [B*Lq, H*D] (layout: the first column block of a NaN-filled q|k|v buffer), kc, vc [B, cap, H*D]
    (views of slabs [B, cap, H*D + 16] whose padding columns are NaN). Poison, all at once: K / V rows at or above
    kv_len[b] and below kv_start[b], q rows below q_pad[b], the padding columns. A planted key below kv_start
    stays finite (it is the key whose leak the case measures). Packed: k, v [B*Lk, H*D], nothing poisoned but
    the rows below kv_start. Seeded from the case name, built on the CPU, moved as whole buffers."""
    B, H, D, Lq, cap = c["B"], c["H"], c["D"], c["Lq"], c["cap"]
    hd = H * D
    g = _gen("mfma-attn-" + c["name"])
    q = torch.randn(B * Lq, hd, generator=g)
    k = torch.randn(B, cap, hd, generator=g)
    v = torch.randn(B, cap, hd, generator=g)
    u = torch.zeros(D)
    u[0] = 1.0
    if c["struct"] in ("rising", "planted"):  # every query shares a component along u: s_ij gains 2 k_j . u
        q = (q.view(B * Lq, H, D) + 2.0 * D ** 0.5 * u).view(B * Lq, hd)
    if c["struct"] == "rising":               # + 10 (14 in log2 units, above the threshold of 8) per 64-key tile,
        # centred on tile 3 so that |lse| stays near 20 (the 1e-5 LSE gate is absolute: ulp(32) = 3.8e-6)
        ramp = 5.0 * ((torch.arange(cap) // KT).float() - 3.0)
        k = (k.view(B, cap, H, D) + ramp[None, :, None, None] * u).view(B, cap, hd)
    keep = torch.zeros(B, cap, dtype=torch.bool)
    if c["struct"] == "planted":              # s = ln(n) + 2.5 against sum_others exp(s) ~ n exp(2.5): p ~ 1/2
        for b in range(B):
            pos = plant_pos(c, b)
            n = eff_len(c, b) - (c["ks"][b] if c["ks"] else 0)
            k[b, pos] = (0.5 * (math.log(n) + 2.5) * u).repeat(H)
            v[b, pos] = PLANT_V
            keep[b, pos] = True
    q, k, v = q.to(BF), k.to(BF), v.to(BF)
    bad = poisoned_rows(c) & ~keep
    if c["kind"] == "packed":  # the packed kernels promise nothing about rows below kv_start (tests/test_oob_guard.py)
        bad[:] = False
    k[bad] = NAN
    v[bad] = NAN
    for b in range(B):
        q[b * Lq:b * Lq + c["q_pad"][b]] = NAN
    d = {}
    if c["kind"] == "packed":
        d["kc"], d["vc"] = k.to(device), v.to(device)
        d["k"], d["v"] = d["kc"].view(B * cap, hd), d["vc"].view(B * cap, hd)
    else:
        for name, t in (("k", k), ("v", v)):
            slab = torch.full((B, cap, hd + PAD_COLS), NAN, dtype=BF)
            slab[:, :, :hd] = t
            d[name + "slab"] = slab.to(device)
            d[name + "c"] = d[name + "slab"][:, :, :hd]
    if c["layout"]:
        qbuf = torch.full((B * Lq, 3 * hd), NAN, dtype=BF)
        qbuf[:, :hd] = q
        d["qbuf"] = qbuf.to(device)
        d["q"] = d["qbuf"][:, :hd]
    else:
        d["q"] = q.to(device)
    return d


def out_block(c, device="cpu"):
    """(buffer, out= view): the middle column block of a sentinel-filled [B*Lq + 2, H*D + 16] buffer"""
    hd = c["H"] * c["D"]
    buf = torch.full((c["B"] * c["Lq"] + 2, hd + 16), SENT, dtype=BF, device=device)
    return buf, buf[1:-1, 8:8 + hd]


def frame_untouched(buf):
    return bool((buf[0] == SENT).all() and (buf[-1] == SENT).all() and (buf[:, :8] == SENT).all()
                and (buf[:, -8:] == SENT).all())


# ---- the honest restatement -----------------------------------------------------------------
MUTANTS = ("ks_m1", "diag_p1", "kvlen_m1", "qpad_m1", "past_p1", "past_m1", "t0_p1", "last_tile_dropped",
           "rescale_o_not_l", "l_from_rounded_p", "p_truncated", "v_row_shift", "v_batch_stride", "kvlen_unclamped",
           "zero_times_v")
# restated faithfully and computes, bit for bit, what the honest form computes on every case: a padding query's
# Q row only reaches its own column of S = K Q^T, and kspan = 0 masks that whole column by index before the row
# maximum is taken. "Loads no Q row" saves the fetch; the mask is what keeps the NaN out.
EQUIVALENT = ("pad_q_loaded",)


def _rows(cache, b, n, ntot, tok_is_batch=False):
    """[ntot, H*D] f32: rows 0 .. n-1 of sequence b read through the flat buffer (token stride cap rows when
    tok_is_batch), zeros behind them as the descriptor returns, NaN for a row outside the allocation"""
    B, cap, hd = cache.shape
    flat = cache.reshape(B * cap, hd).float()
    out = torch.zeros(ntot, hd)
    n = min(n, ntot)
    idx = b * cap + torch.arange(n) * (cap if tok_is_batch else 1)
    inb = idx < B * cap
    out[:n][inb] = flat[idx[inb]]
    out[:n][~inb] = NAN
    return out


def _exp2(x):
    return torch.exp2(x)


def fwd_honest(q, kc, vc, c, mutant=None, fixed=True):
    """attn_fwd_pipe_body.h (CACHED / RAGGED) in torch f32 on the CPU, in its order: per workgroup of 128 queries,
    64-key tiles from t0 = kv_start / 64 to ceil(kend / 64); f32 scores, the index mask, the tile maximum, the
    deferred rescale decided per wave of 32 queries (any lane's tile maximum above m + 8), P = exp2(fma(s, c,
    -m)), l = fma(l, alpha, sum of the unrounded P), P rounded to bf16 (nearest even), o += P V in f32, one bf16
    rounding of o / l, LSE = (m + log2 l) ln 2. V rows of the first tile below kv_start are zeros (fixed) or what
    the cache holds (the parent, mutant zero_times_v). Returns (o [B*Lq, H*D] bf16, lse [B, H, Lq] f32)."""
    B, H, D, Lq, cap = c["B"], c["H"], c["D"], c["Lq"], c["cap"]
    cc = (torch.tensor(c["scale"], dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    O = torch.zeros(B * Lq, H * D, dtype=BF)
    LSE = torch.full((B, H, Lq), float("inf"))
    nqb = -(-Lq // QT)
    for b in range(B):
        Lk = max(c["kv_len"][b], 0) if mutant == "kvlen_unclamped" else eff_len(c, b)
        qpad = min(max(c["q_pad"][b], 0), Lq)
        ks = c["ks"][b] if c["ks"] else 0
        past = Lk - Lq + (mutant == "past_p1") - (mutant == "past_m1")
        nrows = Lk                                   # where the descriptors end
        ntot = (-(-max(nrows, 1) // KT) + 1) * KT
        Kb = _rows(kc, b, nrows, ntot).view(ntot, H, D)
        Vb = _rows(vc, b, nrows, ntot, tok_is_batch=mutant == "v_batch_stride").view(ntot, H, D)
        ks_m = ks - (mutant == "ks_m1")
        for qb in range(nqb):
            qs = torch.arange(QT) + qb * QT
            padq = qs < qpad - (mutant == "qpad_m1")
            load = (qs < Lq) & (~padq if mutant != "pad_q_loaded" else torch.ones_like(padq))
            Qt = torch.zeros(QT, H, D)
            Qt[load] = q[b * Lq + qs[load]].float().view(-1, H, D)
            # (the diagonal already keeps every query below kv_len: the kv_len edge can only be wrong downwards)
            khi = torch.clamp(past + qs + 1 + (mutant == "diag_p1"), max=Lk - (mutant == "kvlen_m1"))
            kspan = torch.clamp(khi - ks_m, min=0)
            kspan[padq] = 0
            kend = min(Lk, past + qb * QT + QT)
            ntiles = 0 if qb * QT + QT <= qpad else -(-kend // KT)
            t0 = ks // KT + (mutant == "t0_p1")
            if mutant == "last_tile_dropped":
                ntiles -= 1
            m = torch.full((H, QT), float("-inf"))
            l = torch.zeros(H, QT)
            o = torch.zeros(H, QT, D)
            for t in range(t0, ntiles):
                j = torch.arange(KT) + t * KT
                s = torch.einsum("qhd,khd->hqk", Qt, Kb[j])
                live = (j[None] >= ks_m) & (j[None] < ks_m + kspan[:, None])
                s = torch.where(live[None], s, torch.full_like(s, float("-inf")))
                tmax = s.max(-1).values * cc
                grow = (tmax > m + THR).view(H, QT // WAVE, WAVE).any(-1, keepdim=True).expand(-1, -1, WAVE).reshape(H, QT)
                mnew = torch.where(grow, torch.maximum(m, tmax), m)
                muse = torch.where(mnew == float("-inf"), torch.zeros_like(m), mnew)
                alpha = torch.where(grow, _exp2(m - muse), torch.ones_like(m))
                o = o * alpha[..., None]
                p = _exp2((s.double() * cc - muse.double()[..., None]).float())
                if mutant == "p_truncated":
                    pb = (p.view(torch.int32) & -65536).view(F32)
                else:
                    pb = p.to(BF).float()
                rs = (pb if mutant == "l_from_rounded_p" else p).sum(-1)
                l = (l if mutant == "rescale_o_not_l" else l * alpha) + rs
                boundary = t == ks // KT and ks % KT != 0
                Vt = Vb[j + 1] if (mutant == "v_row_shift" and boundary) else Vb[j]
                if fixed and mutant != "zero_times_v":
                    Vt = torch.where((j < ks)[:, None, None], torch.zeros_like(Vt), Vt)
                o = o + torch.einsum("hqk,khd->hqd", pb, Vt)
                m = mnew
            inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
            lse = torch.where(l > 0, (m + torch.log2(l)) * LN2, torch.full_like(l, float("inf")))
            ok = qs < Lq
            O[b * Lq + qs[ok]] = (o * inv[..., None]).transpose(0, 1)[ok].reshape(-1, H * D).to(BF)
            LSE[b, :, qs[ok]] = lse[:, ok]
    return O, LSE
