"""The gates of tests/decode_refs.py discriminate, shown on the CPU before any GPU time is spent.

For every input set of tests/test_decode_accuracy_gpu.py (same seeds, same shapes):
  * an honest restatement of the kernel (torch f32, summed in the kernel's order where that is
    cheap, rounded where the kernel rounds) stays inside the gate -- the worst err / gate is printed
    (pytest -s) -- and
  * each one-line mutant of that restatement (a dropped K tail, a window off by one, the wrong
    pairing, ...) violates it. A mutant is checked wherever it changes what is computed (row M-1 read
    as row 0 is no mutant at M = 1); where it does not, the test says so by name, nothing is skipped
    silently.
"""
import pytest
import torch

from tests import decode_refs as R

BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------
# GEMV
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", R.GEMV_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in R.GEMV_CASES])
def test_gemv_gate_passes_honest_and_fails_mutants(M, N, K):
    X, W, _, _, _ = R.gemv_inputs(M, N, K)
    ref, absprod = R.gemv_ref(X, W)
    waves = R.gemv_waves(N, K)
    w, rel = R.gemv_gate(R.gemv_honest(X, W, waves), ref, absprod, K)
    print(f"gemv {M}x{N}x{K}: honest err/gate {w:.3f}, rel-L2 {rel:.2e}")
    assert w <= 1.0 and rel <= 1e-5
    nk = -(-K // 32)
    mutants = {"tail8": dict(drop_tail8=True), "drop_step": dict(drop_step=nk // 2),
               "double_step": dict(double_step=nk // 2)}
    if M > 1:  # at M = 1 row M-1 is row 0
        mutants["row"] = dict(row_last_as_0=True)
    if N > 8:  # at N = 8 there is no row N-9
        mutants["n_clamp"] = dict(clamp_n_tail=True)
    assert ("row" in mutants) == ((M, N, K) != (1, 16, 32)) and ("n_clamp" in mutants) == ((M, N, K) != (2, 8, 64))
    for name, kw in mutants.items():
        assert not R.gemv_gate_ok(R.gemv_honest(X, W, waves, **kw), ref, absprod, K), f"mutant {name} passes the gate"


def test_epilogue_replay_rounds_where_store4_does():
    """v + bias in f32, then one bf16 rounding before each of addend and residual, one at the store"""
    c = torch.tensor([[1.0 + 2.0 ** -10, 3.0]])
    bias = torch.tensor([2.0 ** -9, 0.0]).to(BF)
    add = torch.tensor([[2.0 ** -8, 1.0]]).to(BF)
    res = torch.tensor([[-1.0, 0.5]]).to(BF)
    # expected: the same chain written out step by step
    out = R.epilogue_replay(c, bias, add, res)
    v = (c + bias.float()).to(BF).float() + add.float()
    v = v.to(BF).float() + res.float()
    assert torch.equal(out, v.to(BF))
    assert torch.equal(R.epilogue_replay(c), c.to(BF))
    # the bf16 rounding before the addend is visible: without it the first element differs
    unrounded = ((c + bias.float()) + add.float()).to(BF)
    assert not torch.equal(R.epilogue_replay(c, bias, add), unrounded)


@pytest.mark.parametrize("M,N,K", R.SWIGLU_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in R.SWIGLU_CASES])
def test_swiglu_gate_passes_honest_and_fails_mutants(M, N, K):
    X, W2, _, _, _ = R.gemv_inputs(M, 2 * N, K, name="swiglu")
    ref, absprod = R.gemv_ref(X, W2)
    d = K * 2.0 ** -24 * absprod
    g, up, dg, dup = ref[:, :N], ref[:, N:], d[:, :N], d[:, N:]
    waves = R.gemv_waves(2 * N, K)
    y = R.swiglu_honest(X, W2, waves)
    w = R.swiglu_gate(y, g, up, dg, dup)
    print(f"swiglu {M}x{N}x{K}: honest err/gate {w:.3f}")
    assert w <= 1.0
    # mutants: gate and up rows swapped; the last 8 K elements dropped
    swapped = R.swiglu_honest(X, torch.cat([W2[N:], W2[:N]]), waves)
    assert R.swiglu_gate(swapped, g, up, dg, dup) > 1.0
    Wt = W2.clone()
    Wt[:, K - 8:] = 0
    assert R.swiglu_gate(R.swiglu_honest(X, Wt, waves), g, up, dg, dup) > 1.0
    # up rows paired with the gate rows one 8-row block further on
    if N > 8:
        shifted = torch.cat([W2[:N], W2[N:].roll(8, 0)])
        assert R.swiglu_gate(R.swiglu_honest(X, shifted, waves), g, up, dg, dup) > 1.0


def test_swiglu_issue_form_rejects_honest():
    """The bound without a term for the bf16 rounding of the gate product is exceeded by the honest
    restatement (why swiglu_gate carries |silu'(g)| U |g| |up|)."""
    M, N, K = R.SWIGLU_CASES[1]
    X, W2, _, _, _ = R.gemv_inputs(M, 2 * N, K, name="swiglu")
    ref, absprod = R.gemv_ref(X, W2)
    d = K * 2.0 ** -24 * absprod
    w = R.swiglu_gate_issue_form(R.swiglu_honest(X, W2, R.gemv_waves(2 * N, K)), ref[:, :N], ref[:, N:], d[:, :N], d[:, N:])
    print(f"swiglu, bound without the g rounding: honest err/gate {w:.2f}")
    assert w > 1.0


# ---------------------------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------------------------
SCALE = R.D_HEAD ** -0.5


def _attn_case(name):
    max_len, pairs = R.ATTN_CASES[name]
    q, kc, vc = R.attn_inputs(name, max_len, len(pairs))
    lo = torch.tensor([p[0] for p in pairs], dtype=torch.int32)
    hi = torch.tensor([p[1] for p in pairs], dtype=torch.int32)
    return q, kc, vc, lo, hi, max_len, pairs


def _check_attn_mutants(q, kc, vc, lo, hi, max_len, label):
    ref, pv, n = R.decode_attn_ref(q, kc, vc, lo, hi, SCALE)
    honest = R.attn_honest(q, kc, vc, lo, hi, SCALE)
    rows, (_, zero_ok) = R.attn_gate_rows(honest, ref, pv, n), R.attn_gate(honest, ref, pv, n)
    print(f"attention {label}: honest err/gate {max(rows):.3f}")
    assert max(rows) <= 1.0 and zero_ok
    B = len(lo)
    vis = R.window(lo, hi, max_len)
    nonempty = (hi > lo)

    def must_fail(name, o, applies, somewhere=True):
        r = R.attn_gate_rows(o, ref, pv, n)
        assert bool(applies.any()) or not somewhere, f"{label}: mutant {name} applies to no row"
        for b in range(B):
            if applies[b]:
                assert r[b] > 1.0, f"{label}: mutant {name} passes the gate on row {b} ({r[b]:.3f})"

    # window shifted by one at either end, in both directions (wherever the key set changes)
    for name, dlo, dhi in (("lo+1", 1, 0), ("lo-1", -1, 0), ("hi-1", 0, -1), ("hi+1", 0, 1)):
        lo2, hi2 = (lo + dlo).clamp(0, max_len), (hi + dhi).clamp(0, max_len)
        applies = (R.window(lo2, hi2, max_len) != vis).any(1)
        if name in ("lo+1", "hi-1"):
            assert bool((applies == nonempty).all())
        # (no row below a window that starts at 0, none above one that ends at max_len)
        must_fail(name, R.attn_honest(q, kc, vc, lo2, hi2, SCALE), applies, somewhere=name in ("lo+1", "hi-1"))
    # the chunk that holds the window's middle key dropped
    mid = torch.where(nonempty, (lo + hi - 1) // 2 // R.CHUNK, torch.full_like(lo, -1))
    must_fail("drop_chunk", R.attn_honest(q, kc, vc, lo, hi, SCALE, drop_chunk=mid), nonempty)
    # chunks summed without exp2(m_c - M): a mutant where the window spans two chunks or more
    spans = nonempty & ((hi - 1) // R.CHUNK > lo // R.CHUNK)
    must_fail("no_rescale", R.attn_honest(q, kc, vc, lo, hi, SCALE, no_rescale=True), spans)
    must_fail("swap_heads", R.attn_honest(q, kc, vc, lo, hi, SCALE, swap_heads=True), nonempty)


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_gate_passes_honest_and_fails_mutants(name):
    q, kc, vc, lo, hi, max_len, _ = _attn_case(name)
    _check_attn_mutants(q, kc, vc, lo, hi, max_len, name)


@pytest.mark.parametrize("loc", R.PLANT_LOCS)
def test_planted_key_gate_and_value(loc):
    """the planted key (score ~45, v = 8): inside the window the honest output is 8 within U * 8 and
    an off-by-one that loses it fails both the gate and that; outside the output stays below 4 and an
    off-by-one that admits it fails both"""
    pairs = R.PLANT_PAIRS
    q, kc, vc = R.attn_inputs("plant-" + loc, R.PLANT_MAX_LEN, len(pairs))
    kc, vc = kc.clone(), vc.clone()
    rows = R.plant(q, kc, vc, pairs, loc)
    lo = torch.tensor([p[0] for p in pairs], dtype=torch.int32)
    hi = torch.tensor([p[1] for p in pairs], dtype=torch.int32)
    ref, pv, n = R.decode_attn_ref(q, kc, vc, lo, hi, SCALE)
    o = R.attn_honest(q, kc, vc, lo, hi, SCALE)
    r = R.attn_gate_rows(o, ref, pv, n)
    print(f"attention planted {loc}: honest err/gate {max(r):.3f}")
    assert max(r) <= 1.0
    inside = loc in ("first", "last")
    planted = [b for b, x in enumerate(rows) if x is not None]
    assert len(planted) >= 3
    # the mutant window: loses the planted key (inside) or admits it (outside)
    dlo, dhi = {"first": (1, 0), "last": (0, -1), "below": (-1, 0), "above": (0, 1)}[loc]
    om = R.attn_honest(q, kc, vc, lo + dlo, hi + dhi, SCALE)
    rm = R.attn_gate_rows(om, ref, pv, n)
    for b in planted:
        if inside:
            assert ((o[b].float() - 8.0).abs() <= R.U * 8).all()
            assert not ((om[b].float() - 8.0).abs() <= R.U * 8).all()
        else:
            assert (o[b].float().abs() < 4.0).all()
            assert not (om[b].float().abs() < 4.0).all()
        assert rm[b] > 1.0


# ---------------------------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------------------------
def _check_rope(x, pos, D, label, other_pos):
    w = R.rope_gate(R.rope_honest(x, pos, D), x, pos, D)
    print(f"rope {label}: honest err/gate {w:.3f}")
    assert w <= 1.0
    for name, o in (("interleaved", R.rope_honest(x, pos, D, interleaved=True)),
                    ("flip_sin", R.rope_honest(x, pos, D, flip_sin=True)),
                    ("pos+1", R.rope_honest(x, pos + 1, D)),
                    ("other_pos", R.rope_honest(x, other_pos, D))):
        changed = torch.ones(len(pos), dtype=torch.bool) if name != "other_pos" else other_pos != pos
        if name in ("interleaved", "flip_sin"):
            changed = pos != 0  # at position 0 the rotation is the identity whatever the pairing
        assert bool(changed.any()), f"{label}: mutant {name} applies to no row"
        for t in range(len(pos)):
            if changed[t]:
                r = R.rope_gate(o[t:t + 1], x[t:t + 1], pos[t:t + 1], D)
                assert r > 1.0, f"{label}: mutant {name} passes the gate on row {t} (position {int(pos[t])})"


@pytest.mark.parametrize("D,hq,hk", R.ROPE_CASES)
def test_rope_gate_passes_honest_and_fails_mutants(D, hq, hk):
    q, k, pos = R.rope_inputs(D, hq, hk)
    assert {0, 1, 1087, 4095} <= set(pos.tolist())
    for nm, x in (("q", q), ("k", k)):
        # "rotated with the other row's position": the neighbour's, as a kernel indexing positions wrongly
        _check_rope(x, pos, D, f"D{D} hq{hq} hk{hk} {nm}", pos.roll(1))
        y = R.rope_honest(x, pos, D)
        zero = pos == 0
        assert torch.equal(y[zero], x[zero])  # position 0: bitwise the input
        back = R.rope_inverse_honest(y, pos, D)
        wi = R.worst(back.double() - x.double(), 8 * R.U * R.rope_pair_abs(x, D))
        print(f"rope D{D} hq{hq} hk{hk} {nm}: inverse(forward) err/gate {wi:.3f}")
        assert wi <= 1.0


@pytest.mark.parametrize("Lnew", [1, 3])
@pytest.mark.parametrize("name", list(R.DECODE_ROPE_SETS))
def test_decode_rope_inputs_gate(name, Lnew):
    """the fused forms' inputs: the RoPE gate on the new q / k rows (the mutant "rotated with the
    key's position" uses the cache row, which differs from the position under left padding) and, for
    the attention that follows, the gate against the f64 reference given the rotated q"""
    H, D = R.ATTN_H, R.D_HEAD
    qkv, kc, vc, start, kv_start, pos, max_len = R.decode_rope_inputs(name, Lnew)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    slot = (start.long()[:, None] + torch.arange(Lnew)[None, :]).reshape(-1)
    assert bool((slot != pos).any())
    _check_rope(q, pos, D, f"{name} Lnew{Lnew} q", slot)
    _check_rope(k, pos, D, f"{name} Lnew{Lnew} k", slot)
    if Lnew != 1:
        return
    # attn_decode_rope: keys [kv_start, start], the new row's key rotated, its value copied
    kc, vc = kc.clone(), vc.clone()
    qr, kr = R.rope_honest(q, pos, D), R.rope_honest(k, pos, D)
    for b in range(len(start)):
        kc[b, int(start[b])] = kr[b]
        vc[b, int(start[b])] = v[b]
    o = R.attn_honest(qr, kc, vc, kv_start, start + 1, SCALE)
    ref, pv, n = R.decode_attn_ref(qr, kc, vc, kv_start, start + 1, SCALE)
    w, _ = R.attn_gate(o, ref, pv, n)
    print(f"attention after rope {name}: honest err/gate {w:.3f} given the kernel's rotated q")
    assert w <= 1.0
    # against the f64 rotation of q the same honest output is NOT inside the attention gate: the
    # bf16 roundings of the rotated q move every score by ~U, far above the f32 terms of the gate.
    # The GPU test therefore takes the rotated q from ops.rope (pinned to f64 by the RoPE gate, and
    # bitwise the fused kernel's rotation) and logs the figure against the f64 rotation ungated.
    ref64, pv64, _ = R.decode_attn_ref(R.rope_ref(q, pos, D), kc, vc, kv_start, start + 1, SCALE)
    w64, _ = R.attn_gate(o, ref64, pv64, n)
    print(f"attention after rope {name}: honest err/gate {w64:.2f} against the f64 rotation of q")
    if name == "slots2060":
        assert w64 > 1.0
