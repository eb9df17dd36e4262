"""The decode step's kernels per element against float64: the weight-streaming product
(gemv.hip, plan tile 14 and cullavo_decode_linear), decode attention (decode.hip) and RoPE in its
three forms (ops.rope, ops.rope_kv_append, the ROPE branch of attn_decode_k).

References, gates (with their derivations) and input sets are tests/decode_refs.py;
tests/test_decode_refs_host.py shows on the CPU, for these very inputs, that an honest restatement
of each kernel passes its gate and that every listed mutant fails it. Everything goes through
ops.*; stats of every case are appended to the stats file of tests/test_accuracy_gpu.py, by its
own writer.
"""
import json

import pytest
import torch

from tests import decode_refs as R
from tests.test_accuracy_gpu import _log as _append_stats

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
SCALE = R.D_HEAD ** -0.5
H, D = R.ATTN_H, R.D_HEAD


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def _log(rec):
    print(json.dumps(rec))
    _append_stats(rec)


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------
# GEMV
# ---------------------------------------------------------------------------------------------
SENT = -7.0


def _framed(M, N, dtype):
    """C [M, N]: a view into a [M + 2, N + 8] buffer of sentinels (ldc = N + 8, a spare row either side)"""
    buf = torch.full((M + 2, N + 8), SENT, dtype=dtype, device=DEV)
    return buf, buf[1:M + 1, :N]


def _frame_untouched(buf, M, N):
    return bool((buf[0] == SENT).all() and (buf[M + 1] == SENT).all() and (buf[:, N:] == SENT).all())


@pytest.mark.parametrize("M,N,K", R.GEMV_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in R.GEMV_CASES])
def test_gemv_against_f64_and_epilogue_bitwise(M, N, K):
    from cullavo_amd import _lib
    assert _lib.lib().cullavo_gemm_plan(M, N, K, 0, 0, None) == 14
    X, W, bias, add, res = (t.to(DEV) for t in R.gemv_inputs(M, N, K))
    ref, absprod = R.gemv_ref(X, W)

    def run(dtype, **epi):
        buf, C = _framed(M, N, dtype)
        ops().gemm_ex(0, 0, M, N, K, X, K, W, K, C, N + 8, **epi)
        torch.cuda.synchronize()
        assert _frame_untouched(buf, M, N), "the product wrote outside its [M, N] view"
        return C

    c32 = run(torch.float32)
    w, rel = R.gemv_gate(c32, ref, absprod, K)
    fails = []
    if not (w <= 1.0 and rel <= 1e-5):
        fails.append(f"f32 output: err / (K 2^-24 |X||W|^T) {w:.3f}, rel-L2 {rel:.2e}")
    c16 = run(BF)
    nd = {"none": int((bits(c16) != bits(c32.to(BF))).sum())}
    epis = {"bias_addend": dict(bias=bias, addend=add, ld_addend=N),
            "residual": dict(residual=res, ldr=N),
            "all": dict(bias=bias, addend=add, ld_addend=N, residual=res, ldr=N)}
    for name, kw in epis.items():
        want = R.epilogue_replay(c32, kw.get("bias"), kw.get("addend"), kw.get("residual"))
        nd[name] = int((bits(run(BF, **kw)) != bits(want)).sum())
    # cullavo_decode_linear picks the same instantiation as the plan-14 dispatch: the same bits
    nd["decode_linear"] = int((bits(ops().decode_linear(X, W)) != bits(c16)).sum())
    nd["decode_linear_residual"] = int((bits(ops().decode_linear(X, W, residual=res))
                                        != bits(R.epilogue_replay(c32, None, None, res))).sum())
    _log({"test": "decode_gemv", "case": f"{M}x{N}x{K}", "err_over_f32_bound": w, "rel_l2_f32": rel,
          "bf16_bits_differing": nd})
    fails += [f"{k}: {v} bf16 outputs differ from the replayed epilogue of the f32 product" for k, v in nd.items() if v]
    assert not fails, f"gemv {M}x{N}x{K}: " + "; ".join(fails)


@pytest.mark.parametrize("M,N,K", R.SWIGLU_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in R.SWIGLU_CASES])
def test_decode_linear_swiglu_output_against_f64(M, N, K):
    X, W2, _, _, _ = (t.to(DEV) for t in R.gemv_inputs(M, 2 * N, K, name="swiglu"))
    ref, absprod = R.gemv_ref(X, W2)
    d = K * 2.0 ** -24 * absprod
    y = ops().decode_linear(X, W2, transform=3)
    torch.cuda.synchronize()
    assert y.shape == (M, N)
    w = R.swiglu_gate(y, ref[:, :N], ref[:, N:], d[:, :N], d[:, N:])
    _log({"test": "decode_swiglu", "case": f"{M}x{N}x{K}", "err_over_gate": w})
    assert w <= 1.0, f"swiglu {M}x{N}x{K}: err / gate {w:.3f}"


# ---------------------------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------------------------
def _attend(q, kc, vc, lo, hi, max_len):
    o = ops().attn_decode(q, kc, vc, hi, B=q.shape[0], H=H, D=D, max_len=max_len, scale=SCALE, kv_start=lo)
    torch.cuda.synchronize()
    return o


def _poison_pair(q, kc, vc, lo, hi, max_len, keep_rows=None):
    """the launch twice: cache rows outside [kv_start, kv_len) NaN in K and V, then zero. Returns the
    zero run's output and the failures."""
    vis = R.window(lo, hi, max_len)
    outs = []
    for value in (float("nan"), 0.0):
        k2, v2 = R.fill_outside(kc, vc, vis, value, keep_rows)
        # the caches stay views of rows H*D + 64 wide
        kb = torch.full((kc.shape[0], max_len, H * D + 64), value, dtype=BF, device=DEV)
        vb = torch.full_like(kb, value)
        kb[:, :, :H * D], vb[:, :, :H * D] = k2, v2
        outs.append(_attend(q, kb[:, :, :H * D], vb[:, :, :H * D], lo, hi, max_len))
    fails = []
    if not bool(torch.isfinite(outs[0].float()).all()):
        bad = (~torch.isfinite(outs[0].float())).any(1).nonzero().flatten().tolist()
        fails.append(f"NaN cache rows outside the window reach the output of batch rows {bad}")
    elif not same_bits(outs[0], outs[1]):
        fails.append("outputs differ between NaN and zero rows outside the window")
    return outs[1], fails


def _dev_case(q, kc, vc, pairs):
    lo = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=DEV)
    hi = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=DEV)
    qrow = torch.zeros(len(pairs), 3 * H * D, dtype=BF, device=DEV)
    qrow[:, H * D:2 * H * D] = q.to(DEV)
    return qrow[:, H * D:2 * H * D], kc.to(DEV), vc.to(DEV), lo, hi


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attn_decode_against_f64(name):
    max_len, pairs = R.ATTN_CASES[name]
    q, kc, vc, lo, hi = _dev_case(*R.attn_inputs(name, max_len, len(pairs)), pairs)
    assert q.stride(0) == 3 * H * D
    ref, pv, n = R.decode_attn_ref(q, kc, vc, lo, hi, SCALE)
    o, fails = _poison_pair(q, kc, vc, lo, hi, max_len)
    rows = R.attn_gate_rows(o, ref, pv, n)
    _, zero_ok = R.attn_gate(o, ref, pv, n)
    _log({"test": "decode_attention", "case": name, "max_len": max_len, "pairs": pairs, "err_over_gate_rows": rows,
          "err_over_gate": max(rows), "empty_rows_zero": zero_ok, "poison": fails})
    if not max(rows) <= 1.0:
        fails.append(f"err / gate per batch row {[round(r, 3) for r in rows]}")
    if not zero_ok:
        fails.append("a row with no visible key is not exactly 0")
    assert not fails, f"{name}: " + "; ".join(fails)


@pytest.mark.parametrize("loc", R.PLANT_LOCS)
def test_attn_decode_planted_key(loc):
    """k* = 4 q_h (score ~45 against N(0, 1)) with v* = 8 at the window's first / last row, or one row
    below / above it: inside, the output is 8 within U * 8; outside, it stays below 4. The poison
    fill spares the planted row, so a window off by one meets the planted key, not a NaN."""
    pairs, max_len = R.PLANT_PAIRS, R.PLANT_MAX_LEN
    qc, kcc, vcc = R.attn_inputs("plant-" + loc, max_len, len(pairs))
    kcc, vcc = kcc.clone(), vcc.clone()
    planted = R.plant(qc, kcc, vcc, pairs, loc)
    q, kc, vc, lo, hi = _dev_case(qc, kcc, vcc, pairs)
    ref, pv, n = R.decode_attn_ref(q, kc, vc, lo, hi, SCALE)
    o, fails = _poison_pair(q, kc, vc, lo, hi, max_len, keep_rows=planted)
    rows = R.attn_gate_rows(o, ref, pv, n)
    inside = loc in ("first", "last")
    worst8 = 0.0
    for b, r in enumerate(planted):
        if r is None:
            continue
        if inside:
            d8 = (o[b].float() - 8.0).abs().max().item()
            worst8 = max(worst8, d8)
            if not d8 <= R.U * 8:
                fails.append(f"row {b} {pairs[b]}: planted key at {r} inside the window, output off 8.0 by {d8:.3f}")
        else:
            mx = o[b].float().abs().max().item()
            worst8 = max(worst8, mx)
            if not mx < 4.0:
                fails.append(f"row {b} {pairs[b]}: planted key at {r} outside the window, |output| {mx:.3f}")
    _log({"test": "decode_attention_planted", "case": loc, "err_over_gate": max(rows),
          "worst_off_8" if inside else "worst_abs_output": worst8, "poison": fails})
    if not max(rows) <= 1.0:
        fails.append(f"err / gate per batch row {[round(r, 3) for r in rows]}")
    assert not fails, f"planted {loc}: " + "; ".join(fails)


# ---------------------------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D_,hq,hk", R.ROPE_CASES)
def test_rope_against_f64(D_, hq, hk):
    q0, k0, pos = R.rope_inputs(D_, hq, hk)
    row = torch.zeros(R.ROPE_T, (hq + 2 * hk) * D_ + 16, dtype=BF, device=DEV)
    q, k = row[:, :hq * D_], row[:, hq * D_:(hq + hk) * D_]
    q.copy_(q0)
    k.copy_(k0)
    q0, k0, pos = q0.to(DEV), k0.to(DEV), pos.to(DEV)
    ops().rope(q, k, pos, hq=hq, hk=hk, head_dim=D_, theta=R.THETA)
    torch.cuda.synchronize()
    zero = pos == 0
    assert int(zero.sum()) >= 2
    wq, wk = R.rope_gate(q, q0, pos, D_), R.rope_gate(k, k0, pos, D_)
    fails = []
    if not (wq <= 1.0 and wk <= 1.0):
        fails.append(f"err / gate q {wq:.3f}, k {wk:.3f}")
    if not (same_bits(q[zero], q0[zero]) and same_bits(k[zero], k0[zero])):
        fails.append("position 0 is not bitwise the input")
    if not bool((row[:, (hq + hk) * D_:] == 0).all()):
        fails.append("columns beside q | k were written")
    ops().rope(q, k, pos, hq=hq, hk=hk, head_dim=D_, theta=R.THETA, inverse=True)
    torch.cuda.synchronize()
    wi = max(R.worst(x.double() - x0.double(), 8 * R.U * R.rope_pair_abs(x0, D_)) for x, x0 in ((q, q0), (k, k0)))
    if not wi <= 1.0:
        fails.append(f"inverse(forward) err / gate {wi:.3f}")
    _log({"test": "decode_rope", "case": f"D{D_}_hq{hq}_hk{hk}", "err_over_gate_q": wq, "err_over_gate_k": wk,
          "inverse_err_over_gate": wi})
    assert not fails, f"rope D{D_} hq{hq} hk{hk}: " + "; ".join(fails)


def _decode_rope_case(name, Lnew):
    qkv, kc, vc, start, kv_start, pos, max_len = R.decode_rope_inputs(name, Lnew)
    B = len(start)
    # free cache rows hold NaN, as a torch.empty cache may: everything outside [kv_start, start)
    vis = R.window(kv_start, start, max_len)
    kc, vc = R.fill_outside(kc, vc, vis, float("nan"))
    kb = torch.full((B, max_len, H * D + 64), float("nan"), dtype=BF, device=DEV)
    vb = torch.full_like(kb, float("nan"))
    kb[:, :, :H * D], vb[:, :, :H * D] = kc.to(DEV), vc.to(DEV)
    qkv = qkv.to(DEV)
    return (qkv, qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:], kb, vb, start.to(DEV),
            kv_start.to(DEV), pos.to(DEV), max_len, B)


def _check_new_rows(kb, vb, kb0, vb0, k, v, start, pos, Lnew, B, fails):
    """the rotated key rows against f64, the value rows bitwise, everything else in the buffers
    untouched. Returns the worst RoPE err / gate of the key rows."""
    new = torch.zeros(kb.shape[:2], dtype=torch.bool, device=DEV)
    wk = 0.0
    for b in range(B):
        s = int(start[b])
        new[b, s:s + Lnew] = True
        rows = slice(b * Lnew, (b + 1) * Lnew)
        wk = max(wk, R.rope_gate(kb[b, s:s + Lnew, :H * D], k[rows], pos[rows], D))
        if not same_bits(vb[b, s:s + Lnew, :H * D], v[rows]):
            fails.append(f"value rows of batch row {b} are not bitwise the input")
        zero = pos[rows] == 0
        if bool(zero.any()) and not same_bits(kb[b, s:s + Lnew, :H * D][zero], k[rows][zero]):
            fails.append(f"key row at position 0 (batch row {b}) is not bitwise the input")
    if not wk <= 1.0:
        fails.append(f"rotated key rows: err / gate {wk:.3f}")
    pad = torch.zeros(kb.shape[2], dtype=torch.bool, device=DEV)
    pad[H * D:] = True
    other = ~new[:, :, None] | pad[None, None, :]
    if not (torch.equal(bits(kb)[other], bits(kb0)[other]) and torch.equal(bits(vb)[other], bits(vb0)[other])):
        fails.append("cache elements outside the new rows changed")
    return wk


@pytest.mark.parametrize("Lnew", [1, 3])
@pytest.mark.parametrize("name", list(R.DECODE_ROPE_SETS))
def test_rope_kv_append_against_f64(name, Lnew):
    qkv, q, k, v, kb, vb, start, kv_start, pos, max_len, B = _decode_rope_case(name, Lnew)
    qkv0, kb0, vb0 = qkv.clone(), kb.clone(), vb.clone()
    q0 = qkv0[:, :H * D]
    ops().rope_kv_append(q, k, v, pos, kb[:, :, :H * D], vb[:, :, :H * D], start, hq=H, head_dim=D, theta=R.THETA,
                         B=B, Lnew=Lnew)
    torch.cuda.synchronize()
    fails = []
    wk = _check_new_rows(kb, vb, kb0, vb0, k, v, start, pos, Lnew, B, fails)
    wq = R.rope_gate(q, q0, pos, D)
    if not wq <= 1.0:
        fails.append(f"rotated q: err / gate {wq:.3f}")
    if not same_bits(qkv[:, H * D:], qkv0[:, H * D:]):
        fails.append("k / v inputs changed")
    _log({"test": "decode_rope_kv_append", "case": f"{name}_Lnew{Lnew}", "err_over_gate_q": wq, "err_over_gate_k": wk})
    assert not fails, f"rope_kv_append {name} Lnew {Lnew}: " + "; ".join(fails)


@pytest.mark.parametrize("name", list(R.DECODE_ROPE_SETS))
def test_attn_decode_rope_against_f64(name):
    """The attention output is gated against the f64 softmax given q as the kernel rotates it: that
    rotation is ops.rope's (bitwise, tests/test_generation.py), which test_rope_against_f64 pins to
    f64. Against the unrounded f64 rotation of q no correct kernel meets the attention gate (the bf16
    roundings of the rotated q move every score by ~U, tests/test_decode_refs_host.py measures 30-70x
    the gate for the honest restatement); that figure is logged, not gated."""
    qkv, q, k, v, kb, vb, start, kv_start, pos, max_len, B = _decode_rope_case(name, 1)
    qkv0, kb0, vb0 = qkv.clone(), kb.clone(), vb.clone()
    o = ops().attn_decode_rope(q, k, v, pos, kb[:, :, :H * D], vb[:, :, :H * D], start, B=B, H=H, D=D,
                               max_len=max_len, scale=SCALE, theta=R.THETA, kv_start=kv_start)
    torch.cuda.synchronize()
    fails = []
    if not same_bits(qkv, qkv0):
        fails.append("q / k / v inputs changed")
    wk = _check_new_rows(kb, vb, kb0, vb0, k, v, start, pos, 1, B, fails)
    qr = q.clone()
    ops().rope(qr, None, pos, hq=H, hk=0, head_dim=D, theta=R.THETA)
    torch.cuda.synchronize()
    wq = R.rope_gate(qr, q, pos, D)
    if not wq <= 1.0:
        fails.append(f"rotated q: err / gate {wq:.3f}")
    kc, vc = kb[:, :, :H * D], vb[:, :, :H * D]  # the cache as the kernel left it
    ref, pv, n = R.decode_attn_ref(qr, kc, vc, kv_start, start + 1, SCALE)
    rows = R.attn_gate_rows(o, ref, pv, n)
    if not bool(torch.isfinite(o.float()).all()):
        fails.append("NaN rows outside the window reach the output")
    if not max(rows) <= 1.0:
        fails.append(f"attention err / gate per batch row {[round(r, 3) for r in rows]}")
    ref64, pv64, _ = R.decode_attn_ref(R.rope_ref(q, pos, D), kc, vc, kv_start, start + 1, SCALE)
    w64, _ = R.attn_gate(o, ref64, pv64, n)
    _log({"test": "decode_attn_rope", "case": name, "max_len": max_len, "err_over_gate": max(rows),
          "err_over_gate_rows": rows, "err_over_gate_k": wk, "err_over_gate_q": wq,
          "err_over_gate_vs_f64_rotated_q_ungated": w64})
    assert not fails, f"attn_decode_rope {name}: " + "; ".join(fails)
