"""cullavo_attn_fwd_varlen / cullavo_attn_bwd_varlen: causal attention over sequences of unequal
length packed back to back (ops.attn_fwd_varlen / ops.attn_bwd_varlen).

The varlen kernels are further instantiations of the uniform kernels' bodies: only a workgroup's base
rows, its length and the lse / delta row stride change. So for every sequence b the results are
compared BIT FOR BIT with ops.attn_fwd / ops.attn_bwd at B = 1, L = seq_len[b], causal, on that
sequence's rows alone (same tiles, same summation order), which tests/test_accuracy_gpu.py,
tests/test_attention_masks_gpu.py and tests/test_oob_guard.py pin. On top of that:
  independence  everything sequence b does not own (gap rows, the other sequences' rows, lse / delta
                entries at or beyond seq_len[b]) is NaN: b's results keep their bits and are finite;
                rows outside every sequence keep the sentinel they were framed with;
  f64           one case against tests/parity_refs.attn_ref / bwd_ref per sequence at the gates of
                tests/test_accuracy_gpu.py (LSE 1e-5 absolute, rel-L2 3e-3, element-wise 2^-3 of
                |ref| + row rms);
  errors        argument errors return a code and cullavo_last_error() before anything is launched.
q | k | v and dq | dk | dv are column blocks of one [T, 3 H D] buffer, as the decoder layer holds them.
"""
import functools

import pytest
import torch

from tests import parity_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
SENTINEL = 0x7B7B  # bf16 bits of the frames around every output (a finite value no kernel produces here by chance)

HEADS = [(128, 2), (64, 3)]  # (D, H)
LENGTHS = [(1, 63, 64, 65, 130), (200, 0, 7, 129), (64, 64), (131,)]
GAPS = [0, 3, 70]


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int16)


def layout(lens, gap):
    """sequence b at rows start[b] .. start[b] + lens[b] - 1 with `gap` free rows in front of every
    sequence and behind the last one"""
    start, row = [], 0
    for n in lens:
        row += gap
        start.append(row)
        row += n
    return start, row + gap


@functools.lru_cache(maxsize=None)
def problem(D, H, lens, gap):
    """inputs, the varlen results in sentinel frames and the per-sequence uniform results (computed once,
    shared by the tests, never modified)"""
    start, T = layout(lens, gap)
    hd = H * D
    g = torch.Generator(device=DEV).manual_seed(1000 * D + 10 * len(lens) + gap)
    qkv = torch.randn(T, 3 * hd, device=DEV, generator=g).to(BF)
    do = torch.randn(T, hd, device=DEV, generator=g).to(BF)
    ss = torch.tensor(start, dtype=torch.int32, device=DEV)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    p = dict(D=D, H=H, lens=lens, start=start, T=T, qkv=qkv, do=do, ss=ss, sl=sl, max_len=max(lens),
             scale=D ** -0.5)
    p["o"], p["lse"], p["dqkv"] = run_varlen(p, qkv, do)
    ref = []
    for s, n in zip(start, lens):
        if n == 0:
            ref.append(None)
            continue
        q, k, v = (qkv[s:s + n, i * hd:(i + 1) * hd] for i in range(3))
        o, lse = ops().attn_fwd(q, k, v, B=1, H=H, Lq=n, Lk=n, D=D, scale=p["scale"], causal=True)
        dq, dk, dv = ops().attn_bwd(q, k, v, o, do[s:s + n], lse, B=1, H=H, Lq=n, Lk=n, D=D, scale=p["scale"],
                                    causal=True)
        ref.append(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv))
    torch.cuda.synchronize()
    p["ref"] = ref
    return p


def run_varlen(p, qkv, do, o_in=None, lse_fill=None):
    """forward + backward through the varlen entry points, every output inside a sentinel frame. o_in /
    lse_fill: the independence runs hand the backward an o with NaN rows and pre-fill lse / delta."""
    D, H, T, hd = p["D"], p["H"], p["T"], p["H"] * p["D"]
    B, ml = len(p["lens"]), p["max_len"]
    kw = dict(B=B, H=H, max_len=ml, D=D, scale=p["scale"])
    q, k, v = (qkv[:, i * hd:(i + 1) * hd] for i in range(3))
    o = torch.full((T, hd), SENTINEL, dtype=torch.int16, device=DEV).view(BF)
    lse = torch.full((B, H, ml), float("nan") if lse_fill is None else lse_fill, dtype=torch.float32, device=DEV)
    ops().attn_fwd_varlen(q, k, v, p["ss"], p["sl"], out=o, lse=lse, **kw)
    o_bwd = o
    if o_in is not None:  # b's rows as computed, everything else NaN
        o_bwd = o_in(o)
    dqkv = torch.full((T, 3 * hd), SENTINEL, dtype=torch.int16, device=DEV).view(BF)
    delta = torch.full((B, H, ml), float("nan"), dtype=torch.float32, device=DEV)
    ops().attn_bwd_varlen(q, k, v, o_bwd, do, lse, p["ss"], p["sl"], dq=dqkv[:, :hd], dk=dqkv[:, hd:2 * hd],
                          dv=dqkv[:, 2 * hd:], delta=delta, **kw)
    torch.cuda.synchronize()
    return o, lse, dqkv


def free_rows(p):
    keep = torch.ones(p["T"], dtype=torch.bool, device=DEV)
    for s, n in zip(p["start"], p["lens"]):
        keep[s:s + n] = False
    return keep


CASES = [(D, H, lens, gap) for D, H in HEADS for lens in LENGTHS for gap in GAPS]
IDS = [f"d{D}h{H}-{'_'.join(map(str, lens))}-gap{gap}" for D, H, lens, gap in CASES]


@pytest.mark.parametrize("D,H,lens,gap", CASES, ids=IDS)
def test_bitwise_per_sequence(D, H, lens, gap):
    p = problem(D, H, lens, gap)
    hd = H * D
    bad = []
    for b, (s, n) in enumerate(zip(p["start"], lens)):
        r = p["ref"][b]
        if r is None:
            continue
        got = dict(o=p["o"][s:s + n], dq=p["dqkv"][s:s + n, :hd], dk=p["dqkv"][s:s + n, hd:2 * hd],
                   dv=p["dqkv"][s:s + n, 2 * hd:])
        for nm, t in got.items():
            assert torch.isfinite(t.float()).all(), f"sequence {b} {nm}: not finite"
            if not torch.equal(bits(t), bits(r[nm])):
                bad.append(f"sequence {b} (len {n}) {nm}: {(bits(t) != bits(r[nm])).sum().item()} elements differ")
        if not torch.equal(p["lse"][b, :, :n].contiguous().view(torch.int32), r["lse"][0].contiguous().view(torch.int32)):
            bad.append(f"sequence {b} (len {n}) lse differs")
        # lse entries at or beyond the sequence's length are not written (the NaN they were framed with)
        assert torch.isnan(p["lse"][b, :, n:]).all(), f"sequence {b}: lse written beyond its length"
    assert not bad, "; ".join(bad)
    # rows outside every sequence: untouched
    fr = free_rows(p)
    assert (bits(p["o"])[fr] == SENTINEL).all(), "o: a row outside every sequence was written"
    assert (bits(p["dqkv"])[fr] == SENTINEL).all(), "dq | dk | dv: a row outside every sequence was written"


@pytest.mark.parametrize("D,H,lens,gap", CASES, ids=IDS)
def test_independence(D, H, lens, gap):
    p = problem(D, H, lens, gap)
    hd = H * D
    nan = float("nan")
    fr = free_rows(p)
    for b, (s, n) in enumerate(zip(p["start"], lens)):
        if n == 0:
            continue
        mine = torch.zeros(p["T"], dtype=torch.bool, device=DEV)
        mine[s:s + n] = True
        qkv = torch.where(mine[:, None], p["qkv"], torch.full_like(p["qkv"], nan))
        do = torch.where(mine[:, None], p["do"], torch.full_like(p["do"], nan))
        o, lse, dqkv = run_varlen(p, qkv, do, o_in=lambda o_: torch.where(mine[:, None], o_, torch.full_like(o_, nan)),
                                  lse_fill=nan)
        for nm, t, ref in (("o", o, p["o"]), ("dq|dk|dv", dqkv, p["dqkv"])):
            assert torch.isfinite(t[s:s + n].float()).all(), f"sequence {b} {nm}: not finite beside NaN neighbours"
            assert torch.equal(bits(t[s:s + n]), bits(ref[s:s + n])), f"sequence {b} {nm}: bits moved with its neighbours"
            assert (bits(t)[fr] == SENTINEL).all(), f"{nm}: a row outside every sequence was written"
        assert torch.isfinite(lse[b, :, :n]).all()
        assert torch.equal(lse[b, :, :n].contiguous().view(torch.int32), p["lse"][b, :, :n].contiguous().view(torch.int32))
        assert torch.isnan(lse[b, :, n:]).all()


def test_against_f64():
    """the f64 reference is computed per sequence; the gates of tests/test_accuracy_gpu.py are then taken
    over the packed tensors (all live rows), as that test takes them over its whole batch"""
    D, H, lens = 128, 2, (130, 65, 1)
    p = problem(D, H, lens, 3)
    hd = H * D
    fails = []
    got = {nm: [] for nm in ("O", "dQ", "dK", "dV")}
    want = {nm: [] for nm in got}
    for b, (s, n) in enumerate(zip(p["start"], lens)):
        c = dict(B=1, Lq=n, Lk=n, D=D, scale=p["scale"], causal=True, kind="packed", ks=None, dtype=BF)
        q, k, v = (p["qkv"][s:s + n, i * hd:(i + 1) * hd] for i in range(3))
        o = p["o"][s:s + n]
        lse = p["lse"][b:b + 1, :, :n]
        r = R.attn_ref(q, k.reshape(1, n, hd), v.reshape(1, n, hd), c, R.visibility(c, device=DEV))
        g = R.bwd_ref(r, c, p["do"][s:s + n], o, lse)
        lse_err = (lse.double() - r["LSE"]).abs().max().item()
        print(f"sequence {b} (len {n}): lse max|err| {lse_err:.2e}")
        if not lse_err <= 1e-5:
            fails.append(f"sequence {b} lse max|err| {lse_err:.2e}")
        for nm, out, ref in (("O", o, r["O"]), ("dQ", p["dqkv"][s:s + n, :hd], g["dQ"]),
                             ("dK", p["dqkv"][s:s + n, hd:2 * hd], g["dK"]), ("dV", p["dqkv"][s:s + n, 2 * hd:], g["dV"])):
            got[nm].append(out.double())
            want[nm].append(ref)
    for nm in got:
        out, ref = torch.cat(got[nm]), torch.cat(want[nm])
        err = out - ref
        rel = (err.norm() / ref.norm()).item()
        row_rms = ref.view(-1, H, D).pow(2).mean(-1, keepdim=True).sqrt().expand(-1, H, D).reshape(ref.shape)
        floor = 1e-3 * ref.pow(2).mean().sqrt()  # rows whose exact value is 0 (dQ of a sequence's first query)
        worst = (err.abs() / (ref.abs() + row_rms + floor)).max().item()
        print(f"{nm}: rel-L2 {rel:.2e}, max |err| / (|ref| + row rms) {worst:.2e}")
        if not rel <= 3e-3:
            fails.append(f"{nm} rel-L2 {rel:.2e}")
        if not worst <= 2 ** -3:
            fails.append(f"{nm} max |err| / (|ref| + row rms) {worst:.2e}")
    assert not fails, "; ".join(fails)


def _last_error():
    from cullavo_amd._lib import lib
    return lib().cullavo_last_error().decode()


def test_argument_errors():
    """each returns an error code with a message and launches nothing: the outputs keep their frames"""
    from cullavo_amd._lib import lib
    D, H, lens = 64, 3, (7, 40)
    p = problem(D, H, lens, 3)
    hd, T, B = H * D, p["T"], len(lens)
    q, k, v = (p["qkv"][:, i * hd:(i + 1) * hd] for i in range(3))
    base = dict(B=B, H=H, max_len=p["max_len"], D=D, scale=p["scale"])

    def framed():
        o = torch.full((T, hd), SENTINEL, dtype=torch.int16, device=DEV).view(BF)
        lse = torch.full((B, H, 64), float("nan"), dtype=torch.float32, device=DEV)
        return o, lse

    def raw_fwd(o, lse, *, ss=p["ss"], sl=p["sl"], ldq=q.stride(0), max_len=p["max_len"], D_=D):
        return lib().cullavo_attn_fwd_varlen(q.data_ptr(), ldq, k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                             o.data_ptr(), o.stride(0), lse.data_ptr(),
                                             None if ss is None else ss.data_ptr(), None if sl is None else sl.data_ptr(),
                                             B, H, max_len, D_, p["scale"], ops()._dt(q),
                                             torch.cuda.current_stream().cuda_stream)

    def expect(rc, word):
        msg = _last_error()
        assert rc != 0 and word in msg, f"rc {rc}, message {msg!r}"
        torch.cuda.synchronize()

    # D outside {64, 128}
    o, lse = framed()
    expect(raw_fwd(o, lse, D_=32), "head_dim")
    assert (bits(o) == SENTINEL).all() and torch.isnan(lse).all()
    # a null seq_len
    expect(raw_fwd(o, lse, sl=None), "null")
    assert (bits(o) == SENTINEL).all() and torch.isnan(lse).all()
    # a token stride that is no multiple of 8
    expect(raw_fwd(o, lse, ldq=q.stride(0) + 4), "multiples of 8")
    assert (bits(o) == SENTINEL).all() and torch.isnan(lse).all()
    # max_len below a length: seq_len lives on the device, so the entry points see it only with the
    # read-back check switched on (cullavo_attn_varlen_set_check; off by default: it synchronises)
    prev = lib().cullavo_attn_varlen_set_check(1)
    try:
        expect(raw_fwd(o, lse, max_len=max(lens) - 1), "max_len")
        assert (bits(o) == SENTINEL).all() and torch.isnan(lse).all()
        dqkv = torch.full((T, 3 * hd), SENTINEL, dtype=torch.int16, device=DEV).view(BF)
        with pytest.raises(ValueError, match="max_len"):
            ops().attn_bwd_varlen(q, k, v, p["o"], p["do"], p["lse"][:, :, :max(lens) - 1].contiguous(), p["ss"], p["sl"],
                                  dq=dqkv[:, :hd], dk=dqkv[:, hd:2 * hd], dv=dqkv[:, 2 * hd:],
                                  **dict(base, max_len=max(lens) - 1))
        torch.cuda.synchronize()
        assert (bits(dqkv) == SENTINEL).all()
    finally:
        lib().cullavo_attn_varlen_set_check(prev)
    # the same errors through ops (ValueError / CullavoError carrying cullavo_last_error())
    with pytest.raises(Exception, match="head_dim"):
        ops().attn_fwd_varlen(q[:, :H * 32], k[:, :H * 32], v[:, :H * 32], p["ss"], p["sl"], **dict(base, D=32))
    with pytest.raises(ValueError, match="seq_len"):
        ops().attn_fwd_varlen(q, k, v, p["ss"], p["sl"][:1], **base)


def test_length_above_max_len_is_clamped_by_default():
    """the read-back check is off by default: a length above max_len is then no error. The kernels clamp it
    to max_len, so the sequence is computed as its first max_len rows (bitwise the uniform kernels at that
    length) and nothing outside those rows, the [B, H, max_len] lse / delta or the frames is written."""
    from cullavo_amd._lib import lib
    D, H, n, ml, gap = 128, 2, 100, 70, 3
    hd, T = H * D, n + 2 * gap
    assert lib().cullavo_attn_varlen_set_check(0) == 0  # (and leaves it off)
    g = torch.Generator(device=DEV).manual_seed(5)
    qkv = torch.randn(T, 3 * hd, device=DEV, generator=g).to(BF)
    do = torch.randn(T, hd, device=DEV, generator=g).to(BF)
    q, k, v = (qkv[:, i * hd:(i + 1) * hd] for i in range(3))
    ss = torch.tensor([gap], dtype=torch.int32, device=DEV)
    sl = torch.tensor([n], dtype=torch.int32, device=DEV)
    kw = dict(B=1, H=H, max_len=ml, D=D, scale=D ** -0.5)
    o = torch.full((T, hd), SENTINEL, dtype=torch.int16, device=DEV).view(BF)
    # lse / delta inside larger NaN frames: the [1, H, ml] block the kernels may touch is the front of each
    frame_l = torch.full((2, H, ml), float("nan"), dtype=torch.float32, device=DEV)
    frame_d = torch.full((2, H, ml), float("nan"), dtype=torch.float32, device=DEV)
    ops().attn_fwd_varlen(q, k, v, ss, sl, out=o, lse=frame_l[:1], **kw)
    dqkv = torch.full((T, 3 * hd), SENTINEL, dtype=torch.int16, device=DEV).view(BF)
    ops().attn_bwd_varlen(q, k, v, o, do, frame_l[:1], ss, sl, dq=dqkv[:, :hd], dk=dqkv[:, hd:2 * hd],
                          dv=dqkv[:, 2 * hd:], delta=frame_d[:1], **kw)
    torch.cuda.synchronize()
    s = slice(gap, gap + ml)
    ro, rl = ops().attn_fwd(q[s], k[s], v[s], B=1, H=H, Lq=ml, Lk=ml, D=D, scale=kw["scale"], causal=True)
    rq, rk, rv = ops().attn_bwd(q[s], k[s], v[s], ro, do[s], rl, B=1, H=H, Lq=ml, Lk=ml, D=D, scale=kw["scale"], causal=True)
    assert torch.equal(bits(o[s]), bits(ro)) and torch.equal(frame_l[:1], rl)
    for got, ref in ((dqkv[s, :hd], rq), (dqkv[s, hd:2 * hd], rk), (dqkv[s, 2 * hd:], rv)):
        assert torch.equal(bits(got), bits(ref))
    outside = torch.ones(T, dtype=torch.bool, device=DEV)
    outside[s] = False
    assert (bits(o)[outside] == SENTINEL).all() and (bits(dqkv)[outside] == SENTINEL).all()
    assert torch.isnan(frame_l[1]).all() and torch.isnan(frame_d[1]).all() and torch.isfinite(frame_d[0]).all()
