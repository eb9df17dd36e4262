"""Ragged KV cache: batched follow-up turns of unequal length (cullavo_attn_fwd_ragged /
ops.attn_fwd_ragged, cullavo_kv_append_ragged / ops.kv_append_ragged, generation.KVCache.lengths,
the ragged branch of generation.lm_infer, DecodeGraph(live=True), generate(compact_cache=True)).
Reference: HF's cached forward on a left-padded generation batch, whose masked slots are skipped
by position_ids = cumsum(mask) - 1 (cullavo/arch_cullavo.py:605-636); the compact cache attends the
same keys at the same positions without storing a masked one.

Kernel: tests/test_cached_prefill.py::attn_cached_ref restated in f64 with a per-sequence kv_len /
q_pad, at that file's gates (O rel-L2 <= 3e-3, max |err| / (|ref| + row rms + 1e-3 rms) <= 2^-3, LSE
max|err| <= 1e-5 and > 0 and finite over live queries). Cache rows >= kv_len[b] are NaN in K and V.
Padding and other dead queries are exactly zero rows with lse = +inf, and their number is asserted:
per case 1, 33, 129, 7, 48, 130, 31, 31 (the q_pad rows; no live query of these cases starts below
its kv_start). On the CPU the f64 restatement against a plain f32 torch restatement of the same
inputs measured, over CASES: O rel-L2 6.6e-8 .. 4.5e-7, max row-scaled error 1.3e-7 .. 2.1e-6, LSE
max|err| 8.5e-8 .. 5.6e-7 (each > 0): the gates are met by arithmetic alone and no comparison is empty
(test_reference_against_f32_restatement repeats that measurement on the CPU).

Model: tiny_gpu() on oracle.make_weights(config_small_gpu(), 6), as tests/test_cached_prefill.py;
gates rel-L2 <= 1e-2 ("same arithmetic, different kernels") and <= 3e-2 against the oracle. A
left-padded PREFILL keeps its padding rows in the cache (kv_start, as before this feature), so a
row's `lengths[b] - kv_start[b]` is what equals the solo conversation's `length`.
"""
import ctypes
import functools
import importlib.util
import os

import pytest
import torch

from oracle import cullavo_oracle as O

BF = torch.bfloat16
DEV = "cuda"


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ---------------------------------------------------------------------------------------------
# kernel against float64
# ---------------------------------------------------------------------------------------------
# (B, H, Lq, D, kv_len before the call, n_new, kv_start, dtype): each for an edge of the 128-query /
# 64-key / 32-rows-per-wave tiling
CASES = [
    (2, 2, 2, 128, (1, 3), (2, 1), None, BF),                # the smallest ragged call
    (2, 2, 40, 128, (63, 64), (40, 7), None, BF),            # pad 33; prefix ends either side of a key-tile edge
    (2, 2, 130, 128, (200, 90), (130, 1), (0, 70), BF),      # query tile 0 of seq 1 all padding, kv_len - Lq < 0
    (3, 2, 5, 128, (64, 10, 67), (5, 0, 3), (0, 0, 67), BF),  # nothing new; live queries start at kv_start
    (2, 2, 64, 128, (1088, 1000), (64, 16), None, BF),       # config-3 prefix, two tile counts in one launch
    (2, 3, 200, 64, (5, 300), (200, 70), None, BF),          # the D = 64 kernel
    (2, 2, 40, 32, (24, 3), (40, 9), None, BF),              # the generic kernel: bf16, small head dim
    (2, 2, 40, 128, (24, 3), (40, 9), None, torch.float32),  # the generic kernel: f32 storage
]
DEAD = [1, 33, 129, 7, 48, 130, 31, 31]  # padding + other dead queries per case
PAD_ROWS = 37  # free cache rows behind the longest sequence, NaN (as every row >= kv_len[b])


def case_lengths(case):
    B, H, Lq, D, before, n_new, kv_start, dtype = case
    kv_len = [a + n for a, n in zip(before, n_new)]
    q_pad = [Lq - n for n in n_new]
    return kv_len, q_pad


def make_case(case, seed=23):
    """(q [B*Lq, H*D], k_cache, v_cache [B, max kv_len + 37, H*D], rows >= kv_len[b] NaN), CPU tensors"""
    B, H, Lq, D, before, n_new, kv_start, dtype = case
    kv_len, _ = case_lengths(case)
    g = torch.Generator().manual_seed(seed)
    rows, hd = max(kv_len) + PAD_ROWS, H * D
    q = torch.randn(B * Lq, hd, generator=g).to(dtype)
    kc = torch.randn(B, rows, hd, generator=g).to(dtype)
    vc = torch.randn(B, rows, hd, generator=g).to(dtype)
    for b in range(B):
        kc[b, kv_len[b]:] = float("nan")
        vc[b, kv_len[b]:] = float("nan")
    return q, kc, vc


def attn_ragged_ref(q, kc, vc, B, H, Lq, D, scale, kv_len, q_pad, kv_start, dt=torch.float64):
    """attn_cached_ref with a per-sequence prefix: query i >= q_pad[b] sits at cache row kv_len[b] - Lq
    + i and attends keys kv_start[b] <= j <= that row; in dtype dt. Returns (O [B*Lq, H*D], lse
    [B, H, Lq], dead [B, Lq]: padding and queries with no visible key, O = 0 there)."""
    rows = kc.shape[1]
    dev = q.device
    Q = q.to(dt).view(B, Lq, H, D).transpose(1, 2)
    K = torch.nan_to_num(kc.to(dt), nan=0.0).view(B, rows, H, D).transpose(1, 2)  # free rows: masked below
    V = torch.nan_to_num(vc.to(dt), nan=0.0).view(B, rows, H, D).transpose(1, 2)
    S = (Q @ K.transpose(-1, -2)) * scale  # [B, H, Lq, rows]
    i = torch.arange(Lq, device=dev)[None, :, None]
    j = torch.arange(rows, device=dev)[None, None, :]
    kl = torch.tensor(kv_len, device=dev)[:, None, None]
    qp = torch.tensor(q_pad, device=dev)[:, None, None]
    ks = torch.tensor(kv_start if kv_start is not None else [0] * B, device=dev)[:, None, None]
    vis = (i >= qp) & (j <= kl - Lq + i) & (j >= ks) & (j < kl)  # [B, Lq, rows]
    dead = ~vis.any(-1)
    S = S.masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse.masked_fill(dead[:, None], 0.0)[..., None])  # dead rows: exp(-inf) = 0
    Oh = P @ V
    return Oh.transpose(1, 2).reshape(B * Lq, H * D), lse, dead


def expected_dead(case):
    """the count from q_pad and kv_start alone: the padding rows, and the live queries whose cache
    row lies below kv_start"""
    B, H, Lq, D, before, n_new, kv_start, dtype = case
    kv_len, q_pad = case_lengths(case)
    ks = kv_start if kv_start is not None else [0] * B
    return sum(q_pad[b] + sum(1 for i in range(q_pad[b], Lq) if kv_len[b] - Lq + i < ks[b]) for b in range(B))


def gate_figures(o, lse, O_ref, LSE_ref, dead, B, H, Lq, D):
    live = ~dead[:, None].expand(B, H, Lq)
    lse_err = (lse.double() - LSE_ref)[live].abs().max().item()
    err = o.double() - O_ref
    rel = (err.norm() / O_ref.norm()).item()
    row_rms = O_ref.view(-1, H, D).pow(2).mean(-1, keepdim=True).sqrt().expand(-1, H, D).reshape(O_ref.shape)
    floor = 1e-3 * O_ref.pow(2).mean().sqrt()
    worst = (err.abs() / (O_ref.abs() + row_rms + floor)).max().item()
    return rel, worst, lse_err


@functools.lru_cache(maxsize=None)
def _case(idx):
    """(inputs on the GPU, f64 reference) of CASES[idx]: built once, shared, never modified"""
    B, H, Lq, D, before, n_new, kv_start, dtype = CASES[idx]
    kv_len, q_pad = case_lengths(CASES[idx])
    q, kc, vc = (t.to(DEV) for t in make_case(CASES[idx]))
    return (q, kc, vc), attn_ragged_ref(q, kc, vc, B, H, Lq, D, D ** -0.5, kv_len, q_pad, kv_start)


def _ids():
    return [f"B{c[0]}H{c[1]}Lq{c[2]}D{c[3]}{'ks' if c[6] else ''}{'f32' if c[7] != BF else ''}" for c in CASES]


def test_reference_against_f32_restatement():
    """CPU: the f64 reference against the same statements in f32 on the same inputs meets the gates
    by arithmetic alone, and the dead-query counts are the recorded ones."""
    for idx, case in enumerate(CASES):
        B, H, Lq, D, before, n_new, kv_start, dtype = case
        kv_len, q_pad = case_lengths(case)
        q, kc, vc = make_case(case)
        O64, L64, dead = attn_ragged_ref(q, kc, vc, B, H, Lq, D, D ** -0.5, kv_len, q_pad, kv_start)
        O32, L32, dead32 = attn_ragged_ref(q, kc, vc, B, H, Lq, D, D ** -0.5, kv_len, q_pad, kv_start, dt=torch.float32)
        assert torch.equal(dead, dead32)
        assert int(dead.sum()) == DEAD[idx] == expected_dead(case), (idx, int(dead.sum()))
        assert (O64[dead.reshape(-1)] == 0).all() and torch.isinf(L64[dead[:, None].expand(B, H, Lq)]).all()
        rel, worst, lse_err = gate_figures(O32, L32, O64, L64, dead, B, H, Lq, D)
        print(f"case {idx}: O rel-L2 {rel:.3e}, max row-scaled {worst:.3e}, lse max|err| {lse_err:.3e}")
        assert 0.0 < lse_err <= 1e-5 and rel <= 3e-3 and worst <= 2 ** -3


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=_ids())
def test_attn_fwd_ragged_against_f64(idx):
    B, H, Lq, D, before, n_new, kv_start, dtype = CASES[idx]
    kv_len, q_pad = case_lengths(CASES[idx])
    (q, kc, vc), (O_ref, LSE_ref, dead) = _case(idx)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)  # noqa: E731
    o, lse = ops().attn_fwd_ragged(q, kc, vc, i32(kv_len), B=B, H=H, Lq=Lq, D=D, scale=D ** -0.5, q_pad=i32(q_pad),
                                   kv_start=i32(kv_start) if kv_start is not None else None)
    torch.cuda.synchronize()
    assert o.shape == (B * Lq, H * D) and lse.shape == (B, H, Lq)
    assert torch.isfinite(o).all(), "a free (NaN) cache row reached the output"
    dead_rows = dead.reshape(B * Lq)
    assert int(dead_rows.sum()) == DEAD[idx] == expected_dead(CASES[idx])
    assert (o[dead_rows] == 0).all(), "padding and dead queries must return a zero row"
    dead_h = dead[:, None].expand(B, H, Lq)
    assert (lse[dead_h] == float("inf")).all(), "padding and dead queries must return lse = +inf"
    assert torch.isfinite(lse[~dead_h]).all()
    rel, worst, lse_err = gate_figures(o, lse, O_ref, LSE_ref, dead, B, H, Lq, D)
    print(f"case {idx}: O rel-L2 {rel:.3e}, max row-scaled {worst:.3e}, lse max|err| {lse_err:.3e}")
    assert 0.0 < lse_err < float("inf"), f"lse max|err| {lse_err}: the comparison is broken"
    assert lse_err <= 1e-5, f"lse max|err| {lse_err:.2e}"
    assert rel <= 3e-3, f"O rel-L2 {rel:.2e}"
    assert worst <= 2 ** -3, f"O max |err| / (|ref| + row rms) {worst:.2e}"


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,Lq,past,D", [(2, 2, 130, 200, 128), (1, 3, 200, 5, 64)])
def test_uniform_lengths_are_the_cached_kernel(B, H, Lq, past, D):
    """q_pad = 0 and kv_len = past + Lq for every sequence: O and LSE bitwise ops.attn_fwd_cached's"""
    case = (B, H, Lq, D, (past,) * B, (Lq,) * B, None, BF)
    q, kc, vc = (t.to(DEV) for t in make_case(case, seed=29))
    o0, lse0 = ops().attn_fwd_cached(q, kc, vc, B=B, H=H, Lq=Lq, past=past, D=D, scale=D ** -0.5)
    kv_len = torch.full((B,), past + Lq, dtype=torch.int32, device=DEV)
    o1, lse1 = ops().attn_fwd_ragged(q, kc, vc, kv_len, B=B, H=H, Lq=Lq, D=D, scale=D ** -0.5,
                                     q_pad=torch.zeros(B, dtype=torch.int32, device=DEV))
    o2, lse2 = ops().attn_fwd_ragged(q, kc, vc, kv_len, B=B, H=H, Lq=Lq, D=D, scale=D ** -0.5)  # q_pad null
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
    assert torch.equal(o0, o2) and torch.equal(lse0, lse2)


@pytest.mark.gpu
def test_kv_append_ragged_exact():
    """the live rows land bitwise at start + t - q_pad, every other cache row keeps the sentinel (the
    q_pad[b] rows below start[b] included, which cullavo_kv_append would overwrite); q_pad = 0 is
    ops.kv_append bit for bit"""
    B, Lnew, hd, Lmax = 3, 5, 256, 80
    start, q_pad = (7, 0, 64), (0, 5, 2)
    g = torch.Generator().manual_seed(3)
    k = torch.randn(B * Lnew, hd, generator=g).to(BF).to(DEV)
    v = torch.randn(B * Lnew, hd, generator=g).to(BF).to(DEV)
    sentinel = 1234.0
    kc = torch.full((B, Lmax, hd), sentinel, dtype=BF, device=DEV)
    vc = torch.full((B, Lmax, hd), sentinel, dtype=BF, device=DEV)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)  # noqa: E731
    ops().kv_append_ragged(k, v, kc, vc, i32(start), i32(q_pad), B=B, Lnew=Lnew)
    torch.cuda.synchronize()
    ek = torch.full_like(kc, sentinel)
    ev = torch.full_like(vc, sentinel)
    written = 0
    for b in range(B):
        for t in range(q_pad[b], Lnew):
            ek[b, start[b] + t - q_pad[b]] = k[b * Lnew + t]
            ev[b, start[b] + t - q_pad[b]] = v[b * Lnew + t]
            written += 1
    assert written == 8
    assert torch.equal(kc, ek) and torch.equal(vc, ev)
    ka, va = torch.full_like(kc, sentinel), torch.full_like(vc, sentinel)
    kb, vb = torch.full_like(kc, sentinel), torch.full_like(vc, sentinel)
    ops().kv_append(k, v, ka, va, i32(start), B=B, Lnew=Lnew)
    ops().kv_append_ragged(k, v, kb, vb, i32(start), i32((0, 0, 0)), B=B, Lnew=Lnew)
    assert torch.equal(ka, kb) and torch.equal(va, vb)
    assert not torch.equal(ka, kc)


# ---------------------------------------------------------------------------------------------
# host side (no GPU): argument checks, the header, the built kernels' LDS reads, the bookkeeping
# ---------------------------------------------------------------------------------------------
def test_ragged_entry_points_are_declared_and_bound():
    from cullavo_amd import _lib
    decls = _lib.declarations()
    assert [n for _, n in decls["cullavo_attn_fwd_ragged"][1]] == [
        "q", "ldq", "k_cache", "v_cache", "ld_tok", "ld_batch", "o", "ldo", "lse", "B", "H", "Lq", "kv_len", "q_pad",
        "D", "scale", "kv_start", "dtype", "stream"]
    assert [n for _, n in decls["cullavo_kv_append_ragged"][1]] == [
        "k", "ldk", "v", "ldv", "k_cache", "v_cache", "ld_tok", "ld_batch", "start", "q_pad", "B", "Lnew", "hd",
        "stream"]
    L = _lib.lib()
    assert L.cullavo_attn_fwd_ragged.argtypes is not None and len(L.cullavo_attn_fwd_ragged.argtypes) == 19
    assert len(L.cullavo_kv_append_ragged.argtypes) == 14
    assert L.cullavo_abi_version() == _lib.abi_version()  # pure additions: the header's rule asks for no bump
    from cullavo_amd import ops as _ops
    assert callable(_ops.attn_fwd_ragged) and callable(_ops.kv_append_ragged)


def test_ragged_argument_checks():
    """every documented argument error returns CULLAVO_EINVAL (ValueError) or EUNSUPPORTED with a message
    before anything is launched (the data pointers are null: a launch would fault)"""
    from cullavo_amd import _lib
    hd = 256
    host = (ctypes.c_int32 * 4)(0, 0, 0, 0)  # a non-null kv_len / start / q_pad that is never dereferenced
    p = ctypes.addressof(host)
    # (q, ldq, k_cache, v_cache, ld_tok, ld_batch, o, ldo, lse, B, H, Lq, kv_len, q_pad, D, scale, kv_start, dtype, stream)
    with pytest.raises(ValueError, match="kv_len"):
        _lib.call("attn_fwd_ragged", None, hd, None, None, hd, 64 * hd, None, hd, None, 2, 2, 4, None, None, 128, 1.0,
                  None, 1, None)
    with pytest.raises(ValueError, match="Lq must be at least 1"):
        _lib.call("attn_fwd_ragged", None, hd, None, None, hd, 64 * hd, None, hd, None, 2, 2, 0, p, None, 128, 1.0,
                  None, 1, None)
    with pytest.raises(ValueError, match="batch stride is smaller"):
        _lib.call("attn_fwd_ragged", None, hd, None, None, hd, hd - 8, None, hd, None, 2, 2, 4, p, None, 128, 1.0,
                  None, 1, None)
    with pytest.raises(ValueError, match="token stride smaller than H\\*D"):
        _lib.call("attn_fwd_ragged", None, hd - 8, None, None, hd, 64 * hd, None, hd, None, 2, 2, 4, p, None, 128,
                  1.0, None, 1, None)
    with pytest.raises(Exception, match="head_dim must be 16, 32, 64 or 128"):
        _lib.call("attn_fwd_ragged", None, 192, None, None, 192, 64 * 192, None, 192, None, 1, 2, 4, p, None, 96, 1.0,
                  None, 1, None)
    with pytest.raises(Exception, match="bf16 / f32"):
        _lib.call("attn_fwd_ragged", None, hd, None, None, hd, 64 * hd, None, hd, None, 2, 2, 4, p, None, 128, 1.0,
                  None, 7, None)
    # (k, ldk, v, ldv, k_cache, v_cache, ld_tok, ld_batch, start, q_pad, B, Lnew, hd, stream)
    with pytest.raises(ValueError, match="start positions"):
        _lib.call("kv_append_ragged", None, hd, None, hd, None, None, hd, 64 * hd, None, p, 2, 3, hd, None)
    with pytest.raises(ValueError, match="q_pad"):
        _lib.call("kv_append_ragged", None, hd, None, hd, None, None, hd, 64 * hd, p, None, 2, 3, hd, None)
    with pytest.raises(ValueError, match="multiples of 8"):
        _lib.call("kv_append_ragged", None, hd, None, hd, None, None, hd + 4, 64 * hd, p, p, 2, 3, hd, None)


def test_ragged_kernel_lds_reads_not_used_before_their_wait():
    """attn_fwd_ragged_k shares the pipelined forward's inline-asm LDS reads with deferred counted
    waits: the scan tests/test_cached_prefill.py runs on attn_fwd_cached_k, on the new symbols."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_isa_lds_reads.py")
    spec = importlib.util.spec_from_file_location("_isa_lds_reads", path)
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    if not (os.path.exists(isa.LIB) and os.path.exists(isa.OBJDUMP)):
        pytest.skip("library or llvm-objdump missing")
    kernels = isa._kernels()
    names = ("attn_fwd_ragged_kILi128EE", "attn_fwd_ragged_kILi64EE")
    checked = isa._listed(kernels, names)
    assert len(checked) == 2, checked
    problems = {n: bad[:3] for n in checked if (bad := isa._early_uses([ins for _, ins in kernels[n]]))}
    assert not problems, problems


def test_kvcache_ragged_bookkeeping():
    from cullavo_amd.generation import KVCache
    c = KVCache(2, 3, 16, 2, 4, "cpu", dtype=torch.float32)
    assert c.lengths is None
    c.length = 10
    c.kv_start = torch.tensor([0, 4, 0], dtype=torch.int32)
    c.next_pos = torch.tensor([10, 6, 10])
    assert torch.equal(c.key_mask(), (torch.arange(10)[None] >= c.kv_start[:, None]))
    c.k.copy_(torch.arange(c.k.numel(), dtype=torch.float32).view_as(c.k))
    c.v.copy_(-c.k)
    c.advance_ragged(torch.tensor([3, 0, 7]))  # a ragged step: n_new = Lq - q_pad
    assert c.lengths.dtype == torch.int32 and c.lengths.tolist() == [13, 10, 17]
    assert c.length == 17 == c.get_seq_length() and c.next_pos.tolist() == [13, 6, 17]
    m = c.key_mask()
    assert m.shape == (3, 17) and m.sum(-1).tolist() == [13, 6, 17]
    assert not m[1, :4].any() and m[1, 4:10].all() and not m[1, 10:].any()
    k_old, v_old = c.k.clone(), c.v.clone()
    c.k[:, :, 16:].fill_(5.0)  # (max_len 16 < length 17 cannot happen on a real cache: grow first)
    c.length, c.lengths = 16, torch.tensor([13, 10, 16], dtype=torch.int32)
    c.grow(40)
    assert c.max_len == 40 and c.k.shape == (2, 3, 40, 8) and c.lengths.tolist() == [13, 10, 16]
    assert torch.equal(c.k[:, :, :16], k_old[:, :, :16]) and torch.equal(c.v[:, :, :16], v_old[:, :, :16])
    k, v = c[1]
    assert k.shape == (3, 2, 16, 4) and len(c.to_legacy_cache()) == 2  # rows [:length], as a uniform cache


def test_new_chunk_mask_classifier():
    from cullavo_amd.generation import new_chunk_padding
    assert new_chunk_padding(torch.ones(2, 4, dtype=torch.long), 4) is None
    lead = torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1], [0, 1, 1, 1]])
    q_pad = new_chunk_padding(lead, 4)
    assert q_pad.dtype == torch.int32 and q_pad.tolist() == [2, 0, 1]
    # a [B, past + Lnew] mask: only its last Lnew columns are the new chunk
    assert new_chunk_padding(torch.cat([torch.zeros(3, 5, dtype=torch.long), lead], 1), 4).tolist() == [2, 0, 1]
    zeros = torch.tensor([[0, 0, 0], [0, 1, 1]])
    q_pad = new_chunk_padding(zeros, 3)
    assert q_pad.tolist() == [3, 1] and (3 - q_pad).tolist() == [0, 2]  # a row of zeros: n_new = 0
    with pytest.raises(NotImplementedError, match="masked tokens"):
        new_chunk_padding(torch.tensor([[1, 1, 0, 1], [1, 1, 1, 1]]), 4)
    with pytest.raises(NotImplementedError, match="masked tokens"):
        new_chunk_padding(torch.tensor([[0, 1, 0, 1]]), 4)
    with pytest.raises(ValueError, match="expected"):
        new_chunk_padding(torch.ones(2, 3, dtype=torch.long), 4)


# ---------------------------------------------------------------------------------------------
# model: a ragged turn, early finishers, the unchanged paths, a chunked ragged turn
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _model(seed=6):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable="none", init="none")
    m.load_state_dict(O.make_weights(O.config_small_gpu(), seed))
    m.eval()
    return m


@functools.lru_cache(maxsize=1)
def _two_conversations():
    """two prompts (20 and 25 tokens, one image each), the shorter left-padded into a [2, 25] batch, and
    a second turn of 3 and 7 tokens as one left-padded [2, 7] block with its mask (CPU tensors)"""
    cfg = O.config_small_gpu()
    ids_a, mask_a, pix_a, _ = O.make_inputs(cfg, 1, 20, 3, 51)
    ids_b, mask_b, pix_b, _ = O.make_inputs(cfg, 1, 25, 3, 52)
    pad = cfg.pad_token_id
    ids = torch.cat([torch.cat([torch.full((1, 5), pad), ids_a], 1), ids_b], 0)
    mask = torch.cat([torch.cat([torch.zeros(1, 5, dtype=mask_a.dtype), mask_a], 1), mask_b], 0)
    pix = torch.cat([pix_a, pix_b], 0)
    g = torch.Generator().manual_seed(8)
    t_a = torch.randint(2, cfg.image_token_index, (1, 3), generator=g)
    t_b = torch.randint(2, cfg.image_token_index, (1, 7), generator=g)
    turn = torch.cat([torch.cat([torch.full((1, 4), pad), t_a], 1), t_b], 0)
    tmask = torch.tensor([[0, 0, 0, 0, 1, 1, 1], [1] * 7])
    return dict(a=(ids_a, mask_a, pix_a, t_a), b=(ids_b, mask_b, pix_b, t_b), ids=ids, mask=mask, pix=pix, turn=turn,
                tmask=tmask)


def _prefill_both(m, c):
    return m(input_ids=c["ids"].cuda(), pixel_values=c["pix"].cuda(), attention_mask=c["mask"].cuda(),
             use_cache=True).past_key_values


@pytest.mark.gpu
def test_ragged_turn_equals_solo_turns():
    cfg = O.config_small_gpu()
    W = O.make_weights(cfg, 6)
    m = _model()
    c = _two_conversations()
    cache = _prefill_both(m, c)
    assert cache.lengths is None
    out = m(input_ids=c["turn"].cuda(), past_key_values=cache, attention_mask=c["tmask"].cuda(), use_cache=True)
    cache = out.past_key_values
    assert out.logits.shape == (2, 7, cfg.text.vocab_size) and cache.lengths is not None
    P = cfg.vision.num_patches - 1
    assert cache.lengths.tolist() == [25 + P + 3, 25 + P + 7] and cache.length == 25 + P + 7
    for row, key in enumerate("ab"):
        ids, mask, pix, t = c[key]
        n = t.shape[1]
        solo = m(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda(), use_cache=True)
        solo = m(input_ids=t.cuda(), past_key_values=solo.past_key_values, use_cache=True)
        assert rel_l2(out.logits[row, 7 - n:], solo.logits[0]) <= 1e-2, key
        full = torch.cat([ids, t], 1)
        _, logits_ref, _ = O.forward(W, cfg, full, pix, torch.ones_like(full), None)
        assert rel_l2(out.logits[row, 7 - n:], logits_ref[0, -n:]) <= 3e-2, key
        sc = solo.past_key_values
        ks, ln = int(cache.kv_start[row]), int(cache.lengths[row])
        # the left-padded prefill keeps its padding rows below kv_start: the conversation's own rows
        assert ln - ks == sc.length and int(cache.next_pos[row]) == int(sc.next_pos[0])
        for li in (0, len(cache) - 1):
            assert rel_l2(cache.k[li, row, ks:ln], sc.k[li, 0, :sc.length]) <= 1e-2, (key, li)
            assert rel_l2(cache.v[li, row, ks:ln], sc.v[li, 0, :sc.length]) <= 1e-2, (key, li)
    km = cache.key_mask()
    assert km.shape == (2, cache.length) and km.sum(-1).tolist() == [20 + P + 3, 25 + P + 7]


@pytest.mark.gpu
def test_chunked_ragged_turn_matches_one_pass():
    m = _model()
    c = _two_conversations()
    kw = dict(input_ids=c["turn"].cuda(), attention_mask=c["tmask"].cuda(), use_cache=True)
    a = m(past_key_values=_prefill_both(m, c), **kw)
    m.prefill_chunk = 4  # pieces of columns 0-3 (row 0: all padding) and 4-6
    try:
        cache_b = _prefill_both(m, c)
        b = m(past_key_values=cache_b, **kw)
    finally:
        m.prefill_chunk = None
    ca, cb = a.past_key_values, b.past_key_values
    assert torch.equal(ca.lengths.cpu(), cb.lengths.cpu()) and torch.equal(ca.next_pos.cpu(), cb.next_pos.cpu())
    assert ca.length == cb.length
    for row, n in ((0, 3), (1, 7)):
        assert rel_l2(b.logits[row, 7 - n:], a.logits[row, 7 - n:]) <= 1e-2
        ks, ln = int(ca.kv_start[row]), int(ca.lengths[row])
        for li in (0, len(ca) - 1):
            assert rel_l2(cb.k[li, row, ks:ln], ca.k[li, row, ks:ln]) <= 1e-2
            assert rel_l2(cb.v[li, row, ks:ln], ca.v[li, row, ks:ln]) <= 1e-2


@pytest.mark.gpu
def test_uniform_paths_create_no_lengths():
    """compact_cache=False and an all-ones mask: the ragged path is not entered (cache.lengths is never
    created) and the results are bitwise those of the calls without the new arguments"""
    cfg = O.config_small_gpu()
    m = _model()
    ids, mask, pix, _ = O.make_inputs(cfg, 2, 20, 3, 17)
    kw = dict(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda())
    g0 = m.generate(**kw, max_new_tokens=5, return_dict_in_generate=True)
    g1 = m.generate(**kw, max_new_tokens=5, return_dict_in_generate=True, compact_cache=False)
    assert torch.equal(g0.sequences, g1.sequences)
    assert g0.past_key_values.lengths is None and g1.past_key_values.lengths is None
    L = g0.past_key_values.length
    assert g1.past_key_values.length == L
    assert torch.equal(g0.past_key_values.k[:, :, :L], g1.past_key_values.k[:, :, :L])
    toks = torch.randint(2, cfg.image_token_index, (2, 3), generator=torch.Generator().manual_seed(4)).cuda()
    c0 = m(**kw, use_cache=True).past_key_values
    c1 = m(**kw, use_cache=True).past_key_values
    a = m(input_ids=toks, past_key_values=c0, use_cache=True)
    b = m(input_ids=toks, past_key_values=c1, attention_mask=torch.ones(2, 3, dtype=torch.long, device=DEV),
          use_cache=True)
    assert torch.equal(a.logits, b.logits)
    assert a.past_key_values.lengths is None and b.past_key_values.lengths is None
    assert torch.equal(c0.k[:, :, :c0.length], c1.k[:, :, :c1.length])


# greedy generation on make_inputs(config_small_gpu(), 2, 20, 3, 64) with make_weights(.., 6), found once
# on the GPU from a run without an eos: token 691 is row 0's 4th new token and row 1's 8th
EOS, STOP = 691, (4, 8)


def _ref_argmax_or_near_tie(W, cfg, conv, pix, n0, n_new):
    """test_cached_prefill.py::test_multi_turn_generate_matches_oracle's criterion on tokens conv[n0 ..
    n0 + n_new) of one conversation [1, n] (no pads) against the oracle's full recompute"""
    for i in range(n_new):
        prefix = conv[:, :n0 + i]
        _, lg, _ = O.forward(W, cfg, prefix, pix, torch.ones_like(prefix), None)
        last = lg[0, -1]
        tok = int(conv[0, n0 + i])
        top = torch.topk(last, 2).values
        assert tok == int(last.argmax()) or (last.max() - last[tok]).item() <= 2e-2 * (top[0] - last.min()).item(), i


@pytest.mark.gpu
def test_early_finisher_keeps_its_conversation():
    cfg = O.config_small_gpu()
    W = O.make_weights(cfg, 6)
    m = _model()
    ids, mask, pix, _ = O.make_inputs(cfg, 2, 20, 3, 64)
    kw = dict(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda(), max_new_tokens=20,
              eos_token_id=EOS, return_dict_in_generate=True)
    plain = m.generate(**kw, compact_cache=False)
    r1 = m.generate(**kw, compact_cache=True)
    seq = r1.sequences.cpu()
    assert torch.equal(r1.sequences, plain.sequences)
    stop = [(seq[b, 20:] == EOS).nonzero()[0].item() + 1 for b in range(2)]  # the step that produced eos
    assert tuple(stop) == STOP and stop[0] != stop[1] and seq.shape[1] == 20 + max(stop)
    cache = r1.past_key_values
    L0 = 20 + cfg.vision.num_patches - 1
    # per row, every real token but its eos
    assert cache.lengths.tolist() == [L0 + stop[0] - 1, L0 + stop[1] - 1]
    assert int(cache.lengths[1] - cache.lengths[0]) == stop[1] - stop[0]
    assert cache.next_pos.tolist() == cache.lengths.tolist() and cache.length == L0 + stop[1] - 1
    assert plain.past_key_values.lengths is None and plain.past_key_values.length == L0 + max(stop) - 1

    # the same first turn on the device loop, and both loops without the decode graph
    for extra in (dict(device_loop=True), dict(decode_graph=False), dict(device_loop=True, decode_graph=False)):
        r = m.generate(**kw, compact_cache=True, **extra)
        assert torch.equal(r.sequences, r1.sequences), extra
        assert r.past_key_values.lengths.tolist() == cache.lengths.tolist(), extra
        assert r.past_key_values.next_pos.tolist() == cache.next_pos.tolist(), extra
        for li in (0, len(cache) - 1):
            for b in range(2):
                n = int(cache.lengths[b])
                assert rel_l2(r.past_key_values.k[li, b, :n], cache.k[li, b, :n]) <= 1e-2, (extra, li, b)

    # a second turn on the ragged cache: HF's convention, each row's first id is its last token (eos),
    # 5 and 3 new tokens, the shorter row left-padded
    g = torch.Generator().manual_seed(5)
    new0 = torch.randint(2, cfg.image_token_index, (1, 5), generator=g)
    new1 = torch.randint(2, cfg.image_token_index, (1, 3), generator=g)
    eos = torch.full((1, 1), EOS)
    turn2 = torch.cat([torch.cat([eos, new0], 1), torch.cat([torch.full((1, 2), cfg.pad_token_id), eos, new1], 1)], 0)
    mask2 = torch.tensor([[1] * 6, [0, 0, 1, 1, 1, 1]])
    out = m.generate(input_ids=turn2.cuda(), attention_mask=mask2.cuda(), past_key_values=cache, max_new_tokens=4)
    assert out.shape == (2, 10) and torch.equal(out[:, :6].cpu(), turn2)
    out = out.cpu()
    # the early finisher (row 0): its real tokens through its eos, the new turn, no pads
    conv0 = torch.cat([ids[:1], seq[:1, 20:20 + stop[0]], new0, out[:1, 6:]], 1)
    _ref_argmax_or_near_tie(W, cfg, conv0, pix[:1], 20 + stop[0] + 5, 4)
    conv1 = torch.cat([ids[1:], seq[1:, 20:20 + stop[1]], new1, out[1:, 6:]], 1)
    _ref_argmax_or_near_tie(W, cfg, conv1, pix[1:], 20 + stop[1] + 3, 4)
