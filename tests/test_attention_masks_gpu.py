"""The bf16 MFMA attention kernels (csrc/attention.hip) against float64 where their masks and index
arithmetic can go wrong: left padding (kv_start) on, just before and just after every 32-, 64- and
128-key tile boundary, whole dead key blocks and (causal) dead 128-query blocks beside live ones,
query rows that see no key, Lq != Lk, a batch row with nothing live (kv_start == Lk), every forward
stage / backward mode the dispatch can pick, and the production layout (q | k | v and dq | dk | dv as
column blocks of one buffer, O through out= into a wider one).

Reference (_Ref): f64 attention of [B*L, H*D] q, k, v, dO in torch on the GPU. Key j is live for query
i of batch b iff kv_start[b] <= j < Lk (and j <= i when causal); the softmax runs over live keys only,
rows with none give O = 0 (nan_to_num, as tests/test_parity_modes.py::test_attention_generic). The
backward's delta = rowsum(dO * O) takes the kernel's stored bf16 O, as _attn_ref of
tests/test_accuracy_gpu.py does. The same function restates the FA2 arithmetic in f64 (P rounded to
bf16 before P V and P^T dO, dS rounded to bf16 before the dQ and dK products, O / dQ / dK / dV rounded
to bf16 once): that emulation's rel-L2 against the exact result is the floor the number formats alone
put under a correct kernel. It comes from the reference, never from a kernel's output.

Gates (the first three are test_accuracy_gpu.py's, same definitions):
  LSE      rows with a live key: |lse - LSE_f64| <= 1e-5; rows with none: exactly +inf;
  element  O, dQ, dK, dV: max |err| / (|ref| + rms of ref's (token, head) row + 1e-3 tensor rms) <= 2^-3;
  rel-L2   O, dQ, dK, dV: <= max(3e-3, 1.3 x that tensor's emulated floor) (1.3: what the emulation
           leaves out -- f32 accumulation order, exp2, the deferred rescale);
  zeros    exactly 0 (== 0, no tolerance): O and dQ rows of queries with no live key, dK and dV rows
           of keys j < kv_start[b];
  finite   every element of O, dQ, dK, dV, and LSE on rows with a live key (never NaN anywhere);
  sanity   max |lse - LSE_f64| over live rows is finite and > 0: an f32 LSE cannot equal an f64
           log-sum-exp over hundreds of rows, so 0 means the comparison compared nothing.
No row is excluded from the tolerance gates: rows that see no key have reference 0 and must be 0.

One JSON line per case (floor and measured value per tensor) is appended to the statistics file of
tests/test_accuracy_gpu.py (its _log); the lines of one MI355X run are committed as
profiles/r07/accuracy/attention_masks.jsonl. Measured there over the 50 case / path lines: rel-L2
0.45e-3 .. 2.43e-3 against emulated floors 0.45e-3 .. 2.43e-3 (the small ones are O and dV of cases
with a batch row of one live key, where O = V exactly; no tensor above 1.0002 x its floor), row-scaled
error <= 1.9e-2 (floor <= 1.1e-2), LSE error 3.5e-7 .. 1.1e-6. The regenerated lines of
test_accuracy_gpu.py::test_attention_against_f64 are beside it (attention_f64.jsonl).
"""
import contextlib
import functools
import zlib

import pytest
import torch

from tests.test_accuracy_gpu import _log  # the same statistics file, one line per case

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
H = 2
TENSORS = ("O", "dQ", "dK", "dV")


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def clib():
    from cullavo_amd import _lib
    return _lib


def _bf(x):
    """x (f64) rounded to bf16, back in f64"""
    return x.to(BF).double()


def _rel_l2(a, ref):
    return ((a - ref).norm() / ref.norm()).item()


def _row_scaled(a, ref, D):
    """max |a - ref| / (|ref| + rms of ref's (token, head) row + 1e-3 rms of ref), as test_accuracy_gpu.py"""
    rows, hd = ref.shape
    row_rms = ref.view(rows, hd // D, D).pow(2).mean(-1, keepdim=True).sqrt().expand(-1, -1, D).reshape(ref.shape)
    floor = 1e-3 * ref.pow(2).mean().sqrt()
    return ((a - ref).abs() / (ref.abs() + row_rms + floor)).max().item()


class _Ref:
    """f64 attention forward of one case, computed once; backward(o_kernel) adds the part that
    depends on the kernel's stored O (delta). Exact results in .O, .LSE and backward()'s dict, the
    bf16-emulated ones beside them."""

    def __init__(self, q, k, v, do, *, B, Lq, Lk, D, scale, causal, ks):
        self.B, self.Lq, self.Lk, self.D, self.scale = B, Lq, Lk, D, scale
        dev = q.device

        def heads(x, L):
            return x.double().view(B, L, H, D).transpose(1, 2)  # [B, H, L, D]
        self.Q, self.K, self.V, self.dO = heads(q, Lq), heads(k, Lk), heads(v, Lk), heads(do, Lq)
        i = torch.arange(Lq, device=dev)[None, :, None]
        j = torch.arange(Lk, device=dev)[None, None, :]
        start = torch.as_tensor(ks if ks is not None else [0] * B, device=dev).long()[:, None, None]
        live = (j >= start) & (j < Lk)  # [B, 1 or Lq, Lk]
        if causal:
            live = live & (j <= i)
        live = live.expand(B, Lq, Lk)
        self.live_q = live.any(-1)                               # [B, Lq]: the query sees a key
        self.dead_k = (j < start).reshape(B, Lk)                 # [B, Lk]: keys before kv_start
        S = (self.Q @ self.K.transpose(-1, -2)) * scale
        S = S.masked_fill(~live[:, None], float("-inf"))
        self.LSE = torch.logsumexp(S, -1)                        # [B, H, Lq], -inf where nothing is live
        self.P = torch.nan_to_num(torch.exp(S - self.LSE[..., None]), nan=0.0)
        self.Pb = _bf(self.P)
        self.O = self._flat(self.P @ self.V, Lq)
        self.O_emu = _bf(self._flat(self.Pb @ self.V, Lq))
        self.dV = self._flat(self.P.transpose(-1, -2) @ self.dO, Lk)
        self.dV_emu = _bf(self._flat(self.Pb.transpose(-1, -2) @ self.dO, Lk))
        self.dP = self.dO @ self.V.transpose(-1, -2)

    def _flat(self, x, L):
        return x.transpose(1, 2).reshape(self.B * L, H * self.D)

    def backward(self, o_kernel):
        """{name: (exact, emulated)} of O, dQ, dK, dV with delta from the kernel's O"""
        ok = o_kernel.double().view(self.B, self.Lq, H, self.D).transpose(1, 2)
        delta = (self.dO * ok).sum(-1, keepdim=True)
        dS = self.P * (self.dP - delta)
        dSb = _bf(dS)
        return {
            "O": (self.O, self.O_emu),
            "dQ": (self._flat(dS @ self.K * self.scale, self.Lq), _bf(self._flat(dSb @ self.K * self.scale, self.Lq))),
            "dK": (self._flat(dS.transpose(-1, -2) @ self.Q * self.scale, self.Lk),
                   _bf(self._flat(dSb.transpose(-1, -2) @ self.Q * self.scale, self.Lk))),
            "dV": (self.dV, self.dV_emu),
        }


def gate(rec, ref, o, lse, dq, dk, dv):
    """Every gate of the module docstring on one set of kernel outputs; fills rec, returns the failures."""
    B, Lq, Lk, D = ref.B, ref.Lq, ref.Lk, ref.D
    fails = []
    live_rows = ref.live_q.reshape(B * Lq)
    live_lse = ref.live_q[:, None, :].expand(B, H, Lq)
    dead_keys = ref.dead_k.reshape(B * Lk)
    rec["dead_query_rows"] = int((~live_rows).sum().item())
    rec["masked_key_rows"] = int(dead_keys.sum().item())
    # LSE: live rows against f64 (and the comparison itself: finite, not 0), dead rows +inf
    lse_err = (lse.double() - ref.LSE)[live_lse].abs()
    lse_max = lse_err.max().item() if lse_err.numel() else float("nan")
    rec["lse_max_abs"] = lse_max
    if not (lse_max == lse_max and lse_max != float("inf") and lse_max > 0.0):
        fails.append(f"lse max|err| {lse_max} over live rows is not finite and > 0: the comparison is broken")
    if not lse_max <= 1e-5:
        fails.append(f"lse max|err| {lse_max:.2e}")
    if torch.isnan(lse).any().item():
        fails.append("lse has NaN")
    if not (lse[~live_lse] == float("inf")).all().item():
        fails.append("lse of a row with no live key is not +inf")
    got = {"O": o, "dQ": dq, "dK": dk, "dV": dv}
    refs = ref.backward(o)
    for nm in TENSORS:
        out = got[nm]
        exact, emu = refs[nm]
        if not torch.isfinite(out.float()).all().item():
            fails.append(f"{nm} has non-finite elements")
        zero_rows = dead_keys if nm in ("dK", "dV") else ~live_rows
        nz = int((out[zero_rows] != 0).sum().item())
        if nz:
            what = "keys before kv_start" if nm in ("dK", "dV") else "queries with no live key"
            fails.append(f"{nm}: {nz} nonzero elements on rows of {what}")
        rel, worst = _rel_l2(out.double(), exact), _row_scaled(out.double(), exact, D)
        floor_rel, floor_worst = _rel_l2(emu, exact), _row_scaled(emu, exact, D)
        rec[f"{nm}_rel_l2"], rec[f"{nm}_max_row_scaled"] = rel, worst
        rec[f"{nm}_floor_rel_l2"], rec[f"{nm}_floor_max_row_scaled"] = floor_rel, floor_worst
        bound = max(3e-3, 1.3 * floor_rel)
        if not rel <= bound:
            fails.append(f"{nm} rel-L2 {rel:.2e} > {bound:.2e} (emulated floor {floor_rel:.2e})")
        if not worst <= 2 ** -3:
            fails.append(f"{nm} max |err| / (|ref| + row rms) {worst:.2e}")
    return fails


# ---- cases -----------------------------------------------------------------------------------------
SWEEP_STARTS = ([0, 1, 63, 64], [65, 127, 128, 129], [200, 256, 299, 0])
CASES = {}
for _D, _causal in ((128, True), (64, False), (64, True)):
    for _n, _ks in enumerate(SWEEP_STARTS):
        # the mask edge on / one before / one after each 32-, 64- and 128-key boundary; dead key
        # blocks and (causal) dead 128-query blocks beside live ones; one live key (299)
        CASES[f"sweep_d{_D}_{'causal' if _causal else 'full'}_{_n}"] = dict(B=4, Lq=300, Lk=300, D=_D, causal=_causal, ks=_ks)
CASES.update({
    # one partial tile
    "tile33_d128_causal": dict(B=2, Lq=33, Lk=33, D=128, causal=True, ks=[0, 32]),
    "tile33_d64_full": dict(B=2, Lq=33, Lk=33, D=64, causal=False, ks=[0, 32]),
    # Lq != Lk (non-causal only: the C ABI rejects it when causal)
    "lq70_lk200_d128": dict(B=2, Lq=70, Lk=200, D=128, causal=False, ks=[0, 37]),
    "lq200_lk70_d64": dict(B=2, Lq=200, Lk=70, D=64, causal=False, ks=[0, 69]),
    "lq70_lk200_d128_nostart": dict(B=2, Lq=70, Lk=200, D=128, causal=False, ks=None),
    "lq200_lk70_d64_nostart": dict(B=2, Lq=200, Lk=70, D=64, causal=False, ks=None),
    # nothing live in batch 0 (kv_start == Lk: what modeling.py computes for an all-zero mask row)
    "dead_batch_d128_causal": dict(B=2, Lq=300, Lk=300, D=128, causal=True, ks=[300, 0]),
    "dead_batch_d64_full": dict(B=2, Lq=300, Lk=300, D=64, causal=False, ks=[300, 0]),
    # the production-layout case's shape
    "layout_d128_causal": dict(B=2, Lq=300, Lk=300, D=128, causal=True, ks=[0, 65]),
})


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, kwargs of ops.attn_fwd / attn_bwd, _Ref) of a case: built once, shared, never modified"""
    c = CASES[name]
    B, Lq, Lk, D = c["B"], c["Lq"], c["Lk"], c["D"]
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(name.encode()))
    q, do = (torch.randn(B * Lq, H * D, device=DEV, generator=g).to(BF) for _ in range(2))
    k, v = (torch.randn(B * Lk, H * D, device=DEV, generator=g).to(BF) for _ in range(2))
    kw = dict(B=B, H=H, Lq=Lq, Lk=Lk, D=D, scale=D ** -0.5, causal=c["causal"])
    if c["ks"] is not None:
        assert all(0 <= s <= Lk for s in c["ks"])  # kv_start > Lk is outside the kernels' contract
        kw["kv_start"] = torch.tensor(c["ks"], dtype=torch.int32, device=DEV)
    ref = _Ref(q, k, v, do, B=B, Lq=Lq, Lk=Lk, D=D, scale=kw["scale"], causal=c["causal"], ks=c["ks"])
    return (q, k, v, do), kw, ref


def _record(name, path):
    c = CASES[name]
    return {"test": "attention_masks", "case": name, "path": path, "B": c["B"], "H": H, "Lq": c["Lq"], "Lk": c["Lk"],
            "D": c["D"], "causal": c["causal"], "kv_start": c["ks"]}


def _check(name, path, o, lse, dq, dk, dv):
    torch.cuda.synchronize()
    rec = _record(name, path)
    fails = gate(rec, _case(name)[2], o, lse, dq, dk, dv)
    _log(rec)
    assert not fails, f"{name} [{path}]: " + "; ".join(fails)


@pytest.mark.parametrize("name", list(CASES))
def test_masks_against_f64(name):
    (q, k, v, do), kw, ref = _case(name)
    o, lse = ops().attn_fwd(q, k, v, **kw)
    dq, dk, dv = ops().attn_bwd(q, k, v, o, do, lse, **kw)
    _check(name, "default", o, lse, dq, dk, dv)
    if name.startswith("dead_batch"):  # batch 0: nothing live, everything exactly 0 / +inf
        Lq, Lk = ref.Lq, ref.Lk
        assert not ref.live_q[0].any() and ref.dead_k[0].all()
        for nm, t, L in (("O", o, Lq), ("dQ", dq, Lq), ("dK", dk, Lk), ("dV", dv, Lk)):
            assert (t[:L] == 0).all().item(), f"{name}: {nm} of the batch row with nothing live"
        assert (lse[0] == float("inf")).all().item()


# ---- every dispatch path against the reference ------------------------------------------------------
@contextlib.contextmanager
def _switched(setter, value):
    prev = setter(value)
    try:
        yield
    finally:
        setter(prev)


def _bwd_no_workspace(q, k, v, o, do, lse, *, B, H, Lq, Lk, D, scale, causal, kv_start=None):
    """cullavo_attn_bwd, the entry without a workspace: in mode 7 the mode-4 recompute fallback runs"""
    dq = torch.empty((B * Lq, H * D), dtype=q.dtype, device=q.device)
    dk, dv = (torch.empty((B * Lk, H * D), dtype=q.dtype, device=q.device) for _ in range(2))
    delta = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    args = []
    for t in (q, k, v, o, do):
        args += [t.data_ptr(), t.stride(0)]
    args += [lse.data_ptr(), delta.data_ptr()]
    for t in (dq, dk, dv):
        args += [t.data_ptr(), t.stride(0)]
    clib().call("attn_bwd", *args, B, H, Lq, Lk, D, float(scale), int(causal),
                None if kv_start is None else kv_start.data_ptr(), clib().DT_BF16,
                torch.cuda.current_stream().cuda_stream)
    return dq, dk, dv


PATH_CASES = ["sweep_d128_causal_1", "sweep_d64_full_1", "sweep_d64_causal_1", "lq70_lk200_d128"]
# forward: the default stage, the software-pipelined kernel named explicitly (7) and the plain tile
# loop (4); backward: the 4-wave kernels at 32/32 and 32/64 tiles (0, 2), the 8-wave dK/dV kernel with
# the recomputing dQ (4), with dQ from the stored dS^T (7, workspace), and 7 falling back to 4
PATHS = ["fwd_default", "fwd_stage7", "fwd_stage4", "bwd_mode0", "bwd_mode2", "bwd_mode4", "bwd_mode7_workspace",
         "bwd_mode7_no_workspace"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", PATH_CASES)
def test_dispatch_paths_against_f64(name, path):
    (q, k, v, do), kw, _ = _case(name)
    L_ = clib().lib()
    fwd, bwd = ops().attn_fwd, ops().attn_bwd
    with contextlib.ExitStack() as stack:
        if path.startswith("fwd_stage"):
            stack.enter_context(_switched(L_.cullavo_attn_set_stage, int(path[-1])))
        o, lse = fwd(q, k, v, **kw)
    with contextlib.ExitStack() as stack:
        if path.startswith("bwd_mode"):
            mode = int(path[len("bwd_mode")])
            stack.enter_context(_switched(L_.cullavo_attn_set_bwd_tiles, mode))
            nbytes = L_.cullavo_attn_bwd_workspace(kw["B"], H, kw["Lq"], kw["Lk"], kw["D"], clib().DT_BF16)
            assert (nbytes > 0) == (mode == 7), "only mode 7 asks for the dS^T workspace"
            if path.endswith("no_workspace"):
                bwd = _bwd_no_workspace
        dq, dk, dv = bwd(q, k, v, o, do, lse, **kw)
    _check(name, path, o, lse, dq, dk, dv)


# ---- independence from masked data, bitwise ----------------------------------------------------------
@pytest.mark.parametrize("name", ["sweep_d128_causal_1", "sweep_d64_full_1"])
def test_masked_rows_are_never_read_into_live_results(name):
    """Two runs that differ only in rows that must not matter -- K and V rows j < kv_start[b], and in
    causal mode Q and dO rows i < kv_start[b] (queries with no live key) -- filled with fresh finite
    50 x randn: O, LSE, dQ on rows with a live key and dK, dV on live keys are bit-identical. A leaked
    key with a 50 x score dominates its softmax, so no tolerance is needed. (NaN neighbours:
    tests/test_oob_guard.py.) Every backward mode, since the 4-wave and 8-wave kernels mask differently."""
    (q, k, v, do), kw, ref = _case(name)
    B, Lq, Lk, D = ref.B, ref.Lq, ref.Lk, ref.D
    dead_k = ref.dead_k.reshape(B * Lk)
    dead_q = ~ref.live_q.reshape(B * Lq)
    live_lse = ref.live_q[:, None, :].expand(B, H, Lq)
    assert dead_k.any() and (dead_q.any() or not kw["causal"])
    L_ = clib().lib()

    def run(seed, mode):
        g = torch.Generator(device=DEV).manual_seed(seed)
        fill = lambda n: (torch.randn(n, H * D, device=DEV, generator=g) * 50).to(BF)  # noqa: E731
        q2, k2, v2, do2 = q.clone(), k.clone(), v.clone(), do.clone()
        k2[dead_k] = fill(int(dead_k.sum()))
        v2[dead_k] = fill(int(dead_k.sum()))
        if kw["causal"]:
            q2[dead_q] = fill(int(dead_q.sum()))
            do2[dead_q] = fill(int(dead_q.sum()))
        o, lse = ops().attn_fwd(q2, k2, v2, **kw)
        with _switched(L_.cullavo_attn_set_bwd_tiles, mode):
            dq, dk, dv = ops().attn_bwd(q2, k2, v2, o, do2, lse, **kw)
        torch.cuda.synchronize()
        for t in (o, dq, dk, dv):
            assert torch.isfinite(t.float()).all().item()
        return {"O": o[~dead_q], "LSE": lse[live_lse], "dQ": dq[~dead_q], "dK": dk[~dead_k], "dV": dv[~dead_k]}

    for mode in (-1, 0, 2, 4, 7):
        a, b = run(1001, mode), run(2002, mode)
        for nm in a:
            va, vb = (t.view(torch.int16 if t.dtype == BF else torch.int32) for t in (a[nm], b[nm]))
            assert torch.equal(va, vb), f"{name}: {nm} depends on masked rows (backward mode {mode})"


# ---- production layout ---------------------------------------------------------------------------------
def test_production_layout_bitwise():
    """q | k | v as column blocks of one [T, 3 H D] buffer, dq | dk | dv written into the column blocks
    of another (functions.py's decoder layer), O through out= into a column block of a wider buffer:
    bitwise the contiguous call's results, and nothing written outside the blocks."""
    name = "layout_d128_causal"
    (q, k, v, do), kw, ref = _case(name)
    T, hd = q.shape
    o, lse = ops().attn_fwd(q, k, v, **kw)
    dq, dk, dv = ops().attn_bwd(q, k, v, o, do, lse, **kw)
    qkv = torch.cat([q, k, v], dim=1)
    qs, ks_, vs = qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:]
    sentinel = 7.0  # exact in bf16
    wide = torch.full((T, hd + 128), sentinel, dtype=BF, device=DEV)
    o2, lse2 = ops().attn_fwd(qs, ks_, vs, out=wide[:, 64:64 + hd], **kw)
    assert o2.data_ptr() == wide[:, 64:].data_ptr()
    dqkv = torch.full((T, 3 * hd), sentinel, dtype=BF, device=DEV)
    ops().attn_bwd(qs, ks_, vs, o2, do, lse2, dq=dqkv[:, :hd], dk=dqkv[:, hd:2 * hd], dv=dqkv[:, 2 * hd:], **kw)
    torch.cuda.synchronize()
    i16 = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    assert torch.equal(i16(wide[:, 64:64 + hd]), i16(o)), "O through out= differs from the contiguous call"
    assert (wide[:, :64] == sentinel).all().item() and (wide[:, 64 + hd:] == sentinel).all().item(), \
        "the forward wrote outside its column block"
    assert torch.equal(lse2.view(torch.int32), lse.view(torch.int32))
    for nm, a, b in (("dq", dqkv[:, :hd], dq), ("dk", dqkv[:, hd:2 * hd], dk), ("dv", dqkv[:, 2 * hd:], dv)):
        assert torch.equal(i16(a), i16(b)), f"{nm} written into its column block differs from the contiguous call"
