"""The wide decode product on the GPU (csrc/gemv_wide.hip, ops.decode_linear_wide: 17 <= M <= 64 rows)
and its route through the decode step (generation.wide_route).

Kernel: the f32 output per element against float64 under tests/decode_refs.py's gate for any f32
summation order (K 2^-24 |X||W|^T, rel-L2 1e-5), the bf16 outputs bit for bit epilogue_replay of the
call's own f32 output, transform 3 bitwise swiglu_fwd of the plain product, rows independent of the
other rows in the call, nothing written outside [M, N], bad arguments refused before a launch.
Model (the tiny config at 17 and 33 sequences): the step's Linears go through the wide product with
the switch on and only then, graph replay equals the eager step bitwise, ragged and fp8_sim caches
route the same way, and the logits stay within the project's end-to-end bf16 gate (rel-L2 1e-2,
VERDICT.md) of the tiled route's -- measured 1.8e-4 .. 1.7e-3 without and 7.3e-4 .. 1.2e-3 with
adapters (profiles/r21/wide_decode/model_rel_l2.txt).
"""
import functools

import pytest
import torch

from oracle import cullavo_oracle as O
from tests import decode_refs as R
from tests import decode_wide_refs as WR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"
SENTINEL = 777.0


def _case_id(c):
    return "x".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K):
    """the case's tensors on the GPU and its float64 reference, computed once"""
    X, W, _, add, res = WR.wide_inputs(M, N, K)
    X, W, add, res = X.to(DEV), W.to(DEV), add.to(DEV), res.to(DEV)
    ref, absprod = R.gemv_ref(X, W)
    return X, W, add, res, ref, absprod


# ---------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", WR.WIDE_CASES, ids=[_case_id(c) for c in WR.WIDE_CASES])
def test_wide_f32_gate_and_epilogues_bitwise(M, N, K):
    from cullavo_amd import ops
    X, W, add, res, ref, absprod = _inputs(M, N, K)
    c32 = ops.decode_linear_wide(X, W, out_dtype=torch.float32)
    assert c32.dtype == torch.float32 and tuple(c32.shape) == (M, N)
    w, rel = R.gemv_gate(c32, ref, absprod, K)
    print(f"wide {M}x{N}x{K}: err/gate {w:.3f}, rel-L2 {rel:.2e}")
    assert w <= 1.0 and rel <= 1e-5
    for name, a, r in (("none", None, None), ("addend", add, None), ("residual", None, res), ("both", add, res)):
        y = ops.decode_linear_wide(X, W, addend=a, residual=r)
        assert y.dtype == BF
        assert torch.equal(y, R.epilogue_replay(c32, addend=a, residual=r)), f"{name}: not store4's chain"


@pytest.mark.parametrize("M,N,K", WR.WIDE_SWIGLU_CASES, ids=[_case_id(c) for c in WR.WIDE_SWIGLU_CASES])
def test_transform3_is_swiglu_of_the_plain_product(M, N, K):
    from cullavo_amd import ops
    X, W2, _, _, _ = WR.wide_inputs(M, 2 * N, K)
    X, W2 = X.to(DEV), W2.to(DEV)
    y = ops.decode_linear_wide(X, W2, transform=3)
    assert tuple(y.shape) == (M, N) and y.dtype == BF
    assert torch.equal(y, ops.swiglu_fwd(ops.decode_linear_wide(X, W2)))
    buf = torch.full((M + 2, N + 16), SENTINEL, dtype=BF, device=DEV)
    ops.decode_linear_wide(X, W2, transform=3, out=buf[:M, 8:8 + N])
    assert torch.equal(buf[:M, 8:8 + N], y)
    buf[:M, 8:8 + N] = SENTINEL
    assert bool((buf == SENTINEL).all())


@pytest.mark.parametrize("rows", [17, 33])
@pytest.mark.parametrize("N,K", [(776, 1000), (264, 4096)])
def test_rows_do_not_depend_on_the_other_rows(rows, N, K):
    from cullavo_amd import ops
    X, W, add, res, _, _ = _inputs(64, N, K)
    for kw in (dict(out_dtype=torch.float32), dict()):
        full = ops.decode_linear_wide(X, W, **kw)
        part = ops.decode_linear_wide(X[:rows], W, **kw)
        assert torch.equal(part, full[:rows])
    full = ops.decode_linear_wide(X, W, addend=add, residual=res)
    part = ops.decode_linear_wide(X[:rows], W, addend=add[:rows], residual=res[:rows])
    assert torch.equal(part, full[:rows])


@pytest.mark.parametrize("M,N,K", [(17, 24, 72), (33, 776, 1000), (64, 40, 8200)], ids=["17x24x72", "33x776x1000", "64x40x8200"])
def test_nothing_written_outside_the_block(M, N, K):
    """y: a column block of a wider buffer with more rows than M; x with ldx > K"""
    from cullavo_amd import ops
    X, W, add, res, _, _ = _inputs(M, N, K)
    xbuf = torch.full((M, K + 8), float("nan"), dtype=BF, device=DEV)
    xbuf[:, :K] = X
    want = ops.decode_linear_wide(X, W, addend=add, residual=res)
    for dt in (BF, torch.float32):
        buf = torch.full((M + 3, N + 16), SENTINEL, dtype=dt, device=DEV)
        y = buf[:M, 8:8 + N]
        ops.decode_linear_wide(xbuf[:, :K], W, out=y, addend=add if dt == BF else None,
                               residual=res if dt == BF else None)
        assert torch.equal(y, want if dt == BF else ops.decode_linear_wide(X, W, out_dtype=torch.float32))
        y.fill_(SENTINEL)
        assert bool((buf == SENTINEL).all()), f"{dt}: a store outside rows < M, columns of the block"


@pytest.mark.parametrize("what", ["M16", "M65", "N12", "K60", "transform1", "transform3_residual"])
def test_rejections_leave_the_output_alone(what):
    from cullavo_amd import ops
    M, N, K, kw = 17, 16, 64, {}
    if what == "M16":
        M = 16
    elif what == "M65":
        M = 65
    elif what == "N12":
        N = 12
    elif what == "K60":
        K = 60
    elif what == "transform1":
        kw = dict(transform=1)
    x = torch.ones(M, K, dtype=BF, device=DEV)
    w = torch.ones(N, K, dtype=BF, device=DEV)
    if what == "transform3_residual":
        kw = dict(transform=3, residual=torch.ones(M, N // 2, dtype=BF, device=DEV))
        out = torch.full((M, N // 2), SENTINEL, dtype=BF, device=DEV)
    else:
        out = torch.full((M, N), SENTINEL, dtype=BF, device=DEV)
    with pytest.raises(ValueError) as e:
        ops.decode_linear_wide(x, w, out=out, **kw)
    if what in ("M16", "M65"):
        assert "17 <= M <= 64" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------
# whole model
# ---------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _model(kind="plain"):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    if kind == "lora":
        m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable="lora", init="random", seed=11)
        ar = m.arenas["lora"]  # lora_B starts at zero: make the adapters' term count
        g = torch.Generator(device=DEV).manual_seed(12)
        ar.flat.copy_((0.05 * torch.randn(ar.numel, generator=g, device=DEV)).to(ar.dtype))
    else:
        m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable="none", init="none")
        m.load_state_dict(O.make_weights(O.config_small_gpu(), 6))
    m.eval()
    return m


STEPS = 4


def _prefill(m, B, **kw):
    cfg = O.config_small_gpu()
    ids, mask, pix, _ = O.make_inputs(cfg, B, 8, 3, 50 + B)
    L0 = 8 + cfg.vision.num_patches - 1
    return m._forward_cached(ids.to(DEV), pix.to(DEV), mask.to(DEV), None, None, None, -2, "default", None, True,
                             max_len=L0 + STEPS + 2, **kw).past_key_values


def _tokens(B):
    cfg = O.config_small_gpu()
    return torch.randint(2, cfg.image_token_index, (STEPS, B), generator=torch.Generator().manual_seed(9)).to(DEV)


def _steps(m, B, graph=False, **kw):
    """the logits of STEPS one-token steps after a prefill"""
    from cullavo_amd.generation import DecodeGraph
    cache = _prefill(m, B, **kw)
    toks = _tokens(B)
    g = DecodeGraph(m, cache) if graph else None
    out = []
    for t in toks:
        if g is not None:
            out.append(g.step(t).clone())
        else:
            out.append(m(input_ids=t[:, None], past_key_values=cache, use_cache=True).logits.clone())
    torch.cuda.synchronize()
    return out


@pytest.fixture
def spy(monkeypatch):
    """ops.decode_linear_wide recording (transform, addend given, residual given) per call"""
    from cullavo_amd import ops
    calls = []
    real = ops.decode_linear_wide

    def wrapped(x, w, **kw):
        calls.append((kw.get("transform", 0), kw.get("addend") is not None, kw.get("residual") is not None))
        return real(x, w, **kw)

    monkeypatch.setattr(ops, "decode_linear_wide", wrapped)
    return calls


@pytest.mark.parametrize("B", [17, 33])
def test_step_routes_wide_with_the_switch_and_only_then(monkeypatch, spy, B):
    from cullavo_amd import generation
    m = _model()
    layers = O.config_small_gpu().text.num_hidden_layers
    monkeypatch.setattr(generation, "DECODE_WIDE", True)
    on = _steps(m, B)
    # per layer q|k|v, o (residual), gate|up (transform 3), down (residual); then lm_head
    per_step = [(0, False, False), (0, False, True), (3, False, False), (0, False, True)] * layers + [(0, False, False)]
    assert spy == per_step * STEPS
    del spy[:]
    monkeypatch.setattr(generation, "DECODE_WIDE", False)
    off = _steps(m, B)
    assert spy == []
    monkeypatch.setattr(generation, "DECODE_WIDE", True)
    _steps(m, 16)
    assert spy == []
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.isfinite(a.float()).all()
        r = rel_l2(a, b)
        print(f"B {B} step {i}: wide vs tiled logits rel-L2 {r:.3e}")
        assert r <= 1e-2, (i, r)


@pytest.mark.parametrize("B", [17, 33])
def test_graph_replay_is_the_eager_wide_step(monkeypatch, spy, B):
    from cullavo_amd import generation
    monkeypatch.setattr(generation, "DECODE_WIDE", True)
    m = _model()
    eager = _steps(m, B)
    n = len(spy)
    graph = _steps(m, B, graph=True)
    assert n > 0 and len(spy) == n + n // STEPS  # captured once
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert torch.equal(a, b), i


def test_ragged_and_fp8_sim_caches_route_wide(monkeypatch, spy):
    from cullavo_amd import generation
    monkeypatch.setattr(generation, "DECODE_WIDE", True)
    m = _model()
    B = 17
    layers = O.config_small_gpu().text.num_hidden_layers
    cache = _prefill(m, B, kv_cache_dtype="fp8_sim")
    assert cache.kv_dtype == "fp8_sim"
    cache.make_ragged()
    toks = _tokens(B)
    mask = torch.ones(B, 1, dtype=torch.long, device=DEV)
    mask[3] = 0  # a row that appends nothing this step
    before = cache.lengths.clone()
    lg = m(input_ids=toks[0][:, None], attention_mask=mask, past_key_values=cache, use_cache=True).logits
    assert len(spy) == 4 * layers + 1
    assert torch.isfinite(lg.float()).all()
    assert torch.equal(cache.lengths - before, mask[:, 0].to(torch.int32))
    # generate() keeping the cache compact, on the decode graph
    del spy[:]
    cfg = O.config_small_gpu()
    ids, amask, pix, _ = O.make_inputs(cfg, B, 8, 3, 77)
    out = m.generate(input_ids=ids.to(DEV), pixel_values=pix.to(DEV), attention_mask=amask.to(DEV), max_new_tokens=3,
                     compact_cache=True, kv_cache_dtype="fp8_sim")
    assert out.shape[0] == B and len(spy) >= 4 * layers + 1


def test_adapters_arrive_as_the_addend(monkeypatch, spy):
    from cullavo_amd import generation
    m = _model("lora")
    B = 17
    layers = O.config_small_gpu().text.num_hidden_layers
    monkeypatch.setattr(generation, "DECODE_WIDE", True)
    on = _steps(m, B)
    # every layer product carries its group's term; gate|up is the plain product (the SwiGLU its own launch)
    per_step = [(0, True, False), (0, True, True), (0, True, False), (0, True, True)] * layers + [(0, False, False)]
    assert spy == per_step * STEPS
    monkeypatch.setattr(generation, "DECODE_WIDE", False)
    off = _steps(m, B)
    for i, (a, b) in enumerate(zip(on, off)):
        r = rel_l2(a, b)
        print(f"lora B {B} step {i}: wide vs tiled logits rel-L2 {r:.3e}")
        assert r <= 1e-2, (i, r)
