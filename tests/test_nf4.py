"""NF4 base weights (csrc/nf4.hip, quant.py): the format against a numpy restatement, the decode
product against float64, and the quantised model's decode step, graph and LoRA paths.

bitsandbytes is not a dependency; the format is restated here in numpy (f32 arithmetic where the
format says f32, float64 for the references):
  block     64 consecutive k of one row of W [N, K], K % 64 == 0
  absmax    f32 [N, K/64] = max |w| of the block; an all-zero block: 0, code 7, dequantises to 0
  x         f32(w) / absmax, IEEE f32 division
  code      #{j : x > m_j}, m_j = (L[j] + L[j+1]) / 2 in f32, L = QLoRA's NF4 code book
  packing   uint8 [N, K/2], byte i = element 2i (high nibble) | element 2i+1 (low nibble)
  value     bf16_rne(L[code] * absmax), the product in f32

Measured on the MI355X (profiles/r07/nf4/README_r07.txt): test 3's max |y - y64| / gate is 0.989 for
the NF4 product (K = 64, where the gate is the bf16 output rounding alone) and 92.9 for the bf16
GEMV on the arena's rounded weights (printed, not asserted); test 4b's logits rel-L2 is 6.5e-3
(B = 1) and 7.9e-3 (B = 3, left-padded), with LoRA adapters 8.2e-3 / 7.5e-3, under the 1e-2 gate.
The tiny model's shapes are not in ops.NF4_BF16_FASTER, so every product of test 4 runs the NF4 kernel.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import cullavo_oracle as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

L = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
              -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
              0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941,
              0.7229568362236023, 1.0], dtype=np.float32)
MID = ((L[:-1] + L[1:]) / np.float32(2)).astype(np.float32)
assert MID.dtype == np.float32


# ---- the restatement -----------------------------------------------------------------------------
def bf16_bits(x: np.ndarray) -> np.ndarray:
    """f32 -> bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def round_bf(x: np.ndarray) -> np.ndarray:
    return bf16_val(bf16_bits(np.asarray(x, dtype=np.float32)))


def pack(code: np.ndarray) -> np.ndarray:
    return ((code[:, 0::2].astype(np.uint8) << 4) | code[:, 1::2].astype(np.uint8)).astype(np.uint8)


def unpack(packed: np.ndarray) -> np.ndarray:
    out = np.empty((packed.shape[0], packed.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2] = packed >> 4
    out[:, 1::2] = packed & 15
    return out


def ref_quantize(w: np.ndarray):
    """w f32 [N, K] (bf16 values) -> (code [N, K] uint8 unpacked, absmax f32 [N, K/64], x f32 [N, K])"""
    N, K = w.shape
    blocks = w.reshape(N, K // 64, 64)
    absmax = np.abs(blocks).max(-1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (blocks / absmax[..., None]).astype(np.float32)
    assert x.dtype == np.float32
    code = (x[..., None] > MID).sum(-1).astype(np.uint8)
    code[absmax == 0] = 7
    return code.reshape(N, K), absmax, x.reshape(N, K)


def ref_dequantize_bits(code: np.ndarray, absmax: np.ndarray) -> np.ndarray:
    prod = L[code] * np.repeat(absmax, 64, axis=1)
    assert prod.dtype == np.float32
    return bf16_bits(prod)


def t_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.view(np.int16).copy()).view(BF)


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


SHAPES = [(N, K) for N in (8, 16, 40) for K in (64, 192, 4096)]


# ---- 1. dequantise is bitwise --------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
def test_dequantize_bitwise(N, K):
    from cullavo_amd import ops
    rng = np.random.default_rng(100 + N + K)
    code = rng.integers(0, 16, (N, K), dtype=np.uint8)
    absmax = rng.uniform(1e-3, 4.0, (N, K // 64)).astype(np.float32)
    absmax[N // 2, (K // 64) // 2] = 0.0
    want = ref_dequantize_bits(code, absmax)
    c, a = torch.from_numpy(pack(code)).cuda(), torch.from_numpy(absmax).cuda()
    got = ops.nf4_dequantize(c, a)
    assert got.dtype == BF and np.array_equal(bits_of(got), want)
    assert (got[N // 2, 64 * ((K // 64) // 2):64 * ((K // 64) // 2 + 1)] == 0).all()
    if (N, K) == (40, 192):  # ldw > K: into a strided view, the columns past K untouched
        big = torch.full((N, K + 8), 3.0, dtype=BF, device="cuda")
        ops.nf4_dequantize(c, a, out=big[:, :K])
        assert np.array_equal(bits_of(big[:, :K]), want) and (big[:, K:] == 3.0).all()


# ---- 2. quantise ---------------------------------------------------------------------------------
def _quant_input(N, K, seed=7):
    g = torch.Generator().manual_seed(seed * 1000 + N * 7 + K)
    w = torch.randn(N, K, generator=g).to(BF)
    w[1, :64] = 0  # an all-zero block
    am = w[2, :64].abs().max()
    w[2, 0], w[2, 63] = am, -am  # +-absmax at the block ends
    return w


@pytest.mark.parametrize("N,K", SHAPES)
def test_quantize(N, K):
    from cullavo_amd import ops
    w = _quant_input(N, K)
    code, absmax, x = ref_quantize(w.float().numpy())
    # elements within 2^-22 of a midpoint may round either way in another division sequence; the
    # seed is chosen so the restatement has none at these shapes (checked on the CPU)
    near = (np.abs(x.astype(np.float64)[..., None] - MID.astype(np.float64)) <= 2.0 ** -22).any(-1)
    assert near.sum() <= 1e-4 * near.size
    c, a = ops.nf4_quantize(w.cuda())
    assert c.dtype == torch.uint8 and a.dtype == torch.float32
    assert np.array_equal(a.cpu().numpy().view(np.uint32), absmax.view(np.uint32))
    got = unpack(c.cpu().numpy())
    assert not ((got != code) & ~near).any()
    assert (got[1, :64] == 7).all() and absmax[1, 0] == 0
    assert got[2, 0] == 15 and got[2, 63] == 0
    # round trip: half the widest code-book gap of absmax, plus the bf16 rounding of the value
    back = ops.nf4_dequantize(c, a).float().cpu().numpy().astype(np.float64)
    w64 = w.float().numpy().astype(np.float64)
    bound = np.repeat(absmax.astype(np.float64), 64, axis=1) * float(np.diff(L.astype(np.float64)).max()) / 2 \
        + 2.0 ** -8 * np.abs(w64)
    assert (np.abs(back - w64) <= bound).all()
    if (N, K) == (40, 192):  # a strided source
        big = torch.zeros(N, K + 8, dtype=BF, device="cuda")
        big[:, :K] = w.cuda()
        c2, a2 = ops.nf4_quantize(big[:, :K])
        assert torch.equal(c2, c) and torch.equal(a2, a)


# ---- 3. the decode product against float64 -------------------------------------------------------
_CASE = {}


def _case(N, K):
    """random codes / absmax of a [2N, K] weight (one zero absmax), shared by the tests of a shape"""
    if _CASE.get("key") != (N, K):
        rng = np.random.default_rng(N * 131 + K)
        code = rng.integers(0, 16, (2 * N, K), dtype=np.uint8)
        absmax = rng.uniform(0.01, 0.1, (2 * N, K // 64)).astype(np.float32)
        absmax[N // 3, 0] = 0.0
        _CASE.clear()
        _CASE.update(key=(N, K), code=code, absmax=absmax, c=torch.from_numpy(pack(code)).cuda(),
                     a=torch.from_numpy(absmax).cuda())
    return _CASE


def _ref_product(x64, code, absmax):
    """(X dq(W)^T, |X| |dq(W)|^T) in f64 on the unrounded weights L[code] * absmax, by row chunks"""
    y = np.empty((x64.shape[0], code.shape[0]))
    ya = np.empty_like(y)
    ax = np.abs(x64)
    for r0 in range(0, code.shape[0], 1024):
        w = L.astype(np.float64)[code[r0:r0 + 1024]] * np.repeat(absmax[r0:r0 + 1024].astype(np.float64), 64, axis=1)
        y[:, r0:r0 + 1024] = x64 @ w.T
        ya[:, r0:r0 + 1024] = ax @ np.abs(w).T
    return y, ya


def _ulp_bf16(v):
    """one bf16 ulp at |v| (f64 array)"""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126))) - 7)


def _ratio(err, gate):
    """err / gate for the printed maxima (a zero-absmax row: the reference, the gate and the result are 0)"""
    return np.divide(err, gate, out=np.where(err > 0, np.inf, 0.0), where=gate > 0)


def _silu(v):
    return v / (1.0 + np.exp(-v))


@pytest.mark.parametrize("K", [64, 192, 4096, 11008])
@pytest.mark.parametrize("N", [16, 40, 4096])
@pytest.mark.parametrize("M", [1, 5, 16])
def test_decode_linear_f64(M, N, K):
    from cullavo_amd import ops
    cs = _case(N, K)
    g = torch.Generator().manual_seed(M * 17 + N + K)
    x = torch.randn(M, K, generator=g).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    add = (0.1 * torch.randn(M, N, generator=g)).to(BF)
    x64 = x.float().numpy().astype(np.float64)
    y64, ya = _ref_product(x64, cs["code"], cs["absmax"])
    # the gate: a bf16 output half-ulp (2^-9) with a factor 2, plus the f32 accumulation with the
    # per-block scale FMA, K 2^-23 of the absolute product
    gate = 2.0 ** -8 * np.abs(y64) + K * 2.0 ** -23 * ya
    xc = x.cuda()
    c1, a1 = cs["c"][:N], cs["a"][:N]

    def out(**kw):
        return ops.nf4_decode_linear(xc, c1, a1, **kw).float().cpu().numpy().astype(np.float64)

    # plain
    y = out()
    ratio = _ratio(np.abs(y - y64[:, :N]), gate[:, :N])
    # the margin note's other path: the bf16 GEMV on the arena's bf16(L * absmax) weights (printed,
    # not asserted: its weights carry a 2^-9 relative rounding the gate does not allow for)
    yb = ops.linear(xc, ops.nf4_dequantize(c1, a1)).float().cpu().numpy().astype(np.float64)
    print(f"nf4 decode M={M} N={N} K={K}: max err/gate nf4 {ratio.max():.3f}, "
          f"bf16 GEMV on dequantised weights {_ratio(np.abs(yb - y64[:, :N]), gate[:, :N]).max():.3f}")
    assert (np.abs(y - y64[:, :N]) <= gate[:, :N]).all(), ratio.max()
    # residual / addend: each is added to the bf16-rounded product and the sum rounded again
    # (ops.linear's roundings): the gate before the term, one more bf16 ulp after it
    for name, t in (("residual", res), ("addend", add)):
        ref = y64[:, :N] + t.float().numpy().astype(np.float64)
        y = out(**{name: t.cuda()})
        tol = gate[:, :N] + _ulp_bf16(ref)
        assert (np.abs(y - ref) <= tol).all(), (name, _ratio(np.abs(y - ref), tol).max())
    # both, in store4's order: bf16(bf16(bf16(acc) + addend) + residual)
    ref = y64[:, :N] + add.float().numpy().astype(np.float64)
    tol = gate[:, :N] + _ulp_bf16(ref)
    ref2 = ref + res.float().numpy().astype(np.float64)
    y = out(residual=res.cuda(), addend=add.cuda())
    assert (np.abs(y - ref2) <= tol + _ulp_bf16(ref2)).all()
    # SwiGLU output on the [2N, K] weight: y = bf16(bf16(silu(bf16(g))) * bf16(u)). With g, u inside
    # their gates (which hold their bf16 roundings), silu' <= 1.1 and |silu(g)| <= |g|:
    # |dy| <= 1.1 (|u| + gate_u) gate_g + |silu(g)| gate_u, then the two roundings of the epilogue
    # (2^-9 each, relative) within one bf16 ulp of the result
    g64, u64 = y64[:, :N], y64[:, N:]
    gg, gu = gate[:, :N], gate[:, N:]
    ref = _silu(g64) * u64
    tol = 1.1 * (np.abs(u64) + gu) * gg + np.abs(_silu(g64)) * gu + _ulp_bf16(np.abs(ref) + 1.1 * (np.abs(u64) + gu) * gg
                                                                                + np.abs(_silu(g64)) * gu)
    y = ops.nf4_decode_linear(xc, cs["c"], cs["a"], swiglu_out=True)
    assert y.shape == (M, N)
    y = y.float().cpu().numpy().astype(np.float64)
    assert (np.abs(y - ref) <= tol).all(), _ratio(np.abs(y - ref), tol).max()


def test_decode_linear_deterministic_and_rejections():
    from cullavo_amd import ops
    cs = _case(40, 192)
    x = torch.randn(16, 192, generator=torch.Generator().manual_seed(3)).to(BF).cuda()
    c, a = cs["c"][:40], cs["a"][:40]
    assert torch.equal(ops.nf4_decode_linear(x, c, a), ops.nf4_decode_linear(x, c, a))
    cs = _case(4096, 4096)
    x = torch.randn(5, 4096, generator=torch.Generator().manual_seed(4)).to(BF).cuda()
    r = torch.randn(5, 4096, generator=torch.Generator().manual_seed(5)).to(BF).cuda()
    c, a = cs["c"][:4096], cs["a"][:4096]
    assert torch.equal(ops.nf4_decode_linear(x, c, a, residual=r), ops.nf4_decode_linear(x, c, a, residual=r))
    with pytest.raises(ValueError, match="M <= 16"):
        ops.nf4_decode_linear(torch.zeros(17, 4096, dtype=BF, device="cuda"), c, a)
    with pytest.raises(ValueError, match="64"):  # K = 96
        ops.nf4_decode_linear(torch.zeros(1, 96, dtype=BF, device="cuda"),
                              torch.zeros(16, 48, dtype=torch.uint8, device="cuda"),
                              torch.zeros(16, 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="64"):
        ops.nf4_quantize(torch.zeros(16, 96, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.nf4_decode_linear(torch.zeros(1, 4096, dtype=BF), c.cpu(), a.cpu())
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.nf4_quantize(torch.zeros(16, 64, dtype=BF))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.nf4_dequantize(c.cpu(), a.cpu())


def test_decode_linear_checks_epilogue_operands():
    """residual / addend must be bf16 [M, N] (N after the SwiGLU halving: not accepted there at all)"""
    from cullavo_amd import ops
    cs = _case(40, 192)
    c, a = cs["c"][:40], cs["a"][:40]
    x = torch.zeros(5, 192, dtype=BF, device="cuda")
    ok = torch.zeros(5, 40, dtype=BF, device="cuda")
    for name in ("residual", "addend"):
        with pytest.raises(TypeError, match="bf16"):
            ops.nf4_decode_linear(x, c, a, **{name: ok.float()})
        with pytest.raises(ValueError, match="expected"):
            ops.nf4_decode_linear(x, c, a, **{name: ok[:4]})
        with pytest.raises(ValueError, match="expected"):
            ops.nf4_decode_linear(x, c, a, **{name: torch.zeros(5, 48, dtype=BF, device="cuda")})
        with pytest.raises(ValueError, match="SwiGLU"):
            ops.nf4_decode_linear(x, cs["c"], cs["a"], swiglu_out=True, **{name: ok})
    with pytest.raises(ValueError, match="aligned"):
        ops.nf4_decode_linear(torch.zeros(5, 200, dtype=BF, device="cuda")[:, 4:196], c, a)
    with pytest.raises(ValueError, match="bf16 \\[40, 192\\]"):
        ops.nf4_decode_linear(x, c, a, w=torch.zeros(40, 128, dtype=BF, device="cuda"))


def test_decode_linear_routes_measured_losers_to_bf16(monkeypatch):
    """Given the dequantised weight, a shape listed in ops.NF4_BF16_FASTER runs the bf16 GEMV on it
    (bitwise ops.linear / decode_linear transform 3) up to the listed M and the NF4 product above it;
    an unlisted shape, or no weight, always takes the NF4 product."""
    from cullavo_amd import ops
    assert ops.nf4_prefers_bf16(12288, 4096, 1) and not ops.nf4_prefers_bf16(12288, 4096, 16)
    assert ops.nf4_prefers_bf16(22016, 4096, 8) and not ops.nf4_prefers_bf16(22016, 4096, 16)
    assert not ops.nf4_prefers_bf16(4096, 4096, 1) and not ops.nf4_prefers_bf16(4096, 11008, 1)
    cs = _case(40, 192)
    x = torch.randn(5, 192, generator=torch.Generator().manual_seed(8)).to(BF).cuda()
    r = torch.randn(5, 40, generator=torch.Generator().manual_seed(9)).to(BF).cuda()
    c1, a1 = cs["c"][:40], cs["a"][:40]
    w1, w2 = ops.nf4_dequantize(c1, a1), ops.nf4_dequantize(cs["c"], cs["a"])
    nf = ops.nf4_decode_linear(x, c1, a1, residual=r)
    assert torch.equal(ops.nf4_decode_linear(x, c1, a1, residual=r, w=w1), nf)  # unlisted: NF4
    monkeypatch.setitem(ops.NF4_BF16_FASTER, (40, 192), 5)
    monkeypatch.setitem(ops.NF4_BF16_FASTER, (80, 192), 5)
    assert torch.equal(ops.nf4_decode_linear(x, c1, a1, residual=r, w=w1), ops.linear(x, w1, residual=r))
    assert torch.equal(ops.nf4_decode_linear(x, c1, a1, residual=r, addend=r, w=w1),
                       ops.linear(x, w1, residual=r, addend=r))
    assert torch.equal(ops.nf4_decode_linear(x, cs["c"], cs["a"], swiglu_out=True, w=w2),
                       ops.decode_linear(x, w2, transform=3))
    assert torch.equal(ops.nf4_decode_linear(x, c1, a1, residual=r), nf)  # no weight given: NF4
    monkeypatch.setitem(ops.NF4_BF16_FASTER, (40, 192), 4)  # M = 5 is above the listed rows
    assert torch.equal(ops.nf4_decode_linear(x, c1, a1, residual=r, w=w1), nf)


# ---- 4. model level ------------------------------------------------------------------------------
def _cfg(F=704):
    from cullavo_amd.config import tiny_gpu
    cfg = tiny_gpu()
    return dataclasses.replace(cfg, text_config=dataclasses.replace(cfg.text_config, intermediate_size=F))


def _model(F=704, trainable="none", seed=6):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    m = CuLLaVOModel(_cfg(F), device="cuda", trainable=trainable, init="random", seed=seed)
    if trainable == "lora":  # lora_B starts at zero: make the adapters' term count
        g = torch.Generator(device="cuda").manual_seed(seed)
        ar = m.arenas["lora"]
        ar.flat.copy_((0.05 * torch.randn(ar.numel, generator=g, device="cuda")).to(ar.dtype))
    m.eval()
    return m


def _prompt(B):
    """(ids, mask, pix): B = 1 one unpadded row; B = 3 rows left-padded by 5, 2 and 0 tokens"""
    cfg = O.config_small_gpu()
    ids, mask, pix, _ = O.make_inputs(cfg, 1, 20, 3, 13)
    if B == 1:
        return ids.cuda(), mask.cuda(), pix.cuda()
    rows_i, rows_m = [], []
    for b, npad in enumerate((5, 2, 0)):
        extra = torch.randint(2, cfg.image_token_index, (1, 5 - npad), generator=torch.Generator().manual_seed(b))
        rows_i.append(torch.cat([torch.full((1, npad), cfg.pad_token_id), extra, ids], 1))
        rows_m.append(torch.cat([torch.zeros(1, npad, dtype=mask.dtype), torch.ones(1, 5 - npad, dtype=mask.dtype), mask], 1))
    return torch.cat(rows_i, 0).cuda(), torch.cat(rows_m, 0).cuda(), torch.cat([pix] * 3, 0).cuda()


def _rel_l2(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm()).item()


QUANT_KEYS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def test_quantize_lm_arena_and_idempotence():
    from cullavo_amd import ops
    from cullavo_amd.quant import nf4_weights, quantize_lm_nf4_
    m = _model()
    before = {k: p.detach().clone() for k, p in m.state_dict().items()}
    rep = quantize_lm_nf4_(m)
    n_layers = m.config.text_config.num_hidden_layers
    assert len(rep["quantized"]) == 7 * n_layers and not rep["skipped"]
    assert 3.5 < rep["bf16_bytes"] / rep["nf4_bytes"] < 3.6  # 16 / 4.5 bits
    after = m.state_dict()
    for k, p in after.items():
        if ".layers." in k and k.startswith("language_model") and any(q in k for q in QUANT_KEYS):
            assert k in rep["quantized"]
            assert not torch.equal(p, before[k]), k
        else:  # lm_head, projector, norms, embeddings, the vision tower
            assert k not in rep["quantized"] and torch.equal(p, before[k]), k
    # (a) every quantised arena weight is the dequantised NF4 copy, bit for bit
    for layer in m.language_model.model.layers:
        q = nf4_weights(layer)
        assert set(q) == {"qkv", "o", "gu", "down"}
        for which, (key, shape) in layer._kmajor_specs().items():
            assert torch.equal(ops.nf4_dequantize(*q[which]), layer._arena.view(key, shape)), (key, which)
    # (f) a second call changes no bit
    snap = {k: p.detach().clone() for k, p in after.items()}
    copies = [[t.clone() for t in q] for layer in m.language_model.model.layers for q in nf4_weights(layer).values()]
    rep2 = quantize_lm_nf4_(m)
    assert not rep2["quantized"] and sorted(rep2["kept"]) == sorted(rep["quantized"])
    for k, p in m.state_dict().items():
        assert torch.equal(p, snap[k]), k
    again = [q for layer in m.language_model.model.layers for q in nf4_weights(layer).values()]
    assert all(torch.equal(x, y) for q0, q1 in zip(copies, again) for x, y in zip(q0, q1))
    # a write to the base weights (a checkpoint load, an optimizer step) drops the copies
    m.load_state_dict(before)
    with pytest.warns(RuntimeWarning, match="NF4 copies are dropped"):
        assert all(not nf4_weights(layer) for layer in m.language_model.model.layers)


def _decode_step(m, B, nf4_on, monkeypatch):
    from cullavo_amd import generation
    monkeypatch.setattr(generation, "NF4_DECODE", nf4_on)
    ids, mask, pix = _prompt(B)
    cache = m(input_ids=ids, pixel_values=pix, attention_mask=mask, use_cache=True).past_key_values
    tok = torch.randint(2, 1000, (B, 1), generator=torch.Generator().manual_seed(9)).cuda()
    return m(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].clone()


@pytest.mark.parametrize("trainable", ["none", "lora"])
@pytest.mark.parametrize("B", [1, 3])
def test_model_decode_step_matches_bf16_gemv(monkeypatch, B, trainable):
    """(b), (d): one cached decode step on the NF4 copies against the bf16 GEMV on the same
    (dequantised) arena weights, under the project's bf16 logits gate (rel-L2 <= 1e-2)."""
    from cullavo_amd import ops
    from cullavo_amd.quant import quantize_lm_nf4_
    m = _model(trainable=trainable)
    quantize_lm_nf4_(m)
    calls = []
    real = ops.nf4_decode_linear
    monkeypatch.setattr(ops, "nf4_decode_linear", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    a = _decode_step(m, B, True, monkeypatch)
    n = len(calls)
    assert n == 4 * m.config.text_config.num_hidden_layers
    if trainable == "lora":
        assert sum(k.get("addend") is not None for k in calls) == n and not any(k.get("swiglu_out") for k in calls)
    else:
        assert sum(bool(k.get("swiglu_out")) for k in calls) == n // 4
    b = _decode_step(m, B, False, monkeypatch)
    assert len(calls) == n  # CULLAVO_NF4_DECODE=0: the bf16 GEMV
    rel = _rel_l2(a, b)
    print(f"nf4 decode step B={B} trainable={trainable}: logits rel-L2 vs bf16 GEMV {rel:.3e}")
    assert rel <= 1e-2, rel


def test_model_generate_graph_equals_eager():
    """(c): greedy generate through the captured decode graph is the eager loop, token for token"""
    from cullavo_amd.quant import quantize_lm_nf4_
    m = _model()
    quantize_lm_nf4_(m)
    ids, mask, pix = _prompt(3)
    kw = dict(input_ids=ids, pixel_values=pix, attention_mask=mask, max_new_tokens=8)
    assert torch.equal(m.generate(**kw), m.generate(**kw, decode_graph=False))


def test_model_skips_unaligned_down_proj(monkeypatch):
    """(e): the plain tiny config (intermediate 688: down_proj's K % 64 != 0) keeps down_proj bf16"""
    from cullavo_amd.quant import nf4_weights, quantize_lm_nf4_
    m = _model(F=688)
    rep = quantize_lm_nf4_(m)
    n_layers = m.config.text_config.num_hidden_layers
    assert len(rep["skipped"]) == n_layers and all("down_proj" in k for k in rep["skipped"])
    assert all(set(nf4_weights(layer)) == {"qkv", "o", "gu"} for layer in m.language_model.model.layers)
    a = _decode_step(m, 1, True, monkeypatch)
    b = _decode_step(m, 1, False, monkeypatch)
    assert torch.isfinite(a).all() and _rel_l2(a, b) <= 1e-2
    ids, mask, pix = _prompt(1)
    out = m.generate(input_ids=ids, pixel_values=pix, attention_mask=mask, max_new_tokens=4)
    assert out.shape == (1, 24)
