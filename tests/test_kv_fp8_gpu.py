"""The FP8 KV cache on the GPU (INTEGRATION.md "FP8 KV cache"): the quantising appends, decode
attention on codes, the dequantisation and the whole model, held to the CPU restatements of
tests/kv_fp8_refs.py (shown honest, with failing mutants, by tests/test_kv_fp8_refs_host.py).

With power-of-two scales every dequantised value is a bf16 number, so an fp8 cache is arithmetically
a bf16 cache holding those values: the checks are bitwise against the bf16 kernels that
tests/test_decode_accuracy_gpu.py pins against float64.
"""
import json
import os

import pytest
import torch

from oracle import cullavo_oracle as O
from tests import decode_refs as R
from tests import kv_fp8_refs as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
H, D, B = F.H_TEST, R.D_HEAD, F.B_TEST
HD = H * D
SCALE = D ** -0.5
SENT_CODE, SENT_EXP = 0xAB, 0xCD
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int16)


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32)


def frames(Lmax):
    """sentinel-filled caches on the CPU: codes [B, Lmax, HD], exponents [B, Lmax, H] (K and V)"""
    c = torch.full((B, Lmax, HD), SENT_CODE, dtype=torch.uint8)
    e = torch.full((B, Lmax, H), SENT_EXP, dtype=torch.uint8)
    return c, c.clone(), e, e.clone()


# ---------------------------------------------------------------------------------------------
# 1. appends
# ---------------------------------------------------------------------------------------------
STARTS = (0, 63, 64)


def _expected_append(k, v, start, Lnew, q_pad, Lmax):
    kc, vc, ke, ve = frames(Lmax)
    kq, keq = F.quantise(k, H, D)
    vq, veq = F.quantise(v, H, D)
    for b in range(B):
        pad = int(q_pad[b]) if q_pad is not None else 0
        for t in range(pad, Lnew):
            r = int(start[b]) + t - pad
            kc[b, r], vc[b, r] = kq[b * Lnew + t], vq[b * Lnew + t]
            ke[b, r], ve[b, r] = keq[b * Lnew + t], veq[b * Lnew + t]
    return kc, vc, ke, ve


@pytest.mark.parametrize("Lnew", [1, 5, 70])
def test_append_codes_and_exponents_bit_exact(Lnew):
    """uniform and ragged appends inside sentinel frames: owned rows hold the restatement's codes and
    exponents, every other byte keeps its sentinel. The projection rows are column blocks of wider rows."""
    k, v = F.append_rows(Lnew)
    wide = torch.zeros(B * Lnew, 3 * HD, dtype=BF)
    wide[:, HD:2 * HD], wide[:, 2 * HD:] = k, v
    wide = wide.to(DEV)
    kd, vd = wide[:, HD:2 * HD], wide[:, 2 * HD:]
    Lmax = max(STARTS) + Lnew + 3
    start = i32(STARTS)
    for q_pad in (None, i32([0] * B), i32([0, min(3, Lnew), Lnew])):
        got = [t.to(DEV) for t in frames(Lmax)]
        if q_pad is None:
            ops().kv_append_fp8(kd, vd, *got, start.to(DEV), B=B, Lnew=Lnew, H=H, D=D)
        else:
            ops().kv_append_ragged_fp8(kd, vd, *got, start.to(DEV), q_pad.to(DEV), B=B, Lnew=Lnew, H=H, D=D)
        want = _expected_append(k, v, start, Lnew, q_pad, Lmax)
        for name, g, w in zip(("k codes", "v codes", "k exp", "v exp"), got, want):
            assert torch.equal(g.cpu(), w), (name, Lnew, q_pad)


@pytest.mark.parametrize("Lnew", [1, 5])
def test_append_round_trip_twin(Lnew):
    """sim: the bf16 cache receives the dequantised values, nothing else is written"""
    k, v = F.append_rows(Lnew)
    Lmax = max(STARTS) + Lnew + 3
    start = i32(STARTS)
    sent = torch.full((B, Lmax, HD), -7.0, dtype=BF)
    kc, vc = sent.clone().to(DEV), sent.clone().to(DEV)
    ops().kv_append_fp8(k.to(DEV), v.to(DEV), kc, vc, None, None, start.to(DEV), B=B, Lnew=Lnew, H=H, D=D, sim=True)
    wk, wv = sent.clone(), sent.clone()
    fk, fv = F.fake_quant(k, H, D), F.fake_quant(v, H, D)
    for b in range(B):
        wk[b, STARTS[b]:STARTS[b] + Lnew] = fk[b * Lnew:(b + 1) * Lnew]
        wv[b, STARTS[b]:STARTS[b] + Lnew] = fv[b * Lnew:(b + 1) * Lnew]
    assert torch.equal(bits(kc.cpu()), bits(wk)) and torch.equal(bits(vc.cpu()), bits(wv))


@pytest.mark.parametrize("Lnew", [1, 5])
def test_rope_append_equals_rope_then_append(Lnew):
    k, v = F.append_rows(Lnew)
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B * Lnew, HD, generator=g).to(BF)
    pos = torch.randint(0, 3000, (B * Lnew,), generator=g)
    Lmax = max(STARTS) + Lnew + 3
    start = i32(STARTS).to(DEV)
    a = [t.to(DEV) for t in frames(Lmax)]
    b = [t.to(DEV) for t in frames(Lmax)]
    qa, ka = q.to(DEV), k.to(DEV)
    ops().rope_kv_append_fp8(qa, ka, v.to(DEV), pos.to(DEV), *a, start, hq=H, head_dim=D, theta=R.THETA, B=B, Lnew=Lnew)
    assert torch.equal(bits(ka.cpu()), bits(k))  # k itself is left unrotated
    qb, kb = q.to(DEV), k.to(DEV)
    ops().rope(qb, kb, pos.to(DEV), hq=H, hk=H, head_dim=D, theta=R.THETA)
    ops().kv_append_fp8(kb, v.to(DEV), *b, start, B=B, Lnew=Lnew, H=H, D=D)
    assert torch.equal(bits(qa), bits(qb))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # and against the restatement of the rotated keys
    want_k, want_e = F.quantise(kb.cpu(), H, D)
    for bb in range(B):
        assert torch.equal(a[0][bb, STARTS[bb]:STARTS[bb] + Lnew].cpu(), want_k[bb * Lnew:(bb + 1) * Lnew])
        assert torch.equal(a[2][bb, STARTS[bb]:STARTS[bb] + Lnew].cpu(), want_e[bb * Lnew:(bb + 1) * Lnew])


def test_argument_errors_before_launch():
    k, v = (t.to(DEV) for t in F.append_rows(1))
    kc, vc, ke, ve = (t.to(DEV) for t in frames(8))
    start = i32([0] * B).to(DEV)
    with pytest.raises(ValueError, match="exponents"):
        ops().kv_append_fp8(k, v, kc, vc, None, None, start, B=B, Lnew=1, H=H, D=D)
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        ops().kv_append_fp8(k, v, kc, vc, ke, ve, start, B=B, Lnew=1, H=4, D=64)
    from cullavo_amd._lib import call
    args = (k.data_ptr(), HD, v.data_ptr(), HD, kc.data_ptr(), vc.data_ptr(), HD, 8 * HD)
    tail = (H, 8 * H, start.data_ptr(), B, 1, H)
    with pytest.raises(ValueError, match="exponent"):  # null exponents at the C-ABI
        call("kv_append_fp8", *args, None, None, *tail, D, 0, None)
    with pytest.raises(ValueError, match="aligned"):  # a misaligned code pointer
        call("kv_append_fp8", k.data_ptr(), HD, v.data_ptr(), HD, kc.data_ptr() + 8, vc.data_ptr(), HD, 8 * HD,
             ke.data_ptr(), ve.data_ptr(), *tail, D, 0, None)
    from cullavo_amd._lib import CullavoError
    with pytest.raises(CullavoError, match="head_dim 128"):
        call("kv_append_fp8", *args, ke.data_ptr(), ve.data_ptr(), *tail, 64, 0, None)
    assert bool((kc == SENT_CODE).all()) and bool((ke == SENT_EXP).all())  # nothing was launched


# ---------------------------------------------------------------------------------------------
# 2. decode attention on codes
# ---------------------------------------------------------------------------------------------
def _attn_case(name):
    max_len, pairs = R.ATTN_CASES[name]
    nb = len(pairs)
    q, kc, vc = R.attn_inputs(name, max_len, nb, H=H)
    ks, kl = i32(p[0] for p in pairs), i32(p[1] for p in pairs)
    kcodes, ke = F.quantise(kc.contiguous(), H, D)
    vcodes, ve = F.quantise(vc.contiguous(), H, D)
    vis = R.window(ks, kl, max_len)
    return max_len, nb, q, F.poison_outside(kcodes, vcodes, ke, ve, vis), (kcodes, vcodes, ke, ve), ks, kl


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attn_decode_fp8_bitwise_bf16_on_dequantised(name):
    """windows on every 64-key chunk edge, wholly masked chunks, an empty window, the 33-chunk combine
    loop; every row outside [kv_start, kv_len) is poisoned (code 0x7F = NaN, exponent 255)"""
    max_len, nb, q, poisoned, clean, ks, kl = _attn_case(name)
    pk, pv, pke, pve = (t.to(DEV) for t in poisoned)
    qd, ksd, kld = q.to(DEV), ks.to(DEV), kl.to(DEV)
    kw = dict(B=nb, H=H, D=D, max_len=max_len, scale=SCALE, kv_start=ksd)
    o8 = ops().attn_decode_fp8(qd, pk, pv, pke, pve, kld, **kw)
    kd, vd = ops().kv_dequant_fp8(pk, pv, pke, pve, rows=max_len, H=H, D=D)
    o16 = ops().attn_decode(qd, kd, vd, kld, **kw)
    assert torch.equal(bits(o8), bits(o16))
    assert not bool(torch.isnan(o8.float()).any())
    empty = kl <= ks
    assert bool((o8.cpu()[empty].float() == 0).all())
    if name == "starts576":  # and against f64 softmax on the dequantised cache, at decode_refs' gate
        kdq, vdq = F.dequantise(clean[0], clean[2], H, D), F.dequantise(clean[1], clean[3], H, D)
        ref, pv_abs, n = R.decode_attn_ref(q, kdq, vdq, ks, kl, SCALE)
        w, zero_ok = R.attn_gate(o8.cpu(), ref, pv_abs, n)
        print(f"attn_decode_fp8 {name}: worst err/gate {w:.3f}")
        assert w <= 1.0 and zero_ok


@pytest.mark.parametrize("name", list(R.DECODE_ROPE_SETS))
def test_fused_rope_step_equals_unfused(name):
    """attn_decode_rope_fp8 == rope_kv_append_fp8 + attn_decode_fp8: output, the new row's codes and
    exponents, and nothing else written; the round-trip twin (sim) gives the same output and leaves
    the dequantised row in its bf16 cache"""
    qkv, kbuf, vbuf, start, kv_start, pos, max_len = R.decode_rope_inputs(name, 1, H=H)
    nb = start.shape[0]
    kcodes, ke = F.quantise(kbuf.contiguous(), H, D)
    vcodes, ve = F.quantise(vbuf.contiguous(), H, D)
    qkv, start, kv_start, pos = qkv.to(DEV), start.to(DEV), kv_start.to(DEV), pos.to(DEV)
    q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
    kw = dict(B=nb, H=H, D=D, max_len=max_len, scale=SCALE, kv_start=kv_start)
    a = [t.clone().to(DEV) for t in (kcodes, vcodes, ke, ve)]
    oa = ops().attn_decode_rope_fp8(q, k, v, pos, *a, start, theta=R.THETA, **kw)
    b = [t.clone().to(DEV) for t in (kcodes, vcodes, ke, ve)]
    q2 = q.clone()
    ops().rope_kv_append_fp8(q2, k, v, pos, *b, start, hq=H, head_dim=D, theta=R.THETA, B=nb, Lnew=1)
    ob = ops().attn_decode_fp8(q2, *b, start + 1, **kw)
    assert torch.equal(bits(oa), bits(ob))
    for x, y, orig in zip(a, b, (kcodes, vcodes, ke, ve)):
        assert torch.equal(x, y)
        changed = (x.cpu() != orig).any(-1)
        assert bool((changed.sum(1) <= 1).all())  # at most the new row of each sequence
    kd, vd = ops().kv_dequant_fp8(*[t.to(DEV) for t in (kcodes, vcodes, ke, ve)], rows=max_len, H=H, D=D)
    kd, vd = kd.contiguous(), vd.contiguous()
    osim = ops().attn_decode_rope_fp8(q, k, v, pos, kd, vd, None, None, start, theta=R.THETA, sim=True, **kw)
    assert torch.equal(bits(osim), bits(oa))
    ka, va = ops().kv_dequant_fp8(*a, rows=max_len, H=H, D=D)
    assert torch.equal(bits(kd), bits(ka)) and torch.equal(bits(vd), bits(va))


# ---------------------------------------------------------------------------------------------
# 3. dequantisation and the multi-token routes through the slab
# ---------------------------------------------------------------------------------------------
def test_dequant_bit_exact_and_cached_routes():
    g = torch.Generator().manual_seed(11)
    Lmax = 130 + 33 + 7
    kc = torch.randn(B, Lmax, HD, generator=g).to(BF)
    vc = torch.randn(B, Lmax, HD, generator=g).to(BF)
    kc[0, 3, :D] *= 2.0 ** -40
    vc[1, 7, D:] = 0
    kcodes, ke = F.quantise(kc, H, D)
    vcodes, ve = F.quantise(vc, H, D)
    dev = [t.to(DEV) for t in (kcodes, vcodes, ke, ve)]
    slab = tuple(torch.full((B, Lmax + 5, HD), 3.0, dtype=BF, device=DEV) for _ in range(2))
    kd, vd = ops().kv_dequant_fp8(*dev, rows=Lmax, H=H, D=D, out=slab)
    wk, wv = F.dequantise(kcodes, ke, H, D), F.dequantise(vcodes, ve, H, D)
    assert torch.equal(bits(kd.cpu()), bits(wk)) and torch.equal(bits(vd.cpu()), bits(wv))
    assert bool((slab[0][:, Lmax:] == 3.0).all())  # rows past `rows` untouched
    ref_k, ref_v = wk.to(DEV), wv.to(DEV)  # a bf16 cache holding the dequantised values
    for Lq in (2, 33):
        q = torch.randn(B * Lq, HD, generator=g).to(BF).to(DEV)
        for past in (0, 67, 130):
            for s0 in (0, 5):
                kvs = i32([s0] * B).to(DEV)
                kw = dict(B=B, H=H, Lq=Lq, D=D, scale=SCALE, kv_start=kvs)
                ks_, vs_ = ops().kv_dequant_fp8(*dev, rows=past + Lq, H=H, D=D, out=slab)
                o1, _ = ops().attn_fwd_cached(q, ks_, vs_, past=past, **kw)
                o2, _ = ops().attn_fwd_cached(q, ref_k, ref_v, past=past, **kw)
                assert torch.equal(bits(o1), bits(o2)), (Lq, past, s0)
                kv_len = i32([past + Lq, past + Lq - 1, past + Lq]).to(DEV)
                q_pad = i32([0, 1, 0]).to(DEV)
                o1, _ = ops().attn_fwd_ragged(q, ks_, vs_, kv_len, q_pad=q_pad, **kw)
                o2, _ = ops().attn_fwd_ragged(q, ref_k, ref_v, kv_len, q_pad=q_pad, **kw)
                assert torch.equal(bits(o1), bits(o2)), ("ragged", Lq, past, s0)


# ---------------------------------------------------------------------------------------------
# 4. the quantisation error, stated
# ---------------------------------------------------------------------------------------------
def quant_error_inputs():
    g = torch.Generator().manual_seed(21)
    L = 200
    q = torch.randn(B, HD, generator=g).to(BF)
    kc = torch.randn(B, L, HD, generator=g).to(BF)
    vc = torch.randn(B, L, HD, generator=g).to(BF)
    return L, q, kc, vc, i32([0] * B), i32([L] * B)


def quant_error_cpu():
    """rel-L2 of decode attention on the fake-quantised K, V (the f32 restatement, bf16 output) against
    f64 attention on the unquantised bf16 K, V: unit-normal q, K, V, 200 keys, B 3, H 2.
    python -c "from tests.test_kv_fp8_gpu import quant_error_cpu as f; print(f())" prints 0.0397"""
    L, q, kc, vc, ks, kl = quant_error_inputs()
    ref, _, _ = R.decode_attn_ref(q, kc, vc, ks, kl, SCALE)
    o = R.attn_honest(q, F.fake_quant(kc, H, D), F.fake_quant(vc, H, D), ks, kl, SCALE)
    return F.rel_l2(o, ref)


def test_quantisation_error_matches_cpu_figure():
    L, q, kc, vc, ks, kl = quant_error_inputs()
    ref, _, _ = R.decode_attn_ref(q, kc, vc, ks, kl, SCALE)
    cpu = quant_error_cpu()
    cache = [t.to(DEV) for t in frames(L)]
    ops().kv_append_fp8(kc.reshape(B * L, HD).to(DEV), vc.reshape(B * L, HD).to(DEV), *cache, ks.to(DEV), B=B, Lnew=L,
                        H=H, D=D)
    o = ops().attn_decode_fp8(q.to(DEV), *cache, kl.to(DEV), B=B, H=H, D=D, max_len=L, scale=SCALE, kv_start=ks.to(DEV))
    gpu = F.rel_l2(o.cpu(), ref)
    print(f"fp8 cache, 200 unit-normal keys: rel-L2 of O vs f64 on unquantised K, V: gpu {gpu:.5e}, cpu {cpu:.5e}")
    assert abs(gpu - cpu) <= 0.01 * cpu, (gpu, cpu)


# ---------------------------------------------------------------------------------------------
# 5. whole model (the tiny config of tests/test_generation.py: 2 layers, 2 heads of 128)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    m = CuLLaVOModel(tiny_gpu(), device="cuda", trainable="none", init="none")
    m.load_state_dict(O.make_weights(O.config_small_gpu(), 6))
    m.eval()
    return m


def _prompt(nb, S, seed, left_pad=0):
    cfg = O.config_small_gpu()
    ids, mask, pix, _ = O.make_inputs(cfg, nb, S, 3, seed)
    if left_pad:  # row 0 left-padded
        ids = torch.cat([torch.full((nb, left_pad), cfg.pad_token_id), ids], 1)
        mask = torch.cat([torch.ones(nb, left_pad, dtype=mask.dtype), mask], 1)
        ids[1:, :left_pad] = torch.randint(2, cfg.image_token_index, (nb - 1, left_pad),
                                           generator=torch.Generator().manual_seed(seed))
        mask[0, :left_pad] = 0
    return dict(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda())


def _both(m, **kw):
    a = m.generate(kv_cache_dtype="fp8", **kw)
    b = m.generate(kv_cache_dtype="fp8_sim", **kw)
    return a, b


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("how", ["greedy", "seeded"])
def test_generate_fp8_equals_its_bf16_twin(model, graph, how):
    kw = dict(max_new_tokens=6, decode_graph=graph, **_prompt(2, 20, 31, left_pad=4))
    if how == "seeded":
        kw.update(do_sample=True, temperature=0.9, top_k=50, top_p=0.95, seed=7)
    a, b = _both(model, **kw)
    assert torch.equal(a, b)


def test_forward_logits_bitwise_every_step(model, monkeypatch):
    """prefill, single-token steps on the fused and the unfused route, a multi-token turn (CACHED) and
    a chunked prefill: fp8 and fp8_sim logits bit for bit; an explicit "bf16" is the default's bits"""
    import cullavo_amd.generation as G
    cfg = O.config_small_gpu()
    p = _prompt(2, 20, 32, left_pad=4)
    outs = {}
    for dt in ("fp8", "fp8_sim", "bf16", None):
        lg = []
        model.prefill_chunk = 7 if dt in ("fp8", "fp8_sim") else None
        out = model(**p, use_cache=True, kv_cache_dtype=dt)
        model.prefill_chunk = None
        cache = out.past_key_values
        assert cache.kv_dtype == (dt or "bf16")
        if dt == "fp8":
            cache8 = cache
        lg.append(out.logits)
        g = torch.Generator().manual_seed(3)
        for step in range(4):
            monkeypatch.setattr(G, "FUSE_DECODE_ROPE", step % 2 == 0)
            tok = torch.randint(2, cfg.image_token_index, (2, 1), generator=g).cuda()
            out = model(input_ids=tok, past_key_values=cache, use_cache=True)
            lg.append(out.logits.clone())
        monkeypatch.setattr(G, "FUSE_DECODE_ROPE", True)
        turn = torch.randint(2, cfg.image_token_index, (2, 5), generator=g).cuda()
        lg.append(model(input_ids=turn, past_key_values=cache, use_cache=True).logits)
        outs[dt] = lg
    for x, y in zip(outs["fp8"], outs["fp8_sim"]):
        assert torch.equal(bits(x), bits(y))
    for x, y in zip(outs["bf16"], outs[None]):
        assert torch.equal(bits(x), bits(y))
    # the legacy view of an fp8 cache: dequantised copies, equal to the twin's rows
    k8, v8 = cache8[0]
    assert cache8.k.dtype == torch.uint8 and cache8.k_exp.shape[-1] == H
    assert k8.dtype == BF and k8.shape == (2, H, cache8.get_seq_length(), D)


def test_compact_cache_then_ragged_turn_and_from_legacy(model):
    cfg = O.config_small_gpu()
    p = _prompt(2, 20, 33, left_pad=4)
    res = {}
    for dt in ("fp8", "fp8_sim"):
        out = model.generate(**p, max_new_tokens=8, eos_token_id=5, compact_cache=True, return_dict_in_generate=True,
                             kv_cache_dtype=dt, do_sample=True, top_k=50, seed=11)
        cache = out.past_key_values
        assert cache.kv_dtype == dt and cache.lengths is not None
        g = torch.Generator().manual_seed(4)
        turn = torch.randint(2, cfg.image_token_index, (2, 6), generator=g)
        tmask = torch.ones(2, 6, dtype=torch.long)
        tmask[1, :2] = 0
        legacy = tuple((k.clone(), v.clone()) for k, v in cache.to_legacy_cache())
        lengths, nxt = cache.lengths.clone(), cache.next_pos.clone()
        two = model.generate(input_ids=turn.cuda(), attention_mask=tmask.cuda(), past_key_values=cache,
                             max_new_tokens=5, prefill_chunk=4)
        res[dt] = (out.sequences, two, legacy, lengths, nxt)
    assert torch.equal(res["fp8"][0], res["fp8_sim"][0]) and torch.equal(res["fp8"][1], res["fp8_sim"][1])
    for (k8, v8), (ks_, vs_) in zip(res["fp8"][2], res["fp8_sim"][2]):  # dequantised copies == the twin's rows
        for b in range(2):
            n = int(res["fp8"][3][b])
            assert torch.equal(bits(k8[b, :, :n]), bits(ks_[b, :, :n]))
            assert torch.equal(bits(v8[b, :, :n]), bits(vs_[b, :, :n]))
    # from_legacy(kv_dtype="fp8"): quantising already-dequantised rows is the identity, so a step on the
    # re-imported cache is the step on the original
    from cullavo_amd.generation import KVCache
    p1 = _prompt(2, 20, 34)
    steps = {}
    for dt in ("fp8", "fp8_sim"):
        out = model(**p1, use_cache=True, kv_cache_dtype=dt)
        native = out.past_key_values
        again = KVCache.from_legacy(native.to_legacy_cache(), kv_dtype=dt)
        assert again.kv_dtype == dt
        tok = torch.randint(2, cfg.image_token_index, (2, 1), generator=torch.Generator().manual_seed(9)).cuda()
        a = model(input_ids=tok, past_key_values=again, use_cache=True).logits
        b = model(input_ids=tok, past_key_values=native, use_cache=True).logits
        assert torch.equal(bits(a), bits(b))
        steps[dt] = a
    assert torch.equal(bits(steps["fp8"]), bits(steps["fp8_sim"]))


def test_lora_and_grow_compose(model):
    """adapters attached; eager steps that cross the cache's 256-row growth step"""
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    cfg = O.config_small_gpu()
    m = CuLLaVOModel(tiny_gpu(), device="cuda", trainable="lora", init="random", seed=3)
    m.eval()
    ar = m.arenas["lora"]  # lora_B is zero at init: make the adapters count
    ar.flat.copy_((0.05 * torch.randn(ar.numel, generator=torch.Generator(device="cuda").manual_seed(12),
                                      device="cuda")).to(ar.dtype))
    a, b = _both(m, max_new_tokens=5, **_prompt(2, 20, 35))
    assert torch.equal(a, b)
    p = _prompt(1, 20, 36)
    g = torch.Generator().manual_seed(5)
    toks = torch.randint(2, cfg.image_token_index, (3, 1, 1), generator=g).cuda()
    outs = {}
    for dt in ("fp8", "fp8_sim"):
        out = model(**p, use_cache=True, kv_cache_dtype=dt)
        cache = out.past_key_values
        room = cache.max_len - cache.length  # lm_infer sized it prompt + 256
        cache.max_len = cache.length + 1     # pretend it is nearly full: the second step must grow it
        cap = cache.max_len
        lg = []
        for t in toks:
            lg.append(model(input_ids=t, past_key_values=cache, use_cache=True).logits)
        assert cache.max_len == cap + 256 and room >= 3
        outs[dt] = lg
    for x, y in zip(outs["fp8"], outs["fp8_sim"]):
        assert torch.equal(bits(x), bits(y))


def test_dtype_argument_rules(model):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    p = _prompt(1, 20, 37)
    a = model.generate(**p, max_new_tokens=4)
    b = model.generate(**p, max_new_tokens=4, kv_cache_dtype="bf16")
    assert torch.equal(a, b) and model.kv_cache_dtype == "bf16"
    out = model(**p, use_cache=True, kv_cache_dtype="fp8")
    tok = torch.tensor([[7]]).cuda()
    with pytest.raises(ValueError, match="conflicts"):
        model(input_ids=tok, past_key_values=out.past_key_values, use_cache=True, kv_cache_dtype="bf16")
    with pytest.raises(ValueError, match="conflicts"):
        model.generate(input_ids=tok, past_key_values=out.past_key_values, kv_cache_dtype="fp8_sim")
    with pytest.raises(ValueError, match="one of"):
        model.generate(**p, kv_cache_dtype="e5m2")
    m32 = CuLLaVOModel(tiny_gpu(), device="cuda", trainable="none", init="random", dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        m32.generate(**p, max_new_tokens=2, kv_cache_dtype="fp8")


# ---------------------------------------------------------------------------------------------
# 6. fp8_sim against the bf16 cache: a report, gated loosely
# ---------------------------------------------------------------------------------------------
# The CPU figure: the oracle's attention on fake-quantised K and V against plain, unit-normal inputs
# at the tiny config's prompt length, rel-L2 of the attention output. Produced by
#   python -c "from tests.test_kv_fp8_gpu import oracle_attention_figure as f; print(f())"
# which printed 0.0346. The gate below is 5x that on the logits after 16 steps.
ORACLE_ATTN_REL = 0.0346


def oracle_attention_figure():
    g = torch.Generator().manual_seed(41)
    L = 20 + O.config_small_gpu().vision.num_patches - 1
    q, k, v = (torch.randn(1, H, L, D, generator=g).to(BF) for _ in range(3))

    def fq(x):
        return F.fake_quant(x.transpose(1, 2).reshape(1, L, HD), H, D).view(1, L, H, D).transpose(1, 2)

    def attn(q, k, v):  # the oracle's causal softmax attention in f64
        s = (q.double() @ k.double().transpose(-1, -2)) * SCALE
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
        return torch.softmax(s, -1) @ v.double()

    return F.rel_l2(attn(q, fq(k), fq(v)), attn(q, k, v))


def test_fp8_sim_against_bf16_cache_report(model):
    cfg = O.config_small_gpu()
    p = _prompt(2, 20, 38)
    g = torch.Generator().manual_seed(6)
    toks = torch.randint(2, cfg.image_token_index, (16, 2, 1), generator=g).cuda()
    last = {}
    for dt in ("bf16", "fp8_sim"):
        cache = model(**p, use_cache=True, kv_cache_dtype=dt).past_key_values
        for t in toks:
            out = model(input_ids=t, past_key_values=cache, use_cache=True)
        last[dt] = out.logits.float()
    rel = F.rel_l2(last["fp8_sim"], last["bf16"])
    rec = dict(test="fp8_sim_vs_bf16_logits_after_16_steps", rel_l2=rel, oracle_attention_rel_l2=ORACLE_ATTN_REL,
               gate=5 * ORACLE_ATTN_REL)
    print(json.dumps(rec))
    d = os.path.join(REPO, "profiles", "r20", "kv_fp8")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "fp8_sim_vs_bf16_tiny.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    assert rel <= 5 * ORACLE_ATTN_REL, rec
