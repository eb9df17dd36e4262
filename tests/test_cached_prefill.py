"""Cached forward over several new tokens: attention with a KV-cache prefix (cullavo_attn_fwd_cached,
ops.attn_fwd_cached) and the layers above it (generation.lm_infer with Lnew > 1 on a filled cache,
CuLLaVOModel.forward / generate with past_key_values, chunked prefill). Reference: the cached branch
of cullavo/arch_cullavo.py:605-647 with any number of new input_ids.

Kernel: bottom-right aligned causal softmax attention over the cache rows < past + Lq with the
kv_start mask, restated in f64 the way tests/test_accuracy_gpu.py::_attn_ref is, at that file's
gates (O rel-L2 <= 3e-3, max |err| / (|ref| + row rms + 1e-3 rms) <= 2^-3, LSE max|err| <= 1e-5 and
> 0 and finite). The cache's unused rows are NaN in K and V: a kernel that lets one of them into a
result fails the finiteness check. Rows with no visible key are exactly zero.
On the CPU the f64 restatement against a plain f32 torch restatement of the same inputs measured,
over the cases of CASES: O rel-L2 7.8e-8 .. 4.7e-7, max row-scaled error 3.6e-7 .. 1.8e-6, LSE max|err|
9.5e-8 .. 5.2e-7 (each > 0), queries without a visible key 0 except case 4 (3 of 10): the gates are
met by arithmetic alone, and no comparison is empty.

Model: tiny_gpu() (head_dim 128: the MFMA path) on oracle.make_weights / make_inputs, as
tests/test_generation.py; gates rel-L2 <= 1e-2 ("same arithmetic, different kernels",
test_generation.py:102) and <= 3e-2 against the oracle (test_generation.py:111).
"""
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
# (B, H, Lq, past, D, kv_start, dtype), each chosen for a tile edge (128-query / 64-key tiles)
CASES = [
    (2, 2, 2, 1, 128, None, BF),             # the smallest continuation
    (1, 2, 33, 63, 128, None, BF),           # past one short of a key tile, Lq one over a wave's 32 rows
    (2, 2, 130, 200, 128, (0, 70), BF),      # two query tiles with a 2-row tail, kv_start inside key tile 1
    (1, 2, 64, 1088, 128, None, BF),         # the config-3 prompt length as prefix
    (2, 3, 5, 64, 128, (0, 67), BF),         # sequence 1's first three queries see no key
    (1, 3, 200, 5, 64, None, BF),            # the D = 64 kernel
    (1, 2, 40, 24, 32, None, BF),            # the generic kernel: small head dim
    (1, 2, 40, 24, 128, None, torch.float32),  # the generic kernel: f32 storage
]
PAD_ROWS = 37  # free cache rows behind the filled ones, NaN


def make_case(B, H, Lq, past, D, kv_start, dtype, seed=23):
    """(q [B*Lq, H*D], k_cache, v_cache [B, past + Lq + 37, H*D] with NaN free rows), CPU tensors"""
    g = torch.Generator().manual_seed(seed)
    Lk, hd = past + Lq, H * D
    q = torch.randn(B * Lq, hd, generator=g).to(dtype)
    kc = torch.full((B, Lk + PAD_ROWS, hd), float("nan"), dtype=dtype)
    vc = torch.full((B, Lk + PAD_ROWS, hd), float("nan"), dtype=dtype)
    kc[:, :Lk] = torch.randn(B, Lk, hd, generator=g).to(dtype)
    vc[:, :Lk] = torch.randn(B, Lk, hd, generator=g).to(dtype)
    return q, kc, vc


def attn_cached_ref(q, kc, vc, B, H, Lq, past, D, scale, kv_start, dt=torch.float64):
    """Bottom-right causal softmax attention of the Lq new rows over cache rows < past + Lq, keys
    kv_start[b] <= j <= past + i, in dtype dt. Returns (O [B*Lq, H*D], lse [B, H, Lq], dead [B, Lq]:
    queries with no visible key, O = 0 there)."""
    Lk = past + Lq
    Q = q.to(dt).view(B, Lq, H, D).transpose(1, 2)
    K = kc[:, :Lk].to(dt).view(B, Lk, H, D).transpose(1, 2)
    V = vc[:, :Lk].to(dt).view(B, Lk, H, D).transpose(1, 2)
    S = (Q @ K.transpose(-1, -2)) * scale  # [B, H, Lq, Lk]
    i = torch.arange(Lq, device=q.device)[:, None]
    j = torch.arange(Lk, device=q.device)[None, :]
    ks = torch.tensor(kv_start if kv_start is not None else [0] * B, device=q.device)
    vis = (j <= past + i)[None] & (j[None] >= ks[:, None, None])  # [B, Lq, Lk]
    dead = ~vis.any(-1)
    S = S.masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse.masked_fill(dead[:, None], 0.0)[..., None])  # dead rows: exp(-inf) = 0
    Oh = P @ V
    return Oh.transpose(1, 2).reshape(B * Lq, H * D), lse, dead


@functools.lru_cache(maxsize=None)
def _case(idx):
    """(inputs on the GPU, f64 reference) of CASES[idx]: built once, shared, never modified"""
    B, H, Lq, past, D, kv_start, dtype = CASES[idx]
    q, kc, vc = (t.to(DEV) for t in make_case(B, H, Lq, past, D, kv_start, dtype))
    return (q, kc, vc), attn_cached_ref(q, kc, vc, B, H, Lq, past, D, D ** -0.5, kv_start)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"B{c[0]}H{c[1]}Lq{c[2]}past{c[3]}D{c[4]}"
                                                         f"{'ks' if c[5] else ''}{'f32' if c[6] != BF else ''}"
                                                         for c in CASES])
def test_attn_fwd_cached_against_f64(idx):
    B, H, Lq, past, D, kv_start, dtype = CASES[idx]
    (q, kc, vc), (O_ref, LSE_ref, dead) = _case(idx)
    ks = torch.tensor(kv_start, dtype=torch.int32, device=DEV) if kv_start is not None else None
    o, lse = ops().attn_fwd_cached(q, kc, vc, B=B, H=H, Lq=Lq, past=past, D=D, scale=D ** -0.5, kv_start=ks)
    torch.cuda.synchronize()
    assert o.shape == (B * Lq, H * D) and lse.shape == (B, H, Lq)
    assert torch.isfinite(o).all(), "a free (NaN) cache row reached the output"
    dead_rows = dead.reshape(B * Lq)
    assert int(dead_rows.sum()) == (3 if idx == 4 else 0)
    assert (o[dead_rows] == 0).all(), "a query with no visible key must return a zero row"
    live = ~dead[:, None].expand(B, H, Lq)
    assert torch.isfinite(lse[live]).all()
    lse_err = (lse.double() - LSE_ref)[live].abs().max().item()
    err = o.double() - O_ref
    rel = (err.norm() / O_ref.norm()).item()
    row_rms = O_ref.view(-1, H, D).pow(2).mean(-1, keepdim=True).sqrt().expand(-1, H, D).reshape(O_ref.shape)
    floor = 1e-3 * O_ref.pow(2).mean().sqrt()
    worst = (err.abs() / (O_ref.abs() + row_rms + floor)).max().item()
    print(f"case {CASES[idx][:6]}: O rel-L2 {rel:.3e}, max row-scaled {worst:.3e}, lse max|err| {lse_err:.3e}")
    assert 0.0 < lse_err < float("inf"), f"lse max|err| {lse_err}: the comparison is broken"
    assert lse_err <= 1e-5, f"lse max|err| {lse_err:.2e}"
    assert rel <= 3e-3, f"O rel-L2 {rel:.2e}"
    assert worst <= 2 ** -3, f"O max |err| / (|ref| + row rms) {worst:.2e}"


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,L,D", [(2, 2, 200, 128), (1, 2, 77, 64)])
def test_past_zero_is_the_causal_kernel(B, H, L, D):
    """past = 0: O and LSE bitwise those of ops.attn_fwd(causal=True) on the same rows"""
    q, kc, vc = (t.to(DEV) for t in make_case(B, H, L, 0, D, None, BF, seed=29))
    k = kc[:, :L].reshape(B * L, H * D).contiguous()
    v = vc[:, :L].reshape(B * L, H * D).contiguous()
    o0, lse0 = ops().attn_fwd(q, k, v, B=B, H=H, Lq=L, Lk=L, D=D, scale=D ** -0.5, causal=True)
    o1, lse1 = ops().attn_fwd_cached(q, kc, vc, B=B, H=H, Lq=L, past=0, D=D, scale=D ** -0.5)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


# ---------------------------------------------------------------------------------------------
# host side (no GPU): argument checks, the built kernel's inline-asm LDS reads
# ---------------------------------------------------------------------------------------------
def test_attn_fwd_cached_argument_checks():
    """past < 0 and a cache batch stride below (past + Lq) rows return CULLAVO_EINVAL with a message
    before anything is launched (null pointers: a launch would fault)."""
    from cullavo_amd import _lib
    hd = 256
    # (q, ldq, k_cache, v_cache, ld_tok, ld_batch, o, ldo, lse, B, H, Lq, past, D, scale, kv_start, dtype, stream)
    with pytest.raises(ValueError, match="past must not be negative"):
        _lib.call("attn_fwd_cached", None, hd, None, None, hd, 64 * hd, None, hd, None, 2, 2, 4, -1, 128, 1.0, None, 1, None)
    with pytest.raises(ValueError, match="batch stride is smaller"):
        _lib.call("attn_fwd_cached", None, hd, None, None, hd, 11 * hd, None, hd, None, 2, 2, 4, 8, 128, 1.0, None, 1, None)
    with pytest.raises(Exception, match="head_dim must be 16, 32, 64 or 128"):
        _lib.call("attn_fwd_cached", None, 192, None, None, 192, 64 * 192, None, 192, None, 1, 2, 4, 8, 96, 1.0, None, 1,
                  None)
    # the entry point came with ABI 8; the library and the header agree on the current version
    assert _lib.abi_version() >= 8 and _lib.lib().cullavo_abi_version() == _lib.abi_version()


def test_cached_kernel_lds_reads_not_used_before_their_wait():
    """attn_fwd_cached_k shares the pipelined forward's inline-asm LDS reads with deferred counted
    waits: the same scan of the built code as tests/test_isa_lds_reads.py runs on attn_fwd_pipe_k."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_isa_lds_reads.py")
    spec = importlib.util.spec_from_file_location("_isa_lds_reads", path)
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    if not (os.path.exists(isa.LIB) and os.path.exists(isa.OBJDUMP)):
        pytest.skip("library or llvm-objdump missing")
    kernels = isa._kernels()
    names = ("attn_fwd_cached_kILi128EE", "attn_fwd_cached_kILi64EE")
    checked = isa._listed(kernels, names)
    assert len(checked) == 2, checked
    problems = {n: bad[:3] for n in checked if (bad := isa._early_uses([ins for _, ins in kernels[n]]))}
    assert not problems, problems


# ---------------------------------------------------------------------------------------------
# model: continuation, left padding, chunked prefill, multi-turn generate
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _model(seed=6):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable="none", init="none")
    m.load_state_dict(O.make_weights(O.config_small_gpu(), seed))
    m.eval()
    return m


def _cache_close(a, b):
    assert a.get_seq_length() == b.get_seq_length()
    assert torch.equal(a.next_pos.cpu(), b.next_pos.cpu())
    L = a.get_seq_length()
    for li in (0, len(a) - 1):
        assert rel_l2(a.k[li, :, :L], b.k[li, :, :L]) <= 1e-2, li
        assert rel_l2(a.v[li, :, :L], b.v[li, :, :L]) <= 1e-2, li


@pytest.mark.gpu
def test_continuation_equals_one_pass():
    """(a) one prefill of a 24-token prompt with one image; (b) prefill of its first 17 tokens and the
    image, then one cached forward over the other 7. Raises NotImplementedError without the feature."""
    cfg = O.config_small_gpu()
    W = O.make_weights(cfg, 6)
    m = _model()
    ids, mask, pix, _ = O.make_inputs(cfg, 2, 24, 4, 31)
    a = m(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda(), use_cache=True)
    b0 = m(input_ids=ids[:, :17].cuda(), pixel_values=pix.cuda(), attention_mask=mask[:, :17].cuda(), use_cache=True)
    b = m(input_ids=ids[:, 17:].cuda(), past_key_values=b0.past_key_values, use_cache=True)
    assert b.logits.shape == (2, 7, cfg.text.vocab_size)
    assert rel_l2(b.logits, a.logits[:, -7:]) <= 1e-2
    _, logits_ref, _ = O.forward(W, cfg, ids, pix, mask, None)
    assert rel_l2(b.logits, logits_ref[:, -7:]) <= 3e-2
    _cache_close(b.past_key_values, a.past_key_values)


@pytest.mark.gpu
def test_left_padding_survives_continuation():
    """the batch of test_generation.py::test_left_padded_batch_matches_single, prefilled, then continued
    with 5 tokens: the padded row's continuation logits are the single unpadded run's"""
    cfg = O.config_small_gpu()
    m = _model()
    ids, mask, pix, _ = O.make_inputs(cfg, 1, 20, 3, 13)
    pad = cfg.pad_token_id
    ids2 = torch.cat([torch.full((1, 5), pad), ids], 1)
    mask2 = torch.cat([torch.zeros(1, 5, dtype=mask.dtype), mask], 1)
    extra = torch.randint(2, cfg.image_token_index, (1, 5), generator=torch.Generator().manual_seed(2))
    batch_ids = torch.cat([ids2, torch.cat([extra, ids], 1)], 0)  # row 1: unpadded, longer prompt
    batch_mask = torch.cat([mask2, torch.ones_like(mask2)], 0)
    batch_pix = torch.cat([pix, pix], 0)
    more = torch.randint(2, cfg.image_token_index, (1, 5), generator=torch.Generator().manual_seed(3))
    one = m(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda(), use_cache=True)
    one = m(input_ids=more.cuda(), past_key_values=one.past_key_values, use_cache=True)
    two = m(input_ids=batch_ids.cuda(), pixel_values=batch_pix.cuda(), attention_mask=batch_mask.cuda(),
            use_cache=True)
    full_mask = torch.cat([two.past_key_values.kv_start.cpu()[:, None] <= torch.arange(two.past_key_values.length),
                           torch.ones(2, 5, dtype=torch.bool)], 1).long()
    two = m(input_ids=torch.cat([more, more], 0).cuda(), past_key_values=two.past_key_values,
            attention_mask=full_mask.cuda(), use_cache=True)  # a mask over past + new rows, new part all ones
    assert two.logits.shape == (2, 5, cfg.text.vocab_size)
    assert rel_l2(two.logits[0], one.logits[0]) <= 1e-2


@pytest.mark.gpu
def test_chunked_prefill_matches_one_pass():
    cfg = O.config_small_gpu()
    m = _model()
    ids, mask, pix, _ = O.make_inputs(cfg, 2, 24, 4, 37)
    kw = dict(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda())
    a = m(**kw, use_cache=True)
    assert a.logits.shape[1] == 24 + cfg.vision.num_patches - 1 == 279  # three pieces of <= 100 rows
    m.prefill_chunk = 100
    try:
        b = m(**kw, use_cache=True)
    finally:
        m.prefill_chunk = None
    assert b.logits.shape == a.logits.shape
    assert rel_l2(b.logits[:, -1], a.logits[:, -1]) <= 1e-2
    _cache_close(b.past_key_values, a.past_key_values)
    g1 = m.generate(**kw, prefill_chunk=100, max_new_tokens=4)
    g2 = m.generate(**kw, prefill_chunk=100, max_new_tokens=4)
    assert g1.shape == (2, 28) and torch.equal(g1[:, :24].cpu(), ids)
    assert torch.equal(g1, g2)


@pytest.mark.gpu
def test_multi_turn_generate_matches_oracle():
    """generate(return_dict_in_generate=True), then a second turn on its cache: every token of turn 2
    is the oracle's argmax of the full recompute over the whole conversation so far (the turn-1 prompt,
    the turn-1 tokens in the cache, the last turn-1 token as turn 2's first id, then turn 2)."""
    cfg = O.config_small_gpu()
    W = O.make_weights(cfg, 6)
    m = _model()
    ids, mask, pix, _ = O.make_inputs(cfg, 1, 20, 3, 41)
    r1 = m.generate(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda(), max_new_tokens=4,
                    return_dict_in_generate=True)
    seq1, cache = r1.sequences, r1.past_key_values
    assert seq1.shape == (1, 24)
    L1 = 20 + cfg.vision.num_patches - 1 + 3  # as in HF, the last sampled token is not in the cache
    assert cache.get_seq_length() == L1 and int(cache.next_pos[0]) == L1
    new = torch.randint(2, cfg.image_token_index, (1, 5), generator=torch.Generator().manual_seed(5))
    turn2 = torch.cat([seq1[:, -1:].cpu(), new], 1)  # 6 tokens
    legacy = tuple((k.clone(), v.clone()) for k, v in cache.to_legacy_cache())  # turn 2 again, without the graph
    out = m.generate(input_ids=turn2.cuda(), past_key_values=cache, max_new_tokens=4)
    assert out.shape == (1, 10) and torch.equal(out[:, :6].cpu(), turn2)
    conv = torch.cat([seq1[:, :-1].cpu(), out.cpu()], 1)
    for i in range(4):
        n = 23 + 6 + i
        prefix = conv[:, :n]
        _, lg, _ = O.forward(W, cfg, prefix, pix, torch.ones_like(prefix), None)
        last = lg[0, -1]
        tok = int(conv[0, n])
        top = torch.topk(last, 2).values
        assert tok == int(last.argmax()) or (last.max() - last[tok]).item() <= 2e-2 * (top[0] - last.min()).item(), i
    eager = m.generate(input_ids=turn2.cuda(), past_key_values=legacy, max_new_tokens=4, decode_graph=False)
    assert torch.equal(eager, out)


@pytest.mark.gpu
def test_transformers_layout_cache_takes_several_tokens():
    from cullavo_amd.generation import KVCache
    cfg = O.config_small_gpu()
    m = _model()
    ids, mask, pix, _ = O.make_inputs(cfg, 2, 20, 3, 17)
    ids, mask, pix = ids.cuda(), mask.cuda(), pix.cuda()
    native = m(input_ids=ids, pixel_values=pix, attention_mask=mask, use_cache=True).past_key_values
    legacy = KVCache.from_legacy(tuple((k.clone(), v.clone()) for k, v in native.to_legacy_cache()))
    toks = torch.randint(2, cfg.image_token_index, (2, 3), generator=torch.Generator().manual_seed(4)).cuda()
    a = m(input_ids=toks, past_key_values=legacy, use_cache=True)
    b = m(input_ids=toks, past_key_values=native, use_cache=True)
    assert a.logits.shape == (2, 3, cfg.text.vocab_size) and torch.equal(a.logits, b.logits)


@pytest.mark.gpu
def test_masked_continuation_token_is_refused():
    cfg = O.config_small_gpu()
    m = _model()
    ids, mask, pix, _ = O.make_inputs(cfg, 2, 20, 3, 43)
    cache = m(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda(), use_cache=True).past_key_values
    toks = torch.randint(2, cfg.image_token_index, (2, 4), generator=torch.Generator().manual_seed(6)).cuda()
    hole = torch.ones(2, 4, dtype=torch.long, device=DEV)
    hole[1, 2] = 0
    with pytest.raises(NotImplementedError, match="masked tokens"):
        m(input_ids=toks, past_key_values=cache, attention_mask=hole, use_cache=True)
