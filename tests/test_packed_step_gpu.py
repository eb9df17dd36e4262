"""CuLLaVOModel.packed_rows: the training step on the attended rows only (packed.PackedPlan, the varlen
attention in LlamaLayerFn, the head on [T, d]) on the small kernel-shaped config of tests/test_model_gpu.py.

Batch 3, attended lengths unequal with one row full; right- and left-padded; with pixel_values (the counts
reach the host with the merge's read-back) and text-only (attended_lens from the host).
  oracle     packed_rows against the bf16-faithful oracle at the gates of tests/test_model_gpu.py: logits at
             attended positions rel-L2 <= 1e-2, |dloss| <= 1e-2, every trainable gradient rel-L2 <= 2e-2;
  padded     against the padded path of the same build at dropout 0: loss within 1e-2, logits at attended
             positions rel-L2 <= 1e-2, logits elsewhere exactly 0 (not bitwise: the GEMM plan depends on M);
  tail       with supervised_rows as well, the loss is the packed_rows-only loss within that switch's own
             gate (1e-6 relative, tests/test_supervised_rows_gpu.py);
  lora       trainable="lora" at dropout 0.05 runs; one seed twice gives bitwise equal loss and gradients;
  fallback   a batch without padding takes the padded path: no varlen call, results bitwise the switch-off ones;
  errors     a mask with a hole raises; the f32 parity mode raises NotImplementedError.
"""
import pytest
import torch

from oracle import cullavo_oracle as O

pytestmark = pytest.mark.gpu

PADS = (0, 9, 20)  # padded text tokens per row: one row full
S = 48


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def build(trainable="full", seed=3, packed=False, **kw):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    m = CuLLaVOModel(tiny_gpu(), device="cuda", trainable=trainable, init="none", **kw)
    m.load_state_dict(O.make_weights(O.config_small_gpu(), seed), strict=False)
    if "lora" in m.arenas:
        from cullavo_amd.lora import init_lora_
        init_lora_(m.arenas["lora"], 5)
        m.train()
    m.packed_rows = packed
    return m


def make_batch(side, pixels=True, pads=PADS, seed=3):
    """CPU tensors (ids, mask, pix, labels). right: the oracle's own pad_tail; left: the same rows shifted
    to the right end behind pad tokens. Text-only: the <image> id replaced by an ordinary one, labels [B, S]."""
    cfg = O.config_small_gpu()
    ids, mask, pix, labels = O.make_inputs(cfg, len(pads), S, 3, seed, pad_tail=list(pads) if side == "right" else None)
    if side == "left":
        for b, n in enumerate(pads):
            if n:
                ids[b] = torch.cat([torch.full((n,), cfg.pad_token_id), ids[b, :S - n]])
                mask[b, :n] = 0
    if not pixels:
        ids[ids == cfg.image_token_index] = 7
        g = torch.Generator().manual_seed(seed)
        labels = torch.full((len(pads), S), -100, dtype=torch.long)
        labels[:, S // 2:] = torch.randint(2, 1000, (len(pads), S - S // 2), generator=g)
        pix = None
    return ids, mask, pix, labels


def run(m, b, backward=True, **kw):
    ids, mask, pix, labels = (t.cuda() if t is not None else None for t in b)
    if pix is None and m.packed_rows:
        kw.setdefault("attended_lens", mask.sum(-1).tolist() if not mask.is_cuda else b[1].sum(-1).tolist())
    out = m(input_ids=ids, pixel_values=pix, attention_mask=mask, labels=labels, **kw)
    if backward:
        out.loss.backward()
        for ar in m.arenas.values():
            ar.finalize_grads()
    torch.cuda.synchronize()
    return out


def grads_of(m):
    return {name: ar.grad_flat.float().clone() for name, ar in m.arenas.items() if ar.trainable}


def count_varlen(monkeypatch):
    from cullavo_amd import ops
    calls = []
    fwd = ops.attn_fwd_varlen
    monkeypatch.setattr(ops, "attn_fwd_varlen", lambda *a, **k: (calls.append(1), fwd(*a, **k))[1])
    return calls


@pytest.mark.parametrize("side", ["right", "left"])
def test_packed_step_matches_bf16_oracle(side, monkeypatch):
    b = make_batch(side)
    cfg = O.config_small_gpu()
    Wb = {k: v.requires_grad_(True) for k, v in O.to_bf16(O.make_weights(cfg, 3)).items()}
    loss_ref, logits_ref, aux = O.forward(Wb, cfg, b[0], b[2], b[1], b[3])
    loss_ref.backward()
    calls = count_varlen(monkeypatch)
    m = build(packed=True)
    out = run(m, b)
    assert calls, "the packed path did not run the varlen attention"
    valid = aux["attention_mask"].bool()
    err = rel_l2(out.logits.float().cpu()[valid], logits_ref.float()[valid])
    dloss = abs(out.loss.item() - loss_ref.item())
    print(f"{side}: logits rel-L2 {err:.2e}, |dloss| {dloss:.2e}")
    assert err <= 1e-2 and dloss <= 1e-2
    assert out.logits.float().cpu()[~valid].abs().max().item() == 0.0
    worst, n = 0.0, 0
    for name, ar in m.arenas.items():
        if not ar.trainable:
            continue
        for k, p in ar.params.items():
            ref = Wb[k].grad if k in Wb else None
            if ref is None or float(ref.float().norm()) == 0.0:
                assert p.grad is None or float(p.grad.float().abs().max()) == 0.0, k
                continue
            e = rel_l2(p.grad, ref)
            worst, n = max(worst, e), n + 1
            assert e <= 2e-2, (k, e)
    assert n > 0
    print(f"{side}: worst gradient rel-L2 {worst:.2e} over {n} parameters")


@pytest.mark.parametrize("pixels", [True, False], ids=["pixels", "text"])
@pytest.mark.parametrize("side", ["right", "left"])
def test_packed_against_padded_path(side, pixels, monkeypatch):
    b = make_batch(side, pixels)
    ref = run(build(), b)
    calls = count_varlen(monkeypatch)
    out = run(build(packed=True), b)
    assert calls
    mask = b[1] if not pixels else None
    if mask is None:  # the merged mask: attended where the padded run's kv span says so; take the oracle's
        mask = O.forward(O.to_bf16(O.make_weights(O.config_small_gpu(), 3)), O.config_small_gpu(), b[0], b[2], b[1],
                         b[3])[2]["attention_mask"]
    valid = mask.bool()
    lo, lr = out.logits.float().cpu(), ref.logits.float().cpu()
    err, dloss = rel_l2(lo[valid], lr[valid]), abs(out.loss.item() - ref.loss.item())
    print(f"{side} {'pixels' if pixels else 'text'}: logits rel-L2 {err:.2e}, |dloss| {dloss:.2e}")
    assert err <= 1e-2 and dloss <= 1e-2
    assert lo[~valid].abs().max().item() == 0.0 and int((~valid).sum()) > 0


def test_with_supervised_rows():
    b = make_batch("right")
    n_sup = int((b[3][:, 1:] != -100).sum())
    base = run(build(packed=True), b)
    m = build(packed=True)
    m.supervised_rows = True
    out = run(m, b, num_supervised=n_sup)
    assert out.logits is None
    print(f"loss packed {base.loss.item():.8f}, packed + supervised rows {out.loss.item():.8f}")
    assert abs(out.loss.item() - base.loss.item()) <= 1e-6 * abs(base.loss.item())
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for n, g in grads_of(m).items() if n in ("layers", "head"))


def test_lora_recipe_is_repeatable():
    from cullavo_amd.lora import LoraSettings
    b = make_batch("left")
    res = []
    for _ in range(2):
        m = build(trainable="lora", packed=True, lora=LoraSettings(r=8, lora_dropout=0.05))
        torch.manual_seed(77)  # StepContext draws this forward's lora_seed from torch's CPU generator
        out = run(m, b)
        g = grads_of(m)
        assert torch.isfinite(out.loss) and g["lora"].abs().sum() > 0
        res.append((out.loss.detach().clone(), g))
    assert torch.equal(res[0][0], res[1][0])
    for name in res[0][1]:
        assert torch.equal(res[0][1][name], res[1][1][name]), name


def test_batch_without_padding_takes_the_padded_path(monkeypatch):
    b = make_batch("right", pads=(0, 0, 0))
    ref_m = build()
    ref = run(ref_m, b)
    calls = count_varlen(monkeypatch)
    m = build(packed=True)
    out = run(m, b)
    assert not calls, "a batch without padding ran the varlen attention"
    assert torch.equal(out.loss, ref.loss) and torch.equal(out.logits, ref.logits)
    gr, go = grads_of(ref_m), grads_of(m)
    for name in gr:
        assert torch.equal(go[name], gr[name]), name


def test_errors():
    ids, mask, pix, labels = make_batch("right")
    mask = mask.clone()
    mask[1, 10] = 0  # a zero between attended tokens
    with pytest.raises(ValueError, match="hole"):
        run(build(packed=True), (ids, mask, pix, labels), backward=False)
    m32 = build(packed=True, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        run(m32, make_batch("right"), backward=False)
