"""The layer functions of functions.py on the MI355X against float64, per row: LlamaLayerFn (grid with and
without kv_start, packed, the supervised-row tail, adapters on all four groups at dropout 0 and 0.05; both
decoder layers of the tiny model), ClipLayerFn (frozen tower; adapters on qkv / fc1 / fc2; a trainable
tower; with and without an input gradient), ProjectorFn, HeadLossFn, HeadLossRowsFn and the row movers, on the inputs, references,
emulations and gates of tests/layer_refs.py (proved on the CPU in tests/test_layer_refs_host.py).
A layer is taken out of the tiny model, run on the case's h with layer.run / *.apply as arch_cullavo.py
does, backward is h3.backward(dh3), and the parameter gradients are read from the arenas after
finalize_grads. The references run in f64 on the GPU. The decoder layer also runs with the fused SwiGLU
backward off and with the weight gradients on the side stream: bitwise the default's results.
One JSON line per case, tensor and figure (emulated, measured, ratio) goes to the statistics file of
tests/test_accuracy_gpu.py; the lines of one MI355X run are committed as
profiles/r23/layers/layer_stats.jsonl. MEASURED_RATIOS below quotes that run: 0.64 .. 1.94 overall
against the margin M = 2.0 of layer_refs (the 1.94 is one vector gradient; see layer_refs).

The loss. HeadLossFn's loss is held at the f32 reduction gate (relative 1e-6) twice: to the emulation's
row losses summed in f32, and to the f64 cross-entropy of the logits it returned itself.
HeadLossRowsFn returns no logits; its loss is held at the same gate to HeadLossFn's on the same input.
"""
import functools

import pytest
import torch

from tests import layer_refs as LR
from tests.layer_refs import Mode
from tests.test_accuracy_gpu import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
# measured / emulated figure over the 385 lines of profiles/r23/layers/layer_stats.jsonl (min .. max), against
# the gate layer_refs.M = 2.0
MEASURED_RATIOS = {"layer_decoder": (0.80, 1.40), "layer_decoder_lora": (0.82, 1.17), "layer_clip": (1.00, 1.09),
                   "layer_clip_lora": (0.87, 1.12), "layer_clip_trainable": (0.64, 1.94), "layer_projector": (1.00, 1.00),
                   "layer_head": (1.00, 1.00), "layer_head_rows": (1.00, 1.00)}


@functools.lru_cache(maxsize=None)
def model(trainable="full"):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable=trainable, init="none")
    m.load_state_dict(LR.O.make_weights(LR.CFG, LR.WEIGHT_SEED))
    W = LR.weights()
    for ar in m.arenas.values():
        for k, p in ar.params.items():
            assert torch.equal(p.detach().cpu(), W[k]), k   # the references' weights are the model's, bitwise
    return m


def _finish(m):
    torch.cuda.synchronize()
    for a in m.arenas.values():
        a.finalize_grads()
    torch.cuda.synchronize()


def _begin(m):
    for a in m.arenas.values():
        a.zero_grad()


def _check(test, case, got, emu, exact, **kw):
    recs, fails = LR.gate(got, emu, exact, **kw)
    for r in recs:
        _log({"test": test, "case": case, **r})
    print(case, " ".join(f"{r['figure']}={r['ratio']:.2f}" for r in recs))
    assert not fails, f"{case}: " + "; ".join(fails)


# ---- decoder layer ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decoder_refs(name, layer):
    g, h, dh3 = LR.decoder_case(name)
    W = LR.lm_layer_weights(layer, device=DEV)
    return tuple(LR.decoder_layer(h.to(DEV).double(), dh3.to(DEV).double(), W, g, Mode(k)) for k in ("exact", "emu"))


def _run_decoder(name, li, m=None):
    from cullavo_amd import functions as FN
    from cullavo_amd import ops
    from cullavo_amd.packed import PackedPlan
    lora = m is not None
    m = m or model()
    g, h, dh3 = LR.decoder_case(name)
    layer = m.language_model.model.layers[li]
    kv = torch.tensor(g.kv_start, dtype=torch.int32, device=DEV) if g.kv_start is not None else None
    sctx = FN.StepContext(g.B, g.L, g.pos.to(DEV), kv, lora_seed=LR.LORA_SEED)
    if g.c["form"] == "packed":
        lens = torch.tensor(g.lens, dtype=torch.int32, device=DEV)
        sctx.packed = PackedPlan(torch.arange(g.Tp, device=DEV), (torch.cumsum(lens, 0) - lens).to(torch.int32), lens,
                                 g.T, g.Tp, max(g.lens))
    if g.tail is not None:
        assert layer is m.language_model.model.layers[-1]
        tg = torch.full((g.Tp,), LR.IGNORE, dtype=torch.long, device=DEV)
        tg[g.tail[g.tail >= 0].to(DEV)] = 5
        rows = ops.supervised_rows(tg, g.tail.numel(), LR.IGNORE)
        assert torch.equal(rows.cpu(), g.tail)
        sctx.tail_layer, sctx.tail_rows = layer, rows
    hg = h.to(DEV).requires_grad_(True)
    _begin(m)
    h3 = layer.run(hg, sctx)
    h3.backward(dh3.to(DEV))
    _finish(m)
    P = m.arenas["layers"].params
    pre = f"language_model.model.layers.{li}."
    out = {"h3": h3.detach().clone(), "dh": hg.grad.clone()}
    if lora:
        out.update(_lora_grads(m, pre, LR.LM_GROUPS))
        return out
    for k, names in LR.LM_GRAD_KEYS.items():
        out[k] = torch.cat([P[pre + n].grad for n in names]).clone()
    return out


DECODER_RUNS = [(n, li) for n in LR.DECODER_CASES for li in ((1,) if "tail" in n else (0, 1))]


@pytest.mark.parametrize("name,li", DECODER_RUNS)
def test_decoder_layer_against_f64(name, li, monkeypatch):
    import cullavo_amd.functions as FN
    monkeypatch.setattr(FN, "FUSED_SWIGLU_BWD", True)
    monkeypatch.setattr(FN, "DW_STREAM", "off")
    monkeypatch.setattr(FN, "SWG_OVERLAP", False)
    g = LR.decoder_case(name)[0]
    got = _run_decoder(name, li)
    exact, emu = _decoder_refs(name, li)
    assert got["h3"].shape == exact["h3"].shape and got["dh"].shape == exact["dh"].shape
    _check("layer_decoder", f"{name}/layer{li}", got, emu, exact, zero_rows=g.zero_rows)
    # the A/B switches the layer's backward reads: bitwise the same results
    for flag, value in (("FUSED_SWIGLU_BWD", False), ("DW_STREAM", "side")):
        with monkeypatch.context() as mp:
            mp.setattr(FN, flag, value)
            other = _run_decoder(name, li)
        for k in got:
            assert torch.equal(got[k], other[k]), f"{name}/layer{li}: {k} differs with {flag} = {value}"


def test_tail_with_mlp_adapters_raises():
    """the supervised-row tail does not cover LoRA adapters on the MLP: the layer says so"""
    from cullavo_amd import functions as FN
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    from cullavo_amd.lora import LoraSettings
    m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable="lora", init="random", seed=9,
                     lora=LoraSettings(lora_dropout=0.0, vision_layers=(1, 2)))
    g, h, _ = LR.decoder_case("grid-left+tail")
    layer = m.language_model.model.layers[-1]
    sctx = FN.StepContext(g.B, g.L, g.pos.to(DEV), torch.tensor(g.kv_start, dtype=torch.int32, device=DEV), lora_seed=1)
    sctx.tail_layer, sctx.tail_rows = layer, g.tail.to(DEV)
    with pytest.raises(ValueError, match="supervised-row tail does not cover LoRA"):
        layer.run(h.to(DEV).requires_grad_(True), sctx)


# ---- CLIP layer (frozen tower) ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LR.CLIP_CASES))
def test_clip_layer_against_f64(name):
    m = model()
    B = LR.CLIP_CASES[name]["B"]
    h, dh3 = LR.clip_case(name)
    layer = m.vision_tower.vision_model.encoder.layers[0]
    W = LR.clip_layer_weights(0, device=DEV)
    exact, emu = (LR.clip_layer(h.to(DEV).double(), dh3.to(DEV).double(), W, B, Mode(k)) for k in ("exact", "emu"))
    hg = h.to(DEV).requires_grad_(True)
    _begin(m)
    h3 = layer.run(hg, B, LR.VIT["T"])
    h3.backward(dh3.to(DEV))
    _finish(m)
    got = {"h3": h3.detach(), "dh": hg.grad}
    _check("layer_clip", name, got, emu, exact, keys=("h3", "dh"))
    assert m.arenas["vision"].grad_flat is None   # a frozen tower has no gradient storage to write to
    # without grad mode the forward keeps nothing for a backward and returns the same bits
    with torch.no_grad():
        assert torch.equal(layer.run(h.to(DEV), B, LR.VIT["T"]), got["h3"])


# ---- LoRA adapters in the layers ---------------------------------------------------------------------
ADAPTER = "step1"


@functools.lru_cache(maxsize=None)
def lora_model(p):
    """the tiny model under the lora policy (frozen base, adapters on every LM Linear and on ViT layers 1
    and 2), the adapters holding layer_refs.lora_weights"""
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    from cullavo_amd.lora import LoraSettings, module_seed
    assert module_seed(LR.LORA_SEED, 9, 2) == LR.module_seed(LR.LORA_SEED, 9, 2)
    s = LoraSettings(r=LR.LORA_R, lora_alpha=16.0, lora_dropout=p, adapter=ADAPTER, vision_layers=(1, 2))
    assert s.scaling == LR.LORA_SCALING
    m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable="lora", init="random", lora=s, seed=9)
    m.load_state_dict(LR.O.make_weights(LR.CFG, LR.WEIGHT_SEED), strict=False)
    W = LR.weights()
    for name, ar in m.arenas.items():
        if name != "lora":
            for k, q in ar.params.items():
                assert torch.equal(q.detach().cpu(), W[k]), k
    P = m.arenas["lora"].params
    with torch.no_grad():
        for tower, fmt, layers, groups in (("lm", "language_model.model.layers.{}.", (0, 1), LR.LM_GROUPS),
                                           ("vit", "vision_tower.vision_model.encoder.layers.{}.", (1, 2), LR.VIT_GROUPS)):
            for li in layers:
                for g, sufs in groups:
                    A, B = LR.lora_weights(tower, li)[g]
                    outs = LR.lora_group_shapes(tower)[g][1]
                    off = 0
                    for mi, suf in enumerate(sufs):
                        P[f"{fmt.format(li)}{suf}.lora_A.{ADAPTER}.weight"].copy_(A[mi * LR.LORA_R:(mi + 1) * LR.LORA_R])
                        P[f"{fmt.format(li)}{suf}.lora_B.{ADAPTER}.weight"].copy_(B[off:off + outs[mi]])
                        off += outs[mi]
    return m


def _lora_grads(m, pre, groups):
    P = m.arenas["lora"].params
    out = {}
    for g, sufs in groups:
        for ab in "AB":
            out[f"{g}.{ab}"] = torch.cat([P[f"{pre}{suf}.lora_{ab}.{ADAPTER}.weight"].grad for suf in sufs]).clone()
    return out


@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("name", list(LR.LORA_CASES))
def test_decoder_layer_with_adapters_against_f64(name, li):
    """adapters on all four groups of a decoder layer, dropout 0 and 0.05, the seed fixed through
    StepContext: forward and backward regenerate the same masks, keyed by the row the layer sees"""
    base, p = LR.LORA_CASES[name]
    g, h, dh3 = LR.decoder_case(base)
    got = _run_decoder(base, li, lora_model(p))
    W = LR.lm_layer_weights(li, device=DEV)
    exact, emu = (LR.decoder_layer(h.to(DEV).double(), dh3.to(DEV).double(), W, g, Mode(k),
                                   lora=LR.lora_case_groups(name, li, device=DEV)) for k in ("exact", "emu"))
    _check("layer_decoder_lora", f"{name}/layer{li}", got, emu, exact, keys=LR.LORA_KEYS, zero_rows=g.zero_rows)


@pytest.mark.parametrize("x_grad", [True, False])
@pytest.mark.parametrize("B,p", [(1, 0.05), (3, 0.0)])
def test_clip_layer_with_adapters_against_f64(B, p, x_grad):
    """ViT layer 1 with adapters on qkv / fc1 / fc2 over the frozen base; without an input gradient (the
    first adapted layer of the tower) the backward skips dx1 and layer_norm1 and still writes the adapters"""
    m = lora_model(p)
    li, T = 1, LR.VIT["T"]
    h, dh3 = LR.clip_case("b1" if B == 1 else "b3")
    layer = m.vision_tower.vision_model.encoder.layers[li]
    W = LR.clip_layer_weights(li, device=DEV)
    exact, emu = (LR.clip_layer(h.to(DEV).double(), dh3.to(DEV).double(), W, B, Mode(k),
                                lora=LR.lora_groups("vit", li, p, B * T, DEV)) for k in ("exact", "emu"))
    hg = h.to(DEV).requires_grad_(x_grad)
    _begin(m)
    h3 = layer.run(hg, B, T, LR.LORA_SEED)
    h3.backward(dh3.to(DEV))
    _finish(m)
    got = {"h3": h3.detach(), **_lora_grads(m, f"vision_tower.vision_model.encoder.layers.{li}.", LR.VIT_GROUPS)}
    if x_grad:
        got["dh"] = hg.grad
    else:
        assert hg.grad is None
    _check("layer_clip_lora", f"B{B}/p{p}/{'dh' if x_grad else 'nodh'}", got, emu, exact, keys=tuple(got))


CLIP_GRAD_KEYS = {"wqkv": [f"self_attn.{n}_proj.weight" for n in "qkv"], "bqkv": [f"self_attn.{n}_proj.bias" for n in "qkv"],
                  "wo": ["self_attn.out_proj.weight"], "bo": ["self_attn.out_proj.bias"], "w1": ["mlp.fc1.weight"],
                  "b1": ["mlp.fc1.bias"], "w2": ["mlp.fc2.weight"], "b2": ["mlp.fc2.bias"], "l1w": ["layer_norm1.weight"],
                  "l1b": ["layer_norm1.bias"], "l2w": ["layer_norm2.weight"], "l2b": ["layer_norm2.bias"]}


@pytest.mark.parametrize("x_grad", [True, False])
@pytest.mark.parametrize("name", list(LR.CLIP_CASES))
def test_trainable_clip_layer_against_f64(name, x_grad, monkeypatch):
    """a CLIP layer of a trainable tower (a policy only this test adds): every gradient the backward writes
    -- weights, biases, the fused qkv bias slot, both LayerNorms -- with an input gradient and, as the
    tower's first layer, without one but with a trainable layer_norm1 (dx1 is then recomputed)"""
    import cullavo_amd.modeling as MD
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    monkeypatch.setitem(MD.TRAINABLE_POLICIES, "everything",
                        {"vision": True, "projector": True, "embed": True, "layers": True, "head": True})
    m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable="everything", init="none")
    m.load_state_dict(LR.O.make_weights(LR.CFG, LR.WEIGHT_SEED))
    B, T = LR.CLIP_CASES[name]["B"], LR.VIT["T"]
    h, dh3 = LR.clip_case(name)
    layer = m.vision_tower.vision_model.encoder.layers[0]
    W = LR.clip_layer_weights(0, device=DEV)
    exact, emu = (LR.clip_layer(h.to(DEV).double(), dh3.to(DEV).double(), W, B, Mode(k)) for k in ("exact", "emu"))
    hg = h.to(DEV).requires_grad_(x_grad)
    _begin(m)
    h3 = layer.run(hg, B, T)
    h3.backward(dh3.to(DEV))
    _finish(m)
    P = m.arenas["vision"].params
    pre = "vision_tower.vision_model.encoder.layers.0."
    got = {"h3": h3.detach()}
    got.update({k: torch.cat([P[pre + n].grad for n in names]) for k, names in CLIP_GRAD_KEYS.items()})
    if x_grad:
        got["dh"] = hg.grad
    else:
        assert hg.grad is None
    _check("layer_clip_trainable", f"{name}/{'dh' if x_grad else 'nodh'}", got, emu, exact, keys=tuple(got))


# ---- projector ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_grad", [True, False])
@pytest.mark.parametrize("rows", LR.PROJECTOR_ROWS)
def test_projector_against_f64(rows, x_grad):
    from cullavo_amd.functions import ProjectorFn
    m = model()
    proj = m.multi_modal_projector
    x, dy = LR.projector_case(rows)
    W = LR.projector_weights(device=DEV)
    exact, emu = (LR.projector(x.to(DEV).double(), dy.to(DEV).double(), W, Mode(k)) for k in ("exact", "emu"))
    xg = x.to(DEV).requires_grad_(x_grad)
    _begin(m)
    y = ProjectorFn.apply(xg, proj, *proj.fn_params())
    y.backward(dy.to(DEV))
    _finish(m)
    P = m.arenas["projector"].params
    got = {"y": y.detach()}
    got.update({k: P["multi_modal_projector." + n].grad for k, n in LR.PROJ_GRAD_KEYS.items()})
    if x_grad:
        got["dx"] = xg.grad
    else:
        assert xg.grad is None
    _check("layer_projector", f"rows{rows}/{'dx' if x_grad else 'nodx'}", got, emu, exact, keys=tuple(got),
           exact_keys=("b2",) if rows == 1 else ())


# ---- head -------------------------------------------------------------------------------------------------
def _head_refs(name, with_dlogits):
    h, labels, mask, dlog = LR.head_case(name)
    W = LR.head_weights(device=DEV)
    return tuple(LR.head(h.to(DEV).double(), labels, mask, W, Mode(k), dlog.to(DEV).double() if with_dlogits else None)
                 for k in ("exact", "emu"))


def _head_grads(m):
    return {"n": m.arenas["layers"].params["language_model.model.norm.weight"].grad.clone(),
            "w": m.arenas["head"].params["language_model.lm_head.weight"].grad.clone()}


def _ce64(logits, tg):
    """f64 mean cross-entropy of the given logits over the supervised rows"""
    sup = tg != LR.IGNORE
    lg = logits.double()[sup]
    return float((torch.logsumexp(lg, -1) - lg.gather(1, tg[sup][:, None])[:, 0]).mean())


def _run_head_full(name, with_dlogits):
    from cullavo_amd import ops
    from cullavo_amd.functions import HeadLossFn
    m = model()
    lm = m.language_model
    h, labels, mask, dlog = LR.head_case(name)
    tg = ops.shift_targets(labels.to(DEV), mask.to(DEV), LR.IGNORE)
    assert torch.equal(tg.cpu(), LR.shift_targets(labels, mask))
    hg = h.to(DEV).requires_grad_(True)
    _begin(m)
    loss, logits = HeadLossFn.apply(hg, lm, tg, LR.IGNORE, *lm.head_params())
    if with_dlogits:
        torch.autograd.backward([loss, logits], [None, dlog.to(DEV)])
    else:
        loss.backward()
    _finish(m)
    return {"loss": float(loss.detach()), "logits": logits.detach(), "dh": hg.grad.clone(), **_head_grads(m)}, tg


@pytest.mark.parametrize("with_dlogits", [False, True])
@pytest.mark.parametrize("name", ["rows8", "rows24", "one-row"])
def test_head_loss_against_f64(name, with_dlogits):
    exact, emu = _head_refs(name, with_dlogits)
    got, tg = _run_head_full(name, with_dlogits)
    zero = None if with_dlogits else {"dh": ~exact["sup"]}
    _check("layer_head", f"{name}/{'dlogits' if with_dlogits else 'none'}", got, emu, exact,
           keys=("logits", "dh", "n", "w"), zero_rows=zero)
    ref = _ce64(got["logits"], tg)
    print(name, "loss", got["loss"], "f64 CE of the returned logits", ref, "emulated", emu["loss"], "exact", exact["loss"])
    assert abs(got["loss"] - ref) <= LR.LOSS_GATE * abs(ref)
    # and the issue's gate: the emulation's row losses summed in f32. It can hold only because at K = 256
    # the kernel's logits are the emulation's, bit for bit (bf16 products are exact in f32 and the f32
    # accumulation error almost never reaches a bf16 rounding boundary): the head ratios are exactly 1.0
    ref_emu = LR.f32_sum(emu["row_loss"]) / emu["count"]
    assert abs(got["loss"] - ref_emu) <= LR.LOSS_GATE * abs(ref_emu), (got["loss"], ref_emu)


@pytest.mark.parametrize("compact_in", [False, True])
@pytest.mark.parametrize("name", ["rows8", "rows24", "one-row"])
def test_head_loss_rows_against_f64(name, compact_in):
    from cullavo_amd import ops
    from cullavo_amd.functions import HeadLossRowsFn
    m = model()
    lm = m.language_model
    c = LR.HEAD_CASES[name]
    h, labels, mask, _ = LR.head_case(name)
    exact, emu = _head_refs(name, False)
    full, tg = _run_head_full(name, False)
    T = h.shape[0]
    rows = ops.supervised_rows(tg, c["n"], LR.IGNORE)
    assert int((rows < 0).sum()) == c["n"] - exact["count"] > 0
    src = LR.gather_rows(h.to(DEV), rows) if compact_in else h.to(DEV)
    hg = src.clone().requires_grad_(True)
    _begin(m)
    loss = HeadLossRowsFn.apply(hg, lm, tg, LR.IGNORE, rows, T, compact_in, *lm.head_params())
    loss.backward()
    _finish(m)
    dh = hg.grad
    if compact_in:   # compact rows in, compact gradient out: zero on the -1 slots, then to full height
        assert dh.shape == (c["n"], LR.LM["d"]) and (dh[rows < 0] == 0).all()
        dh = LR.scatter_rows(dh, rows, T)
    got = {"dh": dh, **_head_grads(m)}
    _check("layer_head_rows", f"{name}/{'compact' if compact_in else 'full'}", got, emu, exact, keys=("dh", "n", "w"),
           zero_rows={"dh": ~exact["sup"]})
    loss = float(loss.detach())
    print(name, "loss", loss, "HeadLossFn", full["loss"])
    assert abs(loss - full["loss"]) <= LR.LOSS_GATE * abs(full["loss"])


def test_head_with_every_row_ignored():
    """what the f64 reference gives with no supervised row (loss 0 / 0 = NaN, every gradient exactly 0),
    held for both head functions"""
    from cullavo_amd import ops
    from cullavo_amd.functions import HeadLossRowsFn
    exact, _ = _head_refs("all-ignored", False)
    assert exact["count"] == 0 and exact["loss"] != exact["loss"]
    got, tg = _run_head_full("all-ignored", False)
    print("all ignored: HeadLossFn loss", got["loss"])
    assert got["loss"] != got["loss"]
    for k in ("dh", "n", "w"):
        assert (got[k] == 0).all(), k
    m = model()
    lm = m.language_model
    h = LR.head_case("all-ignored")[0]
    rows = ops.supervised_rows(tg, 8, LR.IGNORE)
    assert (rows == -1).all()
    hg = h.to(DEV).requires_grad_(True)
    _begin(m)
    loss = HeadLossRowsFn.apply(hg, lm, tg, LR.IGNORE, rows, h.shape[0], False, *lm.head_params())
    loss.backward()
    _finish(m)
    loss = float(loss.detach())
    print("all ignored: HeadLossRowsFn loss", loss)
    assert loss != loss
    assert (hg.grad == 0).all() and all((t == 0).all() for t in _head_grads(m).values())


# ---- row movers ---------------------------------------------------------------------------------------------
def test_row_movers_bitwise():
    from cullavo_amd.functions import MergeFn, PackRowsFn, UnpackRowsFn
    rows = torch.tensor(LR.MOVER_ROWS, device=DEV)
    full, n, cols = LR.MOVER_FULL, len(LR.MOVER_ROWS), 256
    x = LR._randn("movers/x", full, cols, 1.0).to(DEV)
    dy = LR._randn("movers/dy", n, cols, 1.0).to(DEV)
    xg = x.clone().requires_grad_(True)
    y = PackRowsFn.apply(xg, rows)
    y.backward(dy)
    assert torch.equal(y, LR.gather_rows(x, rows)) and torch.equal(xg.grad, LR.scatter_rows(dy, rows, full))
    yg = dy.clone().requires_grad_(True)
    z = UnpackRowsFn.apply(yg, rows, full)
    z.backward(x)
    assert torch.equal(z, LR.scatter_rows(dy, rows, full)) and torch.equal(yg.grad, LR.gather_rows(x, rows))
    # MergeFn: out row i = text row src[i] | image row src[i] - n_text | a zero row (src -1); the backward
    # gathers dout at text_dst / img_dst (the transpose, given as a plan)
    n_text, n_img = 5, 4
    text, image = LR._randn("movers/text", n_text, cols, 1.0).to(DEV), LR._randn("movers/img", n_img, cols, 1.0).to(DEV)
    src = torch.tensor([0, 5, 6, -1, 1, 2, 7, 8, 3, 4, -1], device=DEV)
    text_dst = torch.tensor([0, 4, 5, 8, 9], device=DEV)
    img_dst = torch.tensor([1, 2, 6, 7], device=DEV)
    dout = LR._randn("movers/dout", src.numel(), cols, 1.0).to(DEV)
    tg_, ig_ = text.clone().requires_grad_(True), image.clone().requires_grad_(True)
    out = MergeFn.apply(tg_, ig_, src, text_dst, img_dst)
    out.backward(dout)
    assert torch.equal(out, LR.gather_rows(torch.cat([text, image]), src))
    assert torch.equal(tg_.grad, dout[text_dst]) and torch.equal(ig_.grad, dout[img_dst])
