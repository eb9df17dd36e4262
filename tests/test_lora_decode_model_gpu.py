"""The decode step of a model with LoRA adapters (generation.layer_infer, FUSE_DECODE_LORA): the
adapters' up-projection in the epilogues of the weight-streaming products against the materialised
addend, on the tiny config with trainable="lora" and lora_B randomised, bf16 and after
quantize_lm_nf4_ (intermediate size 704 there, so down_proj has an NF4 copy too).

One prefill plus 6 decode steps give the same logits bit for bit with the flag on and off -- eager,
through the captured decode graph and on the ragged cache. With LoraGroup.up_project patched to raise,
the decode steps still run with the flag on (no product of the step materialises its term). A model
with r = 32 adapters, which the kernels do not take, still decodes: the flag changes nothing there
and the term comes from up_project.
"""
import dataclasses
import functools

import pytest
import torch

from oracle import cullavo_oracle as O

pytestmark = pytest.mark.gpu

STEPS = 6


@functools.lru_cache(maxsize=None)
def _model(kind):
    """kind: "bf16", "nf4" (r = 64 adapters on bf16 / NF4 base weights) or "r32" """
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    from cullavo_amd.lora import LoraSettings
    cfg = tiny_gpu()
    if kind == "nf4":
        cfg = dataclasses.replace(cfg, text_config=dataclasses.replace(cfg.text_config, intermediate_size=704))
    s = LoraSettings(r=32, lora_alpha=16.0) if kind == "r32" else LoraSettings()
    m = CuLLaVOModel(cfg, device="cuda", trainable="lora", init="random", lora=s, seed=11)
    ar = m.arenas["lora"]  # lora_B starts at zero: make the adapters' term count
    g = torch.Generator(device="cuda").manual_seed(12)
    ar.flat.copy_((0.05 * torch.randn(ar.numel, generator=g, device="cuda")).to(ar.dtype))
    if kind == "nf4":
        from cullavo_amd.quant import quantize_lm_nf4_
        quantize_lm_nf4_(m)
    m.eval()
    return m


def _prefill(m):
    cfg = O.config_small_gpu()
    ids, mask, pix, _ = O.make_inputs(cfg, 2, 20, 3, 41)
    return m(input_ids=ids.cuda(), pixel_values=pix.cuda(), attention_mask=mask.cuda(), use_cache=True)


def _decode(m, cache, mode):
    """6 decode steps on `cache`: the logits of every step"""
    from cullavo_amd.generation import DecodeGraph
    cfg = O.config_small_gpu()
    toks = torch.randint(2, cfg.image_token_index, (STEPS, 2), generator=torch.Generator().manual_seed(9)).cuda()
    if mode == "ragged":
        cache.make_ragged()
    graph = DecodeGraph(m, cache) if mode == "graph" else None
    out = []
    for i in range(STEPS):
        if graph is not None:
            out.append(graph.step(toks[i]).clone())
        else:
            out.append(m(input_ids=toks[i][:, None], past_key_values=cache, use_cache=True).logits.clone())
    torch.cuda.synchronize()
    return out


def _run(m, mode, monkeypatch, flag):
    from cullavo_amd import generation
    monkeypatch.setattr(generation, "FUSE_DECODE_LORA", flag)
    pre = _prefill(m)
    return [pre.logits.clone()] + _decode(m, pre.past_key_values, mode)


@pytest.mark.parametrize("mode", ["eager", "graph", "ragged"])
@pytest.mark.parametrize("kind", ["bf16", "nf4"])
def test_fused_decode_equals_materialised(monkeypatch, kind, mode):
    m = _model(kind)
    on = _run(m, mode, monkeypatch, True)
    off = _run(m, mode, monkeypatch, False)
    assert len(on) == len(off) == STEPS + 1
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.isfinite(a.float()).all(), i
        assert torch.equal(a, b), f"step {i}: fused and materialised logits differ"


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("kind", ["bf16", "nf4"])
def test_decode_steps_do_not_materialise_the_term(monkeypatch, kind, mode):
    """the decode steps (not the prefill, whose 704-wide gate|up modules the GEMM does not fuse) run
    with LoraGroup.up_project raising"""
    from cullavo_amd import generation, lora
    m = _model(kind)
    monkeypatch.setattr(generation, "FUSE_DECODE_LORA", True)
    pre = _prefill(m)
    want = _decode(m, pre.past_key_values, mode)
    pre = _prefill(m)

    def boom(self, u):
        raise AssertionError("LoraGroup.up_project called in a decode step")

    monkeypatch.setattr(lora.LoraGroup, "up_project", boom)
    got = _decode(m, pre.past_key_values, mode)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_adapters_move_the_logits(monkeypatch):
    """the comparison above is not vacuous: zeroed lora_B changes the decode logits"""
    m = _model("bf16")
    a = _run(m, "eager", monkeypatch, True)
    ar = m.arenas["lora"]
    keep = ar.flat.clone()
    try:
        with torch.no_grad():
            for key, p in ar.params.items():
                if ".lora_B." in key:
                    p.zero_()
        b = _run(m, "eager", monkeypatch, True)
    finally:
        ar.flat.copy_(keep)
    assert not torch.equal(a[-1], b[-1])


def test_r32_adapters_fall_back_to_the_materialised_route(monkeypatch):
    from cullavo_amd import lora
    m = _model("r32")
    calls = []
    real = lora.LoraGroup.up_project
    monkeypatch.setattr(lora.LoraGroup, "up_project", lambda self, u: (calls.append(1), real(self, u))[1])
    on = _run(m, "eager", monkeypatch, True)
    n_on = len(calls)
    off = _run(m, "eager", monkeypatch, False)
    n_layers = m.config.text_config.num_hidden_layers
    # four groups per layer and step, prefill included, whatever the flag says
    assert n_on == len(calls) - n_on == 4 * n_layers * (STEPS + 1)
    for a, b in zip(on, off):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
