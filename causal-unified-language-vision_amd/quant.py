"""NF4 base weights for the language model (the reference's QLoRA recipe).

Reference: prepare_cullavo(bits=4) loads every decoder-layer nn.Linear as bitsandbytes NF4 with
bnb_4bit_compute_dtype=bfloat16, skipping lm_head and the projector
(cullavo/load_cullavo.py:66-83); it trains its LoRA adapters and runs the step-2 generate() on
that 4-bit model.

Here (csrc/nf4.hip; the format is in INTEGRATION.md "NF4"): quantize_lm_nf4_ quantises the fused
q|k|v, o, gate|up and down weights of every decoder layer, keeps the codes and absmax on the layer
and writes the dequantised values back into the bf16 arena. Prefill and training GEMMs then run
the existing bf16 kernels on exactly the weights the 4-bit model has, and the decode step streams
the 4.5-bit copies (generation.layer_infer -> ops.nf4_decode_linear). The bf16 copies are kept, no
double quantisation of absmax, no 8-bit path, the vision tower stays bf16; bitsandbytes itself is
not used.

A layer's NF4 copies are valid for the arena state they were made from (ParamArena._state(): torch
writes and kernel writes alike). An optimizer step on the base weights or a checkpoint load changes
that state, and nf4_weights() then drops the copies instead of decoding from stale ones: the layer
is back on the bf16 GEMV until quantize_lm_nf4_ runs again. With trainable="lora" the base is
frozen and the copies stay.
"""
from __future__ import annotations

import warnings

import torch

from . import ops

NF4_BLOCK = 64


def nf4_weights(layer) -> dict:
    """{"qkv" | "o" | "gu" | "down": (codes, absmax)} of a decoder layer; empty when the layer was
    never quantised or its arena was written since (the stale copies are dropped)."""
    q = getattr(layer, "_nf4", None)
    if not q:
        return {}
    if layer._nf4_state != layer._arena._state():
        # the state covers the layer's whole arena (every decoder layer and its norms share one
        # buffer and one write counter): any write to it drops every layer's copies. Safe, and said
        # aloud, because decode is back on the bf16 GEMV until quantize_lm_nf4_ runs again.
        # The tensors may still be referenced by a captured DecodeGraph, which keeps them alive
        # (DecodeGraph.nf4_refs) for as long as it can be replayed.
        warnings.warn(f"{layer._lp}: the decoder-layer arena was written after quantize_lm_nf4_; its NF4 "
                      "copies are dropped and decode runs on the bf16 GEMV until quantize_lm_nf4_ is called again",
                      RuntimeWarning, stacklevel=2)
        invalidate_nf4(layer)
        return {}
    return q


def invalidate_nf4(layer) -> None:
    """Drop a decoder layer's NF4 copies (its base weights changed)."""
    layer._nf4 = None
    layer._nf4_state = None


def _member_keys(layer, which: str) -> list[str]:
    lp = layer._lp
    return {"qkv": [lp + f"self_attn.{n}_proj.weight" for n in "qkv"],
            "o": [lp + "self_attn.o_proj.weight"],
            "gu": [lp + "mlp.gate_proj.weight", lp + "mlp.up_proj.weight"],
            "down": [lp + "mlp.down_proj.weight"]}[which]


@torch.no_grad()
def quantize_lm_nf4_(model) -> dict:
    """Quantise the decoder layers' Linear weights of `model` (a CuLLaVOModel or its
    LlamaForCausalLM) to NF4 in place; see the module docstring. Returns a report:
    {"quantized": [parameter keys], "skipped": [keys left bf16 because K % 64 != 0],
     "kept": [keys whose NF4 copies were still valid], "nf4_bytes", "bf16_bytes"}.
    Idempotent: layers whose copies are valid are left alone, so a second call changes no bit."""
    lm = getattr(model, "language_model", model)
    layers = list(lm.model.layers)
    report = {"quantized": [], "skipped": [], "kept": [], "nf4_bytes": 0, "bf16_bytes": 0}
    if not layers:
        return report
    arenas = {id(l._arena): l._arena for l in layers}
    for ar in list(getattr(model, "arenas", {}).values()) + list(arenas.values()):
        ar.wait_update()  # pending optimizer updates (FusedAdamW overlap), as generate() does
    fresh = []
    for layer in layers:
        ar = layer._arena
        if ar.dtype != torch.bfloat16:
            raise NotImplementedError("NF4 base weights need the bf16 model (the f32 mode is a parity mode)")
        if nf4_weights(layer):
            for which in layer._nf4:
                report["kept"] += _member_keys(layer, which)
            for which in layer._nf4_skipped:
                report["skipped"] += _member_keys(layer, which)
            continue
        q, skipped = {}, []
        for which, (key, shape) in layer._kmajor_specs().items():
            N, K = shape
            if K % NF4_BLOCK != 0:
                skipped.append(which)
                report["skipped"] += _member_keys(layer, which)
                continue
            w = ar.view(key, shape)
            codes, absmax = ops.nf4_quantize(w)
            ops.nf4_dequantize(codes, absmax, out=w)
            q[which] = (codes, absmax)
            report["quantized"] += _member_keys(layer, which)
            report["nf4_bytes"] += codes.numel() + 4 * absmax.numel()
            report["bf16_bytes"] += 2 * N * K
        layer._nf4, layer._nf4_skipped = q, skipped
        fresh.append(layer)
    # the dequantised values were written by kernels on raw pointers: tell the arenas (their K-major
    # copies refresh), then stamp every valid layer with the state its copies now belong to
    for ar in {id(l._arena): l._arena for l in fresh}.values():
        ar.note_written()
    for layer in layers:
        if layer._nf4 is not None:
            layer._nf4_state = layer._arena._state()
    return report
