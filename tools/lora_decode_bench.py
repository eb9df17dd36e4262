"""What a decode token costs on the model the reference generates with: LoRA adapters (r = 64) on all
seven Linears of every decoder layer, bf16 base weights and load_in_4bit (NF4 copies), with the
adapters' up-projection fused into the weight-streaming products (CULLAVO_DECODE_FUSE with "lora",
generation.FUSE_DECODE_LORA) and materialised (without: the route before the fusion, on kernels whose
code that switch does not touch).

7B shapes, random weights, lora_B filled (it starts at zero), the config-3 prompt (336 px image + 513
text tokens -> 1088 merged rows), batch 1 and 8. One child process per base format. In it, for each
batch, `--pairs` alternating pairs of (materialised, fused): prefill, capture the decode graph under
that setting, 16 warm-up replays, then `--new` timed replays between two device synchronisations
(greedy tokens fed back, as nf4_decode_bench.py). The pairs alternate inside one process on one model
so that both settings see the same weights, allocator state and neighbours; the spread of the
materialised runs is the yardstick for the difference. Launches per token: the library calls of one
eager decode step under each setting (a captured graph replays exactly those).
The same child also times the model with its adapters detached (lora groups off: the adapter-free
decode) once per batch, for the distance that is left.

One JSON line per measurement, a summary line per (base, batch) at the end.

  python tools/lora_decode_bench.py [--new 256] [--pairs 5] [--batches 1,8] [--bases bf16,nf4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(a):
    import torch

    from cullavo_amd import generation, ops
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import llava_1_5_7b
    from cullavo_amd.data import synthetic_batch
    from cullavo_amd.generation import DecodeGraph

    if not torch.cuda.is_available():
        raise SystemExit("lora_decode_bench: needs the GPU (no CPU timing)")
    cfg = llava_1_5_7b()
    m = CuLLaVOModel(cfg, device="cuda", trainable="lora", init="random", seed=0)
    ar = m.arenas["lora"]
    g = torch.Generator(device="cuda").manual_seed(1)
    ar.flat.copy_((0.02 * torch.randn(ar.numel, generator=g, device="cuda")).to(ar.dtype))
    if a.child == "nf4":
        from cullavo_amd.quant import quantize_lm_nf4_
        quantize_lm_nf4_(m)
    m.eval()
    text_len = 513
    L0 = text_len + cfg.vision_config.num_patches - 1

    def prefill(B):
        sb = synthetic_batch(cfg, B, text_len, 35, seed=1234, device="cuda")
        out = m._forward_cached(sb["input_ids"], sb["pixel_values"], sb["attention_mask"], None, None, None,
                                cfg.vision_feature_layer, cfg.vision_feature_select_strategy, None, True,
                                max_len=L0 + a.new + 24)
        return out.past_key_values, out.logits[:, -1]

    def ms_per_token(B, fuse):
        generation.FUSE_DECODE_LORA = fuse
        with torch.no_grad():
            cache, logits = prefill(B)
            graph = DecodeGraph(m, cache)
            for _ in range(16):
                logits = graph.step(logits.argmax(-1))[:, -1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.new):
                logits = graph.step(logits.argmax(-1))[:, -1]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.new * 1e3

    def launches(B, fuse):
        generation.FUSE_DECODE_LORA = fuse
        n = [0]
        inner = ops.call

        def counting(name, *args):
            n[0] += 1
            return inner(name, *args)

        with torch.no_grad():
            cache, logits = prefill(B)
            ops.call = counting
            try:
                m(input_ids=logits.argmax(-1)[:, None], past_key_values=cache, use_cache=True)
            finally:
                ops.call = inner
        return n[0]

    def say(row):
        print(json.dumps(row), flush=True)

    for B in (int(b) for b in a.batches.split(",")):
        base = {"metric": "7B LoRA decode", "base": a.child, "batch": B, "new_tokens": a.new}
        say({**base, "launches_per_token": {"materialised": launches(B, False), "fused": launches(B, True)}})
        t = {"materialised": [], "fused": []}
        for pair in range(a.pairs):
            for tag, fuse in (("materialised", False), ("fused", True)):
                t[tag].append(ms_per_token(B, fuse))
            say({**base, "pair": pair, "materialised_ms_per_token": round(t["materialised"][-1], 4),
                 "fused_ms_per_token": round(t["fused"][-1], 4)})
        # the adapter-free decode of the same model: every layer's groups detached for one run
        from cullavo_amd.lora import NO_LORA
        layers = m.language_model.model.layers
        kept = [layer.lora_groups for layer in layers]
        try:
            for layer in layers:
                layer.lora_groups = {k: NO_LORA for k in layer.lora_groups}
            free = ms_per_token(B, True)
        finally:
            for layer, lg in zip(layers, kept):
                layer.lora_groups = lg
        mat, fus = t["materialised"], t["fused"]
        say({**base, "summary": True, "pairs": a.pairs,
             "materialised_ms_per_token_median": round(statistics.median(mat), 4),
             "materialised_spread": round(max(mat) - min(mat), 4),
             "fused_ms_per_token_median": round(statistics.median(fus), 4),
             "fused_spread": round(max(fus) - min(fus), 4),
             "fused_not_slower_by_more_than_spread": statistics.median(fus) <= statistics.median(mat) + (max(mat) - min(mat)),
             "adapter_free_ms_per_token": round(free, 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--bases", default="bf16,nf4")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for base in a.bases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", base, "--new", str(a.new), "--pairs", str(a.pairs),
               "--batches", a.batches]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:
            if line.startswith("{"):
                sys.stdout.write(line)
                sys.stdout.flush()
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line)
        if p.wait() != 0:
            raise SystemExit(f"lora_decode_bench: the {base} child failed (exit status {p.returncode})")


if __name__ == "__main__":
    main()
