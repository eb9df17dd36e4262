"""Decode at batch 17 .. 64: the wide weight-streaming product (cullavo_decode_linear_wide,
csrc/gemv_wide.hip) against ops.linear's tiles, the route every step above 16 rows took before it.

  products  the five 7B decode products (q|k|v 12288x4096, o 4096x4096 with its residual, gate|up
            22016x4096 with the SwiGLU, down 4096x11008 with its residual, lm_head 32064x4096) at
            M = 17, 32, 64 on ops.decode_linear_wide and on ops.linear (+ ops.swiglu_fwd for gate|up) over
            the same tensors, alternating, each launch on another copy of the weight (cold in the
            Infinity Cache, as in a decode step), HIP-event timed over back-to-back launches. A shape
            counts as a win where the wide median is below the tiles' median by more than the spread
            (max - min) of the tiles' own runs; everything else belongs in ops.WIDE_TILES_FASTER.
  model     ms per token of the 7B model (random weights) after the config-3 prompt (336 px image +
            513 text tokens), greedy, one HIP-graph replay per token, at batch 16, 32, 64 with
            CULLAVO_DECODE_WIDE's switch off and on in alternating pairs.

  python tools/wide_decode_bench.py [--skip-model] [--skip-products] [--rb N] [--ms 17,32,64]
                                    [--batches 16,32,64] [--pairs 5] [--tokens 32] [--out FILE]

--rb N (1, 2, 4): the kernel's lab switch CULLAVO_GEMV_WIDE_RB, weight blocks per workgroup (default:
the library's choice per product).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COLD_BYTES = 512 << 20  # twice the Infinity Cache


def timeit(fn, iters):
    import torch
    for _ in range(10):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def products(say, rec, ms, iters, runs):
    import torch

    from cullavo_amd import ops
    d, F, V = 4096, 11008, 32064
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: (0.02 * torch.randn(*s, device="cuda", generator=g)).bfloat16()
    shapes = (("qkv", 3 * d, d, False, False), ("o", d, d, False, True), ("gate_up", 2 * F, d, True, False),
              ("down", d, F, False, True), ("lm_head", V, d, False, False))
    for name, rows, K, swiglu, with_res in shapes:
        W0 = r(rows, K)
        nbytes = 2 * rows * K
        Ws = [W0] + [W0.clone() for _ in range(COLD_BYTES // nbytes)]
        turn = [0]

        def next_w():
            turn[0] = (turn[0] + 1) % len(Ws)
            return Ws[turn[0]]

        for M in ms:
            x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
            res = torch.randn(M, rows, device="cuda", generator=g).bfloat16() if with_res else None
            if swiglu:
                wide = lambda: ops.decode_linear_wide(x, next_w(), transform=3)
                tile = lambda: ops.swiglu_fwd(ops.linear(x, next_w()))
            else:
                wide = lambda: ops.decode_linear_wide(x, next_w(), residual=res)
                tile = lambda: ops.linear(x, next_w(), residual=res)
            a, b = wide().float(), tile().float()
            err = ((a - b).norm() / b.norm()).item()
            t = {"tiles": [], "wide": []}
            for _ in range(runs):  # alternate the two: the spread is part of the record
                t["tiles"].append(timeit(tile, iters))
                t["wide"].append(timeit(wide, iters))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = (max(t["tiles"]) - min(t["tiles"])) / med["tiles"]
            ratio = med["wide"] / med["tiles"]
            win = ratio < 1.0 - spread
            for tag in ("tiles", "wide"):
                say(f"product {name:8s} M={M:2d} {tag:5s} median {med[tag]:8.2f} us (runs "
                    f"{', '.join(f'{v:.2f}' for v in t[tag])})  {nbytes / med[tag] / 1e3:7.1f} GB/s of weights")
            say(f"product {name:8s} M={M:2d} wide / tiles {ratio:.3f}, tiles spread {spread:.3f}: "
                f"{'wide wins' if win else 'stays on the tiles'}; rel-L2 of the outputs {err:.2e}")
            rec.append(dict(part="product", name=name, rows=rows, K=K, M=M, tiles_us=t["tiles"], wide_us=t["wide"],
                            ratio=round(ratio, 4), tiles_spread=round(spread, 4), wide_wins=win, rel_l2=err))


def model(say, rec, batches, pairs, n_tok):
    import torch

    from cullavo_amd import generation
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import llava_1_5_7b
    from cullavo_amd.data import synthetic_batch
    from cullavo_amd.generation import DecodeGraph
    cfg = llava_1_5_7b()
    m = CuLLaVOModel(cfg, device="cuda", trainable="none", init="random", seed=0)
    m.eval()
    text_len = 513
    L0 = text_len + cfg.vision_config.num_patches - 1

    def ms_per_token(B, wide):
        generation.DECODE_WIDE = wide
        with torch.no_grad():
            sb = synthetic_batch(cfg, B, text_len, 35, seed=1234, device="cuda")
            out = m._forward_cached(sb["input_ids"], sb["pixel_values"], sb["attention_mask"], None, None, None,
                                    cfg.vision_feature_layer, cfg.vision_feature_select_strategy, None, True,
                                    max_len=L0 + n_tok + 24)
            cache, logits = out.past_key_values, out.logits[:, -1]
            del out
            graph = DecodeGraph(m, cache)
            for _ in range(8):
                logits = graph.step(logits.argmax(-1))[:, -1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_tok):
                logits = graph.step(logits.argmax(-1))[:, -1]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n_tok * 1e3

    default = generation.DECODE_WIDE
    for B in batches:
        t = {False: [], True: []}
        for _ in range(pairs):
            for wide in (False, True):
                t[wide].append(ms_per_token(B, wide))
        off, on = statistics.median(t[False]), statistics.median(t[True])
        spread = (max(t[False]) - min(t[False])) / off
        say(f"model 7B B={B:2d} switch off median {off:7.3f} ms/token (runs {', '.join(f'{v:.3f}' for v in t[False])})")
        say(f"model 7B B={B:2d} switch on  median {on:7.3f} ms/token (runs {', '.join(f'{v:.3f}' for v in t[True])})")
        say(f"model 7B B={B:2d} on / off {on / off:.3f}, off spread {spread:.3f}, {B / on * 1e3:.0f} tokens/s with the switch on")
        rec.append(dict(part="model", B=B, off_ms=t[False], on_ms=t[True], ratio=round(on / off, 4),
                        off_spread=round(spread, 4)))
    generation.DECODE_WIDE = default


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-products", action="store_true")
    ap.add_argument("--rb", type=int, default=0)
    ap.add_argument("--ms", default="17,32,64")
    ap.add_argument("--batches", default="16,32,64")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rb:
        os.environ["CULLAVO_GEMV_WIDE_RB"] = str(a.rb)  # read by the library at its first wide launch
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wide_decode_bench: needs the GPU (no CPU timing)")
    lines, rec = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"wide_decode_bench: rb {'library' if not a.rb else a.rb}, {torch.cuda.get_device_name(0)}")
    if not a.skip_products:
        products(say, rec, [int(v) for v in a.ms.split(",")], a.iters, a.runs)
    if not a.skip_model:
        model(say, rec, [int(v) for v in a.batches.split(",")], a.pairs, a.tokens)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            f.write("\n".join(json.dumps(r) for r in rec) + "\n")


if __name__ == "__main__":
    main()
