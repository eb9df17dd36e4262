"""NF4 decode against the bf16 GEMV, in one process, HIP-event timed after warm-up.

  products  the four decode products of the 7B layer at batch 1 and 8 -- q|k|v 12288 x 4096, o
            4096 x 4096, gate|up 2 x 11008 x 4096 with the SwiGLU output, down 4096 x 11008 -- on
            ops.decode_linear / ops.linear (bf16 weights) and on ops.nf4_decode_linear (NF4 copies),
            alternating, each launch on another copy of the weight (cold in the Infinity Cache, as in a decode
            step), with the weight bytes each reads over its time against 6.3 TB/s;
  model     ms per token of the 7B model after the config-3 prompt (336 px image + 513 text tokens),
            one HIP-graph replay per token as bench.py --workload decode times it: bf16, then the
            same model after quant.quantize_lm_nf4_ on the NF4 copies and (CULLAVO_NF4_DECODE=0's
            path) on the bf16 GEMV over the dequantised arena.

  python tools/nf4_decode_bench.py [--skip-model] [--batches 1,8] [--iters N] [--tokens 64] [--out FILE]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cullavo_amd import generation, ops  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s
COLD_BYTES = 640 << 20   # distinct weight bytes cycled through per timed path
ITERS = 0                # --iters: launches per timed run (0: 200)
BATCHES = (1, 8)         # --batches


def timeit(fn, iters=200):
    iters = ITERS or iters
    for _ in range(10):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def products(say):
    d, F = 4096, 11008
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: (0.02 * torch.randn(*s, device="cuda", generator=g)).bfloat16()
    shapes = (("qkv", 3 * d, d, False), ("o", d, d, False), ("gate_up", 2 * F, d, True), ("down", d, F, False))
    for name, N, K, swiglu in shapes:
        # enough distinct copies of the weight, taken in turn, that no launch finds its weight in the
        # 256 MiB Infinity Cache (a decode step streams 13 GB between two uses of a weight)
        W0 = r(N, K)
        codes0, absmax0 = ops.nf4_quantize(W0)
        ops.nf4_dequantize(codes0, absmax0, out=W0)  # the arena's values: both paths on the same weights
        b_bf, b_nf = 2 * N * K, codes0.numel() + 4 * absmax0.numel()
        Ws = [W0] + [W0.clone() for _ in range(COLD_BYTES // b_bf)]
        Qs = [(codes0, absmax0)] + [(codes0.clone(), absmax0.clone()) for _ in range(COLD_BYTES // b_nf)]
        turn = {"bf": 0, "nf": 0}

        def next_w():
            turn["bf"] = (turn["bf"] + 1) % len(Ws)
            return Ws[turn["bf"]]

        def next_q():
            turn["nf"] = (turn["nf"] + 1) % len(Qs)
            return Qs[turn["nf"]]

        for B in BATCHES:
            x = torch.randn(B, K, device="cuda", generator=g).bfloat16()
            if swiglu:
                bf = lambda: ops.decode_linear(x, next_w(), transform=3)
                nf = lambda: ops.nf4_decode_linear(x, *next_q(), swiglu_out=True)
            else:
                bf = lambda: ops.linear(x, next_w())
                nf = lambda: ops.nf4_decode_linear(x, *next_q())
            err = ((nf().float() - bf().float()).norm() / bf().float().norm()).item()
            t = {"bf16": [], "nf4": []}
            for _ in range(3):  # alternate the two: the spread is part of the record
                t["bf16"].append(timeit(bf))
                t["nf4"].append(timeit(nf))
            for tag, nbytes in (("bf16", b_bf), ("nf4", b_nf)):
                us = min(t[tag])
                say(f"product {name:8s} B={B} {tag:5s} {us:8.2f} us (runs {', '.join(f'{v:.2f}' for v in t[tag])})  "
                    f"{nbytes / us / 1e3:7.1f} GB/s of weights = {nbytes / (us * 1e-6) / HBM_ACHIEVABLE:5.3f} of 6.3 TB/s")
            say(f"product {name:8s} B={B} nf4 / bf16 time {min(t['nf4']) / min(t['bf16']):.3f}, rel-L2 of the outputs {err:.2e}")


def model(say, n_tok):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import llava_1_5_7b
    from cullavo_amd.data import synthetic_batch
    from cullavo_amd.generation import DecodeGraph
    from cullavo_amd.quant import quantize_lm_nf4_

    cfg = llava_1_5_7b()
    m = CuLLaVOModel(cfg, device="cuda", trainable="none", init="random", seed=0)
    m.eval()
    text_len = 513
    L0 = text_len + cfg.vision_config.num_patches - 1

    def ms_per_token(B):
        sb = synthetic_batch(cfg, B, text_len, 35, seed=1234, device="cuda")
        with torch.no_grad():
            out = m._forward_cached(sb["input_ids"], sb["pixel_values"], sb["attention_mask"], None, None, None,
                                    cfg.vision_feature_layer, cfg.vision_feature_select_strategy, None, True,
                                    max_len=L0 + n_tok + 24)
            cache, logits = out.past_key_values, out.logits[:, -1]
            graph = DecodeGraph(m, cache)
            for _ in range(16):
                logits = graph.step(logits.argmax(-1))[:, -1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_tok):
                logits = graph.step(logits.argmax(-1))[:, -1]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n_tok * 1e3

    for B in (1, 8):
        say(f"model 7B B={B} bf16                         {ms_per_token(B):7.3f} ms/token")
    t0 = time.perf_counter()
    rep = quantize_lm_nf4_(m)
    torch.cuda.synchronize()
    say(f"quantize_lm_nf4_: {len(rep['quantized'])} weights, {rep['bf16_bytes'] / 1e9:.2f} GB bf16 -> "
        f"{rep['nf4_bytes'] / 1e9:.2f} GB NF4, {time.perf_counter() - t0:.2f} s")
    for B in (1, 8):
        for on in (True, False, True):
            generation.NF4_DECODE = on
            tag = "nf4 copies" if on else "bf16 GEMV on the dequantised arena"
            say(f"model 7B B={B} load_in_4bit, {tag:34s} {ms_per_token(B):7.3f} ms/token")
    generation.NF4_DECODE = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--batches", default="1,8", help="batch sizes of the product runs")
    ap.add_argument("--iters", type=int, default=0, help="launches per timed product run (default 200; small for a counter run)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nf4_decode_bench: needs the GPU (no CPU timing)")
    torch.cuda.set_device(0)
    global ITERS, BATCHES
    ITERS, BATCHES = a.iters, tuple(int(b) for b in a.batches.split(","))

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    products(say)
    if not a.skip_model:
        model(say, a.tokens)


if __name__ == "__main__":
    main()
