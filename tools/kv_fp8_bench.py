"""What the FP8 KV cache costs and gains, in two parts (results: profiles/r20/kv_fp8/).

Kernel level (random caches, no weights): ops.attn_decode on a bf16 cache against
ops.attn_decode_fp8 on codes + exponents at the 7B head geometry (H 32, D 128), batch 1 / 8 / 32 at
1088 and 2112 keys. The two alternate --rounds times after a warm-up of each; each timing is --iters
launches between two device events (back to back, so the caches of one launch are warm for the
next only through L2 / MALL: at these sizes, 36 MB to 1.1 GB of K and V per call, mostly not).
Medians and the spread (max - min) of each.

Model level (the 7B config, random weights, the config-3 prompt: 336 px image + 513 text tokens ->
1088 merged rows): greedy generate() of 256 and 1000 new tokens at batch 1 and 8 with the decode
graph, for kv_cache_dtype "bf16", "fp8_sim" and "fp8", alternating --rounds times in one process
after one warm-up each. ms/token = (generate(N) - generate(1)) / (N - 1): the prefill and the first
sample are timed on their own and subtracted. "fp8" against "fp8_sim" is the kernels' effect at
identical tokens (checked); "fp8" against "bf16" is what a caller gets.

  python tools/kv_fp8_bench.py [--level kernel|model|both] [--rounds 5] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median(x):
    return sorted(x)[len(x) // 2]


def kernel_level(rounds: int, iters: int):
    from cullavo_amd import ops
    H, D = 32, 128
    out = []
    for B in (1, 8, 32):
        for L in (1088, 2112):
            g = torch.Generator(device="cuda").manual_seed(B * 10000 + L)
            q = torch.randn(B, H * D, generator=g, device="cuda").to(torch.bfloat16)
            k = torch.randn(B * L, H * D, generator=g, device="cuda").to(torch.bfloat16)
            v = torch.randn(B * L, H * D, generator=g, device="cuda").to(torch.bfloat16)
            kc8 = torch.empty(B, L, H * D, dtype=torch.uint8, device="cuda")
            vc8 = torch.empty_like(kc8)
            ke = torch.empty(B, L, H, dtype=torch.uint8, device="cuda")
            ve = torch.empty_like(ke)
            zero = torch.zeros(B, dtype=torch.int32, device="cuda")
            ops.kv_append_fp8(k, v, kc8, vc8, ke, ve, zero, B=B, Lnew=L, H=H, D=D)
            kc, vc = k.view(B, L, H * D), v.view(B, L, H * D)
            kv_len = torch.full((B,), L, dtype=torch.int32, device="cuda")
            o = torch.empty(B, H * D, dtype=torch.bfloat16, device="cuda")
            kw = dict(B=B, H=H, D=D, max_len=L, scale=D ** -0.5, out=o)

            def bf16():
                ops.attn_decode(q, kc, vc, kv_len, **kw)

            def fp8():
                ops.attn_decode_fp8(q, kc8, vc8, ke, ve, kv_len, **kw)

            def clock(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / iters  # us per call (both launches and the workspace)

            clock(bf16), clock(fp8)
            tb, tf = [], []
            for _ in range(rounds):
                tb.append(clock(bf16))
                tf.append(clock(fp8))
            kv_bytes = 2 * B * L * H * D
            out.append({"B": B, "keys": L, "bf16_us": [round(t, 1) for t in tb], "fp8_us": [round(t, 1) for t in tf],
                        "bf16_us_median": round(median(tb), 1), "fp8_us_median": round(median(tf), 1),
                        "bf16_spread_us": round(max(tb) - min(tb), 1), "fp8_spread_us": round(max(tf) - min(tf), 1),
                        "fp8_over_bf16": round(median(tf) / median(tb), 3),
                        "bf16_kv_MB": round(2 * kv_bytes / 1e6, 1), "fp8_kv_MB": round((kv_bytes + 2 * B * L * H) / 1e6, 1)})
            del k, v, kc8, vc8
    print(json.dumps({"metric": "attn_decode (bf16 cache) vs attn_decode_fp8 (codes + exponents), per call",
                      "H": H, "D": D, "iters": iters, "shapes": out}), flush=True)


def model_level(rounds: int, text_len: int, batches, new_tokens):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import llava_1_5_7b
    from cullavo_amd.data import synthetic_batch
    cfg = llava_1_5_7b()
    m = CuLLaVOModel(cfg, device="cuda", trainable="none", init="random", seed=0)
    m.eval()
    dtypes = ("bf16", "fp8_sim", "fp8")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for B in batches:
        sb = synthetic_batch(cfg, B, text_len, 35, seed=1234, device="cuda")
        kw = dict(input_ids=sb["input_ids"], pixel_values=sb["pixel_values"], attention_mask=sb["attention_mask"])
        # generate(1): the prefill and the first sample, per dtype (median of 3 after a warm-up)
        first = {}
        for dt in dtypes:
            clock(lambda: m.generate(**kw, max_new_tokens=1, kv_cache_dtype=dt))
            first[dt] = median([clock(lambda: m.generate(**kw, max_new_tokens=1, kv_cache_dtype=dt))[0]
                                for _ in range(3)])
        for N in new_tokens:
            toks = {dt: clock(lambda: m.generate(**kw, max_new_tokens=N, kv_cache_dtype=dt))[1] for dt in dtypes}
            t = {dt: [] for dt in dtypes}
            for _ in range(rounds):
                for dt in dtypes:
                    ms, _ = clock(lambda: m.generate(**kw, max_new_tokens=N, kv_cache_dtype=dt))
                    t[dt].append((ms - first[dt]) / (N - 1))
            rec = {"metric": "7B generate, ms per decoded token (graph replay, greedy)", "batch": B,
                   "prompt_rows": int(sb["input_ids"].shape[1]) + cfg.vision_config.num_patches - 1,
                   "new_tokens": N, "prefill_plus_first_ms": {dt: round(first[dt], 1) for dt in dtypes},
                   "fp8_tokens_equal_fp8_sim": bool(torch.equal(toks["fp8"], toks["fp8_sim"]))}
            for dt in dtypes:
                rec[dt + "_ms_per_token"] = [round(x, 3) for x in t[dt]]
                rec[dt + "_median"] = round(median(t[dt]), 3)
                rec[dt + "_spread"] = round(max(t[dt]) - min(t[dt]), 3)
            rec["fp8_over_fp8_sim"] = round(rec["fp8_median"] / rec["fp8_sim_median"], 4)
            rec["fp8_over_bf16"] = round(rec["fp8_median"] / rec["bf16_median"], 4)
            print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", choices=("kernel", "model", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--text-len", type=int, default=513)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--new-tokens", type=int, nargs="+", default=[256, 1000])
    a = ap.parse_args()
    if a.level in ("kernel", "both"):
        kernel_level(a.rounds, a.iters)
    if a.level in ("model", "both"):
        with torch.no_grad():
            model_level(a.rounds, a.text_len, a.batches, a.new_tokens)


if __name__ == "__main__":
    main()
