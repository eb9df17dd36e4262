"""generate() as the reference calls it, host loop against device loop, on the 7B config with
random weights and the config-3 prompt (336 px image + 512 text tokens -> 1088 merged rows).

For batch 1 and 8, sampling (the reference's do_sample=True, temperature=0.9, top_k=50,
top_p=0.95) and greedy: alternating pairs, in one process, of
  host   generate(generator=...) / generate(): torch ops (generation.sample_next) between replays;
  device generate(seed=...) / generate(device_loop=True): the sampling kernel inside the graph.
Each figure is the wall time of the whole call (prefill, graph capture, every token) and, from it,
the decode time per token after subtracting a 1-token call of the same kind. Then the token choice
alone, event-timed: sample_next against ops.sample_token on [1, 32064] and [8, 32064] logits.
One JSON line per measurement.

  python tools/generate_bench.py [--new 256] [--pairs 5] [--batches 1,8] [--host-only]

--host-only runs the host half only; it uses nothing newer than generate(generator=...), so it also
runs on a commit without the device loop (the baseline check).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REF = dict(do_sample=True, temperature=0.9, top_k=50, top_p=0.95)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, iters=200, warm=20):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--text-len", type=int, default=513)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import llava_1_5_7b
    from cullavo_amd.data import synthetic_batch
    from cullavo_amd.generation import sample_next
    cfg = llava_1_5_7b()
    m = CuLLaVOModel(cfg, device="cuda", trainable="none", init="random", seed=0)
    m.eval()
    for B in (int(b) for b in a.batches.split(",")):
        sb = synthetic_batch(cfg, B, a.text_len, 35, seed=1234, device="cuda")
        inp = dict(input_ids=sb["input_ids"], pixel_values=sb["pixel_values"], attention_mask=sb["attention_mask"])
        for mode in ("sample", "greedy"):
            def host(n, i=0):
                if mode == "greedy":
                    return m.generate(**inp, max_new_tokens=n)
                return m.generate(**inp, max_new_tokens=n, **REF, generator=torch.Generator(device="cuda").manual_seed(i))

            def device(n, i=0):
                if mode == "greedy":
                    return m.generate(**inp, max_new_tokens=n, device_loop=True)
                return m.generate(**inp, max_new_tokens=n, **REF, seed=i)

            paths = [("host", host)] + ([] if a.host_only else [("device", device)])
            base = {}
            for name, fn in paths:  # warm-up, then the 1-token call that is subtracted
                fn(4)
                base[name] = min(timed(lambda: fn(1))[0] for _ in range(2))
            for pair in range(a.pairs):
                row = {"metric": "7B generate", "batch": B, "mode": mode, "new_tokens": a.new, "pair": pair}
                for name, fn in paths:
                    ms, out = timed(lambda: fn(a.new, pair))
                    assert out.shape[1] == inp["input_ids"].shape[1] + a.new
                    row[f"{name}_ms"] = round(ms, 2)
                    row[f"{name}_ms_per_token"] = round((ms - base[name]) / (a.new - 1), 4)
                if not a.host_only:
                    row["device_not_slower"] = row["device_ms"] <= row["host_ms"]
                print(json.dumps(row), flush=True)
    # the token choice alone
    for B in (int(b) for b in a.batches.split(",")):
        logits = (torch.randn(B, cfg.text_config.vocab_size, device="cuda") * 4).to(torch.bfloat16)
        gen = torch.Generator(device="cuda").manual_seed(0)
        row = {"metric": "token choice", "shape": [B, cfg.text_config.vocab_size],
               "sample_next_us": round(event_ms(lambda: sample_next(logits, **REF, generator=gen)) * 1e3, 2),
               "sample_next_greedy_us": round(event_ms(lambda: sample_next(logits, do_sample=False)) * 1e3, 2)}
        if not a.host_only:
            from cullavo_amd import ops
            nxt = torch.zeros(B, dtype=torch.int64, device="cuda")
            step = torch.zeros(B, dtype=torch.int64, device="cuda")
            fin = torch.zeros(B, dtype=torch.uint8, device="cuda")
            row["sample_token_us"] = round(event_ms(lambda: ops.sample_token(
                logits, next_ids=nxt, step=step, temperature=0.9, top_k=50, top_p=0.95, seed=1, finished=fin)) * 1e3, 2)
            row["sample_token_greedy_us"] = round(event_ms(lambda: ops.sample_token(
                logits, next_ids=nxt, step=step, do_sample=False, finished=fin)) * 1e3, 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
