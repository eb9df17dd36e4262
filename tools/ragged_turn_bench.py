"""A batch of follow-up turns of unequal length on the ragged KV cache, in two parts.

Kernel level (random caches, no weights): ops.attn_fwd_ragged at uniform lengths against
ops.attn_fwd_cached at the same shapes (B 8, H 32, D 128, past 1088, Lq 16 / 64 / 512), alternating
--rounds times after a warm-up of each, each timing --iters launches between two device events. The
ragged kernel adds a few scalar loads per workgroup; the figure to read is whether its difference
from attn_fwd_cached stays inside the spread attn_fwd_cached's own repeats show.

Model level (the 7B config, random weights): after the config-3 prompt (336 px image + 513 text
tokens -> 1088 merged rows) is cached for 8 conversations, a second turn whose questions have
lengths 8, 16, ..., 64 runs as ONE ragged call followed by 64 decode steps (generate on the ragged
cache), against the only correct route before the ragged cache: the eight conversations continued
one at a time at batch 1. Host clock around work that ends in a device synchronise; the two
alternate --rounds times after a warm-up of each; medians. Prints one JSON line per part.

  python tools/ragged_turn_bench.py [--level kernel|model|both] [--rounds 5] [--iters 20]
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
    B, H, D, past = 8, 32, 128, 1088
    out = []
    for Lq in (16, 64, 512):
        g = torch.Generator().manual_seed(Lq)
        q = torch.randn(B * Lq, H * D, generator=g).to(torch.bfloat16).cuda()
        kc = torch.randn(B, past + Lq, H * D, generator=g).to(torch.bfloat16).cuda()
        vc = torch.randn(B, past + Lq, H * D, generator=g).to(torch.bfloat16).cuda()
        kv_len = torch.full((B,), past + Lq, dtype=torch.int32, device="cuda")
        q_pad = torch.zeros(B, dtype=torch.int32, device="cuda")
        o = torch.empty(B * Lq, H * D, dtype=torch.bfloat16, device="cuda")

        def cached():
            ops.attn_fwd_cached(q, kc, vc, B=B, H=H, Lq=Lq, past=past, D=D, scale=D ** -0.5, out=o)

        def ragged():
            ops.attn_fwd_ragged(q, kc, vc, kv_len, B=B, H=H, Lq=Lq, D=D, scale=D ** -0.5, q_pad=q_pad, out=o)

        def clock(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / iters  # us per launch

        clock(cached), clock(ragged)
        tc, tr = [], []
        for _ in range(rounds):
            tc.append(clock(cached))
            tr.append(clock(ragged))
        out.append({"Lq": Lq, "cached_us": [round(t, 1) for t in tc], "ragged_us": [round(t, 1) for t in tr],
                    "cached_us_median": round(median(tc), 1), "ragged_us_median": round(median(tr), 1),
                    "cached_spread_us": round(max(tc) - min(tc), 1),
                    "ragged_minus_cached_us": round(median(tr) - median(tc), 1)})
    print(json.dumps({"metric": "attn_fwd_ragged vs attn_fwd_cached, uniform lengths", "B": B, "H": H, "D": D,
                      "past": past, "iters": iters, "shapes": out}), flush=True)


def model_level(rounds: int, text_len: int, steps: int):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import llava_1_5_7b
    from cullavo_amd.data import synthetic_batch
    from cullavo_amd.generation import KVCache
    cfg = llava_1_5_7b()
    B = 8
    m = CuLLaVOModel(cfg, device="cuda", trainable="none", init="random", seed=0)
    m.eval()
    sb = synthetic_batch(cfg, B, text_len, 35, seed=1234, device="cuda")
    ids, mask, pix = sb["input_ids"], sb["attention_mask"], sb["pixel_values"]
    g = torch.Generator().manual_seed(7)
    lens = [8 * (b + 1) for b in range(B)]
    S = max(lens)
    turns = [torch.randint(2, cfg.image_token_index, (1, n), generator=g).cuda() for n in lens]
    block = torch.full((B, S), cfg.pad_token_id, dtype=torch.long, device="cuda")
    bmask = torch.zeros(B, S, dtype=torch.long, device="cuda")
    for b, t in enumerate(turns):
        block[b, S - lens[b]:] = t[0]
        bmask[b, S - lens[b]:] = 1

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    with torch.no_grad():
        cache = m(input_ids=ids, pixel_values=pix, attention_mask=mask, use_cache=True).past_key_values
        rows = cache.get_seq_length()
        cache.grow(rows + S + steps + 1)
        pos0 = cache.next_pos.clone()
        solo = []
        for b in range(B):
            c = KVCache(len(cache), 1, rows + S + steps + 1, cache.H, cache.D, cache.k.device)
            c.k[:, :, :rows].copy_(cache.k[:, b:b + 1, :rows])
            c.v[:, :, :rows].copy_(cache.v[:, b:b + 1, :rows])
            c.kv_start = cache.kv_start[b:b + 1].clone()
            solo.append(c)

        def ragged():
            cache.length, cache.lengths, cache.next_pos = rows, None, pos0.clone()  # the same turn again
            return m.generate(input_ids=block, attention_mask=bmask, past_key_values=cache, max_new_tokens=steps + 1)

        def one_by_one():
            outs = []
            for b, c in enumerate(solo):
                c.length, c.lengths, c.next_pos = rows, None, pos0[b:b + 1].clone()
                outs.append(m.generate(input_ids=turns[b], past_key_values=c, max_new_tokens=steps + 1))
            return outs

        _, gr = clock(ragged)
        _, gs = clock(one_by_one)
        same = sum(int(torch.equal(gr[b, S:], gs[b][0, lens[b]:])) for b in range(B))
        tr, ts = [], []
        for _ in range(rounds):
            tr.append(clock(ragged)[0])
            ts.append(clock(one_by_one)[0])
    print(json.dumps({"metric": "7B ragged second turn (8 questions of 8..64 tokens) + decode steps", "batch": B,
                      "prompt_rows": rows, "decode_steps": steps, "ragged_ms": [round(t, 1) for t in tr],
                      "one_by_one_ms": [round(t, 1) for t in ts], "ragged_ms_median": round(median(tr), 1),
                      "one_by_one_ms_median": round(median(ts), 1),
                      "rows_with_identical_greedy_tokens": f"{same}/{B}"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", choices=("kernel", "model", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--text-len", type=int, default=513)
    ap.add_argument("--steps", type=int, default=64)
    a = ap.parse_args()
    if a.level in ("kernel", "both"):
        kernel_level(a.rounds, a.iters)
    if a.level in ("model", "both"):
        model_level(a.rounds, a.text_len, a.steps)


if __name__ == "__main__":
    main()
