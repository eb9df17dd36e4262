"""A follow-up turn on the 7B config: the wall time of one cached forward over --new tokens after the
config-3 prompt (336 px image + 513 text tokens -> 1088 merged rows) is already in the KV cache,
against what that turn cost before cullavo_attn_fwd_cached: a full prefill of prompt + new tokens.
Host clock around work that ends in a device synchronise; the two alternate --rounds times after a
warm-up of each. Prints one JSON line.

  python tools/continuation_bench.py [--batch 1] [--new 64] [--text-len 513] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--text-len", type=int, default=513)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import llava_1_5_7b
    from cullavo_amd.data import synthetic_batch
    cfg = llava_1_5_7b()
    m = CuLLaVOModel(cfg, device="cuda", trainable="none", init="random", seed=0)
    m.eval()
    sb = synthetic_batch(cfg, a.batch, a.text_len, 35, seed=1234, device="cuda")
    ids, mask, pix = sb["input_ids"], sb["attention_mask"], sb["pixel_values"]
    g = torch.Generator().manual_seed(7)
    new = torch.randint(2, cfg.image_token_index, (a.batch, a.new), generator=g).cuda()
    ids_all = torch.cat([ids, new], 1)
    mask_all = torch.ones_like(ids_all)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    with torch.no_grad():
        cache = m(input_ids=ids, pixel_values=pix, attention_mask=mask, use_cache=True).past_key_values
        prompt_rows = cache.get_seq_length()
        cache.grow(prompt_rows + a.new)
        state = (cache.length, cache.next_pos.clone())

        def cont():
            cache.length, cache.next_pos = state[0], state[1].clone()  # the same turn again
            return m(input_ids=new, past_key_values=cache, use_cache=True).logits

        def reprefill():
            return m(input_ids=ids_all, pixel_values=pix, attention_mask=mask_all, use_cache=True).logits

        _, lc = clock(cont)
        _, lf = clock(reprefill)
        rel = ((lc.float() - lf[:, -a.new:].float()).norm() / lf[:, -a.new:].float().norm()).item()
        tc, tf = [], []
        for _ in range(a.rounds):
            tc.append(clock(cont)[0])
            tf.append(clock(reprefill)[0])
    print(json.dumps({"metric": "7B continuation after a cached prompt", "batch": a.batch, "prompt_rows": prompt_rows,
                      "new_tokens": a.new, "continuation_ms": [round(t, 2) for t in tc],
                      "reprefill_ms": [round(t, 2) for t in tf],
                      "continuation_ms_median": round(sorted(tc)[len(tc) // 2], 2),
                      "reprefill_ms_median": round(sorted(tf)[len(tf) // 2], 2),
                      "logits_rel_l2_vs_reprefill": rel}))


if __name__ == "__main__":
    main()
