"""The packed training step against the padded one (CuLLaVOModel.packed_rows), on the 7B config-3 step at
batch 8 (one GPU): ms/step of both, interleaved and warm, beside the share of the B * L rows that is attended.

  python tools/packed_step_bench.py [--trainable full|lora] [--steps 6] [--warmup 2] [--out FILE]

Two batches:
  ragged   text lengths spread evenly from 64 to 513 tokens on 576 image rows, right-padded to 513: a
           SYNTHETIC spread (the padding share of real lbkllava batches is not measured). Timed padded
           (switch off) and packed (switch on), alternating step by step.
  uniform  the config-3 batch (every row 513 tokens, no padding), switch off and on alternating: the
           packed path is not taken, so the switch must cost nothing.
A step is trainer.train_step (forward, backward, optimizer), host clock around a device synchronise.
On a tree without the switch (the parent commit, for the baseline the padded numbers are quoted against)
only the padded figures are measured. One JSON line per batch on stdout (and appended to --out).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ragged(batch, cfg, lens):
    """right-pad row b of a synthetic config-3 batch to lens[b] text tokens"""
    import torch
    ids, mask, labels = batch["input_ids"].clone(), batch["attention_mask"].clone(), batch["labels"].clone()
    P = cfg.vision_config.num_patches
    for b, n in enumerate(lens):
        ids[b, n:] = cfg.pad_token_id
        mask[b, n:] = 0
        labels[b, n + P - 1:] = cfg.ignore_index
    out = dict(batch, input_ids=ids, attention_mask=mask, labels=labels)
    out["num_supervised"] = int((labels[:, 1:] != cfg.ignore_index).sum())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trainable", default="full", choices=["full", "lora"])
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from cullavo_amd.trainer import CuLLaVO_Trainer
    opt = {"MODEL": {"CONFIG": "llava-1.5-7b"}, "LLM": {"TRAINABLE": a.trainable},
           "DATA": {"BATCH_SIZE_PER_GPU": a.batch, "TEXT_LEN": 513, "IMAGE_COL": 35, "STEPS": 4},
           "BUCKET_MB": 256, "OPTIMIZER": {"OVERLAP": True}}
    tr = CuLLaVO_Trainer(opt)
    tr.init_train()
    cm = tr.model.cullavo_model
    cfg = cm.config
    has_switch = hasattr(cm, "packed_rows")
    uniform = next(iter(tr.train_dataloaders))
    P, S = cfg.vision_config.num_patches, 513
    lens = [64 + round(i * (S - 64) / (a.batch - 1)) for i in range(a.batch)]
    rag = ragged(uniform, cfg, lens)
    L = S + P - 1
    share = sum(n + P - 1 for n in lens) / (a.batch * L)

    def step(batch, packed):
        if has_switch:
            cm.packed_rows = packed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with tr.accel.accumulate(tr.model):
            info, _, _ = tr.train_step(batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(info["loss_llm"])

    def measure(name, batch, extra):
        modes = [False, True] if has_switch else [False]
        ms = {m: [] for m in modes}
        loss = {}
        for i in range(a.warmup + a.steps):
            for m in modes:  # interleaved
                t, loss[m] = step(batch, m)
                if i >= a.warmup:
                    ms[m].append(t)
        rec = dict(batch=name, trainable=a.trainable, B=a.batch, L=L, steps=a.steps, warmup=a.warmup,
                   has_packed_switch=has_switch, off_ms=sorted(ms[False])[len(ms[False]) // 2], off_all_ms=ms[False],
                   off_loss=loss[False], **extra)
        if has_switch:
            rec.update(on_ms=sorted(ms[True])[len(ms[True]) // 2], on_all_ms=ms[True], on_loss=loss[True])
            rec["on_over_off"] = rec["on_ms"] / rec["off_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    measure("ragged", rag, dict(text_lens=lens, image_rows=P, attended_row_share=share,
                                note="synthetic spread 64..513; real lbkllava padding share unmeasured"))
    measure("uniform", uniform, dict(text_lens=[S] * a.batch, image_rows=P, attended_row_share=1.0))


if __name__ == "__main__":
    main()
