"""generate(decode_graph=False) on the 7B config: the host-bound eager decode loop, host and device
sampling, and the compact (ragged) eager loop. usage: eager_bench.py TREE_ROOT [--new 48] [--rounds 3]"""
import json
import sys
import time

root = sys.argv[1]
sys.path.insert(0, root)
import torch  # noqa: E402

new = int(sys.argv[sys.argv.index("--new") + 1]) if "--new" in sys.argv else 48
rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3

from cullavo_amd.arch_cullavo import CuLLaVOModel  # noqa: E402
from cullavo_amd.config import llava_1_5_7b  # noqa: E402
from cullavo_amd.data import synthetic_batch  # noqa: E402

cfg = llava_1_5_7b()
m = CuLLaVOModel(cfg, device="cuda", trainable="none", init="random", seed=0)
m.eval()
sb = synthetic_batch(cfg, 1, 513, 35, seed=1234, device="cuda")
inp = dict(input_ids=sb["input_ids"], pixel_values=sb["pixel_values"], attention_mask=sb["attention_mask"])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


paths = {
    "host_eager": lambda n: m.generate(**inp, max_new_tokens=n, decode_graph=False),
    "device_eager": lambda n: m.generate(**inp, max_new_tokens=n, decode_graph=False, device_loop=True),
    "host_eager_compact": lambda n: m.generate(**inp, max_new_tokens=n, decode_graph=False, compact_cache=True),
}
base = {}
for k, fn in paths.items():
    fn(4)
    base[k] = min(timed(lambda: fn(1)) for _ in range(2))
res = {k: [] for k in paths}
for _ in range(rounds):
    for k, fn in paths.items():
        res[k].append((timed(lambda: fn(new)) - base[k]) / (new - 1))
for k, v in res.items():
    print(json.dumps({"metric": "7B eager generate ms/token", "path": k, "new_tokens": new,
                      "ms_per_token": [round(x, 4) for x in v], "median": round(sorted(v)[len(v) // 2], 4)}), flush=True)
