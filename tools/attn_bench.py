"""Flash attention forward / backward at the production shapes (HIP-event timing):
LM causal D=128 (B=8, L=1088, H=32) and CLIP non-causal D=64 (B=64, T=577, H=16).
Algorithmic FLOPs: fwd 4*B*H*Lq*Lk*D (x1/2 causal), bwd 2.5x fwd."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cullavo_amd import _lib, ops  # noqa: E402


def timeit(fn, iters=10):
    for _ in range(2):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def cached_cases():
    """--cached: ops.attn_fwd_cached (Lq new queries on a 1088-row cache prefix, the config-3 prompt)
    next to ops.attn_fwd causal at Lq = Lk = past + Lq, which computes a superset of the same
    products; the two alternate (three rounds), and the cached rows are compared with the full
    pass's last Lq rows. Algorithmic FLOPs of the cached call: 4 B H D (Lq past + Lq (Lq + 1) / 2)."""
    H, D, past = 32, 128, 1088
    for B in (1, 8):
        for Lq in (16, 64, 512):
            L = past + Lq
            torch.manual_seed(0)
            qkv = (torch.randn(B * L, 3 * H * D, device="cuda") * 0.5).bfloat16()
            q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
            kc = k.reshape(B, L, H * D).contiguous()
            vc = v.reshape(B, L, H * D).contiguous()
            qn = q.reshape(B, L, H * D)[:, past:].reshape(B * Lq, H * D).contiguous()
            kw = dict(B=B, H=H, D=D, scale=D ** -0.5)
            full = lambda: ops.attn_fwd(q, k, v, Lq=L, Lk=L, causal=True, **kw)
            cached = lambda: ops.attn_fwd_cached(qn, kc, vc, Lq=Lq, past=past, **kw)
            o_full = full()[0].reshape(B, L, H * D)[:, past:].reshape(B * Lq, H * D).float()
            o_c = cached()[0].float()
            rel = ((o_c - o_full).norm() / o_full.norm()).item()
            tc, tf = [], []
            for _ in range(3):
                tc.append(timeit(cached, iters=200))
                tf.append(timeit(full, iters=50))
            fl = 4.0 * B * H * D * (Lq * past + Lq * (Lq + 1) / 2)
            print(f"cached B {B} H {H} D {D} past {past} Lq {Lq:4d}: attn_fwd_cached "
                  + " ".join(f"{t * 1e3:7.1f}" for t in tc) + f" us ({fl / min(tc) / 1e9:6.1f} TF) | attn_fwd causal L {L} "
                  + " ".join(f"{t * 1e3:7.1f}" for t in tf) + f" us | rel diff of the shared rows {rel:.1e}", flush=True)


if "--cached" in sys.argv:
    cached_cases()
    sys.exit(0)

STAGES = [int(x) for x in os.environ.get("ATTN_STAGE_AB", "7").split(",")]  # forward kernels, e.g. 4,7,4,7
ref_out = {}
for stage in STAGES:
  if len(STAGES) > 1:
    _lib.lib().cullavo_attn_set_stage(stage)
  for name, B, L, H, D, causal in [("LM causal D128", 8, 1088, 32, 128, True), ("ViT D64", 64, 577, 16, 64, False)]:
    torch.manual_seed(0)
    qkv = (torch.randn(B * L, 3 * H * D, device="cuda") * 0.5).bfloat16()
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    o, lse = ops.attn_fwd(q, k, v, B=B, H=H, Lq=L, Lk=L, D=D, scale=D ** -0.5, causal=causal)
    do = torch.randn_like(o)
    dqkv = torch.empty_like(qkv)
    fl = 4.0 * B * H * L * L * D * (0.5 if causal else 1.0)
    tf = timeit(lambda: ops.attn_fwd(q, k, v, B=B, H=H, Lq=L, Lk=L, D=D, scale=D ** -0.5, causal=causal))
    res = []
    outs = {}
    for mode in (4, 7, 0, 2):  # 4 = 8-wave dK/dV + 4-wave dQ, 7 = 8-wave dK/dV storing dS + dQ from it, 0 / 2 = 4-wave
        _lib.lib().cullavo_attn_set_bwd_tiles(mode)
        tb = timeit(lambda: ops.attn_bwd(q, k, v, o, do, lse, B=B, H=H, Lq=L, Lk=L, D=D, scale=D ** -0.5,
                                         causal=causal, dq=dqkv[:, :H * D], dk=dqkv[:, H * D:2 * H * D],
                                         dv=dqkv[:, 2 * H * D:]))
        outs[mode] = dqkv.float().clone()
        res.append(f"m{mode} {tb * 1e3:7.1f} us {2.5 * fl / tb / 1e9:6.1f} TF")
    diff = ((outs[4] - outs[0]).norm() / outs[0].norm()).item()
    res.append(f"rel(m4, m0) {diff:.1e} rel(m7, m0) {((outs[7] - outs[0]).norm() / outs[0].norm()).item():.1e}")
    key = name
    cur = (o.float().clone(), outs[7])
    if key in ref_out:
        res.append(f"bitwise equal across forward kernels: {torch.equal(ref_out[key][0], cur[0]) and torch.equal(ref_out[key][1], cur[1])}")
    else:
        ref_out[key] = cur
    _lib.lib().cullavo_attn_set_bwd_tiles(-1)
    tag = f"stage {stage} " if len(STAGES) > 1 else ""
    print(f"{tag}{name:16s} fwd {tf * 1e3:8.1f} us {fl / tf / 1e9:7.1f} TF | bwd " + " | ".join(res), flush=True)
