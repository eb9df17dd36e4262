"""The packed training step's row plan: which rows of the padded [B, L] grid are attended, where each
sequence's rows sit once only those are kept, and the checks on the mask that go with it.

Packed order is sequence by sequence, positions ascending. Sizes (T, max_len) come from HOST-side
per-sequence counts, so building a plan never asks the device for anything; the index tensors are
computed on the mask's device from the mask itself. Everything here also runs on CPU tensors
(tests/test_packed_plan_host.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class PackedPlan:
    rows: torch.Tensor       # int64 [Tp]: flat index b * L + t of packed row i, ascending; -1 on the padding rows
    seq_start: torch.Tensor  # int32 [B]: first packed row of sequence b
    seq_len: torch.Tensor    # int32 [B]: its attended rows
    T: int                   # attended rows (host)
    Tp: int                  # T rounded up to a multiple of 8 (the weight-gradient GEMMs' K % 8); the rest are zero rows
    max_len: int             # host upper bound of seq_len


def mask_counts(mask):
    """[2, B] int64 on the mask's device: per row the number of attended positions and the length of the
    span from its first to its last attended position (0 for an empty row). Equal iff the row has no hole."""
    m = mask != 0
    L = m.shape[1]
    count = m.sum(-1)
    first = (m.cumsum(-1) == 0).sum(-1)
    tail = (m.flip(-1).cumsum(-1) == 0).sum(-1)
    span = (L - first - tail).clamp_min(0)
    return torch.stack([count, span])


def check_no_holes(counts, spans):
    """raise on a mask with a hole (a zero after a row's first attended token and before its last): host
    values of mask_counts"""
    bad = [b for b, (c, s) in enumerate(zip(counts, spans)) if int(c) != int(s)]
    if bad:
        raise ValueError(f"packed_rows: the attention mask of row(s) {bad} has a hole (a zero between two attended "
                         f"positions); only left or right padding can be packed")


def packed_plan(mask, lens) -> PackedPlan:
    """mask [B, L] (0 / 1), lens: the host-side attended count of every row (an upper bound is safe: extra
    slots become zero rows; a count below the truth drops that row's tail). No synchronisation."""
    B, L = mask.shape
    lens = [int(n) for n in lens]
    if len(lens) != B or any(n < 0 or n > L for n in lens):
        raise ValueError(f"packed_plan: {len(lens)} counts {lens} for a [{B}, {L}] mask")
    T = sum(lens)
    Tp = max(8, -(-T // 8) * 8)
    dev = mask.device
    m = (mask != 0).reshape(-1)
    dest = torch.cumsum(m, 0) - 1
    rows = torch.full((Tp + 1,), -1, dtype=torch.int64, device=dev)  # slot Tp: the sink of everything not kept
    rows.scatter_(0, torch.where(m & (dest < T), dest, Tp), torch.arange(B * L, device=dev))
    rows[Tp] = -1
    seq_len = (mask != 0).sum(-1)
    seq_start = torch.cumsum(seq_len, 0) - seq_len
    # the device's own counts, held inside the T rows the host sized (a wrong host count must not send the
    # attention kernels past the buffers)
    seq_len = torch.minimum(seq_len, (T - seq_start).clamp_min(0))
    return PackedPlan(rows[:Tp].contiguous(), seq_start.to(torch.int32).contiguous(), seq_len.to(torch.int32).contiguous(),
                      T, Tp, max(lens) if lens else 0)
