"""packed.packed_plan / mask_counts / check_no_holes on the CPU: the packed step's gather index, seq_start,
seq_len and T from masks of both padding sides against a plain Python loop, and the hole detection."""
import pytest
import torch

from cullavo_amd.packed import check_no_holes, mask_counts, packed_plan


def loop_plan(mask):
    rows, start, lens = [], [], []
    B, L = len(mask), len(mask[0])
    for b in range(B):
        start.append(len(rows))
        n = 0
        for t in range(L):
            if mask[b][t]:
                rows.append(b * L + t)
                n += 1
        lens.append(n)
    return rows, start, lens


def right(L, lens):
    return [[1] * n + [0] * (L - n) for n in lens]


def left(L, lens):
    return [[0] * (L - n) + [1] * n for n in lens]


MASKS = {"right": right(11, (11, 3, 7)), "left": left(11, (4, 11, 9)), "mixed": right(9, (9, 2)) + left(9, (5,)),
         "empty_row": right(8, (8, 0, 5)), "multiple_of_8": left(8, (8, 5, 3))}


@pytest.mark.parametrize("name", list(MASKS))
def test_plan_matches_python_loop(name):
    mask = MASKS[name]
    rows, start, lens = loop_plan(mask)
    p = packed_plan(torch.tensor(mask), lens)
    T = len(rows)
    assert p.T == T and p.Tp % 8 == 0 and T <= p.Tp < T + 8 and p.Tp >= 8 and p.max_len == max(lens)
    assert p.rows.dtype == torch.int64 and p.rows.tolist() == rows + [-1] * (p.Tp - T)
    assert p.seq_start.dtype == torch.int32 and p.seq_start.tolist() == start
    assert p.seq_len.dtype == torch.int32 and p.seq_len.tolist() == lens


def test_host_counts_that_disagree_with_the_mask_stay_inside_the_buffers():
    mask = torch.tensor(right(10, (10, 4, 6)))
    rows, start, lens = loop_plan(mask.tolist())
    over = packed_plan(mask, [10, 9, 6])      # an upper bound: extra slots are zero rows
    assert over.rows[:20].tolist() == rows and set(over.rows[20:].tolist()) == {-1} and over.seq_len.tolist() == lens
    under = packed_plan(mask, [10, 4, 2])     # too small: the tail is dropped, nothing points past T
    assert under.T == 16 and under.rows.tolist() == rows[:16]
    assert all(s + n <= under.T for s, n in zip(under.seq_start.tolist(), under.seq_len.tolist()))
    with pytest.raises(ValueError):
        packed_plan(mask, [10, 4])
    with pytest.raises(ValueError):
        packed_plan(mask, [11, 4, 6])


def test_hole_detection():
    for name, mask in MASKS.items():
        c, s = mask_counts(torch.tensor(mask)).tolist()
        assert c == loop_plan(mask)[2], name
        check_no_holes(c, s)
    holes = [[1, 1, 0, 1, 0], [0, 1, 1, 1, 1], [1, 0, 0, 0, 1]]
    c, s = mask_counts(torch.tensor(holes)).tolist()
    assert c == [3, 4, 2] and s == [4, 4, 5]
    with pytest.raises(ValueError, match=r"row\(s\) \[0, 2\]"):
        check_no_holes(c, s)
