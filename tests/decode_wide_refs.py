"""Cases and the honest f32 restatement of the wide decode product (csrc/gemv_wide.hip,
cullavo_decode_linear_wide: Y[M, N] = X[M, K] W[N, K]^T at 17 <= M <= 64). The float64 reference, the
gate and the inputs are tests/decode_refs.py's (gemv_inputs, gemv_ref, gemv_gate, epilogue_replay):
the gate K 2^-24 |X||W|^T per element holds for any f32 summation order, so it is the same bound at
these row counts. tests/test_decode_wide_host.py proves on the CPU that the restatement passes it and
one-line mutants fail; tests/test_decode_wide_gpu.py holds the kernel to it on the same inputs.
No number here was taken from a kernel's output.
"""
import torch

from tests import decode_refs as R

BF = torch.bfloat16
WAVES = 8  # gemv_wide_k: 8 contiguous K ranges for every (N, K)

WIDE_MS = [17, 31, 32, 33, 48, 64]
# an N tail (8, 24, 40: less than one 16-row block's multiple), a K tail that is no multiple of the
# 32-deep k-step (72, 1000, 8200, 136), fewer k-steps than waves (64, 72, 136), long K, wide N
WIDE_NKS = [(8, 64), (24, 72), (776, 1000), (264, 4096), (40, 8200), (16392, 136)]
WIDE_CASES = [(m, n, k) for m in WIDE_MS for (n, k) in WIDE_NKS]
# (M, N, K) of transform 3 (w holds 2N rows)
WIDE_SWIGLU_CASES = [(17, 8, 72), (64, 8200, 136)]


def wide_inputs(M, N, K):
    return R.gemv_inputs(M, N, K, name="wide")


def wide_honest(X, W, drop_tail8=False, drop_step=None, double_step=None, row_last_as_0=False,
                rows16_as_0=False, clamp_n_tail=False):
    """gemv_wide_k restated in torch f32: the 32-deep k-steps dealt to 8 waves as contiguous ranges of
    cdiv(cdiv(K, 32), 8) steps, each range summed in f32 from zero, the eight partials then added in
    wave order. The split depends on K alone: not on M, nor on how many 16-row weight or X blocks a
    workgroup holds. The keyword arguments are the mutants of test_decode_wide_host.py."""
    Xf, Wf = X.float(), W.float()
    M, K = Xf.shape
    N = Wf.shape[0]
    if row_last_as_0:  # row M-1 of X read as row 0
        Xf = Xf.clone()
        Xf[M - 1] = Xf[0]
    if rows16_as_0:  # the second 16-row X block read as the first
        Xf = Xf.clone()
        hi = min(32, M)
        Xf[16:hi] = Xf[0:hi - 16]
    if clamp_n_tail:  # the last 8 weight rows clamped to row N-9
        Wf = Wf.clone()
        Wf[N - 8:] = Wf[N - 9]
    keep = torch.ones(K)
    if drop_tail8:
        keep[K - 8:] = 0
    if drop_step is not None:
        keep[32 * drop_step:32 * drop_step + 32] = 0
    if double_step is not None:
        keep[32 * double_step:32 * double_step + 32] = 2
    Xf = Xf * keep  # exact in f32 (x0, x1, x2)
    nk = -(-K // 32)
    per = -(-nk // WAVES) * 32
    acc = None
    for w in range(WAVES):
        lo, hi = w * per, min(K, (w + 1) * per)
        part = Xf[:, lo:hi] @ Wf[:, lo:hi].T if lo < hi else torch.zeros(M, N)
        acc = part if acc is None else acc + part
    return acc


def wide_swiglu_honest(X, W2):
    """transform 3 on the honest f32 products: W2 [2N, K] = gate rows | up rows; g and u rounded to
    bf16 as the plain product stores them, then bf16(bf16(silu(g)) * u)"""
    N = W2.shape[0] // 2
    z = wide_honest(X, W2)
    g, up = R.bf(z[:, :N]), R.bf(z[:, N:])
    return R.bf(R.bf(g / (1.0 + torch.exp(-g))) * up).to(BF)
