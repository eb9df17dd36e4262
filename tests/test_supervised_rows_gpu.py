"""The supervised-row tail of the training step: the gathered RMSNorm forward, the scattered RMSNorm
backward, and one training step of the tiny model on the compact path against the full path.

Kernel gates: the gather / scatter forms run the same kernels as cullavo_rmsnorm_fwd / _bwd, so
their values are bitwise those of the existing entry points on the gathered inputs; the rows the
scatter does not write are exactly zero (or the given full-height residual gradient). dw: its bound is
the existing kernel's own error against a float64 sum at the shape; it is also bitwise the existing
kernel's dw on full-height inputs with dy = 0 in the other rows, as are the weight gradients of a step.
Model gates: loss relative 1e-6 (f32 reduction order), every gradient arena within the bf16 gradient
tolerance of tests/test_model_gpu.py (rel-L2 2e-2).
"""
import pytest
import torch

from oracle import cullavo_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
T, D = 37, 256
EPS = 1e-5
GRAD_TOL = 2e-2  # tests/test_model_gpu.py check_grads


def ops():
    from cullavo_amd import ops as _ops
    return _ops


def rnd(shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def row_sets():
    """sorted index sets of |rows| in {0, 1, 9, 37}; row 0 and row T-1 are in every set that has room"""
    g = torch.Generator().manual_seed(5)
    mid = (torch.randperm(T - 2, generator=g)[:7] + 1).sort().values.tolist()
    return {"n0": [], "n1_first": [0], "n1_last": [T - 1], "n9": [0] + mid + [T - 1], "n37": list(range(T))}


ROWS = row_sets()


def idx(name, pad=0):
    return torch.tensor(ROWS[name] + [-1] * pad, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("name", list(ROWS))
def test_gathered_rmsnorm_fwd_is_bitwise(name):
    h, w = rnd((T, D), 1), rnd((D,), 2, 0.5) + 1
    rows = idx(name)
    y, rstd, hg = ops().rmsnorm_fwd_rows(h, rows, w, EPS, want_rows=True)
    y_ref, rstd_ref = ops().rmsnorm_fwd(h[rows].contiguous(), w, EPS)
    assert y.shape == (len(ROWS[name]), D)
    assert torch.equal(y, y_ref) and torch.equal(rstd, rstd_ref)
    assert torch.equal(hg, h[rows])
    y2, rstd2 = ops().rmsnorm_fwd_rows(h, rows, w, EPS)
    assert torch.equal(y2, y_ref) and torch.equal(rstd2, rstd_ref)


def test_gathered_rmsnorm_fwd_padding_rows_are_zero():
    h, w = rnd((T, D), 1), rnd((D,), 2, 0.5) + 1
    rows = idx("n9", pad=7)
    y, rstd, hg = ops().rmsnorm_fwd_rows(h, rows, w, EPS, want_rows=True)
    y_ref, rstd_ref = ops().rmsnorm_fwd(h[rows[:9]].contiguous(), w, EPS)
    assert torch.equal(y[:9], y_ref) and torch.equal(rstd[:9], rstd_ref) and torch.equal(hg[:9], h[rows[:9]])
    assert y[9:].float().abs().max().item() == 0.0 and hg[9:].float().abs().max().item() == 0.0
    assert rstd[9:].abs().max().item() == 0.0


def _dw_f64(dy, x, rstd):
    """float64 sum over rows of dy * bf16(x * rstd) (the kernels' x_hat rounding point)"""
    xh = (x.float() * rstd[:, None]).to(BF).double()
    return (dy.double() * xh).sum(0)


@pytest.mark.parametrize("with_dres_full", [False, True], ids=["zero_fill", "dres_full"])
@pytest.mark.parametrize("with_dw", [True, False], ids=["dw", "no_dw"])
@pytest.mark.parametrize("name", list(ROWS))
def test_scattered_rmsnorm_bwd(name, with_dw, with_dres_full):
    n = len(ROWS[name])
    rows = idx(name)
    h, w = rnd((T, D), 1), rnd((D,), 2, 0.5) + 1
    hc = h[rows].contiguous()
    _, rstd = ops().rmsnorm_fwd(hc, w, EPS)
    dy, dres = rnd((n, D), 3), rnd((n, D), 4)
    dres_full = rnd((T, D), 6) if with_dres_full else None
    dw_new = torch.full((D,), 7.0, dtype=torch.float32, device=DEV) if with_dw else None
    dw_old = torch.zeros(D, dtype=torch.float32, device=DEV) if with_dw else None
    dx_full = ops().rmsnorm_bwd_rows(dy, hc, w, rstd, rows, T, dres=dres, dres_full=dres_full, dw=dw_new)
    dx_ref = ops().rmsnorm_bwd(dy, hc, w, rstd, dres=dres, dw=dw_old)
    assert dx_full.shape == (T, D)
    assert torch.equal(dx_full[rows], dx_ref)
    other = torch.ones(T, dtype=torch.bool, device=DEV)
    other[rows] = False
    if with_dres_full:
        assert torch.equal(dx_full[other], dres_full[other])
    else:
        assert dx_full[other].float().abs().sum().item() == 0.0
    if with_dw:
        # the existing kernel's own error against float64 at this shape is the bound (n = 0: it
        # writes nothing, the new entry point owes beta * dw = 0)
        ref = _dw_f64(dy, hc, rstd)
        bound = (dw_old.double() - ref).abs().max().item()
        err = (dw_new.double() - ref).abs().max().item()
        print(f"{name}: dw max|err| vs f64: existing {bound:.3e}, scattered {err:.3e}")
        assert err <= bound


def test_scattered_rmsnorm_bwd_skips_padding_rows():
    """a row set padded with -1 (the compact buffers' K % 8 padding): padding rows write nothing and
    add nothing to dw, whatever their dy holds"""
    n, pad = 9, 7
    rows = idx("n9", pad=pad)
    h, w = rnd((T, D), 1), rnd((D,), 2, 0.5) + 1
    y, rstd, hc = ops().rmsnorm_fwd_rows(h, rows, w, EPS, want_rows=True)
    dy, dres = rnd((n + pad, D), 3), rnd((n + pad, D), 4)
    dw_new = torch.zeros(D, dtype=torch.float32, device=DEV)
    dw_old = torch.zeros(D, dtype=torch.float32, device=DEV)
    dx_full = ops().rmsnorm_bwd_rows(dy, hc, w, rstd, rows, T, dres=dres, dw=dw_new)
    dx_ref = ops().rmsnorm_bwd(dy[:n].contiguous(), hc[:n].contiguous(), w, rstd[:n].contiguous(),
                               dres=dres[:n].contiguous(), dw=dw_old)
    assert torch.equal(dx_full[rows[:n]], dx_ref)
    other = torch.ones(T, dtype=torch.bool, device=DEV)
    other[rows[:n]] = False
    assert dx_full[other].float().abs().sum().item() == 0.0
    # the 9 rows land in other workgroup slots than in the 9-row launch, so dw may differ by the f32
    # summation order of 9 terms per column: (n - 1) * 2^-24 * sum |term| bounds either order
    terms = (dy[:n].double() * (hc[:n].float() * rstd[:n, None]).to(BF).double()).abs().sum(0)
    ref = _dw_f64(dy[:n], hc[:n], rstd[:n])
    tol = ((n - 1) * 2.0 ** -24 * terms).max().item()
    assert (dw_new.double() - ref).abs().max().item() <= tol
    assert (dw_old.double() - ref).abs().max().item() <= tol


@pytest.mark.parametrize("compact_out", [False, True], ids=["scatter", "compact_out"])
@pytest.mark.parametrize("name", ["n0", "n1_last", "n9", "n37"])
def test_rows_rmsnorm_bwd_dw_is_bitwise_the_full_height_kernels(name, compact_out):
    """the rows form walks the full-height rows in the existing kernel's order, so its dw is bitwise the
    existing kernel's on full-height inputs whose other rows have dy = 0 (what the full path computes)"""
    n, pad = len(ROWS[name]), 3
    rows = idx(name, pad=pad)
    h, w = rnd((T, D), 1), rnd((D,), 2, 0.5) + 1
    _, rstd_full = ops().rmsnorm_fwd(h, w, EPS)
    y, rstd, hc = ops().rmsnorm_fwd_rows(h, rows, w, EPS, want_rows=True)
    dy = rnd((n + pad, D), 3)
    dy_full = ops().rows_scatter(dy, rows, T)
    dw_new = torch.full((D,), 7.0, dtype=torch.float32, device=DEV)
    dw_old = torch.full((D,), 7.0, dtype=torch.float32, device=DEV)
    dx = ops().rmsnorm_bwd_rows(dy, hc, w, rstd, rows, T, dw=dw_new, beta=1.0, compact_out=compact_out)
    dx_ref = ops().rmsnorm_bwd(dy_full, h, w, rstd_full, dw=dw_old, beta=1.0)
    assert torch.equal(dw_new, dw_old)
    if compact_out:
        assert dx.shape == (n + pad, D)
        assert torch.equal(dx[:n], dx_ref[rows[:n]]) and dx[n:].float().abs().sum().item() == 0.0
    else:
        assert torch.equal(dx.float(), dx_ref.float())  # -0.0 == 0.0 in the rows without a label


def test_rows_scatter():
    """compact rows land in their full-height rows, every other row is an exact zero; more columns than
    one pass of a wave covers, and an empty row set"""
    rows = idx("n9", pad=7)
    src = rnd((16, 1032), 8)
    dst = ops().rows_scatter(src, rows, T)
    ref = torch.zeros((T, 1032), dtype=BF, device=DEV)
    ref[rows[:9]] = src[:9]
    assert torch.equal(dst, ref)
    empty = ops().rows_scatter(src[:0].contiguous(), idx("n0"), T)
    assert empty.shape == (T, 1032) and empty.float().abs().sum().item() == 0.0


def test_supervised_rows_index():
    tg = torch.full((T,), -100, dtype=torch.int64, device=DEV)
    tg[torch.tensor(ROWS["n9"], device=DEV)] = 5
    rows = ops().supervised_rows(tg, 16)
    assert rows.tolist() == ROWS["n9"] + [-1] * 7
    assert ops().gather_targets(tg, rows).tolist() == [5] * 9 + [-100] * 7
    assert ops().supervised_rows(torch.full_like(tg, -100), 8).tolist() == [-1] * 8


# ---- tiny model: one training step, compact path against full path --------------------------------
def build(seed=2):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    m = CuLLaVOModel(tiny_gpu(), device=DEV, trainable="full", init="none")
    m.load_state_dict(O.make_weights(O.config_small_gpu(), seed))
    m.train()
    return m


def batch(n_labels):
    """text 40 tokens (L = 295 merged); sample b carries labels on its last n_labels[b] positions"""
    ids, mask, pix, labels = O.make_inputs(O.config_small_gpu(), 2, 40, 4, 2)
    L = labels.shape[1]
    g = torch.Generator().manual_seed(11)
    labels[:] = -100
    for b, n in enumerate(n_labels):
        if n:
            labels[b, L - n:] = torch.randint(2, 1000, (n,), generator=g)
    return {"input_ids": ids.to(DEV), "attention_mask": mask.to(DEV), "pixel_values": pix.to(DEV),
            "labels": labels.to(DEV)}


def step(compact, n_labels):
    """one forward + backward; (loss, {arena: grad_flat}, gradient of the last layer's input)"""
    m = build()
    m.supervised_rows = compact
    last = m.language_model.model.layers[-1]
    seen, run = [], last.run

    def run_hooked(h, sctx):
        h.register_hook(seen.append)
        return run(h, sctx)

    last.run = run_hooked
    out = m(**batch(n_labels), num_supervised=sum(n_labels) if compact else None)
    assert (out.logits is None) == compact
    out.loss.backward()
    for ar in m.arenas.values():
        ar.finalize_grads()
    torch.cuda.synchronize()
    grads = {name: ar.grad_flat.float().clone() for name, ar in m.arenas.items() if ar.trainable}
    return out.loss.item(), grads, seen[0]


@pytest.fixture(scope="module")
def full_step():
    return step(False, (13, 1))


def test_tiny_model_step_matches_full_path(full_step):
    loss_f, grads_f, _ = full_step
    loss_c, grads_c, dh_c = step(True, (13, 1))
    print(f"loss full {loss_f:.8f} compact {loss_c:.8f}")
    assert abs(loss_c - loss_f) <= 1e-6 * abs(loss_f)
    assert grads_c.keys() == grads_f.keys()
    for name in grads_f:
        ref = grads_f[name]
        err = ((grads_c[name] - ref).norm() / (ref.norm() + 1e-12)).item()
        print(f"arena {name}: grad rel-L2 compact vs full {err:.3e}")
        assert ref.norm().item() > 0 and err <= GRAD_TOL, (name, err)
    assert dh_c.shape == (2 * 295, 256) and torch.isfinite(dh_c).all()
    # the weight gradients keep the full path's summation order, so what is left is the forward and dX
    # GEMMs' plan at M = 16 against M = 590 (none at the 7B shapes, where the step is bitwise the same)
    assert torch.equal(grads_c["head"], grads_f["head"])


def test_batch_without_supervised_rows():
    """no label at all: the compact path runs its 8 padding rows; loss and head gradients are the full
    path's (the same ce_reduce on an empty set; zero gradients)"""
    loss_f, grads_f, _ = step(False, (0, 0))
    loss_c, grads_c, dh_c = step(True, (0, 0))
    # the mean over an empty selection is NaN on both paths (nn.CrossEntropyLoss); ce_bwd scales the
    # rows without a label by zero, so every gradient from the head is an exact zero on both
    assert loss_f != loss_f and loss_c != loss_c
    for name in grads_f:
        assert torch.equal(grads_c[name], grads_f[name]), name
    assert grads_f["head"].abs().sum().item() == 0.0 and grads_f["layers"].abs().sum().item() == 0.0
    assert torch.isfinite(dh_c).all()
