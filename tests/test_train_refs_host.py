"""The gates of tests/train_refs.py discriminate, shown on the CPU before any GPU time is spent.

For every input set of tests/test_train_accuracy_gpu.py (same seeds, same shapes) an honest
restatement of the kernel (torch f32, summed in the kernel's lane / wave-part / workgroup order,
rounded where the kernel rounds) stays at or below 1.0 of its gate; the worst err / gate of every
family is printed (pytest -s). Each one-line mutant of a restatement exceeds 2.0 on at least one
input set; the sets on which a mutant computes the same thing as the honest form (the padded width
at 4096 columns, wave part 3 of a 520-column row, the next row's rstd of a single row) are named
where they are left out, nothing is skipped silently.
"""
import pytest
import torch

from tests import train_refs as T

BF, F32 = T.BF, T.F32


def _record(worsts, name, value):
    worsts[name] = max(worsts.get(name, 0.0), value)


def _assert_mutants(honest, mutants, label):
    for k, v in sorted(honest.items()):
        print(f"{label} honest {k}: worst err/gate {v:.3f}")
    for k, v in sorted(mutants.items()):
        print(f"{label} mutant {k}: worst err/gate over the sets it applies to {v:.3g}")
    for k, v in honest.items():
        assert v <= 1.0, f"{label}: the honest restatement breaks the {k} gate ({v:.3f})"
    for k, v in mutants.items():
        assert v > 2.0, f"{label}: mutant {k} passes the gate on every input set ({v:.3f})"


# ---------------------------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------------------------
def test_rms_plan_serves_each_case_its_purpose():
    """the geometry the cases were chosen for, from the restated dispatch of rmsnorm_*_impl"""
    assert [T.nch_for(c) for c in (8, 520, 2056, 4096, 5120, 8192)] == [1, 2, 8, 8, 12, 16]
    assert T.rms_fwd_prew(64, 2056, BF) and not T.rms_fwd_prew(65, 2056, BF)
    assert not T.rms_fwd_prew(3, 5120, BF) and not T.rms_fwd_prew(5, 520, F32)
    assert T.rms_bwd_plan(2100, 520, 1, True) == ("rmsnorm_bwd8p_k", 4, 256, 9, 2)   # 5 iterations, 233 * 9 + 3 rows
    assert T.rms_bwd_plan(2100, 520, 1, False)[0] == "rmsnorm_bwd8_k"                # without dw up to 4096 columns
    assert T.rms_bwd_plan(9, 5120, 1, False)[0] == "rmsnorm_bwd8p_k"
    assert T.rms_bwd_plan(37, 4096, 1, True) == ("rmsnorm_bwd8p_k", 4, 10, 4, 2)
    assert T.rms_bwd_plan(9, 5120, 0, True)[0] == T.rms_bwd_plan(7, 8192, 0, True)[0] == "rmsnorm_bwd_k"
    assert T.rms_bwd_plan(37, 4096, 0, True)[0] == "rmsnorm_bwd8_k"


def test_rms_fwd_gate_passes_honest_and_fails_mutants():
    honest, mutants = {}, {}
    for rows, cols, dt in T.RMS_FWD_CASES:
        d = T.norm_inputs(rows, cols, dt)
        x, w = d["x"], d["w"]
        y, r = T.rms_fwd_honest(x, w)
        wr, wy = T.rms_fwd_gate(y, r, x, w)
        _record(honest, "rstd", wr)
        _record(honest, "y", wy)
        for name in ("drop_last_chunk", "padded_div", "no_eps", "w_off8"):
            if name == "padded_div" and 512 * T.nch_for(cols) == cols:
                continue  # 4096 and 8192 columns: the padded width is the width
            ym, rm = T.rms_fwd_honest(x, w, **{name: True})
            _record(mutants, name, max(T.rms_fwd_gate(ym, rm, x, w)))
    _assert_mutants(honest, mutants, "rmsnorm_fwd")


def _rms_bwd_sets(kind):
    """(label, inputs, mode, want_dw, dw_dtype, beta): the GPU test's cases of one kind of data"""
    for rows, cols in T.RMS_BWD_CASES:
        for want in (False, True):
            yield f"{rows}x{cols}-{kind}-m1-dw{int(want)}", T.norm_inputs(rows, cols, BF, kind), 1, want, F32, 0.0
    for rows, cols, want in T.RMS_BWD_MODE0_CASES:
        yield f"{rows}x{cols}-{kind}-m0", T.norm_inputs(rows, cols, BF, kind), 0, want, F32, 0.0
    rows, cols = T.RMS_BWD_F32_CASE
    yield f"{rows}x{cols}-{kind}-f32", T.norm_inputs(rows, cols, F32, kind), 1, True, F32, 0.0
    rows, cols = T.RMS_BWD_BETA_CASE
    yield f"{rows}x{cols}-{kind}-beta", T.norm_inputs(rows, cols, BF, kind), 1, True, BF, 1.0


@pytest.mark.parametrize("kind", T.NORM_KINDS)
def test_rms_bwd_gate_passes_honest_and_fails_mutants(kind):
    """every mutant fails on the unit-normal sets alone and on the correlated sets alone"""
    honest, mutants = {}, {}
    for label, d, mode, want, dw_dtype, beta in _rms_bwd_sets(kind):
        x, dy, w = d["x"], d["dy"], d["w"]
        rows, cols = x.shape
        rstd = T.rms_stats(x)
        kernel, parts, nb, rpb, slots = T.rms_bwd_plan(rows, cols, mode, want)
        for dres in (None, d["dres"]):
            kw = dict(dres=dres, parts=parts, rpb=rpb, slots=slots, want_dw=want, dw_dtype=dw_dtype,
                      dw_old=d["dw_old"], beta=beta)
            dx, dw = T.rms_bwd_honest(dy, x, w, rstd, **kw)
            _record(honest, f"dx {kernel}", T.rms_dx_gate(dx, dy, x, w, rstd, dres))
            if want:
                _record(honest, "dw", T.rms_dw_gate(dw, dy, x, rstd, d["dw_old"], beta))
            names = ["miss_last_chunk"]
            if parts == 4 and cols > 3 * 512:
                names.append("miss_part3")       # up to 1536 columns wave part 3 owns no chunk
            if 512 * T.nch_for(cols) != cols:
                names.append("padded_div")
            if dres is not None:
                names += ["drop_dres", "dres_twice"]
            if rows > 1:
                names.append("rstd_next_row")    # a single row has no next row
            for name in names:  # dx does not depend on the dw sums: left out of the mutants' runs
                dxm, _ = T.rms_bwd_honest(dy, x, w, rstd, **{**kw, "want_dw": False}, **{name: True})
                _record(mutants, name, T.rms_dx_gate(dxm, dy, x, w, rstd, dres))
            if want:
                _, dwm = T.rms_bwd_honest(dy, x, w, rstd, **kw, dw_miss_last_row=True)
                _record(mutants, "dw_miss_last_row", T.rms_dw_gate(dwm, dy, x, rstd, d["dw_old"], beta))
                if rows > 1:
                    _, dwm = T.rms_bwd_honest(dy, x, w, rstd, **kw, rstd_next_row=True)
                    _record(mutants, "dw rstd_next_row", T.rms_dw_gate(dwm, dy, x, rstd, d["dw_old"], beta))
    _assert_mutants(honest, mutants, f"rmsnorm_bwd {kind}")


def test_rms_chained_forward_output_passes_the_backward_gate():
    """the chained case: the restated forward's own f32 rstd, given to the backward and to its f64
    reference alike, under the same gates"""
    rows, cols = 37, 4096
    d = T.norm_inputs(rows, cols, BF, "corr")
    _, rstd = T.rms_fwd_honest(d["x"], d["w"])
    _, parts, _, rpb, slots = T.rms_bwd_plan(rows, cols, 1, True)
    dx, dw = T.rms_bwd_honest(d["dy"], d["x"], d["w"], rstd, dres=d["dres"], parts=parts, rpb=rpb, slots=slots, want_dw=True)
    assert T.rms_dx_gate(dx, d["dy"], d["x"], d["w"], rstd, d["dres"]) <= 1.0
    assert T.rms_dw_gate(dw, d["dy"], d["x"], rstd) <= 1.0


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
def _ln_sets():
    for kind in T.NORM_KINDS:
        for rows, cols in T.LN_CASES:
            yield T.norm_inputs(rows, cols, BF, kind, name="ln")
        yield T.norm_inputs(*T.LN_F32_CASE, F32, kind, name="ln")


def test_layernorm_gates_pass_honest_and_fail_mutants():
    honest, mutants = {}, {}
    for d in _ln_sets():
        x, dy, w, b = d["x"], d["dy"], d["w"], d["b"]
        y, mean_h, rstd_h = T.ln_fwd_honest(x, w, b)
        wm, wr, wy = T.ln_fwd_gate(y, mean_h, rstd_h, x, w, b)
        _record(honest, "fwd mean", wm)
        _record(honest, "fwd rstd", wr)
        _record(honest, "fwd y", wy)
        mean, rstd = T.ln_stats(x)
        for dres in (None, d["dres"]):
            dx, dw, db = T.ln_bwd_honest(dy, x, w, mean, rstd, dres)
            for k, v in zip(("dx", "dw", "db"), T.ln_bwd_gate(dx, dw, db, dy, x, w, mean, rstd, dres)):
                _record(honest, k, v)
            for name in ("no_sg", "no_sgx", "db_miss_row"):
                dxm, dwm, dbm = T.ln_bwd_honest(dy, x, w, mean, rstd, dres, **{name: True})
                g = T.ln_bwd_gate(dxm, dwm, dbm, dy, x, w, mean, rstd, dres)
                _record(mutants, name, g[2] if name == "db_miss_row" else g[0])
        # the chained case: the restated forward's mean and rstd into the backward, the same gates
        dx, dw, db = T.ln_bwd_honest(dy, x, w, mean_h, rstd_h, d["dres"])
        for k, v in zip(("dx", "dw", "db"), T.ln_bwd_gate(dx, dw, db, dy, x, w, mean_h, rstd_h, d["dres"])):
            _record(honest, k + " chained", v)
    _assert_mutants(honest, mutants, "layernorm")


# ---------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------
def test_ce_inputs_place_targets_and_keep_lse_small():
    for rows, V, dt, kind in T.CE_CASES:
        x, t = T.ce_inputs(rows, V, dt, kind)
        lse = T.ce_ref(x, t)[0]
        assert lse.abs().max() < 16
        assert x.stride(0) == -(-V // 8) * 8 and t[0] == 0 and t[1] == V - 1 and t[3] == T.IGNORE
        if V % 8 >= 2:
            assert int(t[2]) >= V // 8 * 8  # a target inside the tail
        if kind == "planted_last":
            assert bool((x.float().argmax(1) == V - 1).all())


def test_ce_gates_pass_honest_and_fail_mutants():
    honest, mutants = {}, {}
    for rows, V, dt, kind in T.CE_CASES:
        x, t = T.ce_inputs(rows, V, dt, kind)
        loss_h, lse_h = T.ce_fwd_honest(x, t)
        wl, wo, zero_ok = T.ce_fwd_gate(loss_h, lse_h, x, t)
        assert zero_ok
        _record(honest, "lse", wl)
        _record(honest, "row_loss", wo)
        if V % 8:
            _record(mutants, "skip_tail", T.ce_fwd_gate(*T.ce_fwd_honest(x, t, skip_tail=True), x, t)[0])
        if V >= 8:  # the 8-wide loop runs
            _record(mutants, "no_rescale", T.ce_fwd_gate(*T.ce_fwd_honest(x, t, no_rescale=True), x, t)[0])
        lse, loss, out = T.ce_stats(x, t)
        assert not T.ce_reduce_check(out, loss, t)
        for gl in T.CE_GRAD_LOSS:
            glt = None if gl is None else torch.tensor([gl], dtype=torch.float32)
            d = T.ce_bwd_honest(x, t, lse, out, glt)
            wd, zero_ok = T.ce_bwd_gate(d, x, t, lse, out, glt)
            assert zero_ok
            _record(honest, "dlogits", wd)
            if V % 8 >= 2:  # row 2's target lies in the tail
                _record(mutants, "no_onehot_in_tail",
                        T.ce_bwd_gate(T.ce_bwd_honest(x, t, lse, out, glt, no_onehot_in_tail=True), x, t, lse, out, glt)[0])
            if gl is not None:
                _record(mutants, "ignore_grad_loss",
                        T.ce_bwd_gate(T.ce_bwd_honest(x, t, lse, out, glt, ignore_grad_loss=True), x, t, lse, out, glt)[0])
            wk, zk = T.ce_bwd_gate(T.ce_bwd_honest(x, t, lse, out, glt, keep_ignored=True), x, t, lse, out, glt)
            _record(mutants, "keep_ignored", wk)
            assert not zk
        # the chained case: the restated forward's own lse into the backward, the same gate
        outc = T.ce_stats(x, t)[2]
        _record(honest, "dlogits chained", T.ce_bwd_gate(T.ce_bwd_honest(x, t, lse_h, outc), x, t, lse_h, outc)[0])
    _assert_mutants(honest, mutants, "cross entropy")


def test_ce_reduce_check_and_shift_targets_ref():
    t = torch.tensor([3, T.IGNORE, 1, T.IGNORE])
    loss = torch.tensor([1.5, 0.0, 2.5, 0.0])
    assert not T.ce_reduce_check(torch.tensor([2.0, 2.0, 0.5]), loss, t)
    assert T.ce_reduce_check(torch.tensor([2.0 + 2.0 ** -21, 2.0, 0.5]), loss, t)
    assert T.ce_reduce_check(torch.tensor([2.0, 3.0, 0.5]), loss, t)
    none = torch.full((4,), T.IGNORE)
    assert not T.ce_reduce_check(torch.tensor([float("nan"), 0.0, float("inf")]), loss, none)
    assert T.ce_reduce_check(torch.tensor([0.0, 0.0, float("inf")]), loss, none)
    labels = torch.tensor([[5, 6, 7], [8, 9, 10]])
    mask = torch.tensor([[1, 1, 0], [1, 0, 1]])
    assert T.shift_targets_ref(labels, mask).tolist() == [6, T.IGNORE, T.IGNORE, T.IGNORE, 10, T.IGNORE]
    assert T.shift_targets_ref(labels, None).tolist() == [6, 7, T.IGNORE, 9, 10, T.IGNORE]
    assert T.shift_targets_ref(labels[:, :1], None).tolist() == [T.IGNORE, T.IGNORE]


# ---------------------------------------------------------------------------------------------
# SwiGLU and activation backward
# ---------------------------------------------------------------------------------------------
def test_act_inputs_hold_the_edges():
    for n, dt in T.ACT_CASES:
        _, v = T.act_inputs(n, dt)
        assert v.abs().max() <= 16 and bool((v == 0).any()) and bool((v == 16).any()) and bool((v == -16).any())
        assert bool(((v.float() + 1.278).abs() < 0.01).any()) and bool(((v.float() + 0.75).abs() < 0.01).any())
    gu, d = T.swiglu_inputs(70, 688)
    g = gu[:, :688].float()
    assert int(((g > -1.40) & (g < -1.15)).sum()) >= 56 and g.abs().max() == 16


def test_swiglu_gates_pass_honest_and_fail_mutants():
    honest, mutants = {}, {}
    for rows, F, dt in T.SWIGLU_CASES:
        gu, d = T.swiglu_inputs(rows, F, dt)
        _record(honest, "fwd", T.swiglu_fwd_gate(T.swiglu_fwd_honest(gu), gu))
        wg, wu = T.swiglu_bwd_gate(T.swiglu_bwd_honest(d, gu), d, gu)
        _record(honest, "dgate", wg)
        _record(honest, "dup", wu)
        _record(mutants, "fwd swap_halves", T.swiglu_fwd_gate(T.swiglu_fwd_honest(gu, swap_halves=True), gu))
        _record(mutants, "slope_no_s", T.swiglu_bwd_gate(T.swiglu_bwd_honest(d, gu, slope_no_s=True), d, gu)[0])
        _record(mutants, "bwd swap_halves", min(T.swiglu_bwd_gate(T.swiglu_bwd_honest(d, gu, swap_halves=True), d, gu)))
    _assert_mutants(honest, mutants, "swiglu")


def test_act_bwd_gates_pass_honest_and_fail_mutants():
    honest, mutants = {}, {}
    for n, dt in T.ACT_CASES:
        dy, v = T.act_inputs(n, dt)
        for act in T.ACTS:
            _record(honest, act, T.act_bwd_gate(T.act_bwd_honest(dy, v, act), dy, v, act))
        _record(mutants, "gelu no_vpdf", T.act_bwd_gate(T.act_bwd_honest(dy, v, "gelu", no_vpdf=True), dy, v, "gelu"))
        _record(mutants, "quick_gelu lose_1702",
                T.act_bwd_gate(T.act_bwd_honest(dy, v, "quick_gelu", lose_1702=True), dy, v, "quick_gelu"))
    _assert_mutants(honest, mutants, "act_bwd")


def test_unit_normal_norm_of_the_old_tests_misses_what_the_gates_catch():
    """the figure the gates exist for: rmsnorm_bwd8p_k's row dot product without wave part 3 moves dx by
    well under 1 % of max|ref| on unit-normal data at 4096 columns (the close() of tests/test_ops_gpu.py
    passes it), and by hundreds of times the per-element gate"""
    rows, cols = 37, 4096
    d = T.norm_inputs(rows, cols, BF, "normal")
    rstd = T.rms_stats(d["x"])
    good, _ = T.rms_bwd_honest(d["dy"], d["x"], d["w"], rstd, dres=d["dres"])
    bad, _ = T.rms_bwd_honest(d["dy"], d["x"], d["w"], rstd, dres=d["dres"], miss_part3=True)
    share = ((bad.float() - good.float()).abs().max() / good.float().abs().max()).item()
    w = T.rms_dx_gate(bad, d["dy"], d["x"], d["w"], rstd, d["dres"])
    print(f"wave part 3 dropped: {100 * share:.2f} % of max|ref|, {w:.0f} x the per-element gate")
    assert share < 1e-2 and w > 2.0
