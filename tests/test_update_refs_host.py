"""The gates of tests/update_refs.py discriminate, shown on the CPU before any GPU time is spent.

For every input set of tests/test_update_accuracy_gpu.py (same seeds, same shapes) an honest
restatement of the kernel (torch f32, the kernel's operation order and rounding points, sums in the
kernel's lane / wave / workgroup order) stays at or below 1.0 of its gate; the worst err / gate of
every family is printed (pytest -s). Each one-line mutant of a restatement exceeds 2.0 on at least
one input set. The sets on which a mutant computes what the honest form computes are named where
they are left out; nothing is skipped silently. The geometry the cases were sized for (AdamW's
second trip, sumsq's further grid-stride passes, colsum's empty row slots, embedding_bwd's register
chunks) is asserted from the restated launch arithmetic.
"""
import math

import torch

from tests import update_refs as R
from tests.test_train_refs_host import _assert_mutants, _record

BF, F32 = R.BF, R.F32


# ---------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------
def test_adamw_plan_serves_each_case_its_purpose():
    """n = 18789 on the vector path: 3 workgroups, 768 threads, two trips; the second trip's first half is
    live in every thread, its second half in 44 of them"""
    g, trips, first_live, second_live, threads = R.adamw_plan(R.ADAM_N_TRIPS, True)
    assert (g, trips, threads) == (3, 2, 768)
    assert first_live == threads and 0 < second_live == 44 < threads // 2
    assert R.ADAM_N_TRIPS % 8 == 5                                   # and a scalar tail behind the vectors
    assert R.adamw_plan(R.ADAM_N_TRIPS, False)[:2] == (19, 0)        # unaligned: the scalar loop alone
    assert R.adamw_plan(5, True)[:2] == (1, 0) and R.adamw_plan(8, True)[:4] == (1, 1, 1, 0)
    # which offsets take which path
    assert [R.adamw_vec(o, BF, BF) for o in (0, 1, 4)] == [True, False, False]
    assert [R.adamw_vec(o, BF, F32) for o in (0, 1, 4)] == [True, False, False]
    assert [R.adamw_vec(o, F32, F32) for o in (0, 1, 4)] == [True, False, True]
    # the constants the cases were chosen for
    c1, c1000 = R.AdamConsts(1, 0.1), R.AdamConsts(1000, 0.1)
    assert abs(c1.d("bc1") - 0.1) < 2.0 ** -20 and c1000.d("bc1") == 1.0
    assert 0.79 < c1000.d("bc2s") < 0.80 and c1.d("bc2s") < 0.04        # sqrt(1 - 0.999^1000) against sqrt(0.001)
    assert c1.d("c1") == 1.0 - c1.d("b1") and c1.d("c2") == 1.0 - c1.d("b2")   # exact in f32


def test_adamw_inputs_hold_the_edges():
    for pdt, sdt in R.ADAM_DTYPES:
        p, g, m, v = R.adamw_inputs(R.ADAM_N_TRIPS, pdt, sdt, 1000, 0.1, 0.37)
        c = R.AdamConsts(1000, 0.1)
        assert g[0] == 0 and m[0] == 0 and v[0] == 0 and g[2] == 0 and m[2] != 0 and v[2] != 0
        _, M1, V1 = R.adamw_state_ref(g, m, v, c, 0.37)
        assert V1[1].sqrt() / c.d("bc2s") < 2.0 ** -10 * c.d("eps") and V1[1] > 0   # eps dominates the denominator
        upd = c.d("step_size") * M1 / (V1.sqrt() / c.d("bc2s") + c.d("eps"))
        # the update is many bf16 ulps of a typical p, and the planted elements cancel against it
        assert upd.abs().median() > 16 * 2.0 ** -7 * p.double().abs().median()
        left = (R.adamw_p_decayed(p, c).double() - upd).abs()
        assert (left[19::16] < 0.25 * upd[19::16].abs()).double().mean() > 0.9
        # buffers at the three offsets really start there
        for off in (0, 1, 4):
            assert (R.at_offset(p, off).data_ptr() - off * p.element_size()) % 16 == 0


def _adam_excused(mutant, pdt, sdt, step, wd, gs):
    """the sets on which a mutant computes what the honest kernel computes"""
    if mutant in ("gs_ignored", "gs_not_in_square"):
        return gs is None or gs == 1.0          # no scale, or the scale 1.0
    if mutant == "no_bc1":
        return step == 1000                     # bc1 = 1 - 0.9^1000 rounds to 1.0f
    if mutant == "decay_after":
        # wd = 0: the decay factor is 1.0f. bf16 parameters at wd = 0.1: p * 0.999 rounds back to p, and the
        # mutant's factor 0.999 on the result is inside U |p'|; the set with lr wd = 0.05 shows it
        return wd == 0.0 or (pdt == BF and wd < 1.0)
    if mutant == "unrounded_moments":
        return sdt == F32                       # an f32 state is not rounded
    return False


def test_adamw_gates_pass_honest_and_fail_mutants():
    for pdt, sdt in R.ADAM_DTYPES:
        honest, mutants = {}, {}
        for n, step, wd, gs, off in R.ADAM_CASES:
            p, g, m, v = R.adamw_inputs(n, pdt, sdt, step, wd, gs)
            c = R.AdamConsts(step, wd)
            for k, w in zip(("m", "v", "p"), R.adamw_gates(*R.adamw_honest(p, g, m, v, c, gs), p, g, m, v, c, gs)):
                _record(honest, k, w)
            if off != 0:
                continue  # the offset moves the buffers, not the values: the restatement is the same
            for name in R.ADAM_MUTANTS:
                if _adam_excused(name, pdt, sdt, step, wd, gs):
                    continue
                _record(mutants, name, max(R.adamw_gates(*R.adamw_honest(p, g, m, v, c, gs, mutant=name), p, g, m, v, c, gs)))
        if sdt == F32:
            assert "unrounded_moments" not in mutants   # excused on every f32-state set, caught with bf16 state
        _assert_mutants(honest, mutants, f"adamw {R.case_id((pdt, sdt))}")


def test_adamw_project_lr_would_hide_the_update():
    """why the sets use lr = 0.01: at the project's 2e-5 the whole update of a typical element is a small
    fraction of U |p|, a per-element gate of that size would pass a kernel that does not update at all"""
    p, g, m, v = R.adamw_inputs(R.ADAM_N_TRIPS, BF, BF, 1000, 0.0, None)
    c = R.AdamConsts(1000, 0.0, lr=2.0e-5)
    _, M1, V1 = R.adamw_state_ref(g, m, v, c, None)
    upd = c.d("step_size") * M1 / (V1.sqrt() / c.d("bc2s") + c.d("eps"))
    plain = torch.ones(p.numel(), dtype=torch.bool)
    plain[3::16] = False
    share = (upd.abs() / (R.U * p.double().abs()).clamp_min(R.FLOOR))[plain].median().item()
    print(f"lr 2e-5: the median update is {share:.3f} of U |p|")
    assert share < 0.5


# ---------------------------------------------------------------------------------------------
# sumsq, clip_coef, scale_inplace
# ---------------------------------------------------------------------------------------------
def test_sumsq_plan_serves_each_case_its_purpose():
    assert R.sumsq_plan(5) == (1, 0, 5) and R.sumsq_plan(8) == (1, 1, 0) and R.sumsq_plan(2051) == (1, 1, 3)
    g, passes, tail = R.sumsq_plan(R.SUMSQ_N_BIG)
    assert g == R.SUMSQ_PARTIALS and passes == 3 and tail == 3      # capped: a second pass for all, a third for 300
    assert R.SUMSQ_N_BIG // 8 - 2 * g * 256 == 300
    assert R.sumsq_plan(R.SUMSQ_PASS)[:2] == (1024, 1)               # the largest n of a single pass
    x = R.sumsq_inputs(2051, BF, "spike").float()
    assert x.abs().max() >= 2.0 ** 10 * x.abs().sort().values[-2]    # one element 2^10 times the rest


def test_sumsq_gate_passes_honest_and_fails_mutants():
    honest, mutants = {}, {}
    for dt in R.SUMSQ_DTYPES:
        for n, kind in R.SUMSQ_CASES:
            x = R.sumsq_inputs(n, dt, kind)
            _record(honest, f"out {R.case_id((dt,))}", R.sumsq_gate(R.sumsq_honest(x), x))
            _, passes, tail = R.sumsq_plan(n)
            for name in R.SUMSQ_MUTANTS:
                if name == "no_tail" and tail == 0:
                    continue   # n = 8: no tail to drop
                if name == "no_second_pass" and passes < 2:
                    continue   # every n but the large one: a single pass
                _record(mutants, name, R.sumsq_gate(R.sumsq_honest(x, mutant=name), x))
    _assert_mutants(honest, mutants, "sumsq")


def test_clip_coef_check_passes_honest_and_rejects_wrong_values():
    for s, mn in R.CLIP_CASES:
        coef, norm = R.clip_coef_honest(s, mn)
        assert not R.clip_coef_check(s, mn, coef, norm), (s, mn)
        assert not R.clip_coef_check(s, mn, coef, None)
    assert R.clip_coef_honest(0.25, 1.0)[0] == 1.0 and R.clip_coef_honest(0.0, 1.0) == (1.0, 0.0)
    coef, norm = R.clip_coef_honest(float("nan"), 1.0)
    assert coef == 1.0 and math.isnan(norm)
    coef, norm = R.clip_coef_honest(7.3, 1.0)
    assert R.clip_coef_check(7.3, 1.0, coef * (1 + 2.0 ** -21), norm)        # 8 E off
    assert R.clip_coef_check(7.3, 1.0, coef, norm * (1 + 2.0 ** -21))
    assert R.clip_coef_check(7.3, 1.0, 1.0 / math.sqrt(7.3 + 1e-6), norm)    # 1e-6 under the root
    assert R.clip_coef_check(0.25, 1.0, 1.0 - 2.0 ** -24, 0.5)               # not exactly 1.0
    assert R.clip_coef_check(0.0, 1.0, 0.0, 0.0)
    assert R.clip_coef_check(float("nan"), 1.0, float("nan"), float("nan"))  # torch's answer: not the kernel's


def test_scale_gate_passes_honest_and_fails_mutant():
    honest, mutants = {}, {}
    for n, dt, s in R.SCALE_CASES:
        x = R.scale_inputs(n, dt)
        y = R.scale_honest(x, s)
        _record(honest, f"y {R.case_id((dt,))}", R.scale_gate(y, x, s))
        if s == 1.0:
            assert torch.equal(y, x)
        else:   # s = 1.0: s * s is s
            _record(mutants, "twice", R.scale_gate(R.scale_honest(x, s, mutant="twice"), x, s))
    _assert_mutants(honest, mutants, "scale_inplace")


# ---------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------
def test_colsum_plan_serves_each_case_its_purpose():
    assert R.COLSUM_SLOTS == 256
    assert [R.colsum_rows_per_lane(r) for r in (1, 255, 256, 257, 1000)] == [1, 1, 1, 2, 4]
    assert 255 < R.COLSUM_SLOTS                  # (255, 264): row slot 255 stays empty
    assert 264 - 256 == 8 and 520 - 512 == 8     # the last column workgroup holds one group of 8
    x, _ = R.colsum_inputs(1000, 520, BF, "cancel")
    X = x.double()
    assert (X.sum(0).abs() < 2.0 ** -8 * X.abs().sum(0)).all()   # columns cancel to under 1/256 of their magnitude


def test_colsum_gate_passes_honest_and_fails_mutants():
    honest, mutants = {}, {}
    for rows, cols, idt, odt, beta, kind in R.COLSUM_CASES:
        x, old = R.colsum_inputs(rows, cols, idt, kind)
        _record(honest, f"out {R.case_id((odt,))}", R.colsum_gate(R.colsum_honest(x, old, beta, odt), x, old, beta))
        for name in R.COLSUM_MUTANTS:
            if name in ("no_last_slot", "no_p31") and rows == 1:
                continue   # (1, 8): row 0 is row lane 0 of partial 0
            if name == "no_beta" and beta == 0.0:
                continue   # nothing to accumulate onto
            _record(mutants, f"{name} {kind}", R.colsum_gate(R.colsum_honest(x, old, beta, odt, mutant=name), x, old, beta))
    _assert_mutants(honest, mutants, "colsum")


def test_colsum_gate_on_the_cancelling_set_catches_a_dropped_partial():
    """the cancelling set holds the gate to what it claims: the column sums are tiny, the gate follows
    sum |x|, and a dropped partial still stands far above it"""
    x, old = R.colsum_inputs(1000, 520, BF, "cancel")
    bad = R.colsum_honest(x, old, 0.0, F32, mutant="no_p31")
    w = R.colsum_gate(bad, x, old, 0.0)
    print(f"colsum without partial 31 on the cancelling set: {w:.0f} x the per-column gate")
    assert w > 2.0


# ---------------------------------------------------------------------------------------------
# embedding backward, forward, row gather
# ---------------------------------------------------------------------------------------------
def test_emb_ids_serve_each_case_their_purpose():
    assert [R.emb_chunks(d) for d in (8, 256, 2048, 2056, 8192)] == [1, 1, 1, 2, 4]
    assert 2056 // 8 - 256 == 1                          # chunk c = 1 of dim 2056: thread 0 alone
    ids = R.emb_ids(700)
    pos = (ids == R.EMB_MANY).nonzero()[:, 0]
    assert pos.numel() > 256 and pos[-1] - pos[0] >= 512   # more than 256 occurrences, three windows from the first
    assert R.emb_ids(300).eq(R.EMB_MANY).sum() >= 99
    for n in (1, 300, 700):
        ids = R.emb_ids(n)
        assert ids[n - 1] == R.EMB_LONE and (ids == R.EMB_LONE).sum() == 1   # a first occurrence at position n - 1
        assert not (ids == 0).any() and not ((ids >= 40) & (ids < R.EMB_LONE)).any()
        if n >= 300:
            assert ids[1] == -100 and ids[2] == R.EMB_VOCAB


def test_emb_bwd_gate_passes_honest_and_fails_mutants():
    honest, mutants, caught_by_sentinel = {}, {}, 0
    for dim, n, tt, td, beta in R.EMB_BWD_CASES:
        ids, dout, old = R.emb_bwd_inputs(dim, n, tt, td)
        w, same = R.emb_bwd_gate(R.emb_bwd_honest(ids, dout, old, beta), ids, dout, old, beta)
        assert same
        _record(honest, f"dtable {R.case_id((tt,))}", w)
        for name in R.EMB_MUTANTS:
            if name == "first_window_only" and n < 300:
                continue   # n = 1: one window
            if name == "chunk0_only" and R.emb_chunks(dim) == 1:
                continue   # dims up to 2048: chunk 0 is the row
            if name == "clamp_ids" and n < 300:
                continue   # n = 1: no id out of range
            if name == "beta_everywhere" and beta == 1.0:
                continue   # 1.0 * old keeps the bits of old
            w, same = R.emb_bwd_gate(R.emb_bwd_honest(ids, dout, old, beta, mutant=name), ids, dout, old, beta)
            if name in ("clamp_ids", "beta_everywhere"):
                assert not same, f"{name}: the untouched rows kept their bits at {dim}, {n}"
            if name == "beta_everywhere":
                caught_by_sentinel += 1
                continue   # the hit rows are right: the bitwise check of the untouched rows alone catches it
            _record(mutants, name, w)
    print(f"embedding_bwd mutant beta_everywhere: untouched rows changed on {caught_by_sentinel} sets (beta = 0)")
    assert caught_by_sentinel >= 1 and set(mutants) == set(R.EMB_MUTANTS) - {"beta_everywhere"}
    _assert_mutants(honest, mutants, "embedding_bwd")


def test_gather_refs():
    for dim, dt in R.GATHER_CASES:
        a, b, ids, src = R.gather_inputs(dim, dt)
        out = R.embedding_fwd_ref(ids, a)
        assert torch.equal(out[1], a[49]) and torch.equal(out[3], out[5]) and not out[[2, 4, 6, 9]].any()
        assert ((ids < 0) | (ids >= R.EMB_VOCAB)).sum() == 4
        o2 = R.row_gather2_ref(src, a, b)
        assert torch.equal(o2[1], b[0]) and torch.equal(o2[4], b[5]) and torch.equal(o2[3], a[49]) and not o2[[2, 6, 10]].any()
        sa = src.clamp_max(R.EMB_VOCAB - 1)
        assert torch.equal(R.row_gather2_ref(sa, a, None)[1], a[49])


# ---------------------------------------------------------------------------------------------
# CLIP front end
# ---------------------------------------------------------------------------------------------
def test_vis_cases_serve_their_purpose():
    assert [R.vis_nch(c[2]) for c in R.VIS_CASES] == [1, 2, 2, 8, 16, 2]
    assert [c[0] * c[1] % 4 for c in R.VIS_CASES[:5]] == [3, 3, 2, 1, 3]   # every last workgroup partly empty


def test_vis_gate_passes_honest_and_fails_mutants():
    honest, mutants = {}, {}
    for B, T, dim, dt in R.VIS_CASES:
        x, cls, pos, w, b = R.vis_inputs(B, T, dim, dt)
        assert (x[::T].float() >= 0.99 * R.VIS_X_CLS).all()
        _record(honest, f"y {R.case_id((dt,))}", R.vis_gate(R.vis_honest(x, cls, pos, w, b, T), x, cls, pos, w, b, T))
        for name in R.VIS_MUTANTS:
            if name == "pos_by_row" and B == 1:
                continue   # one image: row % T is the row
            if name == "padded_div" and 512 * R.vis_nch(dim) == dim:
                continue   # 1024 columns: the padded width is the width
            if name == "v_not_rounded" and dt == F32:
                continue   # an f32 sum is not rounded again
            _record(mutants, name, R.vis_gate(R.vis_honest(x, cls, pos, w, b, T, mutant=name), x, cls, pos, w, b, T))
    _assert_mutants(honest, mutants, "vision_embed_ln")


def test_im2col_ref_is_the_convolution_unfold_and_fails_mutants():
    s = R.IM2COL_SHAPE
    B, C, H, W, patch, kpad = (s[k] for k in ("B", "C", "H", "W", "patch", "kpad"))
    gh, gw = H // patch, W // patch
    assert gh != gw and kpad > C * patch * patch
    for pdt, odt in R.IM2COL_DTYPES:
        pix = R.im2col_inputs(pdt)
        ref = R.im2col_ref(pix, patch, kpad, odt)
        # the order of the convolution's own unfold, written without index arithmetic
        unf = torch.nn.functional.unfold(pix.float(), patch, stride=patch).transpose(1, 2)   # [B, P, C p p]
        got = ref.view(B, 1 + gh * gw, kpad)
        assert torch.equal(got[:, 1:, :C * patch * patch].float(), unf.to(odt).float())
        assert not got[:, 0].any() and not got[:, :, C * patch * patch:].any()
        for name in ("py_by_gh", "swap_ch"):
            assert not torch.equal(R.im2col_ref(pix, patch, kpad, odt, mutant=name), ref), name
    # on a square image the first mutant is the kernel: what the older front-end test could not see
    sq = torch.randn(1, 3, 8, 8, generator=R._gen("im2col-square"))
    assert torch.equal(R.im2col_ref(sq, 4, 48, F32, mutant="py_by_gh"), R.im2col_ref(sq, 4, 48, F32))
