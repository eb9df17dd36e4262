"""The training cycle on the MI355X against the gates of tests/cycle_refs.py (shown to discriminate on the
CPU by tests/test_cycle_refs_host.py): how the model hands every gradient producer its (view, beta) over
the micro-batches of an accumulation cycle, and how the accumulated gradient becomes new weights. The
small kernel-shaped config of tests/test_model_gpu.py; one model per recipe, reused over the cycles
(a cycle starts with zero_grad(), and that reuse is part of what is tested).

  additivity  the arena after the cycle against the sum of the kernels' own single-micro-batch
              gradients, every element of every trainable arena: first write bitwise, the sum within
              sum_{k>=2} U (|acc_k| + 2 |g_k|); keys no micro-batch reaches exactly 0 and skipped;
              sequences (A, B), (A, C), (C, A), (A, B, C); full, reference, LoRA (dropout 0 and
              0.05), supervised rows, packed rows, both, and the f32 parity mode (per tensor, 1e-3);
  stale       NaN in every gradient buffer before a C-only cycle: finite, bitwise the C-only gradient;
  update      six optimizer cycles step by step against float64, teacher-forced: norm and clip
              coefficient over all arenas, the cosine LR, AdamW per key at the key's own step count,
              skipped keys untouched; bf16 and f32 moments, and the side-stream update;
  trainer     Accel(grad_accum=2).accumulate() around CuLLaVOPipeline.forward_step: the gradient that
              reaches each step is the mean of the cycle's micro-batches (accelerate's backward
              divides the loss); grad_accum = 1 is bitwise the plain loss.backward().

One JSON line per case is appended to the statistics file of tests/test_accuracy_gpu.py (its _log);
the lines of one MI355X run are committed as profiles/r22/cycle/cycle_stats.jsonl. Measured there
(worst err / gate per arena): additivity 0.479 .. 0.988 over the bf16 recipes and sequences (0 for the projector where only one
micro-batch of the cycle reaches it: its single write is bitwise the single gradient), the supervised-
and packed-row recipes figure for figure the full recipe's; the f32 parity mode 2.5e-9 .. 2.9e-8 rel-L2
against its 1e-3; update m 0.030 .. 0.996, v 0.268 .. 0.996, p 0.988 .. 0.996 over the 36 cycles (0.996 is
where a bf16 store's half ulp meets its gate); trainer 0.812 .. 0.992. No value above 1.0.
"""
import copy
import types

import pytest
import torch

from oracle import cullavo_oracle as O
from tests import cycle_refs as C
from tests.test_accuracy_gpu import _log  # the same statistics file, one line per case

pytestmark = pytest.mark.gpu

RECIPES = {
    "full": dict(trainable="full"),
    "reference": dict(trainable="reference"),
    "lora": dict(trainable="lora", dropout=0.0),
    "lora-dropout": dict(trainable="lora", dropout=0.05),
    "supervised-rows": dict(trainable="full", supervised=True),
    "packed-rows": dict(trainable="full", packed=True),
    "packed-supervised-rows": dict(trainable="full", packed=True, supervised=True),
    "f32-parity": dict(trainable="full", f32=True),
}
ADDITIVITY_CASES = [(r, s) for r in RECIPES for s in C.SEQUENCES if r != "f32-parity" or s == "AB"]


def build(recipe):
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    r = RECIPES[recipe]
    kw = {}
    if r["trainable"] == "lora":
        from cullavo_amd.lora import LoraSettings
        # vision layer 1 runs, layer 2 lies above the selected feature layer: its adapters never do
        kw["lora"] = LoraSettings(r=64, lora_alpha=16.0, lora_dropout=r["dropout"], vision_layers=(1, 2))
    if r.get("f32"):
        kw["dtype"] = torch.float32
    m = CuLLaVOModel(tiny_gpu(), device="cuda", trainable=r["trainable"], init="none", **kw)
    m.load_state_dict(O.make_weights(O.config_small_gpu(), C.WEIGHT_SEED), strict=False)
    if "lora" in m.arenas:
        from cullavo_amd.lora import init_lora_
        init_lora_(m.arenas["lora"], 5)
        with torch.no_grad():   # init_lora_ leaves lora_B at 0, and with it every lora_A gradient
            g = torch.Generator(device="cuda").manual_seed(3)
            for k, p in m.arenas["lora"].params.items():
                if ".lora_B." in k:
                    p.copy_(torch.randn(p.shape, device="cuda", generator=g) * 0.05)
        m.train()
    m.supervised_rows = bool(r.get("supervised"))
    m.packed_rows = bool(r.get("packed"))
    m._cycle_dropout = bool(r.get("dropout"))
    return m


_BATCHES = {}


def batch(name):
    if not _BATCHES:
        for n, b in C.make_batches().items():
            _BATCHES[n] = (b, tuple(t.cuda() if t is not None else None for t in b))
    return _BATCHES[name]


def forward(m, name):
    host, (ids, mask, pix, labels) = batch(name)
    kw = {}
    if m.supervised_rows:
        kw["num_supervised"] = C.num_supervised(host)
    if pix is None and m.packed_rows:
        kw["attended_lens"] = C.attended_lens(host)
    if getattr(m, "_cycle_dropout", False):
        torch.manual_seed(C.DROPOUT_SEEDS[name])   # StepContext draws the forward's lora_seed from it
    return m(input_ids=ids, pixel_values=pix, attention_mask=mask, labels=labels, **kw)


def trainable_arenas(m):
    return {n: a for n, a in m.arenas.items() if a.trainable}


def snapshot(m):
    """{arena: grad_flat clone}, the range of a key without a write in this cycle as 0 (it still
    holds what the last cycle left)"""
    torch.cuda.synchronize()
    out = {}
    for n, a in trainable_arenas(m).items():
        g = a.grad_flat.clone()
        for k, (o, cnt, _) in a.offsets.items():
            if k not in a._written:
                g[o:o + cnt] = 0
        out[n] = g
    return out


def run_cycle(m, seq, zero=True):
    """one accumulation cycle: (snapshots after each micro-batch, the last after finalize_grads;
    {arena: skipped keys})"""
    if zero:
        for a in m.arenas.values():
            a.zero_grad()
    snaps = []
    for i, name in enumerate(seq):
        forward(m, name).loss.backward()
        if i == len(seq) - 1:
            for a in m.arenas.values():
                a.finalize_grads()
        snaps.append(snapshot(m))
    return snaps, {n: set(a.skipped) for n, a in trainable_arenas(m).items()}


class State:
    def __init__(self, recipe):
        self.recipe, self.m, self.single = recipe, build(recipe), {}

    def g(self, name):
        """the kernels' own gradient of micro-batch `name` alone: ({arena: grad_flat}, skipped)"""
        if name not in self.single:
            snaps, skipped = run_cycle(self.m, (name,))
            for n, a in trainable_arenas(self.m).items():   # the reach rule the other checks rely on
                for k in a.offsets:
                    assert (k in skipped[n]) == (not C.reaches(k, name)), (self.recipe, name, k)
            self.single[name] = (snaps[-1], skipped)
        return self.single[name]


@pytest.fixture(scope="module")
def states():
    cache = {}

    def get(recipe):
        if recipe not in cache:
            cache[recipe] = State(recipe)
        return cache[recipe]
    yield get
    cache.clear()


def _worst_key(a, acc, g, scale=1.0):
    """the key of arena a with the largest err / gate (for the failure message)"""
    best = (0.0, None)
    for k, (o, n, _) in a.offsets.items():
        w = max(C.accum_gates([s[o:o + n] for s in acc], [t[o:o + n] for t in g], scale))
        if w > best[0]:
            best = (w, k)
    return best


def check_accumulated(m, seq, acc, g, skipped, scale=1.0, parity=False):
    """the additivity gates over every trainable arena; returns ({arena: worst}, failures)"""
    worsts, fails = {}, []
    for n, a in trainable_arenas(m).items():
        accs, gs = [s[n] for s in acc], [t[n] for t in g]
        if parity:
            w = max(C.parity_gate(accs[-1][o:o + cnt], [t[o:o + cnt] for t in gs]) for o, cnt, _ in a.offsets.values())
            first = 0.0 if torch.equal(accs[0], gs[0]) else float("inf")
        else:
            first, w = C.accum_gates(accs, gs, scale)
        worsts[n] = w
        if first:
            fails.append(f"arena {n}: the first write is not bitwise the single gradient")
        if not w <= 1.0:
            fails.append(f"arena {n}: worst err/gate {w:.3g}" + ("" if parity else f" at key {_worst_key(a, accs, gs, scale)[1]}"))
        for k, (o, cnt, _) in a.offsets.items():
            reached = any(C.reaches(k, name) for name in seq)
            if (k in skipped[n]) == reached:
                fails.append(f"{k}: reached {reached}, skipped {k in skipped[n]}")
            if not reached and not C.unreached_ok(accs[-1][o:o + cnt], k in skipped[n]):
                fails.append(f"{k}: unreached but not an exact zero")
    return worsts, fails


# ---------------------------------------------------------------------------------------------
# 1. additivity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,sname", ADDITIVITY_CASES)
def test_accumulated_gradient_is_the_sum(states, recipe, sname):
    st, seq = states(recipe), C.SEQUENCES[sname]
    g = [st.g(name)[0] for name in seq]
    acc, skipped = run_cycle(st.m, seq)
    worsts, fails = check_accumulated(st.m, seq, acc, g, skipped, parity=recipe == "f32-parity")
    print(f"{recipe} {sname}: worst err/gate per arena {worsts}")
    _log({"test": "additivity", "recipe": recipe, "sequence": sname, "worst": worsts, "fails": fails})
    assert not fails, f"{recipe} {seq}: " + "; ".join(fails[:8])


@pytest.mark.parametrize("recipe", ["full", "lora", "packed-supervised-rows"])
def test_c_only_cycle_leaves_unreached_keys_zero_and_skipped(states, recipe):
    st = states(recipe)
    run_cycle(st.m, ("A", "B"))
    acc, skipped = run_cycle(st.m, ("C",))
    _, fails = check_accumulated(st.m, ("C",), acc, [st.g("C")[0]], skipped)
    assert not fails, fails[:8]
    proj = st.m.arenas["projector"]
    assert skipped["projector"] == set(proj.offsets) and float(proj.grad_flat.float().abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# 2. stale buffers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", ["full", "lora"])
def test_cycle_ignores_what_the_last_one_left(states, recipe):
    st = states(recipe)
    ref, ref_skipped = st.g("C")
    run_cycle(st.m, ("A", "B"))
    for a in st.m.arenas.values():
        a.zero_grad()
    for a in trainable_arenas(st.m).values():
        a.grad_flat.fill_(float("nan"))   # what a step with an overflowed gradient leaves behind
    acc, skipped = run_cycle(st.m, ("C",), zero=False)
    for n, a in trainable_arenas(st.m).items():
        assert torch.isfinite(acc[-1][n].float()).all(), f"arena {n}: a stale NaN was read"
        assert torch.equal(acc[-1][n], ref[n]), f"arena {n}: not bitwise the C-only gradient"
        assert skipped[n] == ref_skipped[n]
        for k, (o, cnt, _) in a.offsets.items():
            if not C.reaches(k, "C"):
                assert C.unreached_ok(acc[-1][n][o:o + cnt], k in skipped[n]), k
    for a in trainable_arenas(st.m).values():   # leave finite buffers to the tests that reuse the model
        assert torch.isfinite(a.grad_flat.float()).all()


# ---------------------------------------------------------------------------------------------
# 3. the update cycle
# ---------------------------------------------------------------------------------------------
def run_update(recipe, sdt, overlap, max_norm, gated=True):
    """six optimizer cycles; returns (f64 norms, per-cycle worsts, failures)"""
    from cullavo_amd.optim import FusedAdamW
    m = build(recipe)
    opt = FusedAdamW(list(m.arenas.values()), lr=C.LR0, weight_decay=C.WD, state_dtype=sdt, overlap=overlap)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=C.T_MAX, eta_min=C.LR_LAST)
    own = [{k: 0 for k in a.offsets} for a in opt.arenas]
    frozen = {n: a.flat.clone() for n, a in m.arenas.items() if not a.trainable}
    norms, worsts, fails = [], [], []
    opt.zero_grad()
    for i, seq in enumerate(C.UPDATE_CYCLES):
        run_cycle(m, seq, zero=False)
        opt.synchronize()
        torch.cuda.synchronize()
        before = [(a.flat.clone(), a.grad_flat.clone(), mm.clone(), vv.clone())
                  for a, (mm, vv) in zip(opt.arenas, opt.flat_state)]
        steps0 = copy.deepcopy(opt.key_steps)
        lr = opt.param_groups[0]["lr"]
        opt.clip_grad_norm_(max_norm)
        opt.step()
        opt.synchronize()
        torch.cuda.synchronize()
        coef, norm, sumsq = opt._coef.item(), opt._norm.item(), opt._sumsq.item()
        norms.append(C.norm64([b[1] for b in before]))
        recs = {}
        for ai, a in enumerate(opt.arenas):
            p0, g, m0, v0 = before[ai]
            m1, v1 = opt.flat_state[ai]
            assert sum(n for _, n, _ in a.offsets.values()) == a.numel   # the keys tile the arena: nothing between
            for k, (o, n, _) in a.offsets.items():
                reached = any(C.reaches(k, name) for name in seq)
                own[ai][k] += int(reached)
                s = slice(o, o + n)
                recs[k] = dict(p0=p0[s], g=g[s], m0=m0[s], v0=v0[s], p1=a.flat[s], m1=m1[s], v1=v1[s], reached=reached,
                               step=own[ai][k], opt_step=opt.key_steps[ai][k], opt_step0=steps0[ai][k])
        if gated:
            w, f = C.update_gates(recs, i, lr, coef, norm, sumsq, max_norm, arenas={a.name: list(a.offsets) for a in opt.arenas})
            for n, a in m.arenas.items():
                if not a.trainable and not torch.equal(a.flat, frozen[n]):
                    f.append(f"frozen arena {n} moved")
            worsts.append(w)
            fails += [f"cycle {i + 1} {seq}: {x}" for x in f]
        opt.zero_grad()
        sched.step()
    return norms, worsts, fails


_MAX_NORM = {}


def max_norm_of(recipe):
    """the median of the six f64 norms of an unclipped run of the same cycles (AdamW's update hardly
    depends on the gradient's scale, so the clipped runs see nearly the same norms; each run asserts from
    its own norms that some cycles clip and some do not)"""
    if recipe not in _MAX_NORM:
        _MAX_NORM[recipe] = C.median(run_update(recipe, torch.bfloat16, False, 1e30, gated=False)[0])
    return _MAX_NORM[recipe]


@pytest.mark.parametrize("variant", ["bf16-moments", "f32-moments", "overlap"])
@pytest.mark.parametrize("recipe", ["full", "lora"])
def test_update_cycles_against_f64(recipe, variant):
    mx = max_norm_of(recipe)
    sdt = torch.float32 if variant == "f32-moments" else torch.bfloat16
    norms, worsts, fails = run_update(recipe, sdt, variant == "overlap", mx)
    for i, w in enumerate(worsts):
        print(f"{recipe} {variant} cycle {i + 1}: norm {norms[i]:.6g} (max_norm {mx:.6g}), worst m/v/p "
              f"{w['m']:.3f}/{w['v']:.3f}/{w['p']:.3f}")
        _log({"test": "update", "recipe": recipe, "variant": variant, "cycle": i + 1, "norm": norms[i], "max_norm": mx,
              "worst": w})
    assert any(n > mx for n in norms) and any(n < mx for n in norms), (norms, mx)
    assert not fails, "; ".join(fails[:8])
    for i, w in enumerate(worsts):
        assert max(w.values()) <= 1.0, (i + 1, w)


# ---------------------------------------------------------------------------------------------
# 4. the trainer's accumulation path
# ---------------------------------------------------------------------------------------------
def _trainer(m, grad_accum):
    from cullavo_amd.optim import FusedAdamW
    from cullavo_amd.pipeline import CuLLaVOPipeline
    from cullavo_amd.trainer import Accel, DefaultTrainer
    accel = Accel(grad_accum=grad_accum)
    opt = FusedAdamW(list(m.arenas.values()), lr=C.LR0, weight_decay=C.WD)
    accel.optimizer = opt
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=C.T_MAX, eta_min=C.LR_LAST)
    tr = types.SimpleNamespace(model=types.SimpleNamespace(cullavo_model=m), accel=accel, optimizer=opt,
                               lr_scheduler=sched, train_params={"optim_steps": 0})
    tr.compute_loss = lambda f, b: f(tr, b)
    tr.backward_loss = lambda loss: DefaultTrainer.backward_loss(tr, loss)
    tr.update_model = lambda: DefaultTrainer.update_model(tr)
    pipe = CuLLaVOPipeline({"OPTIMIZER": {"GRAD_MAX": 10.0}})
    pipe.forward_func = lambda t, b: {"loss_llm": forward(m, b["name"]).loss}   # instance attribute: not bound
    return tr, pipe


def _trainer_batch(name):
    return {"name": name, "input_ids": batch(name)[1][0]}


def test_trainer_grad_cum():
    """accelerate's Accelerator.backward, which the reference calls, holds
    `loss = loss / self.gradient_accumulation_steps`: each step sees the mean over its cycle."""
    m = build("full")
    tr, pipe = _trainer(m, 2)
    opt, events, at_step = tr.optimizer, [], []
    real = {"zero": opt.zero_grad, "sched": tr.lr_scheduler.step}

    def before_step(*_):
        events.append("step")
        torch.cuda.synchronize()
        at_step.append(({n: ar.grad_flat.clone() for n, ar in trainable_arenas(m).items()},
                        {n: set(ar.skipped) for n, ar in trainable_arenas(m).items()}))
    opt.register_step_pre_hook(before_step)
    opt.zero_grad = lambda *a, **k: (events.append("zero"), real["zero"](*a, **k))[1]
    tr.lr_scheduler.step = lambda *a, **k: (events.append("sched"), real["sched"](*a, **k))[1]

    names, sync, fails, worsts = ("A", "B", "C", "A"), [], [], []
    for c in range(2):
        seq = names[2 * c:2 * c + 2]
        g = [run_cycle(m, (n,))[0][-1] for n in seq]   # at this cycle's weights
        for a in m.arenas.values():
            a.zero_grad()
        acc = []
        for n in seq:
            with tr.accel.accumulate(tr.model):
                pipe.forward_step(tr, _trainer_batch(n))
            sync.append(tr.accel.sync_gradients)
            acc.append(snapshot(m) if not tr.accel.sync_gradients else at_step[-1][0])
        w, f = check_accumulated(m, seq, acc, g, at_step[-1][1], scale=0.5)
        worsts.append(w)
        fails += [f"cycle {c + 1} {seq}: {x}" for x in f]
    print(f"trainer GRAD_CUM 2: worst err/gate per arena {worsts}")
    _log({"test": "trainer", "worst": worsts, "fails": fails})
    assert sync == [False, True, False, True]
    assert events == ["step", "zero", "sched"] * 2 and tr.train_params["optim_steps"] == 2
    assert not fails, "; ".join(fails[:8])


def test_trainer_grad_cum_one_is_plain_backward():
    m = build("full")
    plain = run_cycle(m, ("A",))[0][-1]
    tr, pipe = _trainer(m, 1)
    tr.update_model = lambda: None   # keep the gradient: read it after the step's clip
    for a in m.arenas.values():
        a.zero_grad()
    with tr.accel.accumulate(tr.model):
        pipe.forward_step(tr, _trainer_batch("A"))
    assert tr.accel.sync_gradients
    got = snapshot(m)
    for n in plain:
        assert torch.equal(got[n], plain[n]), n
