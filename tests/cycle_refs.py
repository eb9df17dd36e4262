"""Gates, case tables and host restatements for the training cycle: how the gradient producers share the
never-cleared gradient arenas over the micro-batches of one accumulation cycle (arena.grad_slot's
(view, beta) per key, mark_written for the siblings of a fused slot, finalize_grads, zero_grad) and how
the accumulated gradient becomes new weights (the clip coefficient over all arenas, the LR schedule,
AdamW with per-key step counts and skipped keys). Every kernel on the way is pinned on its own
elsewhere; what is gated here is the composition.
Plain torch on whatever device the tensors live on, nothing of the GPU library is imported:
tests/test_cycle_refs_host.py proves on the CPU that the gates pass the honest forms and fail a set of
one-line mutants, tests/test_cycle_accuracy_gpu.py then holds the model to the same gates.

Additivity. With g_k the gradient of micro-batch k alone (the kernels' own, as stored: one bf16
rounding of the f32 value t_k) and acc_k the arena after micro-batch k of a cycle of n:
  acc_1 = g_1 bitwise (the same kernels on the same inputs at beta 0);
  acc_k = round(acc_{k-1} + t_k), so |acc_k - (acc_{k-1} + g_k)| <= U |acc_k| + |g_k - t_k|, and
  |g_k - t_k| <= U |t_k| <= U |g_k| (1 + U); the gate allows 2 U |g_k|, the second U for a rounding of
  t_k that falls the other way where a plan orders its f32 sum differently at beta 1. Summed:
  |acc_n - sum_k g_k| <= sum_{k >= 2} U (|acc_k| + 2 |g_k|), per element.
Nothing of the size of |g_1| or |g_k| fits under it. A key that a micro-batch does not reach has
g_k = 0 there, and acc_k counts as 0 until the key's first write (the buffer still holds the last
cycle's values then; finalize_grads zeroes what no micro-batch wrote).
U = 2^-8 (tests/decode_refs.py). No number here was taken from a kernel's output.
"""
import math

import torch

from oracle import cullavo_oracle as O
from tests import update_refs as UR
from tests.decode_refs import U, bf, worst
from tests.train_refs import E, FLOOR

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
assert U == 2.0 ** -8

# ---------------------------------------------------------------------------------------------
# micro-batches and sequences
# ---------------------------------------------------------------------------------------------
WEIGHT_SEED = 2
C_PADS, C_LEN = (0, 9, 20), 48
SEQUENCES = {"AB": ("A", "B"), "AC": ("A", "C"), "CA": ("C", "A"), "ABC": ("A", "B", "C")}
DROPOUT_SEEDS = {"A": 101, "B": 202, "C": 303}   # torch.manual_seed before the forward of each micro-batch
# the six optimizer cycles of the update test: cycle 3 leaves the projector out, cycle 5 reaches it
# with its second micro-batch only
UPDATE_CYCLES = (("A", "B"), ("B", "A"), ("C", "C"), ("A", "B"), ("C", "A"), ("A", "C"))
LR0, LR_LAST, WD, T_MAX = 1e-3, 1e-5, 0.1, 6
PARITY_GATE = 1e-3   # the f32 parity mode's rel-L2 gate (tests/test_parity_modes.py)


def make_batches():
    """{"A", "B", "C"} -> (ids, mask, pix, labels) on the CPU. A: image batch, seed 2. B: image batch,
    seed 5, row 1 right-padded by 9. C: text only (no <image> id, no pixels), rows right-padded by
    0 / 9 / 20, labels [B, S] on the second half."""
    cfg = O.config_small_gpu()
    a = O.make_inputs(cfg, 2, 40, 4, 2)
    b = O.make_inputs(cfg, 2, 40, 4, 5, pad_tail=[0, 9])
    ids, mask, _, _ = O.make_inputs(cfg, len(C_PADS), C_LEN, 3, 3, pad_tail=list(C_PADS))
    ids[ids == cfg.image_token_index] = 7
    g = torch.Generator().manual_seed(3)
    labels = torch.full((len(C_PADS), C_LEN), -100, dtype=torch.long)
    labels[:, C_LEN // 2:] = torch.randint(2, 1000, (len(C_PADS), C_LEN - C_LEN // 2), generator=g)
    return {"A": a, "B": b, "C": (ids, mask, None, labels)}


def num_supervised(batch):
    return int((batch[3][:, 1:] != -100).sum())


def attended_lens(batch):
    return batch[1].sum(-1).tolist()


def reaches(key, name, vision_layers_run=2):
    """whether micro-batch `name` sends a gradient to parameter `key`: the text-only batch reaches
    neither the projector nor anything in the vision tower; adapters of a vision layer above the
    selected feature layer (layers >= vision_layers_run) never run at all"""
    if key.startswith("vision_tower."):
        if name == "C":
            return False
        layer = int(key.split(".encoder.layers.")[1].split(".")[0]) if ".encoder.layers." in key else 0
        return layer < vision_layers_run
    if key.startswith("multi_modal_projector."):
        return name != "C"
    return True


def oracle_grads(batch, seed=WEIGHT_SEED, keys=None):
    """bf16-faithful oracle forward + autograd on the CPU: {key: bf16 gradient or None}. A text-only
    batch runs the language model on the token embeddings alone (nothing to merge)."""
    cfg = O.config_small_gpu()
    Wb = {k: v.requires_grad_(True) for k, v in O.to_bf16(O.make_weights(cfg, seed)).items()}
    ids, mask, pix, labels = batch
    if pix is not None:
        loss, _, _ = O.forward(Wb, cfg, ids, pix, mask, labels)
    else:
        embeds = Wb["language_model.model.embed_tokens.weight"][ids]
        pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 1)
        hidden, _ = O.llama_hidden(embeds, mask, pos, Wb, cfg.text, None)
        logits = O.linear(hidden, Wb["language_model.lm_head.weight"]).float()
        loss = O.shifted_ce(logits, labels, mask)
    loss.backward()
    return {k: v.grad for k, v in Wb.items() if keys is None or k in keys}


TRAINABLE_PREFIXES = {
    "full": ("multi_modal_projector.", "language_model."),
    "reference": ("multi_modal_projector.", "language_model.model.embed_tokens.", "language_model.lm_head."),
}


# ---------------------------------------------------------------------------------------------
# additivity gate
# ---------------------------------------------------------------------------------------------
def accum_gates(acc, g, scale=1.0):
    """acc: the accumulated gradient after each micro-batch (the last one after finalize_grads, an
    unwritten range as 0), g: the single-micro-batch gradients (0 where not reached); the terms are
    scale g_k (a power of two: exact). Returns (first, total): first is 0.0 where acc_1 is bitwise
    scale g_1 and inf otherwise; total is the worst |acc_n - sum g_k| / gate over the elements."""
    g = [t.double() * scale for t in g]
    first = 0.0 if torch.equal(acc[0].double(), g[0]) else float("inf")
    ref, gate = g[0].clone(), torch.zeros_like(g[0])
    for a, t in zip(acc[1:], g[1:]):
        ref += t
        gate += U * (a.double().abs() + 2 * t.abs())
    return first, worst(acc[-1].double() - ref, gate)


def parity_gate(acc_n, g):
    """the f32 parity mode, per tensor: rel-L2 of acc_n against sum g_k over PARITY_GATE (a zero
    reference demands an exact zero)"""
    ref = sum(t.double() for t in g)
    err = (acc_n.double() - ref).norm().item()
    n = ref.norm().item()
    return 0.0 if err == 0.0 else (float("inf") if n == 0.0 else err / n / PARITY_GATE)


def unreached_ok(grad, in_skipped):
    """a key no micro-batch of the cycle reached: exactly 0 (no NaN, no stale value) and skipped"""
    return bool(in_skipped) and bool((grad == 0).all())


ACCUM_MUTANTS = ("overwrite", "siblings_not_marked", "stale_kept", "first_write_adds", "bias_takes_weight_once",
                 "sum_not_mean")
_SIBLINGS = ("k_proj.weight", "v_proj.weight", "up_proj.weight")   # written through q's / gate's slot


def _weight_of(key):
    return key[:-len("bias")] + "weight" if key.endswith("bias") else None


def accumulate_honest(terms, stale, mutant=None, unrounded=None, scale=1.0):
    """The cycle restated on the CPU. terms: one {key: f32 gradient or None} per micro-batch (None: not
    reached), stale: {key: what the last cycle left in the buffer}. A reached key's first write stores
    round(scale t) (beta 0), later ones round(acc + scale t) (beta 1); finalize zeroes the rest.
    unrounded: optional per-micro-batch {key: t_k before its own rounding}: what an accumulating kernel
    adds. Returns the list of snapshots (unwritten keys as 0) the GPU test takes, bf16 values in f32."""
    buf = {k: v.float().clone() for k, v in stale.items()}
    written, snaps = set(), []
    mscale = 1.0 if mutant != "sum_not_mean" else 1.0 / scale
    for i, tk in enumerate(terms):
        first_of = {k for k, t in tk.items() if t is not None and k not in written}
        for k, t in tk.items():
            if t is None:
                continue
            t = (unrounded[i][k] if unrounded is not None and k in written else t).float() * (scale * mscale)
            beta = 1.0 if k in written else 0.0
            if mutant == "overwrite" and i == 1:
                beta = 0.0
            if mutant == "siblings_not_marked" and k.endswith(_SIBLINGS):
                beta = 0.0
            if mutant == "first_write_adds" and k not in written:
                beta = 1.0
            if mutant == "bias_takes_weight_once" and k.endswith("bias"):
                beta = 1.0 if _weight_of(k) in first_of else 0.0
            buf[k] = bf(t + buf[k]) if beta else bf(t)
        written |= {k for k, t in tk.items() if t is not None}
        snap = {k: (buf[k].clone() if k in written else torch.zeros_like(buf[k])) for k in buf}
        snaps.append(snap)
    for k in buf:   # finalize_grads
        if k not in written and mutant != "stale_kept":
            buf[k] = torch.zeros_like(buf[k])
    snaps[-1] = {k: buf[k].clone() for k in buf}
    return snaps, {k for k in buf if k not in written}


# ---------------------------------------------------------------------------------------------
# the update cycle
# ---------------------------------------------------------------------------------------------
def cosine_lr(step, total=T_MAX, lr=LR0, last_lr=LR_LAST):
    """the closed form of torch's CosineAnnealingLR (trainer.cosine_lr restated)"""
    return last_lr + (lr - last_lr) * (1 + math.cos(math.pi * step / max(1, total))) / 2


# CosineAnnealingLR steps by its recursive form: a few f64 operations per step on values <= lr, so
# after T_MAX steps within 8 T_MAX roundings of the closed form
LR_TOL = 8 * T_MAX * 2.0 ** -53 * LR0


def norm64(grads):
    """f64 L2 norm over every tensor of `grads` together"""
    return math.sqrt(sum((g.double() ** 2).sum().item() for g in grads))


def median(xs):
    s = sorted(xs)
    return 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]) if len(s) % 2 == 0 else s[len(s) // 2]


def sumsq_check(sumsq, arena_grads):
    """The f32 sum of squares the optimizer accumulated over its arenas (one cullavo_sumsq call each,
    out += S_a) against f64: err / gate. update_refs.sumsq_gate's count of f32 additions for an arena of
    n_a elements bounds that call's own error by count_a E S_a, and each of the += rounds the running
    total once more: E S."""
    S = [(g.double() ** 2).sum().item() for g in arena_grads]
    gate = len(S) * E * sum(S) + FLOOR
    for g, s in zip(arena_grads, S):
        wg, passes, _ = UR.sumsq_plan(g.numel())
        gate += ((8 * passes + 1) + 1 + 6 + 3 + UR._cdiv(wg, 256) + 6 + 3) * E * s
    return abs(sumsq - sum(S)) / gate


def update_gates(keys, t, lr, coef, norm, sumsq, max_norm, wd=WD, arenas=None):
    """One optimizer cycle, teacher-forced. sumsq: the f32 sum of squares the optimizer handed to its
    clip kernel, held to the f64 sum over all arenas together by sumsq_check; coef and norm are then held
    to it by update_refs.clip_coef_check, whose gates are the clip kernel's own three roundings (handing
    that check the f64 sum instead would charge the clip kernel with the summation's error: measured
    2.2 E on the norm where the check allows 2 E). arenas: {arena: [keys]} (default: by key prefix). keys: {key: dict(p0, g, m0, v0, p1, m1, v1, reached,
    step (the test's own count of the cycles that reached the key, this one included),
    opt_step (the optimizer's count after the step), opt_step0 (before it))}; t: scheduler steps so
    far; lr, coef, norm: what the optimizer used (param_groups lr, the device coefficient and norm).
    Returns ({m, v, p: worst err / gate over the reached keys}, list of failures of the exact checks)."""
    fails = []
    if arenas is None:
        arenas = {}
        for k in keys:
            arenas.setdefault(arena_of(k), []).append(k)
    ws = sumsq_check(sumsq, [torch.cat([keys[k]["g"].reshape(-1) for k in ks]) for ks in arenas.values()])
    if not ws <= 1.0:
        fails.append(f"sum of squares {sumsq!r}: err/gate {ws:.3g} against f64")
    fails += UR.clip_coef_check(sumsq, max_norm, coef, norm)
    lr_ref = cosine_lr(t)
    if not abs(lr - lr_ref) <= LR_TOL:
        fails.append(f"lr {lr!r} vs {lr_ref!r} at scheduler step {t}")
    w = {"m": 0.0, "v": 0.0, "p": 0.0}
    for k, r in keys.items():
        if not r["reached"]:
            for n in ("p", "m", "v"):
                if not torch.equal(r[n + "0"], r[n + "1"]):
                    fails.append(f"skipped key {k}: {n} moved")
            if r["opt_step"] != r["opt_step0"]:
                fails.append(f"skipped key {k}: step count {r['opt_step0']} -> {r['opt_step']}")
            continue
        if r["opt_step"] != r["step"]:
            fails.append(f"key {k}: step count {r['opt_step']}, reached in {r['step']} cycles")
        c = UR.AdamConsts(r["step"], wd, lr=lr_ref)
        wm, wv, wp = UR.adamw_gates(r["p1"], r["m1"], r["v1"], r["p0"], r["g"], r["m0"], r["v0"], c, coef)
        w = {"m": max(w["m"], wm), "v": max(w["v"], wv), "p": max(w["p"], wp)}
    return w, fails


UPDATE_MUTANTS = ("global_step", "coef_per_arena", "skipped_decays", "lr_one_late")


def arena_of(key):
    for pre, name in (("multi_modal_projector.", "projector"), ("language_model.model.embed_tokens.", "embed"),
                      ("language_model.lm_head.", "head"), ("language_model.", "layers"), ("vision_tower.", "vision")):
        if key.startswith(pre):
            return name
    raise KeyError(key)


def update_cycle_honest(state, grads, reached, t, global_step, max_norm, sdt, mutant=None, wd=WD):
    """FusedAdamW.clip_grad_norm_ + step restated on the CPU over {key: tensor} dicts. state: {key:
    dict(p, m, v, step)} (updated in place), grads: {key: bf16 accumulated gradient (0 where skipped)},
    reached: the keys with a gradient this cycle. Returns (records for update_gates, lr, coef, norm, sumsq)."""
    sumsq = UR.f32(sum((g.double() ** 2).sum().item() for g in grads.values())).item()
    coef, norm = UR.clip_coef_honest(sumsq, max_norm)
    lr = cosine_lr(t - 1 if mutant == "lr_one_late" else t)
    recs = {}
    for k, s in state.items():
        g = grads[k]
        r = dict(p0=s["p"].clone(), m0=s["m"].clone(), v0=s["v"].clone(), g=g, reached=k in reached, opt_step0=s["step"])
        if k in reached:
            s["step"] += 1
            gs = coef
            if mutant == "coef_per_arena":
                mine = sum((grads[q].double() ** 2).sum().item() for q in grads if arena_of(q) == arena_of(k))
                gs = UR.clip_coef_honest(mine, max_norm)[0]
            c = UR.AdamConsts(global_step if mutant == "global_step" else s["step"], wd, lr=lr)
            s["p"], s["m"], s["v"] = UR.adamw_honest(s["p"], g, s["m"], s["v"], c, gs)
        elif mutant == "skipped_decays":
            s["p"] = UR.adamw_p_decayed(s["p"], UR.AdamConsts(max(s["step"], 1), wd, lr=lr))
        r.update(p1=s["p"].clone(), m1=s["m"].clone(), v1=s["v"].clone(), opt_step=s["step"])
        recs[k] = r
    return recs, lr, coef, norm, sumsq
