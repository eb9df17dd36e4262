"""tests/layer_refs.py on the CPU, for the very inputs of its case tables: the exact reference and the
emulation are what they claim, a second, independent emulation passes every gate at the module's margin,
every one-line mutant of the emulated layer fails a gate (two that cannot are shown to pass), and a single
scaled row passes the whole-tensor rel-L2 gates of tests/test_model_gpu.py (the blind spot the per-row
gates close).
"""
import functools

import pytest
import torch

from tests import layer_refs as LR
from tests.layer_refs import Mode

D = lambda t: t.double()  # noqa: E731
_seen_ratios = []


@functools.lru_cache(maxsize=None)
def _decoder(name, kind, mutant=None, layer=0):
    g, h, dh3 = LR.decoder_case(name)
    return LR.decoder_layer(D(h), D(dh3), LR.lm_layer_weights(layer), g, Mode(kind, mutant))


def _decoder_gate(name, got):
    g = LR.decoder_case(name)[0]
    return LR.gate(got, _decoder(name, "emu"), _decoder(name, "exact"), zero_rows=g.zero_rows)


@pytest.mark.parametrize("name", list(LR.DECODER_CASES))
def test_decoder_second_emulation_passes(name):
    recs, fails = _decoder_gate(name, _decoder(name, "emu2"))
    _seen_ratios.extend(r["ratio"] for r in recs)
    print(name, {r["figure"]: f"{r['emulated']:.2e} x{r['ratio']:.2f}" for r in recs})
    assert not fails, fails
    recs, fails = _decoder_gate(name, _decoder(name, "emu"))   # the emulation itself: ratio 1 everywhere
    assert not fails and all(r["ratio"] == 1.0 for r in recs)


@pytest.mark.parametrize("name", list(LR.DECODER_CASES))
def test_decoder_no_row_is_excluded(name):
    """the exact reference has no zero row but the rows that must come back exactly zero, and the
    emulation keeps those exactly zero"""
    g = LR.decoder_case(name)[0]
    ex, emu = _decoder(name, "exact"), _decoder(name, "emu")
    assert LR.no_zero_reference_rows(ex, list(ex), g.zero_rows) == []
    for k, z in g.zero_rows.items():
        assert (ex[k][z] == 0).all() and (emu[k][z] == 0).all()
    assert g.pad_rows.sum() == (5 if "packed" in name else 0)
    if g.tail is not None:   # 2 padding slots; grid-left: the 7 + 71 rows no supervised row sees
        assert g.zero_rows["h3"].sum() == 2 and g.zero_rows["dh"].sum() == (78 if "grid" in name else 5)


def test_left_padded_sequence_with_one_live_key():
    g = LR.decoder_case("grid-left")[0]
    live = g.live()
    sees = live.any(-1).view(3, 72)
    assert sees[0].all() and sees[1].tolist() == [False] * 7 + [True] * 65 and sees[2].tolist() == [False] * 71 + [True]
    assert g.positions().view(3, 72)[1, 7] == 0 and g.positions().view(3, 72)[2, 71] == 0


def test_exact_attention_is_plain_autograd():
    """_Attn in its exact mode against torch autograd through a masked softmax (grid-right: every query
    sees a key, so the plain form has no NaN to work around)"""
    g = LR.decoder_case("grid-right")[0]
    T, d, H = g.Tp, LR.LM["d"], LR.LM["H"]
    gen = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(T, d, generator=gen, dtype=torch.float64) for _ in range(4))
    grads = []
    for fn in (lambda *a: LR.attention(*a, Mode("exact")), LR.attention_autograd):
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = fn(qq, kk, vv, g.live(), 128 ** -0.5, H)
        o.backward(do)
        grads.append((o.detach(), qq.grad, kk.grad, vv.grad))
    for a, b in zip(*grads):
        assert (a - b).abs().max() <= 1e-12 * b.abs().max()


def test_emulated_delta_takes_the_rounded_o():
    """_Attn's emulated backward against the same backward with delta from the unrounded O (what plain
    autograd through the softmax amounts to): dQ and dK differ, dV, which delta does not enter, does not"""
    g = LR.decoder_case("grid-long")[0]
    gen = torch.Generator().manual_seed(6)
    q, k, v, do = (LR.bf(torch.randn(g.Tp, LR.LM["d"], generator=gen, dtype=torch.float64)) for _ in range(4))
    res = []
    for mutant in (None, "delta_from_exact_o"):
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        LR.attention(qq, kk, vv, g.live(), 128 ** -0.5, LR.LM["H"], Mode("emu", mutant)).backward(do)
        res.append((qq.grad, kk.grad, vv.grad))
    assert not torch.equal(res[0][0], res[1][0]) and not torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("mutant,cases", list(LR.DECODER_MUTANTS.items()))
def test_decoder_mutants_fail(mutant, cases):
    failed = []
    for name in cases:
        recs, fails = _decoder_gate(name, _decoder(name, "emu", mutant))
        if fails:
            failed.append(name)
        print(mutant, name, sorted(((r["ratio"], r["figure"]) for r in recs), reverse=True)[:2])
    assert failed, f"mutant {mutant} passes every gate in {cases}"


@pytest.mark.parametrize("mutant,cases", list(LR.EQUIVALENT_MUTANTS.items()))
def test_equivalent_mutants_pass(mutant, cases):
    """layer_refs.EQUIVALENT_MUTANTS: a shift of every live position of a sequence is invisible to one
    layer (RoPE is relative); the mutant moves the figures by rounding only and passes every gate"""
    for name in cases:
        recs, fails = _decoder_gate(name, _decoder(name, "emu", mutant))
        assert not fails and max(r["ratio"] for r in recs) > 1.0 - 1e-9, fails
        if mutant == "grid_positions":   # not a no-op: the roundings move
            assert not torch.equal(_decoder(name, "emu", mutant)["dh"], _decoder(name, "emu")["dh"])
    if mutant == "tail_dw_gathered":   # in f32 accumulation the order shows, and still passes
        for name in cases:
            a, b = _decoder(name, "emu2", mutant), _decoder(name, "emu2")
            assert not torch.equal(a["wgu"], b["wgu"]) or not torch.equal(a["wd"], b["wd"])
            assert not _decoder_gate(name, a)[1]


@pytest.mark.parametrize("mutant", ["dh_row_zeroed", "dh_row_scaled", "h3_row_scaled"])
@pytest.mark.parametrize("name", ["grid-left", "packed"])
def test_blind_spot_single_row_against_whole_tensor_gates(name, mutant):
    """The reason the per-row gates exist: one wrong row of dh or h3 fails the row gate, while a
    whole-tensor rel-L2 dilutes it by sqrt(rows). A row scaled by 1.1 (h3, or dh) passes the gates of
    tests/test_model_gpu.py (1e-2 on activations, check_grads' 2e-2) as a whole tensor. A row of dh zeroed
    outright sits at 1 / sqrt(rows) = 5e-2 at the 216 and 259 rows of these cases: over 2e-2 had dh
    ever been compared with anything, which before this module it was not. The headroom of the scaled rows
    is thin, 8.2e-3 .. 8.8e-3 against 1e-2 for h3, and most of that is the bf16 noise of the other rows
    (0.1 / sqrt(216) = 6.8e-3 is the row's own share)."""
    ex, mut = _decoder(name, "exact"), _decoder(name, "emu", mutant)
    key = mutant[:2]
    _, fails = _decoder_gate(name, mut)
    assert any(f.startswith(key + ".row") for f in fails), fails
    whole = LR.whole_rel_l2(mut[key], ex[key])
    rows = ex[key].shape[0] - int(LR.decoder_case(name)[0].pad_rows.sum())
    print(name, mutant, f"whole-tensor rel-L2 {whole:.2e} over {rows} rows")
    if mutant == "dh_row_zeroed":
        assert 0.5 / rows ** 0.5 <= whole <= 2.0 / rows ** 0.5
    else:
        assert whole <= (1e-2 if key == "h3" else 2e-2)


# ---- LoRA cases ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lora(name, kind, mutant=None):
    g, h, dh3 = LR.decoder_case(LR.LORA_CASES[name][0])
    return LR.decoder_layer(D(h), D(dh3), LR.lm_layer_weights(0), g, Mode(kind, mutant),
                            lora=LR.lora_case_groups(name, 0, mutant=mutant))


def _lora_gate(name, got):
    g = LR.decoder_case(LR.LORA_CASES[name][0])[0]
    return LR.gate(got, _lora(name, "emu"), _lora(name, "exact"), keys=LR.LORA_KEYS, zero_rows=g.zero_rows)


@pytest.mark.parametrize("name", list(LR.LORA_CASES))
def test_lora_second_emulation_passes(name):
    recs, fails = _lora_gate(name, _lora(name, "emu2"))
    _seen_ratios.extend(r["ratio"] for r in recs)
    assert not fails, fails
    ex = _lora(name, "exact")
    g = LR.decoder_case(LR.LORA_CASES[name][0])[0]
    assert LR.no_zero_reference_rows(ex, LR.LORA_KEYS, g.zero_rows) == []
    # the adapters matter: the output is not the base layer's
    assert LR.row_fig(ex["h3"], _decoder(LR.LORA_CASES[name][0], "exact")["h3"]) > 0.05


@pytest.mark.parametrize("mutant,cases", list(LR.LORA_MUTANTS.items()))
def test_lora_mutants_fail(mutant, cases):
    for name in cases:
        recs, fails = _lora_gate(name, _lora(name, "emu", mutant))
        print(mutant, name, sorted(((r["ratio"], r["figure"]) for r in recs), reverse=True)[:2])
        assert fails, mutant


def test_module_seed_restated():
    assert LR.module_seed(1234, 3, 1) == ((lambda x: ((x ^ (x >> 31)) * 0x94D049BB133111EB) & LR._M64)(
        (1234 * 0x9E3779B97F4A7C15 + 26 * 0xBF58476D1CE4E5B9) & LR._M64))


# ---- CLIP, projector, head ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clip(name, kind, mutant=None):
    h, dh3 = LR.clip_case(name)
    return LR.clip_layer(D(h), D(dh3), LR.clip_layer_weights(0), LR.CLIP_CASES[name]["B"], Mode(kind, mutant))


@pytest.mark.parametrize("name", list(LR.CLIP_CASES))
def test_clip_second_emulation_passes_and_mutants_fail(name):
    ex, emu = _clip(name, "exact"), _clip(name, "emu")
    assert LR.no_zero_reference_rows(ex, list(ex)) == []
    recs, fails = LR.gate(_clip(name, "emu2"), emu, ex)
    _seen_ratios.extend(r["ratio"] for r in recs)
    assert not fails, fails
    for mutant in ("clip_erf_gelu", "clip_no_qkv_bias_grad"):
        assert LR.gate(_clip(name, "emu", mutant), emu, ex)[1], mutant


@functools.lru_cache(maxsize=None)
def _proj(rows, kind, mutant=None):
    x, dy = LR.projector_case(rows)
    return LR.projector(D(x), D(dy), LR.projector_weights(), Mode(kind, mutant))


@pytest.mark.parametrize("rows", LR.PROJECTOR_ROWS)
def test_projector_second_emulation_passes_and_mutant_fails(rows):
    ex, emu = _proj(rows, "exact"), _proj(rows, "emu")
    assert LR.no_zero_reference_rows(ex, list(ex)) == []
    exact_keys = ("b2",) if rows == 1 else ()   # one row: the bias gradient is that row of dy, bitwise
    recs, fails = LR.gate(_proj(rows, "emu2"), emu, ex, exact_keys=exact_keys)
    _seen_ratios.extend(r["ratio"] for r in recs)
    assert not fails, fails
    assert LR.gate(_proj(rows, "emu", "proj_quick_gelu"), emu, ex)[1]


HEAD_KEYS = ("logits", "dh", "n", "w")


@functools.lru_cache(maxsize=None)
def _head(name, kind, mutant=None, with_dlogits=False):
    h, labels, mask, dlog = LR.head_case(name)
    return LR.head(D(h), labels, mask, LR.head_weights(), Mode(kind, mutant), D(dlog) if with_dlogits else None)


@pytest.mark.parametrize("with_dlogits", [False, True])
@pytest.mark.parametrize("name", ["rows8", "rows24", "one-row"])
def test_head_second_emulation_passes_and_mutants_fail(name, with_dlogits):
    ex, emu, emu2 = (_head(name, k, None, with_dlogits) for k in ("exact", "emu", "emu2"))
    sup = ex["sup"]
    assert ex["count"] == sum(LR.HEAD_CASES[name]["sup"]) == int(sup.sum())
    if not with_dlogits:   # rows without a label: an exact zero gradient, in the reference and the emulation
        assert (ex["dh"][~sup] == 0).all() and (emu["dh"][~sup] == 0).all()
        assert LR.no_zero_reference_rows(ex, ["logits", "w"]) == [] and (ex["dh"][sup].norm(dim=-1) > 0).all()
    recs, fails = LR.gate(emu2, emu, ex, keys=HEAD_KEYS)
    _seen_ratios.extend(r["ratio"] for r in recs)
    assert not fails, fails
    assert abs(LR.f32_sum(emu["row_loss"]) / emu["count"] - emu["loss"]) <= LR.LOSS_GATE * abs(emu["loss"])
    for mutant in ("head_unshifted", "head_mean_all_rows"):
        mut = _head(name, "emu", mutant, with_dlogits)
        _, fails = LR.gate(mut, emu, ex, keys=HEAD_KEYS)
        loss_off = abs(mut["loss"] - emu["loss"]) > LR.LOSS_GATE * abs(emu["loss"])
        assert fails and loss_off, mutant


def test_head_with_every_row_ignored():
    """what the reference gives with no supervised row: loss NaN (the mean of an empty selection, as
    torch's CrossEntropyLoss) and every gradient exactly zero"""
    for kind in ("exact", "emu"):
        r = _head("all-ignored", kind)
        assert r["count"] == 0 and r["loss"] != r["loss"]
        assert all((r[k] == 0).all() for k in ("dh", "n", "w"))


def test_row_movers_are_a_gather_and_its_transpose():
    rows = torch.tensor(LR.MOVER_ROWS)
    x = torch.randn(LR.MOVER_FULL, 5, dtype=torch.float64)
    y = torch.randn(rows.numel(), 5, dtype=torch.float64)
    # <gather(x), y> == <x, scatter(y)>: scatter is the transpose of gather
    assert torch.equal((LR.gather_rows(x, rows) * y).sum(), (x * LR.scatter_rows(y, rows, LR.MOVER_FULL)).sum()) or \
        abs(float((LR.gather_rows(x, rows) * y).sum() - (x * LR.scatter_rows(y, rows, LR.MOVER_FULL)).sum())) < 1e-12
    assert (LR.gather_rows(x, rows)[rows < 0] == 0).all()
    assert (LR.scatter_rows(y, rows, LR.MOVER_FULL)[1] == 0).all()


def test_zz_margin_covers_the_second_emulation():
    """the spread of emu2 / emu over everything gated above (the range the module docstring quotes)"""
    if not _seen_ratios:   # run on its own: one case stands for the module
        _seen_ratios.extend(r["ratio"] for r in _decoder_gate("grid-long", _decoder("grid-long", "emu2"))[0])
    r = [x for x in _seen_ratios if x > 0]   # 0: an exactly representable tensor
    print(f"emu2 / emu over {len(r)} figures: {min(r):.2f} .. {max(r):.2f}")
    assert max(_seen_ratios) <= LR.M
