"""The FP8 KV cache's restatements (tests/kv_fp8_refs.py) shown on the CPU, on the inputs of
tests/test_kv_fp8_gpu.py: the quantiser's dequantised values are bf16 numbers exactly, its exponent
is the smallest that fits, the fp8-order attention restatement equals the bf16-order one
(decode_refs.attn_honest) on the dequantised cache bit for bit -- and each one-line mutant fails one
of those checks on the same inputs.
"""
import pytest
import torch

from tests import decode_refs as R
from tests import kv_fp8_refs as F

H, D = F.H_TEST, R.D_HEAD
SCALE = D ** -0.5
QUANT_MUTANTS = ["exp+1", "exp-1", "noclamp", "fnuz", "trunc"]
ATTN_MUTANTS = ["k_scale_on_v", "scale_twice", "v_below_start"]


def bits(t):
    return t.contiguous().view(torch.int16)


def _rows():
    return torch.cat([torch.cat(F.append_rows(L), 0) for L in (1, 5, 70)], 0)


def quantiser_ok(x, mutant=None):
    """every property the format states, on rows x [n, H*D] bf16: the scaled amax fits 448 and would
    not with e - 1 (unless clamped); e >= -100; the dequantised values are finite and exactly bf16;
    the codes are the nearest e4m3 value (error at most half a step, ties to the even mantissa)"""
    codes, eb = F.quantise(x, H, D, mutant)
    e = eb.to(torch.int32) - 127
    xh = x.double().reshape(-1, H, D)
    amax = xh.abs().amax(-1)
    fits = bool((amax * 2.0 ** (-e.double()) <= 448).all())
    smallest = bool(((amax * 2.0 ** (-(e.double() - 1)) > 448) | (e == F.E_MIN)).all())
    clamped = bool((e >= F.E_MIN).all())
    deq32 = F.dequantise_f32(codes, eb, H, D)
    exact = bool(torch.isfinite(deq32).all()) and torch.equal(deq32.to(R.BF).float(), deq32)
    # nearest: no other e4m3 value is closer to the scaled input; on a tie the code's low bit is 0
    grid = torch.arange(256, dtype=torch.uint8).view(F.FP8).double()
    grid = grid[torch.isfinite(grid)].unique()
    scaled = xh * 2.0 ** (-e.double())[..., None]
    val = codes.view(F.FP8).double().reshape(-1, H, D)
    dist = (grid[None, None, None, :] - scaled[..., None]).abs()
    best = dist.amin(-1)
    nearest = bool(((val - scaled).abs() == best).all())
    tie = (dist == best[..., None]).sum(-1) > 1
    even = bool(((codes.reshape(-1, H, D)[tie] & 1) == 0).all())
    return dict(fits=fits, smallest=smallest, clamped=clamped, exact=exact, nearest=nearest and even)


def test_quantiser_properties_hold():
    x = _rows()
    res = quantiser_ok(x)
    assert all(res.values()), res
    # the planted edges did what they were planted for (Lnew = 1 block: rows 0, 1, 2)
    codes, eb = F.quantise(x[:3], H, D)
    e = eb.to(torch.int32) - 127
    assert e[1, 0] == F.E_MIN and int(codes[1, :D].max()) == 0           # all-zero head: clamp, codes 0
    assert e[1, 1] == -5 and e[2, 0] == -4                               # amax 14 | 14.0625
    row = codes[1, D:].view(F.FP8).float()
    assert row[5] == 448 and row[6] == 16 and row[7] == 20 and row[8] == -16  # ties to even
    assert e[0, 0] < -30 and e[0, 1] > 10


@pytest.mark.parametrize("mutant", QUANT_MUTANTS)
def test_quantiser_mutants_fail(mutant):
    res = quantiser_ok(_rows(), mutant)
    print(mutant, res)
    assert not all(res.values()), res


def test_quantiser_mutants_change_codes():
    """the GPU test compares codes and exponents bit for bit: every mutant changes one of them"""
    x = _rows()
    codes, eb = F.quantise(x, H, D)
    for mutant in QUANT_MUTANTS:
        c2, e2 = F.quantise(x, H, D, mutant)
        assert not (torch.equal(codes, c2) and torch.equal(eb, e2)), mutant


def _attn_case(name):
    max_len, pairs = R.ATTN_CASES[name]
    B = len(pairs)
    q, kc, vc = R.attn_inputs(name, max_len, B, H=H)
    ks = torch.tensor([p[0] for p in pairs], dtype=torch.int32)
    kl = torch.tensor([p[1] for p in pairs], dtype=torch.int32)
    kcodes, ke = F.quantise(kc.contiguous(), H, D)
    vcodes, ve = F.quantise(vc.contiguous(), H, D)
    return q, kcodes, vcodes, ke, ve, ks, kl


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attn_restatement_equals_bf16_order_on_dequantised(name):
    q, kcodes, vcodes, ke, ve, ks, kl = _attn_case(name)
    kd, vd = F.dequantise(kcodes, ke, H, D), F.dequantise(vcodes, ve, H, D)
    want = R.attn_honest(q, kd, vd, ks, kl, SCALE)
    vis = R.window(ks, kl, kcodes.shape[1])
    pk, pv, pke, pve = F.poison_outside(kcodes, vcodes, ke, ve, vis)
    got = F.attn_fp8_honest(q, pk, pv, pke, pve, ks, kl, SCALE)
    assert torch.equal(bits(got), bits(want))
    empty = kl <= ks
    assert bool((got[empty].float() == 0).all())
    if name == "starts576":  # a case with rows below kv_start: every mutant is visible there
        for mutant in ATTN_MUTANTS:
            bad = F.attn_fp8_honest(q, pk, pv, pke, pve, ks, kl, SCALE, mutant=mutant)
            assert not torch.equal(bits(bad), bits(want)), mutant
