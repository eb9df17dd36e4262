"""Restatements of the FP8 KV cache (csrc/kv_fp8.h, kv_fp8.hip, the KV_FP8 instantiation of
attn_decode_k in csrc/decode.hip) in plain torch on the CPU, with the one-line mutants that
tests/test_kv_fp8_refs_host.py shows to fail; tests/test_kv_fp8_gpu.py holds the kernels to them.

Format: per (token, head) one exponent byte e + 127, e the smallest integer with amax * 2^-e <= 448
(448 = 1.75 * 2^8, the largest e4m3fn value), clamped to e >= -100; code = e4m3fn round-to-nearest-even
of x * 2^-e; value = f32(code) * 2^e, always a bf16 number. No number here came from a kernel.
"""
import torch

from tests.decode_refs import BF, CHUNK, D_HEAD, window

E_MIN = -100
FP8 = torch.float8_e4m3fn


def pow2(e):
    """2^e as f32 for an integer tensor e"""
    return torch.ldexp(torch.ones(e.shape, dtype=torch.float32), e.to(torch.int32))


def exponent(amax, mutant=None):
    """e [..] (int32) of amax [..] (f32, finite, >= 0) from its exponent field and mantissa, in integer
    arithmetic: amax = m 2^E with 1 <= m < 2 needs 2^(E - e) m <= 1.75 * 2^8, so e = E - 8 for
    m <= 1.75 and E - 7 above. Mutants: 'exp+1', 'exp-1', 'noclamp'."""
    bits = amax.contiguous().view(torch.int32)
    E = ((bits >> 23) & 0xFF) - 127
    mant = bits & 0x7FFFFF
    e = E - 8 + (mant > 0x600000).to(torch.int32)
    if mutant == "exp+1":
        e = e + 1
    if mutant == "exp-1":
        e = e - 1
    if mutant != "noclamp":
        e = e.clamp_min(E_MIN)
    return e


def _truncate(scaled, codes):
    """e4m3 codes of `scaled` rounded toward zero: the nearest-even code stepped one code down in
    magnitude where it overshoots (codes are monotonic in magnitude)"""
    val = codes.view(FP8).float()
    over = val.abs() > scaled.abs()
    return torch.where(over, codes - 1, codes)


def quantise(x, H, D=D_HEAD, mutant=None):
    """x bf16 [..., H*D] -> (codes uint8 [..., H*D], exponent bytes uint8 [..., H]).
    Mutants: the exponent's, 'fnuz' (the gfx942 encoding: bias 8), 'trunc' (round toward zero)."""
    xh = x.float().reshape(*x.shape[:-1], H, D)
    e = exponent(xh.abs().amax(-1), mutant)
    scaled = xh * pow2(-e)[..., None]  # exact: a power of two (an underflow can only end in code 0)
    if mutant == "fnuz":
        codes = scaled.to(torch.float8_e4m3fnuz).view(torch.uint8)
    else:
        codes = scaled.to(FP8).view(torch.uint8)
    if mutant == "trunc":
        codes = _truncate(scaled, codes)
    return codes.reshape(x.shape), (e + 127).to(torch.uint8)


def dequantise_f32(codes, eb, H, D=D_HEAD):
    """f32(code) * 2^e, f32 [..., H*D] (before any rounding to bf16: the host test shows there is none)"""
    v = codes.view(FP8).float().reshape(*codes.shape[:-1], H, D)
    return (v * pow2(eb.to(torch.int32) - 127)[..., None]).reshape(codes.shape)


def dequantise(codes, eb, H, D=D_HEAD):
    return dequantise_f32(codes, eb, H, D).to(BF)


def fake_quant(x, H, D=D_HEAD, mutant=None):
    """quantise, then dequantise: what an "fp8_sim" cache holds"""
    return dequantise(*quantise(x, H, D, mutant), H, D)


def attn_fp8_honest(q, kcodes, vcodes, ke, ve, kv_start, kv_len, scale, D=D_HEAD, mutant=None):
    """attn_decode_k<KV_FP8> + attn_decode_combine_k restated in torch f32, in decode_refs.attn_honest's
    order: the scores are summed over the UNSCALED code values and multiplied by the key's 2^e once,
    p = exp2(s - m_c) is multiplied by the value's 2^e once and P.V summed over unscaled code values;
    no exponent or V row outside [kv_start, kv_len) is read. Mutants: 'k_scale_on_v' (the value's
    scale taken from the key exponents), 'scale_twice' (the key's scale applied to the score twice),
    'v_below_start' (V rows and exponents below kv_start read: only the upper bound masks them)."""
    B, L = kcodes.shape[0], kcodes.shape[1]
    H = q.shape[1] // D
    nc = -(-L // CHUNK)
    Lp = nc * CHUNK
    vis = window(kv_start, kv_len, L)
    vis_v = vis if mutant != "v_below_start" else torch.arange(L)[None, :] < kv_len[:, None]
    visp = torch.zeros(B, Lp, dtype=torch.bool)
    visp[:, :L] = vis
    one, zero = torch.ones(()), torch.zeros(())
    K = torch.zeros(B, Lp, H, D)
    V = torch.zeros(B, Lp, H, D)
    ks = torch.ones(B, Lp, H)
    vs = torch.zeros(B, Lp, H)
    K[:, :L] = torch.where(vis[:, :, None], kcodes.view(FP8).float(), zero).view(B, L, H, D)
    V[:, :L] = torch.where(vis_v[:, :, None], vcodes.view(FP8).float(), zero).view(B, L, H, D)
    ks[:, :L] = torch.where(vis[:, :, None], pow2(ke.to(torch.int32) - 127), one)
    v_exp = ke if mutant == "k_scale_on_v" else ve
    vs[:, :L] = torch.where(vis_v[:, :, None], pow2(v_exp.to(torch.int32) - 127), zero)
    qs = q.float().reshape(B, H, D) * torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    S = torch.einsum("bhd,blhd->bhl", qs, K) * ks.transpose(1, 2)
    if mutant == "scale_twice":
        S = S * ks.transpose(1, 2)
    S = S.masked_fill(~visp[:, None, :], float("-inf"))
    S = S.view(B, H, nc, CHUNK)
    mc = S.amax(-1)
    mfin = torch.where(torch.isinf(mc), torch.zeros_like(mc), mc)
    P = torch.exp2(S - mfin[..., None])
    lc = P.sum(-1)
    Ps = P * vs.transpose(1, 2).reshape(B, H, nc, CHUNK)
    oc = torch.einsum("bhck,bckhd->bhcd", Ps, V.view(B, nc, CHUNK, H, D))
    Mx = mc.amax(-1, keepdim=True)
    Mfin = torch.where(torch.isinf(Mx), torch.zeros_like(Mx), Mx)
    w = torch.where(torch.isinf(mc), torch.zeros_like(mc), torch.exp2(mc - Mfin))
    Lsum = torch.zeros(B, H)
    acc = torch.zeros(B, H, D)
    for c in range(nc):  # chunk order, as the combine kernel
        Lsum = Lsum + w[:, :, c] * lc[:, :, c]
        acc = acc + w[:, :, c, None] * oc[:, :, c]
    o = torch.where(Lsum[..., None] > 0, acc / Lsum.clamp_min(1e-37)[..., None], zero)
    return o.reshape(B, H * D).to(BF)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
H_TEST, B_TEST = 2, 3
POISON_CODE, POISON_EXP = 0x7F, 255  # e4m3fn NaN; 2^128


def append_rows(Lnew, B=B_TEST, H=H_TEST, D=D_HEAD, seed=0):
    """k, v bf16 [B*Lnew, H*D], unit normal, with the quantiser's edge cases planted in the first
    new row of each sequence (so every Lnew has them): a head scaled by 2^-30 and one by 2^20; an
    all-zero head; a head whose amax is 14 = 1.75 * 2^3 exactly (e = -5) holding 17/32 and 19/32, which
    scale to 17 and 19 -- ties between the e4m3 neighbours 16 | 18 | 20, resolved to the even
    mantissas 16 and 20; a head whose amax is the next bf16 above, 14.0625 (e = -4)."""
    g = torch.Generator().manual_seed(1000 + seed + Lnew)
    k = torch.randn(B * Lnew, H, D, generator=g)
    v = torch.randn(B * Lnew, H, D, generator=g)
    for x in (k, v):
        x[0, 0] *= 2.0 ** -30
        x[0, 1] *= 2.0 ** 20
        x[Lnew, 0] = 0.0
        x[Lnew, 1].clamp_(-3, 3)
        x[Lnew, 1, 5], x[Lnew, 1, 6], x[Lnew, 1, 7], x[Lnew, 1, 8] = 14.0, 17.0 / 32, 19.0 / 32, -17.0 / 32
        x[2 * Lnew, 0].clamp_(-3, 3)
        x[2 * Lnew, 0, 9], x[2 * Lnew, 0, 10] = -14.0625, 17.0 / 32
    return k.reshape(B * Lnew, H * D).to(BF), v.reshape(B * Lnew, H * D).to(BF)


def poison_outside(kcodes, vcodes, ke, ve, vis):
    """copies with every row outside the window poisoned: codes e4m3 NaN, exponent byte 255"""
    out = ~vis
    kc, vc, ke2, ve2 = kcodes.clone(), vcodes.clone(), ke.clone(), ve.clone()
    kc[out], vc[out] = POISON_CODE, POISON_CODE
    ke2[out], ve2[out] = POISON_EXP, POISON_EXP
    return kc, vc, ke2, ve2


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()
