"""References, bf16 emulations, figures, gates and case tables for the layer functions of functions.py
(LlamaLayerFn, ClipLayerFn, ProjectorFn, HeadLossFn, HeadLossRowsFn and the row movers): the code that
wires the kernels into a layer. Every kernel is pinned on its own elsewhere; what is gated here is the
wiring, per row, so that one wrong row cannot average out of a whole-tensor norm.
Plain torch on whatever device the tensors live on, nothing of the GPU library is imported:
tests/test_layer_refs_host.py proves on the CPU that the gates pass two honest emulations and fail a set
of one-line mutants, tests/test_layer_accuracy_gpu.py then holds the layers to the same gates.

Exact reference: the layer in float64 end to end (RoPE tables in f64, softmax over live keys only, a
query with no live key gives O = 0), torch autograd for the backward. The attention is one hand-written
Function (forward and FA2-form backward) shared by the exact and the emulated mode; the host test holds
its exact mode to plain autograd through a masked softmax.

bf16 emulation ("emu"): the same arithmetic in f64 on the same inputs, rounded to bf16 where the kernels
store a bf16 tensor. _R rounds its output in the forward and its gradient in the backward, so every stored
forward tensor (x1, qkv, rotated q|k, o, h2, x2, gu, a, h3; CLIP: also pre; head: logits) and the gradient
of every one of them (dx1, dqkv before and after the inverse RoPE, do, dh2, dx2, dgu, da, dh; dlogits) is
rounded once. A GEMM epilogue rounds before it adds a residual and before it applies an activation. The RMSNorm rounds x * rstd before the weight (forward only), RoPE takes bf16 cos / sin and
rounds both products (forward only), the activation backward reads the stored bf16 pre-activation. The
attention backward is FA2's: P and dS rounded to bf16 and delta = rowsum(dO * O) from the ROUNDED O.
Weight gradients are f64 sums of the rounded operands, rounded to bf16 once (the arena's type).
"emu2" is a second, independent emulation: every product accumulates in f32 (torch's own order), and the
attention forward rounds the unnormalised P = exp(S - max) before P V and divides by the f64 row sum
afterwards (the kernels' deferred rescale). It must pass the gates of "emu" as a correct layer must.
Neither emulation reads a kernel's output; their distance from the exact reference is the floor the
number formats put under a correct layer.

Figures (one definition, both test files):
  row     [rows, cols] activations, activation gradients and weight gradients (rows: output features):
          max_t |X_t - R_t|_2 / (|R_t|_2 + FLOOR rms(R) sqrt(cols)), FLOOR of tests/train_refs.py: a
          zero reference row demands an exact zero, no row is excluded;
  block   weight gradients of a fused slot: rel-L2 per block (q, k, v of qkv; gate, up of gate|up);
  elem    vector gradients (norm weights, biases): max |err| / (|ref| + rms(ref));
  zeros   exactly 0: h3 / dh of the packed padding rows, dh of rows HeadLossRowsFn does not supervise;
  finite  every element; sanity: every worst figure is finite and > 0 (a comparison that compared
          nothing fails).
Gate: figure(layer) <= M x figure(emu) for the same tensor and case, one margin M for the module.

M = 2.0, the ceiling the gate rule allows. What M has to cover is what "emu" leaves out (f32 accumulation
order, split-K, exp2, the deferred rescale) and the sampling spread of a maximum over a few hundred rows
or elements: two correct roundings of the same tensor differ in which elements flip, so the worst row of
one is not the worst row of the other. Measured ratio figure / emulated figure:
  on the CPU, the second emulation against the first: 0.68 .. 1.81 over the 193 figures of the tables
  (test_layer_refs_host.py prints the range and asserts it under M);
  on the MI355X (profiles/r23/layers/layer_stats.jsonl, 385 lines): decoder layer 0.80 .. 1.40, with
  adapters 0.82 .. 1.17, CLIP layer 1.00 .. 1.09, with adapters 0.87 .. 1.12, with a trainable tower
  0.64 .. 1.94 (the largest: the layer_norm2 weight gradient at 3 x 257 rows, a maximum over 128
  elements of one bf16 store each; every 2-D tensor of that case is within 1.20), projector and head 1.00
  throughout: at K = 128 .. 256 a product of bf16 values is exact in f32 and the f32 accumulation error
  almost never reaches a bf16 rounding boundary, so those kernels land on the emulation's bits.
A margin of 1.3, the rel-L2 margin of tests/test_attention_masks_gpu.py, would fail correct code on both
machines; 2.0 is the ceiling and holds. Every mutant fails at 2.0 by a wide margin: the nearest, a single
row of dh scaled by 1.1, sits at 10 x its emulated figure (5 x the gate), a zeroed row at 100 x, the
packed dropout mask keyed by the grid row at 38 x, every other wiring mutant at 70 x or more.
Mutants: the 21 of the list this module was written to, under these names -- DECODER_MUTANTS (1-4, 6-11,
20, 21, the two forms of 2 counted once; plus dh_row_scaled, which is not of the list: the blind-spot
test needs it), LORA_MUTANTS (13, 14), the CLIP (15, 16), projector (17) and head (18, 19) mutants named in
their layer functions: 19 listed mutants that must fail. Two listed mutants are expected to pass and are
tested as passing (EQUIVALENT_MUTANTS): 12, the tail's dW operands gathered instead of scattered (a
summation order), and 5, RoPE positions taken from the grid index on a left-padded row (RoPE is relative,
one layer cannot see a per-sequence shift).

LoRA: y = base + B(A(mask o x / (1 - p))) scaling per module, the keep mask from oracle.lora_keep_mask
under the module seed of (step seed, layer, group, module), keyed by the row the layer sees. Emulated
roundings: the staged operand bf16(x / (1 - p)), u, the term (stored in bf16 unless the base GEMM adds it in
its epilogue), round(round(base) + term), du, and the adapters' share of dx added to the stored base dx
(rounded after every module under dropout). The base weights are frozen in these cases, as in the model's
lora policy, so their gradients are not written and not compared.

Inputs: seeded randn, h at rms 0.5 (the token embeddings' scale in oracle.make_weights, what layer 0 is
fed), upstream gradients at rms 2^-10, non-zero in padded rows of the grid too. No number here was taken
from a kernel's output.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from oracle import cullavo_oracle as O
from tests.train_refs import FLOOR

BF, F64 = torch.bfloat16, torch.float64
M = 2.0
H_RMS, G_RMS = 0.5, 2.0 ** -10
IGNORE = -100
WEIGHT_SEED = 2
CFG = O.config_small_gpu()
LM = dict(d=256, H=2, D=128, F=688, V=1024, eps=CFG.text.rms_norm_eps, theta=CFG.text.rope_theta)
VIT = dict(d=128, H=2, D=64, F=512, T=257, eps=CFG.vision.layer_norm_eps)
assert (CFG.text.hidden_size, CFG.text.intermediate_size, CFG.text.vocab_size) == (LM["d"], LM["F"], LM["V"])
assert (CFG.vision.hidden_size, CFG.vision.intermediate_size, CFG.vision.num_patches + 1) == (VIT["d"], VIT["F"], VIT["T"])


# ---------------------------------------------------------------------------------------------
# rounding
# ---------------------------------------------------------------------------------------------
def bf(x):
    """one bf16 round-to-nearest-even of an f64 tensor, back in f64"""
    return x.to(BF).to(x.dtype)


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return bf(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf(g) if ctx.bwd else g), None, None


class _GradMod(torch.autograd.Function):
    """identity in the forward, fn(gradient) in the backward (the mutants' handle on the backward wiring)"""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return ctx.fn(g), None


class Mode:
    """exact | emu | emu2 (module docstring), and the mutant (or None) applied to the emulated layer"""

    def __init__(self, kind="exact", mutant=None):
        assert kind in ("exact", "emu", "emu2")
        self.kind, self.mutant, self.emu = kind, mutant, kind != "exact"

    def R(self, x):     # a stored bf16 tensor: rounded, and its gradient rounded
        return _Round.apply(x, True, True) if self.emu else x

    def Rf(self, x):    # rounded in the forward only
        return _Round.apply(x, True, False) if self.emu else x

    def Rb(self, x):    # gradient rounded only
        return _Round.apply(x, False, True) if self.emu else x

    def lin(self, x, w, b=None):
        if self.kind == "emu2":  # f32 accumulation, torch's own summation order
            return F.linear(x.float(), w.float(), None if b is None else b.float()).double()
        return F.linear(x, w, b)

    def is_(self, name):
        return self.mutant == name


# ---------------------------------------------------------------------------------------------
# pieces
# ---------------------------------------------------------------------------------------------
def rmsnorm(x, w, eps, md):
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return md.R(w * md.Rf(x * rstd))


def layernorm(x, w, b, eps, md):
    return md.R(F.layer_norm(x, (x.shape[-1],), w, b, eps))


def rope_tables(pos, D, theta, md):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=F64, device=pos.device) / D))
    ang = pos.double()[:, None] * inv
    c, s = ang.cos(), ang.sin()
    return (bf(c), bf(s)) if md.emu else (c, s)


def rope(x, c, s, H, md, inverse=False):
    """x [T, H*D]; forward: rnd(rnd(x cos) + rnd(rotate_half(x) sin)); inverse: the transposed rotation"""
    T = x.shape[0]
    xv = x.view(T, H, -1)
    half = xv.shape[-1] // 2
    x1, x2 = xv[..., :half], xv[..., half:]
    c, s = c[:, None], s[:, None]
    if inverse:
        return torch.cat((x1 * c + x2 * s, x2 * c - x1 * s), -1).reshape(x.shape)
    o1 = md.Rf(md.Rf(x1 * c) + md.Rf(-x2 * s))
    o2 = md.Rf(md.Rf(x2 * c) + md.Rf(x1 * s))
    return torch.cat((o1, o2), -1).reshape(x.shape)


class _Attn(torch.autograd.Function):
    """attention of [T, H*D] q, k, v under live [T, T] (query i sees key j); FA2-form backward"""

    @staticmethod
    def forward(ctx, q, k, v, live, scale, H, md):
        T = q.shape[0]
        Q, K, V = (x.view(T, H, -1).transpose(0, 1) for x in (q, k, v))
        S = (Q @ K.transpose(-1, -2)) * scale
        S = S.masked_fill(~live[None], float("-inf"))
        lse = torch.logsumexp(S, -1, keepdim=True)
        P = torch.nan_to_num(torch.exp(S - lse), nan=0.0)
        if md.kind == "emu2":
            mx = torch.nan_to_num(S.max(-1, keepdim=True).values, neginf=0.0)
            Pt = torch.exp(S - mx)
            Of = (bf(Pt) @ V) / Pt.sum(-1, keepdim=True).clamp_min(1e-300)
        else:
            Of = (bf(P) if md.emu else P) @ V
        Of = bf(Of) if md.emu else Of
        if md.is_("delta_from_exact_o"):   # the host test's foil: delta as plain autograd would have it
            Ofs = P @ V
            ctx.save_for_backward(Q, K, V, P, Ofs)
        else:
            ctx.save_for_backward(Q, K, V, P, Of)
        ctx.scale, ctx.md = scale, md
        return Of.transpose(0, 1).reshape(T, -1)

    @staticmethod
    def backward(ctx, do):
        Q, K, V, P, Of = ctx.saved_tensors
        md, scale = ctx.md, ctx.scale
        r = bf if md.emu else (lambda t: t)
        H, T = Q.shape[0], Q.shape[1]
        dO = r(do).view(T, H, -1).transpose(0, 1)
        delta = (dO * Of).sum(-1, keepdim=True)
        dS = r(P * (dO @ V.transpose(-1, -2) - delta))
        dQ = dS @ K * scale
        dK = dS.transpose(-1, -2) @ Q * (1.0 if md.is_("dk_no_scale") else scale)
        dV = r(P).transpose(-1, -2) @ dO
        flat = lambda t: r(t.transpose(0, 1).reshape(T, -1))  # noqa: E731
        return flat(dQ), flat(dK), flat(dV), None, None, None, None


def attention(q, k, v, live, scale, H, md):
    return _Attn.apply(q, k, v, live, scale, H, md)


def attention_autograd(q, k, v, live, scale, H):
    """plain f64 autograd through a masked softmax (rows with a live key only): what _Attn's exact mode
    is held to in the host test"""
    T = q.shape[0]
    Q, K, V = (x.view(T, H, -1).transpose(0, 1) for x in (q, k, v))
    S = ((Q @ K.transpose(-1, -2)) * scale).masked_fill(~live[None], float("-inf"))
    return (torch.softmax(S, -1) @ V).transpose(0, 1).reshape(T, -1)


def _act(v, kind):
    if kind == "quick_gelu":
        return v * torch.sigmoid(1.702 * v)
    assert kind == "gelu"
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


# ---------------------------------------------------------------------------------------------
# inputs and weights
# ---------------------------------------------------------------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _randn(name, rows, cols, rms):
    """bf16 values, [rows, cols], made on the CPU (the same bits wherever the test runs)"""
    return (torch.randn(rows, cols, generator=_gen(name)) * rms).to(BF)


@functools.lru_cache(maxsize=None)
def weights():
    """{key: bf16 tensor} of the tiny model (oracle.make_weights at WEIGHT_SEED, the bf16 cast)"""
    return O.to_bf16(O.make_weights(CFG, WEIGHT_SEED))


def lm_layer_weights(i, W=None, device="cpu"):
    W = weights() if W is None else W
    p = f"language_model.model.layers.{i}."
    g = lambda k: W[p + k].detach().to(device).double()  # noqa: E731
    return {"wqkv": torch.cat([g(f"self_attn.{n}_proj.weight") for n in "qkv"]), "wo": g("self_attn.o_proj.weight"),
            "wgu": torch.cat([g("mlp.gate_proj.weight"), g("mlp.up_proj.weight")]), "wd": g("mlp.down_proj.weight"),
            "n1": g("input_layernorm.weight"), "n2": g("post_attention_layernorm.weight")}


LM_GRAD_KEYS = {"wqkv": ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"),
                "wo": ("self_attn.o_proj.weight",), "wgu": ("mlp.gate_proj.weight", "mlp.up_proj.weight"),
                "wd": ("mlp.down_proj.weight",), "n1": ("input_layernorm.weight",),
                "n2": ("post_attention_layernorm.weight",)}
BLOCKS = {"wqkv": 3, "wgu": 2}   # fused slots: equal blocks along the output features


def clip_layer_weights(i, W=None, device="cpu"):
    W = weights() if W is None else W
    p = f"vision_tower.vision_model.encoder.layers.{i}."
    g = lambda k: W[p + k].detach().to(device).double()  # noqa: E731
    out = {"wqkv": torch.cat([g(f"self_attn.{n}_proj.weight") for n in "qkv"]),
           "bqkv": torch.cat([g(f"self_attn.{n}_proj.bias") for n in "qkv"])}
    for nm, k in (("wo", "self_attn.out_proj.weight"), ("bo", "self_attn.out_proj.bias"), ("w1", "mlp.fc1.weight"),
                  ("b1", "mlp.fc1.bias"), ("w2", "mlp.fc2.weight"), ("b2", "mlp.fc2.bias"), ("l1w", "layer_norm1.weight"),
                  ("l1b", "layer_norm1.bias"), ("l2w", "layer_norm2.weight"), ("l2b", "layer_norm2.bias")):
        out[nm] = g(k)
    return out


def projector_weights(W=None, device="cpu"):
    W = weights() if W is None else W
    g = lambda k: W["multi_modal_projector." + k].detach().to(device).double()  # noqa: E731
    return {"w1": g("linear_1.weight"), "b1": g("linear_1.bias"), "w2": g("linear_2.weight"), "b2": g("linear_2.bias")}


PROJ_GRAD_KEYS = {"w1": "linear_1.weight", "b1": "linear_1.bias", "w2": "linear_2.weight", "b2": "linear_2.bias"}


def head_weights(W=None, device="cpu"):
    W = weights() if W is None else W
    return {"n": W["language_model.model.norm.weight"].detach().to(device).double(),
            "w": W["language_model.lm_head.weight"].detach().to(device).double()}


# ---------------------------------------------------------------------------------------------
# LoRA: y = base + B(A(mask o x / (1 - p))) scaling, per module of a group of Linears sharing x
# ---------------------------------------------------------------------------------------------
LORA_R, LORA_SCALING, LORA_SEED = 64, 16.0 / 64, 1234
_M64 = (1 << 64) - 1
LM_GROUPS = (("qkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("o", ("self_attn.o_proj",)),
             ("gu", ("mlp.gate_proj", "mlp.up_proj")), ("down", ("mlp.down_proj",)))
VIT_GROUPS = (("qkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("fc1", ("mlp.fc1",)),
              ("fc2", ("mlp.fc2",)))


def module_seed(step_seed, uid, m):
    """the per-module dropout seed of lora.module_seed, restated"""
    x = (step_seed * 0x9E3779B97F4A7C15 + (uid * 8 + m + 1) * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 31
    return (x * 0x94D049BB133111EB) & _M64


def lora_group_shapes(tower):
    d, f = (LM["d"], LM["F"]) if tower == "lm" else (VIT["d"], VIT["F"])
    if tower == "lm":
        return {"qkv": (d, (d, d, d)), "o": (d, (d,)), "gu": (d, (f, f)), "down": (f, (d,))}
    return {"qkv": (d, (d, d, d)), "fc1": (d, (f,)), "fc2": (f, (d,))}


@functools.lru_cache(maxsize=None)
def lora_weights(tower, layer):
    """{group: (A [n r, in], B [sum out, r])} bf16 on the CPU: A ~ U(+-1/sqrt(in)) as peft, B ~ 0.05 N(0, 1)
    (non-zero, so every adapter term and gradient is exercised)"""
    out = {}
    for g, (inn, outs) in lora_group_shapes(tower).items():
        gen = _gen(f"lora/{tower}/{layer}/{g}")
        A = ((torch.rand(len(outs) * LORA_R, inn, generator=gen) * 2 - 1) / math.sqrt(inn)).to(BF)
        B = (torch.randn(sum(outs), LORA_R, generator=gen) * 0.05).to(BF)
        out[g] = (A, B)
    return out


def lora_groups(tower, layer, p, rows, device="cpu", row_index=None, uid0=None):
    """{group: dict(A, B, outs, masks, p, fused)} for the layer functions below. masks: per module the keep
    mask of oracle.lora_keep_mask, keyed by the row index the layer sees (0 .. rows-1), or by row_index
    (the mutant); None at p = 0. fused: the term is added in the base GEMM's epilogue unrounded (equal
    module widths, a multiple of 256, more than 16 rows); otherwise it is stored in bf16 first."""
    names = [g for g, _ in (LM_GROUPS if tower == "lm" else VIT_GROUPS)]
    uid0 = (8 * layer if tower == "lm" else (1 << 20) + 8 * layer) if uid0 is None else uid0
    out = {}
    for gi, g in enumerate(names):
        inn, outs = lora_group_shapes(tower)[g]
        A, B = lora_weights(tower, layer)[g]
        masks = None
        if p > 0:
            masks = []
            for m in range(len(outs)):
                n_rows = rows if row_index is None else int(row_index.max()) + 1
                k = torch.as_tensor(O.lora_keep_mask(module_seed(LORA_SEED, uid0 + gi, m), n_rows, inn, p))
                masks.append((k if row_index is None else k[row_index]).to(device))
        out[g] = dict(A=A.to(device).double(), B=B.to(device).double(), outs=outs, masks=masks, p=p,
                      fused=len(set(outs)) == 1 and outs[0] % 256 == 0 and rows > 16)
    return out


def lora_linear(x, w, b, grp, P, key, md, residual=None):
    """The stored output of a group's base Linear with its adapters (or without: grp None), in the GEMM
    epilogue's order: round(alpha AB + bias), + term, [round,] + residual, round. The adapters' share of
    dx is added to the stored base dx module by module (rounded after each under dropout, once without)."""
    if grp is None:
        y = md.lin(x, w, b)
        return md.R(y if residual is None else md.Rf(y) + residual)
    outs, n, r = grp["outs"], len(grp["outs"]), LORA_R
    seq = grp["masks"] is not None
    node, mod_in = x, [None] * n
    for m in reversed(range(n)):
        mod_in[m] = node
        if seq or m == 0:
            node = md.Rb(node)
    y = md.Rf(md.lin(node, w, b))
    ts, off = [], 0
    for m in range(n):
        xin = mod_in[m]
        if seq:
            xin = md.Rf(xin * grp["masks"][m] * (1.0 / (1.0 - grp["p"])))
        u = md.R(md.lin(xin, P[key + ".A"][m * r:(m + 1) * r]))
        t = md.lin(u, P[key + ".B"][off:off + outs[m]]) * LORA_SCALING
        if md.is_("lora_bwd_no_scaling"):
            t = _GradMod.apply(t, lambda g: g / LORA_SCALING)
        ts.append(t)
        off += outs[m]
    t = torch.cat(ts, 1)
    y = y + (t if grp["fused"] else md.Rf(t))
    return md.R(y if residual is None else md.Rf(y) + residual)


def _lora_leaves(P, lora):
    if lora:
        for g, grp in lora.items():
            P[g + ".A"] = grp["A"].detach().clone().requires_grad_(True)
            P[g + ".B"] = grp["B"].detach().clone().requires_grad_(True)


# ---------------------------------------------------------------------------------------------
# decoder layer
# ---------------------------------------------------------------------------------------------
# form grid: B sequences of L rows, pads[b] padding rows on the left (kv_start) or on the right (no
# kv_start: the tail pads are ordinary causal rows). form packed: the attended rows, sequence by
# sequence, then Tp - T zero rows. tail: the supervised-row tail's row set (-1: padding slot).
DECODER_CASES = {
    "grid-left": dict(form="grid", B=3, L=72, pads=(0, 7, 71), left=True),
    "grid-right": dict(form="grid", B=2, L=65, pads=(0, 9), left=False),
    "grid-long": dict(form="grid", B=1, L=200, pads=(0,), left=True),
    "packed": dict(form="packed", lens=(1, 63, 65, 130)),
    # first and last row of sequence 1 (rows 72 + 7 and 143), rows beside them, two -1 slots
    "grid-left+tail": dict(form="grid", B=3, L=72, pads=(0, 7, 71), left=True, tail=(5, 71, 79, 80, 143, 215, -1, -1)),
    # sequence 2 is rows 64 .. 128: its first and last row, the single row of sequence 0, two -1 slots
    "packed+tail": dict(form="packed", lens=(1, 63, 65, 130), tail=(0, 63, 64, 128, 129, 258, -1, -1)),
}


# LoRA cases: adapters on all four groups (frozen base), on a decoder case's geometry and inputs
LORA_CASES = {"lora-p0/grid-left": ("grid-left", 0.0), "lora-p0/packed": ("packed", 0.0),
              "lora-p05/grid-left": ("grid-left", 0.05), "lora-p05/packed": ("packed", 0.05)}
LORA_MUTANTS = {"lora_bwd_no_scaling": ("lora-p0/grid-left",), "lora_mask_by_grid_row": ("lora-p05/packed",)}
LORA_KEYS = ("h3", "dh") + tuple(f"{g}.{ab}" for g, _ in LM_GROUPS for ab in "AB")


def lora_case_groups(name, layer, device="cpu", mutant=None):
    base, p = LORA_CASES[name]
    g = decoder_case(base)[0]
    row_index = None
    if mutant == "lora_mask_by_grid_row" and g.c["form"] == "packed":
        row_index = (g.seq.clamp_min(0) * g.L + g.pos)   # the row of a [B, L] grid the packed row came from
    return lora_groups("lm", layer, p, g.Tp, device, row_index=row_index)


class Geometry:
    """rows, positions and the live-key relation of a decoder case, on the CPU"""

    def __init__(self, c):
        self.c = c
        if c["form"] == "grid":
            B, L = c["B"], c["L"]
            self.B, self.L, self.T = B, L, B * L
            self.Tp = self.T
            t = torch.arange(L)
            mask = torch.stack([(t >= p) if c["left"] else (t < L - p) for p in c["pads"]]).long()
            self.mask = mask
            self.pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 1).reshape(-1)
            self.kv_start = [int(p) for p in c["pads"]] if c["left"] else None
            self.seq = torch.arange(B).repeat_interleave(L)
            key_live = mask.reshape(-1).bool() if c["left"] else torch.ones(B * L, dtype=torch.bool)
            self.grid_pos = t.repeat(B)
        else:
            lens = c["lens"]
            self.B, self.L, self.T = len(lens), max(lens), sum(lens)
            self.Tp = max(8, -(-self.T // 8) * 8)
            self.lens = lens
            self.seq = torch.cat([torch.full((n,), b) for b, n in enumerate(lens)] + [torch.full((self.Tp - self.T,), -1)])
            self.pos = torch.cat([torch.arange(n) for n in lens] + [torch.zeros(self.Tp - self.T, dtype=torch.long)])
            key_live = self.seq >= 0
            self.kv_start = None
        self.key_live = key_live
        self.tail = torch.tensor(c["tail"], dtype=torch.long) if c.get("tail") else None
        pad = self.seq < 0
        if self.tail is None:   # rows that must come back exactly zero: the packed padding rows
            self.zero_rows = {"h3": pad, "dh": pad}
        else:
            # with the tail only its rows carry a gradient into the layer: dh is non-zero on them and on
            # the keys they see, and exactly zero everywhere else; the compact h3 is zero on the -1 slots
            t = self.tail[self.tail >= 0]
            reached = self.live()[t].any(0)
            reached[t] = True
            self.zero_rows = {"h3": self.tail < 0, "dh": ~reached}
        self.pad_rows = pad

    def live(self, mutant=None):
        """[Tp, Tp] bool: query row i sees key row j"""
        i = torch.arange(self.Tp)
        key_live = self.key_live.clone()
        if mutant == "kv_start_ignored" and self.kv_start is not None:
            key_live[self.seq == 1] = True
        live = (self.seq[:, None] == self.seq[None, :]) & (self.seq[:, None] >= 0) & (i[None, :] <= i[:, None]) & key_live[None, :]
        if mutant == "packed_leak" and self.c["form"] == "packed":
            first = self.lens[0] + self.lens[1]     # sequence 2's first query sees sequence 1's keys
            live[first, self.lens[0]:first] = True
        return live

    def positions(self, mutant=None):
        if mutant == "grid_positions" and self.c["form"] == "grid":
            return self.grid_pos
        return self.pos


@functools.lru_cache(maxsize=None)
def decoder_case(name):
    """(Geometry, h [Tp, d] bf16, dh3 bf16 ([n, d] with a tail)) of a decoder case, on the CPU"""
    g = Geometry(DECODER_CASES[name])
    d = LM["d"]
    h = _randn(name + "/h", g.Tp, d, H_RMS)
    h[g.pad_rows] = 0
    if g.tail is not None:
        dh3 = _randn(name + "/dh3", g.tail.numel(), d, G_RMS)
        dh3[g.tail < 0] = 0   # what HeadLossRowsFn hands back on its padding slots
    else:
        dh3 = _randn(name + "/dh3", g.Tp, d, G_RMS)
        dh3[g.pad_rows] = 0
    return g, h, dh3


def decoder_layer(h, dh3, W, g, md, lora=None):
    """One decoder layer forward and backward. h, dh3: f64 values; W: lm_layer_weights; g: Geometry
    (its index tensors are moved to h's device). Returns {"h3", "dh", and one entry per key of W}."""
    dev = h.device
    d, H, D, Fd = LM["d"], LM["H"], LM["D"], LM["F"]
    mu = md.mutant
    h = h.detach().clone().requires_grad_(True)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in W.items()}
    _lora_leaves(P, lora)
    lg = lora or {}
    live = g.live(mu).to(dev)
    c, s = rope_tables(g.positions(mu).to(dev), D, LM["theta"], md)
    zero = torch.zeros_like

    x1 = rmsnorm(h, P["n1"], LM["eps"], md)
    qkv = lora_linear(x1, P["wqkv"], None, lg.get("qkv"), P, "qkv", md)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    inv = lambda t: rope(t, c, s, H, md, inverse=True)  # noqa: E731

    class _Rope(torch.autograd.Function):   # the backward is the layer's own inverse-RoPE call
        @staticmethod
        def forward(ctx, x):
            return rope(x, c, s, H, md)

        @staticmethod
        def backward(ctx, gr):
            return gr if mu == "no_inverse_rope" else inv(gr)
    q, k = md.R(_Rope.apply(q)), md.R(_Rope.apply(k))
    if mu == "dv_roped":
        v = _GradMod.apply(v, inv)
    o = attention(q, k, v, live, D ** -0.5, H, md)
    res1 = x1 if mu == "residual_from_x1" else h
    if mu == "no_dres_norm1":
        res1 = _GradMod.apply(res1, zero)
    h2 = lora_linear(o, P["wo"], None, lg.get("o"), P, "o", md, residual=res1)
    rows = None if g.tail is None else g.tail.to(dev)
    if rows is not None:   # the supervised-row tail: the MLP half on the rows only, -1 slots are zero rows
        keep = (rows >= 0)[:, None]
        h2m = torch.where(keep, h2[rows.clamp_min(0)], torch.zeros((), dtype=F64, device=dev))
    else:
        h2m = h2
    x2 = rmsnorm(h2m, P["n2"], LM["eps"], md)
    up = dn = lambda t: t  # noqa: E731
    if rows is not None and mu != "tail_dw_gathered":
        # the tail's weight-gradient products run over the operands scattered back to full height (zero
        # rows keep the full path's summation order); the mutant sums the compact operands instead
        valid = rows >= 0
        up = lambda t: torch.zeros((g.Tp, t.shape[1]), dtype=F64, device=dev).index_add(0, rows[valid], t[valid])  # noqa: E731
        dn = lambda t: torch.where(keep, t[rows.clamp_min(0)], torch.zeros((), dtype=F64, device=dev))  # noqa: E731
    gu = dn(lora_linear(up(x2), P["wgu"], None, lg.get("gu"), P, "gu", md))
    if mu == "swiglu_bwd_swapped":
        gu = _GradMod.apply(gu, lambda t: torch.cat((t[:, Fd:], t[:, :Fd]), 1))
    a = md.R(F.silu(gu[:, :Fd]) * gu[:, Fd:])
    res2 = h2m
    if mu in ("no_dres_norm2", "tail_no_dh3"):
        res2 = _GradMod.apply(res2, zero)
    h3 = dn(lora_linear(up(a), P["wd"], None, lg.get("down"), P, "down", md, residual=up(res2)))
    h3.backward(dh3)
    out = {"h3": h3.detach(), "dh": h.grad}
    out.update({k_: p.grad for k_, p in P.items()})
    if md.emu:
        out = {k_: (bf(t) if k_ != "h3" else t) for k_, t in out.items()}
    if mu == "dk_into_v":
        w = out["wqkv"].clone()
        w[2 * d:], w[d:2 * d] = out["wqkv"][d:2 * d], 0.0
        out["wqkv"] = w
    if mu == "dh_row_zeroed":   # the last query of sequence 1
        r = _last_row_of_seq1(g)
        out["dh"] = out["dh"].clone()
        out["dh"][r] = 0
    if mu == "dh_row_scaled":
        r = _last_row_of_seq1(g)
        out["dh"] = out["dh"].clone()
        out["dh"][r] *= 1.1
    if mu == "h3_row_scaled":
        r = 0 if g.tail is not None else _last_row_of_seq1(g)
        out["h3"] = out["h3"].clone()
        out["h3"][r] *= 1.1
    return out


def _last_row_of_seq1(g):
    return int((g.seq == 1).nonzero().max())


# Mutants that must PASS, because they change nothing a layer can show: RoPE positions taken from the
# grid index on a left-padded row shift every live row of a sequence by its pad count, and q . k depends
# on position differences only (padded rows are neither keys nor queries that see one). What that mutant
# breaks is the KV-cache prefix, not a training layer.
# The tail's dW operands gathered instead of scattered is a summation order (the scattered rows are exact
# zeros): the gates are not bitwise gates, and it passes them.
EQUIVALENT_MUTANTS = {"grid_positions": ("grid-left",), "tail_dw_gathered": ("grid-left+tail", "packed+tail")}
# mutant -> the decoder cases it is run on (it must fail a gate in at least one of them)
DECODER_MUTANTS = {
    "residual_from_x1": ("grid-long",), "no_dres_norm1": ("grid-long",), "no_dres_norm2": ("grid-long",),
    "no_inverse_rope": ("grid-long",), "dv_roped": ("grid-long",),
    "kv_start_ignored": ("grid-left",), "packed_leak": ("packed",), "dk_no_scale": ("grid-long",),
    "swiglu_bwd_swapped": ("grid-long",), "dk_into_v": ("grid-long",), "tail_no_dh3": ("grid-left+tail", "packed+tail"),
    "dh_row_zeroed": ("grid-left", "packed"), "dh_row_scaled": ("grid-left", "packed"), "h3_row_scaled": ("grid-left", "packed"),
}


# ---------------------------------------------------------------------------------------------
# CLIP encoder layer (frozen tower: the input gradient is the only gradient)
# ---------------------------------------------------------------------------------------------
CLIP_CASES = {"b1": dict(B=1), "b3": dict(B=3)}


@functools.lru_cache(maxsize=None)
def clip_case(name):
    T = CLIP_CASES[name]["B"] * VIT["T"]
    return _randn("clip/" + name + "/h", T, VIT["d"], H_RMS), _randn("clip/" + name + "/dh3", T, VIT["d"], G_RMS)


def clip_layer(h, dh3, W, B, md, lora=None):
    dev = h.device
    d, H, D, T = VIT["d"], VIT["H"], VIT["D"], VIT["T"]
    h = h.detach().clone().requires_grad_(True)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in W.items()}
    _lora_leaves(P, lora)
    lg = lora or {}
    seq = torch.arange(B, device=dev).repeat_interleave(T)
    live = seq[:, None] == seq[None, :]
    x1 = layernorm(h, P["l1w"], P["l1b"], VIT["eps"], md)
    qkv = lora_linear(x1, P["wqkv"], P["bqkv"], lg.get("qkv"), P, "qkv", md)
    o = attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], live, D ** -0.5, H, md)
    h2 = lora_linear(o, P["wo"], P["bo"], None, P, "o", md, residual=h)
    x2 = layernorm(h2, P["l2w"], P["l2b"], VIT["eps"], md)
    pre = lora_linear(x2, P["w1"], P["b1"], lg.get("fc1"), P, "fc1", md)   # the stored bf16 pre-activation
    a = md.R(_act(pre, "gelu" if md.is_("clip_erf_gelu") else "quick_gelu"))
    h3 = lora_linear(a, P["w2"], P["b2"], lg.get("fc2"), P, "fc2", md, residual=h2)
    h3.backward(dh3)
    out = {"h3": h3.detach(), "dh": h.grad}
    out.update({k: p.grad for k, p in P.items()})
    if md.is_("clip_no_qkv_bias_grad"):
        out["bqkv"] = torch.zeros_like(out["bqkv"])
    if md.emu:
        out = {k: (bf(t) if k != "h3" else t) for k, t in out.items()}
    return out


# ---------------------------------------------------------------------------------------------
# projector
# ---------------------------------------------------------------------------------------------
PROJECTOR_ROWS = (1, 257, 771)


@functools.lru_cache(maxsize=None)
def projector_case(rows):
    return _randn(f"proj/{rows}/x", rows, VIT["d"], H_RMS), _randn(f"proj/{rows}/dy", rows, LM["d"], G_RMS)


def projector(x, dy, W, md):
    x = x.detach().clone().requires_grad_(True)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in W.items()}
    pre = md.R(md.lin(x, P["w1"], P["b1"]))   # the activation reads the rounded pre-activation
    a = md.R(_act(pre, "quick_gelu" if md.is_("proj_quick_gelu") else "gelu"))
    y = md.R(md.lin(a, P["w2"], P["b2"]))
    y.backward(dy)
    out = {"y": y.detach(), "dx": x.grad}
    out.update({k: p.grad for k, p in P.items()})
    if md.emu:
        out = {k: (bf(t) if k != "y" else t) for k, t in out.items()}
    return out


# ---------------------------------------------------------------------------------------------
# head: final RMSNorm -> lm_head -> shifted masked CE -> mean over the supervised rows
# ---------------------------------------------------------------------------------------------
# labels [B, L] with `sup` supervised label positions per sequence (the rows before them are the
# supervised rows after the shift); n: HeadLossRowsFn's padded row count (-1 slots: n - supervised)
HEAD_CASES = {
    "rows8": dict(B=2, L=20, pads=(0, 3), sup=(3, 2), n=8),
    "rows24": dict(B=3, L=24, pads=(0, 5, 0), sup=(7, 6, 8), n=24),
    "one-row": dict(B=2, L=20, pads=(0, 3), sup=(0, 1), n=8),
    "all-ignored": dict(B=2, L=20, pads=(0, 3), sup=(0, 0), n=8),
}


def shift_targets(labels, mask, unshifted=False):
    """targets[b, t] = labels[b, t + 1] where mask[b, t + 1] != 0, else IGNORE (the last column: IGNORE)"""
    if unshifted:
        return torch.where(mask != 0, labels, IGNORE).reshape(-1)
    t = torch.full_like(labels, IGNORE)
    t[:, :-1] = torch.where(mask[:, 1:] != 0, labels[:, 1:], IGNORE)
    return t.reshape(-1)


@functools.lru_cache(maxsize=None)
def head_case(name):
    """(h [B L, d] bf16, labels [B, L], mask [B, L] (right padding), dlogits [B L, V] bf16)"""
    c = HEAD_CASES[name]
    B, L = c["B"], c["L"]
    gen = _gen("head/" + name)
    t = torch.arange(L)
    mask = torch.stack([t < L - p for p in c["pads"]]).long()
    labels = torch.full((B, L), IGNORE, dtype=torch.long)
    for b, (p, n) in enumerate(zip(c["pads"], c["sup"])):
        if n:
            labels[b, L - p - n:L - p] = torch.randint(2, 1000, (n,), generator=gen)
    h = _randn("head/" + name + "/h", B * L, LM["d"], 2 * H_RMS)
    dlog = _randn("head/" + name + "/dlogits", B * L, LM["V"], G_RMS)
    return h, labels, mask, dlog


def head(h, labels, mask, W, md, dlogits=None):
    """{"loss", "row_loss" [T] (0 on unsupervised rows), "count", "logits", "dh", "n", "w"}. With no
    supervised row the loss is 0 / 0 = NaN (torch's CrossEntropyLoss on an empty selection, the
    reference's value) and every gradient is 0: nothing depends on a row without a label."""
    h = h.detach().clone().requires_grad_(True)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in W.items()}
    tg = shift_targets(labels, mask, unshifted=md.is_("head_unshifted")).to(h.device)
    sup = tg != IGNORE
    x = rmsnorm(h, P["n"], LM["eps"], md)
    logits = md.R(md.lin(x, P["w"]))
    lg = md.Rb(logits)   # the CE gradient is stored in bf16 before an upstream logits gradient is added
    row = torch.logsumexp(lg, -1) - lg.gather(1, tg.clamp_min(0)[:, None])[:, 0]
    row = torch.where(sup, row, torch.zeros((), dtype=F64, device=h.device))
    count = int(sup.sum())
    denom = h.shape[0] if md.is_("head_mean_all_rows") else count
    total = row.sum()
    loss = total / denom if denom else total * float("nan")
    outs, seeds = ([loss], [None]) if count else ([], [])
    if dlogits is not None:
        outs.append(logits)
        seeds.append(dlogits)
    if outs:
        torch.autograd.backward(outs, seeds)
    z = torch.zeros_like
    out = {"loss": float(loss.detach()), "row_loss": row.detach(), "count": count, "logits": logits.detach(),
           "dh": h.grad if h.grad is not None else z(h), "n": P["n"].grad if P["n"].grad is not None else z(P["n"]),
           "w": P["w"].grad if P["w"].grad is not None else z(P["w"]), "sup": sup}
    if md.emu:
        out.update({k: bf(out[k]) for k in ("dh", "n", "w")})
    return out


def f32_sum(row_loss):
    """the row losses rounded to f32 and summed in f32 (a pairwise order): what the 1e-6 loss gate allows for"""
    return float(row_loss.float().sum())


LOSS_GATE = 1e-6   # tests/test_supervised_rows_gpu.py's f32 reduction gate, relative


# ---------------------------------------------------------------------------------------------
# figures and gates
# ---------------------------------------------------------------------------------------------
def row_fig(x, ref):
    x, ref = x.double(), ref.double()
    if ref.dim() == 1:
        x, ref = x[None], ref[None]
    rms = ref.pow(2).mean().sqrt()
    err = (x - ref).norm(dim=-1)
    den = ref.norm(dim=-1) + FLOOR * rms * math.sqrt(ref.shape[-1])
    r = torch.where(err > 0, err / den.clamp_min(1e-300), torch.zeros_like(err))
    r = torch.where(torch.isnan(err), torch.full_like(r, float("inf")), r)
    return r.max().item()


def block_figs(x, ref, n):
    """rel-L2 of each of the n equal blocks of output features"""
    x, ref = x.double(), ref.double()
    rows = ref.shape[0] // n
    return [((x[i * rows:(i + 1) * rows] - ref[i * rows:(i + 1) * rows]).norm()
             / ref[i * rows:(i + 1) * rows].norm()).item() for i in range(n)]


def elem_fig(x, ref):
    x, ref = x.double(), ref.double()
    return ((x - ref).abs() / (ref.abs() + ref.pow(2).mean().sqrt())).max().item()


def whole_rel_l2(x, ref):
    """tests/test_model_gpu.py's rel_l2: the whole-tensor figure the model tests gate at 1e-2 / 2e-2"""
    return ((x.double() - ref.double()).norm() / (ref.double().norm() + 1e-12)).item()


def figures(name, x, ref):
    """{figure name: value} of one tensor against the exact reference"""
    if ref.dim() == 1:
        return {f"{name}.elem": elem_fig(x, ref)}
    out = {f"{name}.row": row_fig(x, ref)}
    if name in BLOCKS:
        for i, v in enumerate(block_figs(x, ref, BLOCKS[name])):
            out[f"{name}.block{i}"] = v
    return out


def gate(got, emu, exact, keys=None, zero_rows=None, exact_keys=()):
    """got / emu / exact: {tensor: value} of the layer under test, the emulation and the exact reference.
    zero_rows: {tensor: bool [rows]} of the rows that must be exactly zero. exact_keys: tensors the case
    makes exactly representable (a one-row column sum is that row), where an emulated figure of 0 stands
    for "bitwise" instead of failing the sanity check.
    Returns (records [{tensor figure, emulated, measured, ratio}], failures)."""
    recs, fails = [], []
    for k in (keys if keys is not None else [k for k in exact if torch.is_tensor(exact[k]) and exact[k].is_floating_point()]):
        x = got[k]
        if not torch.isfinite(x.double()).all().item():
            fails.append(f"{k} has non-finite elements")
        if zero_rows is not None and k in zero_rows:
            nz = int((x[zero_rows[k].to(x.device)] != 0).sum().item())
            if nz:
                fails.append(f"{k}: {nz} nonzero elements on rows that must be exactly zero")
        fe, fg = figures(k, emu[k], exact[k]), figures(k, x, exact[k])
        for f in fe:
            ratio = fg[f] / fe[f] if fe[f] > 0 else (0.0 if fg[f] == 0 else float("inf"))
            recs.append({"figure": f, "emulated": fe[f], "measured": fg[f], "ratio": ratio})
            if fe[f] == 0.0 and k in exact_keys:
                if fg[f] != 0.0:   # the result is a bf16 value as it stands: bitwise, or wrong
                    fails.append(f"{f}: {fg[f]:.3e} where the result is exactly representable")
                continue
            if not (math.isfinite(fe[f]) and fe[f] > 0):
                fails.append(f"{f}: the emulated figure {fe[f]} is not finite and > 0: the comparison is broken")
            if not (math.isfinite(fg[f]) and fg[f] > 0):
                fails.append(f"{f}: the measured figure {fg[f]} is not finite and > 0: the comparison compared nothing")
            if not fg[f] <= M * fe[f]:
                fails.append(f"{f}: {fg[f]:.3e} > {M} x emulated {fe[f]:.3e}")
    return recs, fails


def no_zero_reference_rows(exact, keys, zero_rows=None):
    """the condition that no case excludes rows from a gate: the exact reference has no zero row except
    the rows that must be exactly zero; returns the offending (tensor, row count) pairs"""
    bad = []
    for k in keys:
        r = exact[k].double()
        if r.dim() != 2:
            continue
        z = r.norm(dim=-1) == 0
        if zero_rows is not None and k in zero_rows:
            z = z & ~zero_rows[k].to(z.device)
        if z.any():
            bad.append((k, int(z.sum())))
    return bad


# ---------------------------------------------------------------------------------------------
# row movers: bitwise gather and its transpose
# ---------------------------------------------------------------------------------------------
def gather_rows(x, rows):
    """x[rows], a zero row where rows == -1"""
    out = x[rows.clamp_min(0)].clone()
    out[rows < 0] = 0
    return out


def scatter_rows(y, rows, full):
    """[full, cols]: y's row i in row rows[i] (rows >= 0, distinct), zeros elsewhere"""
    out = torch.zeros((full, y.shape[1]), dtype=y.dtype, device=y.device)
    keep = rows >= 0
    out[rows[keep]] = y[keep]
    return out


MOVER_ROWS = (0, 3, 8, 16, 17, 36, -1, -1)   # of [37, cols]: first and last row, ascending, then -1 slots
MOVER_FULL = 37
