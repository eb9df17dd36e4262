"""KV-cache decode and generate().

Reference: CuLLaVOModel.generate(**inputs, do_sample=True, temperature=0.9, top_k=50,
top_p=0.95, max_new_tokens=1000, use_cache=True) (cullavo/arch_cullavo.py:362-363, the
step-2 pre-labelling loop) runs HF's GenerationMixin over forward(); the cached branch of that
forward is :605-636 (transformers ~4.37 llava: the new token's position is the number of
attended tokens so far, position_ids = attention_mask.sum(-1) - 1).

MI355X design: the cache is preallocated once per generate() call in HBM as K, V
[layers, B, Lmax, H*D] bf16; the prompt (text + 576 image rows, merged exactly as training
does) is prefilled through the same fused kernels (GEMMs, RoPE, causal flash attention) with
its rotated keys/values appended by kv_append; every decode step runs the layers on one row
per sequence and attends with the split-KV attn_decode kernel. A cached step may also carry
several new tokens per sequence -- a follow-up turn, a second question about an image whose rows
are already cached, the later pieces of a chunked prefill (generate(prefill_chunk=N)): RoPE at
next_pos .. next_pos + n - 1, kv_append, then attn_fwd_cached, the causal flash kernel with a
query offset over the cache's first length + n rows (reference: any number of new input_ids with
past_key_values, arch_cullavo.py:605-647). New turns of unequal length: the ragged cache below. Left-padded batches are
supported through kv_start (keys before the first attended token are masked); a prompt with
holes in its attention mask is not (decode attention reads one contiguous key range).
Sampling (temperature, top-k, top-p, multinomial; or greedy) follows HF's warper order on the
GPU with torch ops: it is O(B x vocab) per token and not a kernel of the hot path.
generate(seed=...) / generate(device_loop=True) take the other route: one HIP kernel
(csrc/sample.hip, ops.sample_token) does the warpers, a Philox draw seeded per sequence and the
eos / pad bookkeeping, is captured at the end of the decode graph (DecodeGraph(sampler=...)) and
writes the next step's input token on the device, so a generation is a row of graph replays with
one host read of `finished` every 16 tokens. It takes 1 <= top_k <= 1024; top_k=0 (the nucleus
over the full vocabulary), repetition penalties and beam search stay with the host loop or are
not implemented.

Ragged cache (batched follow-up turns of unequal length). KVCache.lengths (int32 [B], or None: every
sequence holds `length` rows, everything above) makes the cache compact and ragged: sequence b owns
rows [0, lengths[b]) with no holes and attends [kv_start[b], lengths[b]) -- the keys and RoPE
positions HF computes from a holed attention mask and position_ids = cumsum(mask) - 1
(arch_cullavo.py:605-636), without storing or streaming a masked key. A new turn arrives as a
left-padded [B, Lnew] block with its mask; q_pad[b] is the row's count of leading zeros (a row of
zeros: nothing new), the live rows get positions next_pos[b] .., kv_append_ragged writes them at
lengths[b] .. and attn_fwd_ragged attends with kv_len = lengths + n_new. generate(compact_cache=True)
keeps the cache ragged while it decodes: a row stops advancing with the step that would feed its
eos (DecodeGraph(live=True): pos += live, start += live), so the pads a finished row is fed land on
one scratch row behind its length and a second turn continues every conversation from exactly its
own tokens. `length` stays the high-water mark max(lengths).

How the pieces fit. lm_infer classifies a call (prefill, uniform step, ragged step) and cuts it into
chunks; each chunk takes one attention route -- PREFILL, CACHED, RAGGED, DECODE_FUSED or DECODE,
decided once (decode_route() reads FUSE_DECODE_ROPE per call) -- and run_chunk takes it through every
layer (layer_infer: one ladder over the routes), the final norm and lm_head; DecodeGraph captures the
same run_chunk. KVCache's state moves through its methods only: begin, advance / advance_ragged,
reserve / grow, adopt (a decode graph's buffers become next_pos / lengths) and mark / release (the
state generate() returns). generate() is one loop over a sampler (SamplerState on the device,
HostSampler around sample_next) and a DecodeStepper (graph replay or eager cached forward).
"""
from __future__ import annotations

import torch

from . import ops
from .functions import StepContext
from .lora import NO_LORA, LoraTerm

import os

# decode-step fusions (all bitwise the unfused values), CULLAVO_DECODE_FUSE = comma list:
#   "gu"    (default on) the SwiGLU in the gate|up product's epilogue (cullavo_decode_linear
#           transform 3: one launch instead of the product + cullavo_swiglu_fwd);
#   "rope"  (default on) RoPE + KV append inside decode attention (cullavo_attn_decode_rope);
#   "norm"  the two RMSNorms into the q|k|v and gate|up products' X loads, "swiglu" the SwiGLU into
#           down_proj's X loads (round 4: ~2x slower per product, profiles/r04/decode/decode_fusions_ab.txt;
#           round 5, the whole workgroup normalising: 3.73 vs 3.53 ms per token at batch 1, 4.67 vs
#           4.02 at batch 4 -- every workgroup redoing the row norm still costs more than the one
#           norm launch: off by default). A norm in the TAIL of o_proj / down_proj instead (the last
#           workgroup by an agent-scope counter normalises the rows) measured 3.78 vs 3.53 ms
#           (profiles/r05/decode/pnorm_ab_*): not kept
#   "lora"  (default on) the adapters' up-projection t = scaling * u_m B_m^T in the epilogue of the
#           group's weight-streaming product (cullavo_decode_linear_lora / cullavo_nf4_decode_linear_lora)
#           instead of one K = 64 product per module into an [M, N] addend; with it the fusions above
#           hold for a model with adapters too. Off: the materialised addend (LoraTerm.materialize).
_FUSE = {f.strip() for f in os.environ.get("CULLAVO_DECODE_FUSE", "gu,rope,lora").split(",") if f.strip()}
FUSE_DECODE_NORMS = "norm" in _FUSE
FUSE_DECODE_SWIGLU = "swiglu" in _FUSE
FUSE_DECODE_GU = "gu" in _FUSE
FUSE_DECODE_ROPE = "rope" in _FUSE
FUSE_DECODE_LORA = "lora" in _FUSE
# CULLAVO_NF4_DECODE=0: a model quantised by quant.quantize_lm_nf4_ decodes through the bf16 GEMV on
# its (dequantised) arena weights instead of the 4-bit product on the NF4 copies (A/B switch)
NF4_DECODE = os.environ.get("CULLAVO_NF4_DECODE", "1") != "0"
# CULLAVO_DECODE_WIDE=1: a one-token step at 17 .. 64 sequences runs its Linears on the wide
# weight-streaming product (cullavo_decode_linear_wide) wherever ops.WIDE_TILES_FASTER does not keep the
# shape on ops.linear's tiles. Off by default: on the 7B products the tiles' split-K route already
# streams the weights at 1.9-3.8 TB/s and the wide product beat it only on o up to 32 rows and on
# gate|up and lm_head at 17, so the replayed 7B step measured 0.992 of the tiles' time at batch 32
# (8.120 against 8.183 ms per token, the tiles' own runs spread 0.5 %) and 1.000 at 64, where every
# product stays on the tiles (INTEGRATION.md "Wide decode steps"; profiles/r21/wide_decode/)
DECODE_WIDE = os.environ.get("CULLAVO_DECODE_WIDE", "0") == "1"


def wide_route(B: int, Lnew: int, dtype, switch: bool | None = None) -> bool:
    """Whether a step of Lnew new rows for each of B sequences runs its Linears on the wide
    weight-streaming product (ops.decode_linear_wide): one token per sequence, bf16 rows, 17 <= B <= 64,
    and the switch on (None: DECODE_WIDE, read per call: tests patch it). Everything else keeps its
    route: B <= 16 the GEMV, multi-token steps and the f32 parity model the tiles."""
    if switch is None:
        switch = DECODE_WIDE
    return bool(switch) and Lnew == 1 and dtype == torch.bfloat16 and ops.WIDE_M_MIN <= B <= ops.WIDE_M_MAX


def _wide_takes(w, M: int) -> bool:
    """a weight the wide product takes at M rows: its shape rules, and not a measured loser
    (ops.WIDE_TILES_FASTER), which stays on the tiles"""
    rows, K = w.shape
    return rows % 8 == 0 and K % 8 == 0 and not ops.wide_prefers_tiles(rows, K, M)


def left_pad_span(mask, message: str):
    """(first, count) of a 0/1 mask [B, L] (int64): each row's number of leading zeros and of ones.
    One contiguous attended span per row, left padding only: a zero after a row's first one raises
    NotImplementedError(message)."""
    first = (mask.cumsum(-1) == 0).sum(-1)
    count = mask.sum(-1)
    if bool((count + first != mask.shape[1]).any()):
        raise NotImplementedError(message)
    return first, count


KV_DTYPES = ("bf16", "fp8", "fp8_sim")


class KVCache:
    """Per-layer K, V [B, Lmax, H*D] in HBM plus the per-row state the decode kernels read. The state
    moves through methods only: begin (prefill), advance / advance_ragged (rows appended), reserve /
    grow (capacity), adopt / mark / release (the hand-over to a decode graph and back).
    kv_dtype (INTEGRATION.md "FP8 KV cache"): "bf16" -- k, v hold the rows as they are; "fp8" -- k, v
    hold e4m3 codes (uint8) and k_exp, v_exp [layers, B, Lmax, H] one power-of-two exponent per token
    and head (uint8, e + 127), half the bytes; "fp8_sim" -- a bf16 cache whose appends quantise and
    dequantise, the numerics-identical twin of "fp8" on the bf16 kernels. The bookkeeping is the same
    for all three."""

    def __init__(self, n_layers: int, B: int, max_len: int, H: int, D: int, device, dtype=torch.bfloat16,
                 kv_dtype: str = "bf16"):
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype {kv_dtype!r}: one of {KV_DTYPES}")
        if kv_dtype != "bf16" and (dtype != torch.bfloat16 or D != 128):
            raise NotImplementedError(f"kv_dtype {kv_dtype!r} quantises bf16 rows of head_dim 128 (got {dtype}, "
                                      f"head_dim {D})")
        self.kv_dtype = kv_dtype
        self.k = torch.empty((n_layers, B, max_len, H * D), dtype=torch.uint8 if kv_dtype == "fp8" else dtype,
                             device=device)
        self.v = torch.empty_like(self.k)
        self.k_exp = self.v_exp = None
        if kv_dtype == "fp8":
            self.k_exp = torch.empty((n_layers, B, max_len, H), dtype=torch.uint8, device=device)
            self.v_exp = torch.empty_like(self.k_exp)
        self._slab = None                    # fp8: the bf16 scratch the multi-token routes attend (dequant)
        self.B, self.max_len, self.H, self.D = B, max_len, H, D
        self.length = 0                      # rows written: every sequence's, or max(lengths) when ragged
        self.lengths = None                  # int32 [B]: rows written per sequence (None: `length` for all)
        self.kv_start = None                 # int32 [B]: first attended key (left padding)
        self.next_pos = None                 # int64 [B]: RoPE position of the next token

    def __len__(self):
        return self.k.shape[0]

    def __getitem__(self, layer: int):
        """HF legacy view: (key, value) as [B, H, L, D] over the filled rows. An fp8 cache returns
        dequantised bf16 copies (writing to them does not reach the cache)."""
        B, L, H, D = self.B, self.length, self.H, self.D
        if self.kv_dtype == "fp8":
            k, v = ops.kv_dequant_fp8(self.k[layer], self.v[layer], self.k_exp[layer], self.v_exp[layer], rows=L,
                                      H=H, D=D)
            return k.view(B, L, H, D).transpose(1, 2), v.view(B, L, H, D).transpose(1, 2)
        return (self.k[layer, :, :L].view(B, L, H, D).transpose(1, 2),
                self.v[layer, :, :L].view(B, L, H, D).transpose(1, 2))

    def exps(self, layer: int):
        """the layer's (K, V) exponents [B, Lmax, H] of an fp8 cache; (None, None) otherwise"""
        return (None, None) if self.k_exp is None else (self.k_exp[layer], self.v_exp[layer])

    def append(self, layer: int, k, v, start, Lnew: int, q_pad=None):
        """rows k, v [B*Lnew, >= H*D] into the layer's cache at rows start[b] .. (q_pad: a left-padded
        block, ops.kv_append_ragged), quantised as kv_dtype says"""
        kc, vc, B = self.k[layer], self.v[layer], self.B
        if self.kv_dtype == "bf16":
            if q_pad is None:
                return ops.kv_append(k, v, kc, vc, start, B=B, Lnew=Lnew)
            return ops.kv_append_ragged(k, v, kc, vc, start, q_pad, B=B, Lnew=Lnew)
        kw = dict(B=B, Lnew=Lnew, H=self.H, D=self.D, sim=self.kv_dtype == "fp8_sim")
        if q_pad is None:
            return ops.kv_append_fp8(k, v, kc, vc, *self.exps(layer), start, **kw)
        return ops.kv_append_ragged_fp8(k, v, kc, vc, *self.exps(layer), start, q_pad, **kw)

    def attended(self, layer: int, rows: int):
        """the layer's (K, V) [B, >= rows, H*D] bf16 as attn_fwd_cached / attn_fwd_ragged read them: the
        cache itself, or for fp8 its first `rows` rows dequantised into one scratch slab that every
        layer reuses (stream order: a layer's attention has read it before the next layer's pass writes)"""
        if self.kv_dtype != "fp8":
            return self.k[layer], self.v[layer]
        if self._slab is None or self._slab[0].shape[1] < rows:
            cap = min(256 * -(-rows // 256), self.max_len)
            self._slab = tuple(torch.empty((self.B, cap, self.H * self.D), dtype=torch.bfloat16, device=self.k.device)
                               for _ in range(2))
        return ops.kv_dequant_fp8(self.k[layer], self.v[layer], self.k_exp[layer], self.v_exp[layer], rows=rows,
                                  H=self.H, D=self.D, out=self._slab)

    def get_seq_length(self) -> int:
        return self.length

    def to_legacy_cache(self):
        """transformers' legacy tuple: ((key, value) [B, H, L, D] per layer): views of this cache, or
        for an fp8 cache dequantised bf16 copies"""
        return tuple(self[i] for i in range(len(self)))

    def make_ragged(self):
        """give the cache per-sequence lengths (all `length`); a ragged cache stays ragged"""
        if self.lengths is None:
            self.lengths = torch.full((self.B,), self.length, dtype=torch.int32, device=self.k.device)
        return self

    def key_mask(self):
        """bool [B, length]: the cache slots sequence b attends, kv_start[b] <= j < lengths[b]"""
        j = torch.arange(self.length, device=self.k.device)[None]
        m = j < (self.lengths[:, None] if self.lengths is not None else self.length)
        if self.kv_start is not None:
            m = m & (j >= self.kv_start[:, None])
        return m.expand(self.B, self.length)

    def begin(self, kv_start, next_pos):
        """the prefill state of an empty cache: each row's first attended key and the RoPE position
        that follows its prompt (the prompt's rows arrive through advance(n, positions=False))"""
        self.kv_start, self.next_pos = kv_start, next_pos

    def advance(self, n: int, positions: bool = True):
        """the bookkeeping of a uniform step that appended n rows to every sequence. positions=False:
        next_pos is there already (begin() set it for the whole prompt; a decode graph's replay
        advances the buffer it lent in place)"""
        self.length += n
        if positions:
            self.next_pos = self.next_pos + n

    def reserve(self, rows: int):
        """room for `rows` rows per sequence, grown in 256-row steps (one copy per 256 decode steps)"""
        if rows > self.max_len:
            self.grow(self.max_len + 256 * -(-(rows - self.max_len) // 256))

    def adopt(self, next_pos, lengths):
        """a decode graph's buffers become next_pos and (ragged) lengths: its replays advance them in
        place (`length` stays the high-water mark, through advance(1, positions=False))"""
        self.next_pos = next_pos
        if self.lengths is not None:
            self.lengths = lengths

    def mark(self):
        """the uniform state release() rewinds to"""
        return self.length, self.next_pos.clone()

    def release(self, mark=None, fed: int = 0):
        """the state generate() returns, out of a decode graph's buffers. Ragged: per row, every real
        token but the row's last is cached (no row advanced on a pad). Uniform: mark() + fed rows --
        every returned token but the last; rows a stopped batch ran past are dropped."""
        if self.lengths is not None:
            self.lengths, self.next_pos = self.lengths.clone(), self.next_pos.clone()
            self.length = int(self.lengths.max())
        else:
            self.length, self.next_pos = mark[0] + fed, mark[1] + fed

    def advance_ragged(self, n_new):
        """the bookkeeping of a ragged step that appended n_new[b] (int [B]) rows to sequence b"""
        self.make_ragged()
        n_new = n_new.to(self.lengths.device)
        self.lengths = self.lengths + n_new.to(torch.int32)
        self.next_pos = self.next_pos + n_new.to(self.next_pos.dtype)
        self.length = int(self.lengths.max())

    def grow(self, max_len: int):
        """re-allocate with room for max_len rows per sequence, keeping the filled rows (a ragged
        cache's rows up to its longest sequence's)"""
        if max_len <= self.max_len:
            return
        k = torch.empty((self.k.shape[0], self.B, max_len, self.k.shape[3]), dtype=self.k.dtype, device=self.k.device)
        v = torch.empty_like(k)
        k[:, :, :self.length].copy_(self.k[:, :, :self.length])
        v[:, :, :self.length].copy_(self.v[:, :, :self.length])
        if self.k_exp is not None:
            ke = torch.empty((self.k_exp.shape[0], self.B, max_len, self.H), dtype=torch.uint8, device=self.k.device)
            ve = torch.empty_like(ke)
            ke[:, :, :self.length].copy_(self.k_exp[:, :, :self.length])
            ve[:, :, :self.length].copy_(self.v_exp[:, :, :self.length])
            self.k_exp, self.v_exp = ke, ve
        self.k, self.v, self.max_len = k, v, max_len

    @classmethod
    def from_legacy(cls, legacy, attention_mask=None, extra: int = 256, kv_dtype: str = "bf16"):
        """A transformers-layout cache -- the legacy tuple of per-layer (key, value) [B, H, L, D]
        (what the reference's decode branch indexes, arch_cullavo.py:608-614) or any object with
        to_legacy_cache() (DynamicCache) -- copied into a KVCache with `extra` free rows.
        Attended keys: the reference's rule (:611-632) -- a cached position whose first-layer
        keys are zero is not attended, nor are the
        left-padding positions of the caller's attention_mask -- which must leave one contiguous
        span per sequence (what the decode kernels read). kv_dtype "fp8" / "fp8_sim" quantises the rows
        on the way in."""
        if hasattr(legacy, "to_legacy_cache"):
            legacy = legacy.to_legacy_cache()
        if not isinstance(legacy, (tuple, list)) or not legacy or len(legacy[0]) != 2:
            raise TypeError(f"past_key_values: expected a KVCache or a transformers legacy cache (tuple of per-layer "
                            f"(key, value) [B, H, L, D]), got {type(legacy).__name__}")
        k0 = legacy[0][0]
        B, H, L, D = k0.shape
        cache = cls(len(legacy), B, L + extra, H, D, k0.device, dtype=k0.dtype, kv_dtype=kv_dtype)
        zero = torch.zeros(B, dtype=torch.int32, device=k0.device)
        for i, (k, v) in enumerate(legacy):
            if k.shape != (B, H, L, D) or v.shape != (B, H, L, D):
                raise ValueError(f"layer {i}: key {tuple(k.shape)} / value {tuple(v.shape)} vs {(B, H, L, D)}")
            if kv_dtype == "bf16":
                cache.k[i, :, :L].copy_(k.transpose(1, 2).reshape(B, L, H * D))
                cache.v[i, :, :L].copy_(v.transpose(1, 2).reshape(B, L, H * D))
            else:
                cache.append(i, k.transpose(1, 2).reshape(B * L, H * D), v.transpose(1, 2).reshape(B * L, H * D),
                             zero, L)
        # a slot is unattended when its first-layer keys are all zero: the reference tests only the
        # head-dim component 0 summed over the heads, which a real key also hits by chance (two
        # bf16 values of opposite sign over 2 heads: seen in the tiny config), so every component
        # is required to vanish here
        att = k0.float().abs().sum((1, 3)) != 0
        if attention_mask is not None:
            if attention_mask.shape[1] >= L:  # a mask over the merged rows
                att &= attention_mask[:, :L].to(k0.device) != 0
            else:  # the caller's text-level mask (:618-632): its leading zeros are the left padding
                lead = (attention_mask.to(torch.int64).cumsum(-1) == 0).sum(-1).to(k0.device)
                att &= torch.arange(L, device=k0.device)[None] >= lead[:, None]
        first, count = left_pad_span(att.to(torch.int64), "KV-cache decode needs one contiguous attended span per "
                                     "sequence (left padding only)")
        cache.begin(first.to(torch.int32), count)
        cache.advance(L, positions=False)
        return cache


def new_chunk_padding(attention_mask, Lnew: int):
    """q_pad of a cached step's new chunk: the number of leading zeros of each row of the mask's last
    Lnew columns (a [B, Lnew] mask of the new tokens or a [B, past + Lnew] one), int32 [B]; None when
    every new token is attended. A row of zeros is allowed (q_pad = Lnew: nothing new for that
    sequence); a zero after a row's first attended new token is refused."""
    if attention_mask.dim() != 2 or attention_mask.shape[1] < Lnew:
        raise ValueError(f"attention_mask {tuple(attention_mask.shape)}: expected [B, >= {Lnew}]")
    new = attention_mask[:, -Lnew:] != 0
    if not bool((~new).any()):
        return None
    lead, _ = left_pad_span(new.to(torch.int64), "a continuation chunk with masked tokens after a row's first "
                            "attended one (left padding only: the cache is compact, a hole has no row)")
    return lead.to(torch.int32)


def _decode_lora(t, M: int, rows: int):
    """The lora= arguments that put a group's LoRA term t into the epilogue of its decode product
    (ops.decode_linear, M rows on a weight of `rows` rows), or None: no adapters, FUSE_DECODE_LORA
    off (read per call: tests patch it), or a group the kernels do not take (LoraTerm.decode_args:
    r != 64, uneven modules), whose term is then materialised as before."""
    if t is None or not FUSE_DECODE_LORA:
        return None
    return t.decode_args(M, rows)


def _nf4_linear(q, x, w, group, residual=None, gemv: bool = False, wide: bool = False):
    """One Linear of the decode step: on the NF4 copy q = (codes, absmax) when the layer has one
    (w goes along, so a shape on which the bf16 GEMV measured faster stays there,
    ops.NF4_BF16_FASTER), else on w. gemv: these are decode rows. The group's LoRA term rides in the
    product's epilogue (_decode_lora; ops.nf4_decode_linear takes the LoraTerm itself and decides the
    same way) or, where it cannot, is materialised and passed as the epilogue addend. wide: the rows
    of a wide step (wide_route): the wide product, the term materialised as its addend."""
    t, _ = group.forward(x, False, 0)
    if q is None:
        la = _decode_lora(t, x.shape[0], w.shape[0]) if gemv else None
        if la is not None:
            return ops.decode_linear(x, w, residual=residual, lora=la)
        if wide and _wide_takes(w, x.shape[0]):
            return ops.decode_linear_wide(x, w, residual=residual, addend=t)
        return ops.linear(x, w, residual=residual, addend=t)
    if t is not None and not FUSE_DECODE_LORA:
        t = t.materialize()
    return ops.nf4_decode_linear(x, q[0], q[1], residual=residual, addend=t, w=w)


def _norm_lora(group, h, norm_w, eps: float, rows: int):
    """FUSE_DECODE_NORMS with adapters: u = RMSNorm(h) A^T by the norm-fused product on the group's
    lora_A stack (one launch, no normalised rows in HBM) and the lora= arguments it gives."""
    if group is NO_LORA:
        return None
    u = ops.decode_linear(h, group.a_stack(), transform=1, norm_w=norm_w, eps=eps)
    la = LoraTerm(group, u).decode_args(h.shape[0], rows)
    if la is None:
        raise RuntimeError("layer_infer: a group that passed decode_fusable() gave no decode arguments")
    return la


# The attention routes of a chunk of new rows: decided once per chunk (by lm_infer's callees and the
# decode graph), taken by every layer of it.
PREFILL = "prefill"            # an empty cache: packed causal attention over the chunk's own rows
CACHED = "cached"              # Lnew > 1 on a filled uniform cache: ops.attn_fwd_cached
RAGGED = "ragged"              # a left-padded block on a ragged cache: kv_append_ragged + attn_fwd_ragged
DECODE_FUSED = "decode_fused"  # one row per sequence: RoPE, append and attention in ops.attn_decode_rope
DECODE = "decode"              # one row per sequence: ops.rope_kv_append, then ops.attn_decode


def decode_route(dtype) -> str:  # dtype: the model's rows (a quantised cache decodes bf16 rows)
    """the route of one new row per sequence (FUSE_DECODE_ROPE is read per call: tests patch it)"""
    return DECODE_FUSED if FUSE_DECODE_ROPE and dtype == torch.bfloat16 else DECODE


def layer_infer(layer, h, sctx: StepContext, cache: KVCache, li: int, route: str, start, kv_len=None, q_pad=None,
                attn_len: int | None = None):
    """One LlamaDecoderLayer over sctx.L new rows per sequence on `route`, appending their keys / values
    to the cache at rows start[b] .. (int32 [B]). No autograd.
    kv_len (int32 [B]): the keys a sequence attends, RAGGED (start + its live rows) and DECODE (start + 1).
    q_pad (int32 [B]): RAGGED -- the rows are a left-padded [B, Lnew] block, sequence b's first q_pad[b]
    rows padding. attn_len: the key range the decode routes' split-KV grid is sized for."""
    cfg = layer.cfg
    d, H, D = cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim
    lg = layer.lora_groups
    B, Lnew = sctx.B, sctx.L
    # the decode rows: one per sequence, few enough for the weight-streaming products
    gemv = Lnew == 1 and h.shape[0] <= 16 and h.dtype == torch.bfloat16
    # 17 .. 64 of them: the wide weight-streaming products (NF4 copies are not read above 16 rows: the
    # arena's dequantised bf16 weights, as before)
    wide = wide_route(B, Lnew, h.dtype)
    # the layer's NF4 weight copies (quant.quantize_lm_nf4_; empty: none, or stale and dropped): the
    # decode rows' products stream 4.5 bits per weight (cullavo_nf4_decode_linear), whatever
    # FUSE_DECODE_NORMS / FUSE_DECODE_SWIGLU say; a weight left bf16 (K % 64 != 0) takes ops.linear
    nf4 = {}
    if NF4_DECODE and gemv:
        from .quant import nf4_weights
        nf4 = nf4_weights(layer)
    # FUSE_DECODE_NORMS: the RMSNorms inside the q|k|v and gate|up weight-streaming products
    # (cullavo_decode_linear transform 1 / 4: every workgroup normalises the rows once into LDS; the
    # round-4 per-fragment form was ~2x slower, profiles/r04/decode/decode_fusions_ab.txt) for the
    # rows that fit LDS (M (d + 8) * 2 <= 64 KiB); FUSE_DECODE_SWIGLU: the SwiGLU in down_proj's
    # X loads (transform 2), only without FUSE_DECODE_GU. All bitwise the unfused values.
    # Adapters (FUSE_DECODE_LORA): every product takes its group's term in its epilogue, so these
    # fusions hold with them; u = T(x) A^T comes from the same transform on the lora_A stack.
    fused = (FUSE_DECODE_NORMS and gemv and h.shape[0] * (d + 8) * 2 <= 65536 and not nf4
             and all(g is NO_LORA or (FUSE_DECODE_LORA and g.decode_fusable()) for g in lg.values()))
    M = h.shape[0]
    if fused:
        norm1 = dict(transform=1, norm_w=layer.input_layernorm.weight, eps=cfg.rms_norm_eps)
        qkv = ops.decode_linear(h, layer.w_qkv(), **norm1,
                                lora=_norm_lora(lg["qkv"], h, norm1["norm_w"], norm1["eps"], 3 * d))
    else:
        x1, _ = ops.rmsnorm_fwd(h, layer.input_layernorm.weight, cfg.rms_norm_eps)
        qkv = _nf4_linear(nf4.get("qkv"), x1, layer.w_qkv(), lg["qkv"], gemv=gemv, wide=wide)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    kc, vc, pos = cache.k[li], cache.v[li], sctx.position_ids
    rope = dict(head_dim=D, theta=cfg.rope_theta)
    attn = dict(B=B, H=H, D=D, scale=D ** -0.5, kv_start=sctx.kv_start)
    # the cache's kv_dtype picks the kernels: "fp8" appends codes + exponents and decodes on them,
    # "fp8_sim" appends the round trip into its bf16 cache and reads it with the bf16 kernels
    quant = cache.kv_dtype != "bf16"
    fp8 = dict(sim=cache.kv_dtype == "fp8_sim") if quant else None
    ke, ve = cache.exps(li)
    if route == PREFILL:
        # attends the forward's own bf16 k, v (as on a bf16 cache); only the cache write quantises
        ops.rope(q, k, pos, hq=H, hk=H, **rope)
        cache.append(li, k, v, start, Lnew)
        o, _ = ops.attn_fwd(q, k, v, Lq=Lnew, Lk=Lnew, causal=True, **attn)
    elif route == CACHED:
        # the new rows against the cached prefix and themselves, causal from the row's own position
        # (an fp8 cache: against the dequantised slab of its live rows, the new ones included)
        ops.rope(q, k, pos, hq=H, hk=H, **rope)
        cache.append(li, k, v, start, Lnew)
        ka, va = cache.attended(li, cache.length + Lnew)
        o, _ = ops.attn_fwd_cached(q, ka, va, Lq=Lnew, past=cache.length, **attn)
    elif route == RAGGED:
        ops.rope(q, k, pos, hq=H, hk=H, **rope)
        cache.append(li, k, v, start, Lnew, q_pad)
        # every kv_len[b] <= max(lengths) + Lnew, known on the host (no read-back); rows past kv_len[b]
        # are never attended, whatever their codes dequantise to
        ka, va = cache.attended(li, min(cache.length + Lnew, cache.max_len))
        o, _ = ops.attn_fwd_ragged(q, ka, va, kv_len, Lq=Lnew, q_pad=q_pad, **attn)
    elif route == DECODE_FUSED:
        if quant:
            o = ops.attn_decode_rope_fp8(q, k, v, pos, kc, vc, ke, ve, start, max_len=attn_len, theta=cfg.rope_theta,
                                         **attn, **fp8)
        else:
            o = ops.attn_decode_rope(q, k, v, pos, kc, vc, start, max_len=attn_len, theta=cfg.rope_theta, **attn)
    elif route == DECODE:
        if quant:
            ops.rope_kv_append_fp8(q, k, v, pos, kc, vc, ke, ve, start, hq=H, B=B, Lnew=1, **rope, **fp8)
        elif qkv.dtype == torch.bfloat16:  # rotated k goes straight to the cache (one launch for RoPE + append)
            ops.rope_kv_append(q, k, v, pos, kc, vc, start, hq=H, B=B, Lnew=1, **rope)
        else:
            ops.rope(q, k, pos, hq=H, hk=H, **rope)
            ops.kv_append(k, v, kc, vc, start, B=B, Lnew=1)
        if cache.kv_dtype == "fp8":
            o = ops.attn_decode_fp8(q, kc, vc, ke, ve, kv_len, max_len=attn_len, **attn)
        else:
            o = ops.attn_decode(q, kc, vc, kv_len, max_len=attn_len, **attn)
    else:
        raise ValueError(f"layer_infer: unknown attention route {route!r}")
    h2 = _nf4_linear(nf4.get("o"), o, layer.self_attn.o_proj.weight, lg["o"], residual=h, gemv=gemv, wide=wide)
    w_gu, w_down = layer.w_gu(), layer.mlp.down_proj.weight
    F2 = w_gu.shape[0]
    if fused:
        norm2 = dict(norm_w=layer.post_attention_layernorm.weight, eps=cfg.rms_norm_eps)
        la = _norm_lora(lg["gu"], h2, norm2["norm_w"], norm2["eps"], F2)
        if FUSE_DECODE_GU:  # RMSNorm, gate|up product and SwiGLU in one launch (transform 4)
            a = ops.decode_linear(h2, w_gu, transform=4, **norm2, lora=la)
            return _nf4_linear(None, a, w_down, lg["down"], residual=h2, gemv=True)
        gu = ops.decode_linear(h2, w_gu, transform=1, **norm2, lora=la)
        if FUSE_DECODE_SWIGLU:
            ld = None
            if lg["down"] is not NO_LORA:  # u = SwiGLU(gu) A^T by the same fused X loads
                ld = LoraTerm(lg["down"], ops.decode_linear(gu, lg["down"].a_stack(), transform=2)).decode_args(M, d)
            return ops.decode_linear(gu, w_down, transform=2, residual=h2, lora=ld)
        return _nf4_linear(None, ops.swiglu_fwd(gu), w_down, lg["down"], residual=h2, gemv=True)
    x2, _ = ops.rmsnorm_fwd(h2, layer.post_attention_layernorm.weight, cfg.rms_norm_eps)
    t, _ = lg["gu"].forward(x2, False, 0)
    la = _decode_lora(t, M, F2) if gemv else None
    # gate|up product (+ the adapters' term) + SwiGLU in one launch of the bf16 GEMV: a layer without an
    # NF4 copy, or adapters on a shape where that GEMV measured faster than the NF4 product
    one_launch = gemv and FUSE_DECODE_GU and (t is None or la is not None)
    if "gu" in nf4:
        one_launch = one_launch and t is not None and ops.nf4_prefers_bf16(F2, d, M)
    if one_launch:
        a = ops.decode_linear(x2, w_gu, transform=3, lora=la)
    elif "gu" in nf4:
        if t is None:  # gate|up product + SwiGLU in one launch
            a = ops.nf4_decode_linear(x2, *nf4["gu"], swiglu_out=True, w=w_gu)
        else:
            # adapters on the NF4 product: the term in its epilogue, the SwiGLU its own launch (an adapter
            # model's NF4 calls carry an addend and no SwiGLU output: tests/test_nf4.py pins that)
            a = ops.swiglu_fwd(ops.nf4_decode_linear(x2, *nf4["gu"], w=w_gu,
                                                     addend=t if FUSE_DECODE_LORA else t.materialize()))
    elif la is not None:
        a = ops.swiglu_fwd(ops.decode_linear(x2, w_gu, lora=la))
    elif wide and F2 % 16 == 0 and _wide_takes(w_gu, M):
        # the wide product with the SwiGLU in its epilogue; adapters: their term as the addend of the
        # plain product, then the SwiGLU's own launch
        if t is None and FUSE_DECODE_GU:
            a = ops.decode_linear_wide(x2, w_gu, transform=3)
        else:
            a = ops.swiglu_fwd(ops.decode_linear_wide(x2, w_gu, addend=t))
    else:
        a = ops.swiglu_fwd(ops.linear(x2, w_gu, addend=t))
    return _nf4_linear(nf4.get("down"), a, w_down, lg["down"], residual=h2, gemv=gemv, wide=wide)


SAMPLE_TOP_K_MAX = 1024  # cullavo_sample_token: 1 <= top_k <= 1024


def device_sampling(*, do_sample: bool, temperature: float, top_k: int, top_p: float, generator, seed,
                    device_loop) -> bool:
    """Whether generate() runs its device loop (the sampling kernel, captured into the decode graph)
    or today's host loop around sample_next: the device loop runs when a seed is given (sampling) or
    device_loop=True (greedy, or sampling with a seed); a call with neither runs the host loop.
    Raises ValueError for the combinations neither loop serves."""
    if seed is None and not device_loop:
        return False
    if seed is not None:
        if generator is not None:
            raise ValueError("generate(): seed= (the device loop's Philox streams) and generator= (the host loop's "
                             "torch.Generator) exclude each other")
        if not do_sample:
            raise ValueError("generate(): seed= needs do_sample=True (greedy decoding draws nothing)")
        if device_loop is not None and not device_loop:
            raise ValueError("generate(): seed= runs the device loop; device_loop=False has no seeded sampling "
                             "(pass generator= instead)")
        if not isinstance(top_k, int) or not 1 <= top_k <= SAMPLE_TOP_K_MAX:
            raise ValueError(f"generate(): seed= samples with the device kernel, which takes 1 <= top_k <= "
                             f"{SAMPLE_TOP_K_MAX} (got {top_k}; top_k=0, the nucleus over the full vocabulary, runs "
                             f"on the host loop with generator=)")
        if not (temperature > 0 and temperature < float("inf")) or not 0 < top_p <= 1:
            raise ValueError(f"generate(): temperature must be finite and > 0 and top_p in (0, 1] "
                             f"(got {temperature}, {top_p})")
    elif do_sample:
        raise ValueError("generate(): device_loop=True with do_sample=True needs seed= (the device loop does not "
                         "read a torch.Generator)")
    if generator is not None:
        raise ValueError("generate(): device_loop=True does not take generator=")
    return True


class SamplerState:
    """The device state of one generation on the sampling kernel (ops.sample_token) and its
    parameters: next_ids [B] (the token the next decode step embeds), step [B] (tokens produced, the
    Philox counter), row_offset [B] (each sequence's stream id: with seed it fixes the sequence's
    draws whatever the batch around it), finished [B] and out_tokens [B, max_new_tokens]."""

    def __init__(self, B: int, max_new_tokens: int, device, *, do_sample: bool, temperature: float = 1.0,
                 top_k: int = 50, top_p: float = 1.0, seed: int = 0, eos_token_id: int | None = None,
                 pad_token_id: int = 0, row_offset=None):
        self.next_ids = torch.zeros(B, dtype=torch.int64, device=device)
        self.step = torch.zeros(B, dtype=torch.int64, device=device)
        if row_offset is None:
            self.row_offset = torch.arange(B, dtype=torch.int64, device=device)
        else:
            self.row_offset = torch.as_tensor(row_offset).to(device=device, dtype=torch.int64).reshape(-1).contiguous()
            if self.row_offset.numel() != B:
                raise ValueError(f"sample_offsets: expected {B} stream ids, got {self.row_offset.numel()}")
        self.finished = torch.zeros(B, dtype=torch.uint8, device=device)
        self.out_tokens = torch.full((B, max_new_tokens), pad_token_id, dtype=torch.int64, device=device)
        self.do_sample = bool(do_sample)
        # greedy ignores the warpers; the kernel still validates them
        self.temperature, self.top_k, self.top_p = (temperature, top_k, top_p) if do_sample else (1.0, 1, 1.0)
        self.seed, self.eos_token_id, self.pad_token_id = int(seed), eos_token_id, int(pad_token_id)

    def sample(self, logits):
        """one token per row from logits [B, V] (bf16, a row-strided view): everything in place"""
        ops.sample_token(logits, next_ids=self.next_ids, step=self.step, temperature=self.temperature,
                         top_k=self.top_k, top_p=self.top_p, do_sample=self.do_sample, seed=self.seed,
                         row_offset=self.row_offset, eos_id=self.eos_token_id, pad_id=self.pad_token_id,
                         finished=self.finished, out_tokens=self.out_tokens)

    def tokens(self, n: int):
        """the first n tokens produced, [B, n]"""
        return self.out_tokens[:, :n].clone()


class HostSampler:
    """SamplerState's surface for generate()'s host path: sample_next (torch ops drawing from the
    caller's torch.Generator) plus the finished / pad bookkeeping; no kernel, no Philox state."""

    def __init__(self, B: int, device, *, eos_token_id: int | None, pad_token_id: int, **warpers):
        self.finished = torch.zeros(B, dtype=torch.bool, device=device)
        self.next_ids, self.new = None, []
        self.eos_token_id, self.pad_token_id, self.warpers = eos_token_id, pad_token_id, warpers

    def sample(self, logits):
        tok = sample_next(logits, **self.warpers)
        tok = torch.where(self.finished, torch.full_like(tok, self.pad_token_id), tok)
        self.new.append(tok)
        if self.eos_token_id is not None:
            self.finished |= tok == self.eos_token_id
        self.next_ids = tok

    def tokens(self, n: int):
        return torch.stack(self.new[:n], 1)


class DecodeGraph:
    """One cached decode step of the LM -- the new token's embedding row, every decoder layer at one
    row per sequence, the final norm and lm_head -- captured once as a HIP graph and replayed per
    token (about 330 kernel launches per 7B step; replayed, the host no longer issues them one by
    one). Everything the step reads that changes from token to token lives in device buffers the
    graph owns and advances itself: the token ids (written by the caller before each replay), the
    RoPE positions and the cache write row (+1 at the end of every replay); decode attention runs
    over the cache's full capacity (chunks past a row's length exit at once), so the grid does not
    depend on the current length. The cache must not grow while the graph is alive (generate()
    sizes it for prompt + max_new_tokens).
    With a sampler (SamplerState) the captured step ends with the sampling kernel on its logits and
    reads its token from the sampler's next_ids, which that kernel wrote one replay earlier:
    advance() replays with no host-to-device token copy. Without one the graph is what it was.
    On a ragged cache `start` begins at cache.lengths (the per-row start[b] is what the decode kernels
    take) and becomes cache.lengths, as `pos` becomes cache.next_pos. live=True adds a [B] int32 buffer
    `live`: the captured step ends with pos += live, start += live instead of += 1, so a row whose
    live[b] is 0 appends nothing (its key / value land on the scratch row start[b], which the next
    live step overwrites). With a sampler the step sets live = ~finished itself, before it samples;
    without one the caller writes `live` before each step()."""

    def __init__(self, model, cache: KVCache, sampler: SamplerState | None = None, live: bool = False):
        lm = model.language_model
        self.cache, self.lm = cache, lm
        B = cache.B
        dev = cache.k.device
        self.sampler = sampler
        self.ids = sampler.next_ids if sampler is not None else torch.zeros(B, dtype=torch.long, device=dev)
        self.pos = cache.next_pos.to(torch.int64).clone()
        if cache.lengths is not None:
            self.start = cache.lengths.to(torch.int32).clone()
        else:
            self.start = torch.full((B,), cache.length, dtype=torch.int32, device=dev)
        self.live = torch.ones(B, dtype=torch.int32, device=dev) if live else None
        self.embed = model.get_input_embeddings()
        # the captured kernels hold raw pointers into the layers' NF4 copies: keep the tensors alive
        # for the graph's lifetime even if quant.nf4_weights() drops them from the layers meanwhile
        from .quant import nf4_weights
        self.nf4_refs = [nf4_weights(layer) for layer in lm.model.layers] if NF4_DECODE else []
        # and into the cache's storage (an fp8 cache: codes and exponents): a grow() meanwhile must not free it
        self.kv_refs = (cache.k, cache.v, cache.k_exp, cache.v_exp)
        # adapters: the captured products read lora_A / lora_B (FUSE_DECODE_LORA: in their epilogues, the
        # same route as the eager step, decided by layer_infer at capture) straight from the LoRA arena,
        # whose storage the model owns and never reallocates: it outlives the graph, and a replay after a
        # training step computes with the adapters as that step left them
        self.graph = torch.cuda.CUDAGraph()
        self.steps_left = cache.max_len - cache.length
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        traced = ops._TRACE["key"]
        ops._TRACE["key"] = None  # no per-launch timing events inside the captured graph
        try:
            with torch.cuda.stream(stream):
                with torch.cuda.graph(self.graph, stream=stream, capture_error_mode="thread_local"):
                    self.logits = self._step()
        finally:
            ops._TRACE["key"] = traced
        torch.cuda.current_stream(dev).wait_stream(stream)
        cache.adopt(self.pos, self.start)  # advanced in place by every replay

    def _step(self):
        lm, cache = self.lm, self.cache
        B = cache.B
        if self.live is not None and self.sampler is not None:
            # a row advances until the step that would feed its eos: `finished` as the sampling kernel
            # left it one replay earlier, read before this step's sampling changes it
            self.live.copy_(self.sampler.finished == 0)
        h = self.embed(self.ids[:, None]).reshape(B, lm.cfg.hidden_size)
        sctx = StepContext(B, 1, self.pos[:, None], cache.kv_start, lora_seed=0)
        logits = run_chunk(lm, h, sctx, cache, decode_route(h.dtype), self.start, attn_len=cache.max_len)
        if self.sampler is not None:  # the next step's token, written where this graph's embedding reads it
            self.sampler.sample(logits)
        n = self.live if self.live is not None else 1
        self.pos.add_(n)
        self.start.add_(n)
        return logits.view(B, 1, -1)

    def _replay(self):
        if self.steps_left <= 0:
            raise ValueError("decode graph: the KV cache is full")
        self.graph.replay()
        self.cache.advance(1, positions=False)
        self.steps_left -= 1

    def advance(self):
        """One replay of a graph with a sampler: the token the sampler holds is appended to the cache
        and the kernel at the graph's end samples the next one (no host-to-device copy, no host read)."""
        if self.sampler is None:
            raise ValueError("decode graph: advance() needs a graph captured with a sampler (use step(tokens))")
        self._replay()

    def step(self, tokens):
        """Append `tokens` ([B] ids) to the cache and return the next logits [B, 1, V] (a view of
        the graph's output buffer, overwritten by the next replay)."""
        if self.sampler is not None:
            raise ValueError("decode graph: a graph captured with a sampler picks its own tokens (use advance())")
        self.ids.copy_(tokens.reshape(-1))
        self._replay()
        return self.logits


class DecodeStepper:
    """generate()'s decode step, graph or eager behind one call: feed(sampler) appends the sampler's
    next_ids (one token per row) to the cache and leaves the sampler holding the token after it. With
    graph=True a DecodeGraph is captured -- around the sampling kernel when the sampler is a
    SamplerState (advance(): no host-to-device token copy), else replayed by step(tokens) with the host
    sampler in between; otherwise every step is model._forward_cached. compact: a finished row (its eos
    included) is fed but does not advance (the ragged cache's `live` mask)."""

    def __init__(self, model, cache: KVCache, sampler, *, graph: bool, compact: bool):
        self.model, self.cache, self.compact = model, cache, compact
        self.in_graph = graph and isinstance(sampler, SamplerState)
        self.graph = None
        if graph:
            self.graph = DecodeGraph(model, cache, sampler=sampler if self.in_graph else None, live=compact)

    def feed(self, sampler):
        if self.in_graph:
            return self.graph.advance()
        live = sampler.finished == 0 if self.compact else None
        if self.graph is not None:
            if live is not None:
                self.graph.live.copy_(live)
            logits = self.graph.step(sampler.next_ids)
        else:
            cfg = self.model.config
            logits = self.model._forward_cached(sampler.next_ids[:, None], None,
                                                live[:, None].to(torch.long) if live is not None else None, None,
                                                self.cache, None, cfg.vision_feature_layer,
                                                cfg.vision_feature_select_strategy, None, True).logits
        sampler.sample(logits[:, -1])


def run_chunk(lm, h, sctx: StepContext, cache: KVCache, route: str, start, q_pad=None, live_rows=None,
              attn_len: int | None = None):
    """One chunk of new rows h [B * sctx.L, d] through the LM on one attention route: every decoder
    layer, the final RMSNorm, lm_head; logits [B * sctx.L, V]. The rows' keys / values go to cache rows
    start[b] ..; the caller advances the cache. live_rows (RAGGED): the rows sequence b really appends."""
    kv_len = None
    if route == RAGGED:
        kv_len = start + live_rows
    elif route == DECODE:  # the unfused decode attention reads its key count (the fused one derives it)
        kv_len = start + 1
    for li, layer in enumerate(lm.model.layers):
        h = layer_infer(layer, h, sctx, cache, li, route, start, kv_len, q_pad, attn_len)
    x, _ = ops.rmsnorm_fwd(h, lm.model.norm.weight, lm.cfg.rms_norm_eps)
    if wide_route(sctx.B, sctx.L, x.dtype) and _wide_takes(lm.lm_head.weight, x.shape[0]):
        return ops.decode_linear_wide(x, lm.lm_head.weight)
    return ops.linear(x, lm.lm_head.weight)


def _infer_rows(lm, embeds, position_ids, cache: KVCache, positions: bool):
    """A chunk embeds [B, Lnew, d] appended to a uniform cache at cache.length; logits [B, Lnew, V].
    positions: whether the chunk moves cache.next_pos (KVCache.advance)."""
    B, Lnew, d = embeds.shape
    sctx = StepContext(B, Lnew, position_ids, cache.kv_start, lora_seed=0)
    h = embeds.reshape(B * Lnew, d).contiguous()
    start = torch.full((B,), cache.length, dtype=torch.int32, device=h.device)
    if Lnew == 1:
        route = decode_route(h.dtype)
    else:
        route = CACHED if cache.length > 0 else PREFILL
    logits = run_chunk(lm, h, sctx, cache, route, start, attn_len=cache.length + 1)
    cache.advance(Lnew, positions)
    return logits.view(B, Lnew, -1)


def _infer_ragged(lm, embeds, q_pad, position_ids, cache: KVCache, prefill_chunk: int | None):
    """lm_infer's ragged branch: embeds [B, Lnew, d] is a left-padded block whose first q_pad[b] rows
    of sequence b are padding (q_pad None: none), appended to a cache that is, or hereby becomes,
    ragged. Returns logits [B, Lnew, V]; the padding rows' logits mean nothing."""
    B, Lnew, d = embeds.shape
    dev = embeds.device
    cache.make_ragged()
    q_pad = (torch.zeros(B, dtype=torch.int32, device=dev) if q_pad is None
             else q_pad.to(device=dev, dtype=torch.int32))
    # one token per sequence takes a decode route at start = lengths, as the decode graph does: a
    # padding row's key / value land on the scratch row behind its length and it does not advance
    decode = Lnew == 1
    cache.reserve(cache.length + 1 if decode else int((cache.lengths + (Lnew - q_pad)).max()))
    if position_ids is None:
        # position next_pos[b] + i - q_pad[b] on the live rows, any finite value on the padding
        position_ids = (cache.next_pos[:, None] + torch.arange(Lnew, device=dev) - q_pad[:, None]).clamp_(min=0)
    if decode:
        position_ids = torch.where(q_pad[:, None] > 0, cache.next_pos[:, None], position_ids)
    route = decode_route(embeds.dtype) if decode else RAGGED
    step = Lnew if prefill_chunk is None else prefill_chunk
    if step < 1:
        raise ValueError(f"prefill_chunk must be positive, got {prefill_chunk}")
    logits = []
    for c in range(0, Lnew, step):
        # a piece is columns c .. c + w of the block, its padding the part of q_pad inside it
        w = min(step, Lnew - c)
        qp = (q_pad - c).clamp_(0, w)
        sctx = StepContext(B, w, position_ids[:, c:c + w], cache.kv_start, lora_seed=0)
        h = embeds[:, c:c + w].reshape(B * w, d).contiguous()
        logits.append(run_chunk(lm, h, sctx, cache, route, cache.lengths, qp, w - qp,
                                attn_len=cache.length + 1).view(B, w, -1))
        cache.advance_ragged(w - qp)
    return logits[0] if len(logits) == 1 else torch.cat(logits, 1)


def lm_infer(lm, embeds, attention_mask, position_ids, cache: KVCache | None, max_len: int,
             prefill_chunk: int | None = None, kv_dtype: str = "bf16"):
    """LlamaForCausalLM with a KV cache: prefill (cache None or empty), one decode step, or a
    continuation of Lnew > 1 new tokens per sequence on a filled cache (a follow-up turn, a second
    question about the cached image, the later pieces of a chunked prefill). prefill_chunk: run the
    rows in pieces of at most that many per sequence (None: one pass). Returns (logits [B, Lnew, V]
    bf16, cache). kv_dtype: the format of the cache created here when `cache` is None (an existing
    cache keeps its own)."""
    B, Lnew, d = embeds.shape
    cfg = lm.cfg
    if embeds.dtype != torch.bfloat16:
        raise NotImplementedError("KV-cache decode runs on the bf16 model (the f32 mode is a parity mode)")
    if cache is None:
        cache = KVCache(cfg.num_hidden_layers, B, max_len, cfg.num_attention_heads, cfg.head_dim, embeds.device,
                        kv_dtype=kv_dtype)
    prefill = cache.length == 0
    if prefill:
        if Lnew > cache.max_len:  # kv_append writes rows [0, Lnew) of every sequence's cache
            raise ValueError(f"prompt of {Lnew} rows does not fit the KV cache ({cache.max_len} rows)")
        if attention_mask is None:
            attention_mask = torch.ones(B, Lnew, dtype=torch.long, device=embeds.device)
        am = attention_mask.to(torch.int64)
        first, _ = left_pad_span(am, "KV-cache generation needs left padding (no masked tokens after the first "
                                 "attended one)")
        if position_ids is None:
            position_ids = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
        cache.begin(first.to(torch.int32), position_ids[:, -1].to(torch.int64) + 1)
    else:
        # a ragged cache: any chunk (one token per sequence included) takes the ragged branch. A uniform
        # one: a 2-D mask ending in the new tokens (past + new rows, or the new ones alone) -- the cached
        # part is the cache's own state (kv_start); zeros in the new part may only lead a row (a
        # left-padded turn, which makes the cache ragged); all ones is the uniform step below
        q_pad = None
        if attention_mask is not None and (cache.lengths is not None or Lnew > 1):
            q_pad = new_chunk_padding(attention_mask, Lnew)
        if cache.lengths is not None or q_pad is not None:
            return _infer_ragged(lm, embeds, q_pad, position_ids, cache, prefill_chunk), cache
        cache.reserve(cache.length + Lnew)
        if position_ids is None:
            position_ids = cache.next_pos[:, None]
            if Lnew > 1:
                position_ids = position_ids + torch.arange(Lnew, device=embeds.device)
    # pieces of at most prefill_chunk rows: the first on the empty cache as a plain prefill, the
    # others as continuations (kv_start masks a sequence's left padding in every piece)
    step = Lnew
    if prefill_chunk is not None and Lnew > prefill_chunk:
        if prefill_chunk < 1:
            raise ValueError(f"prefill_chunk must be positive, got {prefill_chunk}")
        step = prefill_chunk
    logits = [_infer_rows(lm, embeds[:, c:c + step], position_ids[:, c:c + step], cache, positions=not prefill)
              for c in range(0, Lnew, step)]
    return (logits[0] if len(logits) == 1 else torch.cat(logits, 1)), cache


def sample_next(logits, *, do_sample: bool, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                generator=None):
    """HF's warper order (temperature -> top-k -> top-p) then multinomial; argmax when greedy."""
    if not do_sample:
        return logits.argmax(-1)
    x = logits.float()
    if temperature != 1.0:
        x = x / temperature
    if top_k and top_k > 0:
        kth = torch.topk(x, min(top_k, x.shape[-1]), dim=-1).values[..., -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    if top_p < 1.0:
        sx, si = torch.sort(x, descending=False, dim=-1)
        cum = sx.softmax(-1).cumsum(-1)
        remove = cum <= (1 - top_p)
        remove[..., -1:] = False
        x = x.masked_fill(remove.scatter(-1, si, remove), float("-inf"))
    return torch.multinomial(x.softmax(-1), 1, generator=generator).squeeze(-1)
