"""CuLLaVOModel: drop-in for the reference's model class (reference cullavo/arch_cullavo.py:24,
546-677) whose dense math runs on the gfx950 kernels.

Same constructor-visible structure (.vision_tower, .multi_modal_projector, .language_model with
.model/.lm_head, .get_input_embeddings(), .config), same forward signature, same
CullavoCausalLMOutputWithPast result (tuple form when return_dict=False) and the same
ValueError for an unknown vision_feature_select_strategy.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Optional, Tuple

import torch
from torch import nn

from . import ops
from .config import CuLLaVOConfig
from .functions import HeadLossFn, HeadLossRowsFn, MergeFn, PackRowsFn, StepContext, UnpackRowsFn
from .lora import NO_LORA, LoraSettings
from .packed import check_no_holes, mask_counts, packed_plan
from .modeling import (CLIPVisionModel, LlamaForCausalLM, LlavaMultiModalProjector, build_arenas, init_random_)


@dataclass
class CullavoCausalLMOutputWithPast:
    """reference cullavo/arch_cullavo.py:14-21"""
    loss: Optional[torch.Tensor] = None
    logits: torch.Tensor = None
    past_key_values: Optional[list] = None
    hidden_states: Optional[Tuple[torch.Tensor]] = None
    attentions: Optional[Tuple[torch.Tensor]] = None
    image_hidden_states: Optional[Tuple[torch.Tensor]] = None

    def __getitem__(self, k):
        if isinstance(k, str):
            return getattr(self, k)
        return self.to_tuple()[k]

    def to_tuple(self):
        return tuple(getattr(self, f.name) for f in fields(self) if getattr(self, f.name) is not None)


@dataclass
class CullavoGenerateOutput:
    """generate(return_dict_in_generate=True): HF's GenerateDecoderOnlyOutput names. As there, the
    cache holds every token of `sequences` but the last sampled one."""
    sequences: torch.Tensor = None
    past_key_values: object = None


class CuLLaVOModel(nn.Module):
    def __init__(self, config: CuLLaVOConfig, *, device="cuda", trainable: str = "full", init: str = "random",
                 seed: int = 0, lora: LoraSettings | None = None, dtype=torch.bfloat16):
        """trainable: "full" | "reference" | "lora" | "none" (modeling.TRAINABLE_POLICIES); "lora"
        adds the reference's peft adapters (lora.LoraSettings, default r=64, alpha=16, p=0.05).
        dtype: torch.bfloat16 (production: the reference's bf16-cast model under bf16 autocast,
        reference cullavo/load_cullavo.py:123-126) or torch.float32 (the parity mode: every
        parameter, activation and kernel operand f32, nothing rounded to bf16)."""
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"dtype {dtype}: bf16 (production) or float32 (parity mode)")
        super().__init__()
        self.dtype = dtype
        if config.vision_config.hidden_act != "quick_gelu" or config.projector_hidden_act != "gelu":
            raise ValueError("CuLLaVO path: CLIP quick_gelu + projector gelu")
        self.config = config
        if trainable == "lora" and lora is None:
            lora = LoraSettings()
        self.lora_settings = lora if trainable == "lora" else None
        self.arenas = build_arenas(config, device, trainable, dtype=dtype, lora=self.lora_settings)
        if init == "random":
            init_random_(self.arenas, seed)
        la = (self.arenas["lora"], self.lora_settings) if "lora" in self.arenas else None
        self.vision_tower = CLIPVisionModel(config.vision_config, self.arenas["vision"], la)
        self.multi_modal_projector = LlavaMultiModalProjector(self.arenas["projector"].params)
        self.language_model = LlamaForCausalLM(config.text_config, self.arenas["embed"], self.arenas["layers"],
                                               self.arenas["head"], la)
        self.trainable_policy = trainable
        # the trainer's opt-in to the supervised-row tail (forward's num_supervised); off, every caller
        # gets the full logits
        self.supervised_rows = False
        # the trainer's opt-in to the packed step: a batch with padding runs the decoder layers and the
        # head on its attended rows only (forward's docstring). Off, every row of [B, L] is run.
        self.packed_rows = False
        # rows per piece of a cached forward's prefill (None: one pass; generate(prefill_chunk=N))
        self.prefill_chunk = None
        # the KV cache a cached forward / generate() creates when the call does not say (kv_cache_dtype=):
        # "bf16", "fp8" (e4m3 codes with a power-of-two scale per token and head, half the bytes) or
        # "fp8_sim" (fp8's numerics on a bf16 cache); generation.KVCache
        self.kv_cache_dtype = "bf16"

    @classmethod
    def from_pretrained(cls, path: str, *, device="cuda", trainable: str = "full", lora: LoraSettings | None = None,
                        load_in_4bit: bool = False, **kw) -> "CuLLaVOModel":
        """llava-hf checkpoint directory (config.json + *.safetensors, ~4.37 or >= 4.45 key
        layout) -> model, streamed into HBM (reference cullavo/load_cullavo.py:86).
        load_in_4bit: the reference's prepare_cullavo(bits=4) numerics (load_cullavo.py:66-83): the
        decoder layers' Linear weights become NF4 after loading (quant.quantize_lm_nf4_; lm_head,
        projector and vision tower stay bf16); the report is kept as model.nf4_report."""
        from .checkpoint import load_llava_safetensors
        m = cls(CuLLaVOConfig.from_json(path), device=device, trainable=trainable, init="none", lora=lora)
        if "lora" in m.arenas:
            from .lora import init_lora_
            init_lora_(m.arenas["lora"], kw.get("seed", 0))
        load_llava_safetensors(m, path)
        if load_in_4bit:
            from .quant import quantize_lm_nf4_
            m.nf4_report = quantize_lm_nf4_(m)
        return m

    # -- reference API -------------------------------------------------------------------------
    # ---- data step (reference cullavo/arch_cullavo.py:28-339, 397-543) ----
    @staticmethod
    def make_system_prompt(processor, device, ignore_index):
        from .prompting import make_system_prompt
        return make_system_prompt(processor, device, ignore_index)

    @staticmethod
    def make_and_add_prompt_and_label(cullavo_prompt, cullavo_label, prompt, answer, processor, device, ignore_index):
        from .prompting import make_and_add_prompt_and_label
        return make_and_add_prompt_and_label(cullavo_prompt, cullavo_label, prompt, answer, processor, device,
                                             ignore_index)

    def step1_process(self, inputs, processor, device, fix_num=5):
        """reference cullavo/arch_cullavo.py:96-339 (prompting.step1_process; boxes drawn on the GPU)"""
        from .prompting import step1_process
        return step1_process(inputs, processor, device, self.config.ignore_index, fix_num)

    def step2_process(self, batched_inputs, processor, device):
        from .prompting import step2_process
        return step2_process(batched_inputs, processor, device, self.config.ignore_index,
                             self.config.vision_config.image_size)

    def step2_preprocess(self, batched_inputs, processor, device, **kw):
        """reference cullavo/arch_cullavo.py:341-395 (prompting.step2_preprocess, on generate())"""
        from .prompting import step2_preprocess
        return step2_preprocess(self, batched_inputs, processor, device, **kw)

    def eval_process(self, images, aux_prompt=None, prompt=None, processor=None, device=None):
        from .prompting import eval_process
        return eval_process(images, aux_prompt, prompt, processor, device, self.config.ignore_index)

    def get_input_embeddings(self):
        return self.language_model.model.embed_tokens

    def get_output_embeddings(self):
        return self.language_model.lm_head

    def to(self, *a, **k):  # parameters are views into HBM arenas: moving would break them
        raise RuntimeError("CuLLaVOModel lives where it was built (pass device= to the constructor)")

    def zero_grad(self, set_to_none: bool = False):
        for ar in self.arenas.values():
            ar.zero_grad()

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Load llava-hf (transformers ~4.37) keys; copies into the arenas in place. peft-wrapped
        keys (`<linear>.base_layer.weight`) map to the base weight."""
        own = {}
        for ar in self.arenas.values():
            own.update(ar.params)
        state_dict = {k.replace(".base_layer.", "."): v for k, v in state_dict.items()}
        missing = [k for k in own if k not in state_dict]
        unexpected = [k for k in state_dict if k not in own]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:5]}..., unexpected {unexpected[:5]}...")
        with torch.no_grad():
            for k, v in state_dict.items():
                if k in own:
                    own[k].copy_(v.to(own[k].dtype))
        return missing, unexpected

    def state_dict(self, *a, **k):
        out = {}
        for ar in self.arenas.values():
            out.update({key: p.detach() for key, p in ar.params.items()})
        return out

    # -- forward (reference cullavo/arch_cullavo.py:546-677) ------------------------------------
    def forward(self, input_ids=None, pixel_values=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, vision_feature_layer=None, vision_feature_select_strategy=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                num_supervised: int | None = None, attended_lens=None, kv_cache_dtype: str | None = None):
        """kv_cache_dtype (with use_cache / past_key_values only): the format of the KV cache this call
        creates -- None: self.kv_cache_dtype; a KVCache passed as past_key_values keeps its own format and
        a conflicting value raises ValueError.
        num_supervised: host-side upper bound of the number of label positions of this batch (counted
        where the batch is built). With self.supervised_rows set (the trainer's opt-in) the loss then
        comes from those rows only and the output carries no logits.
        With self.packed_rows set, a batch with padding is packed: embeddings, the image merge, position
        ids, the mask and the shifted targets are built on the padded grid as always, then the attended
        rows are gathered sequence by sequence, the decoder layers run the varlen attention on [T, d] and
        the head runs on those rows. loss is the padded path's (padding never carried a target); logits
        are [B, L, V] with ZEROS at the positions that are not attended. The per-sequence attended counts
        come to the host with the merge's own read-back; a text-only batch passes them as attended_lens
        (host ints, counted where the batch is built, as num_supervised is; without them the batch runs
        padded) and is trusted to have no hole in its mask. output_hidden_states and a batch without
        padding run the padded path; a mask with a hole raises ValueError; the f32 parity mode raises
        NotImplementedError. LoRA dropout masks are keyed by the packed row, so equality with the padded
        run holds at dropout 0 only. With supervised_rows as well, the tail's rows are packed rows."""
        cfg = self.config
        output_hidden_states = output_hidden_states if output_hidden_states is not None else cfg.output_hidden_states
        return_dict = return_dict if return_dict is not None else cfg.use_return_dict
        vision_feature_layer = vision_feature_layer if vision_feature_layer is not None else cfg.vision_feature_layer
        strategy = (vision_feature_select_strategy if vision_feature_select_strategy is not None
                    else cfg.vision_feature_select_strategy)
        if past_key_values is not None or use_cache:
            return self._forward_cached(input_ids, pixel_values, attention_mask, position_ids, past_key_values,
                                        inputs_embeds, vision_feature_layer, strategy, labels, return_dict,
                                        kv_cache_dtype=kv_cache_dtype)
        if kv_cache_dtype is not None:
            raise ValueError("kv_cache_dtype goes with use_cache=True or past_key_values (this forward keeps no cache)")
        if output_attentions:
            raise NotImplementedError("flash attention never materialises attention probabilities")

        self.vision_tower.eval()  # :578 (no dropout in this tower; kept for parity of intent)
        if self.packed_rows and self.dtype != torch.bfloat16:
            raise NotImplementedError("packed_rows runs the bf16 varlen attention; the f32 parity mode is not packed")

        if inputs_embeds is None:
            B, S = input_ids.shape
            inputs_embeds = self.get_input_embeddings()(input_ids)  # :582
            if pixel_values is not None and S != 1:
                # read back while the tower runs (packed step: the per-row counts ride along)
                stats = self._merge_stats_async(input_ids, attention_mask if self.packed_rows else None)
                image_features = self._image_features(pixel_values, vision_feature_layer, strategy)  # :586-599
                inputs_embeds, attention_mask, position_ids = self._merge(image_features, inputs_embeds, input_ids,
                                                                          attention_mask, stats)  # :600-602
                if self.packed_rows:
                    attended_lens = self._merged_lens(stats[0], B, image_features.shape[1])
                if labels is None:  # :603-604
                    labels = torch.full_like(attention_mask, cfg.ignore_index).to(torch.long)
        B, L, d = inputs_embeds.shape
        if position_ids is None:
            position_ids = torch.arange(L, device=inputs_embeds.device).expand(B, L)
        kv_start = None
        if attention_mask is not None:
            kv_start = (attention_mask.cumsum(-1) == 0).sum(-1).to(torch.int32)
        plan = self._packed_plan(attention_mask, attended_lens, B, L, output_hidden_states)
        if plan is not None:
            return self._forward_packed(inputs_embeds, labels, attention_mask, position_ids, plan, num_supervised,
                                        return_dict)
        sctx = StepContext(B, L, position_ids, kv_start)
        lm = self.language_model
        n_rows = self._tail_rows(num_supervised, labels, B, L, output_hidden_states)
        if n_rows:
            return self._forward_supervised_rows(inputs_embeds, labels, attention_mask, sctx, n_rows, return_dict)
        h, hs = lm.decode(inputs_embeds.reshape(B * L, d).contiguous(), sctx, bool(output_hidden_states))  # :638
        loss = None
        if labels is not None:  # :651-665
            if labels.shape != (B, L):  # the reference's masked / shifted indexing raises here
                if attention_mask is not None:
                    raise IndexError(f"The shape of the mask [{B}, {L - 1}] at index 1 does not match the shape of "
                                     f"the indexed tensor [{labels.shape[0]}, {labels.shape[-1] - 1}] at index 1")
                raise ValueError(f"Expected input batch_size ({B * (L - 1)}) to match target batch_size "
                                 f"({labels.shape[0] * (labels.shape[-1] - 1)}).")
            targets = ops.shift_targets(labels, attention_mask, cfg.ignore_index)
            for ar in self.arenas.values():  # final norm / lm_head: pending optimizer updates
                ar.wait_update()
            loss, logits = HeadLossFn.apply(h, lm, targets, cfg.ignore_index, *lm.head_params())
        else:
            for ar in self.arenas.values():
                ar.wait_update()
            logits = lm.lm_head(lm.model.norm(h))
        logits = logits.view(B, L, -1)
        hs_t = tuple(t.view(B, L, d) for t in hs) if hs else None
        if not return_dict:  # :667-669
            out = (logits,) + ((hs_t,) if hs_t is not None else ())
            return (loss,) + out if loss is not None else out
        return CullavoCausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=None, hidden_states=hs_t,
                                             attentions=None)

    # -- packed step: only the attended rows run the decoder layers and the head ------------------
    @staticmethod
    def _merged_lens(host, B: int, P: int):
        """attended rows per sequence after the merge, from the read-back of _merge_stats_async (already
        waited for by _merge): every attended <image> token became P rows. Raises on a mask with a hole."""
        img, count, span = (host[3 + i * B:3 + (i + 1) * B].tolist() for i in range(3))
        check_no_holes(count, span)
        return [c + n * (P - 1) for c, n in zip(count, img)]

    def _packed_plan(self, attention_mask, attended_lens, B: int, L: int, output_hidden_states):
        """the batch's PackedPlan, or None for the padded path (switch off, no mask or no host-side counts,
        hidden states wanted, or a batch without padding)"""
        if not self.packed_rows or attention_mask is None or attended_lens is None or output_hidden_states:
            return None
        if tuple(attention_mask.shape) != (B, L) or sum(int(n) for n in attended_lens) >= B * L:
            return None
        return packed_plan(attention_mask, attended_lens)

    def _forward_packed(self, inputs_embeds, labels, attention_mask, position_ids, plan, num_supervised, return_dict):
        cfg, lm = self.config, self.language_model
        B, L, d = inputs_embeds.shape
        rows = plan.rows
        live = rows >= 0
        pos = torch.where(live, position_ids.reshape(-1)[rows.clamp_min(0)], 0)
        sctx = StepContext(B, L, pos)
        sctx.packed = plan
        h = PackRowsFn.apply(inputs_embeds.reshape(B * L, d), rows)
        targets = None
        if labels is not None:
            if labels.shape != (B, L):
                raise IndexError(f"The shape of the mask [{B}, {L - 1}] at index 1 does not match the shape of "
                                 f"the indexed tensor [{labels.shape[0]}, {labels.shape[-1] - 1}] at index 1")
            targets = ops.gather_targets(ops.shift_targets(labels, attention_mask, cfg.ignore_index), rows,
                                         cfg.ignore_index)
        n_rows = 0  # the supervised-row tail on top: its rows are packed rows (sized as _tail_rows sizes them)
        if self.supervised_rows and num_supervised is not None and labels is not None:
            n = max(8, -(-int(num_supervised) // 8) * 8)
            n_rows = n if n < plan.Tp else 0
        if n_rows:
            sup = ops.supervised_rows(targets, n_rows, cfg.ignore_index)
            last = lm.model.layers[-1]
            compact = all(last.lora_groups[g] is NO_LORA for g in ("gu", "down"))
            if compact:
                sctx.tail_layer, sctx.tail_rows = last, sup
            h, _ = lm.decode(h, sctx, False)
            for ar in self.arenas.values():
                ar.wait_update()
            loss = HeadLossRowsFn.apply(h, lm, targets, cfg.ignore_index, sup, plan.Tp, compact, *lm.head_params())
            logits = None
        else:
            h, _ = lm.decode(h, sctx, False)
            for ar in self.arenas.values():  # final norm / lm_head: pending optimizer updates
                ar.wait_update()
            if targets is not None:
                loss, logits = HeadLossFn.apply(h, lm, targets, cfg.ignore_index, *lm.head_params())
            else:
                loss, logits = None, lm.lm_head(lm.model.norm(h))
            logits = UnpackRowsFn.apply(logits, rows, B * L).view(B, L, -1)  # zeros where nothing is attended
        if not return_dict:
            return (loss, logits) if loss is not None else (logits,)
        return CullavoCausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=None, hidden_states=None,
                                             attentions=None)

    # -- supervised-row tail: the training step's loss without the rows that carry no label ------
    def _tail_rows(self, num_supervised, labels, B: int, L: int, output_hidden_states) -> int:
        """padded size of the row set, or 0 for the full-logits path (the default: the switch is off,
        no host-side count came with the batch, hidden states are wanted, or nothing would be saved)"""
        if not self.supervised_rows or num_supervised is None or labels is None or output_hidden_states:
            return 0
        if tuple(labels.shape) != (B, L):
            return 0  # the full path raises the reference's error
        n = max(8, -(-int(num_supervised) // 8) * 8)  # K % 8 of the head's dW GEMM; zero rows pad
        return n if n < B * L else 0

    def _forward_supervised_rows(self, inputs_embeds, labels, attention_mask, sctx, n_rows: int, return_dict):
        cfg, lm = self.config, self.language_model
        B, L, d = inputs_embeds.shape
        targets = ops.shift_targets(labels, attention_mask, cfg.ignore_index)
        rows = ops.supervised_rows(targets, n_rows, cfg.ignore_index)
        # the last layer's MLP half feeds only the head: it runs on the rows too (not under LoRA adapters)
        last = lm.model.layers[-1]
        compact = all(last.lora_groups[g] is NO_LORA for g in ("gu", "down"))
        if compact:
            sctx.tail_layer, sctx.tail_rows = last, rows
        h, _ = lm.decode(inputs_embeds.reshape(B * L, d).contiguous(), sctx, False)
        for ar in self.arenas.values():  # final norm / lm_head: pending optimizer updates
            ar.wait_update()
        loss = HeadLossRowsFn.apply(h, lm, targets, cfg.ignore_index, rows, B * L, compact, *lm.head_params())
        if not return_dict:
            return (loss, None)
        return CullavoCausalLMOutputWithPast(loss=loss, logits=None, past_key_values=None, hidden_states=None,
                                             attentions=None)

    # -- KV-cache inference (reference :605-636 and HF generate; generation.py) ------------------
    def _forward_cached(self, input_ids, pixel_values, attention_mask, position_ids, cache, inputs_embeds,
                        vision_feature_layer, strategy, labels, return_dict, max_len: int | None = None,
                        prefill_chunk: int | None = None, kv_cache_dtype: str | None = None):
        from .generation import KVCache, lm_infer
        kv_dtype = self._kv_dtype(cache, kv_cache_dtype)
        if cache is not None and not isinstance(cache, KVCache):
            # transformers-layout cache (legacy tuple / DynamicCache, as the reference's decode branch
            # receives it, arch_cullavo.py:605-636): copied once; the KVCache returned in
            # past_key_values indexes like the legacy tuple (cache[layer] -> (key, value) [B,H,L,D])
            cache = KVCache.from_legacy(cache, attention_mask, kv_dtype=kv_dtype)
        if torch.is_grad_enabled() and any(p.requires_grad for ar in self.arenas.values() for p in ar.params.values()):
            torch.set_grad_enabled(False)  # inference only, as under the reference's torch.inference_mode()
            try:
                return self._forward_cached(input_ids, pixel_values, attention_mask, position_ids, cache,
                                            inputs_embeds, vision_feature_layer, strategy, labels, return_dict,
                                            max_len, prefill_chunk, kv_dtype)
            finally:
                torch.set_grad_enabled(True)
        self.vision_tower.eval()
        first = cache is None or cache.get_seq_length() == 0
        if inputs_embeds is None:
            inputs_embeds = self.get_input_embeddings()(input_ids)
            if first and pixel_values is not None and input_ids.shape[1] != 1:
                image_features = self._image_features(pixel_values, vision_feature_layer, strategy)
                inputs_embeds, attention_mask, position_ids = self._merge(image_features, inputs_embeds, input_ids,
                                                                          attention_mask)
        B, L = inputs_embeds.shape[:2]
        if max_len is None:
            max_len = L + 256
        logits, cache = lm_infer(self.language_model, inputs_embeds, attention_mask, position_ids, cache, max_len,
                                 prefill_chunk if prefill_chunk is not None else self.prefill_chunk, kv_dtype=kv_dtype)
        out = CullavoCausalLMOutputWithPast(loss=None, logits=logits, past_key_values=cache, hidden_states=None,
                                            attentions=None)
        return out if return_dict else out.to_tuple()

    def _kv_dtype(self, cache, kv_cache_dtype: str | None) -> str:
        """the KV-cache format of a cached call: the caller's, else a KVCache's own, else the model's
        default; a KVCache of another format than the caller names is a ValueError"""
        from .generation import KV_DTYPES, KVCache
        if kv_cache_dtype is not None and kv_cache_dtype not in KV_DTYPES:
            raise ValueError(f"kv_cache_dtype {kv_cache_dtype!r}: one of {KV_DTYPES}")
        if isinstance(cache, KVCache):
            if kv_cache_dtype is not None and kv_cache_dtype != cache.kv_dtype:
                raise ValueError(f"kv_cache_dtype {kv_cache_dtype!r} conflicts with the {cache.kv_dtype!r} cache passed "
                                 f"as past_key_values (a cache keeps its format)")
            return cache.kv_dtype
        kv_dtype = kv_cache_dtype if kv_cache_dtype is not None else self.kv_cache_dtype
        if kv_dtype != "bf16" and self.dtype != torch.bfloat16:
            raise NotImplementedError("KV-cache decode runs on the bf16 model (the f32 mode is a parity mode)")
        return kv_dtype

    @torch.no_grad()
    def generate(self, input_ids=None, pixel_values=None, attention_mask=None, max_new_tokens: int = 20,
                 do_sample: bool = False, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                 eos_token_id: int | None = None, pad_token_id: int | None = None, use_cache: bool = True,
                 generator=None, past_key_values=None, return_dict_in_generate: bool = False,
                 prefill_chunk: int | None = None, seed: int | None = None, device_loop: bool | None = None,
                 compact_cache: bool = False, kv_cache_dtype: str | None = None, **kw):
        """Decoder-only generate: returns [B, S + new] (prompt ids then sampled ids), stopping when
        every sequence has produced eos_token_id (finished rows are padded with pad_token_id).
        past_key_values: the cache of an earlier call continues a conversation -- input_ids then holds
        only the new turn (no pixel values; HF's convention: its first id is the last token the earlier
        call sampled, which is not in the cache). return_dict_in_generate: a CullavoGenerateOutput
        (.sequences, .past_key_values) instead of the ids. prefill_chunk: prefill the merged prompt in
        pieces of at most that many rows (None: one pass).
        seed / device_loop: the device loop (generation.SamplerState, the sampling kernel captured at
        the end of the decode graph). seed=int samples with Philox streams keyed by (seed, the
        sequence's stream id, the token's index): reproducible without a torch.Generator and, for a
        sequence, independent of its batch neighbours; the stream ids default to arange(B) and
        sample_offsets=<[B] ints> overrides them. device_loop=True alone decodes greedily on the
        device. With neither argument the host loop around generation.sample_next runs unchanged.
        compact_cache: keep the KV cache ragged and compact (generation.KVCache.lengths). Off, every
        row appends one cache row per step, so a row that met eos early caches the pads it is fed
        afterwards and its conversation cannot be continued correctly. On (host and device loop), a
        row stops advancing with the step that would feed its eos: the returned cache
        (return_dict_in_generate=True) holds, per row, every real token but the row's last one (its
        eos, or the last sampled token of an unfinished row: HF's convention, per row), and the
        sequences are those of compact_cache=False. generate(past_key_values=<that cache>,
        input_ids=<the left-padded new turns>, attention_mask=<[B, S] or [B, past + S]>) then
        continues every conversation; a ragged input cache or a left-padded new turn takes the
        ragged path without the flag.
        kv_cache_dtype: the KV cache's format, "bf16", "fp8" or "fp8_sim" (None: self.kv_cache_dtype, or
        the format of the KVCache passed as past_key_values; a conflicting value raises ValueError)."""
        from .generation import DecodeStepper, HostSampler, KVCache, SamplerState, device_sampling
        if not use_cache:
            raise NotImplementedError("generate() runs on the KV cache (use_cache=True)")
        on_device = device_sampling(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                    generator=generator, seed=seed, device_loop=device_loop)
        for ar in self.arenas.values():  # pending optimizer updates (FusedAdamW overlap)
            ar.wait_update()
        cfg = self.config
        pad = pad_token_id if pad_token_id is not None else cfg.pad_token_id
        B, S = input_ids.shape
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        n_img = int((input_ids == cfg.image_token_index).sum(-1).max()) if pixel_values is not None else 0
        strategy = kw.get("vision_feature_select_strategy", cfg.vision_feature_select_strategy)
        # image feature rows per <image> token: the patches, plus CLS under "full" (:588-597)
        n_feat = cfg.vision_config.num_patches + (1 if strategy == "full" else 0)
        L0 = S + n_img * (n_feat - 1)
        if past_key_values is None:
            out = self._forward_cached(input_ids, pixel_values, attention_mask, None, None, None,
                                       cfg.vision_feature_layer, strategy, None, True,
                                       max_len=L0 + max_new_tokens, prefill_chunk=prefill_chunk,
                                       kv_cache_dtype=kv_cache_dtype)
        else:
            if pixel_values is not None:
                raise NotImplementedError("generate(past_key_values=...) continues with text only: the images "
                                          "are in the cache")
            cache = past_key_values
            kv_dtype = self._kv_dtype(cache, kv_cache_dtype)
            if not isinstance(cache, KVCache):
                cache = KVCache.from_legacy(cache, attention_mask, kv_dtype=kv_dtype)
            # room for the new turn and every new token before the decode graph captures the cache
            cache.grow(cache.length + S + max_new_tokens)
            out = self._forward_cached(input_ids, None, attention_mask, None, cache, None, cfg.vision_feature_layer,
                                       strategy, None, True, prefill_chunk=prefill_chunk)
        cache = out.past_key_values
        compact = bool(compact_cache) or cache.lengths is not None
        if compact:
            cache.make_ragged()
        mark = cache.mark() if return_dict_in_generate and not compact else None
        if on_device:  # the sampling kernel: in the decode graph's capture, or after each eager step
            sampler = SamplerState(B, max_new_tokens, input_ids.device, do_sample=do_sample, temperature=temperature,
                                   top_k=top_k, top_p=top_p, seed=seed if seed is not None else 0,
                                   eos_token_id=eos_token_id, pad_token_id=pad, row_offset=kw.get("sample_offsets"))
        else:
            sampler = HostSampler(B, input_ids.device, eos_token_id=eos_token_id, pad_token_id=pad, do_sample=do_sample,
                                  temperature=temperature, top_k=top_k, top_p=top_p, generator=generator)
        sampler.sample(out.logits[:, -1])  # the first token, from the prefill logits
        # the decode steps replay one captured HIP graph (generation.DecodeGraph) unless asked not to
        stepper = DecodeStepper(self, cache, sampler, compact=compact,
                                graph=kw.get("decode_graph", True) and max_new_tokens > 1 and input_ids.is_cuda)
        check_every = 16  # all-finished test every 16 tokens: one host sync per 16 steps, not per step
        n = 1
        while n < max_new_tokens:
            if eos_token_id is not None and n % check_every == 0 and bool(sampler.finished.all()):
                break
            stepper.feed(sampler)
            n += 1
        gen = sampler.tokens(n)
        if eos_token_id is not None:
            # HF stops at the first step where every row has finished; the steps run past it (at
            # most check_every - 1) hold only padding and are dropped
            done = torch.cumsum((gen == eos_token_id).to(torch.int64), 1) > 0
            all_done = done.all(0)
            if bool(all_done.any()):
                gen = gen[:, :int(all_done.to(torch.int64).argmax()) + 1]
        sequences = torch.cat([input_ids, gen.to(input_ids.dtype)], 1)
        if not return_dict_in_generate:
            return sequences
        cache.release(mark, fed=gen.shape[1] - 1)
        return CullavoGenerateOutput(sequences=sequences, past_key_values=cache)

    # -- pieces ---------------------------------------------------------------------------------
    def _image_features(self, pixel_values, layer: int, strategy: str):
        vt = self.vision_tower.vision_model
        n = vt.cfg.num_hidden_layers
        idx = n + 1 + layer if layer < 0 else layer
        if not 0 <= idx <= n:
            raise IndexError(f"vision_feature_layer {layer} out of range")
        feats = vt.hidden_state(pixel_values, idx)  # hidden_states[layer], only the layers needed
        if strategy == "default":
            feats = feats[:, 1:]
        elif strategy == "full":
            pass
        else:
            raise ValueError(f"Unexpected select feature strategy: {self.config.vision_feature_select_strategy}")
        return self.multi_modal_projector(feats)

    def _merge_stats_async(self, input_ids, attention_mask=None):
        """The three integers that size the merge (max image tokens per row, total image
        tokens, rows ending in <pad>), reduced on the GPU and copied to pinned host memory
        without waiting: the copy completes long before the vision tower enqueued behind it,
        so the host read in _merge does not drain the GPU queue."""
        cfg = self.config
        is_img = input_ids == cfg.image_token_index
        st = torch.stack([is_img.sum(-1).max(), is_img.sum(), (input_ids[:, -1] == cfg.pad_token_id).sum()])
        if attention_mask is not None:
            # the packed step's per-row counts in the same copy: attended <image> tokens, attended
            # positions and their span (packed.mask_counts)
            cs = mask_counts(attention_mask)
            st = torch.cat([st, (is_img & (attention_mask != 0)).sum(-1), cs[0], cs[1]])
        host = torch.empty(st.numel(), dtype=st.dtype, pin_memory=True)
        host.copy_(st, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev

    def _merge(self, image_features, inputs_embeds, input_ids, attention_mask, stats=None):
        """transformers ~4.37 _merge_input_ids_with_image_features on the merge_plan kernel.
        One small device->host read (image-token counts, left-padding flag) sizes the output,
        as the reference's .max() / torch.where do."""
        cfg = self.config
        n_img, P, d = image_features.shape
        B, S = input_ids.shape
        host, ev = stats if stats is not None else self._merge_stats_async(input_ids)
        ev.synchronize()
        n_max, n_total, n_pad_last = (int(x) for x in host[:3].tolist())
        if n_total != n_img:
            raise ValueError(f"The input provided to the model are wrong. The number of image tokens is {n_total} "
                             f"while the number of image given to the model is {n_img}. This prevents correct "
                             f"indexing and breaks batch generation.")
        left_padding = n_pad_last == 0
        L = n_max * (P - 1) + S
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        text_dst, src, mmask, pos = ops.merge_plan(input_ids, attention_mask, L=L, image_token=cfg.image_token_index,
                                                   n_patches=P, left_padding=left_padding)
        n_text = B * S
        flat = src.reshape(-1)
        rows = torch.arange(B * L, device=flat.device)
        is_img_row = flat >= n_text
        img_dst = torch.empty(n_img * P + 1, dtype=torch.int64, device=flat.device)
        img_dst.scatter_(0, torch.where(is_img_row, flat - n_text, n_img * P), rows)
        merged = MergeFn.apply(inputs_embeds.reshape(n_text, d), image_features.reshape(n_img * P, d), flat,
                               text_dst, img_dst[:-1])
        return merged.view(B, L, d), mmask, pos


def build_cullavo(config: CuLLaVOConfig | None = None, **kw) -> CuLLaVOModel:
    from .config import llava_1_5_7b
    return CuLLaVOModel(config or llava_1_5_7b(), **kw)
