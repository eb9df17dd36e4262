"""The inference path's launches, pinned: what generate() and the cached forward ask the library to do.

Every ops.call is recorded as the entry point's name plus the arguments whose declared C type
(_lib.declarations()) is not a pointer: shapes, positions, flags and scales, no address and no stream.
Seven scenarios on the tiny config (a batch of 2, left-padded to unequal lengths) are compared for exact
equality with tests/golden/generation_calls.json, together with the generated ids and the bits of the
last logits (one more cached step on the returned cache, which also pins the state generate() leaves).
A captured decode graph contributes the calls of its capture; its replays make none.

The fixture is recorded by this same test at the commit before a refactor of the path, never from the
code under test: CULLAVO_RECORD_GENERATION_CALLS=1 writes it instead of comparing.
"""
import functools
import json
import os

import pytest
import torch

from oracle import cullavo_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generation_calls.json")
RECORD = os.environ.get("CULLAVO_RECORD_GENERATION_CALLS", "") not in ("", "0")


class _Recorder:
    """ops.call, wrapped: [name, non-pointer argument, ...] per call"""

    def __init__(self, monkeypatch):
        from cullavo_amd import _lib, ops
        self.calls = []
        keep = {n[len("cullavo_"):]: [i for i, (t, _) in enumerate(params) if "*" not in t]
                for n, (_, params) in _lib.declarations().items()}
        inner = ops.call

        def call(name, *args):
            self.calls.append([name] + [_plain(args[i]) for i in keep[name]])
            return inner(name, *args)

        monkeypatch.setattr(ops, "call", call)


def _plain(a):
    a = getattr(a, "value", a)
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    return int(a) if hasattr(a, "__index__") else float(a)


@functools.lru_cache(maxsize=1)
def _model():
    from cullavo_amd.arch_cullavo import CuLLaVOModel
    from cullavo_amd.config import tiny_gpu
    m = CuLLaVOModel(tiny_gpu(), device="cuda", trainable="none", init="none")
    m.load_state_dict(O.make_weights(O.config_small_gpu(), 6))
    m.eval()
    return m


@functools.lru_cache(maxsize=1)
def _prompt():
    """two prompts of 20 and 25 tokens (one image each), the shorter left-padded: [2, 25]"""
    cfg = O.config_small_gpu()
    ids_a, mask_a, pix_a, _ = O.make_inputs(cfg, 1, 20, 3, 71)
    ids_b, mask_b, pix_b, _ = O.make_inputs(cfg, 1, 25, 3, 72)
    ids = torch.cat([torch.cat([torch.full((1, 5), cfg.pad_token_id), ids_a], 1), ids_b], 0)
    mask = torch.cat([torch.cat([torch.zeros(1, 5, dtype=mask_a.dtype), mask_a], 1), mask_b], 0)
    return dict(input_ids=ids.cuda(), pixel_values=torch.cat([pix_a, pix_b], 0).cuda(), attention_mask=mask.cuda())


def _bits(logits):
    return logits.contiguous().view(torch.int16).cpu().tolist()


def _finish(m, res):
    """the generated ids and the logits of one more cached step on the cache generate() returned"""
    seq, cache = res.sequences, res.past_key_values
    out = m(input_ids=seq[:, -1:], past_key_values=cache, use_cache=True)
    return dict(ids=seq.cpu().tolist(), logits=_bits(out.logits[:, -1]))


def _generate(m, **kw):
    return _finish(m, m.generate(**_prompt(), return_dict_in_generate=True, **kw))


def _graph(m, golden):
    return _generate(m, max_new_tokens=5)


def _eager(m, golden):
    return _generate(m, max_new_tokens=5, decode_graph=False)


def _device_loop(m, golden):
    a = _generate(m, max_new_tokens=5, device_loop=True)
    b = _generate(m, max_new_tokens=5, seed=3, do_sample=True, top_k=4)
    return dict(ids=[a["ids"], b["ids"]], logits=[a["logits"], b["logits"]])


def _pick_eos(m):
    """a token row 0 produces (greedy, not first) before row 1 does: found when the fixture is recorded"""
    S = _prompt()["input_ids"].shape[1]
    new = m.generate(**_prompt(), max_new_tokens=6)[:, S:].cpu().tolist()
    for i in range(1, 5):
        t = new[0][i]
        if t not in new[0][:i] and t not in new[1][:i + 2]:
            return t, i + 1
    raise AssertionError(f"no token of row 0 stops it before row 1: {new}")


def _compact_conversation(m, golden):
    cfg = O.config_small_gpu()
    eos = golden["eos"]
    first = m.generate(**_prompt(), max_new_tokens=6, eos_token_id=eos, compact_cache=True,
                       return_dict_in_generate=True)
    S = _prompt()["input_ids"].shape[1]
    new = first.sequences[:, S:].cpu()
    stop = [(new[b] == eos).nonzero()[:1].flatten().tolist() for b in range(2)]
    assert stop[0] == [golden["eos_step"] - 1] and stop[0] != stop[1], stop  # row 0 stops first
    # HF's convention: a row's new turn begins with its last token, which is not in the cache
    last = [int(new[0, stop[0][0]]), int(new[1, -1])]
    g = torch.Generator().manual_seed(9)
    t0 = torch.randint(2, cfg.image_token_index, (5,), generator=g).tolist()
    t1 = torch.randint(2, cfg.image_token_index, (2,), generator=g).tolist()
    turn = torch.tensor([[last[0]] + t0, [cfg.pad_token_id] * 3 + [last[1]] + t1]).cuda()
    tmask = torch.tensor([[1] * 6, [0, 0, 0, 1, 1, 1]]).cuda()
    second = m.generate(input_ids=turn, attention_mask=tmask, past_key_values=first.past_key_values,
                        max_new_tokens=4, return_dict_in_generate=True)
    r = _finish(m, second)
    return dict(ids=[first.sequences.cpu().tolist(), r["ids"]], logits=r["logits"])


def _uniform_follow_up(m, golden):
    cfg = O.config_small_gpu()
    cache = m(**_prompt(), use_cache=True).past_key_values
    toks = torch.randint(2, cfg.image_token_index, (2, 3), generator=torch.Generator().manual_seed(4)).cuda()
    out = m(input_ids=toks, past_key_values=cache, use_cache=True)
    assert cache.lengths is None
    return dict(ids=out.logits[:, -1].argmax(-1).cpu().tolist(), logits=_bits(out.logits[:, -1]))


def _chunked_prefill(m, golden):
    return _generate(m, max_new_tokens=3, prefill_chunk=7)


def _unfused(m, golden):
    return _generate(m, max_new_tokens=5)


SCENARIOS = {
    "graph": _graph,
    "eager": _eager,
    "device_loop": _device_loop,
    "compact_conversation": _compact_conversation,
    "uniform_follow_up": _uniform_follow_up,
    "chunked_prefill": _chunked_prefill,
    "unfused": _unfused,
}


def _load():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_generation_calls(name, monkeypatch):
    from cullavo_amd import generation
    m = _model()
    golden = _load() if os.path.exists(GOLDEN) else {}
    if RECORD and name == "compact_conversation":
        golden["eos"], golden["eos_step"] = _pick_eos(m)
    if name == "unfused":
        monkeypatch.setattr(generation, "FUSE_DECODE_ROPE", False)
        monkeypatch.setattr(generation, "FUSE_DECODE_GU", False)
    rec = _Recorder(monkeypatch)
    got = SCENARIOS[name](m, golden)
    torch.cuda.synchronize()
    got["calls"] = rec.calls
    if RECORD:
        golden[name] = got
        with open(GOLDEN, "w") as f:
            json.dump(golden, f, separators=(",", ":"))
            f.write("\n")
        return
    want = golden[name]
    assert len(got["calls"]) == len(want["calls"]), (len(got["calls"]), len(want["calls"]))
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i}: {g} vs the parent's {w}"
    assert got["ids"] == want["ids"]
    assert got["logits"] == want["logits"]
