"""LoraTerm.decode_args on the host: the lora= tuple of the decode products where their kernels take
the group's term (r = 64, bf16 u with a row stride that is a multiple of 8, modules of one width that
is a multiple of 16, 1 <= M <= 16 rows, N the group's rows), None exactly where they do not."""
import torch

from cullavo_amd.lora import LoraGroup, LoraSettings, LoraTerm

BF = torch.bfloat16


class _Arena:
    """what LoraGroup asks of its arena, on CPU tensors: adjacent parameters in one flat buffer"""

    def __init__(self, mods, r):
        shapes = [(f"p.{suf}.lora_A.step1.weight", (r, inn)) for suf, _, inn in mods]
        shapes += [(f"p.{suf}.lora_B.step1.weight", (out, r)) for suf, out, _ in mods]
        self.flat = torch.zeros(sum(a * b for _, (a, b) in shapes), dtype=BF)
        self.params, self.offset, o = {}, {}, 0
        for k, (a, b) in shapes:
            self.params[k], self.offset[k] = self.flat[o:o + a * b].view(a, b), o
            o += a * b

    def check_adjacent(self, keys):
        pass

    def view(self, key, shape):
        o = self.offset[key]
        return self.flat[o:o + shape[0] * shape[1]].view(shape)


def _term(outs, r=64, in_f=128, M=4, u=None):
    mods = [(f"m{i}", o, in_f) for i, o in enumerate(outs)]
    g = LoraGroup(_Arena(mods, r), "p.", mods, LoraSettings(r=r, lora_alpha=16.0), uid=0)
    if u is None:
        u = torch.zeros((M, len(outs) * r), dtype=BF)
    return LoraTerm(g, u), g


def test_decode_args_tuple():
    t, g = _term([48, 48, 48])
    u, b, width, scale = t.decode_args(4, 144)
    assert u is t.u and width == 48 and scale == 0.25
    assert tuple(b.shape) == (144, 64) and b.is_contiguous()
    assert b.data_ptr() == g.B(0).data_ptr()  # the group's lora_B weights, stacked in output order
    assert t.decode_args(1, 144) is not None and t.decode_args(16, 144) is not None
    # the gate | up pair as the SwiGLU-output product names it: N = the weight's 2 F rows
    t2, _ = _term([704, 704])
    assert t2.decode_args(2, 1408)[2] == 704
    # u as a column block of a wider buffer
    wide = torch.zeros((4, 256), dtype=BF)
    t3, _ = _term([16], u=wide[:, 8:72])
    assert t3.decode_args(4, 16)[0].stride(0) == 256


def test_decode_args_none_exactly_on_the_unsupported_conditions():
    assert _term([48, 48], r=32)[0].decode_args(4, 96) is None          # r != 64
    assert _term([24, 24])[0].decode_args(4, 48) is None                # lora_out % 16 != 0
    assert _term([48, 32])[0].decode_args(4, 80) is None                # modules of unequal width
    t, _ = _term([48, 48])
    assert t.decode_args(4, 48) is None and t.decode_args(4, 192) is None  # N != n_modules * lora_out
    assert t.decode_args(0, 96) is None and t.decode_args(17, 96) is None  # the GEMM's rows (fused_args)
    assert t.decode_args(4, 96) is not None
    odd = torch.zeros((4, 132), dtype=BF)
    assert _term([48, 48], u=odd[:, :128])[0].decode_args(4, 96) is None   # a u row stride 4 past a multiple of 8
    assert _term([48, 48], u=torch.zeros((4, 128)))[0].decode_args(4, 96) is None  # f32 rows
    # fused_args is what it was: the GEMM's rows only, 256-wide modules
    assert t.fused_args(4, 96) is None and t.fused_args(64, 96) is None
    assert _term([256, 256], M=64)[0].fused_args(64, 512) is not None
    assert _term([256, 256], M=64)[0].decode_args(64, 512) is None
