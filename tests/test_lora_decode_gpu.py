"""The decode products with the LoRA up-projection in their epilogue (cullavo_decode_linear_lora,
cullavo_nf4_decode_linear_lora; ops.decode_linear / ops.nf4_decode_linear with lora=) against the
route the decode step took before them, bit for bit.

Reference: t = scaling * u_m B_m^T by one K = 64 gemm_ex per module (LoraGroup.up_project written
out), then ops.linear(x, w, addend=t, residual=...) resp. ops.nf4_decode_linear(..., addend=t); for
the SwiGLU output that product followed by ops.swiglu_fwd; the input transforms by their own kernels
(ops.rmsnorm_fwd, ops.swiglu_fwd) first. The fused kernels do the same arithmetic in the same order,
so the gate is torch.equal and needs no tolerance (the pieces of the reference route are pinned
against float64 by tests/test_decode_accuracy_gpu.py).

Every case runs with what the call does not own poisoned: the decode rows live in a 16-row buffer
whose rows >= M are NaN, u is a column block of a wider NaN buffer (ld_lora_u > n * 64, the other
groups' columns and the rows >= M NaN), lora_B is followed by NaN rows, and y is a view inside a
frame of sentinels. The output must be finite and the frame intact.

CASES names the kernel instantiation each case reaches: gemv_k<XF, NBW, NW, OT, LORA> by
cullavo_decode_linear_lora's switch (K >= 8192: 4-load batches; more than 16384 weight rows: 16 waves;
else 8-load batches, 8 waves) and nf4_gemv_k<NW, 8, OT, LORA> (K > 8192: 16 waves). Both kernels work
on one 16-row block per workgroup in every variant a LoRA call reaches, and lora_out % 16 == 0, so
no module boundary can fall inside a workgroup's rows; the 48-wide modules put boundaries at rows
that are no multiple of 32 or 64.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = 777.0
EPS = 1e-5

# (id, entry, transform, M, K, modules, module width, residual, scaling, instantiation)
# transform 3 / 4 (nf4: "swiglu"): the gate | up pair, two modules of `width` rows each, y [M, width]
CASES = [
    ("gemv-k64-m1", "gemv", 0, 1, 64, 1, 16, False, 0.25, "gemv_k<XF 0, 8, 8, OT 0, true>, one k-step per wave"),
    ("gemv-k128-m3", "gemv", 0, 3, 128, 2, 48, True, 0.3, "gemv_k<XF 0, 8, 8, OT 0, true>"),
    ("gemv-k1088-m8", "gemv", 0, 8, 1088, 3, 256, True, 0.25, "gemv_k<XF 0, 8, 8, OT 0, true>, 48 workgroups"),
    ("gemv-4096x4096-m16", "gemv", 0, 16, 4096, 2, 2048, True, 0.25, "gemv_k<XF 0, 8, 8, OT 0, true>, 7B o_proj"),
    ("gemv-norm", "gemv", 1, 3, 128, 3, 16, True, 0.25, "gemv_k<XF 1, 8, 8, OT 0, true>"),
    ("gemv-swiglu-in", "gemv", 2, 8, 128, 2, 48, False, 0.3, "gemv_k<XF 2, 8, 8, OT 0, true>"),
    ("gemv-swiglu-out", "gemv", 3, 16, 1088, 2, 48, False, 0.25, "gemv_k<XF 0, 8, 8, OT 1, true>"),
    ("gemv-norm-swiglu-out", "gemv", 4, 1, 64, 2, 256, False, 0.3, "gemv_k<XF 1, 8, 8, OT 1, true>"),
    ("gemv-longk", "gemv", 0, 3, 8192, 1, 16, True, 0.25, "gemv_k<XF 0, 4, 8, OT 0, true>"),
    ("gemv-longk-norm", "gemv", 1, 1, 8192, 2, 16, False, 0.3, "gemv_k<XF 1, 4, 8, OT 0, true>"),
    ("gemv-longk-swiglu-in", "gemv", 2, 8, 8192, 1, 48, True, 0.25, "gemv_k<XF 2, 4, 8, OT 0, true>"),
    ("gemv-longk-swiglu-out", "gemv", 3, 3, 8192, 2, 16, False, 0.25, "gemv_k<XF 0, 4, 8, OT 1, true>"),
    ("gemv-longk-norm-swiglu-out", "gemv", 4, 3, 8192, 2, 16, False, 0.3, "gemv_k<XF 1, 4, 8, OT 1, true>"),
    ("gemv-wide", "gemv", 0, 8, 64, 3, 5472, True, 0.25, "gemv_k<XF 0, 4, 16, OT 0, true>, 16416 rows"),
    ("gemv-wide-norm", "gemv", 1, 3, 64, 3, 5472, False, 0.3, "gemv_k<XF 1, 4, 16, OT 0, true>"),
    ("gemv-wide-swiglu-in", "gemv", 2, 1, 64, 3, 5472, True, 0.25, "gemv_k<XF 2, 4, 16, OT 0, true>"),
    ("gemv-wide-swiglu-out", "gemv", 3, 16, 64, 2, 8208, False, 0.25, "gemv_k<XF 0, 4, 16, OT 1, true>, 16416 rows"),
    ("gemv-wide-norm-swiglu-out", "gemv", 4, 3, 64, 2, 8208, False, 0.3, "gemv_k<XF 1, 4, 16, OT 1, true>"),
    ("nf4-k64-m1", "nf4", 0, 1, 64, 1, 16, False, 0.25, "nf4_gemv_k<8, 8, 0, true>, one block"),
    ("nf4-k128-m3", "nf4", 0, 3, 128, 2, 48, True, 0.3, "nf4_gemv_k<8, 8, 0, true>"),
    ("nf4-k1088-m8", "nf4", 0, 8, 1088, 3, 256, True, 0.25, "nf4_gemv_k<8, 8, 0, true>"),
    ("nf4-4096x4096-m16", "nf4", 0, 16, 4096, 2, 2048, True, 0.25, "nf4_gemv_k<8, 8, 0, true>, 7B o_proj"),
    ("nf4-swiglu-m3", "nf4", 3, 3, 128, 2, 48, False, 0.3, "nf4_gemv_k<8, 8, 1, true>"),
    ("nf4-swiglu-m16", "nf4", 3, 16, 1088, 2, 256, False, 0.25, "nf4_gemv_k<8, 8, 1, true>"),
    ("nf4-longk", "nf4", 0, 8, 8256, 2, 16, True, 0.25, "nf4_gemv_k<16, 8, 0, true>"),
    ("nf4-longk-swiglu", "nf4", 3, 1, 8256, 2, 16, False, 0.3, "nf4_gemv_k<16, 8, 1, true>"),
]


def _ops():
    from cullavo_amd import ops
    return ops


def _rows16(t, M):
    """t [M, C] as the first M rows of a 16-row buffer whose other rows are NaN"""
    buf = torch.full((16, t.shape[1]), float("nan"), dtype=t.dtype, device="cuda")
    buf[:M] = t
    return buf[:M]


class Case:
    """One case's inputs on the GPU. The same tensors serve the reference and the fused call."""

    def __init__(self, entry, xt, M, K, n_mod, width, residual, scale, seed=0, zero_b=False):
        ops = _ops()
        g = torch.Generator().manual_seed(1000 + seed)

        def rnd(*shape, s=1.0):
            return (torch.randn(*shape, generator=g) * s).to(BF).cuda()

        self.entry, self.xt, self.M, self.K, self.scale, self.width = entry, xt, M, K, scale, width
        self.n_mod, self.rows = n_mod, n_mod * width
        self.swiglu_out = xt in (3, 4)
        self.N = width if self.swiglu_out else self.rows
        assert not self.swiglu_out or n_mod == 2
        self.x = _rows16(rnd(M, 2 * K if xt == 2 else K), M)
        self.norm_w = (1.0 + 0.1 * torch.randn(K, generator=g)).to(BF).cuda() if xt in (1, 4) else None
        self.w = rnd(self.rows, K, s=K ** -0.5)
        if entry == "nf4":
            self.codes, self.absmax = ops.nf4_quantize(self.w)
        self.residual = rnd(M, self.N) if residual else None
        # u: columns [40, 40 + 64 n) of a [16, 64 n + 104] NaN buffer (the other groups' columns)
        ubuf = torch.full((16, 64 * n_mod + 104), float("nan"), dtype=BF, device="cuda")
        ubuf[:M, 40:40 + 64 * n_mod] = rnd(M, 64 * n_mod, s=0.5)
        self.u = ubuf[:M, 40:40 + 64 * n_mod]
        bbuf = torch.full((self.rows + 16, 64), float("nan"), dtype=BF, device="cuda")
        bbuf[:self.rows] = 0 if zero_b else rnd(self.rows, 64, s=0.25)
        self.b = bbuf[:self.rows]
        self.frame = torch.full((M + 2, self.N + 16), SENTINEL, dtype=BF, device="cuda")
        self.y = self.frame[1:M + 1, 8:8 + self.N]

    def lora(self):
        return self.u, self.b, self.width, self.scale

    def x_eff(self):
        """the rows the product sees, by the transform's own kernel"""
        ops = _ops()
        if self.xt in (1, 4):
            return ops.rmsnorm_fwd(self.x, self.norm_w, EPS)[0]
        if self.xt == 2:
            return ops.swiglu_fwd(self.x)
        return self.x

    def term(self):
        """LoraGroup.up_project written out: one K = 64 product per module, alpha = scaling"""
        ops = _ops()
        t = torch.empty((self.M, self.rows), dtype=BF, device="cuda")
        ldu = self.u.stride(0)
        for m in range(self.n_mod):
            ops.gemm_ex(0, 0, self.M, self.width, 64, self.u[:, 64 * m:], ldu, self.b[self.width * m:], 64,
                        t[:, self.width * m:], self.rows, alpha=self.scale)
        return t

    def reference(self, addend=True):
        ops = _ops()
        t = self.term() if addend else None
        x = self.x_eff()
        if self.entry == "nf4":
            y = ops.nf4_decode_linear(x, self.codes, self.absmax, addend=t, residual=self.residual)
        else:
            y = ops.linear(x, self.w, addend=t, residual=self.residual)
        return ops.swiglu_fwd(y) if self.swiglu_out else y

    def fused(self, lora="own", **kw):
        ops = _ops()
        lora = self.lora() if lora == "own" else lora
        if self.entry == "nf4":
            return ops.nf4_decode_linear(self.x, self.codes, self.absmax, residual=self.residual,
                                         swiglu_out=self.swiglu_out, lora=lora, out=self.y, **kw)
        return ops.decode_linear(self.x, self.w, transform=self.xt, norm_w=self.norm_w, eps=EPS,
                                 residual=self.residual, lora=lora, out=self.y, **kw)

    def frame_intact(self):
        f = self.frame.clone()
        f[1:self.M + 1, 8:8 + self.N] = SENTINEL
        return bool((f == SENTINEL).all())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_term_is_the_materialised_route_bitwise(case):
    _, entry, xt, M, K, n_mod, width, residual, scale, _inst = case
    c = Case(entry, xt, M, K, n_mod, width, residual, scale, seed=len(case[0]))
    ref = c.reference()
    got = c.fused()
    torch.cuda.synchronize()
    assert got.data_ptr() == c.y.data_ptr()
    assert torch.isfinite(got.float()).all()
    assert torch.isfinite(ref.float()).all()
    assert c.frame_intact()
    # the term moves the output: a kernel that dropped it would not pass by accident
    assert not torch.equal(ref, c.reference(addend=False))
    diff = (got.view(torch.int16) != ref.view(torch.int16)).sum().item()
    assert diff == 0, f"{diff} of {ref.numel()} outputs differ from the materialised route"


@pytest.mark.parametrize("entry,xt", [("gemv", 0), ("gemv", 3), ("nf4", 0), ("nf4", 3)])
def test_zero_adapters_give_the_plain_call(entry, xt):
    """lora_B = 0 (peft's initial state): the bits of the call without lora="""
    c = Case(entry, xt, 3, 128, 2, 48, xt == 0, 0.25, seed=7, zero_b=True)
    got = c.fused().clone()
    plain = c.fused(lora=None).clone()
    torch.cuda.synchronize()
    assert c.frame_intact() and torch.isfinite(got.float()).all()
    assert torch.equal(got, plain)
    assert torch.equal(got, c.reference(addend=False))


@pytest.mark.parametrize("entry", ["gemv", "nf4"])
@pytest.mark.parametrize("bad", ["r32", "width24", "rows_not_modules", "u_stride", "f32_rows"])
def test_unsupported_arguments_are_refused_before_any_launch(entry, bad):
    from cullavo_amd._lib import CullavoError
    c = Case(entry, 0, 3, 128, 2, 48, True, 0.25, seed=3)
    u, b, width, scale = c.lora()
    if bad == "r32":  # lora_r = 32: a contiguous [rows, 32] stack
        lora = (u, b[:, :32].contiguous(), width, scale)
    elif bad == "width24":  # lora_out % 16 != 0 (96 rows = 4 x 24)
        lora = (u, b, 24, scale)
    elif bad == "rows_not_modules":  # N = 96 is no multiple of lora_out = 64
        lora = (u, b, 64, scale)
    elif bad == "u_stride":  # a u row stride of 132: 4 past a multiple of 8
        ubuf = torch.zeros((16, 132), dtype=BF, device="cuda")
        lora = (ubuf[:c.M, :128], b, width, scale)
    else:
        lora = (u, b, width, scale)
        c.x = c.x.float()
    with pytest.raises((ValueError, TypeError, CullavoError)):
        c.fused(lora=lora)
    torch.cuda.synchronize()
    assert bool((c.frame == SENTINEL).all())
