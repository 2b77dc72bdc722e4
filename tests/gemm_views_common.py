"""A `bc_gemm` problem whose every operand is a view inside a larger, hostile parent (tests/test_gemm_views_gpu.py, tests/test_gemm_views_cpu.py).

Inputs: A / A2 (row or pixel stride = width + 8), a row-major W (ldw = K + 8), bias, colscale, ln_colsum, the row-vector table, R and R2 lie
inside parents filled with fp16 / fp32 NaN: the pad columns, guard rows in front of row 0 and behind the last row (for a convolution: guard
pixels in front of image 0 and behind the last image).  A K tail, an M-tail row, a weight row past N, a halo pixel outside the batch or a bias
lane past N that reaches a product makes the output NaN.  Outputs: C (and C_t) start `offset` elements into a parent filled with the NaN bit
pattern 0x7E5A (fp32: 0x7FC5A5A5), row stride > width, guard rows in front and behind up to the next multiple of 256 rows plus one more
256-row tile; after the launch every element of the view differs from the sentinel and is finite, every other element of the parent is
bit-equal to the sentinel.  The float64 reference is computed from the fp16-rounded valid sub-tensors only; the bars are the project's own,
through tests.common.close.  Nothing here needs a device: `emulate` is a torch statement of the kernel (with the mistakes a kernel can make)
that tests/test_gemm_views_cpu.py drives the same harness with.
The launch forms of the VAE / CLIP / DINOv2 / SAM front ends (Case.front_end): convolutions on the generic gather (Cin % 64 != 0), the VAE
encoder's pad = (0, 1, 0, 1) stride-2 convolution - whose last output row reads input row H: the next image's first row, or the guard pixels -,
an upsample to an explicit size, the fp32 convolution output at N = 3, the epilogue chain act -> colscale -> alpha -> alpha_dev[...] with GELU /
quick-GELU / SiLU, a scalar, a device scalar and a per-image table behind a device step counter (the table between NaN lanes, its other rows
9.0), and the three launches per image of the VAE mid-block attention through the model's own recording (vae_attention_problem)."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests.common import close, g

SENTINEL = 0x7E5A                       # fp16 NaN: what tests/test_attention_gpu.py fills its output buffers with
SENTINEL32 = 0x7FC5A5A5                 # an fp32 NaN
NAN16, NAN32 = 0x7F33, 0x7FD12345       # what the input parents are filled with: NaN of another payload, so that a leak that keeps its payload
                                        # on the way to the output is told from an element that was never written
PAD = 8                                 # pad columns behind every input row
FRONT = 16                              # guard rows in front of row 0 of an input
FLAVOURS = ("vec", "scalar")            # 16-byte aligned view (offset % 8 == 0, ld % 8 == 0) / ld = width + 4 at an odd offset


# activation -> (its BC_ACT_* name in blobctrl_amd._lib, the float64 statement: GELU is the erf form, quick-GELU x sigmoid(1.702 x))
ACTS = {"gelu": ("ACT_GELU", lambda t: 0.5 * t * (1 + torch.erf(t / math.sqrt(2.0)))),
        "quick_gelu": ("ACT_QUICK_GELU", lambda t: t * torch.sigmoid(1.702 * t)),
        "silu": ("ACT_SILU", lambda t: t * torch.sigmoid(t))}


def _filled(n, device, f32=False, bits=None):
    if f32:
        return torch.full((n,), SENTINEL32 if bits is None else bits, dtype=torch.int32, device=device)
    return torch.full((n,), SENTINEL if bits is None else bits, dtype=torch.int16, device=device)


def _elems_behind(t):
    st = t.untyped_storage()
    return (st.nbytes() - (t.data_ptr() - st.data_ptr())) // t.element_size()


class View:
    """A rows x cols input at `offset` elements inside a NaN-filled parent, row stride `ld`: NaN pad columns, `front` guard rows, `back` guard
    rows (default: up to the next multiple of 256 rows and 64 more)."""

    def __init__(self, x, device, ld=None, front=FRONT, back=None, f32=False):
        x = x.reshape(-1, x.shape[-1])
        self.rows, self.cols = x.shape
        self.ld = self.cols + PAD if ld is None else ld
        self.front = front
        self.back = (-self.rows % 256) + 64 if back is None else back
        self.offset = self.front * self.ld
        self.dtype = torch.float32 if f32 else torch.float16
        self.parent = _filled((self.front + self.rows + self.back) * self.ld + PAD, device, f32, NAN32 if f32 else NAN16).view(self.dtype)
        self.valid().copy_(x.to(self.dtype))

    def valid(self):
        return self.parent.as_strided((self.rows, self.cols), (self.ld, 1), self.offset)

    @property
    def t(self):
        """The view as the launch gets it: a tensor whose data pointer is element (0, 0)."""
        return self.parent[self.offset:]

    def assert_inside(self):
        """What the kernel may address, and a plausible overrun of it (the guard rows, one 8-wide vector), lie inside the parent's storage."""
        assert self.offset - self.front * self.ld >= 0 and self.front >= 1 and self.back >= 1
        assert _elems_behind(self.t) >= (self.rows + self.back - 1) * self.ld + self.cols + PAD
        assert (self.parent.data_ptr() + self.offset * self.parent.element_size()) % 16 == 0 or self.dtype == torch.float32

    def guards_intact(self):
        """Every element of the parent outside the view still holds the NaN it was filled with (an input nobody may write)."""
        bits = self.parent.view(torch.int32 if self.dtype == torch.float32 else torch.int16).cpu()
        outside = torch.ones(bits.numel(), dtype=torch.bool)
        outside[(self.offset + torch.arange(self.rows)[:, None] * self.ld + torch.arange(self.cols)[None, :]).flatten()] = False
        return bool((bits[outside] == (NAN32 if self.dtype == torch.float32 else NAN16)).all())


class Out:
    """`rows` x `width` output at FRONT rows + `extra` elements inside a sentinel-filled parent, row stride `ld` (a transposed output
    [B][N][ldc] is B N rows of rows_per_batch elements).  Guard rows behind: up to the next multiple of 256 rows, and 256 more."""

    def __init__(self, rows, width, ld, device, extra=0, f32=False):
        assert ld >= width
        self.rows, self.width, self.ld, self.f32 = rows, width, ld, f32
        self.offset = FRONT * ld + extra
        self.back = (-rows % 256) + 256
        self.bits = _filled(self.offset + (rows + self.back) * ld + 2 * PAD, device, f32)
        self.sentinel = SENTINEL32 if f32 else SENTINEL

    @property
    def parent(self):
        return self.bits.view(torch.float32 if self.f32 else torch.float16)

    @property
    def t(self):
        return self.parent[self.offset:]

    def reset(self):
        self.bits.fill_(self.sentinel)

    def assert_inside(self):
        assert self.offset >= self.ld + PAD                                        # a row or a vector in front of row 0 is inside the parent
        assert _elems_behind(self.t) >= (self.rows + self.back - 1) * self.ld + self.width + PAD

    def _where(self, i):
        return divmod(int(i) - self.offset, self.ld)

    def check(self, what, rows=None):
        """(values [rows][width] float64, count of sentinel elements checked).  Fails when an element outside the view was written, when
        one inside was not, or when one inside is not finite - with the count and the first offending (row, col) of the view's grid.
        rows: the view's first `rows` rows are the view (a launch that fills a buffer image by image: the rest is still sentinel)."""
        bits = self.bits.cpu()
        idx = self.offset + torch.arange(self.rows if rows is None else rows)[:, None] * self.ld + torch.arange(self.width)[None, :]
        inside = torch.zeros(bits.numel(), dtype=torch.bool)
        inside[idx.flatten()] = True
        wrote = bits != self.sentinel
        stray = wrote & ~inside
        if bool(stray.any()):
            r, c = self._where(stray.nonzero()[0, 0])
            raise AssertionError(f"{what}: {int(stray.sum())} elements outside the view were written, first at (row {r}, col {c})")
        missing = ~wrote[idx]
        if bool(missing.any()):
            r, c = (int(v) for v in missing.nonzero()[0])
            raise AssertionError(f"{what}: {int(missing.sum())} elements of the view were left unwritten, first at (row {r}, col {c})")
        vals = self.parent.cpu()[idx].double()
        leak = ~torch.isfinite(vals)
        if bool(leak.any()):
            r, c = (int(v) for v in leak.nonzero()[0])
            raise AssertionError(f"{what}: {int(leak.sum())} non-finite elements in the view (a leak), first at (row {r}, col {c})")
        return vals, int((~inside).sum())

    def untouched(self):
        return bool((self.bits == self.sentinel).all())


def out_layout(flavour, width):
    """(ld, extra offset) of an output view of `width` columns."""
    assert flavour in FLAVOURS
    return (width + 8, 8) if flavour == "vec" else (width + 4, 5)


def err_over_bar(vals, ref, rtol, atol):
    """max |vals - ref| / (atol + rtol |ref|), the bar of tests.common.close (same float32 arithmetic)."""
    a, b = vals.float(), ref.float()
    if atol is None:
        atol = 2e-3 * max(1.0, float(b.abs().max()))
    r = (a - b).abs() / (atol + rtol * b.abs())
    return float(torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max())


class Prob:
    """One launch: `kw` for Recorder.gemm, the input views, the output views with their references and bars, what must be recorded."""

    def __init__(self, name, kw, views, outs, variant, sk=None, refused=False, spec=None, gn_in=None, gn_out=None, zero_cols=None):
        self.name, self.kw, self.views, self.outs = name, kw, views, outs          # outs: [(label, Out, ref [rows][width] float64, rtol, atol)]
        self.variant, self.sk, self.refused = variant, sk, refused                  # variant: substring of the recorded variant; sk: split count
        self.spec = spec or {}                                                      # what `emulate` needs
        self.gn_in = gn_in                                                          # GroupNorm in front: dict(srcs=[(view name, C, sums)], ...)
        self.gn_out = gn_out                                                        # (B, rows per image, kind): totals of the stored output
        self.zero_cols = zero_cols                                                  # boolean [width]: columns that must be exactly zero

    def assert_inside(self):
        for v in self.views.values():
            v.assert_inside()
        for _, o, _, _, _ in self.outs:
            o.assert_inside()

    def reset(self):
        for _, o, _, _, _ in self.outs:
            o.reset()

    def verify(self):
        """After the launch: (max error over bar, sentinel elements checked).  Prints each figure before it asserts."""
        worst, checked, vals0 = 0.0, 0, None
        for label, o, ref, rtol, atol in self.outs:
            what = f"{self.name} [{label}]"
            vals, n = o.check(what)
            e = err_over_bar(vals, ref, rtol, atol)
            print(f"{what}: max err/bar {e:.3f}, {n} sentinel elements checked")
            close(vals, ref, rtol=rtol, atol=atol, what=what)
            worst, checked = max(worst, e), checked + n
            vals0 = vals if vals0 is None else vals0
        self.vals = vals0                                                           # (the first output as stored, for the statistics check)
        if self.zero_cols is not None:
            assert float(vals0[:, self.zero_cols].abs().max()) == 0.0, f"{self.name}: the columns behind the valid keys carry probability"
        return worst, checked

    def untouched(self):
        return all(o.untouched() for _, o, _, _, _ in self.outs)


def _vec(x, device):
    """An fp32 vector inside an fp32-NaN parent: one guard row of the same length on either side, 8 pad lanes."""
    return View(x[None].float(), device, front=1, back=1, f32=True)


# ---------------------------------------------------------------------------------------------------- dense problems
def dense_problem(name, device, flavour, M, N, K, family="fast", tile_cfg=0, splitk=None, C1=0, colscale=False, R=False, r2=None, out_mode="f16",
                  rpb=0, ldc=None, extra=None, geglu=False, gw_nt=0, ln=False, n_t0=0, softmax=None, gn_groups=0, want_gn=False, bias=True,
                  refused=None, act=None, alpha=1.0, alpha_table=None):
    """A (strided, one or two sources) x W^T (strided row-major, or the packed stream of a BC_TILE_GW* configuration) + the epilogue modes of
    bc_gemm.  r2 = (out_w, xmin); softmax = (group, keep, valid); out_mode f16 / f16t / f32; act gelu / quick_gelu / silu; alpha: the scalar;
    alpha_table = (steps, step, per_image): the device table [steps] or [steps][M / rpb] behind a device step counter.  The reference follows
    the chain of include/blobctrl_hip.h: (acc + bias) -> act -> colscale -> alpha -> alpha_dev[...] -> + R -> + R2."""
    from blobctrl_amd import _lib
    from blobctrl_amd.weights import fold_layernorm, pack_gemm_wreg
    A, W, b = g(1, M, K), g(2, N, K) / math.sqrt(K), g(3, N)
    if ln or gn_groups:
        A = A * 1.5 + 0.4
    Ah, Wh, bq = A.half(), W.half(), b
    x = Ah.double()
    xin, views, gn_in = x, {}, None
    kw = dict(M=M, N=N, K=K, tile_cfg=tile_cfg, splitk=splitk)
    if C1:
        views["A"], views["A2"] = View(Ah[:, :C1], device), View(Ah[:, C1:], device)
        kw.update(A2=views["A2"].t, C1=C1, lda2=views["A2"].ld)
    else:
        views["A"] = View(Ah, device)
    kw.update(A=views["A"].parent, a_offset=views["A"].offset, lda=views["A"].ld)
    if ln:                                            # Linear(LayerNorm(x)) = rstd (x W'^T - mean colsum) + b' (weights.fold_layernorm): stated on W', b'
        gamma, beta = torch.rand(K, generator=torch.Generator().manual_seed(5)) + 0.5, g(6, K) * 0.1
        Wh, cs, bq = fold_layernorm(Wh, b, gamma, beta)
        xin = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
        views["ln_colsum"] = _vec(cs, device)
        kw.update(ln_colsum=views["ln_colsum"].t, ln_eps=1e-5)
    if gn_groups:                                     # GroupNorm applied while the rows are staged: statistics totals of the valid x from the host
        B = M // rpb
        gamma, beta = 1 + 0.2 * g(5, K), 0.2 * g(6, K)
        xb = x.view(B, rpb, K)
        y = F.group_norm(xb.permute(0, 2, 1), gn_groups, gamma.double(), beta.double(), 1e-6).permute(0, 2, 1).reshape(M, K)
        xin = y.half().double()
        gn_in = dict(srcs=[("A", K, torch.stack([xb.sum(1), (xb * xb).sum(1)], -1))], B=B, HW=rpb, G=gn_groups, eps=1e-6, gamma=gamma, beta=beta)
    acc = xin @ Wh.double().t()
    if bias:
        acc = acc + bq.double()
        views["bias"] = _vec(bq, device)
        kw.update(bias=views["bias"].t)
    if gw_nt:
        kw.update(W=pack_gemm_wreg(Wh.to(device), gw_nt))      # (the packed stream as it is)
    else:
        views["W"] = View(Wh, device)
        kw.update(W=views["W"].parent, w_offset=views["W"].offset, ldw=views["W"].ld)
    n_out, zero_cols = N, None
    if geglu:
        r4 = acc.view(M, N // 64, 2, 32)
        acc, n_out = (r4[:, :, 0] * F.gelu(r4[:, :, 1])).reshape(M, N // 2), N // 2
        kw.update(act=_lib.ACT_GEGLU)
    if softmax:
        group, keep, valid = softmax
        p = torch.zeros(M, N // group, keep, dtype=torch.float64)
        if N % group == 0:
            p[..., :valid] = torch.softmax(acc.view(M, N // group, group)[..., :valid], -1)
        else:
            assert refused, "a softmax group must divide N: no reference exists"
        acc, n_out = p.reshape(M, -1), N // group * keep
        zero_cols = (torch.arange(n_out) % keep) >= valid
        kw.update(sm_group=group, sm_keep=keep, sm_valid=valid)
    if act:
        acc = ACTS[act][1](acc)
        kw.update(act=getattr(_lib, ACTS[act][0]))
    if colscale:
        cs_ = 0.5 + torch.rand(n_out, generator=torch.Generator().manual_seed(5))        # (0.5 .. 1.5: where it stands in the chain matters)
        acc = acc * cs_.double()
        views["colscale"] = _vec(cs_, device)
        kw.update(colscale=views["colscale"].t)
    if alpha != 1.0:
        acc = acc * float(torch.tensor(alpha, dtype=torch.float32))                     # (the struct's float)
        kw.update(alpha=alpha)
    if alpha_table:
        # the table as a producer leaves it: one row per step, the launch reads the row a device counter names; every other row holds 9.0
        steps, step, per_image = alpha_table
        nb = M // rpb if per_image else 1
        tab = torch.full((steps, nb), 9.0)
        tab[step] = 0.5 + torch.rand(nb, generator=torch.Generator().manual_seed(11))
        acc = (acc.view(nb, -1, n_out) * tab[step].double()[:, None, None]).reshape(M, n_out)
        views["alpha"] = _vec(tab.flatten(), device)
        kw.update(alpha_dev=views["alpha"].t, alpha_idx=torch.tensor([step], dtype=torch.int32, device=device), alpha_bstride=nb if per_image else 0)
    if R:
        Rh = g(4, M, n_out).half()
        acc = acc + Rh.double()
        views["R"] = View(Rh, device)
        kw.update(R=views["R"].t, ldr=views["R"].ld)
    if rpb:
        kw.update(rows_per_batch=rpb)
    if r2:
        out_w, xmin = r2
        R2h = g(8, rpb, n_out).half()
        msk = (torch.arange(rpb) % out_w >= xmin).double()[None, :, None]
        acc = (acc.view(M // rpb, rpb, n_out) + R2h.double() * msk).reshape(M, n_out)
        views["R2"] = View(R2h, device)
        kw.update(R2=views["R2"].t, ldr2=views["R2"].ld, r2_xmin=xmin, r2_bmod=1, out_w=out_w)
    ld, ex = out_layout(flavour, n_out)
    ex = ex if extra is None else extra
    rtol, atol, outs, gn_out = 2e-3, None, [], None
    if out_mode == "f16t":
        B = M // rpb
        o = Out(B * N, rpb, ldc, device, ex)
        outs.append(("C^T", o, acc.view(B, rpb, N).permute(0, 2, 1).reshape(B * N, rpb), rtol, atol))
        kw.update(out_mode=_lib.OUT_F16_T)
    elif out_mode == "f32":
        o = Out(M, n_out, ld, device, ex, f32=True)
        outs.append(("C fp32", o, acc, 1e-4, 1e-4))
        kw.update(out_mode=_lib.OUT_F32)
    elif n_t0:
        B, nt = M // rpb, N - n_t0
        o = Out(M, n_t0, out_layout(flavour, n_t0)[0] if ldc is None else ldc, device, ex)
        ot = Out(B * nt, rpb, rpb + 8, device, 8)
        outs += [("C", o, acc[:, :n_t0], rtol, atol), ("C_t", ot, acc[:, n_t0:].view(B, rpb, nt).permute(0, 2, 1).reshape(B * nt, rpb), rtol, atol)]
        kw.update(C_t=ot.t, ldc_t=ot.ld, n_t0=n_t0)
    else:
        o = Out(M, n_out, ld if ldc is None else ldc, device, ex)
        outs.append(("C", o, acc, rtol, atol))
        if want_gn:
            kw.update(want_gn=True)
            gn_out = (M // rpb, rpb, family)
    kw.update(out=o.parent, out_offset=o.offset, ldc=o.ld)
    if refused is None:
        refused = flavour == "scalar" and family in ("gw", "g256")            # bc_gemm: "needs 16-byte aligned C / R / R2 / C_t and widths % 8 == 0"
    variant = {"generic": "gemm_kernel<", "gw": "gemm_wreg_kernel<", "g256": "gemm256_kernel<"}.get(family) or f"gemm_fast_kernel<{_lib.TILE_NAMES[tile_cfg]},"
    if family in ("gw", "g256"):
        variant += _lib.TILE_NAMES[tile_cfg] + ","
    spec = dict(kind="dense", M=M, N=N, K=K, n_out=n_out, act=act, alpha=alpha, alpha_table=alpha_table, rpb=rpb or M, f32=out_mode == "f32")
    return Prob(name, kw, views, outs, variant, sk=splitk, refused=refused, spec=spec, gn_in=gn_in, gn_out=gn_out, zero_cols=zero_cols)


# ---------------------------------------------------------------------------------------------------- convolutions
def conv_problem(name, device, flavour, B, H, W, Cin, Cout, family="fast", tile_cfg=0, stride=1, ups=False, C1=0, splitk=None, sk=None, gn=False,
                 resblock=False, want_gn=False, lda_pad=PAD, refused=None, nopad_lo=False, size=None, out_mode="f16", R=False):
    """3x3 convolution, pad 1, over NHWC pixels [B][H W][lda] with guard pixels (>= W + 1 and one 256-row tile) in front of image 0 and behind
    image B - 1.  gn: GroupNorm + SiLU in front (finalize in the kernel's prologue, statistics totals of the valid channels from the host);
    resblock: + time-embedding row through a step table + R + R2 from r2_xmin on.  nopad_lo: no padding on top and left, F.pad(x, (0, 1, 0, 1))
    in front of the convolution (the VAE encoder's downsampler): at an even H and stride 2 the last output row reads input row H - the bottom
    pad, which in memory is the first row of the next image or the guard pixels behind the last one.  ups / size: nearest upsample to twice
    the size / to an explicit size in front.  out_mode f16 / f32; R: + a residual."""
    from blobctrl_amd import _lib
    from blobctrl_amd.weights import pack_conv3x3, pack_conv_wreg
    x = g(1, B, Cin, H, W)
    if gn:
        x = x * 1.7 + 0.3
    w, b = g(2, Cout, Cin, 3, 3) / math.sqrt(9 * Cin), g(3, Cout)
    xh = x.half()
    src, gn_in = xh.double(), None
    pix = xh.permute(0, 2, 3, 1).reshape(B * H * W, Cin)
    guard = W + 1 + 256
    views = {}
    if C1:
        views["A"] = View(pix[:, :C1], device, ld=C1 + lda_pad, front=guard, back=guard)
        views["A2"] = View(pix[:, C1:], device, ld=Cin - C1 + lda_pad, front=guard, back=guard)
    else:
        views["A"] = View(pix, device, ld=Cin + lda_pad, front=guard, back=guard)
    assert not (ups and size)
    Hv, Wv = size if size else ((2 * H, 2 * W) if ups else (H, W))
    pads = 1 if nopad_lo else 2                                  # (bc_gemm's geometry check: Hout = (Hv + pads - 3) / stride + 1)
    Ho, Wo = (Hv + pads - 3) // stride + 1, (Wv + pads - 3) // stride + 1
    M, HWo = B * Ho * Wo, Ho * Wo
    kw = dict(M=M, N=Cout, K=9 * Cin, tile_cfg=tile_cfg, splitk=splitk, A=views["A"].parent, a_offset=views["A"].offset, lda=views["A"].ld,
              conv=dict(Cin=Cin, Hin=H, Win=W, Hv=Hv, Wv=Wv, Hout=Ho, Wout=Wo, stride=stride, nopad_lo=nopad_lo), rows_per_batch=HWo)
    if C1:
        kw.update(A2=views["A2"].t, C1=C1, lda2=views["A2"].ld)
    if gn:
        G = 8
        gamma, beta = 1.0 + 0.2 * g(5, Cin), 0.3 * g(6, Cin)
        src = F.silu(F.group_norm(src, G, gamma.double(), beta.double(), 1e-5)).half().double()
        xb = xh.double().permute(0, 2, 3, 1).reshape(B, H * W, Cin)
        sums = torch.stack([xb.sum(1), (xb * xb).sum(1)], -1)
        srcs = [("A", C1, sums[:, :C1]), ("A2", Cin - C1, sums[:, C1:])] if C1 else [("A", Cin, sums)]
        gn_in = dict(srcs=srcs, B=B, HW=H * W, G=G, eps=1e-5, gamma=gamma, beta=beta)
        kw.update(a_act=_lib.ACT_SILU)
    if ups:
        src = F.interpolate(src, scale_factor=2.0, mode="nearest")
    if size:
        src0, src = src, F.interpolate(src, size=size, mode="nearest")
        # (the reference's float scale and the kernel's integer floor(dst * in / out) name the same source pixels at this size)
        assert torch.equal(src, src0[:, :, torch.arange(Hv) * H // Hv][:, :, :, torch.arange(Wv) * W // Wv])
    wp =pack_conv3x3(w).half()
    if nopad_lo:
        ref = F.conv2d(F.pad(src, (0, 1, 0, 1)), w.half().double(), b.double(), stride=stride)
    else:
        ref = F.conv2d(src, w.half().double(), b.double(), stride=stride, padding=1)
    assert tuple(ref.shape[2:]) == (Ho, Wo)
    if family == "wreg":
        kw.update(W=pack_conv_wreg(wp).to(device))              # (the packed stream as it is)
    else:
        views["W"] = View(wp, device)
        kw.update(W=views["W"].parent, w_offset=views["W"].offset, ldw=views["W"].ld)
    views["bias"] = _vec(b, device)
    kw.update(bias=views["bias"].t)
    if resblock:
        steps, step, xmin = 3, 2, 8
        temb = g(7, steps * B, Cout).half()
        Rh, R2h = g(8, B, Cout, Ho, Wo).half(), g(9, 1, Cout, Ho, Wo).half()
        views["rowvec"] = View(temb, device, front=2, back=2)
        views["R"] = View(Rh.permute(0, 2, 3, 1).reshape(M, Cout), device)
        views["R2"] = View(R2h.permute(0, 2, 3, 1).reshape(HWo, Cout), device)
        ldv = views["rowvec"].ld
        kw.update(rowvec=views["rowvec"].t, ld_rowvec=ldv, rowvec_idx=torch.tensor([step], dtype=torch.int32, device=device), rowvec_step=B * ldv,
                  R=views["R"].t, ldr=views["R"].ld, R2=views["R2"].t, ldr2=views["R2"].ld, r2_xmin=xmin, r2_bmod=1, out_w=Wo)
        ref = ref + temb.double().view(steps, B, Cout)[step][:, :, None, None] + Rh.double()
        ref[..., xmin:] += R2h.double()[..., xmin:]
    if R:
        assert not resblock
        Rh = g(8, B, Cout, Ho, Wo).half()
        views["R"] = View(Rh.permute(0, 2, 3, 1).reshape(M, Cout), device)
        kw.update(R=views["R"].t, ldr=views["R"].ld)
        ref = ref + Rh.double()
    ld, ex = out_layout(flavour, Cout)
    o = Out(M, Cout, ld, device, ex, f32=out_mode == "f32")
    kw.update(out=o.parent, out_offset=o.offset, ldc=o.ld)
    if out_mode == "f32":
        kw.update(out_mode=_lib.OUT_F32)
    gn_out = None
    if want_gn:
        kw.update(want_gn=True)
        gn_out = (B, HWo, family)
    halo = family in ("halo", "wreg")
    if refused is None:
        refused = flavour == "scalar" and halo                 # bc_gemm: the halo convolutions store 16 bytes at a time
    variant = {"halo": "conv_halo_kernel<", "wreg": "conv_wreg_kernel<", "generic": "gemm_kernel<"}.get(family) or \
        f"gemm_fast_kernel<{_lib.TILE_NAMES[tile_cfg]},"
    if gn:
        variant += _lib.TILE_NAMES[tile_cfg] + ",halo_gnfin"
    spec = dict(kind="conv", B=B, H=H, W=W, Cin=Cin, N=Cout, M=M, n_out=Cout, stride=stride, nopad_lo=nopad_lo, Hv=Hv, Wv=Wv, Ho=Ho, Wo=Wo,
                f32=out_mode == "f32")
    ref = ref.permute(0, 2, 3, 1).reshape(M, Cout)
    outs = [("C fp32", o, ref, 1e-4, 1e-4)] if out_mode == "f32" else [("C", o, ref, 4e-3 if gn else 2e-3, None)]
    return Prob(name, kw, views, outs, variant, sk=sk if sk is not None else splitk, refused=refused, spec=spec, gn_in=gn_in, gn_out=gn_out)


# ---------------------------------------------------------------------------------------------------- the VAE mid-block attention
def pad8(n):
    return (n + 7) // 8 * 8


ATTN_STAGES = ("scores", "probs", "o")
ATTN_SHAPES = [(2, 72, 64), (1, 64, 128)]          # (B, N, C): N = 72 is a ragged second 64-tile and 8-aligned, as vae.py requires; K = 72
                                                   # sends P V to the generic kernel, every other launch is gemm_fast


class AttnProb(Prob):
    """The three launches per image of AutoencoderKL._attend - Q K^T with the scale as alpha, bc_softmax_rows in place, P V against V^T - on
    fenced buffers: `check(b, stage)` after each launch, `verify()` after the last.  The score buffer holds ONE image: it is reset to the
    sentinel in front of each image's Q K^T, so that what is checked is what that launch wrote."""

    def __init__(self, name, views, s, o, refs, B, N, C):
        from tests.attention_common import BAR_ATOL, BAR_RTOL
        super().__init__(name, None, views, [("o", o, refs["o"], BAR_RTOL, BAR_ATOL)], None, spec=dict(kind="vae_attn", B=B, N=N, C=C))
        self.s, self.o, self.refs = s, o, refs
        # the scores are a dense GEMM's output: the dense bar; probabilities and the product: the attention bar (tests/attention_common.py)
        self.bars = dict(scores=(2e-3, None), probs=(BAR_RTOL, BAR_ATOL), o=(BAR_RTOL, BAR_ATOL))
        # kind and variant of the launches `_attend` records per image
        fast = lambda k: "gemm_fast_kernel<" if k % 64 == 0 else "gemm_kernel<"
        self.launches = [("vae_attn", fast(C)), ("softmax", ""), ("vae_attn", fast(pad8(N)))]
        self.worst, self.checked = {}, 0

    def assert_inside(self):
        super().assert_inside()
        self.s.assert_inside()

    def reset(self):
        self.s.reset()
        self.o.reset()
        self.worst, self.checked = {}, 0

    def untouched(self):
        return self.s.untouched() and self.o.untouched()

    def check(self, b, stage):
        """After launch `stage` of image b: the score buffer (or the rows of o written so far) is written, finite and inside its bar, every
        sentinel around it is unchanged.  Prints the figure before it asserts."""
        N = self.spec["N"]
        what = f"{self.name} [image {b}: {stage}]"
        if stage == "o":
            vals, n = self.o.check(what, rows=(b + 1) * N)
            ref = self.refs["o"][:(b + 1) * N]
        else:
            vals, n = self.s.check(what)
            ref = self.refs[stage][b]
        rtol, atol = self.bars[stage]
        e = err_over_bar(vals, ref, rtol, atol)
        print(f"{what}: max err/bar {e:.3f}, {n} sentinel elements checked")
        close(vals, ref, rtol=rtol, atol=atol, what=what)
        self.worst[stage] = max(self.worst.get(stage, 0.0), e)
        self.checked += n
        return e

    def verify(self):
        assert sorted(self.worst) == sorted(ATTN_STAGES), f"{self.name}: not every stage was checked"
        for name, v in self.views.items():
            assert v.guards_intact(), f"{self.name}: the NaN guards around {name} were written"
        return max(self.worst.values()), self.checked


def vae_attention_problem(device, B, N, C, qk_scale=1.0):
    """The buffers of the VAE mid-block attention (blobctrl_amd/vae.py: _mid, _attend) as the producers leave them, fenced: qk [B N][2 C]
    (q | k; the weight operand of Q K^T is columns C .. 2 C of the same rows, image b at a per-image offset) and vt [B C][pad8(N)] (V
    transposed, pad columns zero) inside NaN parents - packed rows, as `_attend` addresses them: NaN guard rows in front and behind -, the
    score buffer s [N][pad8(N)] of one image and o [B N][C] inside sentinel parents.  The float64 references - scaled scores, softmax,
    product - are computed from the fp16-rounded operands, nothing rounded in between."""
    assert N % 8 == 0, "VAE attention needs a token count that is a multiple of 8"
    Np = pad8(N)
    qkh = (g(1, B * N, 2 * C) * qk_scale).half()
    vh = g(2, B, N, C).half()
    vth = torch.zeros(B, C, Np, dtype=torch.float16)
    vth[:, :, :N] = vh.permute(0, 2, 1)
    views = dict(qk=View(qkh, device, ld=2 * C), vt=View(vth.reshape(B * C, Np), device, ld=Np))
    q, k = qkh.double().view(B, N, 2 * C)[..., :C], qkh.double().view(B, N, 2 * C)[..., C:]
    scores = q @ k.transpose(1, 2) * float(torch.tensor(C ** -0.5, dtype=torch.float32))          # (alpha is the struct's float)
    probs = torch.softmax(scores, -1)
    refs = dict(scores=scores, probs=probs, o=(probs @ vh.double()).reshape(B * N, C))
    s, o = Out(N, N, Np, device, 8), Out(B * N, C, C, device, 8)
    return AttnProb(f"vae-attention-B{B}-N{N}-C{C}", views, s, o, refs, B, N, C)


def emulate_attention(prob, mutation=None):
    """`_attend` in torch, float64 arithmetic, rounded to fp16 exactly where the three launches store (scores, probabilities, product), checked
    after each launch.  Against the float64 references this is the floor the storage formats leave of each bar.  w_image0: image 0's K rows
    used for every image."""
    assert mutation in (None, "w_image0")
    B, N, C = (prob.spec[k] for k in "BNC")
    Np, qk, vt, s, o = pad8(N), prob.views["qk"], prob.views["vt"], prob.s, prob.o
    alpha = float(torch.tensor(C ** -0.5, dtype=torch.float32))
    sv = s.parent.as_strided((N, N), (s.ld, 1), s.offset)
    for b in range(B):
        s.reset()
        bw = 0 if mutation == "w_image0" else b
        A = qk.parent.as_strided((N, C), (qk.ld, 1), qk.offset + b * N * 2 * C).double()
        Wm = qk.parent.as_strided((N, C), (qk.ld, 1), qk.offset + bw * N * 2 * C + C).double()
        sv.copy_((A @ Wm.t() * alpha).half())
        prob.check(b, "scores")
        sv.copy_(torch.softmax(sv.double(), -1).half())
        prob.check(b, "probs")
        P = s.parent.as_strided((N, Np), (s.ld, 1), s.offset).double()
        Vt = vt.parent.as_strided((C, Np), (vt.ld, 1), vt.offset + b * C * Np).double()
        o.parent.as_strided((N, C), (o.ld, 1), o.offset + b * N * C).copy_((P @ Vt.t()).half())
        prob.check(b, "o")


# ---------------------------------------------------------------------------------------------------- the case tables
# front_end: a launch form of the VAE / CLIP / DINOv2 / SAM front ends, added after tests/golden/gemm_records_before_resolve.json was frozen
# (tests/gemm_records_common.py records the cases that file knows)
Case = namedtuple("Case", "id fn args front_end", defaults=(False,))


def build(case, flavour, device):
    return case.fn(f"{case.id}/{flavour}", device, flavour, **case.args)


def _front_end(id_, fn, args):
    return Case(id_, fn, args, True)


def _tiles():
    from blobctrl_amd import _lib
    return _lib


def generic_cases():
    """The generic kernel (K % 64 != 0): ragged M / N / K, a single 8-wide K step, and the production rank-1 collapse (engine.record_collapse:
    one column of an 8-wide weight matrix, columns 0-4 and 6-7 of every row must survive)."""
    return [Case("generic-130x72x200", dense_problem, dict(M=130, N=72, K=200, family="generic", colscale=True, R=True)),
            Case("generic-33x8x8", dense_problem, dict(M=33, N=8, K=8, family="generic")),
            Case("generic-rank1-collapse", dense_problem, dict(M=128, N=1, K=1032, family="generic", bias=False, ldc=8, extra=5))] + \
        generic_front_end_cases()


def generic_front_end_cases():
    """Convolutions on the generic kernel (Cin % 64 != 0: the tap is computed per 16-byte chunk, one 64-wide K tile spans several taps; the
    VAE's conv_in at Cin = 8, K = 72): stride 1 and 2, the VAE encoder's pad = (0, 1, 0, 1) downsampler at an even size (the last output row
    and column read the bottom / right pad: row H is the next image's first row, or the guard pixels) and at an odd one, the upsample gather at
    an explicit size and at twice the size, the fp32 output at N = 3 (decoder.conv_out), N = 8 with a residual, and Cin = 24, where a K tile
    ends inside a tap (three row tiles at B = 3).  At 5 x 6 -> 9 x 11 floor(i * 5 / 9) equals i >> 1 for every i: 8 x 9 is the size at which
    a gather that shifts where it should scale reads other pixels.  And the scalar epilogue at n_out % 8 != 0 through GELU, LayerScale and
    the per-image table."""
    c = dict(B=2, H=9, W=11, Cin=8, Cout=40, family="generic", lda_pad=0)                             # (the gather reads packed pixels)
    return [_front_end("generic-conv-9x11-s1-N72", conv_problem, dict(c, Cout=72)),
            _front_end("generic-conv-10x12-s2", conv_problem, dict(c, H=10, W=12, stride=2)),
            _front_end("generic-conv-10x12-s2-nopad_lo", conv_problem, dict(c, H=10, W=12, stride=2, nopad_lo=True)),
            _front_end("generic-conv-9x11-s2-nopad_lo", conv_problem, dict(c, stride=2, nopad_lo=True)),
            _front_end("generic-conv-5x6-size9x11", conv_problem, dict(c, H=5, W=6, size=(9, 11))),
            _front_end("generic-conv-5x6-size8x9", conv_problem, dict(c, H=5, W=6, size=(8, 9))),
            _front_end("generic-conv-5x6-ups", conv_problem, dict(c, H=5, W=6, ups=True)),
            # Cin % 64 == 0 and twice the size, yet not gemm_fast's: its upsample gather has the window origin of pad 1 built in
            _front_end("generic-conv-5x6-ups-nopad_lo-Cin64", conv_problem, dict(c, H=5, W=6, Cin=64, ups=True, nopad_lo=True)),
            _front_end("generic-conv-N3-f32", conv_problem, dict(c, Cout=3, out_mode="f32")),
            _front_end("generic-conv-N8-R", conv_problem, dict(c, Cout=8, R=True)),
            _front_end("generic-conv-Cin24-B3", conv_problem, dict(c, B=3, Cin=24)),
            _front_end("generic-130x20x72-gelu-colscale-alpha_per_image", dense_problem,
                       dict(M=130, N=20, K=72, family="generic", act="gelu", colscale=True, rpb=65, alpha_table=(2, 1, True)))]


FAST_MODES = ("dense", "two_source", "splitk3_R", "t100_ldc104", "t100_ldc112", "t77_ldc80", "t96_ldc104", "f32", "geglu", "geglu_sk2",
              "conv1", "conv2", "ups", "conv1_strided_pixels",
              "conv2_nopad", "conv2_nopad_odd", "act_gelu", "act_quick_gelu", "act_silu", "alpha_per_image", "alpha_scalar_sk3")
FAST_FRONT_END_MODES = FAST_MODES[14:]


def fast_case(cfg, mode):
    """gemm_fast, one tile configuration x operand / output mode, on ragged M / N (300 x 200) and a K loop of 3 k-steps."""
    d = dict(family="fast", tile_cfg=cfg, splitk=1)
    conv = dict(B=2, H=9, W=11, Cin=64, Cout=72, family="fast", tile_cfg=cfg, splitk=1, lda_pad=0)       # (the gather reads packed pixels)
    table = {
        "dense": (dense_problem, dict(d, M=300, N=200, K=192, colscale=True)),
        "two_source": (dense_problem, dict(d, M=300, N=200, K=192, C1=128)),
        "splitk3_R": (dense_problem, dict(d, M=300, N=200, K=640, splitk=3, R=True)),
        # rows_per_batch = 100 and 77 are no multiple of 8: the scalar transposed store in either flavour; 96 is: the 16-byte store along the
        # token axis where C is 16-byte aligned (the flavour decides the offset: 8 or 5 elements)
        "t100_ldc104": (dense_problem, dict(d, M=300, N=200, K=192, out_mode="f16t", rpb=100, ldc=104)),
        "t100_ldc112": (dense_problem, dict(d, M=300, N=200, K=192, out_mode="f16t", rpb=100, ldc=112)),
        "t77_ldc80": (dense_problem, dict(d, M=231, N=200, K=192, out_mode="f16t", rpb=77, ldc=80)),
        "t96_ldc104": (dense_problem, dict(d, M=288, N=200, K=192, out_mode="f16t", rpb=96, ldc=104)),
        "f32": (dense_problem, dict(d, M=300, N=200, K=192, out_mode="f32")),
        "geglu": (dense_problem, dict(d, M=300, N=320, K=192, geglu=True)),
        "geglu_sk2": (dense_problem, dict(d, M=300, N=320, K=192, geglu=True, splitk=2)),
        "conv1": (conv_problem, dict(conv)),
        "conv2": (conv_problem, dict(conv, stride=2)),
        "ups": (conv_problem, dict(conv, ups=True)),
        # refused by design: the gather kernels address pixel * Cin, a wider pixel stride would be ignored
        "conv1_strided_pixels": (conv_problem, dict(conv, lda_pad=PAD, refused=True)),
        # the VAE encoder's downsampler: at 10 x 12 output row 4 and column 5 read the bottom / right pad (input row 10, column 12)
        "conv2_nopad": (conv_problem, dict(conv, H=10, W=12, stride=2, nopad_lo=True)),
        "conv2_nopad_odd": (conv_problem, dict(conv, stride=2, nopad_lo=True)),
        # act -> colscale -> alpha (DINOv2 / SAM: GELU; CLIP: quick-GELU)
        "act_gelu": (dense_problem, dict(d, M=300, N=200, K=192, act="gelu", colscale=True, alpha=0.5)),
        "act_quick_gelu": (dense_problem, dict(d, M=300, N=200, K=192, act="quick_gelu", colscale=True, alpha=0.5)),
        "act_silu": (dense_problem, dict(d, M=300, N=200, K=192, act="silu", colscale=True, alpha=0.5)),
        # BlobNet's zero-convs: step 1 of a [2][3] table (the other row holds 9.0), one scalar per image of 100 rows
        "alpha_per_image": (dense_problem, dict(d, M=300, N=200, K=192, rpb=100, alpha_table=(2, 1, True))),
        "alpha_scalar_sk3": (dense_problem, dict(d, M=300, N=200, K=640, splitk=3, alpha_table=(2, 1, False))),
    }
    fn, args = table[mode]
    return Case(f"fast{cfg}-{mode}", fn, args, mode in FAST_FRONT_END_MODES)


GW_MODES = ("plain_bias_R", "ln", "two_source", "C_t", "softmax", "gn_rows", "alpha")


def gw_case(cfg, M, mode):
    """BC_TILE_GW64x128 / 256 / 320 at K = 320: N = 256 / 256 / 320 (two column tiles of GW64x128, one of each of the others).  C_t needs a
    row-major and a transposed column tile: with one tile it is refused, so the case that runs has two (N = 2 BN).  The softmax epilogue
    exists on GW64x128 only (a softmax group is one 64 x 128 workgroup): refused on the other two."""
    lib = _tiles()
    nt = lib.GW_TILES[cfg]
    bn = 64 * nt
    N = 256 if nt < 5 else 320
    d = dict(family="gw", tile_cfg=cfg, gw_nt=nt, M=M, N=N, K=320)
    table = {
        "plain_bias_R": dict(d, R=True),
        "ln": dict(d, ln=True),
        "two_source": dict(d, K=640, C1=320),
        "C_t": dict(d, n_t0=128 if N == bn else bn, rpb=64, refused=True if N == bn else None),
        "C_t_two_tiles": dict(d, N=2 * bn, n_t0=bn, rpb=64),
        "softmax": dict(d, softmax=(128, 80, 77), refused=True if nt != 2 else None),
        "gn_rows": dict(d, gn_groups=32, rpb=64),
        "alpha": dict(d, alpha=0.5),
    }
    return Case(f"{lib.TILE_NAMES[cfg]}-M{M}-{mode}", dense_problem, table[mode], mode == "alpha")


def gw_cases():
    lib = _tiles()
    out = []
    for cfg in (lib.TILE_GW64x128, lib.TILE_GW64x256, lib.TILE_GW64x320):
        for M in (64, 128):
            out += [gw_case(cfg, M, mode) for mode in GW_MODES]
            if lib.GW_TILES[cfg] != 2:
                out.append(gw_case(cfg, M, "C_t_two_tiles"))
    return out


def g256_cases():
    lib = _tiles()
    d = dict(family="g256", tile_cfg=lib.TILE_G256)
    return [Case("g256-256x256x128", dense_problem, dict(d, M=256, N=256, K=128)),
            Case("g256-512x512x256-two_source", dense_problem, dict(d, M=512, N=512, K=256, C1=128)),
            Case("g256-C_t", dense_problem, dict(d, M=512, N=512, K=256, n_t0=256, rpb=256)),
            Case("g256-transposed", dense_problem, dict(d, M=512, N=256, K=128, out_mode="f16t", rpb=256, ldc=264)),
            Case("g256-geglu", dense_problem, dict(d, M=256, N=256, K=128, geglu=True)),
            Case("g256-R_R2_gn", dense_problem, dict(d, M=512, N=512, K=256, R=True, r2=(16, 8), rpb=256, want_gn=True)),
            _front_end("g256-gelu-alpha", dense_problem, dict(d, M=256, N=256, K=128, act="gelu", alpha=0.5))]


def halo_cases(family):
    """BC_TILE_HALO / BC_TILE_WREG: one 8 x 16 tile per image and two, two sources, a last K split shorter than the others (3 chunks in 2
    splits: 2 + 1; 5 in 2: 3 + 2; 5 in 3: 2 + 2 + 1), the fused GroupNorm + SiLU with the in-kernel finalize, the ResBlock epilogue."""
    lib = _tiles()
    cfg = lib.TILE_WREG if family == "wreg" else lib.TILE_HALO
    d = dict(family=family, tile_cfg=cfg, B=2, H=8, W=16, Cin=64, Cout=160, splitk=1)
    cases = [Case(f"{family}-8x16", conv_problem, dict(d)),
             Case(f"{family}-16x16", conv_problem, dict(d, H=16)),
             Case(f"{family}-two_source-128+64", conv_problem, dict(d, Cin=192, C1=128)),
             Case(f"{family}-Cin192-sk2", conv_problem, dict(d, Cin=192, splitk=2)),
             Case(f"{family}-Cin320-sk2", conv_problem, dict(d, Cin=320, splitk=2)),
             Case(f"{family}-Cin320-sk3", conv_problem, dict(d, Cin=320, splitk=3)),
             Case(f"{family}-gn_silu-16x16", conv_problem, dict(d, H=16, gn=True, want_gn=True)),
             Case(f"{family}-gn_silu-two_source-sk2", conv_problem, dict(d, Cin=192, C1=128, splitk=2, gn=True, want_gn=True)),
             Case(f"{family}-resblock-epilogue", conv_problem, dict(d, resblock=True)),
             Case(f"{family}-resblock-epilogue-sk2", conv_problem, dict(d, Cin=192, splitk=2, resblock=True, want_gn=True))]
    if family == "wreg":
        cases.append(Case("wreg-upsample-4x8", conv_problem, dict(d, H=4, W=8, ups=True)))
    # refused by design (bc_conv_halo_ok): the LDS-resident halo tile is staged for pad 1 on every side
    cases.append(_front_end(f"{family}-nopad_lo-refused", conv_problem, dict(d, nopad_lo=True, refused=True)))
    return cases


# ---------------------------------------------------------------------------------------------------- a torch statement of the kernel
MUTATIONS = ("store_vec8", "rows_round64", "skip_one", "k_round64", "row_M", "bias_lane", "halo_unchecked",
             "pad_lo_kept", "pad_hi_unchecked", "ups_shift", "act_swapped", "scale_before_act", "alpha_image0", "alpha_next_step", "w_image0")


def emulate(prob, mutation=None):
    """What the kernel does, in torch: reads the views it is given, computes in float64, stores fp16 (fp32) into the output view.  Dense: A W^T;
    conv: the 3x3 gather at the problem's stride, padding (nopad_lo) and virtual size (Hv x Wv); then the epilogue chain + bias -> act ->
    colscale -> alpha -> table entry -> + R.  The VAE attention problem: emulate_attention.  `mutation` makes one of the mistakes a kernel can
    make:
    store_vec8 (a full 8-wide vector stored at the last column), rows_round64 (M rounded up to 64 rows stored), skip_one (one element left
    unwritten), k_round64 (K rounded up to 64 read from A), row_M (row M of A added into row M - 1), bias_lane (bias lane n_out added into
    column n_out - 1), halo_unchecked (conv: the halo row -1 of image 0 fetched without the bounds test), pad_lo_kept (conv: nopad_lo ignored
    in the gather origin), pad_hi_unchecked (conv: an index equal to Hv or Wv fetched without the bounds test), ups_shift (conv: >> 1 in place
    of * Hin / Hv at an explicit upsample size), act_swapped (quick-GELU where GELU was asked for), scale_before_act (colscale applied
    before the activation), alpha_image0 (image 0's table entry for every image), alpha_next_step (the table row of step + 1), w_image0 (VAE
    attention: image 0's K rows for every image)."""
    assert mutation is None or mutation in MUTATIONS
    s, v = prob.spec, prob.views
    if s["kind"] == "vae_attn":
        return emulate_attention(prob, mutation)
    M, N = s["M"], s["N"]
    Wv = v["W"]
    if s["kind"] == "dense":
        K, a = s["K"], v["A"]
        A = a.parent.as_strided((M, K), (a.ld, 1), a.offset).double()
        Wm = Wv.parent.as_strided((N, K), (Wv.ld, 1), Wv.offset).double()
        acc = A @ Wm.t()
        if mutation == "k_round64":
            K64 = (K + 63) // 64 * 64
            acc = acc + a.parent.as_strided((M, K64 - K), (a.ld, 1), a.offset + K).double().sum(1, keepdim=True)
        if mutation == "row_M":
            acc[M - 1] += a.parent.as_strided((K,), (1,), a.offset + M * a.ld).double() @ Wm.t()
    else:
        B, H, W, Cin, a = s["B"], s["H"], s["W"], s["Cin"], v["A"]
        Hv, Wv_, Ho, Wo, stride = s["Hv"], s["Wv"], s["Ho"], s["Wo"], s["stride"]
        pad_lo = 0 if s["nopad_lo"] and mutation != "pad_lo_kept" else 1
        Wm = Wv.parent.as_strided((N, 9, Cin), (Wv.ld, Cin, 1), Wv.offset).double()
        flat = a.parent.double()
        bb, oy, ox = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), indexing="ij")
        acc = torch.zeros(B, Ho, Wo, N, dtype=torch.float64)
        hi = 1 if mutation == "pad_hi_unchecked" else 0
        for tap in range(9):
            iy, ix = oy * stride - pad_lo + tap // 3, ox * stride - pad_lo + tap % 3          # (on the virtual Hv x Wv grid)
            ok = (iy >= 0) & (iy < Hv + hi) & (ix >= 0) & (ix < Wv_ + hi)
            if mutation == "halo_unchecked":
                ok = ok | ((bb == 0) & (iy == -1))
            if (Hv, Wv_) != (H, W):                                                # nearest: src = floor(dst * in / out)
                if mutation == "ups_shift":
                    iy, ix = iy >> 1, ix >> 1
                else:
                    iy, ix = torch.div(iy * H, Hv, rounding_mode="floor"), torch.div(ix * W, Wv_, rounding_mode="floor")
            pix = (bb * H + iy) * W + ix                                           # (negative in front of image 0)
            idx = a.offset + pix[..., None] * a.ld + torch.arange(Cin)
            val = torch.where(ok[..., None], flat[idx.clamp(0, flat.numel() - 1)], torch.zeros((), dtype=torch.float64))
            acc += val @ Wm[:, tap].t()
        acc = acc.reshape(M, N)
    if "bias" in v:
        bias_p, bias_o = v["bias"].parent.double(), v["bias"].offset
        acc = acc + bias_p[bias_o:bias_o + N]
        if mutation == "bias_lane":
            acc[:, N - 1] += bias_p[bias_o + N]
    cs = 1.0
    if "colscale" in v:
        cs = v["colscale"].parent.double()[v["colscale"].offset:v["colscale"].offset + N]
    if mutation == "scale_before_act":
        acc, cs = acc * cs, 1.0
    act = s.get("act")
    if act:
        acc = ACTS["quick_gelu" if mutation == "act_swapped" and act == "gelu" else act][1](acc)
    acc = acc * cs
    acc = acc * float(torch.tensor(s.get("alpha", 1.0), dtype=torch.float32))
    if s.get("alpha_table"):
        steps, step, per_image = s["alpha_table"]
        nb = M // s["rpb"] if per_image else 1
        tab, row = v["alpha"], step + (1 if mutation == "alpha_next_step" else 0)
        img = torch.arange(M) // s["rpb"] if per_image and mutation != "alpha_image0" else torch.zeros(M, dtype=torch.long)
        acc = acc * tab.parent.double()[tab.offset + row * nb + img][:, None]
    if "R" in v:
        r = v["R"]
        acc = acc + r.parent.as_strided((M, N), (r.ld, 1), r.offset).double()
    _, o, _, _, _ = prob.outs[0]
    dst = o.parent
    rows = M if mutation != "rows_round64" else (M + 63) // 64 * 64
    val = torch.zeros(rows, N, dtype=dst.dtype)
    val[:M] = acc.to(dst.dtype)
    dst.as_strided((rows, N), (o.ld, 1), o.offset).copy_(val)
    if mutation == "store_vec8":
        dst.as_strided((M, 8), (o.ld, 1), o.offset + N - 1).copy_(val[:M, N - 1:].expand(M, 8))
    if mutation == "skip_one":
        o.bits[o.offset + (M // 2) * o.ld + N // 3] = o.sentinel
