"""A `bc_gemm` problem whose every operand is a view inside a larger, hostile parent (tests/test_gemm_views_gpu.py, tests/test_gemm_views_cpu.py).

Inputs: A / A2 (row or pixel stride = width + 8), a row-major W (ldw = K + 8), bias, colscale, ln_colsum, the row-vector table, R and R2 lie
inside parents filled with fp16 / fp32 NaN: the pad columns, guard rows in front of row 0 and behind the last row (for a convolution: guard
pixels in front of image 0 and behind the last image).  A K tail, an M-tail row, a weight row past N, a halo pixel outside the batch or a bias
lane past N that reaches a product makes the output NaN.  Outputs: C (and C_t) start `offset` elements into a parent filled with the NaN bit
pattern 0x7E5A (fp32: 0x7FC5A5A5), row stride > width, guard rows in front and behind up to the next multiple of 256 rows plus one more
256-row tile; after the launch every element of the view differs from the sentinel and is finite, every other element of the parent is
bit-equal to the sentinel.  The float64 reference is computed from the fp16-rounded valid sub-tensors only; the bars are the project's own,
through tests.common.close.  Nothing here needs a device: `emulate` is a torch statement of the kernel (with the mistakes a kernel can make)
that tests/test_gemm_views_cpu.py drives the same harness with."""
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

    def check(self, what):
        """(values [rows][width] float64, count of sentinel elements checked).  Fails when an element outside the view was written, when
        one inside was not, or when one inside is not finite - with the count and the first offending (row, col) of the view's grid."""
        bits = self.bits.cpu()
        idx = self.offset + torch.arange(self.rows)[:, None] * self.ld + torch.arange(self.width)[None, :]
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
                  refused=None):
    """A (strided, one or two sources) x W^T (strided row-major, or the packed stream of a BC_TILE_GW* configuration) + the epilogue modes of
    bc_gemm.  r2 = (out_w, xmin); softmax = (group, keep, valid); out_mode f16 / f16t / f32."""
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
    if colscale:
        cs_ = 1 + 0.5 * g(5, n_out)
        acc = acc * cs_.double()
        views["colscale"] = _vec(cs_, device)
        kw.update(colscale=views["colscale"].t)
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
    spec = dict(kind="dense", M=M, N=N, K=K, n_out=n_out)
    return Prob(name, kw, views, outs, variant, sk=splitk, refused=refused, spec=spec, gn_in=gn_in, gn_out=gn_out, zero_cols=zero_cols)


# ---------------------------------------------------------------------------------------------------- convolutions
def conv_problem(name, device, flavour, B, H, W, Cin, Cout, family="fast", tile_cfg=0, stride=1, ups=False, C1=0, splitk=None, sk=None, gn=False,
                 resblock=False, want_gn=False, lda_pad=PAD, refused=None):
    """3x3 convolution, pad 1, over NHWC pixels [B][H W][lda] with guard pixels (>= W + 1 and one 256-row tile) in front of image 0 and behind
    image B - 1.  gn: GroupNorm + SiLU in front (finalize in the kernel's prologue, statistics totals of the valid channels from the host);
    resblock: + time-embedding row through a step table + R + R2 from r2_xmin on."""
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
    Hv, Wv = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = (Hv - 1) // stride + 1, (Wv - 1) // stride + 1
    M, HWo = B * Ho * Wo, Ho * Wo
    kw = dict(M=M, N=Cout, K=9 * Cin, tile_cfg=tile_cfg, splitk=splitk, A=views["A"].parent, a_offset=views["A"].offset, lda=views["A"].ld,
              conv=dict(Cin=Cin, Hin=H, Win=W, Hv=Hv, Wv=Wv, Hout=Ho, Wout=Wo, stride=stride), rows_per_batch=HWo)
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
    wp = pack_conv3x3(w).half()
    ref = F.conv2d(src, w.half().double(), b.double(), stride=stride, padding=1)
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
    ld, ex = out_layout(flavour, Cout)
    o = Out(M, Cout, ld, device, ex)
    kw.update(out=o.parent, out_offset=o.offset, ldc=o.ld)
    gn_out = None
    if want_gn:
        kw.update(want_gn=True)
        gn_out = (B, HWo, family)
    halo = family in ("halo", "wreg")
    if refused is None:
        refused = flavour == "scalar" and halo                 # bc_gemm: the halo convolutions store 16 bytes at a time
    variant = {"halo": "conv_halo_kernel<", "wreg": "conv_wreg_kernel<"}.get(family) or f"gemm_fast_kernel<{_lib.TILE_NAMES[tile_cfg]},"
    if gn:
        variant += _lib.TILE_NAMES[tile_cfg] + ",halo_gnfin"
    spec = dict(kind="conv", B=B, H=H, W=W, Cin=Cin, N=Cout, M=M, n_out=Cout)
    outs = [("C", o, ref.permute(0, 2, 3, 1).reshape(M, Cout), 4e-3 if gn else 2e-3, None)]
    return Prob(name, kw, views, outs, variant, sk=sk if sk is not None else splitk, refused=refused, spec=spec, gn_in=gn_in, gn_out=gn_out)


# ---------------------------------------------------------------------------------------------------- the case tables
Case = namedtuple("Case", "id fn args")


def build(case, flavour, device):
    return case.fn(f"{case.id}/{flavour}", device, flavour, **case.args)


def _tiles():
    from blobctrl_amd import _lib
    return _lib


def generic_cases():
    """The generic kernel (K % 64 != 0): ragged M / N / K, a single 8-wide K step, and the production rank-1 collapse (engine.record_collapse:
    one column of an 8-wide weight matrix, columns 0-4 and 6-7 of every row must survive)."""
    return [Case("generic-130x72x200", dense_problem, dict(M=130, N=72, K=200, family="generic", colscale=True, R=True)),
            Case("generic-33x8x8", dense_problem, dict(M=33, N=8, K=8, family="generic")),
            Case("generic-rank1-collapse", dense_problem, dict(M=128, N=1, K=1032, family="generic", bias=False, ldc=8, extra=5))]


FAST_MODES = ("dense", "two_source", "splitk3_R", "t100_ldc104", "t100_ldc112", "t77_ldc80", "t96_ldc104", "f32", "geglu", "geglu_sk2",
              "conv1", "conv2", "ups", "conv1_strided_pixels")


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
    }
    fn, args = table[mode]
    return Case(f"fast{cfg}-{mode}", fn, args)


GW_MODES = ("plain_bias_R", "ln", "two_source", "C_t", "softmax", "gn_rows")


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
    }
    return Case(f"{lib.TILE_NAMES[cfg]}-M{M}-{mode}", dense_problem, table[mode])


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
            Case("g256-R_R2_gn", dense_problem, dict(d, M=512, N=512, K=256, R=True, r2=(16, 8), rpb=256, want_gn=True))]


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
    return cases


# ---------------------------------------------------------------------------------------------------- a torch statement of the kernel
MUTATIONS = ("store_vec8", "rows_round64", "skip_one", "k_round64", "row_M", "bias_lane", "halo_unchecked")


def emulate(prob, mutation=None):
    """What the kernel does, in torch: reads the views it is given, computes in float64, stores fp16 into the output view.  Dense: A W^T + bias
    (+ R); conv: 3x3, stride 1, pad 1, + bias.  `mutation` makes one of the mistakes a kernel can make:
    store_vec8 (a full 8-wide vector stored at the last column), rows_round64 (M rounded up to 64 rows stored), skip_one (one element left
    unwritten), k_round64 (K rounded up to 64 read from A), row_M (row M of A added into row M - 1), bias_lane (bias lane n_out added into
    column n_out - 1), halo_unchecked (conv: the halo row -1 of image 0 fetched without the bounds test)."""
    assert mutation is None or mutation in MUTATIONS
    s, v = prob.spec, prob.views
    M, N = s["M"], s["N"]
    bias_p, bias_o = v["bias"].parent.double(), v["bias"].offset
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
        Wm = Wv.parent.as_strided((N, 9, Cin), (Wv.ld, Cin, 1), Wv.offset).double()
        flat = a.parent.double()
        bb, oy, ox = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
        acc = torch.zeros(B, H, W, N, dtype=torch.float64)
        for tap in range(9):
            iy, ix = oy + tap // 3 - 1, ox + tap % 3 - 1
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            if mutation == "halo_unchecked":
                ok = ok | ((bb == 0) & (iy == -1))
            pix = (bb * H + iy) * W + ix                                           # (negative in front of image 0)
            idx = a.offset + pix[..., None] * a.ld + torch.arange(Cin)
            val = torch.where(ok[..., None], flat[idx.clamp(0, flat.numel() - 1)], torch.zeros((), dtype=torch.float64))
            acc += val @ Wm[:, tap].t()
        acc = acc.reshape(M, N)
    acc = acc + bias_p[bias_o:bias_o + N]
    if mutation == "bias_lane":
        acc[:, N - 1] += bias_p[bias_o + N]
    if "R" in v:
        r = v["R"]
        acc = acc + r.parent.as_strided((M, N), (r.ld, 1), r.offset).double()
    _, o, _, _, _ = prob.outs[0]
    dst = o.parent
    rows = M if mutation != "rows_round64" else (M + 63) // 64 * 64
    val = torch.zeros(rows, N, dtype=torch.float16)
    val[:M] = acc.half()
    dst.as_strided((rows, N), (o.ld, 1), o.offset).copy_(val)
    if mutation == "store_vec8":
        dst.as_strided((M, 8), (o.ld, 1), o.offset + N - 1).copy_(val[:M, N - 1:].expand(M, 8))
    if mutation == "skip_one":
        o.bits[o.offset + (M // 2) * o.ld + N // 3] = o.sentinel
