"""The row-chain launches (csrc/rowchain.hip, csrc/rowchain_midx.hip) one by one: a plain float64 reference per launch, NaN-fenced buffers
and designed inputs (tests/test_rowchain_stages_gpu.py, tests/test_rowchain_stages_cpu.py).  Nothing here needs a device.

References: `BlockRef` states every stage of a Transformer2D block from the STATE DICT (not from the packed fragment streams: a packer
mistake must show too), in float64, from the fp16-rounded inputs and weights a launch gets, with no rounding inside a stage:
  IN     GroupNorm (eps 1e-6, statistics of x per image) -> proj_in + bias = h0 -> LayerNorm1 -> q | k [M][2C], V^T [B][C][ldvt]
  MID    to_out + bias + res = h1 -> LayerNorm2 -> attn2.to_q
  MIDX   h1 as MID -> softmax(q K^T d^-0.5) V over T context tokens, 8 heads
  end    to_out + bias + res = h2 -> LayerNorm3 -> GEGLU feed-forward + h2 = h3 -> proj_out + bias + x (+ r2[b % bmod] where pixel
         (pix % out_w) >= r2_xmin) = out [-> (zero_w out + zero_b) * alpha * alpha_dev[idx * max(bstride, 1) + (bstride > 0 ? b : 0)]]
         (one reference for OUT, OUT_FF + OUT_TAIL and OUT_FFP + bc_rowchain_sum).
Fences: every input is a view inside a parent filled with NaN (guard rows in front and behind; rows have ld = C by contract, so there are
no column gaps; V^T has ldvt = rows_per_batch + 8 and NaN padding columns; the statistics totals are integers, their guard rows carry the
poison bc_gn_tot_read turns into NaN); every output is a view inside a parent prefilled with a NaN sentinel: an unwritten row block fails
the bar, a changed sentinel outside the view fails by name (gemm_views_common.Out.check).
Inputs: images differ in offset and scale, x_b = g (0.6 + 0.5 b) + (0.4 b - 0.3); res = 1.5 g + 0.3, a = 0.8 g, r2 = 0.7 g with another
draw per residual image.  Quiet rows (MID, MIDX, block end): every 37th row from row 5 has a = 0 and res = fp16(0.25 + 0.01 g - to_out
bias), so the row in front of the LayerNorm has a variance of about 1e-4 and ln_eps = 1e-5 counts.  The kernels normalise their fp32
accumulator, so they are held to the bar there (the unfused list rounds that row to fp16 first and is not)."""
import torch
import torch.nn.functional as F

from tests import attention_common as ac
from tests import gemm_views_common as gv
from tests.common import block_param_shapes, close, g

HEADS, GROUPS, GN_EPS, LN_EPS = 8, 32, 1e-6, 1e-5
GUARD = 64                              # guard rows in front of and behind every view: one row block
VT_PAD = 8                              # NaN padding columns of V^T
TOT_POISON = 1 << 50                    # slice 2 of a statistics total at or above 2^45 reads as NaN (csrc/bc_common.h bc_gn_tot_read)
QUIET_FIRST, QUIET_STEP = 5, 37
ALPHA_ROW = (0.0, 0.8, 1.0, 0.55)       # per-request zero-conv scales (alpha_bstride = B)


def block_sd(C, cross, zero=False, seed=77):
    """State dict of one Transformer2D block (+ BlobNet's zero-conv), as tests/test_rowchain_gpu.py makes it."""
    from blobctrl_amd import synth
    sd = synth.synth_state_dict(block_param_shapes("transformer", dict(C=C, ctx=768 if cross else None)), seed)
    if zero:
        sd["zero.weight"], sd["zero.bias"] = g(seed + 1, C, C, 1, 1) * 0.05, g(seed + 2, C) * 0.1
    return sd


def layernorm(h, gamma, beta, eps):
    mu, var = h.mean(-1, keepdim=True), h.var(-1, unbiased=False, keepdim=True)
    return (h - mu) / torch.sqrt(var + eps) * gamma + beta


def attention(q, k, v):
    """softmax(q k^T d^-0.5) v per image and head, float64: q [B][N][C], k / v [B][T][C]."""
    d = q.shape[-1] // HEADS
    return ac.reference(q, k, v, HEADS, d, d ** -0.5)


def add_residual(out, r2, B, out_w, r2_xmin, images):
    """out [B HW][C] + r2[images[b]] [HW][C] where pixel (pix % out_w) >= r2_xmin."""
    M, C = out.shape
    mask = (torch.arange(M // B) % out_w >= r2_xmin).double()[None, :, None]
    return (out.view(B, M // B, C) + r2[images] * mask).reshape(M, C)


class BlockRef:
    """The stages of one block in float64.  rounded: weight matrices as the fp16 values the packed trunk holds (vectors stay fp32)."""

    def __init__(self, sd, rounded=True):
        self.C = sd["proj_in.weight"].shape[0]
        self.cross = any(".attn2." in k for k in sd)
        self.sd, self.rounded = sd, rounded

    def m(self, k):
        w = self.sd[k].reshape(self.sd[k].shape[0], -1).float()
        return (w.half() if self.rounded else w).double()

    def v(self, k):
        return self.sd[k].float().double()

    def lin(self, x, name, bias=True):
        y = x @ self.m(name + ".weight").t()
        return y + self.v(name + ".bias") if bias else y

    def stage_in(self, x, B, gn=True, ln_eps=LN_EPS, stats_of=None, stats_x=None):
        """x [M][C] -> h0, q, k [M][C], vt [B][C][HW].  stats_of: image whose GroupNorm statistics image b takes (a named mistake);
        stats_x: the rows the statistics are taken from (default x: a launch gets them as totals, apart from the rows it reads)."""
        M, C = x.shape
        HW, bp = M // B, "transformer_blocks.0."
        xn = x
        if gn:
            xg, sg = x.view(B, HW, GROUPS, C // GROUPS), (x if stats_x is None else stats_x).view(B, HW, GROUPS, C // GROUPS)
            mean, var = sg.mean((1, 3), keepdim=True), sg.var((1, 3), unbiased=False, keepdim=True)
            if stats_of is not None:
                mean, var = mean[stats_of], var[stats_of]
            xn = ((xg - mean) / torch.sqrt(var + GN_EPS)).reshape(M, C) * self.v("norm.weight") + self.v("norm.bias")
        h0 = self.lin(xn, "proj_in")
        n = layernorm(h0, self.v(bp + "norm1.weight"), self.v(bp + "norm1.bias"), ln_eps)
        q, k, v = (self.lin(n, bp + f"attn1.{t}", bias=False) for t in ("to_q", "to_k", "to_v"))
        return dict(h0=h0, q=q, k=k, v=v, vt=v.view(B, HW, C).transpose(1, 2))

    def to_out(self, a, res, attn):
        return self.lin(a, f"transformer_blocks.0.{attn}.to_out.0") + res

    def stage_mid(self, a, res, ln_eps=LN_EPS):
        bp = "transformer_blocks.0."
        h1 = self.to_out(a, res, "attn1")
        n = layernorm(h1, self.v(bp + "norm2.weight"), self.v(bp + "norm2.bias"), ln_eps)
        return dict(h1=h1, q=self.lin(n, bp + "attn2.to_q", bias=False))

    def stage_midx(self, a, res, k, v, ln_eps=LN_EPS):
        """k, v [B][T][C]: the projected context of every image -> h1, attn [M][C]."""
        r = self.stage_mid(a, res, ln_eps)
        B = k.shape[0]
        r["attn"] = attention(r["q"].view(B, -1, self.C), k, v).reshape(-1, self.C)
        return r

    def stage_end(self, a, res, x, B, r2=None, out_w=1, r2_xmin=0, bmod=1, ln_eps=LN_EPS, zero=None, r2_image=None):
        """a, res, x [M][C]; r2 [bmod][HW][C]; zero = (alpha, per-image scales [B] or None) -> h2, h3, out [, zero].  r2_image: the residual
        image that image b takes (default b % bmod; anything else is a named mistake)."""
        M, C = a.shape
        HW, bp = M // B, "transformer_blocks.0."
        h2 = self.to_out(a, res, "attn2" if self.cross else "attn1")
        n = layernorm(h2, self.v(bp + "norm3.weight"), self.v(bp + "norm3.bias"), ln_eps)
        val, gate = self.lin(n, bp + "ff.net.0.proj").chunk(2, -1)
        h3 = self.lin(val * F.gelu(gate), bp + "ff.net.2") + h2
        plain = self.lin(h3, "proj_out") + x
        out = plain if r2 is None else add_residual(plain, r2, B, out_w, r2_xmin, [b % bmod for b in range(B)] if r2_image is None else r2_image)
        r = dict(h2=h2, h3=h3, plain=plain, out=out)
        if zero is not None:
            alpha, scales = zero
            r["zero_unit"] = self.lin(out, "zero")
            z = r["zero_unit"].view(B, HW, C) * alpha
            if scales is not None:
                z = z * scales.double()[:, None, None]
            r["zero"] = z.reshape(M, C)
        return r

    def block(self, x, B, ctx=None):
        """The whole block (float64 attention between the stages): x [M][C], ctx [B][T][768] -> out [M][C]."""
        bp, C = "transformer_blocks.0.", self.C
        s = self.stage_in(x, B)
        a = attention(s["q"].view(B, -1, C), s["k"].view(B, -1, C), s["v"].view(B, -1, C)).reshape(-1, C)
        h = s["h0"]
        if self.cross:
            kc, vc = self.lin(ctx.double(), bp + "attn2.to_k", bias=False), self.lin(ctx.double(), bp + "attn2.to_v", bias=False)
            m = self.stage_midx(a, h, kc, vc)
            a, h = m["attn"], m["h1"]
        return self.stage_end(a, h, x, B)["out"]


# ---------------------------------------------------------------------------------------------------- designed inputs
def image_rows(seed, B, HW, C):
    """x_b = g (0.6 + 0.5 b) + (0.4 b - 0.3): every image has its own offset and scale -> fp16 [B HW][C]."""
    b = torch.arange(B, dtype=torch.float32)[:, None, None]
    return (g(seed, B, HW, C) * (0.6 + 0.5 * b) + (0.4 * b - 0.3)).reshape(B * HW, C).half()


def quiet_rows(M):
    return torch.arange(QUIET_FIRST, M, QUIET_STEP)


def attn_and_res(seed, M, C, to_out_bias, quiet=True):
    """(a = 0.8 g, res = 1.5 g + 0.3) fp16 [M][C]; on the quiet rows a = 0 and res = 0.25 + 0.01 g - to_out bias."""
    a, res = 0.8 * g(seed, M, C), 1.5 * g(seed + 1, M, C) + 0.3
    if quiet:
        rows = quiet_rows(M)
        a[rows] = 0.0
        res[rows] = 0.25 + 0.01 * g(seed + 2, len(rows), C) - to_out_bias.float()
    return a.half(), res.half()


def context_kv(seed, B, T, C, v_scale=1.0):
    """K rows and V rows of the projected context, fp16 [B][T][C]: unit Gaussians.  One key of 80 carries about 1 / 80 x (the largest of d
    deviates) = 0.03 of an output element, ten attention bars (3e-3 + 2e-3 |ref|); tests/test_rowchain_stages_cpu.py measures what a wrong
    key set moves.  A larger V buys more of that and leaves the kernel no room: with V = 4 g the float64 reference lies 0.39 to 0.73 bars
    from a float64 attention that only rounds q, the probabilities and the output to fp16 (0.17 to 0.23 bars at V = g), before any
    accumulation error - the absolute part of the bar does not grow with V."""
    return g(seed, B, T, C).half(), (v_scale * g(seed + 1, B, T, C)).half()


# ---------------------------------------------------------------------------------------------------- fenced buffers
class FencedOut(gv.Out):
    """rows x width output behind GUARD sentinel rows, row stride ld, GUARD sentinel rows behind (checks: gemm_views_common.Out.check)."""

    def __init__(self, rows, width, ld, device, f32=False):
        assert ld >= width
        self.rows, self.width, self.ld, self.f32 = rows, width, ld, f32
        self.offset, self.back = GUARD * ld, GUARD
        self.bits = gv._filled((rows + 2 * GUARD) * ld, device, f32)
        self.sentinel = gv.SENTINEL32 if f32 else gv.SENTINEL

    def assert_inside(self):
        assert self.offset >= GUARD * self.ld and gv._elems_behind(self.t) >= (self.rows + self.back) * self.ld
        assert (self.parent.data_ptr() + self.offset * self.parent.element_size()) % 16 == 0 and (self.ld * self.parent.element_size()) % 16 == 0


def fenced_vec(vec, device):
    """The fp32 vector stream of a launch (biases, LayerNorm affine) with as many NaN lanes in front of it and behind it."""
    return fenced_in(vec.detach().float().cpu()[None], device, f32=True, guard=1)


def fenced_in(x, device, ld=None, f32=False, guard=GUARD, align=16):
    """x [rows][cols] inside a NaN parent: `guard` NaN rows in front and behind, NaN columns from cols to ld."""
    v = gv.View(x, device, ld=x.shape[-1] if ld is None else ld, front=guard, back=guard, f32=f32)
    assert (v.parent.data_ptr() + v.offset * v.parent.element_size()) % align == 0
    return v


class FencedTotals:
    """GroupNorm statistics totals [B][C][6] int64 of x (launch.encode_gn_tot, one slot per channel) between guard images whose every
    total is poisoned: read, they make the statistics NaN."""

    def __init__(self, sums, device):
        from blobctrl_amd.launch import encode_gn_tot
        B, C, _ = sums.shape
        self.parent = torch.zeros(B + 2, C, 6, dtype=torch.int64, device=device)
        self.parent[..., 2] = TOT_POISON
        self.parent[..., 5] = TOT_POISON
        self.parent[1:B + 1] = encode_gn_tot(sums).to(device)
        self.t = self.parent[1:B + 1]


def alpha_table(form, B, device):
    """(alpha, alpha_dev view or None, alpha_idx value or None, bstride, the scale of every image [B] or None).  Every entry of alpha_dev
    but the ones that should be read is NaN, and so are the guard entries around the table."""
    if form == "alpha":
        return 0.7, None, None, 0, None
    if form == "dev":                   # alpha_dev[3], alpha_idx = 2, bstride 0
        t = torch.full((3,), float("nan"))
        t[2] = 0.8
        return 0.9, fenced_in(t[None], device, f32=True, guard=1, align=4), 2, 0, torch.full((B,), 0.8)
    assert form == "dev_b", form        # alpha_dev[3][B], alpha_idx = 1, bstride B: the last B entries of ALPHA_ROW (B = 4: all of them)
    row = torch.tensor(ALPHA_ROW[-B:])
    t = torch.full((3, B), float("nan"))
    t[1] = row
    return 0.9, fenced_in(t.reshape(1, -1), device, f32=True, guard=1, align=4), 1, B, row


ALPHA_FORMS = ("alpha", "dev", "dev_b")


# ---------------------------------------------------------------------------------------------------- one launch (or launch pair) as a problem
class Stage:
    """Inputs (fenced views), outputs [(label, FencedOut, ref [rows][width] float64, bar)] and what the launch needs.  bar: "row" = the
    default bar of tests.common.close (2e-3 |ref| + 2e-3 max(1, scale)), "attn" = attention_common's (3e-3 + 2e-3 |ref|), None = fences
    and finiteness only (the partial-sum buffers between two launches)."""

    def __init__(self, name, views, outs, **args):
        self.name, self.views, self.outs, self.args = name, views, outs, args
        self.vals, self.errs = {}, {}

    def assert_inside(self):
        for v in self.views.values():
            if isinstance(v, gv.View):
                v.assert_inside()
        for _, o, _, _ in self.outs:
            o.assert_inside()

    def out(self, label):
        return next(o for l, o, _, _ in self.outs if l == label)

    def verify(self):
        """(max error over bar, sentinel elements checked); prints every figure before it asserts."""
        worst, checked = 0.0, 0
        for label, o, ref, bar in self.outs:
            what = f"{self.name} [{label}]"
            vals, n = o.check(what)
            checked += n
            self.vals[label] = vals
            if bar is None:
                continue
            e = ac.worst(vals, ref)[0] if bar == "attn" else gv.err_over_bar(vals, ref, 2e-3, None)
            print(f"{what}: max err/bar {e:.3f}, {n} sentinel elements checked")
            self.errs[label] = e
            worst = max(worst, e)
        for label, o, ref, bar in self.outs:
            if bar == "attn":
                assert self.errs[label] <= 1.0, f"{self.name} [{label}]: worst err/bar {self.errs[label]:.2f} (attention bar)"
            elif bar is not None:
                close(self.vals[label], ref, what=f"{self.name} [{label}]")
        return worst, checked


def gn_sums(x, B):
    """(sum, sum of squares) [B][C][2] float64 of x [B HW][C] per image and channel."""
    xb = x.double().view(B, -1, x.shape[-1])
    return torch.stack([xb.sum(1), (xb * xb).sum(1)], -1)


IN_FORMS = ("totals", "affine", "none")


def in_problem(ref, device, B, HW, form, ln_eps=LN_EPS, seed=11):
    """IN: x -> h0, q | k, V^T (ldvt = HW + 8).  form: totals (the finalize runs in the kernel, from fenced statistics totals), affine (a
    host-computed table [B][C][2]), none (x straight into proj_in)."""
    C, M = ref.C, B * HW
    x = image_rows(seed, B, HW, C)
    views = dict(x=fenced_in(x, device))
    xd = x.double()
    if form == "totals":
        views["gn_tot"] = FencedTotals(gn_sums(x, B), device)
    elif form == "affine":
        xg = xd.view(B, HW, GROUPS, C // GROUPS)
        mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
        rstd = (1.0 / torch.sqrt(var + GN_EPS)).repeat_interleave(C // GROUPS, 1)
        mean = mean.repeat_interleave(C // GROUPS, 1)
        a_ = rstd * ref.v("norm.weight")
        views["affine"] = fenced_in(torch.stack([a_, ref.v("norm.bias") - mean * a_], -1).reshape(B, 2 * C).float(), device, f32=True, guard=1)
    else:
        assert form == "none", form
    r = ref.stage_in(xd, B, gn=form != "none", ln_eps=ln_eps)
    ldvt = HW + VT_PAD
    outs = [("h0", FencedOut(M, C, C, device), r["h0"], "row"),
            ("q|k", FencedOut(M, 2 * C, 2 * C, device), torch.cat([r["q"], r["k"]], 1), "row"),
            ("V^T", FencedOut(B * C, HW, ldvt, device), r["vt"].reshape(B * C, HW), "row")]
    return Stage(f"IN C={C} B={B} HW={HW} {form}", views, outs, C=C, M=M, HW=HW, B=B, ldvt=ldvt, form=form, ln_eps=ln_eps)


def mid_problem(ref, device, B, HW, ln_eps=LN_EPS, seed=21):
    C, M = ref.C, B * HW
    a, res = attn_and_res(seed, M, C, ref.v("transformer_blocks.0.attn1.to_out.0.bias"))
    r = ref.stage_mid(a.double(), res.double(), ln_eps)
    views = dict(x=fenced_in(a, device), res=fenced_in(res, device))
    outs = [("h1", FencedOut(M, C, C, device), r["h1"], "row"), ("q", FencedOut(M, C, C, device), r["q"], "row")]
    return Stage(f"MID C={C} B={B} HW={HW} ln_eps={ln_eps:g}", views, outs, C=C, M=M, HW=HW, B=B, ln_eps=ln_eps)


def midx_inputs(ref, B, HW, T, seed=31, v_scale=1.0):
    C = ref.C
    a, res = attn_and_res(seed, B * HW, C, ref.v("transformer_blocks.0.attn1.to_out.0.bias"))
    k, v = context_kv(seed + 5, B, T, C, v_scale)
    return a, res, k, v


def midx_problem(ref, device, B, HW, T, ln_eps=LN_EPS, seed=31, v_scale=1.0):
    """MIDX: K rows [B T][C] (key T of image b is key 0 of image b + 1, the last image's key T is the fence), V^T [B][C][ldvt] with NaN from
    column T on."""
    C, M = ref.C, B * HW
    a, res, k, v = midx_inputs(ref, B, HW, T, seed, v_scale)
    r = ref.stage_midx(a.double(), res.double(), k, v, ln_eps)
    ldvt = (T + 7) // 8 * 8 + VT_PAD
    views = dict(x=fenced_in(a, device), res=fenced_in(res, device), k=fenced_in(k.reshape(B * T, C), device),
                 vt=fenced_in(v.transpose(1, 2).reshape(B * C, T), device, ld=ldvt))
    outs = [("h1", FencedOut(M, C, C, device), r["h1"], "row"), ("attn", FencedOut(M, C, C, device), r["attn"], "attn")]
    return Stage(f"MIDX C={C} B={B} HW={HW} T={T}", views, outs, C=C, M=M, HW=HW, B=B, T=T, ldvt_ctx=ldvt, ln_eps=ln_eps)


# (out_w, r2_xmin, rows per image, B, bmod): block 0 skips the residual, block 1 straddles, block 2 is all right-hand | the skip exactly at
# the boundary | every block wraps lines | the square canvas
R2_CASES = {"w192": (192, 100, 384, 4, 2), "w128": (128, 64, 128, 2, 2), "w24": (24, 16, 192, 2, 1), "w8": (8, 0, 64, 3, 3)}
END_FORMS = (("out", 1), ("ff_tail", 2), ("ff_tail", 5), ("ffp_sum", 2), ("ffp_sum", 5))
END_FORMS_640 = (("ff_tail", 4), ("ffp_sum", 4))


def end_inputs(ref, B, HW, bmod=0, seed=41):
    C, M = ref.C, B * HW
    att = "attn2" if ref.cross else "attn1"
    a, res = attn_and_res(seed, M, C, ref.v(f"transformer_blocks.0.{att}.to_out.0.bias"))
    x = image_rows(seed + 5, B, HW, C)
    r2 = torch.stack([0.7 * g(seed + 10 + i, HW, C) for i in range(bmod)]).half() if bmod else None
    return a, res, x, r2


def end_reference(ref, B, HW, r2case=None, zero_form=None, ln_eps=LN_EPS, seed=41):
    """(inputs, float64 outputs, the residual's arguments, the zero-conv's table) of a block end - device-free, so that a test module
    computes it once per case and shares it among the launch forms."""
    out_w, xmin, _, _, bmod = R2_CASES[r2case] if r2case else (1, 0, HW, B, 0)
    a, res, x, r2 = end_inputs(ref, B, HW, bmod, seed)
    zero = None
    if zero_form:
        alpha, _, _, _, scales = alpha_table(zero_form, B, torch.device("cpu"))
        zero = (alpha, scales)
    r = ref.stage_end(a.double(), res.double(), x.double(), B, r2=None if r2 is None else r2.double(), out_w=out_w, r2_xmin=xmin,
                      bmod=max(bmod, 1), ln_eps=ln_eps, zero=zero)
    return dict(a=a, res=res, x=x, r2=r2, r=r, out_w=out_w, xmin=xmin, bmod=bmod)


def end_problem(ref, device, B, HW, form, nsplit, pre, r2case=None, zero_form=None, ln_eps=LN_EPS):
    """The block end as OUT (form "out"), OUT_FF + OUT_TAIL ("ff_tail") or OUT_FFP + bc_rowchain_sum ("ffp_sum") over nsplit workgroups
    per row block; pre = end_reference(...) of the same case."""
    C, M = ref.C, B * HW
    views = dict(x=fenced_in(pre["a"], device), res=fenced_in(pre["res"], device), res2=fenced_in(pre["x"], device))
    if pre["r2"] is not None:
        views["r2"] = fenced_in(pre["r2"].reshape(-1, C), device)
    outs = [("out", FencedOut(M, C, C, device), pre["r"]["out"], "row")]
    args = dict(C=C, M=M, HW=HW, B=B, form=form, nsplit=nsplit, out_w=pre["out_w"], r2_xmin=pre["xmin"], r2_bmod=pre["bmod"], ln_eps=ln_eps, zero=None)
    if zero_form:
        alpha, dev, idx, bstride, _ = alpha_table(zero_form, B, device)
        if dev is not None:
            views["alpha_dev"] = dev
        args["zero"] = (alpha, idx, bstride)
        outs.append(("zero", FencedOut(M, C, C, device), pre["r"]["zero"], "row"))
    if form == "ff_tail":
        outs.append(("part fp32", FencedOut(nsplit * M, C, C, device, f32=True), None, None))
    elif form == "ffp_sum":
        outs.append(("part fp16", FencedOut((2 if zero_form else 1) * nsplit * M, C, C, device), None, None))
    net = f"blobnet {zero_form}" if zero_form else f"unet r2={r2case or 'none'}"
    return Stage(f"END C={C} B={B} HW={HW} {form}/{nsplit} {net}", views, outs, **args)


# ---------------------------------------------------------------------------------------------------- a torch statement of the IN launch
MUTATIONS = ("store_past", "skip_block", "read_behind", "vt_pad")


def emulate_in(ref, prob, mutation=None):
    """What the IN launch does, in torch: reads the rows of its x view, computes in float64, stores fp16 into its three output views.
    `mutation`: store_past (h0 stored one row block past the view), skip_block (row block 1 of q | k left unwritten), read_behind (the row
    behind x added into the last row), vt_pad (V^T stored 8 columns too wide)."""
    assert mutation is None or mutation in MUTATIONS
    a = prob.args
    C, M, B, HW = a["C"], a["M"], a["B"], a["HW"]
    xv = prob.views["x"]
    x = xv.parent.as_strided((M + 1, C), (xv.ld, 1), xv.offset).double()
    rows = x[:M].clone()
    if mutation == "read_behind":
        rows[M - 1] += x[M]
    r = ref.stage_in(rows, B, gn=a["form"] != "none", ln_eps=a["ln_eps"], stats_x=x[:M])
    h0, qk, vt = (prob.out(l) for l in ("h0", "q|k", "V^T"))
    n = M + 64 if mutation == "store_past" else M
    val = torch.zeros(n, C, dtype=torch.float16)
    val[:M] = r["h0"].half()
    h0.parent.as_strided((n, C), (h0.ld, 1), h0.offset).copy_(val)
    qk.parent.as_strided((M, 2 * C), (qk.ld, 1), qk.offset).copy_(torch.cat([r["q"], r["k"]], 1).half())
    if mutation == "skip_block":
        qk.bits[qk.offset + 64 * qk.ld: qk.offset + 128 * qk.ld] = qk.sentinel
    w = HW + 8 if mutation == "vt_pad" else HW
    v = torch.zeros(B * C, w, dtype=torch.float16)
    v[:, :HW] = r["vt"].reshape(B * C, HW).half()
    vt.parent.as_strided((B * C, w), (vt.ld, 1), vt.offset).copy_(v)
