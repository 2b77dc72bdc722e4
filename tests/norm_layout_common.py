"""The bandwidth launches one by one (csrc/norm.hip, the encoder-side half of csrc/elementwise.hip, the three row ops of csrc/sam_ops.hip):
a float64 reference per launch, NaN-fenced inputs, sentinel-fenced outputs and derived bars (tests/test_norm_layout_gpu.py runs the
problems through the library, tests/test_norm_layout_cpu.py shows on the CPU what the harness sees).  Nothing here needs a device.

Inputs come from tests.common.g, rounded to the type the launch reads; the reference is float64 arithmetic on those rounded values.  Every
fp16 / fp32 input is a view inside a NaN parent (gemm_views_common.View through rowchain_stages_common.fenced_in / fenced_vec): guard rows
in front and behind, NaN pad columns where the ABI has a leading dimension.  Every output is a view inside a sentinel parent
(rowchain_stages_common.FencedOut; FlatOut below for the flat launches, whose guards are counted in elements); an in-place launch gets ONE
buffer, its NaN-fenced input, whose bits outside the view must be what they were (InPlace).

Bars.  ulp16(r): the fp16 spacing at |r|, floored at 2^-24; E20 = 2^-20 stands for a few fp32 roundings.
  exact          bit-equal to the float64 result rounded once to the output type (zeros compared by value)
  fp16 + fp32    ulp16(ref): the fp32 sum rounds before the fp16 store
  LayerNorm      ulp16(ref) + E20 (max|x_row| rstd |gamma| + |beta|)
  GroupNorm      t = a x + b, a = rstd gamma, b = beta - mean a: ulp16(ref) + E20 (|a x| + |b|); with SiLU behind it the affine's error
                 passes through silu' (|silu'| <= 1.1) and SiLU adds its own: ulp16(ref) + 1.1 E20 (|a x| + |b|) + E20 (1 + |t|) |ref|
  softmax        ulp16(ref) + E20 (1 + (rowmax - x)) ref   (the fast exponential's argument error grows with |x - max|)
  silu           ulp16(ref) + E20 (1 + |x|) |ref|
  GELU           ulp16(ref) + 5e-7   (csrc/bc_common.h: bc_gelu_f is within 4.2e-7 of the erf form)
  sample         fp32 out: E20 scale (|mean| + (1 + |logvar_clamped / 2|) |sigma noise|)
  gn_stats       sum within 2^-18 sum|x|, sum of squares within 2^-18 sum x^2 (fp32 partials of at most 32 pixels per wave, exact integer adds)
tests.common.close with the project's defaults stays the ceiling of every comparison."""
import numpy as np
import torch

from tests import gemm_views_common as gv
from tests import rowchain_stages_common as rc
from tests.common import close, g

E20 = 2.0 ** -20
CAP = 2048 * 256                        # threads of a capped grid: ew_blocks (csrc/elementwise.hip), bc_memset_zero
DUP_CAP = 1024 * 256                    # ... of bc_dup_halves
SCALE = float(np.float32(0.18215))      # the latent scaling factor as the fp32 the launch gets
GN_RANGE = 64                           # channels per workgroup of the fused GroupNorm
GN_SLAB = 128                           # pixels per workgroup of bc_gn_stats


def ulp16(r):
    r = r.abs().double()
    e = torch.frexp(r)[1].double() - 11.0
    e = torch.where(r == 0, torch.full_like(e, -24.0), e)
    return torch.exp2(e.clamp(min=-24.0))


def round_once(ref, dtype):
    """float64 -> the output type in ONE rounding (torch goes through fp32 on the way to fp16)."""
    if dtype == torch.float16:
        return torch.from_numpy(ref.numpy().astype(np.float16)).double()
    return ref.to(dtype).double()


def buckets(seed, k, *shape):
    """Integers 0 .. k - 1 drawn from g(seed)."""
    return (g(seed, *shape).abs() * 1000.0).long() % k


# ---------------------------------------------------------------------------------------------------- fenced buffers
class FlatOut(rc.FencedOut):
    """rows x width contiguous output elements between `guard` sentinel ELEMENTS (a flat launch has no row to round up to: a guard of 64
    rows of 180000 elements would only cost time)."""

    def __init__(self, rows, width, device, f32=False, guard=4096):
        self.rows, self.width, self.ld, self.f32 = rows, width, width, f32
        self.offset, self.guard, self.back = guard, guard, 0
        self.bits = gv._filled(rows * width + 2 * guard, device, f32)
        self.sentinel = gv.SENTINEL32 if f32 else gv.SENTINEL

    def assert_inside(self):
        assert self.offset >= 8 and gv._elems_behind(self.t) >= self.rows * self.width + self.guard
        assert (self.parent.data_ptr() + self.offset * self.parent.element_size()) % 16 == 0


class InPlace:
    """The NaN-fenced input of an in-place launch as its output: one buffer, both view and fence.  snapshot() before the launch; check()
    fails when a bit outside the view changed or an element of the view is not finite.  (A store that puts a fence's own NaN bits back
    where they were cannot be seen in place; the out-of-place launches have a sentinel of another payload for that.)"""

    def __init__(self, view):
        self.v, self.before, self.f32 = view, None, view.dtype == torch.float32
        self.rows, self.width, self.ld, self.offset = view.rows, view.cols, view.ld, view.offset

    @property
    def parent(self):
        return self.v.parent

    @property
    def t(self):
        return self.v.t

    def _bits(self):
        return self.v.parent.view(torch.int32 if self.f32 else torch.int16).cpu().clone()

    def snapshot(self):
        self.before = self._bits()

    def assert_inside(self):
        inside(self.v)

    def check(self, what):
        assert self.before is not None, "snapshot() comes before the launch"
        now = self._bits()
        idx = self.offset + torch.arange(self.rows)[:, None] * self.ld + torch.arange(self.width)[None, :]
        view = torch.zeros(now.numel(), dtype=torch.bool)
        view[idx.flatten()] = True
        stray = (now != self.before) & ~view
        if bool(stray.any()):
            r, c = divmod(int(stray.nonzero()[0, 0]) - self.offset, self.ld)
            raise AssertionError(f"{what}: {int(stray.sum())} elements outside the view were written, first at (row {r}, col {c})")
        vals = self.v.parent.cpu()[idx].double()
        leak = ~torch.isfinite(vals)
        if bool(leak.any()):
            r, c = (int(v) for v in leak.nonzero()[0])
            raise AssertionError(f"{what}: {int(leak.sum())} non-finite elements in the view (a leak), first at (row {r}, col {c})")
        return vals, int((~view).sum())

    def untouched(self):
        return bool((self._bits() == self.before).all())


GUARD_WORD = 0x0123456789ABCDE          # what the guard images of a statistics table hold: non-zero (read as totals: poison)


class StatsOut:
    """A statistics table [B][C][GN_TOT_WORDS] that ALREADY holds encoded totals, between two guard images of a non-zero pattern.
    check(): the guard images are bit-identical, the table decodes to finite (sum, sum of squares) [B C][2]."""

    def __init__(self, old_sums, device):
        from blobctrl_amd.launch import encode_gn_tot
        B, C, _ = old_sums.shape
        self.B, self.C, self.f32 = B, C, False
        self.parent = torch.full((B + 2, C, 6), GUARD_WORD, dtype=torch.int64, device=device)
        self.parent[0] += torch.arange(C * 6, device=device).view(C, 6)
        self.parent[1:B + 1] = encode_gn_tot(old_sums).to(device)
        self.t = self.parent[1:B + 1]
        self.before = self.parent.cpu().clone()

    def assert_inside(self):
        assert self.t.data_ptr() % 16 == 0 and self.parent.shape[0] == self.B + 2

    def check(self, what):
        from blobctrl_amd.launch import decode_gn_tot
        now = self.parent.cpu()
        stray = torch.ones(self.B + 2, dtype=torch.bool)
        stray[1:self.B + 1] = False
        changed = (now != self.before)[stray]
        if bool(changed.any()):
            raise AssertionError(f"{what}: {int(changed.sum())} elements outside the view were written (the guard images of the table)")
        vals = decode_gn_tot(now[1:self.B + 1]).reshape(self.B * self.C, 2)
        if not bool(torch.isfinite(vals).all()):
            raise AssertionError(f"{what}: {int((~torch.isfinite(vals)).sum())} non-finite elements in the view (a leak), poisoned totals")
        return vals, int(changed.numel())

    def untouched(self):
        return bool((self.parent.cpu() == self.before).all())


def inside(v):
    """gemm_views_common.View.assert_inside without its 16-byte rule (a scalar launch takes any element; fence() asserts what a launch needs):
    what the launch may address and a plausible overrun of it - the guard rows, one 8-wide vector - lie inside the parent's storage."""
    assert v.front >= 1 and v.back >= 1 and v.offset == v.front * v.ld
    assert gv._elems_behind(v.t) >= (v.rows + v.back - 1) * v.ld + v.cols + gv.PAD


def fence(x, device, ld=None, f32=False, guard=rc.GUARD):
    """x [rows][cols] inside a NaN parent (rowchain_stages_common.fenced_in); the alignment asked of the view is what its launch needs:
    16 bytes where it loads vectors (cols % 8 == 0), the element otherwise."""
    ld_ = x.shape[-1] if ld is None else ld
    vec = (ld_ * (4 if f32 else 2)) % 16 == 0
    return rc.fenced_in(x, device, ld=ld, f32=f32, guard=guard, align=16 if vec else (4 if f32 else 2))


# ---------------------------------------------------------------------------------------------------- one launch as a problem
class Prob:
    """name, op (the launch), args, views (inputs), outs [(label, buffer, ref [rows][width] float64, bar: tensor like ref, or None = exact)],
    f32 {label: an fp32 restatement of the launch, as stored}."""

    def __init__(self, name, op, args, views, outs, f32=None):
        self.name, self.op, self.args, self.views, self.outs = name, op, args, views, outs
        self.f32 = f32 or {}

    def assert_inside(self):
        for v in self.views.values():
            if isinstance(v, gv.View):
                inside(v)
        for _, o, _, _ in self.outs:
            o.assert_inside()

    def prepare(self):
        for _, o, _, _ in self.outs:
            if isinstance(o, InPlace):
                o.snapshot()

    def out(self, label):
        return next(o for l, o, _, _ in self.outs if l == label)

    def untouched(self):
        return all(o.untouched() for _, o, _, _ in self.outs)

    def verify(self):
        """After the launch: (max error over bar, fence elements checked); prints each figure before it asserts."""
        worst, checked = 0.0, 0
        for label, o, ref, bar in self.outs:
            what = f"{self.name} [{label}]"
            vals, n = o.check(what)
            e, nbad = over_bar(vals, ref, bar, torch.float32 if o.f32 else torch.float16)
            print(f"{what}: max err/bar {e:.3f}, {n} sentinel elements checked")
            assert e <= 1.0, f"{what}: {nbad}/{ref.numel()} elements off the bar, max err/bar {e:.4g}" + (" (exact)" if bar is None else "")
            close(vals, ref, what=what)
            worst, checked = max(worst, e), checked + n
        return worst, checked


def over_bar(vals, ref, bar, dtype):
    """(max |vals - ref| / bar, elements over the bar); bar None: 0 where vals equals ref rounded once to `dtype`, else inf."""
    if bar is None:
        bad = vals != round_once(ref, dtype)
        return (float("inf") if bool(bad.any()) else 0.0), int(bad.sum())
    r = (vals - ref).abs() / bar
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max()), int((r > 1.0).sum())


# ---------------------------------------------------------------------------------------------------- LayerNorm
LN_WIDTHS = (8, 504, 512, 520, 1024, 1032, 1280, 2048)
LN_FAMILIES = ("3g+1", "mean100", "eps_visible", "unit")
LN_LAYOUTS = ("packed", "padded", "pooled")


def ln_passes(C):
    return 1 if C <= 512 else 2 if C <= 1024 else 4


def ln_input(family, seed, rows, C):
    """(x fp32 [rows][C], eps)."""
    if family == "3g+1":
        return 3.0 * g(seed, rows, C) + 1.0, 1e-5
    if family == "mean100":
        return 100.0 + 0.25 * g(seed, rows, C), 1e-5
    if family == "eps_visible":                       # variance about 1.2e-6: eps = 1e-5 is nine tenths of what the root sees
        return 1.0 + buckets(seed, 4, rows, C).float() * 2.0 ** -10, 1e-5
    assert family == "unit", family
    return g(seed, rows, C), 1e-6


def layernorm_problem(device, C, rows, layout, family, seed=101):
    """packed: ldx = ldy = C; padded: (C + 8, C + 16); pooled: DINOv2's final LayerNorm, row 0 of each of `rows` images of three rows
    (ldx = 3 C, ldy = C; the other two rows of every image are NaN)."""
    ldx, ldy = {"packed": (C, C), "padded": (C + 8, C + 16), "pooled": (3 * C, C)}[layout]
    x, eps = ln_input(family, seed, rows, C)
    xh = x.half()
    gamma, beta = 1.0 + 0.2 * g(seed + 1, C), 0.3 * g(seed + 2, C)
    views = dict(x=fence(xh, device, ld=ldx), gamma=rc.fenced_vec(gamma, device), beta=rc.fenced_vec(beta, device))
    xd, gd, bd = xh.double(), gamma.double(), beta.double()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ref = (xd - mu) * rstd * gd + bd
    bar = ulp16(ref) + E20 * (xd.abs().max(1, keepdim=True).values * rstd * gd.abs() + bd.abs())
    xf = xh.float()
    mf = xf.mean(1, keepdim=True)
    vf = ((xf - mf) ** 2).mean(1, keepdim=True)
    f32 = ((xf - mf) * torch.rsqrt(vf + eps) * gamma + beta).half().double()
    outs = [("y", rc.FencedOut(rows, C, ldy, device), ref, bar)]
    return Prob(f"layernorm C={C} rows={rows} {layout} {family}", "layernorm", dict(rows=rows, C=C, ldx=ldx, ldy=ldy, eps=eps), views, outs,
                dict(y=f32))


def layernorm_cases():
    """Every width with every family, rows 1 / 5 / 37 in turn (none a multiple of the four rows of a workgroup); every layout at 8, 520,
    1032 and 2048."""
    cases = []
    for i, C in enumerate(LN_WIDTHS):
        for j, fam in enumerate(LN_FAMILIES):
            cases.append(dict(C=C, rows=(1, 5, 37)[(i + j) % 3], layout="packed", family=fam))
    for i, C in enumerate((8, 520, 1032, 2048)):
        cases.append(dict(C=C, rows=37, layout="padded", family=LN_FAMILIES[i]))
        cases.append(dict(C=C, rows=5, layout="pooled", family=LN_FAMILIES[(i + 1) % 4]))
    return cases


# ---------------------------------------------------------------------------------------------------- softmax
SM_COLS = (8, 504, 512, 520, 2048, 2056, 4096, 4104, 9208, 9216)
SM_FAMILIES = ("3g", "huge", "last11", "masked")


def softmax_problem(device, cols, rows, pad, family, seed=201, ld=None):
    """In place, ld = cols + pad.  3g | 60000 - 2000 |g| (overflows without the max subtraction) | 0.5 g with the last column 11 (the
    normaliser must see the last register pass) | 3g with every seventh entry -inf (exactly 0 in the reference)."""
    gx = g(seed, rows, cols)
    if family == "3g":
        x = 3.0 * gx
    elif family == "huge":
        x = 60000.0 - 2000.0 * gx.abs()
    elif family == "last11":
        x = 0.5 * gx
        x[:, -1] = 11.0
    else:
        assert family == "masked", family
        x = 3.0 * gx
        x.view(-1)[::7] = float("-inf")
    xh = x.half()
    ld = cols + pad if ld is None else ld
    view = fence(xh, device, ld=max(ld, cols))
    xd = xh.double()
    ref = torch.softmax(xd, 1)
    d = xd.max(1, keepdim=True).values - xd
    d = torch.where(torch.isinf(d), torch.zeros_like(d), d)
    bar = ulp16(ref) + E20 * (1.0 + d) * ref
    xf = xh.float()
    e = torch.exp(xf - xf.max(1, keepdim=True).values)
    f32 = (e / e.sum(1, keepdim=True)).half().double()
    return Prob(f"softmax cols={cols} rows={rows} ld={ld} {family}", "softmax", dict(rows=rows, cols=cols, ld=ld), dict(x=view),
                [("p", InPlace(view), ref, bar)], dict(p=f32))


def softmax_cases(cols):
    return [dict(cols=cols, rows=rows, pad=pad, family=fam) for rows in (1, 9) for pad in (0, 8) for fam in SM_FAMILIES]


# ---------------------------------------------------------------------------------------------------- GroupNorm
GN_SHAPES = ((16, 0, 4, 1), (24, 40, 4, 37), (64, 0, 64, 33), (1280, 640, 32, 129), (2560, 0, 32, 40), (3072, 0, 32, 8), (208, 0, 2, 70))
GN_B = 2


def groupnorm_problem(device, shape, silu, stats, eps=None, family="2g+0.5", seed=301):
    """(C1, C2, G, HW) at B = 2 over the concat (x1 | x2).  stats: "recorded" (a bc_gn_stats pass in front) or "encoded" (totals encoded from
    float64 sums, between poisoned guard images: rowchain_stages_common.FencedTotals)."""
    C1, C2, G, HW = shape
    B, C = GN_B, C1 + C2
    eps = (1e-5 if stats == "recorded" else 1e-6) if eps is None else eps
    x = (2.0 * g(seed, B * HW, C) + 0.5) if family == "2g+0.5" else (30.0 + 0.5 * g(seed, B * HW, C))
    xh = x.half()
    gamma, beta = 1.0 + 0.2 * g(seed + 1, C), 0.3 * g(seed + 2, C)
    views = dict(x1=fence(xh[:, :C1], device), gamma=rc.fenced_vec(gamma, device), beta=rc.fenced_vec(beta, device))
    if C2:
        views["x2"] = fence(xh[:, C1:], device)
    if stats == "encoded":
        views["tot1"] = rc.FencedTotals(rc.gn_sums(xh[:, :C1], B), device)
        if C2:
            views["tot2"] = rc.FencedTotals(rc.gn_sums(xh[:, C1:], B), device)
    xd = xh.double().view(B, HW, G, C // G)
    mean, var = xd.mean((1, 3), keepdim=True), xd.var((1, 3), unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    a = (rstd.expand(B, 1, G, C // G).reshape(B, 1, C) * gamma.double())
    b = beta.double() - mean.expand(B, 1, G, C // G).reshape(B, 1, C) * a
    xd = xd.reshape(B, HW, C)
    t = a * xd + b
    aff = (a * xd).abs() + b.abs()
    tf = xd.float() * a.float() + b.float()
    if silu:
        ref = t * torch.sigmoid(t)
        bar = ulp16(ref) + 1.1 * E20 * aff + E20 * (1.0 + t.abs()) * ref.abs()
        f32 = tf / (1.0 + torch.exp(-tf))
    else:
        ref, bar, f32 = t, ulp16(t) + E20 * aff, tf
    M = B * HW
    outs = [("y", rc.FencedOut(M, C, C, device), ref.reshape(M, C), bar.reshape(M, C))]
    return Prob(f"groupnorm {shape} silu={int(silu)} {stats} eps={eps:g} {family}", "groupnorm",
                dict(C1=C1, C2=C2, G=G, HW=HW, B=B, eps=eps, silu=silu, stats=stats), views, outs, dict(y=f32.half().double().reshape(M, C)))


def groupnorm_cases(shape):
    cases = [dict(shape=shape, silu=silu, stats=stats) for silu in (True, False) for stats in ("recorded", "encoded")]
    if shape in ((24, 40, 4, 37), (1280, 640, 32, 129)):
        cases.append(dict(shape=shape, silu=True, stats="encoded", family="30+0.5g"))
    return cases


GS_SHAPES = ((2, 8, 1), (2, 520, 129), (1, 1280, 37))


def gn_stats_problem(device, shape, seed=351):
    """bc_gn_stats alone into a table that already holds totals: old + new."""
    B, C, HW = shape
    xh = (2.0 * g(seed, B * HW, C) + 0.5).half()
    old = torch.stack([50.0 * g(seed + 1, B, C).double(), 400.0 + 90.0 * g(seed + 2, B, C).double().abs()], -1)
    new = rc.gn_sums(xh, B)
    xa = xh.double().view(B, HW, C)
    bar = 2.0 ** -18 * torch.stack([xa.abs().sum(1), (xa * xa).sum(1)], -1)
    out = StatsOut(old, device)
    from blobctrl_amd.launch import decode_gn_tot, encode_gn_tot
    old_q = decode_gn_tot(encode_gn_tot(old))                 # (the table holds the old totals to 2^-60)
    xf = xh.float().view(B, HW, C)
    f32 = old_q + torch.stack([xf.sum(1), (xf * xf).sum(1)], -1).double()
    return Prob(f"gn_stats {shape}", "gn_stats", dict(B=B, C=C, HW=HW), dict(x=fence(xh, device)),
                [("totals", out, (old_q + new).reshape(B * C, 2), bar.reshape(B * C, 2))], dict(totals=f32.reshape(B * C, 2)))


# ---------------------------------------------------------------------------------------------------- layout launches
TO_NHWC_SHAPES = ((2, 3, 35, 8), (1, 4, 7, 8), (2, 5, 33, 16), (1, 3, 70000, 8))
TO_NCHW_SHAPES = ((2, 4, 35), (1, 3, 180000))
PATCHIFY_SHAPES = ((2, 28, 42, 14, 592), (1, 16, 32, 16, 768), (1, 8, 8, 4, 56), (1, 448, 448, 14, 592))


def to_nhwc_problem(device, shape, src_f32, seed=401):
    B, C, HW, Cpad = shape
    x = g(seed, B * C, HW)
    x = x if src_f32 else x.half()
    ref = torch.zeros(B, HW, Cpad, dtype=torch.float64)
    ref[..., :C] = x.double().view(B, C, HW).permute(0, 2, 1)
    outs = [("nhwc", rc.FencedOut(B * HW, Cpad, Cpad, device), ref.reshape(B * HW, Cpad), None)]
    return Prob(f"nchw_to_nhwc {shape} src={'fp32' if src_f32 else 'fp16'}", "to_nhwc", dict(B=B, C=C, HW=HW, Cpad=Cpad, f32=src_f32),
                dict(x=fence(x, device, f32=src_f32, guard=2)), outs)


def to_nchw_problem(device, shape, dst_f32, seed=411):
    B, C, HW = shape
    xh = g(seed, B * HW, C).half()
    ref = xh.double().view(B, HW, C).permute(0, 2, 1).reshape(B * C, HW)
    return Prob(f"nhwc_to_nchw {shape} dst={'fp32' if dst_f32 else 'fp16'}", "to_nchw", dict(B=B, C=C, HW=HW, ld=C + 4, f32=dst_f32),
                dict(x=fence(xh, device, ld=C + 4)), [("nchw", FlatOut(B * C, HW, device, f32=dst_f32), ref, None)])


def patchify_problem(device, shape, seed=421):
    B, H, W, p, Kpad = shape
    px = g(seed, B * 3 * H, W)
    gh, gw, K = H // p, W // p, 3 * p * p
    ref = torch.zeros(B * gh * gw, Kpad, dtype=torch.float64)
    ref[:, :K] = px.double().view(B, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, K)
    return Prob(f"patchify {shape}", "patchify", dict(B=B, H=H, W=W, patch=p, Kpad=Kpad), dict(px=fence(px, device, f32=True, guard=2)),
                [("rows", rc.FencedOut(B * gh * gw, Kpad, Kpad, device), ref, None)])


# ---------------------------------------------------------------------------------------------------- embeddings
CLS_POS_SHAPES = ((2, 5, 16), (3, 256, 1024))
EMBED_SHAPES = ((2, 7, 16, 99), (3, 77, 768, 1000), (3, 700, 2048, 50))
TOK_GUARD = 16                          # NaN rows in front of token 0 and behind token vocab - 1 (the ids reach -3 and vocab + 7)


def add_cls_pos_problem(device, shape, seed=431):
    B, T, D = shape
    ph, cls, pos = g(seed, B * T, D).half(), g(seed + 1, D), 0.5 * g(seed + 2, T + 1, D)
    tok = torch.cat([cls.double().expand(B, 1, D), ph.double().view(B, T, D)], 1)
    ref = (tok + pos.double()).reshape(B * (T + 1), D)
    f32 = (tok.float() + pos).half().double().reshape(B * (T + 1), D)
    views = dict(patches=fence(ph, device), cls=rc.fenced_vec(cls, device), pos=fence(pos, device, f32=True, guard=B * (T + 1)))
    return Prob(f"add_cls_pos {shape}", "add_cls_pos", dict(B=B, T=T, D=D), views,
                [("tokens", rc.FencedOut(B * (T + 1), D, D, device), ref, ulp16(ref))], dict(tokens=f32))


def embed_ids(seed, B, T, vocab):
    ids = buckets(seed, vocab, B, T)
    special = torch.tensor([-3, 0, vocab - 1, vocab, vocab + 7])
    for b in range(B):                                         # (another place in every image)
        ids[b, b:b + 5] = special
    return ids


def embed_tokens_problem(device, shape, zero_pos=False, seed=441):
    """zero_pos: the gather alone (exact); else the sum of the fp16 row and the fp32 position row t (never row b T + t: B > 1)."""
    B, T, D, vocab = shape
    ids = embed_ids(seed, B, T, vocab)
    tok, pos = g(seed + 1, vocab, D).half(), torch.zeros(T, D) if zero_pos else 0.5 * g(seed + 2, T, D)
    rows = tok.double()[ids.clamp(0, vocab - 1)]               # [B][T][D]
    ref = (rows + pos.double()).reshape(B * T, D)
    f32 = (rows.float() + pos).half().double().reshape(B * T, D)
    views = dict(tok=fence(tok, device, guard=TOK_GUARD), pos=fence(pos, device, f32=True, guard=B * T))
    return Prob(f"embed_tokens {shape}{' gather' if zero_pos else ''}", "embed_tokens", dict(B=B, T=T, D=D, vocab=vocab, ids=ids.reshape(-1).to(device)),
                views, [("rows", rc.FencedOut(B * T, D, D, device), ref, None if zero_pos else ulp16(ref))], {} if zero_pos else dict(rows=f32))


# ---------------------------------------------------------------------------------------------------- sample, silu
SAMPLE_SHAPES = ((2, 4, 35), (1, 4, 140000))
LOGVARS = (-40.0, -30.0, 0.0, 20.0, 25.0)
SILU_SIZES = (1, 255, 257, 600000)


def gaussian_sample_problem(device, shape, seed=451):
    B, Cz, HW = shape
    mean, noise = g(seed, B * HW, Cz), g(seed + 1, B * Cz, HW)
    lv = torch.tensor(LOGVARS)[buckets(seed + 2, 5, B * HW, Cz)]
    mom = torch.cat([mean, lv], 1).half()
    md = mom.double().view(B, HW, 2 * Cz).permute(0, 2, 1)     # [B][2 Cz][HW]
    m, l = md[:, :Cz].reshape(B * Cz, HW), md[:, Cz:].reshape(B * Cz, HW).clamp(-30.0, 20.0)
    sn = torch.exp(0.5 * l) * noise.double()
    ref = (m + sn) * SCALE
    bar = E20 * SCALE * (m.abs() + (1.0 + (0.5 * l).abs()) * sn.abs())
    f32 = ((m.float() + torch.exp(0.5 * l.float()) * noise) * np.float32(SCALE)).double()
    return Prob(f"gaussian_sample {shape}", "gaussian_sample", dict(B=B, Cz=Cz, HW=HW), dict(mom=fence(mom, device), noise=fence(noise, device, f32=True, guard=2)),
                [("z", FlatOut(B * Cz, HW, device, f32=True), ref, bar)], dict(z=f32))


def silu_problem(device, n, inplace, seed=461):
    x = (8.0 * g(seed, n)).clamp(-20.0, 20.0)
    if n > 8:
        x[:8] = torch.tensor([65504.0, -65504.0, 0.0, -0.0, 20.0, -20.0, 1.0, -1.0])
    xh = x.half()[None]
    xd = xh.double()
    ref = xd / (1.0 + torch.exp(-xd))
    bar = ulp16(ref) + E20 * (1.0 + xd.abs()) * ref.abs()
    xf = xh.float()
    f32 = (xf / (1.0 + torch.exp(-xf))).half().double()
    view = fence(xh, device, guard=1)
    out = InPlace(view) if inplace else FlatOut(1, n, device)
    return Prob(f"silu n={n} {'in place' if inplace else 'out of place'}", "silu", dict(n=n, inplace=inplace), dict(x=view), [("y", out, ref, bar)], dict(y=f32))


# ---------------------------------------------------------------------------------------------------- the row ops of the SAM path
ADD_ROWS_SHAPES = ((6, 3, 16), (5, 5, 8))
ACT_CHUNKS = (1, 257)


def add_pos_problem(device, shape=(2, 9, 24), seed=471):
    B, T, D = shape
    xh, pos = g(seed, B * T, D).half(), 0.5 * g(seed + 1, T, D)
    ref = (xh.double().view(B, T, D) + pos.double()).reshape(B * T, D)
    f32 = (xh.float().view(B, T, D) + pos).half().double().reshape(B * T, D)
    return Prob(f"add_pos {shape}", "add_pos", dict(B=B, T=T, D=D), dict(x=fence(xh, device), pos=fence(pos, device, f32=True, guard=B * T)),
                [("y", rc.FencedOut(B * T, D, D, device), ref, ulp16(ref))], dict(y=f32))


def add_rows_problem(device, shape, seed=481):
    rows, b_rows, C = shape
    a, b = g(seed, rows, C).half(), g(seed + 1, b_rows, C).half()
    ref = (a.double().view(rows // b_rows, b_rows, C) + b.double()).reshape(rows, C)
    return Prob(f"add_rows {shape}", "add_rows", dict(rows=rows, b_rows=b_rows, C=C), dict(a=fence(a, device), b=fence(b, device)),
                [("y", rc.FencedOut(rows, C, C, device), ref, None)])


def act_rows_problem(device, chunks, relu, seed=491):
    n = 8 * chunks
    x = (5.0 * g(seed, n)).clamp(-12.0, 12.0)
    x[:4] = torch.tensor([12.0, -12.0, 0.0, -0.0])
    xh = x.half()[None]
    xd = xh.double()
    view = fence(xh, device, guard=1)
    if relu:
        ref, bar, f32 = xd.clamp(min=0.0), None, {}
    else:
        ref = 0.5 * xd * (1.0 + torch.erf(xd * 0.5 ** 0.5))
        # (the restatement takes erfc(|z|) as the kernel does: 1 + erf(z) in fp32 cancels on the negative side, 6e-7 at x = -4)
        xf = xh.float()
        ec = torch.special.erfc(xf.abs() * 0.70710678118654752)
        bar, f32 = ulp16(ref) + 5e-7, dict(y=(0.5 * xf * torch.where(xf >= 0, 2.0 - ec, ec)).half().double())
    return Prob(f"act_rows chunks={chunks} {'relu' if relu else 'gelu'}", "act_rows", dict(n=n, act=1 if relu else 0), dict(x=view),
                [("y", InPlace(view), ref, bar)], f32)


# ---------------------------------------------------------------------------------------------------- dup_halves, memset_zero
DUP_HALF_BYTES = (16, 48, 4096 + 16, 5 * 2 ** 20 + 32)          # the last is more than 1024 x 256 x 16 bytes
DUP_SLOTS = (0, 2, 3, 5)                                        # of the six: p1 and p4 are null
DUP_NULL_BYTES = 64                                             # the size a null slot is passed with
MEMSET_BYTES = (16, 4080, 9 * 2 ** 20)                          # the last is more than 2048 x 256 x 16 bytes


def dup_halves_problem(device, seed=501):
    """Four buffers [2][bytes_k] of fp16: the first half holds data, the second the sentinel; behind 2 bytes_k the fence."""
    outs = []
    for k, nbytes in enumerate(DUP_HALF_BYTES):
        n = nbytes // 2
        half = g(seed + k, n).half()
        o = FlatOut(1, 2 * n, device)
        o.parent[o.offset:o.offset + n] = half.to(device)
        outs.append((f"slot {DUP_SLOTS[k]}", o, torch.cat([half, half]).double()[None], None))
    return Prob("dup_halves", "dup_halves", dict(bytes=DUP_HALF_BYTES), {}, outs)


def memset_zero_problem(device, nbytes):
    return Prob(f"memset_zero {nbytes}", "memset_zero", dict(bytes=nbytes), {}, [("zeros", FlatOut(1, nbytes // 2, device), torch.zeros(1, nbytes // 2, dtype=torch.float64), None)])


# ---------------------------------------------------------------------------------------------------- every problem by entry point
MAKERS = {
    "bc_layernorm": lambda d: [layernorm_problem(d, **c) for c in layernorm_cases()],
    "bc_softmax_rows": lambda d: [softmax_problem(d, **c) for cols in SM_COLS for c in softmax_cases(cols)],
    "groupnorm": lambda d: [groupnorm_problem(d, **c) for s in GN_SHAPES for c in groupnorm_cases(s)],
    "bc_gn_stats": lambda d: [gn_stats_problem(d, s) for s in GS_SHAPES],
    "bc_nchw_to_nhwc_f16": lambda d: [to_nhwc_problem(d, s, f) for s in TO_NHWC_SHAPES for f in (True, False)],
    "bc_nhwc_to_nchw": lambda d: [to_nchw_problem(d, s, f) for s in TO_NCHW_SHAPES for f in (True, False)],
    "bc_patchify": lambda d: [patchify_problem(d, s) for s in PATCHIFY_SHAPES],
    "bc_add_cls_pos": lambda d: [add_cls_pos_problem(d, s) for s in CLS_POS_SHAPES],
    "bc_embed_tokens": lambda d: [embed_tokens_problem(d, s) for s in EMBED_SHAPES] + [embed_tokens_problem(d, EMBED_SHAPES[0], zero_pos=True)],
    "bc_gaussian_sample": lambda d: [gaussian_sample_problem(d, s) for s in SAMPLE_SHAPES],
    "bc_silu": lambda d: [silu_problem(d, n, ip) for n in SILU_SIZES for ip in (True, False)],
    "bc_add_pos": lambda d: [add_pos_problem(d)],
    "bc_add_rows": lambda d: [add_rows_problem(d, s) for s in ADD_ROWS_SHAPES],
    "bc_act_rows": lambda d: [act_rows_problem(d, c, r) for c in ACT_CHUNKS for r in (True, False)],
    "bc_dup_halves": lambda d: [dup_halves_problem(d)],
    "bc_memset_zero": lambda d: [memset_zero_problem(d, b) for b in MEMSET_BYTES],
}
"""Entry point (groupnorm: bc_gn_apply_fused, or bc_gn_finalize + bc_gn_apply) -> device -> the list of its problems that must pass (the
refused forms are stated in the test modules)."""


# ---------------------------------------------------------------------------------------------------- a torch statement of every launch
MUTATIONS = {
    "layernorm": ("cover_divisor", "no_eps", "one_pass", "stride_C", "affine_pass0", "rows_round4"),
    "softmax": ("no_max", "pad_cols", "norm_512", "last_pass", "rows_round4"),
    "groupnorm": ("range_stats", "x1_for_x2", "pixel_tail", "wrong_cpg"),
    "gn_stats": ("overwrite", "slab_tail"),
    "to_nhwc": ("cap", "cp_swapped", "pad_unwritten"),
    "to_nchw": ("cap", "cp_swapped"),
    "patchify": ("cap", "pad_unwritten"),
    "add_cls_pos": ("cap", "pos_by_row"),
    "embed_tokens": ("cap", "no_clamp", "pos_by_row"),
    "gaussian_sample": ("cap", "no_clamp"),
    "silu": ("cap",),
    "dup_halves": ("cap", "uncompacted"),
    "memset_zero": ("cap",),
    "add_pos": (), "add_rows": (), "act_rows": (),
}


def _rd(view, rows, cols, ld=None, first=0):
    """rows x cols elements of the parent of `view` from element `first` of the view on, row stride ld - whatever lies there."""
    return view.parent.as_strided((rows, cols), (view.ld if ld is None else ld, 1), view.offset + first)


def _st(o, vals, first=0):
    """Store vals [rows][cols] at the view's rows (row stride o.ld), from element `first` of the view on."""
    dt = torch.float32 if o.f32 else torch.float16
    vals = torch.where(torch.isnan(vals), torch.full_like(vals, float("nan")), vals)     # (a computed NaN: not the payload of the fence it came from)
    o.parent.as_strided(tuple(vals.shape), (o.ld, 1), o.offset + first).copy_(vals.to(dt))


def _flat_idx(o):
    return (o.offset + torch.arange(o.rows)[:, None] * o.ld + torch.arange(o.width)[None, :]).flatten()


def _unwrite(o, mask):
    """Put back what the buffer held before the launch where mask [rows][width] is set: the sentinel, or an in-place launch's input."""
    idx = _flat_idx(o)[mask.flatten()]
    if isinstance(o, InPlace):
        b = o.parent.view(torch.int32 if o.f32 else torch.int16)
        b[idx] = o.before[idx]
    else:
        o.bits[idx] = o.sentinel


def _cap(o, per_thread=1, cap=CAP):
    """Only the first `cap` threads' worth of the output's elements (in the order of the flat index) is done."""
    n = o.rows * o.width
    _unwrite(o, (torch.arange(n) >= cap * per_thread).view(o.rows, o.width))


def emulate(prob, mutation=None):
    """What the launch of `prob` does, in torch: reads its views where the kernel reads them, computes in float64, stores into the output
    views.  `mutation` (MUTATIONS[prob.op]) makes one of the mistakes such a kernel can make."""
    assert mutation is None or mutation in MUTATIONS[prob.op], (prob.op, mutation)
    prob.prepare()
    globals()["_emulate_" + prob.op](prob, prob.args, prob.views, mutation)


def _emulate_layernorm(prob, a, v, m):
    """cover_divisor: mean and variance divided by the lanes' coverage 64 x 8 x MAXC, not by C | no_eps | one_pass: E[x^2] - mean^2 in fp32 |
    stride_C: the row stride taken as C | affine_pass0: gamma / beta of register pass i >= 1 indexed as pass 0 | rows_round4."""
    rows, C, ldx, eps = a["rows"], a["C"], a["ldx"], a["eps"]
    R = (rows + 3) // 4 * 4 if m == "rows_round4" else rows
    x = _rd(v["x"], R, C, C if m == "stride_C" else ldx).double()
    n = 512 * ln_passes(C) if m == "cover_divisor" else C
    if m == "one_pass":
        xf = x.float()
        mu = xf.sum(1, keepdim=True) / n
        var = ((xf * xf).sum(1, keepdim=True) / n - mu * mu).clamp(min=0.0).double()
        mu = mu.double()
    else:
        mu = x.sum(1, keepdim=True) / n
        var = ((x - mu) ** 2).sum(1, keepdim=True) / n
    col = torch.arange(C) % 512 if m == "affine_pass0" else torch.arange(C)
    gam, bet = (v[k].parent[v[k].offset + col].double() for k in ("gamma", "beta"))
    y = (x - mu) / torch.sqrt(var + (0.0 if m == "no_eps" else eps)) * gam + bet
    _st(prob.out("y"), y)


def _emulate_softmax(prob, a, v, m):
    """no_max: exp(x) in fp32 without the max subtraction | pad_cols: the row taken ld wide | norm_512: the normaliser from the first 512
    columns | last_pass: the last register pass (512 columns) not stored | rows_round4."""
    rows, cols, ld = a["rows"], a["cols"], a["ld"]
    R = (rows + 3) // 4 * 4 if m == "rows_round4" else rows
    W = ld if m == "pad_cols" else cols
    o = prob.out("p")
    x = _rd(v["x"], R, W).double()
    if m == "no_max":
        e = torch.exp(x.float()).double()
    else:
        e = torch.exp(x - x.max(1, keepdim=True).values)
    p = (e / e[:, :512 if m == "norm_512" else W].sum(1, keepdim=True))[:, :cols]
    _st(o, p)
    if m == "last_pass":
        _unwrite(o, (torch.arange(cols) >= (cols - 1) // 512 * 512)[None].expand(rows, cols))


def _emulate_groupnorm(prob, a, v, m):
    """range_stats: a group that straddles a 64-channel workgroup range takes its statistics from the range's own channels | x1_for_x2: x1
    read for the channels >= C1 | pixel_tail: the pixels behind the last full 32 of an image not stored | wrong_cpg: n = HW C1 / G."""
    C1, C2, G, HW, B, eps = a["C1"], a["C2"], a["G"], a["HW"], a["B"], a["eps"]
    C, M = C1 + C2, B * HW
    cpg = C // G
    if m == "x1_for_x2":
        x = _rd(v["x1"], M, C, C1).double()
    else:
        x = torch.cat([_rd(v["x1"], M, C1).double()] + ([_rd(v["x2"], M, C2).double()] if C2 else []), 1)
    xs = torch.cat([v["x1"].valid().double()] + ([v["x2"].valid().double()] if C2 else []), 1).view(B, HW, C)   # (statistics: the totals)
    s, q = xs.sum(1), (xs * xs).sum(1)                         # [B][C]
    ch = torch.arange(C)
    key = ch // cpg * (C // GN_RANGE + 2) + (ch // GN_RANGE if m == "range_stats" else 0)
    _, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    S = torch.zeros(B, len(cnt), dtype=torch.float64).index_add_(1, inv, s)[:, inv]
    Q = torch.zeros(B, len(cnt), dtype=torch.float64).index_add_(1, inv, q)[:, inv]
    n = HW * ((C1 // G) if (m == "wrong_cpg" and C2) else cpg) * (cnt[inv].double() / cpg if m == "range_stats" else 1.0)
    mean = S / n
    var = (Q / n - mean * mean).clamp(min=0.0)
    aa = (1.0 / torch.sqrt(var + eps)) * v["gamma"].valid().double()
    bb = v["beta"].valid().double() - mean * aa
    t = x.view(B, HW, C) * aa[:, None] + bb[:, None]
    y = t * torch.sigmoid(t) if a["silu"] else t
    o = prob.out("y")
    _st(o, y.reshape(M, C))
    if m == "pixel_tail":
        _unwrite(o, (torch.arange(M) % HW >= HW // 32 * 32)[:, None].expand(M, C))


def _emulate_gn_stats(prob, a, v, m):
    """overwrite: the totals stored, not added | slab_tail: a slab of one pixel skipped."""
    from blobctrl_amd.launch import encode_gn_tot
    B, C, HW = a["B"], a["C"], a["HW"]
    x = _rd(v["x"], B * HW, C).double().view(B, HW, C)
    if m == "slab_tail" and HW % GN_SLAB == 1:
        x = x[:, :HW - 1]
    enc = encode_gn_tot(torch.stack([x.sum(1), (x * x).sum(1)], -1))
    o = prob.out("totals")
    if m == "overwrite":
        o.t.copy_(enc)
    else:
        o.t.add_(enc)


def _emulate_to_nhwc(prob, a, v, m):
    """cap | cp_swapped: element (b, c, p) of the source taken as (b, p, c) | pad_unwritten: the lanes C .. Cpad not stored."""
    B, C, HW, Cpad = a["B"], a["C"], a["HW"], a["Cpad"]
    src = _rd(v["x"], B * C, HW).double().view(B, C, HW)
    y = torch.zeros(B, HW, Cpad, dtype=torch.float64)
    y[..., :C] = src.reshape(B, HW, C) if m == "cp_swapped" else src.permute(0, 2, 1)
    o = prob.out("nhwc")
    _st(o, y.reshape(B * HW, Cpad))
    if m == "pad_unwritten":
        _unwrite(o, (torch.arange(Cpad) >= C)[None].expand(B * HW, Cpad))
    if m == "cap":
        _cap(o)


def _emulate_to_nchw(prob, a, v, m):
    B, C, HW = a["B"], a["C"], a["HW"]
    src = _rd(v["x"], B * HW, C).double().view(B, HW, C)
    y = src.reshape(B, C, HW) if m == "cp_swapped" else src.permute(0, 2, 1)
    o = prob.out("nchw")
    _st(o, y.reshape(B * C, HW))
    if m == "cap":
        _cap(o)


def _emulate_patchify(prob, a, v, m):
    B, H, W, p, Kpad = a["B"], a["H"], a["W"], a["patch"], a["Kpad"]
    gh, gw, K = H // p, W // p, 3 * p * p
    px = _rd(v["px"], B * 3 * H, W).double()
    y = torch.zeros(B * gh * gw, Kpad, dtype=torch.float64)
    y[:, :K] = px.view(B, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, K)
    o = prob.out("rows")
    _st(o, y)
    if m == "pad_unwritten":
        _unwrite(o, (torch.arange(Kpad) >= K)[None].expand(B * gh * gw, Kpad))
    if m == "cap":
        _cap(o)


def _pos_rows(view, B, T, by_row):
    """The position rows of B images of T tokens [B T][D]: row t, or - the mistake - row b T + t."""
    rows = torch.arange(B * T) if by_row else torch.arange(B * T) % T
    return _rd(view, B * T, view.cols).double()[rows]


def _emulate_add_cls_pos(prob, a, v, m):
    B, T, D = a["B"], a["T"], a["D"]
    tok = torch.cat([v["cls"].valid().double().expand(B, 1, D), _rd(v["patches"], B * T, D).double().view(B, T, D)], 1)
    o = prob.out("tokens")
    _st(o, tok.reshape(B * (T + 1), D) + _pos_rows(v["pos"], B, T + 1, m == "pos_by_row"))
    if m == "cap":
        _cap(o)


def _emulate_embed_tokens(prob, a, v, m):
    B, T, D, vocab = a["B"], a["T"], a["D"], a["vocab"]
    ids = a["ids"].cpu()
    ids = ids if m == "no_clamp" else ids.clamp(0, vocab - 1)
    table = _rd(v["tok"], vocab + 2 * TOK_GUARD, D, first=-TOK_GUARD * D).double()
    o = prob.out("rows")
    _st(o, table[ids + TOK_GUARD] + _pos_rows(v["pos"], B, T, m == "pos_by_row"))
    if m == "cap":
        _cap(o, per_thread=8)


def _emulate_gaussian_sample(prob, a, v, m):
    B, Cz, HW = a["B"], a["Cz"], a["HW"]
    md = _rd(v["mom"], B * HW, 2 * Cz).double().view(B, HW, 2 * Cz).permute(0, 2, 1)
    mean, lv = md[:, :Cz].reshape(B * Cz, HW), md[:, Cz:].reshape(B * Cz, HW)
    lv = lv if m == "no_clamp" else lv.clamp(-30.0, 20.0)
    o = prob.out("z")
    _st(o, (mean + torch.exp(0.5 * lv) * _rd(v["noise"], B * Cz, HW).double()) * SCALE)
    if m == "cap":
        _cap(o)


def _emulate_silu(prob, a, v, m):
    x = _rd(v["x"], 1, a["n"]).double()
    o = prob.out("y")
    _st(o, x / (1.0 + torch.exp(-x)))
    if m == "cap":
        _cap(o)


def _emulate_add_pos(prob, a, v, m):
    B, T, D = a["B"], a["T"], a["D"]
    _st(prob.out("y"), _rd(v["x"], B * T, D).double() + _pos_rows(v["pos"], B, T, False))


def _emulate_add_rows(prob, a, v, m):
    rows, b_rows, C = a["rows"], a["b_rows"], a["C"]
    _st(prob.out("y"), _rd(v["a"], rows, C).double() + _rd(v["b"], b_rows, C).double()[torch.arange(rows) % b_rows])


def _emulate_act_rows(prob, a, v, m):
    x = _rd(v["x"], 1, a["n"]).double()
    _st(prob.out("y"), x.clamp(min=0.0) if a["act"] else 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5)))


def _emulate_dup_halves(prob, a, v, m):
    """cap: 262144 threads' worth of 16 bytes | uncompacted: compacted slot k takes the size the caller passed for slot k of the six."""
    passed = [DUP_NULL_BYTES] * 6
    for k, slot in enumerate(DUP_SLOTS):
        passed[slot] = a["bytes"][k]
    for k, (_, o, _, _) in enumerate(prob.outs):
        n = (passed[k] if m == "uncompacted" else a["bytes"][k]) // 2
        done = min(n, DUP_CAP * 8) if m == "cap" else n
        src = o.bits[o.offset:o.offset + done].clone()
        o.bits[o.offset + n:o.offset + n + done] = src


def _emulate_memset_zero(prob, a, v, m):
    o = prob.outs[0][1]
    n = a["bytes"] // 2
    o.bits[o.offset:o.offset + (min(n, CAP * 8) if m == "cap" else n)] = 0
