"""Cases, inputs, float64 references and fenced problems of perturbed-attention guidance (tests/test_pag_cpu.py, tests/test_pag_gpu.py,
tools/make_golden.py golden_blocks_pag / golden_unet_pag / golden_pipeline_call_pag).  Nothing here needs a device.

The float64 restatements below - the block whose attn1 is the identity on V for the perturbed images, the guidance formulas, the step of
one table row - are what the GPU tests check launches against; tests/test_pag_cpu.py holds them to the reference's own outputs
(tests/golden/blocks_pag.npz) first."""
import torch
import torch.nn.functional as F

from tests import norm_layout_common as nl
from tests.common import g

BP = "transformer_blocks.0."

# ---------------------------------------------------------------------------------------------------- bc_attention_identity alone
IDENTITY_BATCHES = ((3, 2), (2, 1), (6, 4))               # (B, b0)
IDENTITY_TOKENS = (64, 72, 288)                           # one full tile; a ragged second tile; 288 = the 768^2 mid block (ragged fifth)
IDENTITY_HEADS = ((2, 8), (8, 40), (8, 160))              # C = 16 (a quarter of a channel tile), 320 (five tiles), 1280
IDENTITY_LDO_EXTRA = (0, 8)


def sentinel_rows(rows, cols):
    """A finite fp16 pattern with no two neighbours equal: what the output buffer holds before the launch."""
    i = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols)
    return ((i * 7 + 3) % 1021 - 510).div(8).half()


class IdentityProblem:
    """One bc_attention_identity launch in fenced buffers: V^T [B * C][HW] inside a NaN parent with row stride ldvt = ceil64(HW) (its
    pad columns are NaN), the output [B * HW][C] an in-place NaN-fenced buffer of row stride ldo that holds `sentinel_rows`."""

    def __init__(self, device, B, b0, HW, heads, d, ldo_extra, seed=5100):
        self.B, self.b0, self.HW, self.C = B, b0, HW, heads * d
        self.ldvt, self.ldo = (HW + 63) // 64 * 64, self.C + ldo_extra
        self.v = g(seed + HW + self.C, B, HW, self.C).half()                                 # [B][HW][C]: what to_v put out
        self.vt = nl.fence(self.v.transpose(1, 2).reshape(B * self.C, HW), device, ld=self.ldvt)
        self.before = sentinel_rows(B * HW, self.C)
        self.o = nl.InPlace(nl.fence(self.before, device, ld=self.ldo))

    def assert_inside(self):
        nl.inside(self.vt)
        self.o.assert_inside()

    def args(self):
        """The arguments of Recorder.attention_identity."""
        return (self.vt.t, self.o.t, self.B, self.b0, self.HW, self.C, self.ldvt, self.ldo)

    def expected(self):
        """[B * HW][C] fp16: the sentinel rows of the images in front of b0, then V."""
        want = self.before.clone()
        want[self.b0 * self.HW:] = self.v.reshape(self.B * self.HW, self.C)[self.b0 * self.HW:]
        return want


# ---------------------------------------------------------------------------------------------------- the guidance and the step
def pag_guidance(eps, B, g_scale, s, single):
    """`_apply_perturbed_attention_guidance` in the dtype of `eps` ([chunks * B, ...]): e_u + g (e_c - e_u) + s (e_c - e_p) on
    [uncond | cond | perturbed], or with `single` e_c + s (e_c - e_p) on [cond | perturbed]."""
    if single:
        ec, ep = eps[:B], eps[B:2 * B]
        return ec + s * (ec - ep)
    eu, ec, ep = eps[:B], eps[B:2 * B], eps[2 * B:3 * B]
    return eu + g_scale * (ec - eu) + s * (ec - ep)


def host_step(c, e, x, hist, noise, third):
    """float64: one coefficient row `c` on the guided eps `e` [B][4][h][w] (+ c12 * noise, + c13 * x0_{i-2}): (x_next, hist_next [3][n])."""
    c = c.double()
    n = x.numel()
    m0, m1, last = (hist.double()[k].reshape(x.shape) for k in range(3))
    xd, e = x.double(), e.double()
    x0 = xd * c[0] - e * c[1]
    xc = c[3] * last + c[4] * m0 + c[5] * m1 + c[6] * x0 if c[2] != 0 else xd
    xn = c[7] * xc + c[8] * x0 + c[9] * m0 + c[10] * e
    if third:
        xn = xn + c[13] * m1
    if noise is not None:
        xn = xn + c[12] * noise.double()
    return xn, torch.stack([x0.reshape(n), m0.reshape(n), xc.reshape(n)])


STEP_B, STEP_H, STEP_W, STEP_N = 2, 3, 5, 4
STEP_FORMS = ("plain", "noise", "third")
STEP_BAR = 1e-6                        # max-abs error over max |reference|, per buffer: the bar of tests/test_lcm_gpu.py's step test


def step_inputs(form, single, seed=5200):
    """The fp32 inputs of one bc_pag_scheduler_step launch at step index 1 of STEP_N: coef [N][16] (every column the form reads is
    non-zero, the corrector branch on), pag_table [N] with distinct rows, eps token-major [chunks * B][h][2w][4] whose LEFT halves are
    garbage, latents, hist, noise.  Returns a dict; `eps_nchw` = the right halves as [chunks * B][4][h][w]."""
    B, h, w, N = STEP_B, STEP_H, STEP_W, STEP_N
    chunks = 2 if single else 3
    coef = 0.5 + torch.rand(N, 16, generator=torch.Generator().manual_seed(seed)) * 0.5
    coef[:, 11] = torch.tensor([7.5, 5.0, 3.0, 2.0])
    if form != "third":
        coef[:, 13] = 0.0
    pag_table = torch.tensor([3.0, 1.75, 0.5, 0.0])
    eps_nchw = g(seed + 1, chunks * B, 4, h, w)
    tok = torch.randn(chunks * B, h, 2 * w, 4, generator=torch.Generator().manual_seed(seed + 2)) * 50
    tok[:, :, w:] = eps_nchw.permute(0, 2, 3, 1)
    return dict(coef=coef, pag_table=pag_table, tok=tok, eps_nchw=eps_nchw, x=g(seed + 3, B, 4, h, w), hist=g(seed + 4, 3, B * 4 * h * w),
                noise=torch.stack([g(seed + 10 + i, B, 4, h, w) for i in range(N)]) if form == "noise" else None, step=1)


def step_reference(inp, form, single, eps_nchw=None, s_row=None):
    """float64 from the launch's own fp32 inputs: (eps_guided, x_next, hist_next).  `eps_nchw` / `s_row`: a wrong launch - other chunks,
    the scale of another table row - for the power check."""
    i = inp["step"]
    eps = (inp["eps_nchw"] if eps_nchw is None else eps_nchw).double()
    s = float(inp["pag_table"][i if s_row is None else s_row])
    e = pag_guidance(eps, STEP_B, float(inp["coef"][i, 11]), s, single)
    xn, hist = host_step(inp["coef"][i], e, inp["x"], inp["hist"], None if inp["noise"] is None else inp["noise"][i], form == "third")
    return e, xn, hist


def step_power(inp, form, single):
    """{wrong launch: share of the latent elements on which its float64 result lies outside STEP_BAR of the true one} - the cond and
    perturbed chunks swapped, the scale taken from the row in front and from the row behind."""
    B = STEP_B
    _, ref, _ = step_reference(inp, form, single)
    bar = STEP_BAR * ref.abs().max()
    e = inp["eps_nchw"]
    lo = 0 if single else B
    swapped = torch.cat([e[:lo], e[lo + B:lo + 2 * B], e[lo:lo + B]])
    wrong = {"swapped": dict(eps_nchw=swapped), "row_before": dict(s_row=inp["step"] - 1), "row_behind": dict(s_row=inp["step"] + 1)}
    return {k: float(((step_reference(inp, form, single, **kw)[1] - ref).abs() > bar).double().mean()) for k, kw in wrong.items()}


# ---------------------------------------------------------------------------------------------------- one block with the PAG processor
# One Transformer2DModel with PAGCFGIdentitySelfAttnProcessor2_0 (chunks = 3: [uncond | cond | perturbed]) or
# PAGIdentitySelfAttnProcessor2_0 (chunks = 2: [cond | perturbed]) on attn1 (tests/golden/blocks_pag.npz, tools/make_golden.py
# golden_blocks_pag), on the smallest canvas at which the planner still takes each form, as tests/ip_adapter_common.py IP_BLOCK_CASES:
# 320 channels from one 64-row block (row-chain; BC_PLAN rowchain=0 gives the unfused list on the same fixture), 640 channels from 64 row
# blocks (row-chain), 1280 channels at HW = 64 (gemm_wreg.hip).  B = 6 puts both chunk boundaries inside the batch.  The cond and the
# perturbed chunk get identical inputs.  Outputs only (every `sub`-th pixel): weights and inputs come from seeds.
PAG_BLOCK_CASES = {
    "pag_320": dict(C=320, heads=8, ctx=768, B=6, H=8, W=16, sub=4, chunks=3),
    "pag_640": dict(C=640, heads=8, ctx=768, B=3, H=32, W=64, sub=16, chunks=3),
    "pag_1280": dict(C=1280, heads=8, ctx=768, B=6, H=8, W=8, sub=4, chunks=3),
    "pag_320_nocfg": dict(C=320, heads=8, ctx=768, B=4, H=8, W=16, sub=4, chunks=2),
}
PAG_BLOCK_SEED = 5300


def pag_block_weights(name):
    """The block's state dict as Transformer2DModel spells it."""
    from blobctrl_amd import synth
    from tests.common import block_param_shapes
    return synth.synth_state_dict(block_param_shapes("transformer", PAG_BLOCK_CASES[name]), PAG_BLOCK_SEED + sorted(PAG_BLOCK_CASES).index(name))


def pag_block_inputs(name):
    """(x NCHW [B][C][H][W], text context [B][7][ctx]): the last chunk is a copy of the chunk in front of it."""
    p = PAG_BLOCK_CASES[name]
    i, n = sorted(PAG_BLOCK_CASES).index(name), p["B"] // p["chunks"]
    x, ctx = g(5400 + i, p["B"] - n, p["C"], p["H"], p["W"]), g(5500 + i, p["B"] - n, 7, p["ctx"])
    return torch.cat([x, x[-n:]]), torch.cat([ctx, ctx[-n:]])


def attention64(sd, p, x, ctx, heads, identity_from=None):
    """attention_processor.py AttnProcessor2_0 in the dtype of x; images >= identity_from take to_out(to_v(x)) (the PAG identity)."""
    B, N, C = x.shape
    src = x if ctx is None else ctx
    w = lambda k: sd[p + k].to(x.dtype)
    v = F.linear(src, w("to_v.weight"))
    d = C // heads
    split = lambda t: t.view(B, -1, heads, d).transpose(1, 2)
    q, k = split(F.linear(x, w("to_q.weight"))), split(F.linear(src, w("to_k.weight")))
    o = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, -1) @ split(v)
    o = o.transpose(1, 2).reshape(B, -1, C)
    if identity_from is not None:
        o = torch.cat([o[:identity_from], v[identity_from:]])
    return F.linear(o, w("to_out.0.weight"), w("to_out.0.bias"))


def pag_block_reference(sd, x, ctx, heads, groups=32, n_perturbed=0, dtype=torch.float64):
    """transformer_2d.py:479-527 + attention.py:421-541 in `dtype`, attn1 of the last `n_perturbed` images replaced by the identity on V
    (PAGCFGIdentitySelfAttnProcessor2_0 / PAGIdentitySelfAttnProcessor2_0): NCHW in, NCHW out."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x, ctx = x.to(dtype), ctx.to(dtype)
    B, C, H, W = x.shape
    h = F.group_norm(x, groups, sd["norm.weight"], sd["norm.bias"], 1e-6)
    h = F.conv2d(h, sd["proj_in.weight"], sd["proj_in.bias"]).permute(0, 2, 3, 1).reshape(B, H * W, C)
    ln = lambda t, k: F.layer_norm(t, (C,), sd[BP + k + ".weight"], sd[BP + k + ".bias"], 1e-5)
    h = attention64(sd, BP + "attn1.", ln(h, "norm1"), None, heads, identity_from=B - n_perturbed if n_perturbed else None) + h
    h = attention64(sd, BP + "attn2.", ln(h, "norm2"), ctx, heads) + h
    val, gate = F.linear(ln(h, "norm3"), sd[BP + "ff.net.0.proj.weight"], sd[BP + "ff.net.0.proj.bias"]).chunk(2, dim=-1)
    h = F.linear(val * F.gelu(gate), sd[BP + "ff.net.2.weight"], sd[BP + "ff.net.2.bias"]) + h
    h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)
    return F.conv2d(h, sd["proj_out.weight"], sd["proj_out.bias"]) + x


def pag_block_plan(name, device, perturbed=True):
    """The block of a case recorded through TrunkPlan on `device` ("cpu": recording only) with the block's prefix among the plan's PAG
    layers, as the planner records a PAG layer.  Returns (recorder, segment, output Act)."""
    from blobctrl_amd.engine import Act, TrunkConfig, TrunkPlan
    from blobctrl_amd.launch import Recorder
    from blobctrl_amd.weights import PackedTrunk
    p = PAG_BLOCK_CASES[name]
    dev = torch.device(device)
    x, ctx = pag_block_inputs(name)
    sd = {"blk." + k: v for k, v in pag_block_weights(name).items()}
    sd["conv_in.weight"] = torch.zeros(8, 4, 3, 3)                      # (PackedTrunk expects a trunk: unused stand-ins)
    sd["none.time_emb_proj.weight"], sd["none.time_emb_proj.bias"] = torch.zeros(8, 1280), torch.zeros(8)
    pw = PackedTrunk(sd, dev, (320, 640, 1280, 1280))
    rec = Recorder(dev)
    seg = rec.begin(name)
    plan = TrunkPlan(rec, pw, TrunkConfig(in_channels=4, num_heads=p["heads"], norm_num_groups=32, cross_attention_dim=p["ctx"]), p["B"], p["H"], p["W"])
    plan.res_events, plan.res_bmod = None, 1
    if perturbed:
        plan.pag_layers, plan.pag_images = frozenset(["blk."]), p["B"] // p["chunks"]
    plan.record_context(ctx.reshape(-1, p["ctx"]).half().to(dev), ctx.shape[1])
    B, C, H, W = x.shape
    out, _ = plan.transformer("blk.", Act(x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous().half().to(dev), C, H, W))
    return rec, seg, out


# ---------------------------------------------------------------------------------------------------- the tiny UNet with PAG processors
# tests/golden/unet_tiny_pag.npz (tools/make_golden.py golden_unet_pag): the tiny UNet of tests.common at batch 3 = [uncond | cond |
# perturbed] on the wide canvas of unet_tiny_ip.npz, with seeded residual stand-ins; the processors set by PAGMixin._set_pag_attn_processor.
PAG_UNET_LAYERS = {"mid": ["mid"], "down1_up": ["down_blocks.1", "up"]}
PAG_UNET_GEOMETRY = (3, 16, 32)
PAG_RES_SCALE = 0.1
# The tiny UNet's mid block alone moves eps by 2.5 bars (1e-2 of eps' scale) with the weights of tests.common, and by 0.4 to 4.2 over the
# seeds, canvases (16 x 32, 32 x 64, 16 x 16), timesteps, input and residual scales tried: its attn1 output is a small part of what the
# twelve up-block resnets and their skips make of it.  The PAG fixtures therefore run the tiny UNet with ONE weight changed - the value
# projection of the mid block's attn1 times PAG_MID_VALUE_GAIN, on the reference's side and on the engine's - so that what the perturbation
# touches carries more of eps: 24 bars for "mid" alone at this gain (8.9 at 4, 14.9 at 8), fp16 rounding of weights and inputs unchanged
# (1.3e-3 of scale at every gain).  Every case of both fixtures asserts 10 bars.
PAG_MID_VALUE_KEY = "mid_block.attentions.0.transformer_blocks.0.attn1.to_v.weight"
PAG_MID_VALUE_GAIN = 16.0
PAG_UNET_SEED = 5600
PAG_MATCH_IDS = ("mid", "down", "up", "down_blocks.1", "up_blocks.(1|2)", "attentions.0", "blocks.1", "down_blocks.0.attentions.1", "no_such_layer")
PAG_SCALE_TIMESTEPS = (999, 801, 601, 401, 201, 1)
PAG_SCALE_CASES = {"plain": (3.0, 0.0), "adaptive": (3.0, 0.005), "clamped": (1.0, 0.01)}


def pag_tiny_unet_weights():
    """The UNet state dict of the PAG fixtures: tests.common.tiny_weights with the mid block's attn1.to_v times PAG_MID_VALUE_GAIN."""
    from tests.common import tiny_weights
    usd = dict(tiny_weights()[0])
    usd[PAG_MID_VALUE_KEY] = usd[PAG_MID_VALUE_KEY] * PAG_MID_VALUE_GAIN
    return usd


def pag_unet_inputs():
    """(x [3][5][H][W], text [3][7][ctx], residual seed): images 1 and 2 - cond and perturbed - are identical."""
    from tests.common import TINY
    _, H, W = PAG_UNET_GEOMETRY
    x, ehs = g(PAG_UNET_SEED + 500, 2, 5, H, W), g(PAG_UNET_SEED + 501, 2, 7, TINY["ctx"])
    return torch.cat([x, x[1:]]), torch.cat([ehs, ehs[1:]]), PAG_UNET_SEED


def pag_residual(seed, shape):
    """One residual stand-in [3][C][H][W'] of `shape` = (C, H, W'): images 1 and 2 identical."""
    r = g(seed, 2, *shape) * PAG_RES_SCALE
    return torch.cat([r, r[1:]])


# ---------------------------------------------------------------------------------------------------- __call__ with PAG
# tests/golden/pipeline_call_pag.npz (tools/make_golden.py golden_pipeline_call_pag): the case ddim_neg2 of pipeline_call.npz, 3 steps, with
# seeds of its own; case -> the keywords that differ.  "euler" runs EulerDiscreteScheduler (a table that scales the model input).
PAG_CALL_LAYERS = "mid"
# The cases the PAG pipelines' defaults give: layers "mid", pag_scale = 3.0, on the UNet of pag_tiny_unet_weights (with the weights of
# tests.common the 1 x 2 tokens of the mid block at 64 x 64 pixels move the edit by 1.6 bars).  The adaptive case falls from 1.67 to 0.33 and
# clamps at 0 on the last of its three steps.
PAG_CALL_CASES = {
    "pag": dict(pag_scale=3.0),
    "adaptive": dict(pag_scale=3.0, pag_adaptive_scale=0.004),
    "half": dict(pag_scale=1.5),
    "off": dict(),
    "nocfg": dict(pag_scale=3.0, guidance_scale=1.0),
    "nocfg_off": dict(guidance_scale=1.0),
    "euler": dict(pag_scale=3.0),
    "euler_off": dict(),
}
PAG_CALL_PAIRS = (("pag", "off"), ("adaptive", "pag"), ("adaptive", "off"), ("half", "pag"), ("half", "off"), ("nocfg", "nocfg_off"),
                  ("euler", "euler_off"))
PAG_CALL_SEEDS = dict(seed=2052, rng_seed=51)
