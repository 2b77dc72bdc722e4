"""Masked edits (include/blobctrl_blend.h): what the CPU tests, the GPU tests and tools/make_golden.py share - the cases of
tests/golden/pipeline_call_blend.npz, the mask, and the float64 restatement of the blended step with its power check."""
import numpy as np
import torch

from tests.common import g

STEP_BAR = 1e-6                         # max-abs error over max |reference|, per buffer: the bar of the PAG and LCM step tests
CALL_BAR = 1e-2                         # of the latents' scale: the bar of every pipeline-call test

# ---------------------------------------------------------------------------------------------------- the fixture's cases
# The reference's own `__call__` at 64 x 64, 3 steps, case `ddim_neg2` of pipeline_call.npz (two prompts, negative prompts), `latents=` given,
# the blend applied to what scheduler.step returns with the reference scheduler's own add_noise (tools/make_golden.py
# golden_pipeline_call_blend says why not from callback_on_step_end).  Every case runs with and without the blend.
BLEND_SEEDS = dict(seed=2031, rng_seed=37, latents=5401, image=5402)
BLEND_STEPS = 3
BLEND_CASES = {
    "unipc": dict(scheduler="unipc"),
    "ddim": dict(scheduler="ddim"),
    "ddim_eta": dict(scheduler="ddim", eta=0.5),
    "dpm2m": dict(scheduler="dpm2m"),
    "dpm3m": dict(scheduler="dpm3m", num_inference_steps=5),      # (orders 1, 2, 3, 2, 1: at 3 steps a 3M table is the 2M table)
    "sde": dict(scheduler="sde"),
    "euler": dict(scheduler="euler"),
    "eulera": dict(scheduler="eulera"),
    "lcm_nocfg": dict(scheduler="lcm", guidance_scale=1.0),
    "ddim_two": dict(scheduler="ddim", num_images_per_prompt=2),
}
# asymmetric, 30 of 64 cells set: rows and columns differ, so a transposed, flipped or channel-indexed mask is another mask
BLEND_MASK = np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                       [0, 1, 1, 1, 0, 0, 0, 0],
                       [0, 1, 1, 1, 1, 1, 0, 0],
                       [0, 1, 1, 1, 1, 1, 1, 0],
                       [0, 0, 1, 1, 1, 1, 1, 1],
                       [0, 0, 0, 1, 1, 1, 1, 1],
                       [1, 0, 0, 0, 0, 1, 1, 1],
                       [1, 1, 0, 0, 0, 0, 0, 1]], dtype=np.float32)


def make_scheduler(mod, kind, sd):
    """The scheduler of a case from `mod` - the reference's `diffusers` or blobctrl_amd.schedulers: the same names and calls on both."""
    ddim = mod.DDIMScheduler(**sd, clip_sample=False, set_alpha_to_one=False)
    if kind == "ddim":
        return ddim
    if kind == "unipc":
        return mod.UniPCMultistepScheduler(**sd)
    if kind in ("dpm2m", "dpm3m", "sde"):
        extra = dict(dpm2m={}, dpm3m=dict(solver_order=3), sde=dict(algorithm_type="sde-dpmsolver++"))[kind]
        return mod.DPMSolverMultistepScheduler.from_config(ddim.config, **extra)
    if kind == "euler":
        return mod.EulerDiscreteScheduler.from_config(ddim.config)
    if kind == "eulera":
        return mod.EulerAncestralDiscreteScheduler.from_config(ddim.config, timestep_spacing="leading")
    if kind == "lcm":
        return mod.LCMScheduler.from_config(ddim.config)
    raise KeyError(kind)


def blend_inputs(batch):
    """(start latents = the noise, image latents, mask [1][1][8][8]) of the fixture's calls at `batch` images."""
    return g(BLEND_SEEDS["latents"], batch, 4, 8, 8), g(BLEND_SEEDS["image"], batch, 4, 8, 8) * 0.18215 * 5, \
        torch.from_numpy(BLEND_MASK)[None, None]


# ---------------------------------------------------------------------------------------------------- the blended step in float64
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


def blend(xn, image, bnoise, mask, row):
    """float64: xn [B][4][h][w] blended with a * image + s * bnoise through mask [B][h][w] (one value for the 4 channels)."""
    m = mask.double()[:, None]
    p = float(row[0]) * image.double() + float(row[1]) * bnoise.double()
    return (1 - m) * p + m * xn.double()


def guidance(eps, B, g_scale, s, single, pag):
    """The guided eps in the dtype of `eps`: [uncond | cond (| perturbed)] or with `single` [cond (| perturbed)]."""
    if single:
        ec = eps[:B]
        return ec + s * (ec - eps[B:2 * B]) if pag else ec
    eu, ec = eps[:B], eps[B:2 * B]
    e = eu + g_scale * (ec - eu)
    return e + s * (ec - eps[2 * B:3 * B]) if pag else e


STEP_SHAPES = ((2, 3, 5), (3, 9, 10))   # (B, h, w): 120 elements = one partial block; 1080 = four full blocks and a partial one
STEP_N = 4
STEP_FORMS = ("plain", "noise", "third")


def step_inputs(shape, form, single, pag, seed=5500, binary=False):
    """The fp32 inputs of one bc_blend_scheduler_step launch at step index 1 of STEP_N at `shape`: coef [N][16] (every column the form
    reads is non-zero, the corrector branch on), pag_table and blend_table [N] with distinct rows, eps token-major [chunks * B][h][2w][4]
    whose LEFT halves are garbage, latents, hist, noise, image, bnoise and a mask that differs per image - soft values in (0, 1), or with
    `binary` 0 / 1."""
    B, h, w = shape
    N = STEP_N
    chunks = (1 if single else 2) + (1 if pag else 0)
    gen = torch.Generator().manual_seed(seed)
    coef = 0.5 + torch.rand(N, 16, generator=gen) * 0.5
    coef[:, 11] = torch.tensor([7.5, 5.0, 3.0, 2.0])
    if form != "third":
        coef[:, 13] = 0.0
    blend_table = 0.25 + torch.rand(N, 2, generator=gen)
    mask = torch.rand(B, h, w, generator=gen) * 0.9 + 0.05
    if binary:
        mask = (mask > 0.5).float()
    eps_nchw = g(seed + 1, chunks * B, 4, h, w)
    tok = torch.randn(chunks * B, h, 2 * w, 4, generator=torch.Generator().manual_seed(seed + 2)) * 50
    tok[:, :, w:] = eps_nchw.permute(0, 2, 3, 1)
    return dict(shape=shape, coef=coef, pag_table=torch.tensor([3.0, 1.75, 0.5, 0.0]) if pag else None, blend_table=blend_table, mask=mask,
                tok=tok, eps_nchw=eps_nchw, x=g(seed + 3, B, 4, h, w), hist=g(seed + 4, 3, B * 4 * h * w),
                noise=torch.stack([g(seed + 10 + i, B, 4, h, w) for i in range(N)]) if form == "noise" else None,
                image=g(seed + 5, B, 4, h, w), bnoise=g(seed + 6, B, 4, h, w), step=1)


def step_reference(inp, form, single, wrong=None):
    """float64 from the launch's own fp32 inputs: (eps_guided, x_next, hist_next).  `wrong`: one of WRONG_LAUNCHES, for the power check."""
    i, (B, h, w) = inp["step"], inp["shape"]
    pag = inp["pag_table"] is not None
    e = guidance(inp["eps_nchw"].double(), B, float(inp["coef"][i, 11]), float(inp["pag_table"][i]) if pag else 0.0, single, pag)
    noise = None if inp["noise"] is None else inp["noise"][i]
    image, bnoise, mask, row = inp["image"], inp["bnoise"], inp["mask"], inp["blend_table"][i]
    if wrong == "blend order" and noise is not None:                      # the blend in front of the noise term
        xn, hist = host_step(inp["coef"][i], e, inp["x"], inp["hist"], None, form == "third")
        return e, blend(xn, image, bnoise, mask, row) + inp["coef"][i, 12].double() * noise.double(), hist
    xn, hist = host_step(inp["coef"][i], e, inp["x"], inp["hist"], noise, form == "third")
    if wrong == "mask indexing":                                          # the mask indexed per channel: element i of the flat mask
        flat = inp["mask"].reshape(-1)                                    # ... read as [B][4][h][w]; behind the mask lies other data
        behind = torch.rand(B * 4 * h * w - flat.numel(), generator=torch.Generator().manual_seed(77))
        m = torch.cat([flat, behind]).reshape(B, 4, h, w).double()
        p = float(row[0]) * image.double() + float(row[1]) * bnoise.double()
        return e, (1 - m) * p + m * xn, hist
    if wrong == "mask batch":
        mask = mask[:1].expand_as(mask)
    if wrong == "table columns":
        row = row.flip(0)
    if wrong == "table row":                                              # the row of the step's own timestep, one row early
        row = inp["blend_table"][i - 1]
    return e, blend(xn, image, bnoise, mask, row), hist


WRONG_LAUNCHES = ("mask indexing", "mask batch", "table columns", "table row", "blend order")


def step_power(inp, form, single):
    """{wrong launch: share of the blended latent elements on which its float64 result lies outside STEP_BAR of the true one}.  "blend
    order" exists only where the step has a noise term; "mask batch" is measured on the images behind the first."""
    _, ref, _ = step_reference(inp, form, single)
    bar = STEP_BAR * ref.abs().max()
    out = {}
    for wrong in WRONG_LAUNCHES:
        if wrong == "blend order" and inp["noise"] is None:
            continue
        off = (step_reference(inp, form, single, wrong)[1] - ref).abs() > bar
        out[wrong] = float((off[1:] if wrong == "mask batch" else off).double().mean())
    return out
