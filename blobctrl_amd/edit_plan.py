"""One description of an edit plan, and the plan recorded from it.

`PlanSpec` names the switches of a plan; the cache key, the buffers and the step form are all read from it.  `EditPlan` is the recorded
plan: its buffers (allocated by the constructor, in the order the `.bcplan` buffer table has always had) and its three segments, which
`record_plan` fills - prologue, step_active (BlobNet + UNet), step_inactive (UNet only)."""
import os
from dataclasses import dataclass

import torch

from . import options
from .engine import IpAdapter, TrunkPlan
from .launch import Recorder
from .weights import ip_adapter_embed_dim, ip_adapter_tokens, pad8


def ip_key(entry, ad):
    """An adapter's part of a plan key: (image tokens per UNet image, width of its input[, tokens of a Plus adapter's hidden states])."""
    images, hidden = (entry[0], entry[1:]) if ad.get("layout") == "plus" else (entry, ())
    return (ip_adapter_tokens(ad) * images, ip_adapter_embed_dim(ad)) + tuple(hidden)


@dataclass(frozen=True)
class PlanSpec:
    """What tells one edit plan from another.  `denoise` and `compile_plan` take every one of these switches from the EditSetup of their
    call (`EditSetup.plan_spec`) and fill the tables with `_write_tables`; a call without lists never asks for `requests`.

    B, h, w, T, ctx_dim, nsteps: the batch, the latent canvas, the prompt tokens and their width, the loop length.  Every plan form owns
    `t_table` [nsteps], `coef` [nsteps][16] and `scale_table` [nsteps * Bi] unless a switch below says otherwise.
    per_request: the B samples are B independent edit requests (own fg / bg latents, scores, DINO features and conditioning scales) instead
    of B variations of one edit.
    stochastic: DDIM with eta > 0 or SDE-DPM-Solver++ - the plan owns the named buffer `variance_noise` [nsteps][B][4][h][w] and its steps
    end in bc_cfg_scheduler_step_noise (eta and the noise itself are per-call contents of the coefficient table and of that buffer, so one
    plan and its graphs serve every eta > 0 and every seed).
    third_order: a table with third-order DPM-Solver++ rows (column 13) - the steps end in bc_cfg_scheduler_step3.  Every other table
    (UniPC, DDIM, DPM-Solver++ of order 1 / 2) runs on the same plan: only the tables differ.  Not with `stochastic`.
    scaled: a table that scales the model input (Euler, Euler-ancestral, Heun: `scheduler.scale_model_input`, pipe:1032) - the BlobNet and
    UNet inputs are assembled by the `_scaled` entry points, which divide the noisy latents by column 14 of the current row.  A plan of its
    own (and with it graphs of its own): no other table ever replays these launches.
    single: a guidance-free (single-pass) plan, pipe:1031 / 1095 with do_classifier_free_guidance False: `ctx` holds the B positive
    prompts, the UNet runs once per request at batch B (no CFG pair, so no CFG-prefix sharing and no BC_SPLIT_CFG) and the step ends in
    bc_scheduler_step_single, which takes the right half of image b as eps.  BlobNet is what it is in every plan: batch B.
    freeu: FreeU is on (UNet2DConditionModel.enable_freeu) - every UNet forward runs bc_freeu in front of the six channel concats of
    up_blocks.0 / up_blocks.1, reading (s1, s2, b1, b2) from the named buffer `freeu` (fp32 [4], refilled per edit: one plan and its graphs
    serve every setting).  A plan of its own; BlobNet's up blocks never run it.
    requests: a request batch (per_request) whose requests run their OWN schedules - step count, guidance scale, control window, eta,
    timesteps.  The loop has nsteps = the longest request's evaluations; the plan owns `coef` [B][nsteps][16] (a table per request,
    finished rows marked in column 15), `t_rows_unet` [nsteps][Bu] / `t_rows_blob` [nsteps][B] (a timestep per step and image; no
    `t_table`) and `scale_table` [nsteps][B]; the time tables come from bc_timestep_embedding_rows, a scaling table assembles through the
    `_requests` entry points (a divisor per image) and both step segments end in bc_scheduler_step_requests.  The networks are what they
    are in every request batch.
    ip: images per loaded IP-Adapter (empty: none); an entry is (images, tokens of the hidden states) for an IP-Adapter Plus.  The plan owns
    the named buffers `ip_embeds<i>` (fp16 [UNet batch * images][embed dim], per-edit inputs like `ctx`); its prologue projects them to
    image tokens and to K_ip / V_ip per attn2 block, and every UNet forward runs one bc_attention_ip per adapter behind each attn2 (16 per
    adapter).  The key holds the adapter configuration - count, tokens each, embedding width - and never the scales, which the launches
    read from the adapters' device tables.  In-process only.
    ip_masked: the call brings `ip_adapter_masks` (only ever with `ip`) - every attn2 runs bc_attention_ip_masked in the place of
    bc_attention_ip (one softmax per image, weighted by that image's mask), and the plan owns one named fp16 buffer `ip_mask<i>_<rows>`
    [images][rows] per adapter and attention level, refilled per edit (ip_masks.fill_plan_masks).  A plan of its own; the key gains
    "masked" and the images per adapter, never the masks: another mask of the same shape replays the same plan and the same whole-edit
    graph.
    pag: perturbed-attention guidance - the sorted tuple of block prefixes ("mid_block.attentions.0.", ...) whose attn1 is perturbed
    (pag.resolve_layers).  The UNet runs B more images, the perturbed ones, behind the others: [uncond | cond | perturbed] (3B), or with
    `single` [cond | perturbed] (2B); `ctx`, `timestep_cond` and every `ip_embeds<i>` are sized for that batch and the last chunk is
    filled with a copy of the cond chunk.  In the named blocks bc_attention runs on the images in front and bc_attention_identity gives
    the perturbed ones their own V; both step segments end in bc_pag_scheduler_step, which reads the scale of the step from the named
    buffer `pag_table` (fp32 [nsteps], refilled per edit).  The key holds the prefixes and never the scales: another pag_scale or
    pag_adaptive_scale replays the same plan and the same whole-edit graph.  No CFG-prefix sharing (it pairs images b and b + Bu / 2) and
    no BC_SPLIT_CFG; not with `requests`.  In-process only.
    blend: a masked edit (pipeline_stable_diffusion_inpaint.py:1272-1285) - after every step the latents outside a mask are the original
    image's latents noised to the next timestep.  The plan owns the named buffers `blend_image` / `blend_noise` [B][4][h][w], `blend_mask`
    [B][h][w] and `blend_table` [nsteps][2] (all fp32, refilled per edit), and both step segments end in bc_blend_scheduler_step, which
    takes `pag_table` too (NULL where the plan has none) and serves every step form.  The key gains "blend" and never the mask or the
    image: another mask replays the same plan and the same whole-edit graph.  Not with `requests`.  In-process only.

    Read from those, once: Bi - images (fg / bg / score / feature sets) behind the batch.  Bu - images the UNet runs: the CFG pair of every
    sample, or the sample alone; with PAG the perturbed copy of the (conditional) sample behind them.  cfg_pairs - images b and b + Bu / 2
    of the UNet batch are the CFG pair of sample b (a PAG batch is no batch of pairs).  ip_images - images per adapter.  assemble_suffix -
    the form of the input-assembly entry points: `_scaled`, with (coef, step_idx, nsteps) in front of the output, when the table scales
    the model input; `_requests`: the same with a table, hence a divisor, per request."""
    B: int
    h: int
    w: int
    T: int
    ctx_dim: int
    nsteps: int
    per_request: bool = False
    stochastic: bool = False
    third_order: bool = False
    scaled: bool = False
    single: bool = False
    freeu: bool = False
    requests: bool = False
    ip: tuple = ()
    ip_masked: bool = False
    pag: tuple = ()
    blend: bool = False

    def __post_init__(self):
        put = lambda name, v: object.__setattr__(self, name, v)
        for name in ("per_request", "stochastic", "third_order", "scaled", "single", "freeu", "requests", "blend"):
            put(name, bool(getattr(self, name)))
        put("ip", tuple(self.ip or ()))
        put("ip_masked", bool(self.ip and self.ip_masked))
        put("pag", tuple(self.pag or ()))
        put("Bi", self.B if self.per_request else 1)
        put("Bu", (self.B if self.single else 2 * self.B) + (self.B if self.pag else 0))
        put("cfg_pairs", not self.single and not self.pag)
        put("ip_images", tuple(e if isinstance(e, int) else e[0] for e in self.ip))
        put("assemble_suffix", ("_requests" if self.requests else "_scaled") if self.scaled else "")

    def validate(self):
        if self.requests and not self.per_request:
            raise ValueError("per-request schedules need a request batch (per_request)")
        if self.pag and self.requests:
            raise NotImplementedError("perturbed-attention guidance with per-request schedules: bc_pag_scheduler_step reads ONE coefficient "
                                      "table and ONE pag_table; run the requests with shared steps, guidance scale, window and eta")
        if self.blend and self.requests:
            raise NotImplementedError("a masked edit (blend) with per-request schedules: bc_blend_scheduler_step reads ONE coefficient "
                                      "table and ONE blend_table; run the requests with shared steps, guidance scale, window and eta")
        if self.stochastic and self.third_order:
            raise NotImplementedError("a third-order step has no noise term (the reference's third-order update has no SDE branch)")

    def key(self, adapters=()):
        """What the engine caches the plan under; `adapters`: the engine's loaded IP-Adapters.  `set_ip_adapters` finds the plans that go
        with an adapter by their ("ip", ...) entries."""
        switches = (("step3", self.third_order), ("scaled", self.scaled), ("single", self.single), ("freeu", self.freeu), ("requests", self.requests))
        ip = (("ip", len(self.ip)) + tuple(ip_key(entry, ad) for entry, ad in zip(self.ip, adapters)),) if self.ip else ()
        masked = (("ip", "masked") + self.ip_images,) if self.ip_masked else ()
        pag = (("pag",) + self.pag,) if self.pag else ()
        return (self.B, self.h, self.w, self.T, self.ctx_dim, self.nsteps, self.per_request, self.stochastic) + \
            tuple(name for name, on in switches if on) + ip + masked + pag + (("blend",) if self.blend else ())

    def step_call(self):
        """The entry point a step segment ends in, and what it takes around (B, h, w): (name, arguments between `hist` and `B`, arguments
        between `w` and `eps_out`); a string names a buffer of the plan (NULL where the plan does not own it).  The first row that applies:
        the blend, PAG, requests and single entry points each serve every step form - noise (or NULL), nsteps, third[, single]."""
        forms = ("variance_noise", self.nsteps, int(self.third_order), int(self.single))
        blend = ("pag_table", "blend_image", "blend_noise", "blend_mask", "blend_table")
        calls = ((self.blend, "bc_blend_scheduler_step", blend, forms), (self.pag, "bc_pag_scheduler_step", ("pag_table",), forms), (self.requests, "bc_scheduler_step_requests", (), forms),
                 (self.single, "bc_scheduler_step_single", (), forms[:3]), (self.stochastic, "bc_cfg_scheduler_step_noise", (-1.0,), forms[:2]),
                 (self.third_order, "bc_cfg_scheduler_step3", (-1.0,), (self.nsteps,)), (True, "bc_cfg_scheduler_step", (-1.0,), ()))
        return next(tuple(call) for on, *call in calls if on)


class EditPlan:
    """The launch plan of one PlanSpec.  The constructor allocates the buffers; an attribute is None where the form does not own it."""

    def __init__(self, spec, eng):
        s, f32, rec = spec, torch.float32, Recorder(eng.device)
        self.spec, self.rec = spec, rec
        self.single, self.stochastic, self.third_order, self.scaled, self.requests = s.single, s.stochastic, s.third_order, s.scaled, s.requests
        self.Bi, self.pag, self.ip_masked, self.feat_dim = s.Bi, s.pag, s.ip_masked, eng.feat_dim
        B, Bi, Bu, h, w, n, F = s.B, s.Bi, s.Bu, s.h, s.w, s.nsteps, eng.feat_dim
        self.latents = rec.zeros(B, 4, h, w, dtype=f32, name="latents")
        self.fg_lat, self.bg_lat = (rec.zeros(Bi, 4, h, w, dtype=f32, name=name) for name in ("fg_lat", "bg_lat"))
        self.fg_score, self.bg_score = (rec.zeros(Bi, h, w, dtype=f32, name=name) for name in ("fg_score", "bg_score"))
        self.feat = rec.zeros(Bi, max(F, 1), dtype=f32, name="feat")
        self.pag_table = rec.zeros(n, dtype=f32, name="pag_table") if s.pag else None
        self.ctx = rec.zeros(Bu, s.T, s.ctx_dim, name="ctx")
        # a UNet with time_cond_proj_dim (a distilled LCM UNet): the guidance-scale embedding of every UNet image, replay-time data like
        # the guidance scale itself - zero when the caller gives none (cond_proj has no bias: the add is then + 0)
        cond_dim = eng.unet_cfg.time_cond_proj_dim
        self.timestep_cond = None if cond_dim is None else rec.zeros(Bu, pad8(cond_dim), name="timestep_cond")
        self.step_idx = rec.zeros(1, dtype=torch.int32, name="step_idx")
        self.t_rows_unet = rec.zeros(n, Bu, dtype=f32, name="t_rows_unet") if s.requests else None
        self.t_rows_blob = rec.zeros(n, B, dtype=f32, name="t_rows_blob") if s.requests else None
        self.t_table = None if s.requests else rec.zeros(n, dtype=f32, name="t_table")
        self.coef = rec.zeros(*((B,) if s.requests else ()), n, 16, dtype=f32, name="coef")
        self.scale_table = rec.zeros(n * Bi, dtype=f32, name="scale_table")   # [step][image] conditioning_scale * keep
        self.hist = rec.zeros(3, B * 4 * h * w, dtype=f32, name="hist")
        self.eps_guided = rec.zeros(B, 4, h, w, dtype=f32, name="eps_guided")
        self.variance_noise = rec.zeros(n, B, 4, h, w, dtype=f32, name="variance_noise") if s.stochastic else None
        self.freeu = rec.zeros(4, dtype=f32, name="freeu") if s.freeu else None
        self.blend_image, self.blend_noise = (rec.zeros(B, 4, h, w, dtype=f32, name=name) if s.blend else None for name in ("blend_image", "blend_noise"))
        self.blend_mask = rec.zeros(B, h, w, dtype=f32, name="blend_mask") if s.blend else None
        self.blend_table = rec.zeros(n, 2, dtype=f32, name="blend_table") if s.blend else None
        # rank-1 collapse of the BlobNet feature channels (per-edit weight; round 6: per-IMAGE weights for a batch of independent requests -
        # conv_in then runs as one launch per image, engine.record_collapse)
        self.collapse = F > 3 and "conv_in.featmat" in eng.blob_w.h
        unet_cin = pad8(eng.unet_cfg.in_channels)
        # 8-channel inputs (the UNet's 4 latents + score; BlobNet's rank-1-collapsed 4 latents + 2 x score) are assembled directly as
        # the 3x3 im2col operand [rows][128] of conv_in, which then runs as a dense GEMM on the LDS-DMA fast path (K = 72 does not)
        self.unet_im2col, self.blob_im2col = unet_cin == 8, self.collapse
        self.feat16 = rec.zeros(Bi, pad8(max(F, 1)), name="feat16")
        self.blob_in = rec.zeros(B, h * 2 * w, 128 if self.blob_im2col else pad8(eng.blob_cfg.in_channels))
        self.unet_in = rec.zeros(Bu, h * 2 * w, 128 if self.unet_im2col else unet_cin)
        # what recording fills in: the segments, the BlobNet residuals and the UNet outputs of the two step segments, the adapters' inputs
        self.prologue = self.step_active = self.step_inactive = self.residuals = self.eps_active = self.eps_inactive = None
        self.ip_embeds, self.ip_adapters = [], []                # (the adapters' mask_bufs fill up as the UNet forwards are recorded)
        self.split_cfg, self.half_time, self.eps_all = False, None, None      # BC_SPLIT_CFG: the batch-B time table and both halves' eps
        self.guidance, self.loop_graphs, self.captured = [7.5], {}, False        # what replaying keeps: the last call's scale, its graphs
        self.options, self.options_non_default = options.effective(), options.non_default()     # (what BC_PLAN says while this plan is recorded)


def _record_prologue(P, eng):
    """Once per edit: prompt K / V (and the IP-Adapters' image side), the rank-1 collapse, the time-embedding path of every step (read in
    the step through the device step counter).  Returns the UNet and BlobNet forwards that own that state."""
    s, rec = P.spec, P.rec
    H, W = s.h, 2 * s.w
    P.prologue = rec.begin("prologue")
    unet = TrunkPlan(rec, eng.unet_w, eng.unet_cfg, s.Bu, H, W)
    unet.freeu_params, unet.pag_layers, unet.pag_images = P.freeu, frozenset(s.pag), s.B if s.pag else 0
    made = [IpAdapter.for_plan(rec, ad, s.Bu, entry, name=f"ip_embeds{i}", masked=s.ip_masked, mask_name=f"ip_mask{i}")
            for i, (entry, ad) in enumerate(zip(s.ip, eng.ip_adapters))]
    unet.ip_adapters = P.ip_adapters = [m[0] for m in made]
    P.ip_embeds = [m[1] for m in made]
    unet.record_context(P.ctx, s.T)
    blob = TrunkPlan(rec, eng.blob_w, eng.blob_cfg, s.B, H, W)
    if P.collapse:
        blob.record_collapse(P.feat16, per_image=s.B if s.per_request else 0)
    # (a timestep per step, or with `requests` per step and image; BlobNet never has a cond_proj: pipe:1063 passes no timestep_cond)
    unet.record_time_table(P.t_rows_unet if s.requests else P.t_table, s.nsteps, P.step_idx, cond=P.timestep_cond, per_image=s.requests)
    blob.record_time_table(P.t_rows_blob if s.requests else P.t_table, s.nsteps, P.step_idx, per_image=s.requests)
    # CFG halves on two streams (opt-in, BC_SPLIT_CFG=1; single edits only - larger batches fill the GPU with the batch-2B UNet)
    P.split_cfg = s.B == 1 and eng.two_streams and bool(os.environ.get("BC_SPLIT_CFG")) and s.cfg_pairs
    if P.split_cfg:
        # the uncond / cond halves of the UNet batch as two batch-B plans on their own streams (ids 0 and 2): more concurrent
        # kernels for a GPU that one batch-2 UNet does not fill, at the price of reading the UNet weights twice per step
        # (measured, same box, interleaved: 11.56 vs 11.73 ms per active step, +2-3 % edits/s; 1108 instead of 725 launches.
        #  Not the default: it trades per-kernel efficiency - every self-attention then runs at batch 1, the 64x64-tile GEMM
        #  becomes the largest kernel of the step - for concurrency, a gain inside the box-to-box spread)
        P.half_time = TrunkPlan(rec, eng.unet_w, eng.unet_cfg, s.B, H, W)
        P.half_time.record_time_table(P.t_table, s.nsteps, P.step_idx, cond=None if P.timestep_cond is None else P.timestep_cond[:s.B])
        P.eps_all = rec.zeros(2 * s.B, H * W, eng.unet_cfg.out_channels, dtype=torch.float32)
    return unet, blob


def _record_assemble(P, blobnet):
    """The input of a net from the latents and its image's latents and scores (BlobNet: the foreground's, and the DINO feature; the UNet:
    the background's), as conv_in's im2col operand where the net takes that."""
    s = P.spec
    lat, score, out, Bout, im2col = (P.fg_lat, P.fg_score, P.blob_in, s.B, P.blob_im2col) if blobnet else \
        (P.bg_lat, P.bg_score, P.unet_in, s.Bu, P.unet_im2col)
    front = (P.latents.data_ptr(), s.B, lat.data_ptr(), score.data_ptr())
    divisor = (P.coef.data_ptr(), P.step_idx.data_ptr(), s.nsteps) if s.scaled else ()
    if im2col:
        P.rec.call("bc_assemble_input_im2col" + s.assemble_suffix, *front, s.Bi, Bout, s.h, s.w, int(blobnet), *divisor, out.data_ptr(), kind="assemble")
    else:
        F = P.feat_dim if blobnet else 0
        P.rec.call("bc_assemble_input" + s.assemble_suffix, *front, P.feat.data_ptr() if F > 0 else None, s.Bi, F, Bout, s.h, s.w,
                   out.shape[-1], 0, *divisor, out.data_ptr(), kind="assemble")


def _record_blobnet(P, blob):
    """The BlobNet branch of an active step, recorded for the side stream: fork (side waits for the start of the step on main), every
    residual is signalled when its zero-conv finishes, the UNet waits right before the GEMM whose epilogue adds it."""
    s, rec = P.spec, P.rec
    fork = rec.new_event()
    rec.signal(fork)
    rec.sid = 1
    rec.wait(fork)
    _record_assemble(P, blobnet=True)
    residuals = blob.record_forward(P.blob_in, None, zero_scale=(1.0, P.scale_table, P.step_idx, s.B if s.per_request else 0),
                                    signal_residuals=True, im2col=P.blob_im2col)
    rec.sid = 0
    return residuals


def _record_split_cfg(P, unet, residuals):
    """The UNet forward as its two CFG halves, the cond half on stream 2; returns eps of both."""
    rec, B = P.rec, P.spec.B

    half = lambda b0: TrunkPlan(rec, unet.pw, unet.cfg, B, unet.H, unet.W).share_from(unet, images=(b0, b0 + B), time=P.half_time)
    ready, joined = rec.new_event(), rec.new_event()
    rec.signal(ready)                                   # unet_in assembled (stream 0)
    rec.sid = 2
    rec.wait(ready)
    half(B).record_forward(P.unet_in[B:], residuals, eps_out=P.eps_all[B:], im2col=P.unet_im2col)   # cond half
    rec.signal(joined)
    rec.sid = 0
    half(0).record_forward(P.unet_in[:B], residuals, eps_out=P.eps_all[:B], im2col=P.unet_im2col)   # uncond half
    rec.wait(joined)
    return P.eps_all


def _record_unet_step(P, unet, residuals):
    """Assemble the UNet input, run the UNet (adding `residuals`), guide and step: the rest of a step segment.  Returns eps."""
    s = P.spec
    _record_assemble(P, blobnet=False)
    eps = _record_split_cfg(P, unet, residuals) if P.split_cfg else \
        unet.record_forward(P.unet_in, residuals, im2col=P.unet_im2col, cfg_pairs=s.cfg_pairs)
    name, head, tail = s.step_call()
    held = lambda args: [getattr(P, a) if isinstance(a, str) else a for a in args]
    P.rec.call(name, eps, P.latents, P.coef, P.step_idx, P.hist, *held(head), s.B, s.h, s.w, *held(tail), P.eps_guided, 1, kind="cfg_step")
    return eps


def record_plan(eng, spec):
    """The plan of `spec` on the engine's weights: buffers, prologue, step A (BlobNet + UNet) and step I (UNet only: cond_scale == 0, the
    BlobNet output is multiplied by 0, bn:936-938)."""
    P = EditPlan(spec, eng)
    unet, blob = _record_prologue(P, eng)
    P.step_active = P.rec.begin("step_active")
    P.residuals = _record_blobnet(P, blob)
    P.eps_active = _record_unet_step(P, unet, P.residuals)
    P.step_inactive = P.rec.begin("step_inactive")
    P.eps_inactive = _record_unet_step(P, TrunkPlan(P.rec, unet.pw, unet.cfg, unet.B, unet.H, unet.W).share_from(unet), None)
    return P
