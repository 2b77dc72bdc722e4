"""Full-size (SD-1.5 / BlobNet, 512x512 canvas 64x128) parity of ONE denoise step against the CPU oracle on the same
seeded synthetic weights and inputs: the BASELINE.json tolerance (PSNR >= 40 dB, max-abs <= 1e-2 of the tensor scale) at the
benchmark's own problem size.  ~1 minute of host CPU time for the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.common import g, psnr  # noqa: E402


@pytest.fixture(scope="module")
def full():
    import bench
    from oracle.nets import NetConfig
    usd, bsd = bench.synth_weights()
    ucfg, bcfg = bench.full_configs()
    return dict(usd=usd, bsd=bsd, ucfg=ucfg, bcfg=bcfg, oucfg=NetConfig(in_channels=5, cross_attention_dim=768),
                obcfg=NetConfig(in_channels=1029, cross_attention_dim=None))


def test_full_size_blobnet_and_unet_step(full):
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from oracle.nets import blobnet_forward, unet_forward
    torch.set_num_threads(min(32, len(__import__("os").sched_getaffinity(0))))
    h, w = 64, 128
    t = torch.tensor(601)
    # ---- BlobNet at batch 1 (how the engine runs it) ----
    xb = torch.cat([g(1, 1, 4, h, w), g(2, 1, 1, h, w).abs().clamp(max=1), g(3, 1, 1024, h, w) * 0.3], 1)
    blobnet = BlobNetModel(full["bsd"], full["bcfg"])
    down, mid, up = blobnet(xb.cuda(), t, conditioning_scale=1.0, return_dict=False)
    rd, rm, ru = blobnet_forward(full["bsd"], full["obcfg"], xb, t, 1.0)
    worst = 0.0
    for a, b in list(zip(down, rd)) + [(mid, rm)] + list(zip(up, ru)):
        a, b = a.float().cpu().numpy(), b.numpy()
        scale = max(np.abs(b).max(), 1e-6)
        worst = max(worst, np.abs(a - b).max() / scale)
        assert psnr(a, b) > 40.0
    assert worst < 1e-2, f"BlobNet residual max-abs/scale {worst:.3e}"
    # ---- UNet at CFG batch 2 with the ORACLE's residuals (isolates the UNet) ----
    xu = g(4, 2, 5, h, w)
    ehs = g(5, 2, 77, 768)
    sq = lambda r: r[..., -r.shape[-2]:].contiguous()
    rd2 = [sq(r).repeat(2, 1, 1, 1) for r in rd]
    rm2 = sq(rm).repeat(2, 1, 1, 1)
    ru2 = [sq(r).repeat(2, 1, 1, 1) for r in ru]
    ref = unet_forward(full["usd"], full["oucfg"], xu, t, ehs, rd2, rm2, ru2).numpy()
    unet = UNet2DConditionModel(full["usd"], full["ucfg"])
    eps = unet(xu.cuda(), t, encoder_hidden_states=ehs.cuda(), down_block_add_samples=[r.cuda() for r in rd2],
               mid_block_add_sample=rm2.cuda(), up_block_add_samples=[r.cuda() for r in ru2], return_dict=False)[0]
    eps = eps.float().cpu().numpy()
    err = np.abs(eps - ref).max() / np.abs(ref).max()
    print(f"full-size UNet eps: max-abs/scale {err:.3e}, PSNR {psnr(eps, ref):.1f} dB; BlobNet residuals worst {worst:.3e}")
    assert err < 1e-2 and psnr(eps, ref) > 40.0


def _step_vs_oracle(full, h, w, requests, tag):
    """One BlobNet forward at batch `requests` and one UNet forward at the CFG batch 2 x requests (with the ORACLE's residuals: isolates the
    UNet) on an h x w canvas through the modules, against oracle.nets: all 28 BlobNet residuals and the UNet's eps at the BASELINE.json bar."""
    import os
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from oracle.nets import blobnet_forward, unet_forward
    torch.set_num_threads(min(32, len(os.sched_getaffinity(0))))
    n = requests
    t = torch.tensor(601)
    xb = torch.cat([g(11, n, 4, h, w), g(12, n, 1, h, w).abs().clamp(max=1), g(13, n, 1024, h, w) * 0.3], 1)
    blobnet = BlobNetModel(full["bsd"], full["bcfg"])
    down, mid, up = blobnet(xb.cuda(), t, conditioning_scale=1.0, return_dict=False)
    rd, rm, ru = blobnet_forward(full["bsd"], full["obcfg"], xb, t, 1.0)
    assert len(down) + 1 + len(up) == len(rd) + 1 + len(ru) == 28
    worst, worst_db = 0.0, 1e9
    for a, b in list(zip(down, rd)) + [(mid, rm)] + list(zip(up, ru)):
        a, b = a.float().cpu().numpy(), b.numpy()
        assert a.shape == b.shape
        worst = max(worst, np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))
        worst_db = min(worst_db, psnr(a, b))
    del blobnet
    xu = g(14, 2 * n, 5, h, w)
    ehs = g(15, 2 * n, 77, 768)
    sq = lambda r: r[..., -r.shape[-2]:].contiguous()          # (the slice the pipeline passes: the right-hand H columns of the canvas)
    rd2 = [sq(r).repeat(2, 1, 1, 1) for r in rd]
    rm2 = sq(rm).repeat(2, 1, 1, 1)
    ru2 = [sq(r).repeat(2, 1, 1, 1) for r in ru]
    ref = unet_forward(full["usd"], full["oucfg"], xu, t, ehs, rd2, rm2, ru2).numpy()
    unet = UNet2DConditionModel(full["usd"], full["ucfg"])
    eps = unet(xu.cuda(), t, encoder_hidden_states=ehs.cuda(), down_block_add_samples=[r.cuda() for r in rd2],
               mid_block_add_sample=rm2.cuda(), up_block_add_samples=[r.cuda() for r in ru2], return_dict=False)[0]
    eps = eps.float().cpu().numpy()
    err = np.abs(eps - ref).max() / np.abs(ref).max()
    print(f"full-size step {tag}: UNet eps max-abs/scale {err:.3e}, PSNR {psnr(eps, ref):.1f} dB; BlobNet residuals worst {worst:.3e}, {worst_db:.1f} dB")
    assert worst < 1e-2 and worst_db > 40.0, f"{tag}: BlobNet residuals max-abs/scale {worst:.3e}, PSNR {worst_db:.1f} dB"
    assert err < 1e-2 and psnr(eps, ref) > 40.0, f"{tag}: UNet eps {err:.3e} / {psnr(eps, ref):.1f} dB"


def test_full_size_step_576x448(full):
    """A 576 x 448 edit: canvas 72 x 112 (9 x 7 convolution tiles), then 36 x 56, 18 x 28 and 9 x 14 - maps on which every fused family is
    ineligible and the fallback launch list runs at 640 and 1280 channels.  The oracle costs what the 512 x 512 step above costs (the same
    pixel count to 2 %)."""
    _step_vs_oracle(full, 72, 112, 1, "576x448")


def test_full_size_step_520x520(full):
    """A 520 x 520 edit: canvas 65 x 130, then 33 x 65, 17 x 33 and 9 x 17 - odd maps at every level, explicit-size upsamples and skips at
    full width.  The oracle costs what the 512 x 512 step above costs."""
    _step_vs_oracle(full, 65, 130, 1, "520x520")


def test_full_size_step_512x512_request_batch_3(full):
    """512 x 512 at request batch 3: BlobNet at B = 3, the UNet at B = 6 - an odd batch between the sizes the other tests run (1, 2, 4, 8).
    The oracle runs three BlobNet and six UNet images: about five times the cost of the one-minute 512 x 512 case above on a host where that
    one takes its minute (measured on one 32-thread box: 20 s against 9 s)."""
    _step_vs_oracle(full, 64, 128, 3, "512x512 x3")


def test_full_size_two_step_loop_vs_oracle(full):
    """The north-star bar at the benchmark's own size: final latents of a (2-step, DDIM, CFG 7.5) 512x512 edit through the
    hipGraph-replayed engine vs the CPU oracle loop on the same seeded weights and inputs: PSNR >= 40 dB, max-abs <= 1e-2 of the
    latent scale.  ~1.5 minutes of host CPU time (the oracle runs BlobNet on both CFG halves like the reference does)."""
    import os
    import bench
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    from oracle import pipeline as o_pipe, schedulers as o_sched
    torch.set_num_threads(min(32, len(os.sched_getaffinity(0))))
    h = w = 64
    inp = bench.synth_inputs(h, w, batch=1)
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device="cuda:0")
    pipe = BlobCtrlEngine(full["usd"], full["bsd"], full["ucfg"], full["bcfg"], device="cuda:0", scheduler="ddim")
    out = pipe(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=2, guidance_scale=7.5,
               latents=inp["latents"]).cpu().numpy()
    ref = o_pipe.denoise_loop(full["usd"], full["oucfg"], full["bsd"], full["obcfg"], o_sched.DDIMOracle(), 2, inp["latents"],
                              inp["prompt"], inp["fg"], inp["bg"], score.cpu().float(), inp["dino"], 7.5, 1.0, 0.0, 1.0).numpy()
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"full-size 2-step loop: final latents max-abs/scale {err:.3e}, PSNR {psnr(out, ref):.1f} dB")
    assert err < 1e-2 and psnr(out, ref) > 40.0


@pytest.mark.parametrize("batch", [1, 2])
def test_cfg_invariant_prefix_equals_the_plain_plan(full, batch, monkeypatch):
    """Round 6: conv_in, the residual add, down_blocks.0.resnets.0 and the head of down_blocks.0.attentions.0 up to its self-attention
    run once per CFG image pair (engine.cfg_prefix_ok; the two images are identical until the prompt enters at attn2).  One denoise step
    through the plan with and without it: the UNet's eps of EVERY image agrees to fp16 rounding (measured 2e-3 of scale; not bit for bit:
    at half the batch the planner picks other tiles for conv_in, whose workgroups round their fp32 GroupNorm partial sums over other row
    counts - the last bits of the statistics differ), the plan really is the shorter one (123.5 GFLOP per image pair and step less, one
    bc_dup_halves launch), and the loop fixtures of the REAL reference (test_fullsize_loop_gpu.py) run through the prefix by default."""
    import bench
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    h = w = 64
    inp = bench.synth_inputs(h, w, batch=batch)
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device="cuda:0")
    eps, lat, flops, kinds = [], [], [], []
    for plain in (False, True):
        if plain:
            monkeypatch.setenv("BC_PLAN", "cfg_prefix=0")
        pipe = BlobCtrlEngine(full["usd"], full["bsd"], full["ucfg"], full["bcfg"], device="cuda:0", scheduler="ddim")
        out = pipe(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=1, guidance_scale=7.5, latents=inp["latents"])
        P = pipe.plan_for(batch, h, w, 77, 768, 1)
        torch.cuda.synchronize()
        eps.append(P.eps_active.float().cpu().view(2 * batch, -1))
        lat.append(out.float().cpu())
        flops.append((P.step_active.flops, P.step_inactive.flops))
        kinds.append(P.step_active.kinds.get("dup_halves", 0))
        del pipe
    assert torch.isfinite(eps[0]).all() and kinds == [1, 0]
    worst = 0.0
    for img in range(2 * batch):
        a, b = eps[0][img].numpy(), eps[1][img].numpy()
        worst = max(worst, np.abs(a - b).max() / np.abs(b).max())
        assert psnr(a, b) > 55.0
    err_lat = (lat[0] - lat[1]).abs().max().item() / lat[1].abs().max().item()
    saved = (flops[1][0] - flops[0][0]) / 1e9 / batch
    print(f"CFG-invariant prefix, batch {batch}: eps max-abs/scale vs the plain plan {worst:.3e}, latents after the step {err_lat:.3e}; "
          f"{saved:.1f} GFLOP per image pair and step less ({flops[1][0] / 1e12:.3f} -> {flops[0][0] / 1e12:.3f} TFLOP per active step)")
    assert worst < 5e-3 and err_lat < 5e-3
    assert 110.0 < saved < 140.0 and flops[1][1] - flops[0][1] == flops[1][0] - flops[0][0]
