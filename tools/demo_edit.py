#!/usr/bin/env python3
"""End-to-end edit on the HIP path, the stages of scripts/blobctrl_inference.py in order (inf:112-205):
   ellipse -> splat scores | fg crop -> DINOv2 pooled feature | prompt ids -> CLIP embeddings | fg/bg images -> VAE latents
   -> 50-step blob-conditioned denoise loop -> VAE decode -> image.
With --models DIR it loads the released layout (README.md:115-128: DIR/stable-diffusion-v1-5/{unet,vae,text_encoder},
DIR/blobnet, DIR/unet_lora, DIR/dinov2-large); without it, seeded synthetic weights of the same architectures are used (no
checkpoints exist offline), which exercises every kernel and prints per-stage timings but produces noise, not a picture.
With --sam DIR_OR_PTH --click X,Y the edit starts where the app's does: Segment-Anything turns the click on the foreground image into a
mask and the mask into the blob's ellipse (DIR = a transformers directory, PTH = the original sam_vit_h_4b8939.pth, "synth" = seeded
synthetic ViT-H weights).  With --sam ... --sam-auto K there is no click: SamAutomaticMaskGenerator segments everything in the image and
the K-th largest mask gives the blob.  With --sam ... --click X,Y --device-inputs the image is uploaded once and neither it nor the mask
leaves the GPU: `set_image(device tensor)` (`resample.sam_pixel_values`) -> `predict_torch` -> `masks.clean_masks` ->
`edit_inputs.ellipses_from_masks` (the row extents come to the host, n * H * 8 bytes) -> `object_regions` / `build_edit_inputs_batch` ->
`vae_input`, DINOv2's input from `resample.dinov2_pixel_values`, and the edit is a "move" of the clicked object.
With --ip-adapter PATH --ip-image FILE the edit takes an image prompt: PATH is a local IP-Adapter .safetensors file (base or Plus) with its
CLIP vision tower in the folder `image_encoder` beside it; the image goes through CLIPImageProcessor, the tower
(blobctrl_amd.clip_vision) and - for a Plus adapter - the Resampler in the plan's prologue, and every attn2 runs bc_attention_ip on its
tokens.  --ip-adapter synth uses a seeded tiny tower (320 wide, 4 layers) and a seeded Plus adapter of 16 queries; without --ip-image the
image is seeded noise.
With --ip-adapter ... --ip-mask blob|FILE the image prompt is confined to a region (cross_attention_kwargs["ip_adapter_masks"] of the
reference): `blob` is the edit's own target ellipse, filled on the device (edit_inputs.ellipse_masks); FILE is a mask image of the frame.
Either goes through IPAdapterMaskProcessor.preprocess and ip_masks.canvas_masks (the UNet's canvas is the background frame beside the
edited one), and every attn2 runs bc_attention_ip_masked on the mask downsampled to its level.
With --device-inputs --zoom PAD the edit is a zoomed ("only masked") one (blobctrl_amd.overlay): the box around the start and
target ellipses, padded by PAD and grown to the frame's ratio, is blown up to the model's resolution (`zoom_edit`), the model edits that
frame, and the result is pasted back over the original through the ellipses' mask blurred with --blur F (`blur`, `apply_overlay`) - all
on the device; pixels outside the blurred mask keep the original's bytes.
With --pag-scale S [--pag-layers mid,up_blocks.1] [--pag-adaptive-scale A] the edit runs perturbed-attention guidance (blobctrl_amd.pag): the
UNet takes a third copy of the sample whose self-attention in the named layers is the identity on V, and eps gains S (eps_cond - eps_perturbed).
With --device-inputs --keep-background the edit is a masked one (include/blobctrl_blend.h): `edit_inputs.edit_region_masks` builds the union
of the start and target ellipses on the device, and after every step the latents outside it are the untouched frame's, noised to that step."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def image_prompt(args, pipe, unet_keys):
    """--ip-adapter / --ip-image: load the adapter into the engine, encode the image with the CLIP vision tower and return the keyword
    the engine's call takes: `ip_adapter_image_embeds` = [[negative, positive]] - hidden_states[-2] of the image and of an all-zero image
    for a Plus adapter, image_embeds and zeros for a base one."""
    from blobctrl_amd import synth
    from blobctrl_amd.checkpoint import load_ip_adapter
    from blobctrl_amd.clip_vision import CLIPVisionModelWithProjection
    from blobctrl_amd.image_processor import CLIPImageProcessor
    from blobctrl_amd.weights import convert_ip_adapter, ip_adapter_on_device, ip_attn2_prefixes
    prefixes = ip_attn2_prefixes(unet_keys)
    ctx = pipe.unet_cfg.cross_attention_dim
    if args.ip_adapter == "synth":
        sys.path.insert(0, os.path.join(REPO, "tools"))
        from ip_adapter_probe import plus_adapter_shapes
        D, L, n = 320, 4, (224 // 14) ** 2 + 1
        shapes = {"vision_model.embeddings.class_embedding": (D,), "vision_model.embeddings.patch_embedding.weight": (D, 3, 14, 14),
                  "vision_model.embeddings.position_embedding.weight": (n, D), "vision_model.pre_layrnorm.weight": (D,),
                  "vision_model.pre_layrnorm.bias": (D,), "vision_model.post_layernorm.weight": (D,), "vision_model.post_layernorm.bias": (D,),
                  "visual_projection.weight": (1024, D)}
        for i in range(L):
            q = f"vision_model.encoder.layers.{i}."
            for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
                shapes[q + f"self_attn.{m}.weight"], shapes[q + f"self_attn.{m}.bias"] = (D, D), (D,)
            shapes.update({q + "layer_norm1.weight": (D,), q + "layer_norm1.bias": (D,), q + "layer_norm2.weight": (D,), q + "layer_norm2.bias": (D,),
                           q + "mlp.fc1.weight": (4 * D, D), q + "mlp.fc1.bias": (4 * D,), q + "mlp.fc2.weight": (D, 4 * D), q + "mlp.fc2.bias": (D,)})
        tower = CLIPVisionModelWithProjection(synth.synth_state_dict(shapes, 171), num_heads=4, hidden_act="gelu")
        kv = {f"{1 + 2 * j}.to_{m}_ip.weight": (c, ctx) for j, c in enumerate(pipe.unet_w.h[bp + "attn2.to_k.weight"].shape[0] for bp in prefixes)
              for m in "kv"}
        sd = {"image_proj": dict(synth.synth_state_dict(plus_adapter_shapes(embed=D, hidden=256, ctx=ctx), 172)),
              "ip_adapter": dict(synth.synth_state_dict(kv, 173))}
    else:
        (sd,) = load_ip_adapter(args.ip_adapter)
        tower = CLIPVisionModelWithProjection.from_pretrained(os.path.dirname(os.path.abspath(args.ip_adapter)), subfolder="image_encoder")
    adapter = ip_adapter_on_device(convert_ip_adapter(sd, prefixes, ctx), pipe.device)
    pipe.set_ip_adapters([adapter])
    size = tower.config.image_size
    if args.ip_image:
        from PIL import Image
        image = Image.open(args.ip_image)
    else:
        image = np.random.Generator(np.random.PCG64(7)).integers(0, 256, (300, 400, 3), dtype=np.uint8)
    px = CLIPImageProcessor(size=size, crop_size=size)(image, return_tensors="pt").pixel_values
    plus = adapter.get("layout") == "plus"
    if plus:
        pos = tower(px, output_hidden_states=True).hidden_states[-2]
        neg = tower(torch.zeros_like(px), output_hidden_states=True).hidden_states[-2]
    else:
        pos = tower(px).image_embeds
        neg = torch.zeros_like(pos)
    embeds = torch.stack([neg, pos], 0).reshape(2, 1, *pos.shape[1:])
    print(f"image prompt: {'Plus' if plus else 'base'} adapter, tower {tower.L} layers x {tower.D}, embeds {tuple(embeds.shape)}")
    return dict(ip_adapter_image_embeds=[embeds])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--out", default=None, help="write the edited image as a .npy [H,W,3] float array")
    ap.add_argument("--sam", default=None, help="SAM weights: a transformers directory, the original .pth, or 'synth'")
    ap.add_argument("--click", default=None, help="X,Y pixel of the click on the foreground image (with --sam)")
    ap.add_argument("--sam-auto", type=int, default=None, metavar="K",
                    help="take the blob from the K-th largest mask of SamAutomaticMaskGenerator instead of a click (with --sam)")
    ap.add_argument("--min-region-area", type=int, default=0, metavar="N",
                    help="despeckle the SAM mask(s) on the GPU first: fill holes and remove islands of fewer than N pixels (with --sam)")
    ap.add_argument("--device-inputs", action="store_true",
                    help="build the edit's inputs on the GPU from the device mask (with --sam, click prompts): blobctrl_amd.edit_inputs")
    ap.add_argument("--zoom", type=int, default=None, metavar="PAD",
                    help="edit only the box around the blobs, padded by PAD pixels, at full model resolution, and paste it back (with --device-inputs)")
    ap.add_argument("--blur", type=float, default=4, metavar="F", help="blur factor of the paste-back mask (with --zoom; the reference's default 4)")
    ap.add_argument("--ip-adapter", default=None, help="an IP-Adapter .safetensors file with `image_encoder/` beside it, or 'synth'")
    ap.add_argument("--ip-image", default=None, help="the image prompt (any file PIL opens); seeded noise without it")
    ap.add_argument("--ip-mask", default=None, metavar="blob|FILE",
                    help="confine the image prompt (with --ip-adapter): 'blob' = the edit's target ellipse, or a mask image of the frame")
    ap.add_argument("--keep-background", action="store_true",
                    help="a masked edit (with --device-inputs): only the start and target ellipses are repainted, the rest keeps the input")
    ap.add_argument("--pag-scale", type=float, default=0.0, metavar="S", help="perturbed-attention guidance scale (0 = off; the PAG pipelines use 3.0)")
    ap.add_argument("--pag-layers", default="mid", metavar="IDS", help="comma-separated layer ids as diffusers' set_pag_applied_layers takes them (with --pag-scale)")
    ap.add_argument("--pag-adaptive-scale", type=float, default=0.0, metavar="A", help="the scale falls by A per timestep below 1000 (with --pag-scale)")
    ap.add_argument("--preview-vae", default=None, metavar="PATH|synth", help="a TAESD folder (config.json + diffusion_pytorch_model.safetensors), or 'synth'")
    ap.add_argument("--preview-every", type=int, default=5, metavar="N", help="preview every N-th step (with --preview-vae)")
    ap.add_argument("--preview-dir", default="previews", metavar="DIR", help="where the step_<i>.png files go (with --preview-vae)")
    args = ap.parse_args()
    if args.preview_vae and args.preview_every < 1:
        ap.error("--preview-every needs N >= 1")
    if args.ip_image and not args.ip_adapter:
        ap.error("--ip-image needs --ip-adapter")
    if args.ip_mask and not args.ip_adapter:
        ap.error("--ip-mask needs --ip-adapter")
    if args.device_inputs and (not args.sam or args.sam_auto is not None):
        ap.error("--device-inputs needs --sam and a click prompt")
    if args.zoom is not None and not args.device_inputs:
        ap.error("--zoom needs --device-inputs")
    if args.keep_background and not args.device_inputs:
        ap.error("--keep-background needs --device-inputs (the mask is built from the edit's ellipses on the device)")
    if (args.click or args.sam_auto is not None) and not args.sam:
        ap.error("--click / --sam-auto need --sam")
    if args.click and args.sam_auto is not None:
        ap.error("--click and --sam-auto exclude each other")
    import bench
    from blobctrl_amd import synth
    from blobctrl_amd.clip_text import CLIPTextModel
    from blobctrl_amd.dinov2 import Dinov2Model
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import blob_dict_from_ellipse, splat_features
    from blobctrl_amd.vae import AutoencoderKL

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    t0 = sync()
    if args.models:
        sd15 = os.path.join(args.models, "stable-diffusion-v1-5")
        unet = UNet2DConditionModel.from_pretrained(sd15, subfolder="unet", extra_in_channels=1, lora_path=os.path.join(args.models, "unet_lora"))
        blob = BlobNetModel.from_pretrained(os.path.join(args.models, "blobnet"))
        vae = AutoencoderKL.from_pretrained(sd15, subfolder="vae")
        clip = CLIPTextModel.from_pretrained(sd15, subfolder="text_encoder")
        dino = Dinov2Model.from_pretrained(os.path.join(args.models, "dinov2-large"))
        pipe = BlobCtrlEngine(unet.weights, blob.weights, unet.trunk_config, blob.trunk_config, scheduler="unipc", vae=vae,
                                              text_encoder=clip)
    else:
        ucfg, bcfg = bench.full_configs()
        usd, bsd = bench.synth_weights()
        vae = AutoencoderKL(synth.synth_state_dict(synth.vae_param_shapes(), 33))
        clip = CLIPTextModel(synth.synth_state_dict(synth.clip_text_param_shapes(), 88), num_heads=12)
        dino = Dinov2Model(synth.synth_state_dict(synth.dinov2_param_shapes(1024, 24, 4, 14, 37 * 37), 99), num_heads=16)
        pipe = BlobCtrlEngine(usd, bsd, ucfg, bcfg, scheduler="unipc", vae=vae, text_encoder=clip)
    ip_kwargs = {}
    if args.ip_adapter:
        ip_kwargs = image_prompt(args, pipe, unet._sd.keys() if args.models else usd.keys())
    t1 = sync()
    R = args.res
    rng = np.random.Generator(np.random.PCG64(0))
    fg = torch.from_numpy(rng.uniform(-1, 1, (1, 3, R, R)).astype(np.float32))
    bg = torch.from_numpy(rng.uniform(-1, 1, (1, 3, R, R)).astype(np.float32))
    s = R / 512.0
    ellipse = [[361.1067 * s, 367.8526 * s], [85.4812 * s, 103.6543 * s], 87.3739]            # the README's move_hat target blob
    if args.sam:
        from blobctrl_amd.blob_edit import ellipse_from_click
        from blobctrl_amd.sam import SamModel, SamPredictor
        if args.sam == "synth":
            sd = synth.synth_state_dict(synth.sam_param_shapes(), 131)
            sam = SamModel(sd)
        else:
            sam = SamModel.from_pretrained(args.sam) if os.path.isdir(args.sam) else SamModel.from_checkpoint(args.sam)
        image = ((fg[0].permute(1, 2, 0).numpy() + 1) * 127.5).round().clip(0, 255).astype(np.uint8)
        if args.sam_auto is not None:
            from blobctrl_amd.blob_edit import ellipses_from_image
            from blobctrl_amd.sam import SamAutomaticMaskGenerator
            # (seeded synthetic weights predict IoUs and stabilities far below the package's thresholds and masks that all span the frame:
            # keep every mask of a coarser grid then, or nothing would be left to choose from)
            kw = dict(points_per_side=8, pred_iou_thresh=-1e9, stability_score_thresh=0.0, box_nms_thresh=1.0) if args.sam == "synth" else {}
            ts = sync()
            blobs = ellipses_from_image(SamAutomaticMaskGenerator(sam, **kw), image, min_region_area=args.min_region_area)
            if not 0 <= args.sam_auto < len(blobs):
                raise SystemExit(f"--sam-auto {args.sam_auto}: the generator found {len(blobs)} masks")
            e, ann = blobs[args.sam_auto]
            print(f"SAM segment-everything: {len(blobs)} masks in {1e3 * (sync() - ts):.1f} ms (first call: planning + graph capture); mask "
                  f"{args.sam_auto}: area {ann['area']}, bbox {ann['bbox']}, predicted IoU {ann['predicted_iou']:.3f} -> ellipse {e}")
        elif args.device_inputs:
            from blobctrl_amd import edit_inputs, masks as bc_masks, resample
            from blobctrl_amd.image_processor import Dinov2ImageProcessor
            click = [float(v) for v in (args.click or f"{R // 2},{R // 2}").split(",")]
            image_dev = torch.from_numpy(image).cuda()        # the one upload: SAM, the cut-out and DINOv2 all read this tensor
            ts = sync()
            predictor = SamPredictor(sam)
            predictor.set_image(image_dev)
            pts = predictor.transform.apply_coords_torch(torch.tensor([[click]], dtype=torch.float32, device="cuda"), predictor.original_size)
            found, _, _ = predictor.predict_torch(pts, torch.ones(1, 1, dtype=torch.int32, device="cuda"), multimask_output=False)
            te = sync()
            clean, _, _ = bc_masks.clean_masks(found[:, 0], args.min_region_area)
            ells, boxes = edit_inputs.ellipses_from_masks(clean)
            if boxes[0] is None:
                raise SystemExit(f"--device-inputs: the mask of click {click} is empty")
            if ells[0] is None:                           # (seeded synthetic SAM weights give masks that span the frame: nothing to fit)
                print(f"no ellipse can be fitted to the mask of click {click} (box {boxes[0]}): the README's blob stands in for it")
                ells = [((ellipse[0][0], ellipse[0][1]), (ellipse[1][0], ellipse[1][1]), ellipse[2])]
            target =((ells[0][0][0] + 0.1 * R, ells[0][0][1]), ells[0][1], ells[0][2])          # the edit: move the object right
            fg_u8 = edit_inputs.object_regions(image_dev, clean, boxes)
            frame, start = image_dev, ells[0]
            # (the foreground stays what it was: the object cut out of the whole frame onto its own centred canvas, which is what DINOv2
            # describes whatever frame the edit runs in; the background and both ellipses move into the zoomed frame)
            if args.zoom is not None:                         # the model sees the padded box around both blobs at its full resolution
                from blobctrl_amd import overlay
                overlay.blur_params(args.blur)                # (an unsupported factor is refused here, not after the edit)
                zoom_crop, frame, zoom_mask, start, target = overlay.zoom_edit(image_dev, ells[0], target, R, R, args.zoom)
                print(f"zoom: box {zoom_crop} of the {R} x {R} frame edited at {R} x {R}")
            bg_u8, score, _ = edit_inputs.build_edit_inputs_batch(["move"], frame, [start], [target], [1.0])
            fg, bg = edit_inputs.vae_input(fg_u8), edit_inputs.vae_input(bg_u8)
            dino_px = resample.dinov2_pixel_values(fg_u8[0], Dinov2ImageProcessor())
            print(f"SAM click {click} -> device mask in {1e3 * (te - ts):.1f} ms (first call: planning + graph capture); mask -> ellipse {ells[0]}, "
                  f"box {boxes[0]}, fg / bg / score on the device in {1e3 * (sync() - te):.1f} ms")
            e = target
        else:
            click = [float(v) for v in (args.click or f"{R // 2},{R // 2}").split(",")]
            ts = sync()
            predictor = SamPredictor(sam)
            e = ellipse_from_click(predictor, image, [click], min_region_area=args.min_region_area)
            te = sync()
            e2 = ellipse_from_click(predictor, None, [click], min_region_area=args.min_region_area)
            print(f"SAM click {click} -> ellipse {e} in {1e3 * (te - ts):.1f} ms (first call: planning + graph capture); "
                  f"second click {1e3 * (sync() - te):.1f} ms, same ellipse: {e2 == e}")
        ellipse = [list(e[0]), list(e[1]), e[2]]
    if not args.device_inputs:
        score = splat_features(**blob_dict_from_ellipse(ellipse, R, R), score_size=(R // 8, R // 8), return_d_score=True)
    t2 = sync()
    crop = dino_px if args.device_inputs else torch.nn.functional.interpolate(fg, size=(224, 224), mode="bilinear", align_corners=False)
    feats = dino(crop).pooler_output.view(1, 1, -1)
    t3 = sync()
    ids = torch.from_numpy(rng.integers(0, 49408, size=(2, 1, 77)).astype(np.int64))
    prompt = pipe.encode_prompt(ids[1], ids[0])
    t4 = sync()
    if args.ip_mask:
        from blobctrl_amd import edit_inputs as ei, ip_masks
        from blobctrl_amd.image_processor import IPAdapterMaskProcessor
        if args.ip_mask == "blob":                            # the blob says where, the image prompt says what: uint8 255 / 0, on the device
            frame_mask = ei.ellipse_masks([(tuple(ellipse[0]), tuple(ellipse[1]), ellipse[2])], R, R)[0]
        else:
            from PIL import Image
            frame_mask = Image.open(args.ip_mask)
        m = IPAdapterMaskProcessor().preprocess(frame_mask, height=R, width=R)
        ip_kwargs["ip_adapter_masks"] = [ip_masks.canvas_masks(m.reshape(1, m.shape[0], m.shape[2], m.shape[3]))]
        print(f"--ip-mask {args.ip_mask}: {100 * float(m.float().mean()):.1f} % of the frame takes the image prompt")
    if args.preview_vae:
        pipe.load_preview_vae(synth.synth_state_dict(synth.tiny_vae_param_shapes(), 33) if args.preview_vae == "synth" else args.preview_vae)
        os.makedirs(args.preview_dir, exist_ok=True)

        def show(p, i, t, kw):
            if i % args.preview_every == 0:
                p.preview(kw["latents"], "pil")[0].save(os.path.join(args.preview_dir, f"step_{i:03d}.png"))
            return {}
        ip_kwargs["callback_on_step_end"] = show
        print(f"--preview-vae {args.preview_vae}: a PNG every {args.preview_every} steps into {args.preview_dir} (a callback runs the loop step by step)")
    if args.pag_scale > 0:
        from blobctrl_amd import pag
        layers = pag.resolve_layers(pipe.unet_cfg, args.pag_layers.split(","))
        ip_kwargs.update(pag_scale=args.pag_scale, pag_adaptive_scale=args.pag_adaptive_scale, pag_applied_layers=layers)
        print(f"--pag-scale {args.pag_scale}: {len(layers)} self-attention layers perturbed, UNet batch 3")
    if args.keep_background:
        # a masked edit: only the start and the target ellipse may be repainted; everywhere else every step puts back the untouched
        # frame's latents, noised to that step (with --zoom the frame is the zoomed one, and the paste-back below finishes the job)
        region = edit_inputs.edit_region_masks(["move"], [start], [target], R, R)
        ip_kwargs.update(blend_image_latents=pipe.encode_latents(edit_inputs.vae_input(frame)), blend_mask=region)
        print(f"--keep-background: {100 * float((region > 127).float().mean()):.1f} % of the frame may be repainted, the rest keeps the input's latents")
    otype = "pt" if args.zoom is not None else "np"           # a zoomed edit's result stays on the device for the paste-back
    img = pipe(prompt, None, None, score, feats, num_inference_steps=args.steps, guidance_scale=7.5,
               generator=torch.Generator().manual_seed(0), blobnet_conditioning_scale=1.0, blobnet_control_guidance_end=0.9,
               fg_image=fg, bg_image=bg, output_type=otype, **ip_kwargs)
    t5 = sync()
    print(f"models {t1 - t0:.1f} s | splat {1e3 * (t2 - t1):.1f} ms | DINOv2 {1e3 * (t3 - t2):.1f} ms | CLIP {1e3 * (t4 - t3):.1f} ms | "
          f"VAE encode x2 + {args.steps}-step loop + VAE decode {1e3 * (t5 - t4):.1f} ms (first call: includes planning + graph capture)")
    t6 = sync()
    img = pipe(prompt, None, None, score, feats, num_inference_steps=args.steps, guidance_scale=7.5,
               generator=torch.Generator().manual_seed(0), blobnet_conditioning_scale=1.0, blobnet_control_guidance_end=0.9,
               fg_image=fg, bg_image=bg, output_type=otype, **ip_kwargs)
    t7 = sync()
    print(f"second edit (plans cached): {1e3 * (t7 - t6):.1f} ms end to end; image {tuple(img.shape)}, range [{img.min():.3f}, {img.max():.3f}]")
    if args.zoom is not None:
        t8 = sync()
        pasted = overlay.apply_overlay(overlay.blur(zoom_mask, args.blur), image_dev, overlay.to_uint8(img, do_denormalize=False), zoom_crop)
        t9 = sync()
        kept = int((pasted[0] == image_dev).all(-1).sum())
        print(f"zoom: blur + paste-back on the device {1e3 * (t9 - t8):.2f} ms; {kept} of {R * R} pixels keep the original's bytes")
        img = pasted.float().div(255).cpu().numpy()
    if args.out:
        np.save(args.out, img[0])


if __name__ == "__main__":
    main()
