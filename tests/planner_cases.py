"""The planner sweep (tests/test_planner_paths_gpu.py): ONE block at SD-1.5 / BlobNet widths per case, (kind, channels, B, H, W, options),
chosen so that every switch of the denoise planner (blobctrl_amd/engine.py, launch.py, options.py and the library's eligibility functions)
is taken both ways.  This module holds the table, the recording of a case through the engine's own block methods, what a recorded plan
says about the kernel families it took, and the float64 reference (oracle/nets.py on the fp16-rounded input and the fp16-rounded matrices
the engine packs: the difference measures the kernels, not the quantisation of the weights)."""
import functools
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

from blobctrl_amd import synth
from tests.common import block_param_shapes, g

T_CTX, D_CTX = 77, 768
ZERO_ALPHA = 0.75            # BlobNet's conditioning scale on the zero-conv outputs (any value that is not 1)

# kind: resnet | transformer | down | up | dense.  p: the block's channels (resnet: cin, cout, split = channels of the first concat source
# or 0; transformer: C, cross; up: C, size = explicit output size or None; dense: N, K with B * H * W rows).  net: "unet" | "blob".
# fam / nofam: substrings that must / must not occur among the recorded launches ("kind|variant|rocprof" per launch).
Case = namedtuple("Case", "id kind p B H W net opts r2 zero prefix fam nofam")


def _c(id, kind, p, B, H, W, net="unet", opts=None, r2=False, zero=False, prefix="blk.", fam=(), nofam=()):
    return Case(id, kind, p, B, H, W, net, dict(opts or {}), r2, zero, prefix, tuple(fam), tuple(nofam))


def _res(cin, cout, split=0):
    return dict(cin=cin, cout=cout, split=split)


WREG2, WREG0, IGEMM = "conv_wreg_kernel<2>", "conv_wreg_kernel<0>", ", true, false>"     # (gemm_fast_kernel<tile, conv, upsample>)
GW, G256, FAST = "gemm_wreg_kernel<", "gemm256_kernel", "gemm_fast_kernel<"
SPLIT = ">+splitk_reduce|conv_"                                                        # (a split-K convolution on conv_wreg / conv_halo)
UPB = "up_blocks.2.attentions.0."                                                      # (rowchain_ok's exception for BlobNet's up blocks)

CASES = [
    # ------------------------------------------------------------------------------------------------ ResBlocks, one source
    _c("res320-64x128", "resnet", _res(320, 320), 1, 64, 128, fam=[WREG2, "halo_gnfin>"], nofam=[SPLIT, IGEMM]),
    _c("res320-72x112", "resnet", _res(320, 320), 1, 72, 112, fam=[WREG2], nofam=[IGEMM]),
    _c("res320-65x130", "resnet", _res(320, 320), 1, 65, 130, fam=["conv3x3|" + FAST, IGEMM, "groupnorm"], nofam=["conv_wreg"]),
    _c("res320-32x16-tall", "resnet", _res(320, 320), 2, 32, 16, fam=[WREG2], nofam=[IGEMM]),
    _c("res320-8x16-r2", "resnet", _res(320, 320), 2, 8, 16, r2=True, fam=[WREG2], nofam=[SPLIT]),
    _c("res320-8x16-halo", "resnet", _res(320, 320), 2, 8, 16, opts=dict(wreg=0), fam=["conv_halo_kernel<2>"], nofam=["conv_wreg"]),
    _c("res320-unet-B6", "resnet", _res(320, 320), 6, 8, 16, fam=[WREG2], nofam=[WREG0, "groupnorm"]),
    _c("res320-unet-B8", "resnet", _res(320, 320), 8, 8, 16, fam=[WREG0, "groupnorm"], nofam=[WREG2]),
    _c("res320-blob-B3", "resnet", _res(320, 320), 3, 8, 16, net="blob", fam=[WREG2], nofam=[WREG0, "groupnorm"]),
    _c("res320-blob-B4", "resnet", _res(320, 320), 4, 8, 16, net="blob", fam=[WREG0, "groupnorm"], nofam=[WREG2]),
    _c("res320-640-32x64-r2", "resnet", _res(320, 640), 2, 32, 64, r2=True, fam=[WREG2, "halo_gnfin_sc"], nofam=["conv1x1|"]),
    _c("res320-640-36x56", "resnet", _res(320, 640), 2, 36, 56, fam=["conv1x1|" + FAST, IGEMM], nofam=["conv_wreg", "_sc", GW]),
    _c("res640-1280-16x32", "resnet", _res(640, 1280), 2, 16, 32, fam=[WREG2, "halo_gnfin_sc"], nofam=["conv1x1|"]),
    _c("res640-1280-18x28", "resnet", _res(640, 1280), 2, 18, 28, fam=["conv1x1|" + FAST, IGEMM], nofam=["conv_wreg", "_sc", GW]),
    _c("res640-1280-16x32-nofold", "resnet", _res(640, 1280), 2, 16, 32, opts=dict(sc_fold=0), fam=["conv1x1|" + GW, WREG2], nofam=["_sc"]),
    _c("res640-1280-8x16-B8-nofold", "resnet", _res(640, 1280), 8, 8, 16, opts=dict(sc_fold=0), fam=["conv1x1|" + GW, WREG0], nofam=["_sc"]),
    _c("res640-1280-8x16-B10-nofold", "resnet", _res(640, 1280), 10, 8, 16, opts=dict(sc_fold=0), fam=["conv1x1|" + FAST, WREG0], nofam=["_sc", "conv1x1|" + GW]),
    _c("res640-1280-9x14-B5", "resnet", _res(640, 1280), 5, 9, 14, opts=dict(sc_fold=0), fam=["conv1x1|" + FAST, IGEMM], nofam=["conv_wreg", GW]),
    _c("res1280-16x32-r2", "resnet", _res(1280, 1280), 2, 16, 32, r2=True, fam=[WREG2, SPLIT], nofam=[IGEMM]),
    _c("res1280-8x16", "resnet", _res(1280, 1280), 2, 8, 16, fam=[WREG2, SPLIT], nofam=[IGEMM]),
    _c("res1280-9x14-r2", "resnet", _res(1280, 1280), 2, 9, 14, r2=True, fam=[IGEMM, "groupnorm"], nofam=["conv_wreg"]),
    _c("res1280-9x17-blob", "resnet", _res(1280, 1280), 1, 9, 17, net="blob", fam=[IGEMM], nofam=["conv_wreg"]),
    # ------------------------------------------------------------------------------------------------ ResBlocks of the up path: (hidden | skip)
    _c("res2560-1280-8x16", "resnet", _res(2560, 1280, 1280), 2, 8, 16, fam=[WREG2, "_sc"], nofam=["conv1x1|"]),
    _c("res2560-1280-8x16-nofold", "resnet", _res(2560, 1280, 1280), 2, 8, 16, opts=dict(sc_fold=0), fam=["conv1x1|" + GW], nofam=["_sc"]),
    _c("res2560-1280-9x17", "resnet", _res(2560, 1280, 1280), 1, 9, 17, fam=["conv1x1|" + FAST, IGEMM], nofam=["conv_wreg", GW]),
    _c("res1920-1280-16x32", "resnet", _res(1920, 1280, 1280), 2, 16, 32, fam=[WREG2, "_sc"], nofam=["conv1x1|"]),
    _c("res1920-1280-17x33", "resnet", _res(1920, 1280, 1280), 2, 17, 33, fam=["conv1x1|" + FAST, IGEMM], nofam=["conv_wreg"]),
    _c("res1920-640-16x32", "resnet", _res(1920, 640, 1280), 1, 16, 32, fam=[WREG2, "_sc"], nofam=["conv1x1|"]),
    _c("res1280-640-32x64", "resnet", _res(1280, 640, 640), 1, 32, 64, fam=[WREG2, "_sc"], nofam=["conv1x1|"]),
    _c("res1280-640-33x65-blob", "resnet", _res(1280, 640, 640), 1, 33, 65, net="blob", fam=["conv1x1|" + FAST, IGEMM], nofam=["conv_wreg"]),
    _c("res960-640-32x64", "resnet", _res(960, 640, 640), 1, 32, 64, fam=[WREG2, "_sc"], nofam=["conv1x1|"]),
    _c("res960-320-32x64", "resnet", _res(960, 320, 640), 1, 32, 64, fam=[WREG2, "_sc"], nofam=["conv1x1|"]),
    _c("res640-320-64x128", "resnet", _res(640, 320, 320), 1, 64, 128, fam=[WREG2, "_sc"], nofam=["conv1x1|", SPLIT]),
    _c("res640-320-65x130", "resnet", _res(640, 320, 320), 1, 65, 130, fam=["conv1x1|" + FAST, IGEMM], nofam=["conv_wreg"]),
    # ------------------------------------------------------------------------------------------------ Transformer2D, 320 channels
    _c("tfm320-cross-8x16-r2", "transformer", dict(C=320, cross=True), 2, 8, 16, r2=True, fam=["rowchain_kernel<midx>", "rowchain_kernel<out>"]),
    _c("tfm320-self-8x16-zero", "transformer", dict(C=320, cross=False), 2, 8, 16, net="blob", zero=True, fam=["rowchain_kernel<out,zero>"], nofam=["midx", "zero_conv|"]),
    _c("tfm320-self-32x16-tall", "transformer", dict(C=320, cross=False), 1, 32, 16, net="blob", zero=True, fam=["rowchain_kernel<out,zero>"]),
    _c("tfm320-cross-36x56", "transformer", dict(C=320, cross=True), 2, 36, 56, fam=["layernorm", "qkv|" + FAST], nofam=["rowchain|", G256]),
    _c("tfm320-cross-18x28-r2", "transformer", dict(C=320, cross=True), 2, 18, 28, r2=True, fam=["layernorm", "qkv|" + FAST], nofam=["rowchain|"]),
    _c("tfm320-self-9x17-zero", "transformer", dict(C=320, cross=False), 1, 9, 17, net="blob", zero=True, fam=["zero_conv|", "layernorm"], nofam=["rowchain|"]),
    _c("tfm320-cross-128blocks", "transformer", dict(C=320, cross=True), 4, 32, 64, opts=dict(ff_split_320=2), fam=["out_ffp/2", "rowchain_sum"]),
    _c("tfm320-cross-192blocks", "transformer", dict(C=320, cross=True), 6, 32, 64, opts=dict(ff_split_320=2), fam=["rowchain_kernel<out>"], nofam=["out_ff", "rowchain_sum"]),
    # ------------------------------------------------------------------------------------------------ Transformer2D, 640 channels
    _c("tfm640-unet-16blocks", "transformer", dict(C=640, cross=True), 2, 16, 32, fam=["qkv|" + GW, "attention"], nofam=["rowchain|", "ctx_fold"]),
    _c("tfm640-unet-32blocks", "transformer", dict(C=640, cross=True), 4, 16, 32, fam=["layernorm", "ff|" + G256], nofam=["rowchain|", GW]),
    _c("tfm640-unet-64blocks-r2", "transformer", dict(C=640, cross=True), 8, 16, 32, r2=True, fam=["rowchain_kernel<midx>", "out_ffp/4", "rowchain_sum"]),
    _c("tfm640-unet-80blocks", "transformer", dict(C=640, cross=True), 10, 16, 32, fam=["rowchain_kernel<midx>", "rowchain_kernel<out>"], nofam=["out_ff", "rowchain_sum"]),
    _c("tfm640-unet-18x28-r2", "transformer", dict(C=640, cross=True), 2, 18, 28, r2=True, fam=["layernorm", "qkv|" + FAST], nofam=["rowchain|", GW]),
    _c("tfm640-blobdown-32blocks", "transformer", dict(C=640, cross=False), 4, 16, 32, net="blob", zero=True, fam=["layernorm", "zero_conv|"], nofam=["rowchain|"]),
    _c("tfm640-blobdown-64blocks", "transformer", dict(C=640, cross=False), 8, 16, 32, net="blob", zero=True, fam=["out_ff/2", "rowchain_kernel<out_tail,zero>"], nofam=["out_ffp", "zero_conv|"]),
    _c("tfm640-blobup-16blocks", "transformer", dict(C=640, cross=False), 2, 16, 32, net="blob", zero=True, prefix=UPB, fam=["qkv|" + GW, "zero_conv|"], nofam=["rowchain|"]),
    _c("tfm640-blobup-32blocks", "transformer", dict(C=640, cross=False), 4, 16, 32, net="blob", zero=True, prefix=UPB, fam=["out_ff/2", "rowchain_kernel<out_tail,zero>"], nofam=["zero_conv|"]),
    _c("tfm640-blobup-64blocks", "transformer", dict(C=640, cross=False), 8, 16, 32, net="blob", zero=True, prefix=UPB, fam=["out_ff/2", "rowchain_kernel<out_tail,zero>"], nofam=["zero_conv|"]),
    _c("tfm640-unetup-32blocks", "transformer", dict(C=640, cross=True), 4, 16, 32, prefix=UPB, fam=["layernorm"], nofam=["rowchain|"]),
    _c("tfm640-blob-33x65-zero", "transformer", dict(C=640, cross=False), 1, 33, 65, net="blob", zero=True, fam=["layernorm", "zero_conv|"], nofam=["rowchain|"]),
    # ------------------------------------------------------------------------------------------------ Transformer2D, 1280 channels
    _c("tfm1280-cross-16x32-B2-r2", "transformer", dict(C=1280, cross=True), 2, 16, 32, r2=True, fam=["qkv|" + GW, "ctx_fold", "_softmax_wimg", "ff|" + G256]),
    _c("tfm1280-cross-16x32-B3", "transformer", dict(C=1280, cross=True), 3, 16, 32, fam=["layernorm", "qkv|" + G256], nofam=[GW, "ctx_fold"]),
    _c("tfm1280-cross-8x16-B2", "transformer", dict(C=1280, cross=True), 2, 8, 16, fam=["qkv|" + GW, "ctx_fold", "ff|" + GW], nofam=[G256, "layernorm"]),
    _c("tfm1280-cross-8x16-B4", "transformer", dict(C=1280, cross=True), 4, 8, 16, fam=["qkv|" + GW, "attn_out|" + GW, "ff|" + G256], nofam=["ctx_fold", "xattn"]),
    _c("tfm1280-cross-8x16-B8", "transformer", dict(C=1280, cross=True), 8, 8, 16, fam=["qkv|" + GW, "ff|" + G256], nofam=["ctx_fold"]),
    _c("tfm1280-cross-8x16-B10", "transformer", dict(C=1280, cross=True), 10, 8, 16, fam=["layernorm", "qkv|" + G256], nofam=[GW, "ctx_fold"]),
    _c("tfm1280-cross-9x14-r2", "transformer", dict(C=1280, cross=True), 2, 9, 14, r2=True, fam=["layernorm", "qkv|" + FAST], nofam=[GW, G256, "xattn|"]),
    _c("tfm1280-self-8x16-zero", "transformer", dict(C=1280, cross=False), 1, 8, 16, net="blob", zero=True, fam=["qkv|" + GW, "zero_conv|"], nofam=["rowchain|"]),
    _c("tfm1280-self-17x33-zero", "transformer", dict(C=1280, cross=False), 1, 17, 33, net="blob", zero=True, fam=["layernorm", "zero_conv|"], nofam=[GW]),
    # ------------------------------------------------------------------------------------------------ Downsample (stride 2)
    _c("down320-64x128", "down", dict(C=320), 1, 64, 128, fam=["downsample|" + FAST]),
    _c("down320-65x130", "down", dict(C=320), 1, 65, 130, fam=["downsample|" + FAST]),
    _c("down640-32x64", "down", dict(C=640), 2, 32, 64, fam=["downsample|" + FAST]),
    _c("down640-33x65", "down", dict(C=640), 1, 33, 65, fam=["downsample|" + FAST]),
    _c("down1280-16x32", "down", dict(C=1280), 2, 16, 32, fam=["downsample|" + FAST]),
    _c("down1280-17x33", "down", dict(C=1280), 1, 17, 33, fam=["downsample|" + FAST]),
    _c("down1280-18x28", "down", dict(C=1280), 3, 18, 28, fam=["downsample|" + FAST]),
    # ------------------------------------------------------------------------------------------------ Upsample (+ conv3x3)
    _c("up1280-8x16-x2", "up", dict(C=1280, size=None), 2, 8, 16, fam=["upsample|conv_wreg_kernel<", WREG0]),
    _c("up1280-9x14-x2", "up", dict(C=1280, size=None), 2, 9, 14, fam=["upsample|" + FAST, ", true, true>"], nofam=["conv_wreg"]),
    _c("up1280-9x17-to-17x33", "up", dict(C=1280, size=(17, 33)), 1, 9, 17, fam=["upsample|gemm_kernel<"], nofam=["conv_wreg", FAST]),
    _c("up1280-16x32-x2", "up", dict(C=1280, size=None), 1, 16, 32, fam=["upsample|conv_wreg_kernel<"]),
    _c("up1280-17x33-to-33x65", "up", dict(C=1280, size=(33, 65)), 1, 17, 33, fam=["upsample|gemm_kernel<"], nofam=["conv_wreg", FAST]),
    _c("up640-32x64-x2", "up", dict(C=640, size=None), 1, 32, 64, fam=["upsample|conv_wreg_kernel<"]),
    _c("up640-33x65-to-65x130", "up", dict(C=640, size=(65, 130)), 1, 33, 65, fam=["upsample|gemm_kernel<"], nofam=["conv_wreg", FAST]),
    _c("up640-18x28-x2", "up", dict(C=640, size=None), 1, 18, 28, fam=["upsample|" + FAST, ", true, true>"], nofam=["conv_wreg"]),
    # ------------------------------------------------------------------------------------------------ a dense projection (TrunkPlan.dense)
    _c("dense1280-60tiles", "dense", dict(N=1280, K=1280), 12, 16, 16, fam=["linear|" + FAST], nofam=[G256]),
    _c("dense1280-65tiles", "dense", dict(N=1280, K=1280), 13, 16, 16, fam=["linear|" + G256]),
    _c("dense1280-M3200", "dense", dict(N=1280, K=1280), 25, 8, 16, fam=["linear|" + FAST], nofam=[G256]),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---------------------------------------------------------------------------------------------------- weights and inputs
def _key(case):
    """What the numbers of a case depend on (NOT its planner options or prefix: cases that differ only there share weights, inputs, reference)."""
    return (case.kind, tuple(sorted((k, str(v)) for k, v in case.p.items())), case.B, case.H, case.W, case.r2, case.zero)


def _seed(case, salt=0):
    return zlib.crc32(repr(_key(case)).encode()) % 100000 + salt


def _shapes(case):
    p = case.p
    if case.kind == "resnet":
        sh = block_param_shapes("resnet", dict(cin=p["cin"], cout=p["cout"]))
    elif case.kind == "transformer":
        sh = block_param_shapes("transformer", dict(C=p["C"], ctx=D_CTX if p["cross"] else None))
    elif case.kind in ("down", "up"):
        sh = block_param_shapes("downsample", dict(C=p["C"]))
    else:
        sh = {"lin.weight": (p["N"], p["K"]), "lin.bias": (p["N"],)}
    if case.zero:
        sh["zc.weight"], sh["zc.bias"] = (p["C"], p["C"], 1, 1), (p["C"],)
    return sh


@functools.lru_cache(maxsize=4)
def _numbers(key, seed):
    """(state dict of the block, inputs) of the cases with this key, fp32 as synthesised."""
    case = next(c for c in CASES if _key(c) == key)
    p, B, H, W = case.p, case.B, case.H, case.W
    sd = synth.synth_state_dict(_shapes(case), seed)
    inp = {}
    if case.kind == "dense":
        inp["x"] = g(seed + 1, B * H * W, p["K"])
    else:
        inp["x"] = g(seed + 1, B, p.get("cin", p.get("C")), H, W)
    if case.kind == "resnet":
        inp["temb"] = g(seed + 2, B, 1280)
    if case.kind == "transformer" and p["cross"]:
        inp["ctx"] = g(seed + 3, B, T_CTX, D_CTX)
    if case.r2:
        assert W > H, "the BlobNet residual of a non-square map is its right-hand H x H square"
        inp["r2"] = g(seed + 4, B, p.get("cout", p.get("C")), H, H)
    return sd, inp


def numbers(case):
    return _numbers(_key(case), _seed(case))


# ---------------------------------------------------------------------------------------------------- recording
def _act(x, device):
    from blobctrl_amd.engine import Act
    B, C, H, W = x.shape
    return Act(x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous().half().to(device), C, H, W)


def record(case, device):
    """Record the case through the engine's block methods under the BC_PLAN the caller has set.  Returns (rec, seg, outs) with outs =
    {"out": Act or tensor [, "zero": tensor]}."""
    from blobctrl_amd.engine import TrunkConfig, TrunkPlan
    from blobctrl_amd.launch import Recorder
    from blobctrl_amd.weights import PackedTrunk
    device = torch.device(device)
    p, B, H, W, px = case.p, case.B, case.H, case.W, case.prefix
    sd0, inp = numbers(case)
    sd = {("zc." + k[3:] if k.startswith("zc.") else px + k): v for k, v in sd0.items()}
    sd["conv_in.weight"] = torch.zeros(8, 4, 3, 3)                      # (PackedTrunk expects a trunk: unused stand-ins)
    if case.kind != "resnet":
        sd["none.time_emb_proj.weight"], sd["none.time_emb_proj.bias"] = torch.zeros(8, 1280), torch.zeros(8)
    pw = PackedTrunk(sd, device, (320, 640, 1280, 1280))
    blob = case.net == "blob"
    cross = D_CTX if case.kind == "transformer" and p["cross"] else None
    cfg = TrunkConfig(in_channels=4, num_heads=8, norm_num_groups=32, cross_attention_dim=cross, is_blobnet=blob)
    rec = Recorder(device)
    seg = rec.begin(case.id)
    plan = TrunkPlan(rec, pw, cfg, B, H, W)
    plan.res_events, plan.res_bmod = None, B
    r2 = None
    if case.r2:
        r = inp["r2"]
        # full-canvas token-major [B][H * W][C] (engine.Residuals); the columns left of r2_xmin = W - H hold a value that must not be added
        canvas = torch.full((B, H, W, r.shape[1]), 1000.0)
        canvas[:, :, W - H:, :] = r.permute(0, 2, 3, 1)
        r2 = canvas.reshape(B, H * W, r.shape[1]).contiguous().half().to(device)
    outs = {}
    if case.kind == "resnet":
        # time_emb_proj(silu(temb)) of every ResBlock is one GEMM in the engine (record_time); silu(temb) in fp16 is the given input
        plan.tproj = plan.dense(F.silu(inp["temb"]).half().to(device), B, 1280, "temb_all", pw.temb_total, kind="temb")
        x = inp["x"]
        s = p["split"]
        a, b = (_act(x[:, :s], device), _act(x[:, s:], device)) if s else (_act(x, device), None)
        buf = rec.empty(B, H * W, p["cout"])                           # the caller's output buffer, as record_forward's prefix passes one
        outs["out"] = plan.resnet(px, a, b, p["cout"], r2=r2, out=buf)
        assert outs["out"].t.data_ptr() == buf.data_ptr()
    elif case.kind == "transformer":
        if cross:
            plan.record_context(inp["ctx"].reshape(-1, D_CTX).half().to(device), T_CTX)
        zero = ("zc", ZERO_ALPHA, None, None, 0) if case.zero else None
        out, pre = plan.transformer(px, _act(inp["x"], device), r2=r2, zero=zero)
        if case.zero and pre is None:                                  # (as record_forward's _Feats.append: a launch of its own)
            pre = plan.dense(out.t, B * H * W, out.C, "zc", out.C, kind="zero_conv", alpha=ZERO_ALPHA, rows_per_batch=H * W)
        outs["out"] = out
        if case.zero:
            outs["zero"] = pre
    elif case.kind == "down":
        outs["out"] = plan.conv3x3(_act(inp["x"], device), px + "conv", p["C"], stride=2, kind="downsample")
    elif case.kind == "up":
        size = p["size"] or (2 * H, 2 * W)
        outs["out"] = plan.conv3x3(_act(inp["x"], device), px + "conv", p["C"], up_to=size, kind="upsample")
    else:
        outs["out"] = plan.dense(inp["x"].half().to(device), B * H * W, p["K"], px + "lin", p["N"])
    return rec, seg, outs


def launches(rec):
    return [f"{m['kind']}|{m['variant']}|{m['rocprof']}" for m in rec.seg.meta]


def check_family(case, rec):
    ls = launches(rec)
    for s in case.fam:
        assert any(s in l for l in ls), f"{case.id}: no launch with '{s}' - the planner took another family:\n" + "\n".join(ls)
    for s in case.nofam:
        assert not any(s in l for l in ls), f"{case.id}: a launch with '{s}' - the planner took another family:\n" + "\n".join(ls)


def family(rec):
    """Short name of what ran, for the margins table: the distinct kernels of the block's launches in order."""
    names = []
    for m in rec.seg.meta:
        if m["kind"] in ("temb", "memset", "gn_stats", "ctx_kv", "pack_kv"):
            continue
        v, rp = m["variant"], m["rocprof"]
        n = v if "rowchain" in v else rp if rp.startswith("conv_") else rp.split("<")[0]
        if rp.startswith("gemm_fast_kernel") and ", true, " in rp:
            n += "<conv>"
        if "+splitk_reduce" in v:
            n += "/splitk"
        if n not in names:
            names.append(n)
    return " ".join(names)


# ---------------------------------------------------------------------------------------------------- which switch went which way
def sides(case, rec):
    """The (switch, side) pairs this recorded case shows: the side from the case's geometry AND the kernel family the plan took."""
    ls = launches(rec)
    has = lambda s: any(s in l for l in ls)
    p, B, H, W = case.p, case.B, case.H, case.W
    M, HW = B * H * W, H * W
    net = case.net
    out = set()
    dflt = not case.opts
    if case.kind == "resnet":
        wreg = has("conv3x3|conv_wreg_kernel")
        if dflt:
            out.add(("conv_eligible", "aligned:conv_wreg" if wreg else "ragged:implicit_gemm"))
            assert wreg == (W % 16 == 0 and H % 8 == 0) and wreg != has(IGEMM), ls
            if wreg:
                requests = B if net == "blob" else max(1, B // 2)
                out.add((f"gn_pass_min_requests/{net}", (f"{requests}:" if requests >= 3 else "<3:") + ("pass+conv_wreg<0>" if has(WREG0) else "fused_conv_wreg<2>")))
                assert has(WREG0) != has(WREG2)
                out.add(("conv_splitk", "split" if has(SPLIT) else "unsplit"))
            if p["cin"] != p["cout"]:
                out.add(("sc_fold_eligible", "folded" if has("_sc") else "launch"))
        if case.opts == dict(wreg=0):
            out.add(("conv_eligible", "aligned:conv_halo"))
        if case.opts == dict(sc_fold=0) and p["cout"] == 1280:
            side = "gw" if has("conv1x1|" + GW) else "over_gw_maxm" if M > 1024 and M % 64 == 0 else "rejected_by_gemm_wreg"
            out.add(("shortcut_gw", side))
        if case.r2:
            out.add(("r2_xmin", f"resnet{p['cout']}"))
    elif case.kind == "transformer":
        C = p["C"]
        rc = has("rowchain_kernel")
        if C in (320, 640):
            out.add((f"rowchain_hw64/{C}", ("hw%64==0" if HW % 64 == 0 else "hw%64!=0") + (":rowchain" if rc else ":launch_list")))
            assert HW % 64 == 0 or not rc
        if C == 640 and HW % 64 == 0:
            who = "unet" if net == "unet" else "blob_up" if case.prefix.startswith("up_blocks") else "blob_down"
            out.add((f"rowchain_min_blocks_640/{who}", f"{M // 64}:" + ("rowchain" if rc else "gw" if has("qkv|" + GW) else "launch_list")))
        if rc and (C == 640 or case.opts.get("ff_split_320")):
            out.add((f"block_end_split/{C}", ("<=" if M // 64 <= (64 if C == 640 else 128) else ">") + (":split" if has("out_ff") else ":one_launch")))
            if has("out_ff"):
                out.add(("block_end_form", "out_ffp+sum" if has("out_ffp") else "out_ff+out_tail"))
        if rc and p["cross"]:
            assert has("midx"), ls
        if C == 1280:
            gw = has("qkv|" + GW)
            out.add(("gw_maxm", ("rejected_by_gemm_wreg" if HW % 64 else (f"{M}:" if M >= 1024 else "<1024:") + ("gw" if gw else "launch_list"))))
            assert gw == (HW % 64 == 0 and M <= 1024), ls
            if gw and p["cross"]:
                out.add(("ctx_fold_maxb", f"{B}:" + ("folded" if has("xattn|") else "attention")))
                assert has("_softmax_wimg") == has("xattn|") and (has("ctx_fold|") or not has("xattn|"))
            if gw:
                out.add(("g256_min_tiles/ff1", (f"{(M // 256) * 40}:" if M % 256 == 0 else "m%256!=0:") + ("gemm256" if has("ff|" + G256) else "gemm_wreg")))
        if case.r2:
            out.add(("r2_xmin", f"transformer{C}:" + ("rowchain" if rc else "gw" if has("qkv|" + GW) else "launch_list")))
        if case.zero:
            out.add(("zero_conv", "in_rowchain" if has(",zero>") else "launch"))
        out.add(("is_blobnet", net))
    elif case.kind == "up":
        Hv, Wv = p["size"] or (2 * H, 2 * W)
        geo = "explicit_size" if p["size"] else "x2_aligned" if Wv % 16 == 0 and Hv % 8 == 0 else "x2_ragged"
        out.add(("ups_wreg", geo + (":conv_wreg" if has("conv_wreg") else ":implicit_gemm" if has(FAST) else ":generic_gemm")))
    elif case.kind == "down":
        out.add(("downsample", "aligned" if W % 16 == 0 and H % 8 == 0 else "ragged"))
    else:
        tiles = (M // 256) * (p["N"] // 256)
        out.add(("g256_min_tiles", ("m%256!=0" if M % 256 else f"{tiles}") + (":gemm256" if has(G256) else ":gemm_fast")))
    return out


# ---------------------------------------------------------------------------------------------------- float64 reference
def _r16(t):
    return t.half().double()


@functools.lru_cache(maxsize=4)
def _reference(key, seed):
    from oracle import nets
    case = next(c for c in CASES if _key(c) == key)
    p, B = case.p, case.B
    sd0, inp = _numbers(key, seed)
    sd = {"blk." + k: (_r16(v) if v.ndim > 1 else v.double()) for k, v in sd0.items()}     # matrices in fp16, vectors in fp32: as PackedTrunk
    x = _r16(inp["x"])
    ref = {}
    with torch.no_grad():
        if case.kind == "resnet":
            # the engine's input is silu(temb) in fp16: per image, time_emb_proj(that) goes into the bias and the oracle's own silu(temb) sees 0
            s = _r16(F.silu(inp["temb"]))
            wt, bt = sd["blk.time_emb_proj.weight"], sd["blk.time_emb_proj.bias"]
            outs = []
            for b in range(B):
                sdb = dict(sd)
                sdb["blk.time_emb_proj.bias"] = bt + wt @ s[b]
                outs.append(nets.resnet_block(sdb, "blk.", x[b:b + 1], torch.zeros(1, 1280, dtype=torch.float64), 32))
            out = torch.cat(outs)
        elif case.kind == "transformer":
            ctx = _r16(inp["ctx"]) if p["cross"] else None
            out = nets.transformer_2d(sd, "blk.", x, ctx, 8, 32)
        elif case.kind == "down":
            out = nets.downsample(sd, "blk.", x)
        elif case.kind == "up":
            out = nets.upsample(sd, "blk.", x, p["size"])
        else:
            out = F.linear(x, sd["blk.lin.weight"], sd["blk.lin.bias"])
        if case.r2:
            out = nets.add_right(out, _r16(inp["r2"]))
        ref["out"] = out.numpy()
        if case.zero:
            ref["zero"] = (F.conv2d(out, sd["blk.zc.weight"], sd["blk.zc.bias"]) * ZERO_ALPHA).numpy()
    return ref


def reference(case):
    """{"out": float64 NCHW (dense: [M, N]) [, "zero": ...]}: shared by the cases that differ only in planner options."""
    return _reference(_key(case), _seed(case))


def nchw(t, B, H, W):
    t = t.t if hasattr(t, "t") and not torch.is_tensor(t) else t
    return t.float().cpu().view(B, H, W, -1).permute(0, 3, 1, 2).numpy()
