"""The ResBlock's 1x1 shortcut folded into conv2's K loop (BcGemm.S, csrc/conv_wreg.hip): out = conv3x3(silu(gn(h))) + conv1x1(x | skip) +
time-embedding row + BlobNet residual as ONE launch, at the shapes of a 512^2 denoise step (both trunks' M = 128 ... 16384 rows; one- and
two-source shortcuts; unsplit, split-K - every split takes a share of both kinds of chunk - including splits of shortcut chunks
only; the GroupNorm finalized in the prologue, read as an affine table, or applied by a pass in front).

Reference: fp32 torch on the same fp16-rounded inputs.  Bars:
  * the block tests' own (tests/test_blocks_gpu.py::_check): max-abs / scale < 1e-2 and PSNR > 40 dB;
  * the folded form's error may exceed the unfolded form's (conv1x1 launch, fp16 shortcut tensor, residual read) on the same seed by at
    most the unfolded form's spread over three seeds - the fold REMOVES one fp16 rounding, so it should be equal or better;
  * folded against unfolded on identical inputs: they differ by that rounding of the shortcut (half an ulp of |shortcut|), the two outputs'
    own half-ulp roundings and summation order: max-abs difference <= 4 * 2^-11 * max(|out|, |shortcut|).
Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.common import g, psnr  # noqa: E402
from tests.test_kernels_gpu import h, rec, run  # noqa: E402,F401

G, EPS = 32, 1e-5

# (B, H, W, C = conv2's channels, S1, S2 = channels of the shortcut's sources (S2 = 0: one source), splitk (None: the planner's))
STEP_SHAPES = [
    (1, 8, 16, 1280, 1280, 1280, None),     # M = 128
    (2, 8, 16, 1280, 1280, 1280, None),     # M = 256   up block, 8 x 16 level
    (1, 16, 32, 1280, 640, 0, None),        # M = 512   down block 640 -> 1280
    (2, 16, 32, 1280, 640, 0, None),        # M = 1024
    (2, 16, 32, 1280, 1280, 1280, None),    # M = 1024  up block
    (2, 16, 32, 1280, 1280, 640, None),
    (1, 32, 64, 640, 320, 0, None),         # M = 2048  down block 320 -> 640
    (2, 32, 64, 640, 320, 0, None),         # M = 4096
    (2, 32, 64, 640, 640, 1280, None),      # M = 4096  up block
    (2, 32, 64, 640, 640, 640, None),
    (2, 32, 64, 640, 640, 320, None),
    (1, 64, 128, 320, 320, 640, None),      # M = 8192
    (2, 64, 128, 320, 320, 640, None),      # M = 16384
    (2, 64, 128, 320, 320, 320, None),
]
SPLIT_SHAPES = [
    (1, 32, 64, 640, 320, 0, 1),            # 10 + 5 chunks in one workgroup
    (1, 64, 128, 320, 320, 320, 1),         # 5 + 10
    (1, 64, 128, 320, 320, 640, 4),         # 5 + 15 chunks: 2 + 4 per split: three splits with nine-tap chunks, the fourth with shortcut chunks only
    (1, 16, 32, 1280, 640, 0, 4),           # 20 + 10 chunks: 5 + 3 per split, the last split with one shortcut chunk
    (2, 8, 16, 1280, 1280, 1280, 15),       # 20 + 40 chunks: 2 + 3 per split, 14 splits, the last four hold shortcut chunks only
    (1, 8, 16, 1280, 1280, 640, 10),        # 20 + 30 chunks: 2 + 3 per split; the source boundary (chunk 20 of the shortcut) inside a split
    (1, 32, 64, 640, 640, 320, 7),          # 10 + 15 chunks: 2 + 3 per split, five splits
]


def _nhwc(x):
    B, C, H, W = x.shape
    return h(x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous())


def _case(seed, B, H, W, C, S1, S2):
    Cs = S1 + S2
    s = 100 * seed
    d = dict(hid=g(s + 1, B, C, H, W) * 1.7 + 0.3, x1=g(s + 2, B, S1, H, W), x2=g(s + 3, B, S2, H, W) * 0.8 + 0.1 if S2 else None,
             w=g(s + 4, C, C, 3, 3) / math.sqrt(9 * C), b=g(s + 5, C), wsc=g(s + 6, C, Cs) / math.sqrt(Cs), bsc=g(s + 7, C),
             gamma=1.0 + 0.2 * g(s + 8, C), beta=0.3 * g(s + 9, C), temb=g(s + 10, B, C), r2=g(s + 11, 1, C, H, W))
    return d


def _reference(d, B, H, W, C, S1, S2):
    """fp32 on the GPU from the fp16-rounded inputs; the 3x3 convolution as nine shifted matrix products (plain fp32 GEMMs).  Returns
    (out, shortcut) as [B][C][H][W] on the CPU."""
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = "cuda"
    hid = d["hid"].half().float().to(dev)
    y = F.silu(F.group_norm(hid, G, d["gamma"].to(dev), d["beta"].to(dev), EPS)).half().float()
    yp = F.pad(y, (1, 1, 1, 1)).permute(0, 2, 3, 1)                                  # [B][H + 2][W + 2][C]
    w = d["w"].half().float().to(dev)
    out = torch.zeros(B, H, W, C, device=dev, dtype=torch.float32)
    for ky in range(3):
        for kx in range(3):
            out += yp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
    xs = d["x1"] if d["x2"] is None else torch.cat([d["x1"], d["x2"]], 1)
    sc = xs.half().float().to(dev).permute(0, 2, 3, 1) @ d["wsc"].half().float().to(dev).t() + d["bsc"].to(dev)
    out = out + d["b"].to(dev) + sc + d["temb"].half().float().to(dev)[:, None, None, :]
    xmin = W - H if W > H else 0
    out[:, :, xmin:] += d["r2"].half().float().to(dev).permute(0, 2, 3, 1)[:, :, xmin:]
    return out.permute(0, 3, 1, 2).cpu(), sc.permute(0, 3, 1, 2).cpu()


def _launch(rec, d, B, H, W, C, S1, S2, sk, affine, fold):
    """conv2 of the block through the recorder: `fold` True = one launch (BcGemm.S), False = conv1x1 launch + residual read."""
    from blobctrl_amd import _lib
    from blobctrl_amd.weights import pack_conv3x3, pack_conv_wreg
    Cs, M, HW = S1 + S2, B * H * W, H * W
    p3, wsc = pack_conv3x3(d["w"]).half(), d["wsc"].half()

    def fn():
        t, x1, x2 = _nhwc(d["hid"]), _nhwc(d["x1"]), (_nhwc(d["x2"]) if S2 else None)
        gam, bet = d["gamma"].cuda(), d["beta"].cuda()
        kw = {}
        if affine == 2:
            kw.update(a_gn=dict(x1=t, C1=C, x2=None, C2=0, B=B, HW=HW, G=G, eps=EPS, gamma=gam, beta=bet), a_act=_lib.ACT_SILU)
        elif affine == 1:
            kw.update(a_affine=rec.gn_affine(t, C, None, 0, B, HW, G, EPS, gam, bet), a_act=_lib.ACT_SILU)
        else:
            t = rec.groupnorm(t, C, None, 0, B, HW, G, EPS, gam, bet, True)
        if fold:
            kw.update(S=x1, lds=S1, Cs=Cs, W=pack_conv_wreg(p3, wsc).cuda(), bias=(d["b"] + d["bsc"]).cuda())
            if S2:
                kw.update(S2=x2, lds2=S2, S1=S1)
        else:
            skw = dict(A2=x2, C1=S1, lda=S1, lda2=S2) if S2 else {}
            sc = rec.gemm(A=x1, W=wsc.cuda(), M=M, N=C, K=Cs, out=rec.empty(M, C), bias=d["bsc"].cuda(), **skw)
            kw.update(R=sc, ldr=C, W=pack_conv_wreg(p3).cuda(), bias=d["b"].cuda())
        out = rec.gemm(A=t, lda=C, M=M, N=C, K=9 * C, out=rec.empty(M, C), conv=dict(Cin=C, Hin=H, Win=W, Hout=H, Wout=W, stride=1),
                       rows_per_batch=HW, tile_cfg=_lib.TILE_WREG, splitk=sk, rowvec=h(d["temb"]), ld_rowvec=C, R2=_nhwc(d["r2"]), ldr2=C,
                       r2_xmin=W - H if W > H else 0, r2_bmod=1, out_w=W, want_gn=True, **kw)
        meta = rec.seg.meta[-1]
        assert meta["rocprof"] == f"conv_wreg_kernel<{affine}>", meta
        assert ("_sc" in meta["variant"]) == fold, meta["variant"]
        return out, rec.tots[out.data_ptr()], meta["shape"][-1]
    out, tot, sk_used = run(rec, fn)
    return out.float().cpu().view(B, H, W, C).permute(0, 3, 1, 2), out, tot, sk_used


def _errors(got, ref):
    got, ref = got.numpy(), ref.numpy()
    return float(np.abs(got - ref).max() / np.abs(ref).max()), float(psnr(got, ref))


def _check_case(rec, B, H, W, C, S1, S2, sk, affine, sk_folded=None):
    name = f"[{B * H * W}, {C}, 9*{C}+{S1}{'|' + str(S2) if S2 else ''}] sk={sk} affine={affine}"
    ef, eu = [], []
    for seed in (1, 2, 3):
        d = _case(seed, B, H, W, C, S1, S2)
        ref, sc_ref = _reference(d, B, H, W, C, S1, S2)
        fold, fold_raw, tot, sk_f = _launch(rec, d, B, H, W, C, S1, S2, sk, affine, True)
        unf, _, _, sk_u = _launch(rec, d, B, H, W, C, S1, S2, sk, affine, False)
        assert sk_folded is None or sk_f == sk_folded, (sk_f, sk_folded)
        (e_f, p_f), (e_u, p_u) = _errors(fold, ref), _errors(unf, ref)
        diff = float((fold - unf).abs().max())
        bound = 4 * 2.0 ** -11 * max(float(ref.abs().max()), float(sc_ref.abs().max()))
        print(f"fold {name} seed {seed}: folded {e_f:.3e} / {p_f:.1f} dB (splitk {sk_f}), unfolded {e_u:.3e} / {p_u:.1f} dB (splitk {sk_u}); "
              f"folded vs unfolded max-abs {diff:.3e} (bound {bound:.3e})")
        ef.append((e_f, p_f)), eu.append((e_u, p_u))
        assert e_f < 1e-2 and p_f > 40.0, f"{name} seed {seed}: {e_f:.3e} / {p_f:.1f} dB"
        assert diff <= bound, f"{name} seed {seed}: folded vs unfolded {diff:.3e} > {bound:.3e}"
        if seed == 1:
            # GroupNorm statistics of the fp16-rounded output (the next block's norm1 reads them)
            from blobctrl_amd.launch import decode_gn_tot, gn_tot_slots
            s = gn_tot_slots(decode_gn_tot(tot).float())
            o = fold_raw.float().cpu().view(B, H * W, C)
            want = gn_tot_slots(torch.stack([o.sum(1), (o * o).sum(1)], -1))
            assert torch.allclose(s[..., 0], want[..., 0], rtol=1e-3, atol=1e-2 * (H * W) ** 0.5)
            assert torch.allclose(s[..., 1], want[..., 1], rtol=1e-3, atol=1e-2 * (H * W) ** 0.5)
    spread = max(e for e, _ in eu) - min(e for e, _ in eu)
    print(f"fold {name}: unfolded spread over seeds {spread:.3e}")
    for (e_f, _), (e_u, _) in zip(ef, eu):
        assert e_f <= e_u + spread, f"{name}: folded {e_f:.3e} exceeds unfolded {e_u:.3e} by more than the unfolded spread {spread:.3e}"


@pytest.mark.parametrize("B,H,W,C,S1,S2,sk", STEP_SHAPES)
def test_fold_step_shapes_fused_groupnorm(rec, B, H, W, C, S1, S2, sk):
    _check_case(rec, B, H, W, C, S1, S2, sk, 2)


# splits the folded launch runs where the shares of the two kinds of chunk run out at different splits: the last ones hold shortcut chunks only
SC_ONLY_SPLITS = {(2, 8, 16, 1280, 1280, 1280, 15): 14, (1, 64, 128, 320, 320, 640, 4): 4}


@pytest.mark.parametrize("affine", [2, 1, 0])
@pytest.mark.parametrize("B,H,W,C,S1,S2,sk", SPLIT_SHAPES)
def test_fold_splits_all_forms(rec, B, H, W, C, S1, S2, sk, affine):
    _check_case(rec, B, H, W, C, S1, S2, sk, affine, SC_ONLY_SPLITS.get((B, H, W, C, S1, S2, sk)))


@pytest.mark.parametrize("affine", [1, 0])
@pytest.mark.parametrize("B,H,W,C,S1,S2,sk", [STEP_SHAPES[1], STEP_SHAPES[5], STEP_SHAPES[8], STEP_SHAPES[12]])
def test_fold_step_shapes_other_forms(rec, B, H, W, C, S1, S2, sk, affine):
    _check_case(rec, B, H, W, C, S1, S2, sk, affine)


def test_device_packer_matches_python(rec):
    from blobctrl_amd import _lib
    from blobctrl_amd.weights import pack_conv_wreg
    lib = _lib.load()
    for N, Cin, Cs in [(320, 320, 640), (640, 640, 1920), (1280, 1280, 2560)]:
        w = torch.randint(-32768, 32767, (N, 9 * Cin), dtype=torch.int16, generator=torch.Generator().manual_seed(N))
        ws = torch.randint(-32768, 32767, (N, Cs), dtype=torch.int16, generator=torch.Generator().manual_seed(Cs))
        wd, sd = w.cuda(), ws.cuda()
        out = torch.empty(N, 9 * Cin + Cs, dtype=torch.int16, device="cuda")
        _lib.check(lib.bc_conv_wreg_pack_sc(wd.data_ptr(), N, Cin, sd.data_ptr(), Cs, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "pack_sc")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), pack_conv_wreg(w, ws))


@pytest.mark.parametrize("gn_pass", [False, True])
@pytest.mark.parametrize("split", [0, 320])
def test_resnet_block_folds_and_matches_the_launch_list(split, gn_pass, monkeypatch):
    """engine.resnet on a 320 -> 640 block with shortcut at 32 x 64 (one source, and the up-block form hidden | skip): the default plan
    records no conv1x1 launch, BC_PLAN sc_fold=0 records the launch list it replaced, and the two outputs differ by the shortcut's rounding."""
    from tests.common import set_plan
    from tests.test_blocks_gpu import _act, _plan, _run
    B, H, W, Cin, Cout = 2, 32, 64, 640 if split else 320, 640
    sd = {"norm1.weight": 1.0 + 0.2 * g(1, Cin), "norm1.bias": 0.3 * g(2, Cin), "conv1.weight": g(3, Cout, Cin, 3, 3) / math.sqrt(9 * Cin),
          "conv1.bias": g(4, Cout), "time_emb_proj.weight": g(5, Cout, 1280) / math.sqrt(1280), "time_emb_proj.bias": g(6, Cout),
          "norm2.weight": 1.0 + 0.2 * g(7, Cout), "norm2.bias": 0.3 * g(8, Cout), "conv2.weight": g(9, Cout, Cout, 3, 3) / math.sqrt(9 * Cout),
          "conv2.bias": g(10, Cout), "conv_shortcut.weight": g(11, Cout, Cin, 1, 1) / math.sqrt(Cin), "conv_shortcut.bias": g(12, Cout)}
    x, temb = g(13, B, Cin, H, W), g(14, B, 1280)
    outs, scs = [], []
    for fold in (True, False):
        set_plan(monkeypatch, sc_fold=fold, gn_pass_min_requests=1 if gn_pass else 0)
        rec_, seg, plan = _plan("fold", sd, B, H, W)
        plan.tproj = plan.dense(F.silu(temb).half().cuda(), B, 1280, "temb_all", plan.pw.temb_total, kind="temb")
        out = plan.resnet("blk.", _act(x[:, :split]), _act(x[:, split:]), Cout) if split else plan.resnet("blk.", _act(x), None, Cout)
        kinds, variants = list(rec_.seg.kinds), [m.get("variant", "") for m in rec_.seg.meta]
        assert ("conv1x1" in kinds) == (not fold), kinds
        assert any("_sc" in v for v in variants) == fold, variants
        assert any(m.get("rocprof") == f"conv_wreg_kernel<{0 if gn_pass else 2}>" for m in rec_.seg.meta)
        _run(seg)
        outs.append(out.t.float().cpu())
    xs = x.half().float().permute(0, 2, 3, 1).reshape(-1, Cin)
    sc = xs @ sd["conv_shortcut.weight"].reshape(Cout, Cin).half().float().t() + sd["conv_shortcut.bias"]
    diff = float((outs[0] - outs[1]).abs().max())
    bound = 4 * 2.0 ** -11 * max(float(outs[1].abs().max()), float(sc.abs().max()))
    print(f"resnet 320->640 split={split} gn_pass={gn_pass}: folded vs sc_fold=0 max-abs {diff:.3e} (bound {bound:.3e}), launches {len(kinds)}")
    assert diff <= bound
