#!/usr/bin/env python3
"""conv2 of a ResBlock with its 1x1 shortcut FOLDED into the K loop (BcGemm.S, csrc/conv_wreg.hip) against conv1x1 launch + conv2 with
the residual read, on the shapes of a 512^2 step, one process, interleaved.  PROBE_COLD=1: weights from HBM (caches flushed before every
launch), as in the step.  PROBE_SK=a,b: explicit K splits of the folded form besides the planner's.  With BC_WREG_STAMPS=1 the library
prints where the folded launch's cycles go (the shortcut phase separately)."""
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from blobctrl_amd import _lib  # noqa: E402
from blobctrl_amd.launch import Recorder, encode_gn_tot  # noqa: E402
from blobctrl_amd.weights import pack_conv_wreg  # noqa: E402
from tools.tune_gemm import time_launch, time_launch_cold  # noqa: E402

dev = torch.device("cuda:0")
rec = Recorder(dev)
stream = torch.cuda.current_stream().cuda_stream
# (B, H, W, C, S1, S2): conv2 C -> C, shortcut over S1 | S2 channels
SHAPES = [(2, 8, 16, 1280, 1280, 1280), (1, 8, 16, 1280, 1280, 1280), (2, 16, 32, 1280, 1280, 1280), (2, 16, 32, 1280, 1280, 640),
          (2, 16, 32, 1280, 640, 0), (1, 16, 32, 1280, 640, 0), (2, 32, 64, 640, 640, 1280), (2, 32, 64, 640, 640, 640),
          (2, 32, 64, 640, 640, 320), (2, 32, 64, 640, 320, 0), (1, 32, 64, 640, 320, 0), (2, 64, 128, 320, 320, 640),
          (2, 64, 128, 320, 320, 320), (1, 64, 128, 320, 320, 320)]
cold = os.environ.get("PROBE_COLD")
thrash = torch.zeros(160 << 20, dtype=torch.float32, device=dev) if cold else None
if os.environ.get("PROBE_SHAPES"):
    SHAPES = [SHAPES[int(i)] for i in os.environ["PROBE_SHAPES"].split(",")]
sks = [None] + [int(v) for v in os.environ.get("PROBE_SK", "").split(",") if v]
for (B, H, W, C, S1, S2) in SHAPES:
    Cs, HW, M = S1 + S2, H * W, B * H * W
    hid = torch.randn(B, HW, C, device=dev, dtype=torch.float16)
    x1 = torch.randn(B, HW, S1, device=dev, dtype=torch.float16)
    x2 = torch.randn(B, HW, S2, device=dev, dtype=torch.float16) if S2 else None
    wt = (torch.randn(C, 9 * C, device=dev) / math.sqrt(9 * C)).half()
    wsc = (torch.randn(C, Cs, device=dev) / math.sqrt(Cs)).half()
    w_plain, w_fold = pack_conv_wreg(wt), pack_conv_wreg(wt, wsc)
    bias, temb = torch.randn(C, device=dev), torch.randn(B, C, device=dev).half()
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    conv = dict(Cin=C, Hin=H, Win=W, Hout=H, Wout=W, stride=1)
    f = hid.float().view(B, HW // 128, 128, C)
    rec.tots[hid.data_ptr()] = encode_gn_tot(torch.stack([f.sum((1, 2)), (f * f).sum((1, 2))], -1)).to(dev)
    common = dict(A=hid, lda=C, M=M, N=C, K=9 * C, conv=conv, rows_per_batch=HW, tile_cfg=_lib.TILE_WREG, a_act=_lib.ACT_SILU, want_gn=True,
                  rowvec=temb, ld_rowvec=C, a_gn=dict(x1=hid, C1=C, x2=None, C2=0, B=B, HW=HW, G=32, eps=1e-5, gamma=gamma, beta=beta))
    segs = {}
    s0 = rec.begin("conv2_alone")
    rec.gemm(W=w_plain, out=rec.empty(M, C), bias=bias, **common)
    segs[f"conv2 alone({s0.meta[-1]['shape'][-1]})"] = s0
    s1 = rec.begin("unfolded")
    skw = dict(A2=x2, C1=S1, lda=S1, lda2=S2) if S2 else {}
    sc = rec.gemm(A=x1, W=wsc, M=M, N=C, K=Cs, out=rec.empty(M, C), bias=bias, kind="conv1x1", **skw)
    rec.gemm(W=w_plain, out=rec.empty(M, C), bias=bias, R=sc, ldr=C, **common)
    segs[f"1x1 + conv2({s1.meta[-1]['shape'][-1]})"] = s1
    for sk in sks:
        s2 = rec.begin(f"folded_sk{sk}")
        fkw = dict(S2=x2, lds2=S2, S1=S1) if S2 else {}
        rec.gemm(W=w_fold, out=rec.empty(M, C), bias=bias, S=x1, lds=S1, Cs=Cs, splitk=sk, **fkw, **common)
        segs[f"folded sk={sk}({s2.meta[-1]['shape'][-1]})"] = s2
    res = {}
    for rnd in range(3):
        for k, s in segs.items():
            res.setdefault(k, []).append(time_launch_cold(rec, s, stream, 6, thrash, [t for t in (hid, x1, x2) if t is not None])
                                         if cold else time_launch(rec, s, stream, 10))
    line = f"[{M}, {C}, 9*{C}+{S1}{'|' + str(S2) if S2 else ''}]:"
    for k, v in res.items():
        line += f" | {k} {sorted(v)[1]:7.1f} us"
    print(line, flush=True)
