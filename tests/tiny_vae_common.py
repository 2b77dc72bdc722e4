"""Helpers of tests/test_tiny_vae_cpu.py and tests/test_tiny_vae_gpu.py: the fixture (tests/golden/autoencoder_tiny.npz, written by
tools/make_golden.py golden_tiny_vae from the reference class), the synthetic weights both sides regenerate, a float64 restatement of the
decoder written from its layer list, and one launch of bc_tiny_conv3x3 as a problem in NaN-fenced buffers with its float64 reference and
error bound."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.common import g

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 33
BLOCKS = (3, 3, 3, 1)
CASES = ("a", "b", "c")
FORMS = ("in", "block_ab", "block_c", "up", "out")
SIZES = ((3, 5), (9, 33), (17, 8))


def fixture():
    z = np.load(os.path.join(HERE, "golden", "autoencoder_tiny.npz"))
    return z, json.loads(str(z["meta"])), [(k, tuple(v)) for k, v in json.loads(str(z["schema"]))]


def weights():
    from blobctrl_amd import synth
    return synth.synth_state_dict(synth.tiny_vae_param_shapes(), SEED)


def layer_list():
    """(state-dict prefix, form, stage of the output) per convolution, from the architecture: conv_in + ReLU; per stage its blocks of
    conv ReLU conv ReLU conv + skip ReLU; between stages a nearest-2x upsample and a bias-free convolution; a last convolution with bias."""
    out, i = [("decoder.layers.0", "in", 0)], 2
    for s, n in enumerate(BLOCKS):
        for _ in range(n):
            out += [(f"decoder.layers.{i}.conv.{j}", f, s) for j, f in ((0, "a"), (2, "b"), (4, "c"))]
            i += 1
        if s < len(BLOCKS) - 1:
            out.append((f"decoder.layers.{i + 1}", "up", s + 1))
            i += 2
        else:
            out.append((f"decoder.layers.{i}", "out", s))
    return out


def decoder64(sd, z):
    """The decoder in float64: z [B][4][h][w] -> sample [B][3][8h][8w]."""
    w = lambda k: sd[k].double()
    x = torch.tanh(z.double() / 3) * 3
    skip = None
    for name, form, _ in layer_list():
        if form == "up":
            x = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w(name + ".weight"), None, padding=1)
            continue
        y = F.conv2d(x, w(name + ".weight"), w(name + ".bias"), padding=1)
        if form == "out":
            return 2 * y - 1
        if form == "a":
            skip = x
        x = F.relu(y + skip) if form == "c" else F.relu(y)
    raise AssertionError("no output layer")


def quantise64(sample):
    """(bytes [B][H][W][3] uint8, distance of the float value from the nearest rounding boundary) of clamp(v / 2 + 0.5, 0, 1) * 255."""
    q = (sample.double() / 2 + 0.5).clamp(0, 1) * 255
    q = q.permute(0, 2, 3, 1)
    return torch.round(q).to(torch.uint8), (q - torch.floor(q) - 0.5).abs()


# ---------------------------------------------------------------------------------------------------- one launch as a problem
class Problem:
    """One bc_tiny_conv3x3 launch.  H x W is the INPUT size; the `up` form writes 2H x 2W.  Every tensor is fp16-exact (the bias fp32)."""

    def __init__(self, form, B, H, W, seed=5):
        self.form, self.B, self.H, self.W = form, B, H, W
        self.Ci = 4 if form == "in" else 64
        self.Co = 3 if form == "out" else 64
        self.up = form == "up"
        self.Ho, self.Wo = (2 * H, 2 * W) if self.up else (H, W)
        x = g(seed, B, self.Ci, H, W).half()
        if form != "in":
            x = x.clamp(min=0) + 0.25 * g(seed + 1, B, self.Ci, H, W).half()      # (mostly what a ReLU leaves, some negatives)
            x = x.half()
        wt = (g(seed + 2, self.Co, self.Ci, 3, 3) / math.sqrt(9 * self.Ci)).half()
        self.x, self.w = x, wt
        # (the image's bias centres y on 0.5: the bytes then use the whole range and both clamps)
        self.bias = None if self.up else 0.3 * g(seed + 3, self.Co) + (0.5 if form == "out" else 0.0)
        self.skip = g(seed + 4, B, 64, H, W).half() if form == "block_c" else None
        xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if self.up else x.double()
        y = F.conv2d(xin, wt.double(), None if self.bias is None else self.bias.double(), padding=1)
        S = F.conv2d(xin.abs(), wt.double().abs(), None, padding=1)
        if self.skip is not None:
            y, S = y + self.skip.double(), S + self.skip.double().abs()
        if form in ("in", "block_ab", "block_c"):
            y = F.relu(y)
        if form == "out":
            y = 2 * y - 1
        self.ref = y                                                   # [B][Co][Ho][Wo] float64
        # 2^-11 |ref| (the fp16 rounding of the output; dropped for the fp32 image) + 2^-24 (the fp16 subnormal step) + 576 2^-24 S (fp32
        # accumulation of at most 576 products in any order)
        self.bound = (0.0 if form == "out" else 2.0 ** -11) * y.abs() + 2.0 ** -24 + 576 * 2.0 ** -24 * S

    def packed_weight(self):
        """fp16 [Co'][3][3][Ci'] as the module packs it: Ci 4 -> 8 and Co 3 -> 8 with zeros."""
        from blobctrl_amd.weights import pack_conv3x3
        w = self.w.float()
        if self.Co == 3:
            w = torch.cat([w, torch.zeros(5, *w.shape[1:])], 0)
        return pack_conv3x3(w).half()

    def pixels(self, t, pad_to=None):
        """NCHW -> [B * H * W][C] rows (channels padded with zeros to `pad_to`)."""
        B, C, H, W = t.shape
        p = t.permute(0, 2, 3, 1).reshape(B * H * W, C)
        if pad_to and pad_to > C:
            p = torch.cat([p, torch.zeros(p.shape[0], pad_to - C, dtype=p.dtype)], 1)
        return p.contiguous()
