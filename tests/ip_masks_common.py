"""Inputs, float64 references, fenced problems and fixture cases of the IP-Adapter masks (tests/test_ip_masks_cpu.py,
tests/test_ip_masks_gpu.py, tools/make_golden.py).  Nothing here needs a device.

bc_attention_ip_masked adds w * sum_i m[i, r] * softmax_i(scale Q K_i^T) V_i onto O in place: one softmax per image over that image's Tp
keys, weighted row by row with the image's mask.  The reference is float64 arithmetic on the launch's own fp16 inputs (mask included).  The
bar is the project's attention bar (tests/attention_common.py), the one bc_attention_ip is held to: the launch rounds once, at the fp16
store; the extra multiply by m[i, r] / l_i and the sum over images are fp32.

The masks are drawn in [-0.4, 1.3] - the range bicubic downsampling of a 0 / 1 mask reaches - with three special regions laid on the row
blocks of the kernel (`block_rows`): block 0 exactly zero for every image; block 1 zero for the LAST image only; the last (ragged) block
zero but for one row.  `mask_power` shows FROM THE REFERENCE ALONE that a mask applied to the wrong image, one softmax shared by all
images, and an ignored mask each move at least half of the rows with a non-zero mask past the bar."""
import numpy as np
import torch

from tests import attention_common as ac
from tests import ip_adapter_common as ipc
from tests import norm_layout_common as nl
from tests import rowchain_stages_common as rc
from tests.common import g

B, ROWS = ipc.B, ipc.ROWS               # 2 x 72 rows: the ragged count of the unmasked test
HEADS_D = ((2, 8), (8, 40), (8, 80), (8, 160))
IMAGES_TP = ((1, 4), (2, 4), (3, 5), (1, 16), (2, 16), (4, 16), (2, 32))
HEADS_D_MORE = ((2, 16), (2, 32), (2, 64))                              # the other head sizes the masked kernels are built for,
IMAGES_TP_MORE = ((3, 5), (2, 16))                                      # ... at a ragged Tp and at one both kernels take (block_rows = 32)
WEIGHTS = ipc.WEIGHTS
MASK_LO, MASK_HI = -0.4, 1.3


def block_rows(heads, d):
    """Rows of one image a workgroup of the scalar kernel takes (csrc/bc_attention_ip.h ip_scalar_geometry: about 5 items per lane group,
    at most 32 rows, all heads in one slab at these sizes): 32, 30, 15 and 7 rows for HEADS_D, 32 for HEADS_D_MORE."""
    per_pass = 4 * (64 // (d // 8))
    return max(1, min(32, 5 * per_pass // heads))


def make_mask(heads, d, images, seed=0):
    """fp16 [images][ROWS]: uniform in [MASK_LO, MASK_HI] with the three special regions.  Returns (mask, {region: rows})."""
    bs = block_rows(heads, d)
    assert 2 * bs <= ROWS
    rng = np.random.Generator(np.random.PCG64(9100 + seed))
    m = torch.from_numpy(rng.uniform(MASK_LO, MASK_HI, size=(images, ROWS)).astype(np.float32)).half()
    assert bool((m != 0).all())
    last0 = (ROWS - 1) // bs * bs
    single = last0 + (ROWS - last0) // 2
    m[:, :bs] = 0
    if images > 1:
        m[images - 1, bs:2 * bs] = 0
    keep = m[:, single].clone()
    m[:, last0:] = 0
    m[:, single] = keep
    regions = dict(zero=list(range(bs)), one_image=list(range(bs, 2 * bs)) if images > 1 else [],
                   single_zero=[r for r in range(last0, ROWS) if r != single], single=[single])
    return m, regions


def make_inputs(heads, d, images, Tp, seed=0):
    """fp16 q, k, v, o_in as tests/ip_adapter_common.py makes them for T = images * Tp keys, with a heavy key at the end of EVERY image, and
    the mask."""
    q, k, v, o = ipc.make_inputs(heads, d, images * Tp, seed)
    k = k.float()
    u, t = ac.sign_vector(d, heads), (10.0 / d ** 0.5) ** 0.5
    for i in range(images - 1):                                          # (ipc.make_inputs made the last key of all heavy already)
        k[:, i * Tp + Tp - 1] += (ipc.HEAVY_SCORE / 10.0) * t * u
    mask, regions = make_mask(heads, d, images, seed)
    return q, k.half(), v, o, mask, regions


def attention_per_image(q, k, v, heads, d, images, Tp):
    """float64 [images][B][ROWS][C]: softmax(d^-0.5 Q K_i^T) V_i of every image."""
    return torch.stack([ac.reference(q, k[:, i * Tp:(i + 1) * Tp], v[:, i * Tp:(i + 1) * Tp], heads, d, d ** -0.5) for i in range(images)])


def reference(q, k, v, o_in, mask, heads, d, images, Tp, w):
    """O_in + w * sum_i m[i, r] * attention_i in float64 from the fp16 inputs: [B][ROWS][C]."""
    a = attention_per_image(q, k, v, heads, d, images, Tp)
    return o_in.double() + w * (mask.double()[:, None, :, None] * a).sum(0)


def mask_power(q, k, v, o_in, mask, heads, d, images, Tp, w):
    """{name: share of the rows with a non-zero mask (of any image; counted per batch element) on which a wrong computation lies outside
    the bar of the true one}: `swapped` - the masks of images 0 and 1 exchanged (two images at least); `shared` - one softmax over all
    images' keys, times the mean mask (two images at least); `ignored` - the mask taken as 1 (per-image softmax, summed)."""
    ref = reference(q, k, v, o_in, mask, heads, d, images, Tp, w)
    bars = ac.bar(ref)
    rows = (mask != 0).any(0)
    wrong = {"ignored": reference(q, k, v, o_in, torch.ones_like(mask), heads, d, images, Tp, w)}
    if images > 1:
        sw = mask.clone()
        sw[0], sw[1] = mask[1], mask[0]
        wrong["swapped"] = reference(q, k, v, o_in, sw, heads, d, images, Tp, w)
        wrong["shared"] = o_in.double() + w * mask.double().mean(0)[None, :, None] * ac.reference(q, k, v, heads, d, d ** -0.5)
    return {n: float((((x - ref).abs() / bars).amax(-1) > 1.0)[:, rows].double().mean()) for n, x in wrong.items()}


class Problem:
    """One launch in fenced buffers, as tests/ip_adapter_common.py Problem builds them: Q a strided view (ldq = 2 C, NaN behind column C),
    K / V with NaN pad columns, O the NaN-fenced in-place buffer, the weight one fp32 word between NaN words, the mask fp16
    [images][ldm = ROWS + 8] with NaN pad columns and NaN guard rows."""

    def __init__(self, device, heads, d, images, Tp, w, seed=0):
        self.heads, self.d, self.images, self.Tp, self.w, self.C = heads, d, images, Tp, w, heads * d
        Cc, T = self.C, images * Tp
        q, k, v, o, mask, self.regions = self.cpu = make_inputs(heads, d, images, Tp, seed)
        self.q = nl.fence(q.reshape(B * ROWS, Cc), device, ld=2 * Cc)
        self.k = nl.fence(k.reshape(B * T, Cc), device, ld=Cc + 8, guard=1)
        self.v = nl.fence(v.reshape(B * T, Cc), device, ld=Cc + 8, guard=1)
        self.o = nl.InPlace(nl.fence(o.reshape(B * ROWS, Cc), device, ld=Cc + 8))
        self.wdev = rc.fenced_in(torch.tensor([[w]]), device, f32=True, guard=1, align=4)
        self.m = nl.fence(mask, device, ld=ROWS + 8, guard=1)
        self.o_in = o.reshape(B * ROWS, Cc)
        self.ref = reference(q, k, v, o, mask, heads, d, images, Tp, w).reshape(B * ROWS, Cc)

    def assert_inside(self):
        for x in (self.q, self.k, self.v, self.m):
            nl.inside(x)
        self.o.assert_inside()

    def args(self):
        """The arguments of Recorder.attention_ip_masked, and of bc_attention_ip_masked(_with) once tensors are pointers."""
        return (self.q.t, self.k.t, self.v.t, self.o.t, B, ROWS, self.heads, self.d, self.images, self.Tp, self.q.ld, self.k.ld, self.o.ld,
                self.d ** -0.5, self.wdev.t, self.m.t, self.m.ld)

    def rows_of(self, region):
        """Rows of O (over both batch elements) that belong to a mask region."""
        return [b * ROWS + r for b in range(B) for r in self.regions[region]]


# ---------------------------------------------------------------------------------------------------- the downsampling
# tests/golden/ip_mask_downsample.npz (tools/make_golden.py golden_ip_mask_downsample): (H, W, rows) of every case; the last two pad.
DOWNSAMPLE_CASES = ([(64, 64, r) for r in (64, 16, 4, 1)] + [(64, 128, r) for r in (128, 32, 8, 2)] + [(40, 56, 35), (24, 40, 15)] +
                    [(64, 64, 128), (64, 128, 64)])
DOWNSAMPLE_PADDED = ((64, 64, 128), (64, 128, 64))
DOWNSAMPLE_GRIDS = {(64, 64, 64): (8, 8), (64, 64, 16): (4, 4), (64, 64, 4): (2, 2), (64, 64, 1): (1, 1), (64, 128, 128): (8, 16),
                    (64, 128, 32): (4, 8), (64, 128, 8): (2, 4), (64, 128, 2): (1, 2), (40, 56, 35): (5, 7), (24, 40, 15): (3, 5),
                    (64, 64, 128): (12, 10), (64, 128, 64): (6, 10)}


def ellipse(H, W, cy, cx, ry, rx):
    """uint8 0 / 1 [H][W]: pixel centres inside the ellipse (centre and radii as fractions of the frame)."""
    y, x = np.mgrid[0:H, 0:W]
    return ((((y + 0.5) / H - cy) / ry) ** 2 + (((x + 0.5) / W - cx) / rx) ** 2 <= 1.0).astype(np.uint8)


def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[int(round(y0 * H)):int(round(y1 * H)), int(round(x0 * W)):int(round(x1 * W))] = 1
    return m


def downsample_masks(H, W):
    """The two 0 / 1 masks [2][H][W] every downsampling case runs on: an off-centre ellipse and a rectangle that touches two borders."""
    return np.stack([ellipse(H, W, 0.45, 0.4, 0.3, 0.22), rect(H, W, 0.0, 0.6, 0.55, 1.0)])


# ---------------------------------------------------------------------------------------------------- blocks, tiny UNet, __call__
# tests/golden/blocks_ip_masks.npz (golden_blocks_ip_masks): the block cases of tests/ip_adapter_common.py IP_BLOCK_CASES, every adapter's
# tokens split into images of 4 tokens - ip_320: one adapter, one image; ip_640: two adapters, the second with two images; ip_1280: one
# adapter with two images.  Masks are 0 / 1 at 64 rows and the canvas' aspect ratio.
BLOCK_MASK_ROWS = 64
SHAPES = (lambda H, W: ellipse(H, W, 0.5, 0.3, 0.38, 0.24), lambda H, W: rect(H, W, 0.35, 0.9, 0.55, 0.95),
          lambda H, W: rect(H, W, 0.0, 0.3, 0.1, 0.9))          # (pairwise disjoint: swapping two of them moves every covered pixel)


def images_of(tokens):
    return tuple(T // 4 for T in tokens)


def _masks(images, H, W, first=0):
    """[fp32 [1][n][H][W]] per adapter; every image another shape of SHAPES."""
    out, s = [], first
    for n in images:
        out.append(torch.from_numpy(np.stack([SHAPES[(s + j) % len(SHAPES)](H, W) for j in range(n)])[None].astype(np.float32)))
        s += n
    return out


def swap_images(masks):
    """The same list with the masks of the first two images exchanged in every adapter that has two."""
    return [m[:, [1, 0] + list(range(2, m.shape[1]))] if m.shape[1] > 1 else m for m in masks]


def block_masks(name):
    p = ipc.IP_BLOCK_CASES[name]
    return _masks(images_of(p["tokens"]), BLOCK_MASK_ROWS, BLOCK_MASK_ROWS * p["W"] // p["H"])


def block_has_swap(name):
    return any(n > 1 for n in images_of(ipc.IP_BLOCK_CASES[name]["tokens"]))


def ip_block_plan_masked(name, device):
    """tests/ip_adapter_common.py ip_block_plan with every adapter made for masks.  Returns (recorder, segment, output Act, adapters)."""
    from blobctrl_amd.engine import Act, IpAdapter, TrunkConfig, TrunkPlan
    from blobctrl_amd.launch import Recorder
    from blobctrl_amd.weights import PackedTrunk
    p = ipc.IP_BLOCK_CASES[name]
    dev = torch.device(device)
    sd_block, ip = ipc.ip_block_weights(name)
    x, ctx, tokens = ipc.ip_block_inputs(name)
    sd = {"blk." + k: v for k, v in sd_block.items()}
    sd["conv_in.weight"] = torch.zeros(8, 4, 3, 3)                      # (PackedTrunk expects a trunk: unused stand-ins)
    sd["none.time_emb_proj.weight"], sd["none.time_emb_proj.bias"] = torch.zeros(8, 1280), torch.zeros(8)
    pw = PackedTrunk(sd, dev, (320, 640, 1280, 1280))
    rec = Recorder(dev)
    seg = rec.begin(name)
    plan = TrunkPlan(rec, pw, TrunkConfig(in_channels=4, num_heads=p["heads"], norm_num_groups=32, cross_attention_dim=p["ctx"]), p["B"], p["H"], p["W"])
    plan.res_events, plan.res_bmod = None, 1
    plan.ip_adapters = [IpAdapter({"blk." + ipc.BP: (wk.half().to(dev), wv.half().to(dev))}, torch.tensor([s], dtype=torch.float32, device=dev),
                                  tokens=tok.half().to(dev), n_images=tok.shape[1] // 4, num_tokens=4, masked=True, mask_name=f"ip_mask{i}")
                        for i, ((wk, wv), s, tok) in enumerate(zip(ip, ipc.IP_BLOCK_SCALES[name], tokens))]
    plan.record_context(ctx.reshape(-1, p["ctx"]).half().to(dev), ctx.shape[1])
    Bn, C, H, W = x.shape
    out, _ = plan.transformer("blk.", Act(x.permute(0, 2, 3, 1).reshape(Bn, H * W, C).contiguous().half().to(dev), C, H, W))
    return rec, seg, out, plan.ip_adapters


# tests/golden/unet_tiny_ip_masks.npz (golden_unet_ip_masks): the cases of IP_UNET_CASES with masks at the image resolution (8 x the
# latent canvas).
def unet_masks(case):
    geo, images = ipc.IP_UNET_CASES[case]
    _, H, W = ipc.IP_GEOMETRIES[geo]
    return _masks(images, 8 * H, 8 * W, first=1)


# tests/golden/pipeline_call_ip_masks.npz (golden_pipeline_call_ip_masks): the call of pipeline_call_ip.npz with masks.  The UNet of this
# pipeline runs on a canvas twice as wide as the image (two 8 x 8 latent frames side by side), so the stored uint8 mask images are 64 x 128
# - the canvas' aspect ratio - and go through IPAdapterMaskProcessor.preprocess(mask, 64, 128).
def call_mask_images():
    """{"A": uint8 [64][128] 0 / 255, "B": ...}: A an ellipse on the right frame, B a rectangle on the left one."""
    return {"A": 255 * ellipse(64, 128, 0.5, 0.75, 0.32, 0.17), "B": 255 * rect(64, 128, 0.1, 0.7, 0.05, 0.4)}
