"""Inputs, float64 references and the fenced problem of the IP-Adapter launch bc_attention_ip (tests/test_ip_adapter_gpu.py,
tests/test_ip_adapter_cpu.py).  Nothing here needs a device.

The launch adds w * softmax(scale Q K^T) V over an image's T adapter tokens onto O in place.  The reference is float64 arithmetic on the
launch's own fp16 inputs: O_in + w * attn64.  The bar is the project's attention bar (tests/attention_common.py): the launch rounds once,
at the fp16 store (2^-11 |ref|), and its fp32 dot products, exponentials and sums stay orders of magnitude inside the absolute term.

Inputs that can see a wrong key set: every query carries a component along a sign vector u, and key HEAVY = T - 1 of each image points
along u with a score of about +4, so that one key holds a large share of every row's mass whatever T is.  `key_set_power` shows FROM THE
REFERENCE ALONE that dropping that key, or taking it (K and V row) from the other image, moves at least half of the rows past the bar."""
import math

import torch

from tests import attention_common as ac
from tests import norm_layout_common as nl
from tests import rowchain_stages_common as rc
from tests.common import g

B, ROWS = 2, 72                         # 72 rows: a ragged last row block at every head size (blocks of 32, 30, 20, 15, 7 rows), a block
                                        # boundary at the image boundary
HEADS = (2, 8)
HEAD_DIMS = (8, 40, 80, 160)
TOKENS = (1, 4, 5, 16, 64)
WEIGHTS = (1.0, 0.35, -0.5)
HEAVY_SCORE = 4.0


def make_inputs(heads, d, T, seed=0):
    """fp16 q [B][ROWS][C], k / v [B][T][C], o_in [B][ROWS][C] on the CPU."""
    Cc = heads * d
    q, k, v, o = g(seed + 1, B, ROWS, Cc), g(seed + 2, B, T, Cc), g(seed + 3, B, T, Cc), g(seed + 4, B, ROWS, Cc)
    u, t = ac.sign_vector(d, heads), math.sqrt(10.0 / math.sqrt(d))                 # (t u) . (t u) / sqrt(d) = 10
    q = 0.5 * q + t * u
    k = 0.5 * k
    k[:, T - 1] += (HEAVY_SCORE / 10.0) * t * u
    return q.half(), k.half(), v.half(), o.half()


def reference(q, k, v, o_in, heads, d, w):
    """O_in + w * softmax(d^-0.5 Q K^T) V in float64 from the fp16 inputs: [B][ROWS][C]."""
    return o_in.double() + w * ac.reference(q, k, v, heads, d, d ** -0.5)


def wrong_key_sets(k, v):
    """{name: (k, v)} with the key set wrong by one key: HEAVY dropped (absent when it is the only key), HEAVY taken from the other image."""
    T = k.shape[1]
    out = {}
    if T > 1:
        keep = [t for t in range(T) if t != T - 1]
        out["dropped"] = (k[:, keep], v[:, keep])
    ks, vs = k.clone(), v.clone()
    ks[:, T - 1], vs[:, T - 1] = k.flip(0)[:, T - 1], v.flip(0)[:, T - 1]
    out["other_image"] = (ks, vs)
    return out


def key_set_power(q, k, v, o_in, heads, d, w):
    """{name: share of the B * ROWS rows on which the float64 result with that wrong key set lies outside the bar of the true one}."""
    ref = reference(q, k, v, o_in, heads, d, w)
    bars = ac.bar(ref)
    return {name: float((((reference(q, k2, v2, o_in, heads, d, w) - ref).abs() / bars).amax(-1) > 1.0).double().mean())
            for name, (k2, v2) in wrong_key_sets(k, v).items()}


class Problem:
    """One launch in fenced buffers: Q a strided view (ldq = 2 C, NaN behind column C), K / V with NaN pad columns, O the NaN-fenced
    in-place buffer, the weight one fp32 word between NaN words."""

    def __init__(self, device, heads, d, T, w, seed=0):
        self.heads, self.d, self.T, self.w, self.C = heads, d, T, w, heads * d
        Cc = self.C
        self.cpu = make_inputs(heads, d, T, seed)
        q, k, v, o = self.cpu
        self.q = nl.fence(q.reshape(B * ROWS, Cc), device, ld=2 * Cc)
        self.k = nl.fence(k.reshape(B * T, Cc), device, ld=Cc + 8, guard=1)
        self.v = nl.fence(v.reshape(B * T, Cc), device, ld=Cc + 8, guard=1)
        self.o = nl.InPlace(nl.fence(o.reshape(B * ROWS, Cc), device, ld=Cc + 8))
        self.wdev = rc.fenced_in(torch.tensor([[w]]), device, f32=True, guard=1, align=4)
        self.ref = reference(q, k, v, o, heads, d, w).reshape(B * ROWS, Cc)

    def assert_inside(self):
        for x in (self.q, self.k, self.v):
            nl.inside(x)
        self.o.assert_inside()

    def args(self):
        """The arguments of Recorder.attention_ip."""
        return (self.q.t, self.k.t, self.v.t, self.o.t, B, ROWS, self.heads, self.d, self.T, self.q.ld, self.k.ld, self.o.ld, self.d ** -0.5,
                self.wdev.t)


# ---------------------------------------------------------------------------------------------------- one block with the IP processor
# One Transformer2DModel with IPAdapterAttnProcessor2_0 on attn2 (tests/golden/blocks_ip.npz, tools/make_golden.py golden_blocks_ip), on
# the smallest canvas at which the planner still takes each form: 320 channels from one 64-row block (row-chain; BC_PLAN rowchain=0 gives
# the unfused list on the same fixture), 640 channels from 64 row blocks (row-chain), 1280 channels at HW = 64 (gemm_wreg.hip).  The
# fixture keeps every `sub`-th pixel of the output in both directions.  Outputs only: weights, inputs and tokens come from seeds.
IP_BLOCK_CASES = {
    "ip_320": dict(C=320, heads=8, ctx=768, B=2, H=8, W=16, sub=2, tokens=(4,)),
    "ip_640": dict(C=640, heads=8, ctx=768, B=2, H=32, W=64, sub=16, tokens=(4, 8)),            # two adapters, the second with two images
    "ip_1280": dict(C=1280, heads=8, ctx=768, B=2, H=8, W=8, sub=2, tokens=(8,)),
}
IP_BLOCK_SCALES = {"ip_320": (0.6,), "ip_640": (0.7, 0.4), "ip_1280": (0.6,)}
IP_BLOCK_SEED = 4200
BP = "transformer_blocks.0."


def ip_block_weights(name):
    """(the block's state dict as Transformer2DModel spells it, [(to_k_ip, to_v_ip)] per adapter)."""
    from blobctrl_amd import synth
    from tests.common import block_param_shapes
    p = IP_BLOCK_CASES[name]
    seed = IP_BLOCK_SEED + sorted(IP_BLOCK_CASES).index(name)
    sd = synth.synth_state_dict(block_param_shapes("transformer", p), seed)
    ip = synth.synth_state_dict({f"to_{n}_ip.{i}.weight": (p["C"], p["ctx"]) for i in range(len(p["tokens"])) for n in "kv"}, seed + 50)
    return sd, [(ip[f"to_k_ip.{i}.weight"], ip[f"to_v_ip.{i}.weight"]) for i in range(len(p["tokens"]))]


def ip_block_inputs(name):
    """(x NCHW, text context [B][7][ctx], [image tokens [B][T_i][ctx]] per adapter)."""
    p = IP_BLOCK_CASES[name]
    i = sorted(IP_BLOCK_CASES).index(name)
    x, ctx = g(4300 + i, p["B"], p["C"], p["H"], p["W"]), g(4400 + i, p["B"], 7, p["ctx"])
    return x, ctx, [g(4500 + 10 * i + j, p["B"], T, p["ctx"]) for j, T in enumerate(p["tokens"])]


def ip_block_plan(name, device, scales=None, adapters=True):
    """The block of a case recorded through TrunkPlan on `device` ("cpu": recording only), as tests/test_blocks_gpu.py records its blocks.
    Returns (recorder, segment, output Act, [scale table per adapter])."""
    from blobctrl_amd.engine import Act, IpAdapter, TrunkConfig, TrunkPlan
    from blobctrl_amd.launch import Recorder
    from blobctrl_amd.weights import PackedTrunk
    p = IP_BLOCK_CASES[name]
    dev = torch.device(device)
    sd_block, ip = ip_block_weights(name)
    x, ctx, tokens = ip_block_inputs(name)
    sd = {"blk." + k: v for k, v in sd_block.items()}
    sd["conv_in.weight"] = torch.zeros(8, 4, 3, 3)                      # (PackedTrunk expects a trunk: unused stand-ins)
    sd["none.time_emb_proj.weight"], sd["none.time_emb_proj.bias"] = torch.zeros(8, 1280), torch.zeros(8)
    pw = PackedTrunk(sd, dev, (320, 640, 1280, 1280))
    rec = Recorder(dev)
    seg = rec.begin(name)
    plan = TrunkPlan(rec, pw, TrunkConfig(in_channels=4, num_heads=p["heads"], norm_num_groups=32, cross_attention_dim=p["ctx"]), p["B"], p["H"], p["W"])
    plan.res_events, plan.res_bmod = None, 1
    tables = []
    if adapters:
        scales = IP_BLOCK_SCALES[name] if scales is None else scales
        tables = [torch.tensor([s], dtype=torch.float32, device=dev) for s in scales]
        plan.ip_adapters = [IpAdapter({"blk." + BP: (wk.half().to(dev), wv.half().to(dev))}, tab, tokens=tok.half().to(dev))
                            for (wk, wv), tab, tok in zip(ip, tables, tokens)]
    plan.record_context(ctx.reshape(-1, p["ctx"]).half().to(dev), ctx.shape[1])
    B, C, H, W = x.shape
    out, _ = plan.transformer("blk.", Act(x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous().half().to(dev), C, H, W))
    return rec, seg, out, tables


# ---------------------------------------------------------------------------------------------------- the tiny UNet with adapters
# tests/golden/unet_tiny_ip.npz (tools/make_golden.py golden_ip_adapter), laid out like unet_tiny_freeu.npz: the tiny UNet with seeded
# residual stand-ins on a wide and a square canvas; case -> (geometry, images per adapter).  Adapter i of a case is tiny_ip_adapter(i).
IP_EMBED_DIM = 24
IP_GEOMETRIES = {"wide16": (2, 16, 32), "square16": (2, 16, 16)}
IP_UNET_CASES = {"wide16_one": ("wide16", (1,)), "square16_two": ("square16", (2, 1))}
IP_UNET_SCALES = {"wide16_one": (0.8,), "square16_two": (0.7, 0.5)}
IP_OTHER_FACTOR = 0.4                   # eps_other_scale: every scale times this
IP_RES_SCALE = 0.1


def tiny_ip_adapter(i, seed=4600):
    """Adapter i for the tiny UNet of tests.common in the original layout {"image_proj", "ip_adapter"}: key id 1 + 2 j belongs to the j-th
    attn2 processor in attn_processors order (down, up, mid)."""
    from blobctrl_amd import synth
    from blobctrl_amd.weights import IP_NUM_TOKENS, ip_attn2_prefixes
    from tests.common import TINY, tiny_weights
    usd = tiny_weights()[0]
    ctx = TINY["ctx"]
    proj = synth.synth_state_dict({"proj.weight": (IP_NUM_TOKENS * ctx, IP_EMBED_DIM), "proj.bias": (IP_NUM_TOKENS * ctx,),
                                   "norm.weight": (ctx,), "norm.bias": (ctx,)}, seed + 100 * i)
    shapes = {}
    for j, bp in enumerate(ip_attn2_prefixes(usd.keys())):
        C = usd[bp + "attn2.to_k.weight"].shape[0]
        shapes[f"{1 + 2 * j}.to_k_ip.weight"], shapes[f"{1 + 2 * j}.to_v_ip.weight"] = (C, ctx), (C, ctx)
    return {"image_proj": dict(proj), "ip_adapter": dict(synth.synth_state_dict(shapes, seed + 100 * i + 1))}


def ip_unet_inputs(case):
    """(x [B][5][H][W], text [B][7][ctx], residual seed, [image_embeds [B][n_images][IP_EMBED_DIM]] per adapter) of a case."""
    from tests.common import TINY
    geo, images = IP_UNET_CASES[case]
    B, H, W = IP_GEOMETRIES[geo]
    seed = 7000 + 1000 * sorted(IP_UNET_CASES).index(case)
    return g(seed + 500, B, 5, H, W), g(seed + 501, B, 7, TINY["ctx"]), seed, [g(seed + 510 + i, B, n, IP_EMBED_DIM) for i, n in enumerate(images)]


# ---------------------------------------------------------------------------------------------------- __call__ with an adapter
# tests/golden/pipeline_call_ip.npz (tools/make_golden.py golden_pipeline_call_ip): the case ddim_neg2 of pipeline_call.npz (two images per
# prompt, classifier-free guidance) with tiny_ip_adapter(0) loaded.
IP_CALL_SCALE, IP_CALL_SCALE_OTHER = 1.0, 0.5
IP_CALL_SCALE_DICT = {"down": {"block_1": [0.0, 1.0]}, "up": {"block_2": [0.25, 0.5, 0.75]}, "mid": 0.3}


def ip_call_embeds():
    """`ip_adapter_image_embeds[0]` of the call: [2 = negative, positive][1 image][IP_EMBED_DIM]; the negative half is zero, as the
    reference's own encoder gives it for an image prompt."""
    return torch.cat([torch.zeros(1, 1, IP_EMBED_DIM), 3.0 * g(4700, 1, 1, IP_EMBED_DIM)], 0)
