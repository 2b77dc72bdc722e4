"""IP-Adapter masks without a GPU: the new header and op code, the arguments the host wrappers refuse before any launch, the plan
runtime's view of the op, the recorder and engine listings with and without masks, the checks on `ip_adapter_masks`, the mask processor
against the reference's preprocessed masks, the grid formula, and the kernel test inputs' power to see a wrong use of the masks
(tests/ip_masks_common.py)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from blobctrl_amd import _lib, ip_masks
from tests import ip_adapter_common as ipc
from tests import ip_masks_common as mc

HERE = os.path.dirname(os.path.abspath(__file__))
SIG = "ppppiiiiiiiiifppi"


# ---------------------------------------------------------------------------------------------------- ABI and tables
def test_header_declares_op_55_and_the_prototypes():
    inc = os.path.join(HERE, "..", "include")
    text = open(os.path.join(inc, "blobctrl_ip_mask.h")).read()
    assert "enum { BC_OP_ATTENTION_IP_MASKED = BC_OP_IP_END + 1, BC_OP_IP_MASK_END };" in text and '#include "blobctrl_ip.h"' in text
    assert "int bc_attention_ip_masked(const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads, int d," in text
    assert "int images, int tokens_per_image, int ldq, int ldkv, int ldo, float qk_scale, const float* w, const bc_half* mask," in text
    assert "int bc_attention_ip_masked_path(int d, int images, int tokens_per_image, int rows_per_batch, int heads);" in text
    assert "int bc_attention_ip_masked_with(int path," in text and "int bc_ip_mask_downsample(const void* mask, int is_u8, int images," in text
    # the older headers are as they were
    assert "enum { BC_OP_ATTENTION_IP = BC_OP_COUNT, BC_OP_IP_END };" in open(os.path.join(inc, "blobctrl_ip.h")).read()
    assert "BC_OP_COUNT = 53" in open(os.path.join(inc, "blobctrl_hip.h")).read()


def test_op_tables():
    older = (_lib.OPS, _lib.REQUEST_OPS, _lib.SAM_OPS, _lib.SAM_BATCH_OPS, _lib.IP_OPS)
    assert _lib._OP_TABLES == older and _lib._OP_TABLES_BEYOND == (_lib.IP_MASK_OPS,) and _lib.IP_MASK_OPS == {"bc_attention_ip_masked": 55}
    assert list(_lib.IP_SIGNATURES) == ["bc_attention_ip"] and list(_lib.IP_MASK_SIGNATURES) == ["bc_attention_ip_masked"]
    assert list(_lib.IP_MASK_DIRECT_SIGNATURES) == ["bc_ip_mask_downsample", "bc_attention_ip_masked_path", "bc_attention_ip_masked_with"]
    assert _lib.op_code("bc_attention_ip_masked") == 55 and _lib.op_signature("bc_attention_ip_masked") == SIG
    assert _lib.op_code("bc_attention_ip") == 53 and _lib.op_signature("bc_attention_ip") == "ppppiiiiiiiifp"      # the older tables still resolve
    assert _lib.op_code("bc_mask_stats") == 52 and _lib.op_signature("bc_freeu") == "pipiiipippppp"
    for name in list(_lib.IP_MASK_SIGNATURES) + list(_lib.IP_MASK_DIRECT_SIGNATURES):
        assert name not in _lib.EXPORTED_SYMBOLS and not any(name in t for t in _lib._OP_TABLES)
        assert getattr(_lib.load(), name).argtypes is not None
    for name in _lib.IP_MASK_DIRECT_SIGNATURES:                                # direct launches and plain entry points: no op code
        with pytest.raises(KeyError):
            _lib.op_code(name)
    lib = _lib.load()
    # the masked rule: the unmasked rule's measured classes at images x Tp keys where Tp is a multiple of 16, the scalar kernel elsewhere
    for d, heads in ((40, 8), (80, 8), (160, 8), (40, 2), (8, 2), (64, 8)):
        for images, Tp in mc.IMAGES_TP + ((4, 4), (16, 4), (1, 64), (3, 16), (1, 48)):
            want = lib.bc_attention_ip_path(d, images * Tp, 4096, heads) if Tp % 16 == 0 else 0
            assert lib.bc_attention_ip_masked_path(d, images, Tp, 4096, heads) == want, (d, heads, images, Tp)
    assert lib.bc_attention_ip_masked_path(40, 2, 16, 4096, 8) == 1 and lib.bc_attention_ip_masked_path(40, 4, 4, 4096, 8) == 0
    assert lib.bc_attention_ip_masked_path(40, 5, 16, 4096, 8) == 0 and lib.bc_attention_ip_masked_path(40, 0, 16, 4096, 8) == 0


def _call(lib, path=None, **over):
    a = dict(Q=0x1000, K=0x2000, V=0x3000, O=0x4000, B=2, rows=72, heads=8, d=40, images=2, Tp=4, ldq=640, ldkv=320, ldo=320, scale=0.158,
             w=0x5000, mask=0x6000, ldm=80)
    a.update(over)
    args = (a["Q"], a["K"], a["V"], a["O"], a["B"], a["rows"], a["heads"], a["d"], a["images"], a["Tp"], a["ldq"], a["ldkv"], a["ldo"],
            a["scale"], a["w"], a["mask"], a["ldm"], None)
    return lib.bc_attention_ip_masked(*args) if path is None else lib.bc_attention_ip_masked_with(path, *args)


@pytest.mark.parametrize("over,word", [
    (dict(Q=None), b"null"), (dict(K=None), b"null"), (dict(V=None), b"null"), (dict(O=None), b"null"), (dict(w=None), b"null"),
    (dict(mask=None), b"null"), (dict(images=0), b"images=0"), (dict(Tp=0), b"tokens_per_image=0"), (dict(images=5, Tp=13), b"images=5 x tokens_per_image=13"),
    (dict(images=65, Tp=1), b"images=65"), (dict(images=1, Tp=65), b"tokens_per_image=65"), (dict(ldm=71), b"ldm=71"),
    (dict(d=24), b"d=24"), (dict(ldq=312), b"ldq=312"), (dict(ldo=324), b"ldo=324"), (dict(ldkv=312), b"ldkv=312"),
    (dict(Q=0x1008), b"16-byte"), (dict(K=0x2002), b"16-byte"), (dict(V=0x3004), b"16-byte"), (dict(O=0x4008), b"16-byte"),
    (dict(w=0x5002), b"fp32 word"), (dict(mask=0x6001), b"aligned fp16"),
    (dict(B=0), b"B=0"), (dict(rows=0), b"rows_per_batch=0"), (dict(heads=0), b"heads=0"),
])
def test_masked_attention_refuses_bad_arguments_before_any_launch(over, word):
    """Every refusal comes from the host wrapper (the pointers are not device memory: a launch would not return an argument error)."""
    lib = _lib.load()
    assert _call(lib, **over) == 1
    assert b"bc_attention_ip_masked" in lib.bc_last_error() and word in lib.bc_last_error(), lib.bc_last_error()


def test_named_paths_refuse_what_they_cannot_run():
    lib = _lib.load()
    assert _call(lib, path=2) == 1 and b"path=2" in lib.bc_last_error()
    assert _call(lib, path=-1) == 1 and b"path=-1" in lib.bc_last_error()
    assert _call(lib, path=1, Tp=4) == 1 and b"tokens_per_image=4" in lib.bc_last_error()          # path 1 with Tp % 16 != 0
    assert _call(lib, path=1, images=3, Tp=5) == 1 and b"tokens_per_image=5" in lib.bc_last_error()
    for path in (0, 1):                                                       # every other refusal holds for a named path too
        assert _call(lib, path=path, Tp=16, Q=None) == 1 and b"null" in lib.bc_last_error()
        assert _call(lib, path=path, Tp=16, images=5) == 1 and b"images=5 x tokens_per_image=16" in lib.bc_last_error()
        assert _call(lib, path=path, Tp=16, ldm=71) == 1 and b"ldm=71" in lib.bc_last_error()


@pytest.mark.parametrize("over,word", [
    (dict(mask=None), b"null"), (dict(out=None), b"null"), (dict(images=0), b"images=0"), (dict(H=0), b"H=0"), (dict(mh=0), b"mask_h=0"),
    (dict(mh=9), b"fit rows=64"), (dict(ldo=63), b"ldo=63"), (dict(out=0x2001), b"misaligned"), (dict(mask=0x1002), b"misaligned"),
])
def test_downsample_refuses_bad_arguments_before_any_launch(over, word):
    lib = _lib.load()
    a = dict(mask=0x1000, u8=0, images=2, H=64, W=64, mh=8, mw=8, rows=64, out=0x2000, ldo=64)
    a.update(over)
    assert lib.bc_ip_mask_downsample(a["mask"], a["u8"], a["images"], a["H"], a["W"], a["mh"], a["mw"], a["rows"], a["out"], a["ldo"], None) == 1
    assert b"bc_ip_mask_downsample" in lib.bc_last_error() and word in lib.bc_last_error(), lib.bc_last_error()


def test_plan_runtime_takes_the_masked_op_in_process_only(tmp_path):
    """bc_plan_add_op accepts op 55 with its argument count and refuses one fewer; op 54 is still no op; a plan that holds op 55 is not
    written to a file."""
    lib = _lib.load()
    plan = C.c_void_p()
    assert lib.bc_plan_create(C.byref(plan)) == 0
    seg = lib.bc_plan_segment(plan, b"t")
    words = (C.c_uint64 * len(SIG))()
    assert lib.bc_plan_add_op(plan, seg, 0, 55, words, len(SIG)) == 0
    assert lib.bc_plan_add_op(plan, seg, 0, 55, words, len(SIG) - 1) < 0 and b"op 55 takes 17" in lib.bc_last_error()
    assert lib.bc_plan_add_op(plan, seg, 0, 54, words, len(SIG)) < 0 and lib.bc_plan_add_op(plan, seg, 0, 54, words, 14) < 0
    assert lib.bc_plan_add_op(plan, seg, 0, 56, words, len(SIG)) < 0                             # BC_OP_IP_MASK_END is no op either
    assert lib.bc_plan_num_launches(plan, seg) == 1
    buf = (_lib.BcPlanBuffer * 1)()
    buf[0].name, buf[0].address, buf[0].bytes = b"x", 0x1000, 16
    path = str(tmp_path / "ipm.bcplan")
    assert lib.bc_plan_save(plan, path.encode(), buf, 1) != 0 and b"in-process only" in lib.bc_last_error()
    assert not os.path.exists(path)
    assert lib.bc_plan_destroy(plan) == 0


# ---------------------------------------------------------------------------------------------------- recorder, block and engine listings
def test_recorder_records_the_masked_launch_on_the_cpu():
    from blobctrl_amd.launch import Recorder
    rec = Recorder(torch.device("cpu"))
    try:
        seg = rec.begin("t")
        q, kv, o, w = torch.zeros(144, 640).half(), torch.zeros(2, 8, 320).half(), torch.zeros(144, 320).half(), torch.ones(1)
        m = torch.zeros(2, 80).half()
        assert rec.attention_ip_masked(q, kv, kv, o, 2, 72, 8, 40, 2, 4, 640, 320, 320, 40 ** -0.5, w, m, 80) is o
        assert dict(seg.kinds) == {"attention_ip_masked": 1} and seg.meta[0]["variant"] == "attention_ip_masked_kernel<40>"
        assert seg.meta[0]["bytes"] == 2 * (3 * 144 * 320 + 2 * 2 * 8 * 320 + 2 * 72)
        kv32 = torch.zeros(2, 32, 320).half()                                  # two images of 16 tokens: the tiles, named in the listing
        rec.attention_ip_masked(q, kv32, kv32, o, 2, 72, 8, 40, 2, 16, 640, 320, 320, 40 ** -0.5, w, m, 80)
        assert seg.meta[1]["variant"] == "attention_ip_masked_tiles_kernel<40,2>" and seg.meta[1]["kind"] == "attention_ip_masked"
    finally:
        rec.close()


@pytest.mark.parametrize("name", sorted(ipc.IP_BLOCK_CASES))
def test_block_listing_with_masks(name):
    """Recording only: the block made for masks holds the launches of the block made without them, one for one, with attention_ip_masked
    where attention_ip stood, and one mask buffer [images][H W] per adapter."""
    p = ipc.IP_BLOCK_CASES[name]
    rec, seg, _, _ = ipc.ip_block_plan(name, "cpu")
    try:
        plain = [(m["kind"], m["variant"]) for m in seg.meta]
    finally:
        rec.close()
    rec, seg, _, adapters = mc.ip_block_plan_masked(name, "cpu")
    try:
        masked = [(m["kind"], m["variant"]) for m in seg.meta]
        bufs = [{rows: tuple(b.shape) for rows, b in ad.mask_bufs.items()} for ad in adapters]
    finally:
        rec.close()
    assert len(masked) == len(plain) and sum(k == "attention_ip_masked" for k, _ in masked) == len(p["tokens"])
    assert [k for k, _ in masked] == ["attention_ip_masked" if k == "attention_ip" else k for k, _ in plain]
    assert [e for e in masked if e[0] != "attention_ip_masked"] == [e for e in plain if e[0] != "attention_ip"]
    HW = p["H"] * p["W"]
    assert bufs == [{HW: (n, HW)} for n in mc.images_of(p["tokens"])]


def _engine(n_adapters):
    from tests.test_ip_adapter_cpu import _engine as make
    return make(n_adapters)


def _listing(seg):
    return [(m["kind"], m["variant"], m["shape"], m["sid"]) for m in seg.meta]


def test_engine_listings_with_and_without_masks():
    """A compile-only engine on the tiny nets with two adapters, the first with two images.  With masks: a plan of its own whose key
    says "masked" and the images per adapter, the same launch count in every segment with attention_ip_masked where attention_ip stood,
    and the named buffers ip_mask<i>_<rows> for the four attention levels.  Without masks: key, listing and buffers are what they are
    in an engine that never heard of masks."""
    from tests.common import TINY
    args = (1, 8, 8, 7, TINY["ctx"], 3)
    eng = _engine(2)
    plain = eng.plan_for(*args, ip=(2, 1))
    key_plain = list(eng._plans)[-1]
    assert key_plain[-1] == ("ip", 2, (8, ipc.IP_EMBED_DIM), (4, ipc.IP_EMBED_DIM)) and not plain.ip_masked
    assert not any(ad.mask_bufs for ad in plain.ip_adapters)
    masked = eng.plan_for(*args, ip=(2, 1), ip_masked=True)
    key_masked = list(eng._plans)[-1]
    assert masked is not plain and masked.ip_masked and key_masked[:-1] == key_plain and key_masked[-1] == ("ip", "masked", 2, 1)
    assert eng.plan_for(*args, ip=(2, 1), ip_masked=True) is masked and eng.plan_for(*args, ip=(2, 1)) is plain       # both stay cached
    for a, b in ((plain.prologue, masked.prologue), (plain.step_active, masked.step_active), (plain.step_inactive, masked.step_inactive)):
        la, lb = _listing(a), _listing(b)
        assert len(la) == len(lb) and [e[0] for e in lb] == ["attention_ip_masked" if e[0] == "attention_ip" else e[0] for e in la]
        assert [e for e in lb if e[0] != "attention_ip_masked"] == [e for e in la if e[0] != "attention_ip"]
    assert sum(e[0] == "attention_ip_masked" for e in _listing(masked.step_inactive)) == 32
    levels = {128, 32, 8, 2}                                                  # the 8 x 16 canvas and its three halvings
    for i, (ad, n) in enumerate(zip(masked.ip_adapters, (2, 1))):
        assert set(ad.mask_bufs) == levels and all(tuple(b.shape) == (n, rows) and b.dtype == torch.float16 for rows, b in ad.mask_bufs.items())
    assert {f"ip_mask{i}_{rows}" for i in range(2) for rows in levels} <= set(masked.rec.named)
    assert not any(n.startswith("ip_mask") for n in plain.rec.named)
    # an engine that was never asked for masks records what it always recorded
    other = _engine(2).plan_for(*args, ip=(2, 1))
    for a, b in ((plain.prologue, other.prologue), (plain.step_active, other.step_active), (plain.step_inactive, other.step_inactive)):
        assert _listing(a) == _listing(b)
    eng.set_ip_adapters([])                                                   # unload: both adapter plans go
    assert not any(isinstance(x, tuple) for k in eng._plans for x in k)


def test_compile_plan_with_an_adapter_still_raises(tmp_path):
    from tests.common import TINY
    with pytest.raises(NotImplementedError, match="in-process only"):
        _engine(1).compile_plan(str(tmp_path / "x.bcplan"), 1, 8, 8, 7, TINY["ctx"], 3)


# ---------------------------------------------------------------------------------------------------- checks on the masks
def test_mask_checks_follow_the_processor():
    m1, m2 = torch.zeros(1, 1, 16, 16), torch.zeros(1, 2, 16, 16)
    assert [tuple(m.shape) for m in ip_masks.check_masks([m2, m1], [2, 1])] == [(1, 2, 16, 16), (1, 1, 16, 16)]
    legacy = ip_masks.check_masks(torch.zeros(2, 1, 16, 16), [1, 1])           # the legacy form: a tensor [adapters][1][H][W]
    assert [tuple(m.shape) for m in legacy] == [(1, 1, 16, 16)] * 2
    with pytest.raises(ValueError, match=r"Length of ip_adapter_masks array \(1\) must match length of self.scale array \(2\) and number of "
                                         r"ip_hidden_states \(2\)"):
        ip_masks.check_masks([m1], [1, 1])
    for bad in ([m1[0]], [m1.numpy()], [torch.zeros(2, 1, 16, 16)], "masks"):
        with pytest.raises(ValueError, match=r"Each element of the ip_adapter_masks array should be a tensor with shape \[1, "
                                             r"num_images_for_ip_adapter, height, width\]. Please use `IPAdapterMaskProcessor`"):
            ip_masks.check_masks(bad, [1])
    with pytest.raises(ValueError, match=r"Number of masks \(1\) does not match number of ip images \(2\) at index 1"):
        ip_masks.check_masks([m1, m1], [1, 2])


def test_kwargs_split_and_lora_scale_keep_their_behaviour():
    from blobctrl_amd.weights import lora_scale_of
    m = [torch.zeros(1, 1, 8, 8)]
    assert ip_masks.split_kwargs(None) == (None, None) and ip_masks.split_kwargs({}) == ({}, None)
    rest, masks = ip_masks.split_kwargs({"scale": 0.5, "ip_adapter_masks": m})
    assert rest == {"scale": 0.5} and masks is m and lora_scale_of(rest) == 0.5
    rest, masks = ip_masks.split_kwargs({"ip_adapter_masks": m})
    assert rest is None and masks is m and lora_scale_of(rest) == 1.0
    with pytest.raises(ValueError, match="supports only 'scale'.*foo"):
        lora_scale_of({"scale": 0.5, "foo": 1})
    with pytest.raises(ValueError, match="ip_adapter_masks"):                 # whoever does not take the key out first is still refused
        lora_scale_of({"ip_adapter_masks": m})
    rest, _ = ip_masks.split_kwargs({"scale": 0.5, "foo": 1, "ip_adapter_masks": m})
    with pytest.raises(ValueError, match="foo"):
        lora_scale_of(rest)


def test_unet_shell_checks_masks_and_ignores_them_without_an_adapter():
    """UNet2DConditionModel.forward on the CPU shell: with an adapter the masks are checked in front of everything that needs a device;
    without one the key is ignored (the call then fails where every CPU call fails: the library has no CPU path)."""
    from blobctrl_amd.modules import UNet2DConditionModel
    from tests.common import TINY, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    unet = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0], device="cpu", lazy=True)
    x, ehs = torch.zeros(2, 5, 16, 16), torch.zeros(2, 7, TINY["ctx"])
    unet.load_ip_adapter_weights(ipc.tiny_ip_adapter(0))
    e = [torch.zeros(2, 1, ipc.IP_EMBED_DIM)]
    with pytest.raises(ValueError, match="Number of masks"):
        unet(x, 10, ehs, added_cond_kwargs={"image_embeds": e}, cross_attention_kwargs={"ip_adapter_masks": [torch.zeros(1, 2, 16, 16)]})
    with pytest.raises(ValueError, match="Length of ip_adapter_masks array"):
        unet(x, 10, ehs, added_cond_kwargs={"image_embeds": e}, cross_attention_kwargs={"ip_adapter_masks": []})
    with pytest.raises(ValueError, match="foo"):
        unet(x, 10, ehs, added_cond_kwargs={"image_embeds": e}, cross_attention_kwargs={"ip_adapter_masks": [], "foo": 1})
    unet.unload_ip_adapter()
    with pytest.raises(Exception) as info:                                    # no adapter: not a word about the masks
        unet(x, 10, ehs, cross_attention_kwargs={"ip_adapter_masks": "anything"})
    assert "ip_adapter_masks" not in str(info.value) and not isinstance(info.value, ValueError)


# ---------------------------------------------------------------------------------------------------- the mask processor
def test_mask_processor_is_bit_equal_to_the_reference(golden_dir):
    """IPAdapterMaskProcessor.preprocess on the host, PIL and numpy input, against what the reference's preprocess made of the same
    stored uint8 images (tests/golden/pipeline_call_ip_masks.npz), at the stored size and through the lanczos resize to half of it."""
    from PIL import Image
    from blobctrl_amd.image_processor import IPAdapterMaskProcessor
    z = np.load(os.path.join(golden_dir, "pipeline_call_ip_masks.npz"))
    images = mc.call_mask_images()
    mp = IPAdapterMaskProcessor()
    for tag in ("A", "B"):
        assert np.array_equal(z[f"mask_{tag}"], images[tag])
        for name, (h, w) in ((f"pre_{tag}", (64, 128)), (f"pre_{tag}_32x64", (32, 64))):
            ref = z[name]
            for src in (Image.fromarray(z[f"mask_{tag}"]), z[f"mask_{tag}"], Image.fromarray(z[f"mask_{tag}"]).convert("RGB")):
                got = mp.preprocess(src, height=h, width=w)
                assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1, h, w)
                assert np.array_equal(got.reshape(1, 1, h, w).numpy(), ref), name
        assert 0 < z[f"pre_{tag}_32x64"].mean() < 1
    both = mp.preprocess([Image.fromarray(z["mask_A"]), Image.fromarray(z["mask_B"])], height=64, width=128)
    assert tuple(both.shape) == (2, 1, 64, 128)
    stacked = both.reshape(1, both.shape[0], both.shape[2], both.shape[3])     # the caller's stacking: [1][images][H][W]
    assert np.array_equal(stacked[0, 0].numpy(), z["pre_A"][0, 0]) and np.array_equal(stacked[0, 1].numpy(), z["pre_B"][0, 0])
    assert tuple(mp.preprocess(Image.fromarray(z["mask_A"][:61, :125]), None, None).shape) == (1, 1, 56, 120)       # multiples of 8
    with pytest.raises(ValueError, match="incorrect format"):
        mp.preprocess("mask.png")
    with pytest.raises(_lib.BlobCtrlHipError):                                # the device route has no CPU fallback
        mp.preprocess(torch.zeros(64, 128, dtype=torch.uint8), 32, 64)


# ---------------------------------------------------------------------------------------------------- the grid and the restatement
def test_grid_formula_and_float64_restatement_against_the_reference(golden_dir):
    """mask_grid gives the grids of the fixture's cases, warns in the reference's words exactly where the reference warned, and raises
    where the reference divides by zero; the float64 restatement of the launch agrees with the reference's fp32 downsample."""
    z = np.load(os.path.join(golden_dir, "ip_mask_downsample.npz"))
    for H, W, rows in mc.DOWNSAMPLE_CASES:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            grid = ip_masks.mask_grid(rows, H, W)
        warned = [c for c in caught if issubclass(c.category, UserWarning)]
        assert grid == mc.DOWNSAMPLE_GRIDS[(H, W, rows)] and grid[0] * grid[1] <= rows
        assert bool(warned) == bool(z[f"{H}x{W}_{rows}_warned"]) == ((H, W, rows) in mc.DOWNSAMPLE_PADDED)
        if warned:
            assert str(warned[0].message) == ("The aspect ratio of the mask does not match the aspect ratio of the output image. "
                                              "Please update your masks or adjust the output size for optimal performance.")
        ref = z[f"{H}x{W}_{rows}"]
        got = ip_masks.downsample_reference(mc.downsample_masks(H, W), rows)
        err = np.abs(got - ref).max()
        print(f"downsample {H} x {W} -> {rows}: float64 restatement vs the reference's fp32 {err:.2e}, range [{ref.min():.3f}, {ref.max():.3f}]")
        assert got.shape == ref.shape and err <= 4e-6 and not got[:, grid[0] * grid[1]:].any()        # (fp32 coordinates and sums of the reference)
    for rows, H, W in ((1, 64, 128), (3, 8, 64)):
        with pytest.raises(ValueError, match="divides by zero"):
            ip_masks.mask_grid(rows, H, W)
    # the area never exceeds rows: the reference's truncation branch cannot be reached
    for rows in range(1, 300):
        for H, W in ((64, 64), (64, 128), (128, 64), (40, 56), (24, 40), (8, 24)):
            try:
                mh, mw = ip_masks.mask_grid(rows, H, W, warn=False)
            except ValueError:
                continue
            assert 1 <= mh * mw <= rows


# ---------------------------------------------------------------------------------------------------- the kernel test's inputs
@pytest.mark.parametrize("images,Tp", mc.IMAGES_TP)
@pytest.mark.parametrize("heads,d", mc.HEADS_D)
def test_inputs_see_a_wrong_use_of_the_masks(heads, d, images, Tp):
    """From the float64 reference alone, for every weight the GPU test uses: the masks of two images exchanged, one softmax shared by
    all images, and the mask ignored each leave the attention bar on at least half of the rows where a mask is non-zero."""
    q, k, v, o, mask, regions = mc.make_inputs(heads, d, images, Tp)
    bs = mc.block_rows(heads, d)
    assert not mask[:, regions["zero"]].any() and len(regions["zero"]) == bs and bool((mask[:, regions["single"]] != 0).all())
    assert not mask[:, regions["single_zero"]].any() and float(mask.min()) >= mc.MASK_LO and float(mask.max()) <= mc.MASK_HI
    if images > 1:
        assert not mask[images - 1, regions["one_image"]].any() and bool((mask[:images - 1, regions["one_image"]] != 0).all())
    for w in mc.WEIGHTS:
        power = mc.mask_power(q, k, v, o, mask, heads, d, images, Tp, w)
        assert set(power) == ({"ignored", "swapped", "shared"} if images > 1 else {"ignored"}) and min(power.values()) >= 0.5, (w, power)
    prob = mc.Problem("cpu", heads, d, images, Tp, 0.35)
    prob.assert_inside()
    assert prob.q.ld == 2 * heads * d and prob.m.ld == mc.ROWS + 8 and prob.ref.shape == (mc.B * mc.ROWS, heads * d)
