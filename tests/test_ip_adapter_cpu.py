"""The IP-Adapter launch without a GPU: its place in the op tables, its prototype, the arguments the host wrapper refuses before any launch,
the plan runtime's view of the op, and the test inputs' power to see a wrong key set (tests/ip_adapter_common.py)."""
import ctypes as C
import os

import pytest

from blobctrl_amd import _lib
from tests import ip_adapter_common as ip

HERE = os.path.dirname(os.path.abspath(__file__))
SIG = "ppppiiiiiiiifp"


def test_ip_op_table_extends_the_closed_tables():
    older = (_lib.OPS, _lib.REQUEST_OPS, _lib.SAM_OPS, _lib.SAM_BATCH_OPS)
    assert _lib.IP_OPS == {"bc_attention_ip": 53} and _lib._OP_TABLES == older + (_lib.IP_OPS,)
    codes = sorted(c for t in older for c in t.values())
    assert codes == [c for c in range(53) if c not in (_lib.OP_SIGNAL, _lib.OP_WAIT)]            # the older tables: 0 .. 52, unchanged
    assert not set(_lib.IP_OPS) & {n for t in older for n in t} and not set(_lib.IP_OPS.values()) & set(codes)
    assert len(_lib.OPS) == 36 and len(_lib.REQUEST_OPS) == 4 and len(_lib.SAM_OPS) == 9 and len(_lib.SAM_BATCH_OPS) == 2
    assert "bc_attention_ip" not in _lib.EXPORTED_SYMBOLS and list(_lib.IP_SIGNATURES) == ["bc_attention_ip"]
    assert _lib.op_code("bc_attention_ip") == 53 and _lib.op_signature("bc_attention_ip") == SIG
    assert _lib.op_code("bc_mask_stats") == 52 and _lib.op_signature("bc_freeu") == "pipiiipippppp"         # the older tables still resolve


def test_ip_header_declares_the_op_and_the_prototype():
    inc = os.path.join(HERE, "..", "include")
    text = open(os.path.join(inc, "blobctrl_ip.h")).read()
    assert "enum { BC_OP_ATTENTION_IP = BC_OP_COUNT, BC_OP_IP_END };" in text
    assert "int bc_attention_ip(const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads, int d, int T," in text
    assert "int ldq, int ldkv, int ldo, float qk_scale, const float* w, bc_stream stream);" in text
    assert "#define BC_ATTENTION_IP_MAX_T 64" in text and _lib.ATTENTION_IP_MAX_T == 64
    assert "BC_OP_COUNT = 53" in open(os.path.join(inc, "blobctrl_hip.h")).read()                             # the base enum stays closed


def _call(lib, **over):
    a = dict(Q=0x1000, K=0x2000, V=0x3000, O=0x4000, B=2, rows=72, heads=8, d=40, T=4, ldq=640, ldkv=320, ldo=320, scale=0.158, w=0x5000)
    a.update(over)
    return lib.bc_attention_ip(a["Q"], a["K"], a["V"], a["O"], a["B"], a["rows"], a["heads"], a["d"], a["T"], a["ldq"], a["ldkv"], a["ldo"],
                               a["scale"], a["w"], None)


@pytest.mark.parametrize("over,word", [
    (dict(Q=None), b"null"), (dict(K=None), b"null"), (dict(V=None), b"null"), (dict(O=None), b"null"), (dict(w=None), b"null"),
    (dict(T=0), b"T=0"), (dict(T=65), b"T=65"), (dict(d=24), b"d=24"), (dict(d=0), b"d=0"), (dict(d=128), b"d=128"),
    (dict(ldq=312), b"ldq=312"), (dict(ldo=312), b"ldo=312"), (dict(ldkv=312), b"ldkv=312"),
    (dict(ldq=644), b"ldq=644"), (dict(ldo=324), b"ldo=324"), (dict(ldkv=324), b"ldkv=324"),
    (dict(Q=0x1008), b"16-byte"), (dict(K=0x2002), b"16-byte"), (dict(V=0x3004), b"16-byte"), (dict(O=0x4008), b"16-byte"),
    (dict(B=0), b"B=0"), (dict(rows=0), b"rows_per_batch=0"), (dict(heads=0), b"heads=0"),
])
def test_attention_ip_refuses_bad_arguments_before_any_launch(over, word):
    lib = _lib.load()
    assert _call(lib, **over) == 1
    assert b"bc_attention_ip" in lib.bc_last_error() and word in lib.bc_last_error(), lib.bc_last_error()


def test_plan_runtime_takes_the_ip_op_in_process_only(tmp_path):
    """bc_plan_add_op accepts op 53 with its argument count and refuses one fewer; a plan that holds it is not written to a file."""
    lib = _lib.load()
    plan = C.c_void_p()
    assert lib.bc_plan_create(C.byref(plan)) == 0
    seg = lib.bc_plan_segment(plan, b"t")
    words = (C.c_uint64 * len(SIG))()
    assert lib.bc_plan_add_op(plan, seg, 0, 53, words, len(SIG)) == 0
    assert lib.bc_plan_add_op(plan, seg, 0, 53, words, len(SIG) - 1) < 0 and b"op 53 takes 14" in lib.bc_last_error()
    assert lib.bc_plan_add_op(plan, seg, 0, 54, words, len(SIG)) < 0                               # BC_OP_IP_END is no op
    assert lib.bc_plan_num_launches(plan, seg) == 1
    buf = (_lib.BcPlanBuffer * 1)()
    buf[0].name, buf[0].address, buf[0].bytes = b"x", 0x1000, 16
    path = str(tmp_path / "ip.bcplan")
    assert lib.bc_plan_save(plan, path.encode(), buf, 1) != 0 and b"in-process only" in lib.bc_last_error()
    assert not os.path.exists(path)
    assert lib.bc_plan_destroy(plan) == 0


def test_recorder_records_attention_ip_on_the_cpu():
    """Recorder.attention_ip in a compile-only recorder: one launch of kind attention_ip with the planner's bookkeeping."""
    import torch
    from blobctrl_amd.launch import Recorder
    rec = Recorder(torch.device("cpu"))
    try:
        seg = rec.begin("t")
        q, kv, o, w = torch.zeros(144, 640).half(), torch.zeros(2, 4, 320).half(), torch.zeros(144, 320).half(), torch.ones(1)
        assert rec.attention_ip(q, kv, kv, o, 2, 72, 8, 40, 4, 640, 320, 320, 40 ** -0.5, w) is o
        assert dict(seg.kinds) == {"attention_ip": 1} and seg.meta[0]["variant"] == "attention_ip_kernel<40>"
        assert seg.meta[0]["bytes"] == 2 * (3 * 144 * 320 + 2 * 2 * 4 * 320)
    finally:
        rec.close()


@pytest.mark.parametrize("heads,d,T", [(2, 8, 1), (8, 40, 4), (2, 160, 64), (8, 80, 5)])
def test_inputs_see_a_wrong_key_set(heads, d, T):
    """The float64 result with the heavy key dropped, or taken from the other image, leaves the bar on at least half of the rows for
    every weight the GPU test uses (the GPU test repeats this for each of its cases before it launches)."""
    q, k, v, o = ip.make_inputs(heads, d, T)
    for w in ip.WEIGHTS:
        power = ip.key_set_power(q, k, v, o, heads, d, w)
        assert ("dropped" in power) == (T > 1) and min(power.values()) >= 0.5, (w, power)
    prob = ip.Problem("cpu", heads, d, T, 0.35)
    prob.assert_inside()
    assert prob.q.ld == 2 * heads * d and prob.ref.shape == (ip.B * ip.ROWS, heads * d)


@pytest.mark.parametrize("name,form", [("ip_320", "rowchain"), ("ip_320", "unfused"), ("ip_640", "rowchain"), ("ip_1280", "gw")])
def test_block_listing_with_and_without_an_adapter(name, form, monkeypatch):
    """Recording only: with adapters loaded every form of the block holds one bc_attention_ip per adapter right behind attn2's text
    attention and neither CHAIN_MIDX nor bc_ctx_fold; without one the listing has no such launch and keeps the fused cross-attention."""
    from tests.common import set_plan
    if form == "unfused":
        set_plan(monkeypatch, rowchain=0, gw=0)
    p = ip.IP_BLOCK_CASES[name]
    listings = {}
    for adapters in (False, True):
        rec, seg, _, _ = ip.ip_block_plan(name, "cpu", adapters=adapters)
        try:
            listings[adapters] = [(m["kind"], m["variant"]) for m in seg.meta]
        finally:
            rec.close()
    off, on = listings[False], listings[True]
    fused = lambda ls: any("midx" in v for _, v in ls) or any(k == "ctx_fold" for k, _ in ls)  # noqa: E731
    assert not any(k == "attention_ip" for k, _ in off) and fused(off) == (form != "unfused")
    assert sum(k == "attention_ip" for k, _ in on) == len(p["tokens"]) and not fused(on)
    assert any(k == "rowchain" for k, _ in on) == (form == "rowchain") and any("gemm_wreg_kernel" in v for _, v in on) == (form == "gw")
    first = [k for k, _ in on].index("attention_ip")
    text = on[first - 1]
    assert text[0] == "attention" and [k for k, _ in on[first:first + len(p["tokens"])]] == ["attention_ip"] * len(p["tokens"])
    assert sum(k == "ip_kv" for k, _ in on) == 2 * len(p["tokens"])
    # without the image side and the q the fused forms hide, the rest of the listing is the adapter-less block's with BC_PLAN midx=0 / ctx_fold=0
    set_plan(monkeypatch, midx=0, ctx_fold=0, **(dict(rowchain=0, gw=0) if form == "unfused" else {}))
    rec, seg, _, _ = ip.ip_block_plan(name, "cpu", adapters=False)
    try:
        plain = [(m["kind"], m["variant"]) for m in seg.meta]
    finally:
        rec.close()
    assert [e for e in on if e[0] not in ("attention_ip", "ip_kv")] == plain


# ---------------------------------------------------------------------------------------------------- weights
def test_key_ids_follow_the_reference_processor_order(golden_dir):
    """Key ids 1, 3, 5, ... against the list the reference's loader walked (tests/golden/unet_tiny_ip.npz): names, order and shapes."""
    import numpy as np
    from blobctrl_amd.weights import convert_ip_adapter, ip_attn2_prefixes
    from tests.common import TINY, tiny_weights
    z = np.load(os.path.join(golden_dir, "unet_tiny_ip.npz"))
    usd = tiny_weights()[0]
    prefixes = ip_attn2_prefixes(usd.keys())
    assert [bp + "attn2.processor" for bp in prefixes] == list(z["key_names"]) and len(prefixes) == 16
    sd = ip.tiny_ip_adapter(0)
    conv = convert_ip_adapter(sd, prefixes, TINY["ctx"])
    assert list(conv["kv"]) == prefixes
    for bp, kid, shape in zip(prefixes, z["key_ids"], z["key_shapes"]):
        wk, wv = conv["kv"][bp]
        assert tuple(wk.shape) == tuple(wv.shape) == tuple(shape)
        assert wk.equal(sd["ip_adapter"][f"{kid}.to_k_ip.weight"]) and wv.equal(sd["ip_adapter"][f"{kid}.to_v_ip.weight"])
    assert tuple(conv["proj_w"].shape) == (4 * TINY["ctx"], ip.IP_EMBED_DIM) and tuple(conv["norm_w"].shape) == (TINY["ctx"],)


def test_loader_error_surface(tmp_path):
    import torch
    from blobctrl_amd.checkpoint import load_ip_adapter
    from blobctrl_amd.weights import convert_ip_adapter, ip_attn2_prefixes
    from tests.common import TINY, tiny_weights
    prefixes = ip_attn2_prefixes(tiny_weights()[0].keys())
    good = ip.tiny_ip_adapter(0)
    for keys, word in (({"latents": torch.zeros(1, 16, 8)}, "Plus"), ({"proj.0.weight": 0, "proj.3.weight": 0}, "Full"),
                       ({"perceiver_resampler.proj_in.weight": 0}, "FaceID Plus"), ({"norm.weight": 0, "proj.0.weight": 0}, "FaceID")):
        with pytest.raises(NotImplementedError, match=word):
            convert_ip_adapter(dict(image_proj=keys, ip_adapter=good["ip_adapter"]), prefixes, TINY["ctx"])
    with pytest.raises(NotImplementedError, match="LoRA"):
        convert_ip_adapter(dict(image_proj=good["image_proj"], ip_adapter=dict(good["ip_adapter"], **{"0.to_k_lora.down.weight": 0})), prefixes, TINY["ctx"])
    short = dict(good["ip_adapter"])
    short.pop("31.to_v_ip.weight")
    with pytest.raises(ValueError, match="31.to_v_ip.weight"):
        convert_ip_adapter(dict(image_proj=good["image_proj"], ip_adapter=short), prefixes, TINY["ctx"])
    with pytest.raises(ValueError, match="cross_attention_dim"):
        convert_ip_adapter(good, prefixes, TINY["ctx"] + 8)
    with pytest.raises(NotImplementedError, match="pickle"):
        load_ip_adapter(str(tmp_path / "ip-adapter_sd15.bin"))
    with pytest.raises(ValueError, match="image_proj and ip_adapter"):
        load_ip_adapter({"image_proj": {}})
    assert len(load_ip_adapter([good, good])) == 2 and set(load_ip_adapter(good)[0]) == {"image_proj", "ip_adapter"}


def test_safetensors_file_with_prefixes_loads_like_the_dict(tmp_path):
    from blobctrl_amd.checkpoint import load_ip_adapter, write_safetensors
    good = ip.tiny_ip_adapter(1)
    flat = {f"{part}.{k}": v for part in good for k, v in good[part].items()}
    path = str(tmp_path / "ip-adapter_tiny.safetensors")
    write_safetensors(path, flat)
    (back,) = load_ip_adapter(path)
    assert set(back) == set(good) and all(set(back[p]) == set(good[p]) and all(back[p][k].equal(good[p][k]) for k in good[p]) for p in good)


# ---------------------------------------------------------------------------------------------------- the loop engine, recording only
def _engine(n_adapters=0):
    import torch
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.weights import convert_ip_adapter, ip_adapter_on_device, ip_attn2_prefixes
    from tests.common import TINY, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True)
    prefixes = ip_attn2_prefixes(usd.keys())
    eng.set_ip_adapters([ip_adapter_on_device(convert_ip_adapter(ip.tiny_ip_adapter(i), prefixes, TINY["ctx"]), torch.device("cpu"))
                         for i in range(n_adapters)])
    return eng


def _listing(seg, drop=()):
    return [(m["kind"], m["variant"], m["shape"], m["sid"]) for m in seg.meta if m["kind"] not in drop]


def _count(seg, name):
    return sum(name in (m["variant"] or "") or m["kind"] == name for m in seg.meta)


def test_engine_listings_with_none_one_and_two_adapters(tmp_path, monkeypatch):
    """A compile-only engine on the tiny nets.  Without an adapter the plan is the one an engine records that never heard of adapters
    (also after a load and unload); with one adapter every UNet forward holds 16 bc_attention_ip launches and neither bc_rowchain_midx
    nor bc_ctx_fold, with two 32; BlobNet's launches are unchanged; what is left of the UNet's listing is the adapter-less one of
    BC_PLAN midx=0 / ctx_fold=0, launch for launch; compile_plan with an adapter loaded raises."""
    from tests.common import TINY, set_plan
    args = (1, 8, 8, 7, TINY["ctx"], 3)
    plain = _engine().plan_for(*args)
    assert not plain.ip_embeds and _count(plain.step_inactive, "attention_ip") == 0
    ip_kinds = ("attention_ip", "ip_kv", "ip_proj")
    blob = lambda P: [e for e in _listing(P.step_active) if e[3] == 1]
    for n in (1, 2):
        eng = _engine(n)
        with pytest.raises(NotImplementedError, match="in-process only"):
            eng.compile_plan(str(tmp_path / "x.bcplan"), *args)
        P = eng.plan_for(*args, ip=(1,) * n)
        key = list(eng._plans)[-1]
        assert key[-1] == ("ip", n) + ((4, ip.IP_EMBED_DIM),) * n and [tuple(e.shape) for e in P.ip_embeds] == [(2, ip.IP_EMBED_DIM)] * n
        for seg in (P.step_active, P.step_inactive):
            assert _count(seg, "attention_ip") == 16 * n and _count(seg, "midx") == 0 and _count(seg, "ctx_fold") == 0
        assert _count(P.prologue, "ip_proj") == n and _count(P.prologue, "ip_kv") == 32 * n and _count(P.prologue, "layernorm") >= n
        assert blob(P) == blob(plain)
        # two images for the first adapter: a plan of its own (8 tokens), the same launches
        P2 = eng.plan_for(*args, ip=(2,) + (1,) * (n - 1))
        assert P2 is not P and list(eng._plans)[-1][-1][2] == (8, ip.IP_EMBED_DIM) and _count(P2.step_inactive, "attention_ip") == 16 * n
        # unload: the adapter plans go, the adapter-less plan is the plain one
        eng.set_ip_adapters([])
        assert not any(isinstance(x, tuple) for k in eng._plans for x in k)
        back = eng.plan_for(*args)
        for a, b in ((back.prologue, plain.prologue), (back.step_active, plain.step_active), (back.step_inactive, plain.step_inactive)):
            assert _listing(a) == _listing(b)
    one = _engine(1).plan_for(*args, ip=(1,))
    set_plan(monkeypatch, midx=0, ctx_fold=0)
    unfused = _engine().plan_for(*args)
    for a, b in ((one.step_active, unfused.step_active), (one.step_inactive, unfused.step_inactive)):
        assert _listing(a, drop=ip_kinds) == _listing(b)


def test_engine_checks_the_image_embeddings():
    import torch
    eng = _engine(1)
    e = torch.zeros(2, 1, ip.IP_EMBED_DIM)
    assert eng._ip_layout([e], 2, 1, False)[0] == (1,) and eng._ip_layout([e[:1]], 2, 1, True)[1][0].shape[0] == 2
    for bad, word in (([e[:1]], "UNet batch"), ([e, e], "one tensor per loaded"), (e, "one tensor per loaded"), ([e[..., :8]], "embed"),
                      (None, "are loaded")):
        with pytest.raises(ValueError, match=word):
            eng._ip_layout(bad, 2, 1, False)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        _engine()._ip_layout([e], 2, 1, False)


def test_pipeline_scale_expansion_and_input_checks(golden_dir):
    """set_ip_adapter_scale's expansion for a float, a list and the per-block dict against the per-processor lists the reference ended up
    with (tests/golden/pipeline_call_ip.npz); check_inputs and prepare_ip_adapter_image_embeds as pipe:422-436 / the vendored function."""
    import types
    import numpy as np
    import torch
    from blobctrl_amd.modules import UNet2DConditionModel
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline as Pipe
    from tests.common import tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    z = np.load(os.path.join(golden_dir, "pipeline_call_ip.npz"))
    unet = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0], device="cpu", lazy=True)
    unet.load_ip_adapter_weights(ip.tiny_ip_adapter(0))
    stub = types.SimpleNamespace(unet=unet, _engine=None)
    stub.ip_adapter_scale_lists = types.MethodType(Pipe.ip_adapter_scale_lists, stub)
    for tag, arg in (("float", ip.IP_CALL_SCALE), ("list", [ip.IP_CALL_SCALE_OTHER]), ("dict", ip.IP_CALL_SCALE_DICT)):
        Pipe.set_ip_adapter_scale(stub, arg)
        assert unet.__dict__["ip_adapters"][0]["scales"].tolist() == [float(np.float32(v)) for v in z[f"scales_{tag}"]], tag
    assert len(set(z["scales_dict"].tolist())) > 4
    with pytest.raises(ValueError, match="Cannot assign 2 scale_configs to 1 IP-Adapter"):
        Pipe.set_ip_adapter_scale(stub, [1.0, 0.5])
    with pytest.raises(ValueError, match="Expected 3 scales for up.block_1, got 2"):
        Pipe.set_ip_adapter_scale(stub, {"up": {"block_1": [1.0, 0.5]}})
    Pipe.unload_ip_adapter(stub)
    assert unet.config.encoder_hid_dim_type is None and not unet.__dict__["ip_adapters"]
    ok = dict(prompt="a", callback_steps=None)
    e = torch.zeros(2, 1, ip.IP_EMBED_DIM)
    stub._callback_tensor_inputs = ["latents"]
    with pytest.raises(ValueError, match="Provide either `ip_adapter_image` or `ip_adapter_image_embeds`"):
        Pipe.check_inputs(stub, ip_adapter_image=object(), ip_adapter_image_embeds=[e], **ok)
    with pytest.raises(ValueError, match="has to be of type `list`"):
        Pipe.check_inputs(stub, ip_adapter_image_embeds=e, **ok)
    with pytest.raises(ValueError, match="3D or 4D tensors but is 2D"):
        Pipe.check_inputs(stub, ip_adapter_image_embeds=[e[0]], **ok)
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
        Pipe.check_inputs(stub, ip_adapter_image=object(), **ok)
    Pipe.check_inputs(stub, ip_adapter_image_embeds=[e], **ok)
    (out,) = Pipe.prepare_ip_adapter_image_embeds(stub, None, [torch.arange(2.0).view(2, 1, 1)], "cpu", 3, True)
    assert out.flatten().tolist() == [0.0] * 3 + [1.0] * 3
    (out,) = Pipe.prepare_ip_adapter_image_embeds(stub, None, [torch.arange(2.0).view(2, 1, 1)], "cpu", 2, False)
    assert out.flatten().tolist() == [0.0, 1.0, 0.0, 1.0]
