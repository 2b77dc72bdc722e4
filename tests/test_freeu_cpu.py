"""FreeU, host side: the closed form of fourier_filter(threshold=1) against torch.fft, the frequency list and basis table the kernel
reads, what a compiled plan launches with FreeU on (six BC_OP_FREEU records per UNet forward, directly in front of the resnets of
up_blocks.0 / up_blocks.1, in a version-7 file) and off (the listing it always had), and the public surface: enable_freeu / disable_freeu
on the UNet module and the pipeline, the truthiness rule, torch.ops.blobctrl.freeu's fake kernel, the exported symbol."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests.common import TINY, build_plan_dump, plan_named as _named, plan_stored as _stored, tiny_weights

OP_GEMM, OP_GN_STATS, OP_FREEU = 0, 1, 37
FREEU = (0.9, 0.2, 1.5, 1.6)
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)
SIZES = [(4, 8), (8, 16), (3, 6), (6, 12), (1, 2), (2, 4), (12, 24), (5, 7), (2, 2)]


# ------------------------------------------------------------------------------------------------------------ the closed form
def fourier_filter_fft(x, scale):
    """fourier_filter(x, threshold=1, scale) restated with torch.fft in the dtype of x: fftn, fftshift, the mask box
    [H // 2 - 1, H // 2 + 1) x [W // 2 - 1, W // 2 + 1) set to `scale`, ifftshift, ifftn, .real."""
    B, C, H, W = x.shape
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(B, C, H, W, dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - 1:crow + 1, ccol - 1:ccol + 1] = scale
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real


def fourier_filter_closed(x, scale):
    """out = x + (s - 1) / (H W) sum_k (A_k cos_k + S_k sin_k) in float64 over the engine's own basis table (what bc_freeu computes)."""
    from blobctrl_amd.engine import freeu_basis
    B, C, H, W = x.shape
    basis = freeu_basis(H, W).reshape(H * W, 8)
    v = x.reshape(B, C, H * W).to(torch.float64)
    return (v + (scale - 1.0) / (H * W) * ((v @ basis) @ basis.T)).reshape(B, C, H, W)


@pytest.mark.parametrize("H,W", SIZES)
def test_closed_form_equals_the_fft_filter(H, W):
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(100 * H + W)) + 0.7      # (a DC offset)
    for s in (0.9, 0.2):
        want, got = fourier_filter_fft(x, s), fourier_filter_closed(x, s)
        scale = want.abs().max().item()
        assert (got - want).abs().max().item() <= 1e-9 * scale, (H, W, s)
        assert (want - x).abs().max().item() > (0.05 if s == 0.9 else 0.5)              # (the filter is no identity at these sizes)


def test_frequency_list_is_a_set_and_the_basis_is_exact():
    from blobctrl_amd.engine import freeu_basis, freeu_frequencies
    assert freeu_frequencies(1, 2) == [(0, 0), (0, 1)] and freeu_frequencies(1, 1) == [(0, 0)]          # H = 1: one row index, not two
    assert freeu_frequencies(2, 2) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert freeu_frequencies(4, 8) == [(0, 0), (0, 7), (3, 0), (3, 7)] and freeu_frequencies(3, 1) == [(0, 0), (2, 0)]
    for H, W in SIZES + [(24, 48), (1, 1)]:
        b = freeu_basis(H, W)
        fr = freeu_frequencies(H, W)
        assert b.shape == (H * W, 4, 2) and b.dtype == torch.float64 and len(set(fr)) == len(fr) <= 4
        assert not b[:, len(fr):].any()                                                               # unused pairs: zero rows
        assert (b[:, 0, 0] == 1).all() and not b[:, 0, 1].any()                                       # DC: cos = 1, no sine
        y, x = torch.arange(H * W) // W, torch.arange(H * W) % W
        for k, (ky, kx) in enumerate(fr):
            th = 2 * np.pi * (ky * y.double() / H + kx * x.double() / W)
            assert (b[:, k, 0] - torch.cos(th)).abs().max() < 1e-13 and (b[:, k, 1] - torch.sin(th)).abs().max() < 1e-13
    # an undeduplicated list would count H = 1 twice: the closed form then misses the fft filter by the filter's own effect
    x = torch.randn(1, 1, 1, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) + 0.7
    assert (fourier_filter_closed(x, 0.2) - fourier_filter_fft(x, 0.2)).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------------------ compiled plans
@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("dump")


@pytest.fixture(scope="module")
def plan_dump(dump_dir):
    return build_plan_dump(dump_dir)


def _engine(**kw):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    return BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True, max_cached_plans=16, **kw)


def _version(path):
    return struct.unpack("<I", open(path, "rb").read()[4:8])[0]


def _listing_hash(dump_dir, path):
    r = subprocess.run([os.path.join(str(dump_dir), "plan_dump"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    return hashlib.sha256(r.stdout.encode()).hexdigest()


def _resnet_log(monkeypatch):
    """Every TrunkPlan.resnet call as (is BlobNet, block prefix, launches recorded in the segment before it)."""
    from blobctrl_amd import engine
    log, orig = [], engine.TrunkPlan.resnet

    def resnet(self, p, *a, **k):
        log.append((self.cfg.is_blobnet, p, self.rec.seg.name, len(self.rec.seg.meta)))
        return orig(self, p, *a, **k)
    monkeypatch.setattr(engine.TrunkPlan, "resnet", resnet)
    return log


def _check_sites(P, log, forwards_per_segment=1):
    """Six freeu launches per UNet forward, each the launch directly in front of up_blocks.{0,1}.resnets.{0,1,2} of the UNet and nowhere else."""
    for seg in (P.step_active, P.step_inactive):
        kinds = [m["kind"] for m in seg.meta]
        sites = [n for blob, p, name, n in log if name == seg.name and not blob and p.startswith(("up_blocks.0.", "up_blocks.1."))]
        assert len(sites) == 6 * forwards_per_segment and kinds.count("freeu") == len(sites), (seg.name, sites)
        assert all(kinds[n - 1] == "freeu" for n in sites)
        others = [n for blob, p, name, n in log if name == seg.name and n not in sites]
        assert others and all(n == 0 or kinds[n - 1] != "freeu" for n in others)
        stages = [m["shape"][5] for m in seg.meta if m["kind"] == "freeu"]
        assert stages == [0, 0, 0, 1, 1, 1] * forwards_per_segment
        assert all(m["sid"] != 1 for m in seg.meta if m["kind"] == "freeu")                 # never on BlobNet's stream
    assert "freeu" not in [m["kind"] for m in P.prologue.meta]


def test_tiny_plans_with_freeu_hold_six_records_per_unet_forward(plan_dump, dump_dir, tmp_path, monkeypatch):
    log = _resnet_log(monkeypatch)
    B, h, w, T, n = 1, 8, 8, 7, 4
    fresh = _engine()                                                  # an engine whose FreeU API is never touched
    before = str(tmp_path / "before.bcplan")
    fresh.compile_plan(before, B, h, w, T, TINY["ctx"], n, blobnet_control_guidance_end=0.5)
    del log[:]
    eng = _engine()
    on, off = str(tmp_path / "on.bcplan"), str(tmp_path / "off.bcplan")
    seq = eng.compile_plan(on, B, h, w, T, TINY["ctx"], n, blobnet_control_guidance_end=0.5, freeu=FREEU)
    key_on = next(reversed(eng._plans))
    P = eng._plans[key_on]
    _check_sites(P, log)
    assert eng.compile_plan(off, B, h, w, T, TINY["ctx"], n, blobnet_control_guidance_end=0.5) == seq
    key_off = next(reversed(eng._plans))
    assert key_on == key_off + ("freeu",) and eng._plans[key_off].freeu is None
    # FreeU off: the file the untouched engine wrote, launch for launch and buffer for buffer
    assert _listing_hash(dump_dir, off) == _listing_hash(dump_dir, before) and _version(off) == _version(before) == 5
    assert _version(on) == 7                                           # BC_OP_FREEU is a version-7 op; the dump below is a reload
    bufs, segs = plan_dump(on)
    obufs, osegs = plan_dump(off)
    assert [op for op, _, _ in segs["prologue"]] == [op for op, _, _ in osegs["prologue"]]
    for name in ("step_active", "step_inactive"):
        ops, oops = [op for op, _, _ in segs[name]], [op for op, _, _ in osegs[name]]
        assert ops.count(OP_FREEU) == 6 and OP_FREEU not in oops
        # the FreeU-off listing plus the six records; the statistics passes of the twelve tensors bc_freeu replaced are gone (their
        # totals come out of the launch), and none is added
        rest, missing, it = [op for op in ops if op != OP_FREEU], [], iter(oops)
        for op in rest:
            for o in it:
                if o == op:
                    break
                missing.append(o)
            else:
                raise AssertionError(f"{name}: the FreeU listing is not the FreeU-off listing plus FreeU records")
        missing += list(it)
        assert set(missing) <= {OP_GN_STATS} and len(missing) <= 12, (name, missing)
        assert ops.count(OP_GN_STATS) == oops.count(OP_GN_STATS) - len(missing)
        # BlobNet's branch (stream 1) is what it was: the same launches with the same scalar arguments
        strip = lambda recs: [(op, [a for a in args if not a.startswith("p")]) for op, sid, args in recs if sid == 1]
        assert strip(segs[name]) == strip(osegs[name]) and (len(strip(segs[name])) > 100) == (name == "step_active")
        recs = [(sid, a) for op, sid, a in segs[name] if op == OP_FREEU]
        assert [a[7] for _, a in recs] == ["0", "0", "0", "1", "1", "1"] and all(sid == 0 for sid, _ in recs)
        for _, a in recs:
            assert _named(bufs, a[6]) == ("freeu", 0) and a[4] == str(2 * B)
            HW = int(a[5])
            assert HW in (2 * 1, 4 * 2) and bufs[int(a[8][1:].split("+")[0])][1] == HW * 8 * 4          # the basis table of the site's size
            assert len({a[0], a[2], a[9], a[10]}) == 4                                               # outputs are buffers of their own
    sizes = {n_: b_ for n_, b_ in bufs.values() if n_ != "-"}
    osizes = {n_: b_ for n_, b_ in obufs.values() if n_ != "-"}
    assert sizes.pop("freeu") == 16 and sizes == osizes
    assert np.frombuffer(_stored(on)["freeu"], np.float32).tolist() == [np.float32(v) for v in FREEU]
    # a reader that does not know the op refuses the file as an unknown op code: a version-6 header cannot carry it
    raw = bytearray(open(on, "rb").read())
    raw[4:8] = struct.pack("<I", 6)
    (tmp_path / "v6.bcplan").write_bytes(bytes(raw))
    with pytest.raises(AssertionError, match="unknown op"):
        plan_dump(str(tmp_path / "v6.bcplan"))


def test_freeu_composes_with_single_pass_and_a_scaled_table(tmp_path, monkeypatch):
    from blobctrl_amd.schedulers import EulerDiscreteScheduler
    log = _resnet_log(monkeypatch)
    eng = _engine()
    path = str(tmp_path / "x.bcplan")
    eng.compile_plan(path, 2, 8, 8, 7, TINY["ctx"], 4, guidance_scale=1.0, single_pass=True, freeu=FREEU)
    key = next(reversed(eng._plans))
    assert key[-2:] == ("single", "freeu") and eng._plans[key].single and eng._plans[key].freeu.shape == (4,)
    _check_sites(eng._plans[key], log)
    assert [m["shape"][1] for m in eng._plans[key].step_active.meta if m["kind"] == "freeu"] == [2] * 6       # the UNet at batch B
    del log[:]
    s = EulerDiscreteScheduler(**SD)
    eng.set_scheduler(s.kind, s.table_params())
    eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 4, freeu=FREEU)
    key = next(reversed(eng._plans))
    assert key[-2:] == ("scaled", "freeu") and eng._plans[key].scaled and _version(path) == 7
    _check_sites(eng._plans[key], log)
    del log[:]
    P = eng.plan_for(1, 8, 8, 7, TINY["ctx"], 4, stochastic=True, per_request=True, freeu=True)
    assert next(reversed(eng._plans))[-1] == "freeu" and P.stochastic
    _check_sites(P, log)


def test_split_cfg_runs_freeu_in_both_halves(monkeypatch):
    monkeypatch.setenv("BC_SPLIT_CFG", "1")
    log = _resnet_log(monkeypatch)
    eng = _engine()
    P = eng.plan_for(1, 8, 8, 7, TINY["ctx"], 4, freeu=True)
    assert P.split_cfg
    for seg in (P.step_active, P.step_inactive):
        fu = [m for m in seg.meta if m["kind"] == "freeu"]
        assert len(fu) == 12 and sorted({m["sid"] for m in fu}) == [0, 2] and all(m["shape"][1] == 1 for m in fu)


def test_the_truthiness_rule_runs_the_plain_plan(tmp_path):
    from blobctrl_amd.engine import freeu_enabled
    assert freeu_enabled(FREEU) and freeu_enabled([0.5, 0.5, 1, 1]) and not freeu_enabled(None)
    for bad in ((0.9, 0.0, 1.5, 1.6), (0.0, 0.2, 1.5, 1.6), (0.9, 0.2, 0, 1.6), (0.9, 0.2, 1.5, None), (None, None, None, None)):
        assert not freeu_enabled(bad), bad
    eng = _engine()
    path = str(tmp_path / "x.bcplan")
    eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 4, freeu=(0.9, 0.2, 1.5, 0.0))
    assert "freeu" not in next(reversed(eng._plans)) and _version(path) == 5 and len(eng._plans) == 1
    eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 4)
    assert len(eng._plans) == 1 and eng.cache_stats["plan_hits"] == 1


# ------------------------------------------------------------------------------------------------------------ SD-1.5 widths
@pytest.fixture(scope="module")
def full_engine():
    """A compile-only engine at full SD-1.5 widths.  The weights are zeros (a plan's launches do not depend on their values)."""
    from blobctrl_amd import synth
    from blobctrl_amd.engine import TrunkConfig
    from blobctrl_amd.pipeline import BlobCtrlEngine
    boc = (320, 640, 1280, 1280)
    us = synth.trunk_param_shapes(5, boc, 2, 768, 4, blobnet=False)
    bs = synth.trunk_param_shapes(1029, boc, 2, None, None, blobnet=True)
    zeros = lambda sh: {k: torch.zeros(1).expand(*v) if len(v) else torch.zeros(()) for k, v in sh.items()}
    return BlobCtrlEngine(zeros(us), zeros(bs), TrunkConfig(in_channels=5),
                          TrunkConfig(in_channels=1029, cross_attention_dim=None, out_channels=0, is_blobnet=True), device="cpu",
                          scheduler="ddim", compile_only=True, max_cached_plans=2)


@pytest.mark.parametrize("hw", [64, 96])
def test_full_width_plans_gain_exactly_the_six_launches(full_engine, hw, monkeypatch):
    """512^2 (64 x 128 canvas, FreeU at 8 x 16 and 16 x 32) and 768^2 (96 x 192 canvas, 12 x 24 and 24 x 48) at the SD-1.5 widths: every
    producer in front of a FreeU site emits its statistics itself there, so the recorder's listing with FreeU on IS the FreeU-off
    listing plus six launches per UNet forward - no statistics pass more or less.  (The recorder's own listing: a full-width plan
    file holds gigabytes of weights, so none is written here; the file format is covered on the tiny nets.)"""
    log = _resnet_log(monkeypatch)
    P0 = full_engine.plan_for(1, hw, hw, 77, 768, 2)
    del log[:]
    P1 = full_engine.plan_for(1, hw, hw, 77, 768, 2, freeu=True)
    _check_sites(P1, log)
    ident = lambda m: (m["kind"], m["variant"], m["shape"], m["sid"])
    for name in ("prologue", "step_active", "step_inactive"):
        a, b = [ident(m) for m in getattr(P0, name).meta], [ident(m) for m in getattr(P1, name).meta]
        assert [m for m in b if m[0] != "freeu"] == a, name
        fu = [m for m in b if m[0] == "freeu"]
        assert len(fu) == (0 if name == "prologue" else 6)
        if fu:
            s0, s1 = (hw // 8) * (hw // 4), (hw // 4) * (hw // 2)
            assert [m[2] for m in fu] == [("freeu", 2, s0, 1280, 1280, 0)] * 3 + [("freeu", 2, s1, 1280, 1280, 1), ("freeu", 2, s1, 1280, 1280, 1),
                                                                                ("freeu", 2, s1, 1280, 640, 1)]


# ------------------------------------------------------------------------------------------------------------ public surface
def test_unet_module_and_pipeline_surface():
    from blobctrl_amd.modules import UNet2DConditionModel
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from tests.gpu_common import tiny_trunk_configs
    unet = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0], device="cpu", lazy=True)
    assert unet.freeu is None
    unet.enable_freeu(*FREEU)
    assert unet.freeu == FREEU
    unet.enable_freeu(s1=0.6, s2=0.4, b1=1.2, b2=1.4)
    assert unet.freeu == (0.6, 0.4, 1.2, 1.4)
    unet.disable_freeu()
    assert unet.freeu is None
    # the module's own plans are keyed on it, the parameters in a plan buffer
    P0 = unet._plan(1, 8, 16, 7, TINY["ctx"], False)
    P1 = unet._plan(1, 8, 16, 7, TINY["ctx"], False, freeu=True)
    assert sorted(len(k) for k in unet._plans) == [6, 7] and ("freeu" in list(unet._plans)[1])
    assert P1.freeu.shape == (4,) and P1.freeu.dtype == torch.float32 and not hasattr(P0, "freeu")
    # (a GroupNorm pass is named after where its statistics come from: with FreeU they come out of bc_freeu, not out of a pass)
    kinds = lambda P: [m["kind"].replace("groupnorm_fused_stats", "groupnorm") for m in P.seg.meta]
    k0, k1 = kinds(P0), kinds(P1)
    assert k1.count("freeu") == 6 and "freeu" not in k0
    assert [k for k in k1 if k not in ("freeu", "gn_stats")] == [k for k in k0 if k != "gn_stats"] and k1.count("gn_stats") <= k0.count("gn_stats")
    # the pipeline forwards to the UNet, with the reference's signature and its error
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    pipe.unet = unet
    pipe.enable_freeu(0.9, 0.2, b1=1.5, b2=1.6)
    assert unet.freeu == FREEU
    pipe.disable_freeu()
    assert unet.freeu is None
    pipe.unet = None
    with pytest.raises(ValueError, match="The pipeline must have `unet` for using FreeU."):
        pipe.enable_freeu(*FREEU)


def test_freeu_op_has_a_fake_kernel_and_refuses_the_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from blobctrl_amd import _lib, ops  # noqa: F401
    assert str(torch.ops.blobctrl.freeu.default._schema) == "blobctrl::freeu(Tensor hidden, Tensor skip, Tensor params, SymInt stage) -> (Tensor, Tensor)"
    with FakeTensorMode():
        h = torch.empty(2, 3, 6, 64, dtype=torch.float16, device="cuda")
        s = torch.empty(2, 3, 6, 32, dtype=torch.float16, device="cuda")
        oh, os_ = torch.ops.blobctrl.freeu(h, s, torch.empty(4, device="cuda"), 1)
        assert (oh.shape, oh.dtype, oh.device) == (h.shape, torch.float16, h.device)
        assert (os_.shape, os_.dtype, os_.device) == (s.shape, torch.float16, s.device)
    with pytest.raises(_lib.BlobCtrlHipError, match="no CPU fallback"):
        torch.ops.blobctrl.freeu(torch.zeros(1, 2, 2, 8, dtype=torch.float16), torch.zeros(1, 2, 2, 8, dtype=torch.float16), torch.ones(4), 0)
    with pytest.raises(ValueError, match="share batch"):
        torch.ops.blobctrl.freeu(torch.zeros(1, 2, 2, 8, dtype=torch.float16), torch.zeros(1, 2, 3, 8, dtype=torch.float16), torch.ones(4), 0)
    # the schemas of the ops that were there before
    assert "timestep_cond=None) -> Tensor" in str(torch.ops.blobctrl.unet_forward.default._schema)
    assert "variance_noise=None) -> Tensor" in str(torch.ops.blobctrl.denoise.default._schema)


OLD_OPS = {"bc_gemm": 0, "bc_gn_stats": 1, "bc_gn_finalize": 2, "bc_gn_apply_fused": 3, "bc_gn_apply": 4, "bc_layernorm": 5, "bc_attention": 6,
           "bc_attention_causal": 7, "bc_assemble_input": 8, "bc_timestep_embedding": 9, "bc_timestep_embedding_table": 10,
           "bc_cfg_scheduler_step": 11, "bc_embed_tokens": 12, "bc_softmax_rows": 13, "bc_patchify": 14, "bc_add_cls_pos": 15, "bc_silu": 16,
           "bc_nchw_to_nhwc_f16": 17, "bc_nhwc_to_nchw": 18, "bc_gaussian_sample": 19, "bc_rowchain": 22, "bc_assemble_input_im2col": 23,
           "bc_memset_zero": 24, "bc_rowchain_midx": 25, "bc_rowchain_pack_kv": 26, "bc_rowchain_sum": 27, "bc_ctx_fold": 28,
           "bc_dup_halves": 29, "bc_cfg_scheduler_step_noise": 30, "bc_cfg_scheduler_step3": 31, "bc_assemble_input_scaled": 32,
           "bc_assemble_input_im2col_scaled": 33, "bc_scheduler_step_single": 34, "bc_timestep_embedding_table_cond": 35,
           "bc_timestep_embedding_cond": 36}


def test_bc_freeu_is_exported_beside_every_symbol_that_was_there():
    from blobctrl_amd import _lib
    lib = _lib.load()                                                  # (raises when a declared symbol does not resolve)
    assert "bc_freeu" in _lib.EXPORTED_SYMBOLS and lib.bc_freeu is not None and len(_lib.EXPORTED_SYMBOLS) == 92
    assert _lib.OPS == dict(OLD_OPS, bc_freeu=OP_FREEU) and set(OLD_OPS) < set(_lib.EXPORTED_SYMBOLS)
    assert _lib.op_signature("bc_freeu") == "pipiiipippppp"
    for name in ("bc_plan_save", "bc_plan_load", "bc_plan_capture_loop", "bc_splat_scores", "bc_conv_wreg_pack", "bc_graph_launch"):
        assert name in _lib.EXPORTED_SYMBOLS
    # argument checks of the host wrapper: refused before anything is launched (no GPU is touched)
    assert lib.bc_freeu(None, 64, None, 64, 1, 8, None, 0, None, None, None, None, None, None) == 1
    assert b"null pointer" in lib.bc_last_error()
    p = 4096                                                           # (any non-null, aligned address: the checks below fail first)
    for kw, word in ((dict(C_h=60), b"widths"), (dict(stage=2), b"stage"), (dict(B=0), b"bad shape"), (dict(hidden_out=p), b"buffers of their own"),
                     (dict(basis=p + 4), b"alignment")):
        a = dict(hidden=p, C_h=64, skip=2 * p, C_s=64, B=1, HW=8, params=3 * p, stage=0, basis=4 * p, hidden_out=5 * p, skip_out=6 * p,
                 tot_h=7 * p, tot_s=8 * p)
        a.update(kw)
        assert lib.bc_freeu(*a.values(), None) == 1 and word in lib.bc_last_error(), kw
