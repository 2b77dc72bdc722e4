"""Every switch of the denoise planner, taken both ways at the widths SD-1.5 and BlobNet really have (tests/planner_cases.py): ONE block
per case, recorded through the engine's own block methods (TrunkPlan.resnet / .transformer / .conv3x3 / .dense), replayed through the C ABI
and compared with the float64 CPU restatement of the same block (oracle/nets.py) on the same fp16-rounded input and fp16-rounded matrices.

Before a case is replayed, the recorded plan must show the kernel family the case was chosen for (`fam` / `nofam` of the table): a planner
change that reroutes a shape breaks the case loudly instead of silently moving its coverage.  `test_table_crosses_every_switch` records the
whole table and compares the (switch, side) pairs it shows with the list written out below.

Bar: BASELINE.json's - max-abs <= 1e-2 of the reference's max-abs and PSNR >= 40 dB (peak = the reference's max-abs) - over the whole output
and, separately, over the last tile row and the last tile column of the map (8 x 16 pixel tiles: where a wrong border tile would sit).
Measured values are printed per case (profiles/planner_sweep_margins.txt is a copy of one run).

Host time: the float64 references take 0.1 - 4 s each on 16 threads, 42 s in all (the 1280-channel upsamplers and transformer blocks the longest); cases that
differ only in planner options share one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import planner_cases as pc  # noqa: E402
from tests.common import set_plan  # noqa: E402

# Both sides of every planner switch (ISSUE: block sweep).  switch -> the sides the table must show; "N:" prefixes are the deciding count
# (requests, M, row blocks, tiles) of the case that shows the side.
REQUIRED = {
    # bc_conv_halo_eligible (W % 16, H % 8, Cin % 64, N % 160): conv_wreg / conv_halo against the implicit-GEMM tiles
    "conv_eligible": {"aligned:conv_wreg", "aligned:conv_halo", "ragged:implicit_gemm"},
    # gn_pass_min_requests (4): UNet B = 6 (3 requests) against B = 8, BlobNet B = 3 against B = 4
    "gn_pass_min_requests/unet": {"<3:fused_conv_wreg<2>", "3:fused_conv_wreg<2>", "4:pass+conv_wreg<0>"},
    "gn_pass_min_requests/blob": {"3:fused_conv_wreg<2>", "4:pass+conv_wreg<0>"},
    # bc_conv_wreg_sc_eligible; with sc_fold=0 the gw 1x1 shortcut at Cout = 1280: M = 1024 against 1280, and M % 64 != 0
    "sc_fold_eligible": {"folded", "launch"},
    "shortcut_gw": {"gw", "over_gw_maxm", "rejected_by_gemm_wreg"},
    # launch.py halo_ctas / halo_min_cps / halo_full: a convolution pass that runs unsplit against a split one
    "conv_splitk": {"split", "unsplit"},
    # bc_rowchain_supported (HW % 64) at 320 and 640 channels
    "rowchain_hw64/320": {"hw%64==0:rowchain", "hw%64!=0:launch_list"},
    "rowchain_hw64/640": {"hw%64==0:rowchain", "hw%64==0:launch_list", "hw%64!=0:launch_list"},
    # rowchain_min_blocks_640 (64) and rowchain_min_blocks_640_blob_up (32); below them gemm_wreg (M <= gw_maxm) or the launch list
    "rowchain_min_blocks_640/unet": {"16:gw", "32:launch_list", "64:rowchain", "80:rowchain"},
    "rowchain_min_blocks_640/blob_down": {"32:launch_list", "64:rowchain"},
    "rowchain_min_blocks_640/blob_up": {"16:gw", "32:rowchain", "64:rowchain"},
    # rowchain_ff_split: up to 64 row blocks at 640 channels, up to 128 at 320 (ff_split_320=2: its default 1 is the one-launch form)
    "block_end_split/640": {"<=:split", ">:one_launch"},
    "block_end_split/320": {"<=:split", ">:one_launch"},
    "block_end_form": {"out_ffp+sum", "out_ff+out_tail"},
    # gw_maxm (1024): 16 x 32 at B = 2 against 3, 8 x 16 at B = 8 against 10, and a map bc_gemm_wreg_eligible rejects (HW % 64)
    "gw_maxm": {"<1024:gw", "1024:gw", "1280:launch_list", "1536:launch_list", "rejected_by_gemm_wreg"},
    # ctx_fold_maxb (2)
    "ctx_fold_maxb": {"2:folded", "4:attention", "8:attention"},
    # g256_min_tiles (64) and bc_gemm256_eligible (M % 256): a 1280 x 1280 projection, and ff.net.0 of the gemm_wreg blocks
    "g256_min_tiles": {"60:gemm_fast", "65:gemm256", "m%256!=0:gemm_fast"},
    "g256_min_tiles/ff1": {"m%256!=0:gemm_wreg", "40:gemm_wreg", "80:gemm256", "160:gemm256"},
    # the ups_wreg test of TrunkPlan.conv3x3
    "ups_wreg": {"x2_aligned:conv_wreg", "x2_ragged:implicit_gemm", "explicit_size:generic_gemm"},
    "downsample": {"aligned", "ragged"},
    # the BlobNet residual on a non-square map (r2_xmin = W - H) per block kind, width and the family that adds it
    "r2_xmin": {"resnet320", "resnet640", "resnet1280", "transformer320:rowchain", "transformer320:launch_list", "transformer640:rowchain",
                "transformer640:launch_list", "transformer1280:gw", "transformer1280:launch_list"},
    # BlobNet's zero-conv inside the row-chain's last launch against a launch of its own
    "zero_conv": {"in_rowchain", "launch"},
    "is_blobnet": {"unet", "blob"},
}


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))


def _plan_opts(monkeypatch, case):
    monkeypatch.delenv("BC_PLAN", raising=False)
    if case.opts:
        set_plan(monkeypatch, **case.opts)


def _run(seg):
    seg.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _measure(got, ref, tile_rows, tile_cols):
    """[(region, max-abs / scale, PSNR)] over the whole output, its last tile row and its last tile column (scale = peak = the reference's
    max-abs over the whole output)."""
    scale = float(np.abs(ref).max())
    d = got.astype(np.float64) - ref
    rows, cols = d.shape[-2], d.shape[-1]
    r0, c0 = rows - ((rows - 1) % tile_rows + 1), cols - ((cols - 1) % tile_cols + 1)
    out = []
    for name, part in (("whole", d), ("last tile row", d[..., r0:, :]), ("last tile column", d[..., c0:])):
        out.append((name, float(np.abs(part).max()) / scale, float(10 * np.log10(scale * scale / max(np.mean(part ** 2), 1e-30)))))
    return out


@pytest.mark.parametrize("cid", [c.id for c in pc.CASES])
def test_block_on_its_planner_path(cid, monkeypatch):
    case = pc.BY_ID[cid]
    _plan_opts(monkeypatch, case)
    rec, seg, outs = pc.record(case, "cuda:0")
    try:
        pc.check_family(case, rec)
        pc.sides(case, rec)                              # (asserts that the family agrees with the case's geometry)
        fam = pc.family(rec)
        _run(seg)
        ref = pc.reference(case)
        B, H, W = case.B, case.H, case.W
        failed = []
        for key in sorted(outs):
            if case.kind == "dense":
                got, tiles = outs[key].float().cpu().numpy(), (256, 256)
            else:
                o = outs[key]
                Ho, Wo = ref[key].shape[-2:]
                got, tiles = pc.nchw(o, B, Ho, Wo), (8, 16)
            assert got.shape == ref[key].shape, (got.shape, ref[key].shape)
            assert np.isfinite(got).all(), f"{cid} {key}: non-finite output"
            ms = _measure(got, ref[key], *tiles)
            print(f"planner case {cid} [{key}]: " + "; ".join(f"{n} max-abs/scale {e:.3e} PSNR {p:.1f} dB" for n, e, p in ms) + f" | {fam}")
            failed += [f"{key} {n}: {e:.3e} / {p:.1f} dB" for n, e, p in ms if not (e <= 1e-2 and p >= 40.0)]
        assert not failed, f"{cid} ({fam}): " + ", ".join(failed)
    finally:
        rec.close()


def test_table_crosses_every_switch(monkeypatch):
    """Record (no replay) every case and collect which side of which switch it shows: exactly the list above."""
    seen = {}
    for case in pc.CASES:
        _plan_opts(monkeypatch, case)
        rec, _, _ = pc.record(case, "cuda:0")
        try:
            pc.check_family(case, rec)
            for switch, side in pc.sides(case, rec):
                seen.setdefault(switch, set()).add(side)
        finally:
            rec.close()
    assert seen == REQUIRED, {k: (sorted(seen.get(k, ())), sorted(REQUIRED.get(k, ()))) for k in set(seen) | set(REQUIRED) if seen.get(k) != REQUIRED.get(k)}


def _gemm_refs(rec):
    """(out, R) of every recorded bc_gemm, in order (Recorder.gemm keeps its operands alive as one tuple per launch)."""
    return [(k[3], k[5]) for k in rec.keep if isinstance(k, tuple) and len(k) == 18]


def test_shortcut_buffer_does_not_alias_conv2_output(monkeypatch):
    """A 2560 -> 1280 block at 8 x 16 with sc_fold=0 takes the gemm_wreg 1x1 shortcut (M = 256 <= gw_maxm).  Its buffer once shadowed the
    caller's `out=`, so conv2 wrote over the residual it was reading: conv2's output is the caller's buffer and is not its residual."""
    case = pc.BY_ID["res2560-1280-8x16-nofold"]
    _plan_opts(monkeypatch, case)
    rec, _, outs = pc.record(case, "cuda:0")
    try:
        pc.check_family(case, rec)
        refs = _gemm_refs(rec)                            # ... conv1, the 1x1 shortcut, conv2
        (sc_out, _), (out, R) = refs[-2], refs[-1]
        assert R is not None and R.data_ptr() == sc_out.data_ptr()
        assert out.data_ptr() == outs["out"].t.data_ptr() and out.data_ptr() != R.data_ptr()
    finally:
        rec.close()


@pytest.mark.parametrize("operand", ["R", "R2", "S"])
def test_gemm_rejects_an_output_over_its_residual(operand):
    from blobctrl_amd import _lib
    from blobctrl_amd.launch import Recorder
    rec = Recorder(torch.device("cuda:0"))
    try:
        rec.begin("overlap")
        M, N, K = 128, 160, 64
        a, w, x = rec.empty(M, K), rec.empty(N, 9 * K), rec.empty(M + 8, N)
        other = rec.empty(M, N)
        n0 = len(rec.seg)
        if operand == "R":
            bad = dict(A=a, W=w[:, :K].contiguous(), M=M, N=N, K=K, out=x, R=x, ldr=N)
        elif operand == "R2":                             # (overlapping, not identical: the residual starts a few rows into the output)
            bad = dict(A=a, W=w[:, :K].contiguous(), M=M, N=N, K=K, out=x, R=other, ldr=N, R2=x[8:], ldr2=N, r2_bmod=1, out_w=16, rows_per_batch=M)
        else:
            conv = dict(Cin=K, Hin=8, Win=16, Hv=8, Wv=16, Hout=8, Wout=16, stride=1)
            bad = dict(A=a, W=w, M=M, N=N, K=9 * K, out=x, conv=conv, tile_cfg=_lib.TILE_WREG, lda=K, S=x, lds=N, Cs=64)
        with pytest.raises(_lib.BlobCtrlHipError, match="overlaps " + operand):
            rec.gemm(**bad)
        assert len(rec.seg) == n0                         # nothing was recorded
        rec.gemm(A=a, W=w[:, :K].contiguous(), M=M, N=N, K=K, out=x, R=other, ldr=N)      # disjoint buffers record as before
        assert len(rec.seg) == n0 + 1
    finally:
        rec.close()
