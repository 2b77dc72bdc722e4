"""Every row-chain launch (csrc/rowchain.hip, csrc/rowchain_midx.hip) on its own against the plain float64 reference of its operation, in
NaN-fenced buffers (tests/rowchain_stages_common.py; what that harness sees is shown on the CPU in tests/test_rowchain_stages_cpu.py).
The launches go through Recorder.rowchain / rowchain_midx / rowchain_sum / rowchain_kv_stream with the streams of weights.pack_rowchain
from a PackedTrunk - the calls engine.transformer_rowchain makes, one launch per segment - so h0, q | k, V^T, h1, the cross-attention
output and the zero-conv residual are each inspected where they are written, not behind two softmaxes.  Bars: tests.common.close's default
(2e-3 |ref| + 2e-3 max(1, scale)) for every row output, attention_common's for the MIDX attention output.  Every case prints a MARGIN line
(profiles/rowchain_stage_margins.txt is a copy of one run)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib  # noqa: E402
from tests import rowchain_stages_common as rc  # noqa: E402

DEV = torch.device("cuda:0")
CHANNELS = (320, 640)


@pytest.fixture
def rec():
    from blobctrl_amd.launch import Recorder
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    r = Recorder(DEV)
    yield r
    r.close()


@pytest.fixture(scope="module")
def trunks():
    """(C, cross, zero) -> (float64 reference of the block, its PackedTrunk): one of each per module."""
    from blobctrl_amd.weights import PackedTrunk
    cache = {}

    def get(C, cross, zero=False):
        if (C, cross, zero) not in cache:
            sd = rc.block_sd(C, cross, zero)
            full = {"blk." + k: v for k, v in sd.items()}
            full["conv_in.weight"] = torch.zeros(8, 4, 3, 3)                      # (PackedTrunk expects a trunk: unused stand-ins)
            full["none.time_emb_proj.weight"], full["none.time_emb_proj.bias"] = torch.zeros(8, 1280), torch.zeros(8)
            cache[(C, cross, zero)] = (rc.BlockRef(sd), PackedTrunk(full, DEV, (320, 640, 1280, 1280)))
        return cache[(C, cross, zero)]
    return get


@pytest.fixture(scope="module")
def end_refs():
    """The float64 block end of a case, computed once and shared by its launch forms."""
    cache = {}

    def get(ref, key, **kw):
        if key not in cache:
            cache[key] = rc.end_reference(ref, **kw)
        return cache[key]
    return get


def packed(pw, prob, kind, zname=None, nsplit=1):
    """(weight stream, vec) of weights.pack_rowchain; vec as a view inside an fp32-NaN parent of the problem (a lane read behind the last
    bias reaches the output)."""
    from blobctrl_amd.weights import pack_rowchain
    cache = pw.__dict__.setdefault("_rowchain", {})
    key = ("blk.", kind, zname, nsplit)
    if key not in cache:
        cache[key] = pack_rowchain(pw, "blk.", kind, zname, nsplit)
    w, vec = cache[key]
    prob.views[f"vec{kind}"] = rc.fenced_vec(vec, DEV)
    return w, prob.views[f"vec{kind}"].t


def run(rec, prob, record):
    prob.assert_inside()
    seg = rec.begin("stage")
    record()
    seg.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return seg


def margin(prob, worst, checked):
    each = ", ".join(f"{label} {e:.3f}" for label, e in prob.errs.items())
    print(f"MARGIN {prob.name}: max err/bar {worst:.3f} ({each}) | {checked} sentinel elements checked")


# ---------------------------------------------------------------------------------------------------- IN
@pytest.mark.parametrize("form", rc.IN_FORMS)
@pytest.mark.parametrize("B,HW", [(3, 64), (2, 192)])              # every workgroup another image | three row blocks per image
@pytest.mark.parametrize("C", CHANNELS)
def test_in_launch(rec, trunks, C, B, HW, form):
    ref, pw = trunks(C, True)
    prob = rc.in_problem(ref, DEV, B, HW, form)
    v, a = prob.views, prob.args

    def record():
        w, vec = packed(pw, prob, _lib.CHAIN_IN)
        kw = {}
        if form == "totals":
            kw["gn_in"] = (v["gn_tot"].t, pw.f["blk.norm.weight"], pw.f["blk.norm.bias"], rc.GROUPS, rc.GN_EPS)
        elif form == "affine":
            kw["affine"] = v["affine"].t
        rec.rowchain(_lib.CHAIN_IN, C, a["M"], HW, v["x"].t, w, vec, prob.out("h0").t, out1=prob.out("q|k").t, out2=prob.out("V^T").t,
                     ldvt=a["ldvt"], ln_eps=a["ln_eps"], **kw)
    run(rec, prob, record)
    worst, checked = prob.verify()
    # (V^T: the 8 padding columns of every channel row are part of the sentinels Out.check found untouched)
    assert checked >= B * C * rc.VT_PAD + 2 * rc.GUARD * (3 * C + a["ldvt"])
    margin(prob, worst, checked)


# ---------------------------------------------------------------------------------------------------- MID
@pytest.mark.parametrize("B,HW,ln_eps", [(2, 64, rc.LN_EPS), (1, 192, rc.LN_EPS), (2, 64, 1e-3)])
@pytest.mark.parametrize("C", CHANNELS)
def test_mid_launch(rec, trunks, C, B, HW, ln_eps):
    ref, pw = trunks(C, True)
    prob = rc.mid_problem(ref, DEV, B, HW, ln_eps)
    v, a = prob.views, prob.args

    def record():
        w, vec = packed(pw, prob, _lib.CHAIN_MID)
        rec.rowchain(_lib.CHAIN_MID, C, a["M"], HW, v["x"].t, w, vec, prob.out("h1").t, out1=prob.out("q").t, res=v["res"].t, ln_eps=ln_eps)
    run(rec, prob, record)
    margin(prob, *prob.verify())


# ---------------------------------------------------------------------------------------------------- MIDX
@pytest.mark.parametrize("T", [1, 17, 48, 77, 80])
@pytest.mark.parametrize("C", CHANNELS)
def test_midx_launch(rec, trunks, C, T):
    B, HW = 3, 64
    ref, pw = trunks(C, True)
    prob = rc.midx_problem(ref, DEV, B, HW, T)
    v, a = prob.views, prob.args

    def record():
        w, vec = packed(pw, prob, _lib.CHAIN_MID)
        kvs = rec.rowchain_kv_stream(v["k"].t, v["vt"].t, B, T, C, a["ldvt_ctx"])
        rec.rowchain_midx(C, a["M"], HW, v["x"].t, w, vec, kvs, T, rc.HEADS, (C // rc.HEADS) ** -0.5, prob.out("h1").t, prob.out("attn").t,
                          res=v["res"].t, ln_eps=a["ln_eps"])
    run(rec, prob, record)
    margin(prob, *prob.verify())


# ---------------------------------------------------------------------------------------------------- the block end
def record_end(rec, pw, prob):
    """OUT | OUT_FF + OUT_TAIL | OUT_FFP + bc_rowchain_sum, as engine.transformer_rowchain records them.  Returns the statistics table."""
    v, a = prob.views, prob.args
    C, M, HW, B, nsplit, ln_eps = a["C"], a["M"], a["HW"], a["B"], a["nsplit"], a["ln_eps"]
    x, res, res2, out = v["x"].t, v["res"].t, v["res2"].t, prob.out("out").t
    tot = rec.new_tot(B, C)
    kw, zname, zout = {}, None, None
    if "r2" in v:
        kw.update(r2=v["r2"].t, r2_xmin=a["r2_xmin"], r2_bmod=a["r2_bmod"], out_w=a["out_w"])
    if a["zero"] is not None:
        alpha, idx, bstride = a["zero"]
        zname, zout = "blk.zero", prob.out("zero").t
        kw.update(out1=zout, alpha=alpha, alpha_dev=v["alpha_dev"].t if "alpha_dev" in v else None,
                  alpha_idx=None if idx is None else torch.tensor([idx], dtype=torch.int32, device=DEV), alpha_bstride=bstride)
    if a["form"] == "out":
        w, vec = packed(pw, prob, _lib.CHAIN_OUT, zname)
        rec.rowchain(_lib.CHAIN_OUT, C, M, HW, x, w, vec, out, res=res, res2=res2, gn_tot=tot, ln_eps=ln_eps, **kw)
    elif a["form"] == "ff_tail":
        ffp = prob.out("part fp32").t
        w, vec = packed(pw, prob, _lib.CHAIN_OUT_FF, zname, nsplit)
        rec.rowchain(_lib.CHAIN_OUT_FF, C, M, HW, x, w, vec, None, res=res, part=ffp, nsplit=nsplit, ln_eps=ln_eps)
        w, vec = packed(pw, prob, _lib.CHAIN_OUT_TAIL, zname)
        rec.rowchain(_lib.CHAIN_OUT_TAIL, C, M, HW, None, w, vec, out, res2=res2, gn_tot=tot, part=ffp, nsplit=nsplit, ln_eps=ln_eps, **kw)
    else:
        pp = prob.out("part fp16").t
        w, vec = packed(pw, prob, _lib.CHAIN_OUT_FFP, zname, nsplit)
        kw2 = {k: v_ for k, v_ in kw.items() if k != "out1"}
        rec.rowchain(_lib.CHAIN_OUT_FFP, C, M, HW, x, w, vec, None, out1=zout, res=res, res2=res2, part=pp, nsplit=nsplit, ln_eps=ln_eps, **kw2)
        rec.rowchain_sum(C, M, HW, pp, nsplit, out, gn_tot=tot, out1=zout)
    return tot


def check_end(rec, pw, prob):
    from blobctrl_amd.launch import decode_gn_tot, gn_tot_slots
    hold = {}
    seg = run(rec, prob, lambda: hold.update(tot=record_end(rec, pw, prob)))
    a = prob.args
    # (the split forms launch nsplit * M / 64 workgroups: the partial-sum buffer between the two launches is an output like any other -
    #  every row block of every slice written, nothing around it)
    worst, checked = prob.verify()
    # statistics totals of `out`: the per-image sums of the fp16 output (tests/test_rowchain_gpu.py's tolerance); nothing else in the chunk
    # the table was carved from has been added to
    tot = hold["tot"]
    have = gn_tot_slots(decode_gn_tot(tot).float())
    o = prob.vals["out"].float().view(a["B"], a["HW"], a["C"])
    want = gn_tot_slots(torch.stack([o.sum(1), (o * o).sum(1)], -1))
    assert bool(torch.isfinite(have).all()), f"{prob.name}: non-finite statistics totals"
    for i, what in enumerate(("sums", "sums of squares")):
        assert torch.allclose(have[..., i], want[..., i], rtol=1e-3, atol=1e-2 * a["HW"] ** 0.5), f"{prob.name}: {what} of the output, per image"
    chunk = rec._tot_chunk[(seg.id, 0)][0]
    assert int((chunk != 0).sum()) == int((tot != 0).sum()), f"{prob.name}: statistics were added outside the table"
    margin(prob, worst, checked)


def _forms(C):
    return rc.END_FORMS + (rc.END_FORMS_640 if C == 640 else ())


UNET_END = [(C, form, ns, case) for C in CHANNELS for form, ns in _forms(C) for case in list(rc.R2_CASES) + [None]]


@pytest.mark.parametrize("C,form,nsplit,case", UNET_END, ids=[f"{C}-{f}{n}-{c or 'no_r2'}" for C, f, n, c in UNET_END])
def test_unet_block_end(rec, trunks, end_refs, C, form, nsplit, case):
    """r2 cases (out_w, r2_xmin, rows per image, B, bmod): rowchain_stages_common.R2_CASES; without r2: (B=2, HW=128)."""
    ref, pw = trunks(C, True)
    _, _, HW, B, _ = rc.R2_CASES[case] if case else (0, 0, 128, 2, 0)
    pre = end_refs(ref, (C, "unet", case), B=B, HW=HW, r2case=case)
    check_end(rec, pw, rc.end_problem(ref, DEV, B, HW, form, nsplit, pre, r2case=case))


BLOB_END = [(C, form, ns, B, HW, z) for C in CHANNELS for form, ns in _forms(C) for B, HW in ((4, 64), (1, 192)) for z in rc.ALPHA_FORMS]


@pytest.mark.parametrize("C,form,nsplit,B,HW,zero_form", BLOB_END, ids=[f"{C}-{f}{n}-B{B}xHW{HW}-{z}" for C, f, n, B, HW, z in BLOB_END])
def test_blobnet_block_end(rec, trunks, end_refs, C, form, nsplit, B, HW, zero_form):
    """alpha alone | alpha_dev[3] with alpha_idx = 2, bstride 0 | alpha_dev[3][B] with alpha_idx = 1, bstride B (the last B entries of
    rowchain_stages_common.ALPHA_ROW); every other entry of alpha_dev is NaN."""
    ref, pw = trunks(C, False, True)
    pre = end_refs(ref, (C, "blobnet", B, HW, zero_form), B=B, HW=HW, zero_form=zero_form)
    check_end(rec, pw, rc.end_problem(ref, DEV, B, HW, form, nsplit, pre, zero_form=zero_form))


@pytest.mark.parametrize("form,nsplit", [("ff_tail", 2), ("ffp_sum", 5)])
@pytest.mark.parametrize("C", CHANNELS)
def test_twelve_row_blocks_in_the_split_forms(rec, trunks, end_refs, C, form, nsplit):
    """Row-block counts: 2, 3, 4, 6 and 24 run above; here 12 - above 8 and no multiple of 8, 24 / 60 workgroups through the remap."""
    ref, pw = trunks(C, True)
    pre = end_refs(ref, (C, "unet", "12 blocks"), B=4, HW=192)
    check_end(rec, pw, rc.end_problem(ref, DEV, 4, 192, form, nsplit, pre))
