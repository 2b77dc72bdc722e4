"""The GEMM family (csrc/gemm.hip, gemm_fast.hip, gemm_wreg.hip, gemm256.hip, conv_halo.hip, conv_wreg.hip and the split-K reducers) on
operands that are views inside hostile parents (tests/gemm_views_common.py): NaN around every input, a NaN sentinel around every output.  A
read outside a view shows as a non-finite output, a store outside one as a changed sentinel; inside, the float64 reference holds at the
project's bars.  Every case runs in a 16-byte aligned flavour (the vector epilogues) and in one that forces the scalar epilogue - or asserts
that bc_gemm refuses that (family, flavour) pair -, asserts the kernel family the recorder names for it, and prints its margin
(profiles/gemm_views_margins.txt is a copy of one run).  The VAE mid-block attention runs through the model's own recording, launch by
launch, on the same kind of buffers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib  # noqa: E402
from tests import gemm_views_common as gv  # noqa: E402

DEV = torch.device("cuda:0")


@pytest.fixture
def rec():
    from blobctrl_amd.launch import Recorder
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    r = Recorder(DEV)
    yield r
    r.close()


def launch(rec, prob):
    """Record the problem's one bc_gemm and run it; the extents the kernel may address are checked against the parents' storage first."""
    from blobctrl_amd.launch import encode_gn_tot
    prob.assert_inside()
    prob.reset()
    kw = dict(prob.kw)
    seg = rec.begin("views")
    if prob.gn_in:                        # the statistics totals of the VALID channels of each source, as a producer would have left them
        gi, srcs = prob.gn_in, []
        for name, C, sums in prob.gn_in["srcs"]:
            x, tot = prob.views[name].t, encode_gn_tot(sums).to(DEV)
            rec.tots[x.data_ptr()] = tot
            rec.tots_per_channel.add(id(tot))
            rec.keep.append(tot)
            srcs.append((x, C))
        x2, C2 = srcs[1] if len(srcs) > 1 else (None, 0)
        kw["a_gn"] = dict(x1=srcs[0][0], C1=srcs[0][1], x2=x2, C2=C2, B=gi["B"], HW=gi["HW"], G=gi["G"], eps=gi["eps"],
                          gamma=gi["gamma"].to(DEV), beta=gi["beta"].to(DEV))
    rec.gemm(**kw)
    meta = rec.seg.meta[-1]
    seg.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return meta


def check_output_statistics(rec, prob, vals):
    """want_gn: the totals the launch added to (a table carved from a zeroed chunk) against the sums of the fp16 output it stored - a NaN pad
    channel or guard row that reached the statistics shows here."""
    from blobctrl_amd.launch import decode_gn_tot, gn_tot_slots
    from tests.common import close
    B, rpb, family = prob.gn_out
    o = prob.outs[0][1]
    tot = rec.tots[o.parent.data_ptr() + o.offset * 2]
    ov = vals.view(B, rpb, -1)
    want = gn_tot_slots(torch.stack([ov.sum(1), (ov * ov).sum(1)], -1))
    have = gn_tot_slots(decode_gn_tot(tot))
    assert bool(torch.isfinite(have).all()), f"{prob.name}: non-finite GroupNorm totals"
    if family in ("halo", "wreg"):                          # (tests/test_conv_halo_gpu.py)
        assert torch.allclose(have[..., 0], want[..., 0], rtol=1e-3, atol=1e-2 * rpb ** 0.5), f"{prob.name}: sums"
        assert torch.allclose(have[..., 1], want[..., 1], rtol=1e-3, atol=1e-2 * rpb ** 0.5), f"{prob.name}: sums of squares"
    else:                                                   # (tests/test_kernels_gpu.py::test_gemm256_modes)
        close(have, want, rtol=1e-4, atol=1e-2 * max(1.0, rpb / 256), what=f"{prob.name}: GroupNorm statistics")


def run_case(rec, case):
    for flavour in gv.FLAVOURS:
        prob = gv.build(case, flavour, DEV)
        if prob.refused:
            with pytest.raises(_lib.BlobCtrlHipError):
                launch(rec, prob)
            torch.cuda.synchronize()
            assert prob.untouched(), f"{prob.name}: a refused launch wrote"
            print(f"MARGIN {prob.name}: refused by bc_gemm")
            continue
        meta = launch(rec, prob)
        sk = meta["shape"][-1]
        assert meta["kind"] == "gemm" and meta["variant"].startswith(prob.variant), (prob.name, meta["variant"], prob.variant)
        assert ("+splitk_reduce" in meta["variant"]) == (sk > 1) and (prob.sk is None or sk == prob.sk), (prob.name, meta["variant"], sk)
        worst, checked = prob.verify()
        if prob.gn_out:
            assert prob.kw["out"].data_ptr() + prob.outs[0][1].offset * 2 in rec.tots, f"{prob.name}: no fused statistics"
            check_output_statistics(rec, prob, prob.vals)
        print(f"MARGIN {prob.name}: {meta['variant']} | max err/bar {worst:.3f} | {checked} sentinel elements checked")


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", gv.generic_cases(), ids=_ids(gv.generic_cases()))
def test_generic_kernel_views(rec, case):
    run_case(rec, case)


@pytest.mark.parametrize("mode", gv.FAST_MODES)
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5, 6, 7])
def test_gemm_fast_views(rec, cfg, mode):
    run_case(rec, gv.fast_case(cfg, mode))


@pytest.mark.parametrize("case", gv.gw_cases(), ids=_ids(gv.gw_cases()))
def test_gemm_wreg_views(rec, case):
    run_case(rec, case)


@pytest.mark.parametrize("case", gv.g256_cases(), ids=_ids(gv.g256_cases()))
def test_gemm256_views(rec, case):
    run_case(rec, case)


@pytest.mark.parametrize("case", gv.halo_cases("halo") + gv.halo_cases("wreg"), ids=_ids(gv.halo_cases("halo") + gv.halo_cases("wreg")))
def test_halo_and_wreg_convolution_views(rec, case):
    run_case(rec, case)


@pytest.mark.parametrize("B,N,C", gv.ATTN_SHAPES)
def test_vae_attention_launches_in_fenced_buffers(rec, B, N, C):
    """The VAE mid-block attention through the model's own recording (AutoencoderKL._attend), one launch at a time: per image Q K^T whose
    weight operand is columns C .. 2 C of the rows that hold A (image b at a per-image offset, the scale as alpha), bc_softmax_rows in place,
    P V at K = pad8(N) against V^T.  After each launch the buffer it wrote is written, finite and inside its bar (scores: the dense bar;
    probabilities and product: the attention bar) with every sentinel around it unchanged; at the end every NaN guard of qk and vt is intact."""
    from blobctrl_amd.vae import AutoencoderKL
    prob = gv.vae_attention_problem(DEV, B, N, C)
    prob.assert_inside()
    prob.reset()
    seg = rec.begin("vae_attention")
    AutoencoderKL._attend(rec, prob.views["qk"].t, prob.views["vt"].t, prob.s.t, prob.o.t, B, N, C)
    assert len(seg.meta) == 3 * B
    for i in range(len(seg.meta)):
        seg.enable(i, False)
    stream = torch.cuda.current_stream().cuda_stream
    for i, m in enumerate(seg.meta):
        b, st = divmod(i, 3)
        kind, variant = prob.launches[st]
        assert m["kind"] == kind and m["variant"].startswith(variant), (prob.name, i, m["kind"], m["variant"])
        if st == 0:
            prob.s.reset()                                      # (the score buffer holds one image: what is checked is what this image wrote)
        seg.enable(i, True)
        seg.run(stream)
        torch.cuda.synchronize()
        seg.enable(i, False)
        prob.check(b, gv.ATTN_STAGES[st])
    worst, checked = prob.verify()
    names = " / ".join(seg.meta[i]["variant"] or seg.meta[i]["kind"] for i in range(3))
    print(f"MARGIN {prob.name}: {names} | max err/bar " + ", ".join(f"{st} {prob.worst[st]:.3f}" for st in gv.ATTN_STAGES) +
          f" | {checked} sentinel elements checked")
