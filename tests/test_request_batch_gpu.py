"""Request batches whose requests run their own schedules, on the MI355X: the three per-image kernels (bc_scheduler_step_requests, the
`_requests` assemblies, bc_timestep_embedding_rows) against fp64 host rows and against the scalar kernels' bits; the mixed edit against
the reference's own loop outputs (loop_tiny.npz) and against every request run alone; uniform lists against the scalar request batch, bit
for bit; plan / graph caching across mixes of values; a compiled mixed plan replayed through the plan runtime; the dispatcher op."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.common import TINY, g, psnr, tiny_weights  # noqa: E402
from tests.gpu_common import make_pipeline  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)
DEV = "cuda:0"
STEPS, GUIDANCE = [4, 6, 5], [7.5, 3.0, 1.0]
WINDOWS, STRENGTHS = ((0.0, 1.0), (0.2, 0.7), (0.0, 0.5)), [1.0, 0.0, 1.7]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-9))


# ------------------------------------------------------------------------------------------------------------------ 1. step kernel
def _request_rows(kind, lengths, nsteps):
    """coef [B][nsteps][16]: request b = the first lengths[b] rows of a `kind` table of its own (another step count per request, so the
    rows differ), its own guidance scale in column 11, finished rows (column 15) behind them."""
    from blobctrl_amd.schedulers import DPMSolverMultistepTable, EulerAncestralTable, HeunTable
    make = {"heun": HeunTable, "dpm3": lambda: DPMSolverMultistepTable(solver_order=3), "eulera": EulerAncestralTable}[kind]
    coef = torch.zeros(len(lengths), nsteps, 16)
    for b, n in enumerate(lengths):
        rows = make().set_timesteps(8 + b).coef
        assert rows.shape[0] >= n
        coef[b, :n] = rows[:n]
        coef[b, n:, 14] = coef[b, n:, 15] = 1.0
        coef[b, :, 11] = GUIDANCE[b]
    return coef


def _host_row(c, e, x, hist_b, noise):
    """fp64: one table row on one image (tests/test_euler_gpu.py `_host_step`, after the guidance): (x', [x0, m0, x_c])."""
    c = c.double()
    m0, m1, last = (hist_b[k].double() for k in range(3))
    xd, e = x.double(), e.double()
    x0 = xd * c[0] - e * c[1]
    xc = c[3] * last + c[4] * m0 + c[5] * m1 + c[6] * x0 if c[2] != 0 else xd
    xn = c[7] * xc + c[8] * x0 + c[9] * m0 + c[10] * e + c[13] * m1
    if noise is not None:
        xn = xn + c[12] * noise.double()
    return xn, torch.stack([x0, m0, xc])


@pytest.mark.parametrize("single", [0, 1])
@pytest.mark.parametrize("kind", ["heun", "dpm3", "eulera"])
def test_the_requests_step_applies_every_images_own_row_and_leaves_finished_images_alone(kind, single):
    from blobctrl_amd import _lib
    lib = _lib.load()
    B, h, w, nsteps, lengths = 3, 8, 8, 6, (4, 6, 5)
    per = 4 * h * w
    coef_host = _request_rows(kind, lengths, nsteps)
    third, noisy = kind == "dpm3", kind == "eulera"
    assert bool((coef_host[:, :, 13] != 0).any()) == third and bool((coef_host[:, :, 12] != 0).any()) == noisy
    assert kind != "heun" or bool((coef_host[:, :, 2] != 0).any())                       # corrector columns live
    coef = coef_host.to(DEV)
    noise_host = torch.stack([g(200 + i, B, 4, h, w) for i in range(nsteps)])
    noise = noise_host.to(DEV)
    x = (g(1, B, 4, h, w) * 3).to(DEV)
    hist = torch.zeros(3, B * per, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    eps_out = torch.full((B, 4, h, w), -77.0, device=DEV)
    Be = B if single else 2 * B

    def launch(tok):
        _lib.check(lib.bc_scheduler_step_requests(tok.data_ptr(), x.data_ptr(), coef.data_ptr(), idx.data_ptr(), hist.data_ptr(), B, h, w,
                                                  noise.data_ptr() if noisy else None, nsteps, int(third), single, eps_out.data_ptr(), 1,
                                                  _stream()), "bc_scheduler_step_requests")
        torch.cuda.synchronize()

    for i in range(nsteps):
        tok_host = g(100 + i, Be, h, 2 * w, 4) * 2
        if i >= lengths[0]:                                    # request 0 has finished: whatever the networks put out for it
            tok_host[0] = float("nan")
            if not single:
                tok_host[B] = float("nan")
        x_in, hist_in, eo_in = x.cpu(), hist.cpu().reshape(3, B, per), eps_out.cpu()
        launch(tok_host.to(DEV))
        x_out, hist_out, eo_out = x.cpu(), hist.cpu().reshape(3, B, per), eps_out.cpu()
        for b in range(B):
            if i >= lengths[b]:                                # bit for bit what it was
                assert torch.equal(x_out[b], x_in[b]) and torch.equal(hist_out[:, b], hist_in[:, b]) and torch.equal(eo_out[b], eo_in[b]), (i, b)
                continue
            right = tok_host.double()[:, :, w:, :].permute(0, 3, 1, 2)                   # [Be][4][h][w]
            e = right[b] if single else right[b] + float(coef_host[b, i, 11].double()) * (right[B + b] - right[b])
            xn, hr = _host_row(coef_host[b, i], e, x_in[b], hist_in[:, b].reshape(3, 4, h, w), noise_host[i, b] if noisy else None)
            for got, ref, what in ((x_out[b], xn, "latents"), (hist_out[:, b].reshape(3, 4, h, w), hr, "hist"), (eo_out[b], e, "eps_out")):
                err = (got.double() - ref).abs().max().item()
                assert err <= 1e-6 * ref.abs().max().item(), (kind, single, i, b, what, err)
        assert torch.isfinite(x_out).all() and torch.isfinite(hist_out).all() and torch.isfinite(eo_out).all(), i
    assert int(idx.item()) == nsteps
    # a step index outside the table leaves everything as it is, and `advance` still counts
    for start in (nsteps, -3):
        idx.fill_(start)
        before = (x.clone(), hist.clone(), eps_out.clone())
        launch((g(9, Be, h, 2 * w, 4) * 2).to(DEV))
        assert all(torch.equal(a, b_) for a, b_ in zip(before, (x, hist, eps_out))) and int(idx.item()) == start + 1


# ------------------------------------------------------------------------------------------------------------------ 2. assemblies
def _canvas(lat, img, score, feat, Bout, Cpad, dup, div):
    """tests/test_euler_gpu.py `_canvas` with a divisor PER LATENT (`div` [Blat] fp32, or None = no scaling)."""
    Blat, Bimg = lat.shape[0], img.shape[0]
    h, w = lat.shape[-2:]
    F = 0 if feat is None else feat.shape[1]
    X = torch.zeros(Bout, h, 2 * w, Cpad, dtype=torch.float16)
    noisy = torch.zeros(Bout, h, 2 * w, Cpad, dtype=torch.bool)
    x = lat if div is None else lat / div.reshape(-1, 1, 1, 1)
    for b in range(Bout):
        bi = b % Bimg
        X[b, :, :w, :4] = img[bi].permute(1, 2, 0).half()
        X[b, :, w:, :4] = x[b % Blat].permute(1, 2, 0).half()
        noisy[b, :, w:, :4] = True
        sc = torch.cat([score[bi], score[bi]], 1)
        X[b, :, :, 4] = sc.half()
        if F:
            X[b, :, :, 5:5 + F] = (sc[:, :, None] * feat[bi][None, None, :]).half()
        elif dup:
            X[b, :, :, 5] = sc.half()
    return X, noisy


def _im2col(X8):
    B, h, W, _ = X8.shape
    pad = torch.zeros(B, h + 2, W + 2, 8, dtype=X8.dtype)
    pad[:, 1:-1, 1:-1] = X8
    out = torch.zeros(B, h, W, 128, dtype=X8.dtype)
    for t in range(9):
        out[..., t * 8:t * 8 + 8] = pad[:, t // 3:t // 3 + h, t % 3:t % 3 + W]
    return out.reshape(B, h * W, 128)


@pytest.mark.parametrize("F", [0, 11])
@pytest.mark.parametrize("Bout,Bimg", [(2, 1), (6, 1), (6, 3)])
@pytest.mark.parametrize("h,w", [(8, 8), (5, 7)])
def test_requests_assemblies_divide_every_images_noisy_latents_by_its_own_divisor(h, w, Bout, Bimg, F):
    from blobctrl_amd import _lib
    from blobctrl_amd.schedulers import EulerDiscreteTable
    lib = _lib.load()
    Blat, nsteps = Bout // 2, 10
    # every image its own divisors: the Euler table's, spread apart per latent; the last row of latent 0 says "do not divide"
    coef_host = torch.stack([EulerDiscreteTable().set_timesteps(nsteps).coef for b in range(Blat)]).clone()
    for b in range(Blat):
        coef_host[b, :, 14] *= 1.0 + 0.37 * b
    coef_host[0, nsteps - 1, 14] = 0.0
    assert len(set(coef_host[:, :, 14].reshape(-1).tolist())) == Blat * nsteps
    coef = coef_host.to(DEV)
    lat = g(1, Blat, 4, h, w) * 9.0
    img, score = g(2, Bimg, 4, h, w), g(3, Bimg, h, w).abs()
    feat = g(4, Bimg, F) if F else None
    d_lat, d_img, d_score = lat.to(DEV), img.to(DEV), score.to(DEV)
    d_feat = feat.to(DEV) if F else None
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    Cpad = 8 if F == 0 else 16

    def plain(requests):
        X = torch.full((Bout, h, 2 * w, Cpad), 7.0, dtype=torch.float16, device=DEV)
        extra = (coef.data_ptr(), idx.data_ptr(), nsteps) if requests else ()
        fn = lib.bc_assemble_input_requests if requests else lib.bc_assemble_input
        _lib.check(fn(d_lat.data_ptr(), Blat, d_img.data_ptr(), d_score.data_ptr(), d_feat.data_ptr() if F else None, Bimg, F, Bout, h, w,
                      Cpad, 0, *extra, X.data_ptr(), _stream()), "assemble")
        torch.cuda.synchronize()
        return X.cpu()

    def im2col(requests, dup):
        X = torch.full((Bout, h * 2 * w, 128), 7.0, dtype=torch.float16, device=DEV)
        extra = (coef.data_ptr(), idx.data_ptr(), nsteps) if requests else ()
        fn = lib.bc_assemble_input_im2col_requests if requests else lib.bc_assemble_input_im2col
        _lib.check(fn(d_lat.data_ptr(), Blat, d_img.data_ptr(), d_score.data_ptr(), Bimg, Bout, h, w, dup, *extra, X.data_ptr(), _stream()),
                   "assemble_im2col")
        torch.cuda.synchronize()
        return X.cpu()

    forms = [("plain", plain, lambda div: _canvas(lat, img, score, feat, Bout, Cpad, 0, div))]
    if F == 0:
        for dup in (0, 1):
            def ref(div, dup=dup):
                X, noisy = _canvas(lat, img, score, None, Bout, 8, dup, div)
                return _im2col(X), _im2col(noisy)
            forms.append((f"im2col dup={dup}", lambda requests, dup=dup: im2col(requests, dup), ref))
    for what, run, ref in forms:
        unscaled = run(False)
        want0, noisy = ref(None)
        assert torch.equal(unscaled, want0), what
        for step in (0, nsteps // 2, nsteps - 1):
            idx.fill_(step)
            got = run(True)
            div = coef_host[:, step, 14].clone()
            div[div == 0] = 1.0                                                 # a zero divisor: that image is not divided
            want, _ = ref(div)
            assert torch.equal(got[~noisy], unscaled[~noisy]), (what, step)     # everything else: the unscaled kernel's bits
            assert torch.equal(got, want), (what, step)                         # the noisy entries: fp16(fp32(x) / c14_b), exactly
            assert not torch.equal(got[noisy], unscaled[noisy]) or (Blat == 1 and step == nsteps - 1), (what, step)
            if step == nsteps - 1:                                              # latent 0 (images 0 and Blat): the unscaled output
                per_img = got.reshape(Bout, -1)
                assert torch.equal(per_img[0], unscaled.reshape(Bout, -1)[0]) and torch.equal(per_img[Blat], unscaled.reshape(Bout, -1)[Blat])
        for step in (nsteps, nsteps + 2, -1):                                   # no table row: the unscaled kernel's output
            idx.fill_(step)
            assert torch.equal(run(True), unscaled), (what, step)
        assert int(idx.item()) == -1


# ------------------------------------------------------------------------------------------------------------------ 3. embedding rows
@pytest.mark.parametrize("cond", [False, True])
def test_embedding_rows_give_the_table_kernels_bits(cond):
    from blobctrl_amd import _lib
    lib = _lib.load()
    rows, dim, per_step = 12, 32, 4
    proj = (g(7, per_step, dim) * 0.3).to(DEV) if cond else None

    def table(ts):
        """bc_timestep_embedding_table[_cond] for len(ts) steps of `per_step` rows."""
        t = torch.tensor(ts, dtype=torch.float32, device=DEV)
        out = torch.zeros(len(ts) * per_step, dim, dtype=torch.float16, device=DEV)
        if cond:
            _lib.check(lib.bc_timestep_embedding_table_cond(t.data_ptr(), len(ts), per_step, dim, proj.data_ptr(), out.data_ptr(), _stream()), "table_cond")
        else:
            _lib.check(lib.bc_timestep_embedding_table(t.data_ptr(), len(ts), per_step, dim, out.data_ptr(), _stream()), "table")
        torch.cuda.synchronize()
        return out.cpu()

    def by_rows(ts):
        t = torch.tensor(ts, dtype=torch.float32, device=DEV)
        out = torch.zeros(len(ts), dim, dtype=torch.float16, device=DEV)
        _lib.check(lib.bc_timestep_embedding_rows(t.data_ptr(), len(ts), dim, proj.data_ptr() if cond else None, per_step if cond else 0,
                                                  out.data_ptr(), _stream()), "rows")
        torch.cuda.synchronize()
        return out.cpu()

    steps = [981.0, 500.0, 1.0]
    assert torch.equal(by_rows([t for t in steps for _ in range(per_step)]), table(steps))         # equal t in every row of a step
    distinct = [999.0, 981.0, 760.5, 593.502, 500.0, 479.508, 320.0, 250.0, 19.0, 1.0, 0.0, 7.25]
    assert len(distinct) == rows
    got = by_rows(distinct)
    for r, t in enumerate(distinct):                                                                # row by row: that kernel at that t
        assert torch.equal(got[r], table([t])[r % per_step]), (cond, r, t)
    assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------------------------ engine
def _loop_inputs():
    from oracle import blob_splat
    score = torch.from_numpy(blob_splat.splat_scores_from_ellipse([[40.0, 42.0], [20.0, 30.0], 25.0], 64, 64, 8, 8))
    return dict(latents=g(31, 1, 4, 8, 8), prompt=g(32, 2, 7, TINY["ctx"]), fg=g(33, 1, 4, 8, 8) * 0.18215 * 5,
                bg=g(34, 1, 4, 8, 8) * 0.18215 * 5, score=score, dino=g(35, 1, 1, TINY["feat"]))


@pytest.mark.parametrize("sname", ["unipc", "ddim"])
@pytest.mark.parametrize("graphs", [False, True])
def test_a_mixed_batch_of_two_matches_the_references_loops(sname, graphs):
    """4. The 5-step edit (window [0, 1]) and the 6-step edit (window [0, 0.67]) of loop_tiny.npz as ONE batch of two requests: each
    lands on the final latents of the reference's own loop, at the bars of test_denoise_loop_matches_reference."""
    z = np.load(os.path.join(GOLD, "loop_tiny.npz"))
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    pipe = make_pipeline(usd, bsd, scheduler=sname, use_graphs=graphs)
    w5, w6 = ([float(v) for v in z[f"{sname}_{n}_window"]] for n in (5, 6))
    assert (w5, [round(v, 2) for v in w6]) == ([0.0, 1.0], [0.0, 0.67])
    two = lambda t: torch.cat([t, t], 0)
    args = (torch.cat([a["prompt"][:1], a["prompt"][:1], a["prompt"][1:], a["prompt"][1:]], 0), two(a["fg"]), two(a["bg"]), two(a["score"]),
            two(a["dino"]))
    kw = dict(num_inference_steps=[5, 6], guidance_scale=[7.5, 7.5], latents=two(a["latents"]),
              blobnet_control_guidance_start=[w5[0], w6[0]], blobnet_control_guidance_end=[w5[1], w6[1]])
    out = pipe(*args, **kw).cpu().numpy()
    for b, n in enumerate((5, 6)):
        ref = z[f"{sname}_{n}_final"]
        e, p = _rel(out[b:b + 1], ref), psnr(out[b:b + 1], ref)
        print(f"{sname} graphs={graphs} request {b} ({n} steps): rel err {e:.3e}, PSNR {p:.1f} dB")
        assert e < 1e-2 and p > 40.0, (sname, n, e, p)
    assert np.array_equal(out, pipe(*args, **kw).cpu().numpy())                                 # a second call: bit-identical
    assert [t.tolist() for t in pipe.timesteps] == [pipe._scheduler_table(n).timesteps.tolist() for n in (5, 6)]
    if graphs:
        assert pipe.cache_stats["plans_recorded"] == 1 and pipe.cache_stats["loop_graph_captures"] == 1 and pipe.cache_stats["loop_graph_hits"] == 1


def _request_batch(B=3):
    return dict(prompt=torch.cat([g(92, B, 7, TINY["ctx"]), g(93, B, 7, TINY["ctx"])]), fg=g(94, B, 4, 8, 8), bg=g(95, B, 4, 8, 8),
                score=g(96, B, 2, 8, 8).abs().clamp(max=1), dino=g(97, B, 1, TINY["feat"]), latents=g(91, B, 4, 8, 8))


def _one(a, b, B=3):
    """Request b of a request batch as a call of its own."""
    return (torch.cat([a["prompt"][b:b + 1], a["prompt"][B + b:B + b + 1]]), a["fg"][b:b + 1], a["bg"][b:b + 1], a["score"][b:b + 1],
            a["dino"][b:b + 1])


def _schedulers():
    from blobctrl_amd import schedulers as S
    return {"dpm_2m_karras": lambda: S.DPMSolverMultistepScheduler(use_karras_sigmas=True),
            "dpm_3m": lambda: S.DPMSolverMultistepScheduler(solver_order=3),
            "dpm_sde": lambda: S.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"),
            "dpm_sde_generators": lambda: S.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"),
            "euler_karras": lambda: S.EulerDiscreteScheduler(**dict(SD, use_karras_sigmas=True)),
            "euler_ancestral": lambda: S.EulerAncestralDiscreteScheduler(**SD), "heun": lambda: S.HeunDiscreteScheduler(**SD),
            "ddim_eta": lambda: S.DDIMScheduler(), "lcm": lambda: S.LCMScheduler.from_config(S.DDIMScheduler().config)}


@pytest.fixture(scope="module")
def engine():
    usd, bsd = tiny_weights()
    return make_pipeline(usd, bsd, scheduler="ddim")


@pytest.mark.parametrize("name", sorted(_schedulers()))
def test_every_request_of_a_mixed_batch_equals_the_request_alone(engine, name):
    """5. Steps (4, 6, 5), guidance (7.5, 3.0, 1.0), windows ((0, 1), (0.2, 0.7), (0, 0.5)), strengths (1.0, 0.0, 1.7) in one batch: every
    request equals the same request run alone through the same engine, at the bar of
    test_request_batch_mixed_ops_equals_single_edits_tiny (the request alone takes the rank-1 conv_in collapse per edit, the batch per
    image: two fp16 realisations): < 1e-2 of scale and > 50 dB.  (LCM runs single-pass: its guidance is off for every request.)"""
    s = _schedulers()[name]()
    engine.set_scheduler(s.kind, s.table_params())
    a, B = _request_batch(), 3
    evals = [2 * n - 1 for n in STEPS] if name == "heun" else STEPS
    nmax = max(evals)
    gs = [1.0, 1.0, 1.0] if name == "lcm" else GUIDANCE
    etas = [0.0, 0.5, 1.0] if name == "ddim_eta" else None
    kw = dict(num_inference_steps=list(STEPS), guidance_scale=list(gs), blobnet_conditioning_scale=list(STRENGTHS),
              blobnet_control_guidance_start=[s_ for s_, _ in WINDOWS], blobnet_control_guidance_end=[e_ for _, e_ in WINDOWS])
    if etas:
        kw["eta"] = etas
    noisy = name in ("dpm_sde", "dpm_sde_generators", "euler_ancestral", "ddim_eta", "lcm")
    noise = g(98, nmax, B, 4, 8, 8) if noisy and name != "dpm_sde_generators" else None
    if name == "dpm_sde_generators":
        kw["generator"] = [torch.Generator().manual_seed(500 + b) for b in range(B)]
    elif noisy:
        kw["variance_noise"] = noise
    batched = engine.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], latents=a["latents"], **kw).cpu().numpy()
    assert batched.shape == (B, 4, 8, 8) and np.isfinite(batched).all()
    assert next(reversed(engine._plans))[-1] == "requests"
    for b in range(B):
        alone = dict(num_inference_steps=STEPS[b], guidance_scale=gs[b], blobnet_conditioning_scale=STRENGTHS[b],
                     blobnet_control_guidance_start=WINDOWS[b][0], blobnet_control_guidance_end=WINDOWS[b][1])
        if etas:
            alone["eta"] = etas[b]
        if name == "dpm_sde_generators":
            alone["generator"] = torch.Generator().manual_seed(500 + b)
        elif noisy and (etas is None or etas[b] > 0):
            alone["variance_noise"] = noise[:evals[b], b:b + 1]
        single = engine.denoise(*_one(a, b), latents=a["latents"][b:b + 1], **alone).cpu().numpy()
        e, p = _rel(batched[b:b + 1], single), psnr(batched[b:b + 1], single)
        print(f"{name} request {b}: mixed batch vs the request alone rel {e:.3e}, PSNR {p:.1f} dB")
        assert e < 1e-2 and p > 50.0, (name, b, e, p)
    assert _rel(batched[0:1], batched[2:3]) > 1e-2                                                # (the requests really differ)


@pytest.mark.parametrize("name", ["ddim", "euler_karras", "dpm_sde_generators", "heun"])
def test_uniform_lists_give_the_scalar_request_batchs_bits(engine, name):
    """6. Lists of B equal values: the same arithmetic on the same GEMM shapes as the scalar request-batch call - bit-identical latents."""
    from blobctrl_amd import schedulers as S
    s = S.DDIMScheduler() if name == "ddim" else _schedulers()[name]()
    engine.set_scheduler(s.kind, s.table_params())
    a, B = _request_batch(), 3
    args = (a["prompt"], a["fg"], a["bg"], a["score"], a["dino"])
    gens = lambda: dict(generator=[torch.Generator().manual_seed(700 + b) for b in range(B)]) if name == "dpm_sde_generators" else {}
    scalar = engine.denoise(*args, latents=a["latents"], num_inference_steps=5, guidance_scale=4.0, blobnet_conditioning_scale=list(STRENGTHS),
                            blobnet_control_guidance_start=0.0, blobnet_control_guidance_end=0.7, **gens())
    assert "requests" not in next(reversed(engine._plans))
    listed = engine.denoise(*args, latents=a["latents"], num_inference_steps=[5] * B, guidance_scale=[4.0] * B,
                            blobnet_conditioning_scale=list(STRENGTHS), blobnet_control_guidance_start=[0.0] * B,
                            blobnet_control_guidance_end=[0.7] * B, **gens())
    assert next(reversed(engine._plans))[-1] == "requests"
    assert torch.equal(scalar, listed), (name, _rel(listed.cpu().numpy(), scalar.cpu().numpy()))
    mixed = engine.denoise(*args, latents=a["latents"], num_inference_steps=5, guidance_scale=[4.0] * B,              # scalars and lists mix
                           blobnet_conditioning_scale=list(STRENGTHS), blobnet_control_guidance_end=[0.7] * B, **gens())
    assert torch.equal(scalar, mixed)


def test_other_values_replay_the_same_plan_and_graph():
    """7. Tables, timesteps, scales and guidance are per-edit data: another mix with the same nmax and active pattern is a plan hit and a
    graph hit; a scalar call in between keeps its own plan, and every result stays what it was."""
    usd, bsd = tiny_weights()
    pipe = make_pipeline(usd, bsd, scheduler="ddim")
    a, B = _request_batch(), 3
    args = (a["prompt"], a["fg"], a["bg"], a["score"], a["dino"])
    first = dict(num_inference_steps=[4, 6, 5], guidance_scale=[7.5, 3.0, 1.0], blobnet_control_guidance_end=[1.0, 0.7, 0.5])
    other = dict(num_inference_steps=[6, 3, 2], guidance_scale=[2.0, 9.0, 5.0], blobnet_control_guidance_end=[0.67, 1.0, 1.0],
                 blobnet_conditioning_scale=[0.5, 1.0, 0.0])                     # (active in steps 0-3 again: any request active)
    x1 = pipe(*args, latents=a["latents"], **first)
    st = dict(pipe.cache_stats)
    assert st["plans_recorded"] == 1 and st["loop_graph_captures"] == 1 and st["plan_hits"] == 0 and st["loop_graph_hits"] == 0
    x2 = pipe(*args, latents=a["latents"], **other)
    st = dict(pipe.cache_stats)
    assert st["plans_recorded"] == 1 and st["loop_graph_captures"] == 1 and st["plan_hits"] == 1 and st["loop_graph_hits"] == 1
    assert _rel(x2.cpu().numpy(), x1.cpu().numpy()) > 1e-2
    xs = pipe(*args, latents=a["latents"], num_inference_steps=6, guidance_scale=7.5, blobnet_control_guidance_end=0.67)
    st = dict(pipe.cache_stats)
    assert st["plans_recorded"] == 2 and st["loop_graph_captures"] == 2 and len(pipe._plans) == 2
    assert torch.equal(pipe(*args, latents=a["latents"], **first), x1) and torch.equal(pipe(*args, latents=a["latents"], **other), x2)
    assert torch.equal(pipe(*args, latents=a["latents"], num_inference_steps=6, guidance_scale=7.5, blobnet_control_guidance_end=0.67), xs)
    st = dict(pipe.cache_stats)
    assert st["plans_recorded"] == 2 and st["loop_graph_captures"] == 2 and st["plan_hits"] == 4 and st["loop_graph_hits"] == 4


def test_callbacks_traces_and_teacher_latents_of_a_mixed_batch(engine):
    """`callback_on_step_end` is given the [B] timesteps of the step; a trace has nmax entries; teacher latents past a request's end are
    ignored for that request."""
    from blobctrl_amd import schedulers as S
    s = S.DDIMScheduler()
    engine.set_scheduler(s.kind, s.table_params())
    a, B = _request_batch(), 3
    args = (a["prompt"], a["fg"], a["bg"], a["score"], a["dino"])
    kw = dict(num_inference_steps=list(STEPS), guidance_scale=list(GUIDANCE), latents=a["latents"])
    plain = engine.denoise(*args, trace=[], **kw)                                                 # (step by step, as the runs below)
    seen, trace = [], []
    out = engine.denoise(*args, callback_on_step_end=lambda p, i, t, d: seen.append((i, t.clone())), trace=trace, **kw)
    assert torch.equal(out, plain) and len(trace) == 6 and [i for i, _ in seen] == list(range(6))
    tabs = [engine._scheduler_table(n).timesteps for n in STEPS]
    for i, t in seen:
        assert t.shape == (B,) and t.tolist() == [int(tb[min(i, len(tb) - 1)]) for tb in tabs]
    assert torch.equal(trace[4][1][0], trace[3][1][0]) and not torch.equal(trace[4][1][1], trace[3][1][1])     # request 0 finished at step 4
    # teacher forcing with the run's own latents reproduces it; garbage past a request's end changes nothing for that request
    teacher = [a["latents"].to(DEV)] + [t[1] for t in trace[:-1]]
    teacher[5] = teacher[5].clone()
    teacher[5][0] = float("nan")                                                                   # (request 0 ended after step 3)
    forced = engine.denoise(*args, teacher_latents=teacher, **kw)
    assert torch.equal(forced, plain)


# ------------------------------------------------------------------------------------------------------------------ 8. plan runtime
def _hip():
    """The HIP runtime this process already runs on (the one torch loaded), for copies into a loaded plan's buffers."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    hip.hipMemset.argtypes, hip.hipMemset.restype = [C.c_void_p, C.c_int, C.c_size_t], C.c_int
    return hip


def _read_io(path):
    raw = open(path, "rb").read()
    n, o, out = struct.unpack_from("<I", raw, 0)[0], 4, {}
    for _ in range(n):
        name = raw[o:o + 32].split(b"\0")[0].decode()
        nbytes = struct.unpack_from("<Q", raw, o + 32)[0]
        out[name] = raw[o + 40:o + 40 + nbytes]
        o += 40 + nbytes
    return out


def test_a_compiled_mixed_plan_replays_to_the_engines_latents(tmp_path):
    """tools/make_plan_fixture.py --requests compiles the mixed Euler edit WITHOUT a GPU (a child process that sees none); the file is
    loaded here through the plan API (bc_plan_load, bc_plan_buffer, bc_step, bc_plan_capture_loop, bc_graph_launch) and must land on what
    the engine computes for the same edit, eagerly and as one whole-loop graph: tests/c/plan_edit.c's bar, 1e-2 of scale."""
    from blobctrl_amd import _lib, schedulers as S
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_plan_fixture as fx
    lib = _lib.load()
    usd, bsd = tiny_weights()
    eng = make_pipeline(usd, bsd, scheduler="ddim")
    s = S.EulerDiscreteScheduler(steps_offset=1)
    eng.set_scheduler(s.kind, s.table_params())
    a = fx.request_inputs()
    mine = eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], latents=a["latents"], **fx.REQUESTS).cpu().numpy()
    assert np.isfinite(mine).all()
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")          # the compile step must not need a GPU
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_plan_fixture.py"), str(tmp_path), "--requests"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    path = str(tmp_path / "tiny_edit.bcplan")
    assert struct.unpack("<I", open(path, "rb").read()[4:8])[0] == 8
    io = _read_io(str(tmp_path / "tiny_edit_io.bin"))
    plan = C.c_void_p()
    _lib.check(lib.bc_plan_load(path.encode(), C.byref(plan)), "bc_plan_load")
    try:
        hip = _hip()

        def buffer(name):
            p, n = C.c_void_p(), C.c_longlong()
            _lib.check(lib.bc_plan_buffer(plan, name.encode(), C.byref(p), C.byref(n)), f"bc_plan_buffer({name})")
            return p, n.value

        def reset():
            torch.cuda.synchronize()
            for name in ("latents", "ctx", "fg_lat", "bg_lat", "bg_score", "fg_score", "feat", "feat16"):
                p, n = buffer(name)
                assert n == len(io[name]), name
                assert hip.hipMemcpy(p, io[name], n, 1) == 0, name                # (host to device)
            for name in ("step_idx", "hist"):
                p, n = buffer(name)
                assert hip.hipMemset(p, 0, n) == 0, name
            torch.cuda.synchronize()

        def result():
            torch.cuda.synchronize()
            p, n = buffer("latents")
            host = np.empty(mine.shape, np.float32)
            assert n == host.nbytes and hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), p, n, 2) == 0       # (device to host)
            return host

        seg = {n: lib.bc_plan_find_segment(plan, n.encode()) for n in ("prologue", "step_active", "step_inactive")}
        assert min(seg.values()) >= 0
        seq = np.frombuffer(io["sequence"], np.int32).tolist()
        assert seq == [1, 1, 1, 1, 0, 0]
        ids = [seg["prologue"]] + [seg["step_active"] if on else seg["step_inactive"] for on in seq]
        streams = [torch.cuda.Stream(DEV) for _ in range(3)]
        arr = (C.c_void_p * 3)(*[st.cuda_stream for st in streams])
        reset()
        for i in ids:                                                            # eager replay of the launch lists
            _lib.check(lib.bc_step(plan, i, arr, 3), "bc_step")
        eager = result()
        print(f"eager replay vs the engine: rel {_rel(eager, mine):.3e}")
        assert _rel(eager, mine) < 1e-2
        graph = C.c_void_p()
        _lib.check(lib.bc_plan_capture_loop(plan, (C.c_int * len(ids))(*ids), len(ids), arr, 3, C.byref(graph)), "bc_plan_capture_loop")
        try:
            for rep in range(2):
                reset()
                _lib.check(lib.bc_graph_launch(graph, streams[0].cuda_stream), "bc_graph_launch")
                got = result()
                print(f"whole-loop graph (replay {rep}) vs the engine: rel {_rel(got, mine):.3e}")
                assert _rel(got, mine) < 1e-2 and np.array_equal(got, eager)
        finally:
            torch.cuda.synchronize()
            lib.bc_graph_destroy(graph)
    finally:
        lib.bc_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------------------------ 9. dispatcher
def test_list_arguments_reach_the_denoise_requests_op(engine):
    from torch.utils._python_dispatch import TorchDispatchMode
    from blobctrl_amd import ops, schedulers as S
    s = S.DDIMScheduler()
    engine.set_scheduler(s.kind, s.table_params())
    a, B = _request_batch(), 3
    args = (a["prompt"], a["fg"], a["bg"], a["score"], a["dino"])
    lists = ([4, 6, 5], [7.5, 3.0, 1.0], [1.0, 0.0, 1.7], [0.0, 0.2, 0.0], [1.0, 0.7, 0.5])
    torch.library.opcheck(torch.ops.blobctrl.denoise_requests, (*args, a["latents"], *lists, ops.register(engine)),
                          test_utils=("test_schema", "test_faketensor"))
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if "blobctrl" in str(func):
                seen.append(str(func))
            return func(*args, **(kwargs or {}))
    kw = dict(num_inference_steps=lists[0], guidance_scale=lists[1], blobnet_conditioning_scale=lists[2],
              blobnet_control_guidance_start=lists[3], blobnet_control_guidance_end=lists[4])
    with Spy():
        x = engine(*args, latents=a["latents"], **kw)
        y = engine(*args, latents=a["latents"], num_inference_steps=[4, 6, 5])              # one list, the rest scalar defaults
        z = engine(*args, latents=a["latents"], num_inference_steps=4, guidance_scale=7.5)  # no list: the op it always went through
    assert seen == ["blobctrl.denoise_requests.default", "blobctrl.denoise_requests.default", "blobctrl.denoise.default"]
    assert torch.equal(x, engine.denoise(*args, latents=a["latents"], **kw))
    assert torch.equal(y, engine.denoise(*args, latents=a["latents"], num_inference_steps=[4, 6, 5]))
    assert torch.equal(z, engine.denoise(*args, latents=a["latents"], num_inference_steps=4, guidance_scale=7.5))
