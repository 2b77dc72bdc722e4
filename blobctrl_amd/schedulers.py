"""Scheduler coefficient tables for the hipGraph-captured denoise loop.

The reference schedulers mutate Python state and build small tensors every step
(D/schedulers/scheduling_unipc_multistep.py:822-901, scheduling_ddim.py:342-468).  Every quantity they compute depends
only on the sigma / alpha tables, so each step is a fixed LINEAR combination of
    x (current latents), eps (guided noise prediction), last_sample, x0_{i-1}, x0_{i-2}
whose scalar coefficients are precomputed here per step index, uploaded once, and applied by one fused kernel
(`bc_cfg_scheduler_step`).  Row layout (16 floats per step):
    [0] 1/alpha_t   [1] sigma_t/alpha_t                    x0   = x*c0 - eps*c1
    [2] use_corrector
    [3] cc_x [4] cc_m0 [5] cc_m1 [6] cc_mt                 x_c  = c3*last + c4*x0_{i-1} + c5*x0_{i-2} + c6*x0      (UniC)
    [7] cp_x [8] cp_m0 [9] cp_m1 [10] cp_eps               x'   = c7*x_c + c8*x0 + c9*x0_{i-1} + c10*eps           (UniP / DDIM)
    [11] guidance scale (filled by the engine)
    [12] std_dev_t                                         x'  += c12*noise[i]     (stochastic DDIM, eta > 0; SDE-DPM-Solver++; 0 otherwise)
    [13] cp_m2                                             x'  += c13*x0_{i-2}     (third-order DPM-Solver++, `bc_cfg_scheduler_step3`)
    [14] input divisor sqrt(sigma_t^2 + 1)                 the networks read x / c14 (`scale_model_input`; the sigma-space schedulers Euler,
                                                           Euler-ancestral and Heun: `bc_assemble_input_scaled`, `bc_assemble_input_im2col_scaled`).
                                                           0 in every other table: UniPC, DDIM and DPM-Solver++ do not scale their input and
                                                           never reach a kernel that reads the column
    [15] finished                                          only in the per-request tables of a request batch whose requests run their own
                                                           schedules (`request_tables`, coef [B][nmax][16], `bc_scheduler_step_requests`):
                                                           != 0 marks a row past the request's last step - "leave this image alone", the
                                                           step neither reads its eps nor writes its latents / history.  0 in every table
                                                           a scheduler builds; no other kernel reads the column
Scalar maths follows the reference in fp32 torch CPU ops (same operation order) so the tables match it to rounding.
DPM-Solver++ (scheduling_dpmsolver_multistep.py) fills c0 / c1 (x0), c7 (x), c8 (x0), c9 (x0_{i-1}), c12 (SDE noise) and c13 (order 3).
The sigma-space (k-diffusion) schedulers work on x = x0 + sigma * eps: an Euler step x' = x + (sigma_next - sigma) * eps is c0 = 1,
c1 = sigma, c7 = 1, c10 = sigma_next - sigma; Euler-ancestral steps down to sigma_down and adds c12 = sigma_up times the step's noise; Heun's
second stage reads the first stage's x (`last`) and x0 (`m0`) through the corrector columns c2 - c4.
LCMScheduler (scheduling_lcm.py:498-592) is linear too: denoised = c_out * x0 + c_skip * x, x' = sqrt(abar_prev) * denoised +
sqrt(1 - abar_prev) * noise, i.e. c0 = 1/sqrt(abar_t), c1 = sqrt(1 - abar_t)/sqrt(abar_t), c7 = sqrt(abar_prev) * c_skip,
c8 = sqrt(abar_prev) * c_out, c12 = sqrt(1 - abar_prev); the last step returns `denoised` itself: c7 = c_skip, c8 = c_out, c12 = 0.

SD-1.5 scheduler config: betas 0.00085 -> 0.012 scaled_linear, 1000 train steps, steps_offset 1,
epsilon prediction; UniPC: solver_order 2, bh2, predict_x0, lower_order_final, linspace spacing, final sigma 0;
DDIM: leading spacing, clip_sample False, set_alpha_to_one False; eta >= 0 (eta > 0 adds std_dev_t * variance_noise, the noise being
drawn on the host in the reference's order: scheduling_ddim.py:438-466).
"""
import numpy as np
import torch


def _alphas_cumprod(num_train, beta_start, beta_end):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


class _Base:
    order = 1
    init_noise_sigma = 1.0
    scales_input = False                                                  # True: the networks read x / c14 (the sigma-space tables)

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
        self.num_train = num_train_timesteps
        self.alphas_cumprod = _alphas_cumprod(num_train_timesteps, beta_start, beta_end)
        self.timesteps = None
        self.coef = None

    def scale_model_input(self, sample, timestep=None):        # identity for both (pipe:1032)
        return sample

    def table(self) -> torch.Tensor:
        """[num_steps, 16] float32 coefficient rows."""
        return self.coef

    @staticmethod
    def _as(sigma):                                                       # (alpha_t, sigma_t) of a sigma (dpmsolver_multistep.py:468-472)
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def _blend_pair(self, i):
        """(a, s) of add_noise(., ., timesteps[i]): sqrt(abar), sqrt(1 - abar) (add_noise of scheduling_ddim.py / scheduling_lcm.py)."""
        abar = self.alphas_cumprod[self.timesteps[i]]
        return abar ** 0.5, (1 - abar) ** 0.5

    def blend_rows(self) -> torch.Tensor:
        """[num_steps, 2] float32 for a masked edit (`bc_blend_scheduler_step`'s blend_table): row i = (a, s) with
        add_noise(image, noise, timesteps[i + 1]) = a * image + s * noise - what the kept region holds after step i - and the last row
        (1, 0): the image itself (pipeline_stable_diffusion_inpaint.py:1272-1285)."""
        n = len(self.timesteps)
        rows = torch.zeros(n, 2, dtype=torch.float32)
        for i in range(n - 1):
            rows[i, 0], rows[i, 1] = self._blend_pair(i + 1)
        rows[n - 1, 0] = 1.0
        return rows

    def _lam(self, i):                                                    # lambda = log(alpha) - log(sigma) of self.sigmas[i]
        a, s = self._as(self.sigmas[i])
        return torch.log(a) - torch.log(s)


class UniPCTable(_Base):
    """UniPCMultistepScheduler restated as a coefficient table (scheduling_unipc_multistep.py:282-360, 453-901)."""

    def __init__(self, solver_order=2, **kw):
        super().__init__(**kw)
        assert solver_order == 2, "the coefficient form is written for the reference's solver_order=2 / bh2"

    def _blend_pair(self, i):                                             # (alpha_t, sigma_t) of the interpolated sigma, as its add_noise
        return self._as(self.sigmas[i])

    def set_timesteps(self, n, device=None):
        ts = np.linspace(0, self.num_train - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = n
        self.coef = self._build(n)
        return self

    @staticmethod
    def _bh(h, rks, order):
        hh = -h
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        B_h = torch.expm1(hh)
        R, b = [], []
        fact = 1
        for i in range(1, order + 1):
            R.append(torch.pow(rks, i - 1))
            b.append(h_phi_k * fact / B_h)
            fact *= i + 1
            h_phi_k = h_phi_k / hh - 1 / fact
        return h_phi_1, B_h, torch.stack(R), torch.tensor(b)

    def _build(self, n):
        coef = torch.zeros(n, 16, dtype=torch.float32)
        lower_order_nums = 0
        prev_order = None
        for i in range(n):
            alpha_t, sigma_t = self._as(self.sigmas[i])
            coef[i, 0] = 1.0 / alpha_t
            coef[i, 1] = sigma_t / alpha_t
            # ---- UniC corrector with the PREVIOUS step's order (:854-868, :652-787)
            if i > 0:
                order = prev_order
                alpha_s0, sigma_s0 = self._as(self.sigmas[i - 1])
                lam_t = torch.log(alpha_t) - torch.log(sigma_t)
                lam_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
                h = lam_t - lam_s0
                rks = []
                for k in range(1, order):
                    rks.append((self._lam(i - (k + 1)) - lam_s0) / h)
                rks.append(1.0)
                rks_t = torch.tensor(rks)
                h_phi_1, B_h, R, b = self._bh(h, rks_t, order)
                rhos_c = torch.tensor([0.5]) if order == 1 else torch.linalg.solve(R, b)
                cc_x = sigma_t / sigma_s0
                cc_m0 = -alpha_t * h_phi_1
                cc_m1 = torch.tensor(0.0)
                cc_mt = -alpha_t * B_h * rhos_c[-1]
                cc_m0 = cc_m0 + alpha_t * B_h * rhos_c[-1]                 # -(alpha B_h rho_last) * (-m0)
                if order == 2:
                    w = alpha_t * B_h * rhos_c[0] / rks_t[0]               # D1 = (m1 - m0) / rk
                    cc_m1 = -w
                    cc_m0 = cc_m0 + w
                coef[i, 2] = 1.0
                coef[i, 3], coef[i, 4], coef[i, 5], coef[i, 6] = cc_x, cc_m0, cc_m1, cc_mt
            # ---- UniP predictor (:877-888, :523-650)
            this_order = min(2, n - i)
            this_order = min(this_order, lower_order_nums + 1)
            alpha_n, sigma_n = self._as(self.sigmas[i + 1])
            lam_n = torch.log(alpha_n) - torch.log(sigma_n)
            lam_t = torch.log(alpha_t) - torch.log(sigma_t)
            h = lam_n - lam_t
            rks = []
            for k in range(1, this_order):
                rks.append((self._lam(i - k) - lam_t) / h)
            rks.append(1.0)
            rks_t = torch.tensor(rks)
            h_phi_1, B_h, R, b = self._bh(h, rks_t, this_order)
            cp_x = sigma_n / sigma_t
            cp_m0 = -alpha_n * h_phi_1
            cp_m1 = torch.tensor(0.0)
            if this_order == 2:
                w = alpha_n * B_h * 0.5 / rks_t[0]                          # rhos_p = 0.5 (:619-620)
                cp_m1 = -w
                cp_m0 = cp_m0 + w
            coef[i, 7], coef[i, 8], coef[i, 9] = cp_x, cp_m0, cp_m1
            prev_order = this_order
            if lower_order_nums < 2:
                lower_order_nums += 1
        assert torch.isfinite(coef).all(), "non-finite UniPC coefficient"
        return coef


class DDIMTable(_Base):
    """DDIMScheduler as a coefficient table (scheduling_ddim.py:253-261, 297-340, 342-468); eta > 0 fills column 12 with std_dev_t."""

    def set_timesteps(self, n, device=None, eta=0.0):
        ratio = self.num_train // n
        ts = (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.int64) + 1
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = n
        self.eta = float(eta)
        coef = torch.zeros(n, 16, dtype=torch.float32)
        final_alpha = self.alphas_cumprod[0]
        for i, t in enumerate(ts.tolist()):
            prev_t = t - ratio
            a_t = self.alphas_cumprod[t]
            a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else final_alpha
            variance = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
            std = eta * variance ** 0.5
            coef[i, 0] = 1.0 / a_t ** 0.5
            coef[i, 1] = (1 - a_t) ** 0.5 / a_t ** 0.5
            coef[i, 8] = a_prev ** 0.5
            coef[i, 10] = (1 - a_prev - std ** 2) ** 0.5
            coef[i, 12] = std
            if not torch.isfinite(coef[i]).all():
                raise ValueError(f"eta = {eta}: DDIM step {i} (timestep {t}) has 1 - alpha_prev - std_dev_t^2 < 0, "
                                 "no finite update (the reference would produce NaN latents)")
        self.coef = coef
        return self


# the DPMSolverMultistepScheduler options a coefficient table depends on (the engine keys its tables and plans on them)
DPM_OPTIONS = dict(solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, euler_at_final=False,
                   use_karras_sigmas=False, use_lu_lambdas=False, final_sigmas_type="zero", lambda_min_clipped=-float("inf"),
                   timestep_spacing="linspace", steps_offset=0)


class DPMSolverMultistepTable(_Base):
    """DPMSolverMultistepScheduler as a coefficient table (scheduling_dpmsolver_multistep.py:306-408 timesteps / sigmas, 612-887 the
    first-, second- and third-order updates, 963-995 the order of each step).  Data prediction only ("dpmsolver++" and its SDE form
    "sde-dpmsolver++"): x0 = (x - sigma_s0 * eps) / alpha_s0 in c0 / c1, the update x' = c7 * x + c8 * x0 + c9 * x0_{i-1} + c13 * x0_{i-2}
    (+ c12 * noise for the SDE).  Caller `timesteps` are taken as the reference takes them."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, **options):
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end)
        unknown = set(options) - set(DPM_OPTIONS)
        if unknown:
            raise TypeError(f"unknown DPM-Solver option(s) {sorted(unknown)}")
        o = dict(DPM_OPTIONS, **options)
        if o["algorithm_type"] not in ("dpmsolver++", "sde-dpmsolver++"):
            raise NotImplementedError(f"algorithm_type {o['algorithm_type']!r} is not tabulated (dpmsolver++ and sde-dpmsolver++ are)")
        if o["solver_type"] not in ("midpoint", "heun"):
            raise NotImplementedError(f"solver_type {o['solver_type']!r} is not tabulated (midpoint and heun are)")
        if o["solver_order"] not in (1, 2, 3):
            raise NotImplementedError(f"solver_order {o['solver_order']} is not tabulated (1, 2 and 3 are)")
        if o["solver_order"] == 3 and o["algorithm_type"] == "sde-dpmsolver++":
            raise NotImplementedError("solver_order=3 with algorithm_type 'sde-dpmsolver++': the reference's third-order update has no "
                                      "SDE branch (scheduling_dpmsolver_multistep.py:871-886)")
        self.options = o
        self.sde = o["algorithm_type"] == "sde-dpmsolver++"
        self.sigmas = None
        self.num_inference_steps = None

    def _blend_pair(self, i):                                             # (alpha_t, sigma_t) of the interpolated sigma, as its add_noise
        return self._as(self.sigmas[i])

    # ---- scheduling_dpmsolver_multistep.py:306-408
    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None):
        o = self.options
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `timesteps`.")
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `custom_timesteps`.")
        if timesteps is not None and o["use_karras_sigmas"]:
            raise ValueError("Cannot use `timesteps` with `config.use_karras_sigmas = True`")
        if timesteps is not None and o["use_lu_lambdas"]:
            raise ValueError("Cannot use `timesteps` with `config.use_lu_lambdas = True`")
        ac = self.alphas_cumprod
        if timesteps is not None:
            ts = np.array(timesteps).astype(np.int64)
        else:
            lambda_t = torch.log(torch.sqrt(ac)) - torch.log(torch.sqrt(1 - ac))
            clipped_idx = torch.searchsorted(torch.flip(lambda_t, [0]), o["lambda_min_clipped"])
            last_timestep = ((self.num_train - clipped_idx).numpy()).item()
            n = num_inference_steps
            if o["timestep_spacing"] == "linspace":
                ts = np.linspace(0, last_timestep - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
            elif o["timestep_spacing"] == "leading":
                step_ratio = last_timestep // (n + 1)
                ts = (np.arange(0, n + 1) * step_ratio).round()[::-1][:-1].copy().astype(np.int64)
                ts += o["steps_offset"]
            elif o["timestep_spacing"] == "trailing":
                step_ratio = self.num_train / n
                ts = np.arange(last_timestep, 0, -step_ratio).round().copy().astype(np.int64)
                ts -= 1
            else:
                raise ValueError(f"{o['timestep_spacing']} is not supported. Please make sure to choose one of 'linspace', 'leading' or "
                                 "'trailing'.")
        sigmas = (((1 - ac) / ac) ** 0.5).numpy().copy()
        log_sigmas = np.log(sigmas)
        if o["use_karras_sigmas"]:
            sigmas = np.flip(sigmas).copy()
            sigmas = self._convert_to_karras(sigmas, num_inference_steps)
            ts = np.array([self._sigma_to_t(s, log_sigmas) for s in sigmas]).round()
        elif o["use_lu_lambdas"]:
            lambdas = np.flip(log_sigmas.copy())
            lambdas = self._convert_to_lu(lambdas, num_inference_steps)
            sigmas = np.exp(lambdas)
            ts = np.array([self._sigma_to_t(s, log_sigmas) for s in sigmas]).round()
        else:
            sigmas = np.interp(ts, np.arange(0, len(sigmas)), sigmas)
        if o["final_sigmas_type"] == "sigma_min":
            sigma_last = float(((1 - ac[0]) / ac[0]) ** 0.5)
        elif o["final_sigmas_type"] == "zero":
            sigma_last = 0
        else:
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {o['final_sigmas_type']}")
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [sigma_last]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts).to(dtype=torch.int64)
        self.num_inference_steps = len(ts)
        self.coef = self._build()
        return self

    @staticmethod
    def _sigma_to_t(sigma, log_sigmas):                                   # :445-466
        log_sigma = np.log(np.maximum(sigma, 1e-10))
        dists = log_sigma - log_sigmas[:, np.newaxis]
        low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_sigmas[low_idx], log_sigmas[high_idx]
        w = np.clip((low - log_sigma) / (low - high), 0, 1)
        t = (1 - w) * low_idx + w * high_idx
        return t.reshape(sigma.shape)

    @staticmethod
    def _convert_to_karras(in_sigmas, num_inference_steps):               # :475-498 (the config has no sigma_min / sigma_max)
        sigma_min, sigma_max = in_sigmas[-1].item(), in_sigmas[0].item()
        rho = 7.0
        ramp = np.linspace(0, 1, num_inference_steps)
        min_inv_rho, max_inv_rho = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
        return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho

    @staticmethod
    def _convert_to_lu(in_lambdas, num_inference_steps):                  # :500-511
        lambda_min, lambda_max = in_lambdas[-1].item(), in_lambdas[0].item()
        rho = 1.0
        ramp = np.linspace(0, 1, num_inference_steps)
        min_inv_rho, max_inv_rho = lambda_min ** (1 / rho), lambda_max ** (1 / rho)
        return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho

    def step_orders(self):
        """The solver order of every step (step, :963-995): lower_order_nums, lower_order_final, lower_order_second."""
        o = self.options
        N = self.num_inference_steps
        orders, lower_order_nums = [], 0
        for i in range(N):
            lower_order_final = (i == N - 1) and (o["euler_at_final"] or (o["lower_order_final"] and N < 15)
                                                  or o["final_sigmas_type"] == "zero")
            lower_order_second = (i == N - 2) and o["lower_order_final"] and N < 15
            if o["solver_order"] == 1 or lower_order_nums < 1 or lower_order_final:
                orders.append(1)
            elif o["solver_order"] == 2 or lower_order_nums < 2 or lower_order_second:
                orders.append(2)
            else:
                orders.append(3)
            if lower_order_nums < o["solver_order"]:
                lower_order_nums += 1
        return orders

    def _build(self):
        o = self.options
        midpoint = o["solver_type"] == "midpoint"
        N = self.num_inference_steps
        coef = torch.zeros(N, 16, dtype=torch.float32)
        for i, order in enumerate(self.step_orders()):
            alpha_s0, sigma_s0 = self._as(self.sigmas[i])
            coef[i, 0] = 1.0 / alpha_s0
            coef[i, 1] = sigma_s0 / alpha_s0
            alpha_t, sigma_t = self._as(self.sigmas[i + 1])
            if float(sigma_t) == 0.0:
                # final step to sigma 0 (always first order, :963-967): lambda_t = h = +inf; the first-order rows have the finite limits
                # sigma_t / sigma_s0 (* e^-h) = 0, alpha_t (1 - e^-h) = alpha_t (1 - e^-2h) = alpha_t, sigma_t sqrt(1 - e^-2h) = 0
                assert order == 1
                coef[i, 8] = alpha_t
                continue
            lambda_t = torch.log(alpha_t) - torch.log(sigma_t)
            lambda_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
            h = lambda_t - lambda_s0
            if self.sde:
                c_x = sigma_t / sigma_s0 * torch.exp(-h)
                a = alpha_t * (1 - torch.exp(-2.0 * h))                     # weight of D0
                b = 0.5 * a if midpoint else alpha_t * ((1.0 - torch.exp(-2.0 * h)) / (-2.0 * h) + 1.0)   # weight of D1
                coef[i, 12] = sigma_t * torch.sqrt(1.0 - torch.exp(-2 * h))
            else:
                c_x = sigma_t / sigma_s0
                a = -(alpha_t * (torch.exp(-h) - 1.0))
                b = -0.5 * (alpha_t * (torch.exp(-h) - 1.0)) if midpoint else alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)
            coef[i, 7] = c_x
            if order == 1:                                                   # :654-679
                coef[i, 8] = a
            elif order == 2:                                                 # :723-802: D1 = (m0 - m1) / r0
                r0 = (lambda_s0 - self._lam(i - 1)) / h
                w = b * (1.0 / r0)
                coef[i, 8] = a + w
                coef[i, 9] = -w
            else:                                                            # :846-878 (dpmsolver++ only)
                lambda_s1, lambda_s2 = self._lam(i - 1), self._lam(i - 2)
                h_0, h_1 = lambda_s0 - lambda_s1, lambda_s1 - lambda_s2
                r0, r1 = h_0 / h, h_1 / h
                b = alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)              # x_t = c7 x + a D0 + b D1 - c D2 (whatever solver_type)
                c = alpha_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5)
                i0, i1 = 1.0 / r0, 1.0 / r1
                k, q = r0 / (r0 + r1), 1.0 / (r0 + r1)
                # D1_0 = i0 (m0 - m1), D1_1 = i1 (m1 - m2), D1 = D1_0 + k (D1_0 - D1_1), D2 = q (D1_0 - D1_1), expanded in m0, m1, m2
                coef[i, 8] = a + b * (1 + k) * i0 - c * q * i0
                coef[i, 9] = -b * ((1 + k) * i0 + k * i1) + c * q * (i0 + i1)
                coef[i, 13] = b * k * i1 - c * q * i1
        assert torch.isfinite(coef).all(), "non-finite DPM-Solver coefficient"
        return coef



# ---- the sigma-space (k-diffusion) schedulers: EulerDiscrete, EulerAncestralDiscrete, HeunDiscrete --------------------------------------
# the options a table depends on (the engine keys its tables and plans on them), with the reference's defaults
EULER_OPTIONS = dict(interpolation_type="linear", use_karras_sigmas=False, timestep_spacing="linspace", timestep_type="discrete",
                     steps_offset=0, final_sigmas_type="zero")
EULER_ANCESTRAL_OPTIONS = dict(timestep_spacing="linspace", steps_offset=0)
HEUN_OPTIONS = dict(use_karras_sigmas=False, timestep_spacing="linspace", steps_offset=0)


class _SigmaTable(_Base):
    """What the three sigma-space tables share: the spaced (float32, possibly fractional) timesteps, the interpolated sigmas,
    `init_noise_sigma` and the Euler row.  `scales_input`: the networks read x / sqrt(sigma^2 + 1), column 14."""
    scales_input = True
    _option_defaults = {}

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, **options):
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end)
        unknown = set(options) - set(self._option_defaults)
        if unknown:
            raise TypeError(f"unknown {type(self).__name__} option(s) {sorted(unknown)}")
        self.options = dict(self._option_defaults, **options)
        self.sigmas = None
        self.num_inference_steps = None

    def _train_sigmas(self):
        return (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy().copy()

    def _blend_pair(self, i):                                             # the latents live in sigma space: image + sigma * noise
        return 1.0, self.sigmas[i]                                        # (scheduling_euler_discrete.py add_noise)

    def _spaced(self, n):                                                 # scheduling_euler_discrete.py:357-381 (the same in all three)
        o = self.options
        if o["timestep_spacing"] == "linspace":
            return np.linspace(0, self.num_train - 1, n, dtype=np.float32)[::-1].copy()
        if o["timestep_spacing"] == "leading":
            step_ratio = self.num_train // n
            ts = (np.arange(0, n) * step_ratio).round()[::-1].copy().astype(np.float32)
            ts += o["steps_offset"]
            return ts
        if o["timestep_spacing"] == "trailing":
            step_ratio = self.num_train / n
            ts = np.arange(self.num_train, 0, -step_ratio).round().copy().astype(np.float32)
            ts -= 1
            return ts
        raise ValueError(f"{o['timestep_spacing']} is not supported. Please make sure to choose one of 'linspace', 'leading' or "
                         "'trailing'.")

    def _karras(self, sigmas, log_sigmas, n):                             # :395-397: fractional timesteps, not rounded
        sigmas = DPMSolverMultistepTable._convert_to_karras(sigmas, n)
        return sigmas, np.array([DPMSolverMultistepTable._sigma_to_t(s, log_sigmas) for s in sigmas])

    @property
    def init_noise_sigma(self):                                           # :244-250: of the CURRENT sigmas, so read it after set_timesteps
        sig = self.sigmas if self.sigmas is not None else torch.from_numpy(self._train_sigmas())
        max_sigma = sig.max()
        if self.options["timestep_spacing"] in ("linspace", "trailing"):
            return float(max_sigma)
        return float((max_sigma ** 2 + 1) ** 0.5)

    @staticmethod
    def _euler_row(row, sigma, target, up=None):
        """x0 = x - sigma * eps; x' = x + (target - sigma) * eps (+ up * noise); the networks read x / sqrt(sigma^2 + 1)."""
        row[0] = 1.0
        row[1] = sigma
        row[7] = 1.0
        row[10] = target - sigma
        row[14] = (sigma ** 2 + 1) ** 0.5
        if up is not None:
            row[12] = up


class EulerDiscreteTable(_SigmaTable):
    """EulerDiscreteScheduler as a coefficient table (scheduling_euler_discrete.py:301-420 timesteps / sigmas, 493-599 the step with
    s_churn = 0, i.e. gamma = 0 and sigma_hat = sigma).  Caller `timesteps` are taken as the reference takes them."""
    _option_defaults = EULER_OPTIONS

    def __init__(self, **kw):
        super().__init__(**kw)
        o = self.options
        if o["interpolation_type"] == "log_linear":
            raise NotImplementedError("interpolation_type 'log_linear' is not tabulated ('linear' is)")
        if o["timestep_type"] != "discrete":
            raise NotImplementedError(f"timestep_type {o['timestep_type']!r} is not tabulated ('discrete' is)")

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None):
        o = self.options
        if sigmas is not None:
            raise NotImplementedError("custom `sigmas` are not tabulated: pass num_inference_steps or `timesteps`")
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `timesteps` or `sigmas.")
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `timesteps` or `sigmas`.")
        if timesteps is not None and o["use_karras_sigmas"]:
            raise ValueError("Cannot set `timesteps` with `config.use_karras_sigmas = True`.")
        n = num_inference_steps if num_inference_steps is not None else len(timesteps)
        ts = np.array(timesteps).astype(np.float32) if timesteps is not None else self._spaced(n)
        sig = self._train_sigmas()
        log_sigmas = np.log(sig)
        if o["interpolation_type"] != "linear":
            raise ValueError(f"{o['interpolation_type']} is not implemented. Please specify interpolation_type to either 'linear' or "
                             "'log_linear'")
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        if o["use_karras_sigmas"]:
            sig, ts = self._karras(sig, log_sigmas, n)
        if o["final_sigmas_type"] == "sigma_min":
            sigma_last = ((1 - self.alphas_cumprod[0]) / self.alphas_cumprod[0]) ** 0.5
        elif o["final_sigmas_type"] == "zero":
            sigma_last = 0
        else:
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {o['final_sigmas_type']}")
        self.sigmas = torch.from_numpy(np.concatenate([sig, [sigma_last]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts.astype(np.float32))
        self.num_inference_steps = n
        coef = torch.zeros(n, 16, dtype=torch.float32)
        for i in range(n):
            self._euler_row(coef[i], self.sigmas[i], self.sigmas[i + 1])
        assert torch.isfinite(coef).all(), "non-finite Euler coefficient"
        self.coef = coef
        return self


class EulerAncestralTable(_SigmaTable):
    """EulerAncestralDiscreteScheduler as a coefficient table (scheduling_euler_ancestral_discrete.py:277-320, 345-440): an Euler step down
    to sigma_down, then sigma_up times the step's noise in column 12 - the steps end in bc_cfg_scheduler_step_noise.  The reference's
    set_timesteps takes no caller `timesteps`."""
    _option_defaults = EULER_ANCESTRAL_OPTIONS
    sde = True                                                            # a noise term in every step (the engine's stochastic plan)

    def set_timesteps(self, num_inference_steps, device=None):
        n = num_inference_steps
        ts = self._spaced(n)
        sig = self._train_sigmas()
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = n
        coef = torch.zeros(n, 16, dtype=torch.float32)
        for i in range(n):
            sigma_from, sigma_to = self.sigmas[i], self.sigmas[i + 1]
            sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
            sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
            self._euler_row(coef[i], sigma_from, sigma_down, up=sigma_up)
        assert torch.isfinite(coef).all(), "non-finite Euler-ancestral coefficient"
        self.coef = coef
        return self


class HeunTable(_SigmaTable):
    """HeunDiscreteScheduler as a coefficient table (scheduling_heun_discrete.py:225-305, 370-467).  `timesteps` / `sigmas` are the
    reference's interleaved ones: n inference steps are 2n - 1 network evaluations = rows.  A first-stage row is the Euler row to
    sigma_next (c2 = 0, so the step kernel leaves last = x, m0 = x0); the second-stage row, on the first stage's result, is
        x' = last + dt / 2 * ((last - m0) / sigma + eps),   dt = sigma_next - sigma,
    i.e. c2 = 1, c3 = 1 + dt / (2 sigma), c4 = -dt / (2 sigma), c7 = 1, c10 = dt / 2, with x0 and the input divisor at sigma_next.
    The last evaluation (sigma_next = 0) is a lone first stage, as in the reference."""
    order = 2
    _option_defaults = HEUN_OPTIONS

    def blend_rows(self):
        raise NotImplementedError("a masked edit (blend) with the Heun scheduler: the reference's second stage takes eps as (sample - x0) / "
                                  "sigma_next from its own state, independent of the blended sample, while this table expresses that stage "
                                  "through the current latents (`last`), which the blend changes - use Euler, Euler-ancestral, DDIM, "
                                  "DPM-Solver++, UniPC or LCM")

    def set_timesteps(self, num_inference_steps, device=None):
        n = num_inference_steps
        ts = self._spaced(n)
        sig = self._train_sigmas()
        log_sigmas = np.log(sig)
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        if self.options["use_karras_sigmas"]:
            sig, ts = self._karras(sig, log_sigmas, n)
        s = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        t = torch.from_numpy(ts)
        self.sigmas = torch.cat([s[:1], s[1:-1].repeat_interleave(2), s[-1:]])
        self.timesteps = torch.cat([t[:1], t[1:].repeat_interleave(2)])
        self.num_inference_steps = n
        coef = torch.zeros(2 * n - 1, 16, dtype=torch.float32)
        for k in range(n):
            sigma, sigma_next = s[k], s[k + 1]
            self._euler_row(coef[2 * k], sigma, sigma_next)
            if k == n - 1:
                break
            row = coef[2 * k + 1]
            dt = sigma_next - sigma
            w = dt / (2 * sigma)
            row[0] = 1.0
            row[1] = sigma_next
            row[2] = 1.0
            row[3] = 1 + w
            row[4] = -w
            row[7] = 1.0
            row[10] = dt / 2
            row[14] = (sigma_next ** 2 + 1) ** 0.5
        assert torch.isfinite(coef).all(), "non-finite Heun coefficient"
        self.coef = coef
        return self


# ---- LCMScheduler (latent-consistency models: LCM-LoRA or a distilled LCM UNet, 1-8 steps) ----------------------------------------------
# the options a table depends on (the engine keys its tables and plans on them), with the reference's defaults (scheduling_lcm.py:196-215)
LCM_OPTIONS = dict(original_inference_steps=50, timestep_scaling=10.0, set_alpha_to_one=True)


class LCMTable(_Base):
    """LCMScheduler as a coefficient table (scheduling_lcm.py:349-488 the skipping timestep schedule, 490-496 the boundary-condition
    scalings, 498-592 the step).  Every step but the last adds sqrt(1 - abar_prev) times the step's noise (column 12), so the steps end in
    bc_cfg_scheduler_step_noise; the last step's row has c12 = 0 and its noise slice is never drawn (`draws`).  On the last step the
    reference takes prev_timestep = timestep, so `final_alpha_cumprod` (set_alpha_to_one) is never read: the option is kept for the key
    only.  Caller `timesteps` and `strength` are taken as the reference takes them."""
    sde = True                                                            # a noise term in the steps (the engine's stochastic plan)

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, **options):
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end)
        unknown = set(options) - set(LCM_OPTIONS)
        if unknown:
            raise TypeError(f"unknown LCMTable option(s) {sorted(unknown)}")
        self.options = dict(LCM_OPTIONS, **options)
        self.num_inference_steps = None
        self.draws = None

    def set_timesteps(self, num_inference_steps=None, device=None, original_inference_steps=None, timesteps=None, strength=1.0):
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `custom_timesteps`.")
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `custom_timesteps`.")
        original_steps = original_inference_steps if original_inference_steps is not None else self.options["original_inference_steps"]
        if original_steps > self.num_train:
            raise ValueError(f"`original_steps`: {original_steps} cannot be larger than `self.config.train_timesteps`: {self.num_train} as "
                             f"the unet model trained with this scheduler can only handle maximal {self.num_train} timesteps.")
        k = self.num_train // original_steps                              # the skipping step of the distillation schedule
        origin = np.asarray(list(range(1, int(original_steps * strength) + 1))) * k - 1
        if timesteps is not None:
            timesteps = [int(t) for t in timesteps]
            for i in range(1, len(timesteps)):
                if timesteps[i] >= timesteps[i - 1]:
                    raise ValueError("`custom_timesteps` must be in descending order.")
            if timesteps[0] >= self.num_train:
                raise ValueError(f"`timesteps` must start before `self.config.train_timesteps`: {self.num_train}.")
            ts = np.array(timesteps, dtype=np.int64)
            self.num_inference_steps = len(ts)
            init_timestep = min(int(self.num_inference_steps * strength), self.num_inference_steps)
            # the reference leaves num_inference_steps at the FULL length here (its TODO at :452), so with strength < 1 no step index
            # ever reaches num_inference_steps - 1: the last row then draws noise too and, with prev_t = t, re-noises to its own level
            ts = ts[max(self.num_inference_steps - init_timestep, 0):]
        else:
            n = num_inference_steps
            if n > self.num_train:
                raise ValueError(f"`num_inference_steps`: {n} cannot be larger than `self.config.train_timesteps`: {self.num_train} as "
                                 f"the unet model trained with this scheduler can only handle maximal {self.num_train} timesteps.")
            skipping_step = len(origin) // n
            if skipping_step < 1:
                raise ValueError(f"The combination of `original_steps x strength`: {original_steps} x {strength} is smaller than "
                                 f"`num_inference_steps`: {n}. Make sure to either reduce `num_inference_steps` to a value smaller than "
                                 f"{int(original_steps * strength)} or increase `strength` to a value higher than "
                                 f"{float(n / original_steps)}.")
            self.num_inference_steps = n
            if n > original_steps:
                raise ValueError(f"`num_inference_steps`: {n} cannot be larger than `original_inference_steps`: {original_steps} because "
                                 "the final timestep schedule will be a subset of the `original_inference_steps`-sized initial timestep "
                                 "schedule.")
            origin = origin[::-1].copy()
            idx = np.floor(np.linspace(0, len(origin), num=n, endpoint=False)).astype(np.int64)
            ts = origin[idx]
        self.timesteps = torch.from_numpy(ts).to(dtype=torch.int64)
        self.coef = self._build()
        return self

    def _build(self):
        ts, ac = self.timesteps, self.alphas_cumprod
        N = len(ts)
        coef = torch.zeros(N, 16, dtype=torch.float32)
        self.c_skip, self.c_out, self.draws = [], [], []
        for i in range(N):
            t = ts[i]
            prev_t = ts[i + 1] if i + 1 < N else t                         # :535-539
            a_t, a_prev = ac[t], ac[prev_t]
            scaled_t = t * self.options["timestep_scaling"]                # :490-496, sigma_data = 0.5
            c_skip = 0.5 ** 2 / (scaled_t ** 2 + 0.5 ** 2)
            c_out = scaled_t / (scaled_t ** 2 + 0.5 ** 2) ** 0.5
            coef[i, 0] = 1.0 / a_t.sqrt()
            coef[i, 1] = (1 - a_t).sqrt() / a_t.sqrt()
            noisy = i != self.num_inference_steps - 1                      # :578
            coef[i, 7] = a_prev.sqrt() * c_skip if noisy else c_skip
            coef[i, 8] = a_prev.sqrt() * c_out if noisy else c_out
            coef[i, 12] = (1 - a_prev).sqrt() if noisy else 0.0
            self.c_skip.append(float(c_skip))
            self.c_out.append(float(c_out))
            self.draws.append(bool(noisy))
        assert torch.isfinite(coef).all(), "non-finite LCM coefficient"
        return coef


# scheduler kinds whose table takes options as a fourth `table_params()` entry
OPTION_KINDS = ("dpmsolver", "euler", "euler_ancestral", "heun", "lcm")


def table_class(kind):
    """Scheduler kind -> its coefficient table class, for the drop-in schedulers and the engine alike ("unipc", "dpmsolver", "euler",
    "euler_ancestral", "heun", "lcm"; every other kind tabulates DDIM)."""
    return {"unipc": UniPCTable, "dpmsolver": DPMSolverMultistepTable, "euler": EulerDiscreteTable,
            "euler_ancestral": EulerAncestralTable, "heun": HeunTable, "lcm": LCMTable}.get(kind, DDIMTable)


def apply_table_step(coef_row, eps, x, hist, noise=None):
    """Host (torch) evaluation of one table row - the same arithmetic `bc_cfg_scheduler_step` (with `noise`,
    `bc_cfg_scheduler_step_noise`; with a third-order row, `bc_cfg_scheduler_step3`) performs after CFG.  Used by the drop-in scheduler
    objects; `hist` = dict(m0, m1, last)."""
    c = coef_row
    x0 = x * c[0] - eps * c[1]
    xc = x
    if c[2] != 0:
        xc = c[3] * hist["last"] + c[4] * hist["m0"] + c[5] * hist["m1"] + c[6] * x0
    xn = c[7] * xc + c[8] * x0 + c[9] * hist["m0"] + c[10] * eps
    if c[13] != 0:
        xn = xn + c[13] * hist["m1"]
    if noise is not None:
        xn = xn + c[12] * noise
    hist["m1"], hist["m0"], hist["last"] = hist["m0"], x0, xc
    return xn


def stack_request_tables(tables, guidance):
    """Tables that have had their `set_timesteps` (one per request) -> (coef [B][nmax][16], t_rows [nmax][B] fp32, evals [B]): request
    b's rows as they are, left-aligned, with its guidance scale in column 11; behind them FINISHED rows up to the longest request -
    column 15 = 1 (the step leaves the image alone), column 14 = 1 (its input is not divided), every other column 0, the request's last
    timestep repeated.  Nothing of a scheduler is restated: the rows are the tables' own."""
    if len(tables) != len(guidance):
        raise ValueError(f"{len(tables)} tables for {len(guidance)} guidance scales")
    evals = [int(t.table().shape[0]) for t in tables]
    nmax = max(evals)
    coef = torch.zeros(len(tables), nmax, 16, dtype=torch.float32)
    t_rows = torch.zeros(nmax, len(tables), dtype=torch.float32)
    for b, (t, n) in enumerate(zip(tables, evals)):
        coef[b, :n] = t.table()
        coef[b, :, 11] = float(guidance[b])
        coef[b, n:, 14] = 1.0
        coef[b, n:, 15] = 1.0
        ts = t.timesteps.to(torch.float32)
        t_rows[:n, b] = ts
        t_rows[n:, b] = ts[-1]
    return coef, t_rows, evals


def request_tables(table_factory, steps_or_timesteps, guidance, eta=None):
    """The per-request tables of a request batch: `table_factory()` makes a fresh table object, request b gets its own
    `set_timesteps(n_b)` (an int), `set_timesteps(timesteps=ts_b)` (a list) or, with `eta` (one per request, DDIM), `set_timesteps(n_b,
    eta=eta_b)`; the results are stacked by `stack_request_tables`."""
    if eta is not None and len(eta) != len(steps_or_timesteps):
        raise ValueError(f"{len(eta)} eta values for {len(steps_or_timesteps)} requests")
    tables = []
    for b, st in enumerate(steps_or_timesteps):
        t = table_factory()
        if isinstance(st, (list, tuple)):
            t.set_timesteps(timesteps=list(st))
        elif eta is not None:
            t.set_timesteps(int(st), eta=float(eta[b]))
        else:
            t.set_timesteps(int(st))
        tables.append(t)
    return stack_request_tables(tables, guidance)


def randn_tensor(shape, generator=None, device=None, dtype=torch.float32):
    """D/utils/torch_utils.py:38-83: a CPU generator draws on the CPU (then the tensor moves to `device`), a list of generators draws
    one [1, ...] slice per sample (a one-element list counts as its generator), None uses the global RNG of `device`."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    rand_device = device
    if generator is not None:
        gtype = generator[0].device.type if isinstance(generator, list) else generator.device.type
        if gtype != device.type and gtype == "cpu":
            rand_device = torch.device("cpu")
        elif gtype != device.type:
            raise ValueError(f"Cannot generate a {device} tensor from a generator of type {gtype}.")
    if isinstance(generator, list) and len(generator) == 1:
        generator = generator[0]
    if isinstance(generator, list):
        if len(generator) != shape[0]:
            raise ValueError(f"a list of {len(generator)} generators for a batch of {shape[0]}")
        one = (1,) + tuple(shape[1:])
        return torch.cat([torch.randn(one, generator=g_, device=rand_device, dtype=dtype) for g_ in generator], 0).to(device)
    return torch.randn(tuple(shape), generator=generator, device=rand_device, dtype=dtype).to(device)


def draw_variance_noise(num_steps, shape, generator=None, device=None, draws=None):
    """The `variance_noise` of every step of a stochastic DDIM edit, [num_steps, *shape] fp32 on `device`: one `randn_tensor(shape,
    generator, device)` per step, in step order - the draws `DDIMScheduler.step` makes (scheduling_ddim.py:455-458).
    `draws` (one bool per step, an LCM table's): a step that draws nothing (LCMScheduler's last, scheduling_lcm.py:578) gets a zero
    slice and leaves the generator where it is."""
    if draws is None:
        return torch.stack([randn_tensor(shape, generator, device) for _ in range(num_steps)], 0)
    assert len(draws) == num_steps
    return torch.stack([randn_tensor(shape, generator, device) if d else torch.zeros(tuple(shape), dtype=torch.float32, device=device)
                        for d in draws], 0)


class TableScheduler:
    """Drop-in for `pipeline.scheduler`: set_timesteps / timesteps / init_noise_sigma /
    scale_model_input / step(noise_pred, t, latents, return_dict=False)[0] / order."""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, kind="unipc", **kw):
        self.table_impl = table_class(kind)(**kw)
        self.kind = kind

    def _set_timesteps(self, device, *table_args, **table_kw):
        """(Re)tabulate with the table's own `set_timesteps` arguments and rewind: step 0, no history."""
        self.table_impl.set_timesteps(*table_args, **table_kw)
        self.timesteps = self.table_impl.timesteps.to(device) if device is not None else self.table_impl.timesteps
        self._i = 0
        self._hist = None

    def set_timesteps(self, num_inference_steps, device=None):
        self._set_timesteps(device, num_inference_steps)

    def scale_model_input(self, sample, timestep=None):
        """pipe:1032.  Identity for UniPC, DDIM and DPM-Solver++; a sigma-space table divides by column 14 of the current row,
        sqrt(sigma^2 + 1), as its reference does (scheduling_euler_discrete.py:277-299)."""
        if not self.table_impl.scales_input:
            return sample
        return sample / self.table_impl.coef[self._i, 14].to(sample.device)

    def _apply_row(self, model_output, sample, noise=None):
        """Table row `_i` applied to (model_output, sample): creates the history on the first step, then moves on to the next row."""
        if self._hist is None:
            z = torch.zeros_like(sample)
            self._hist = dict(m0=z, m1=z.clone(), last=z.clone())
        out = apply_table_step(self.table_impl.coef[self._i].tolist(), model_output, sample, self._hist, noise)
        self._i += 1
        return out

    def step(self, model_output, timestep, sample, return_dict=False, **kw):
        return (self._apply_row(model_output, sample),)


class SchedulerConfig(dict):
    """`scheduler.config` with attribute and mapping access (the scripts do `X.from_config(pipeline.scheduler.config)`, inf:276-277)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


_SD15 = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
             prediction_type="epsilon")


class _ConfiguredScheduler(TableScheduler):
    _kind = None
    _defaults = {}

    def __init__(self, **kw):
        cfg = self._make_config(kw)
        if cfg["beta_schedule"] != "scaled_linear" or cfg["prediction_type"] != "epsilon":
            raise NotImplementedError("only the SD-1.5 configuration (scaled_linear betas, epsilon prediction) is tabulated")
        self._check(cfg)
        super().__init__(self._kind, num_train_timesteps=cfg["num_train_timesteps"], beta_start=cfg["beta_start"],
                         beta_end=cfg["beta_end"])
        self.config = cfg
        self.timesteps = None

    @classmethod
    def _make_config(cls, kw):
        """`.config` of an object built with the keyword arguments `kw`: SD-1.5 values, this class's defaults, then what the caller gave."""
        cfg = dict(_SD15)
        cfg.update(cls._defaults)
        cfg.update({k: v for k, v in kw.items() if v is not None})
        # like diffusers' `_use_default_values`: keys the caller did not give are NOT inherited by another class's from_config
        return SchedulerConfig(cfg, _use_default_values=sorted(k for k in cfg if k not in kw or kw[k] is None))

    @classmethod
    def _known(cls, src):
        """The entries of `src` that are constructor arguments of this class."""
        known = set(_SD15) | set(cls._defaults)
        return {k: v for k, v in src.items() if k in known}

    def _check(self, cfg):
        pass

    @classmethod
    def from_config(cls, config, **kw):
        """Like diffusers' ConfigMixin.from_config: keys this class knows are taken from `config` (another scheduler's config is
        fine - unknown keys such as PNDM's `skip_prk_steps` are dropped), everything else keeps this class's defaults."""
        defaulted = set(dict(config).get("_use_default_values", ()))
        src = {k: v for k, v in dict(config).items() if k not in defaulted}
        src.update(kw)
        return cls(**cls._known(src))

    def table_params(self):
        """(num_train_timesteps, beta_start, beta_end): what the engine builds its coefficient table from."""
        return (int(self.config["num_train_timesteps"]), float(self.config["beta_start"]), float(self.config["beta_end"]))

    @property
    def kind(self):
        return self._kind

    @kind.setter
    def kind(self, v):
        pass


class PNDMScheduler(_ConfiguredScheduler):
    """What SD-1.5's `scheduler/scheduler_config.json` names.  The reference scripts only read its `.config` and build UniPC (or
    DDIM) from it (inf:276-277), so this class carries the configuration and refuses to step."""
    _kind = None
    _defaults = dict(skip_prk_steps=True, set_alpha_to_one=False, timestep_spacing="leading", clip_sample=False)

    def __init__(self, **kw):
        self.config = self._make_config(kw)
        self.timesteps = None
        self.table_impl = None

    def set_timesteps(self, *a, **k):
        raise NotImplementedError("PNDM is not tabulated: replace it as the scripts do, "
                                  "pipeline.scheduler = UniPCMultistepScheduler.from_config(pipeline.scheduler.config)")

    step = set_timesteps


def scheduler_from_config_dir(path):
    """`<model>/scheduler/scheduler_config.json` -> the scheduler object its `_class_name` names (PNDM / UniPC / DDIM / DPM-Solver /
    Euler / Euler-ancestral / Heun / LCM)."""
    import json
    import os
    with open(os.path.join(path, "scheduler_config.json")) as f:
        cfg = json.load(f)
    name = cfg.get("_class_name", "PNDMScheduler")
    classes = {"PNDMScheduler": PNDMScheduler, "UniPCMultistepScheduler": UniPCMultistepScheduler, "DDIMScheduler": DDIMScheduler,
               "DPMSolverMultistepScheduler": DPMSolverMultistepScheduler, "EulerDiscreteScheduler": EulerDiscreteScheduler,
               "EulerAncestralDiscreteScheduler": EulerAncestralDiscreteScheduler, "HeunDiscreteScheduler": HeunDiscreteScheduler,
               "LCMScheduler": LCMScheduler}
    if name not in classes:
        raise NotImplementedError(f"scheduler class {name} is not available (PNDM config holder, UniPC, DDIM, DPM-Solver, Euler, "
                                  "Euler-ancestral and Heun are, and LCM)")
    return classes[name](**classes[name]._known(cfg))


class UniPCMultistepScheduler(_ConfiguredScheduler):
    """Drop-in for diffusers' UniPCMultistepScheduler as the scripts configure it (`from_config(PNDM config)`)."""
    _kind = "unipc"
    _defaults = dict(solver_order=2, solver_type="bh2", predict_x0=True, lower_order_final=True, timestep_spacing="linspace",
                     final_sigmas_type="zero", thresholding=False)

    def _check(self, cfg):
        if (cfg["solver_order"], cfg["solver_type"], cfg["predict_x0"], cfg["lower_order_final"], cfg["timestep_spacing"],
                cfg["final_sigmas_type"], cfg["thresholding"]) != (2, "bh2", True, True, "linspace", "zero", False):
            raise NotImplementedError("UniPC is tabulated for solver_order=2 / bh2 / predict_x0 / lower_order_final / linspace / "
                                      "final sigma zero (what the reference scripts run)")


class DDIMScheduler(_ConfiguredScheduler):
    """Drop-in for diffusers' DDIMScheduler with the SD-1.5 scheduler_config.json values; `step(..., eta=, generator=,
    variance_noise=)` as in scheduling_ddim.py:342-468 (eta > 0: stochastic DDIM, noise drawn with the reference's randn_tensor)."""
    _kind = "ddim"
    _defaults = dict(clip_sample=False, set_alpha_to_one=False, timestep_spacing="leading", thresholding=False)

    def _check(self, cfg):
        if cfg["clip_sample"] or cfg["set_alpha_to_one"] or cfg["timestep_spacing"] != "leading" or cfg["steps_offset"] != 1 or \
                cfg["thresholding"]:
            raise NotImplementedError("DDIM is tabulated for clip_sample=False, set_alpha_to_one=False, leading spacing, steps_offset=1")

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None, variance_noise=None,
             return_dict=True):
        """One DDIM update.  (use_clipped_model_output changes nothing without clipping or thresholding, which this configuration
        has neither of.)  Returns `(prev_sample,)`, or an object with `.prev_sample` for return_dict=True."""
        if eta < 0:
            raise NotImplementedError("eta < 0 is not a DDIM variance")
        tab = self.table_impl
        if float(eta) != getattr(tab, "eta", 0.0):                     # (re)tabulate for this eta; raises for a non-finite row
            tab.set_timesteps(tab.num_inference_steps, eta=float(eta))
        noise = None
        if eta > 0:
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                                 " `variance_noise` stays `None`.")
            noise = variance_noise if variance_noise is not None else \
                randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        out = self._apply_row(model_output, sample, noise)
        return _StepOutput(out) if return_dict else (out,)


class _StepOutput(tuple):
    """`DDIMSchedulerOutput`-like: `.prev_sample`, and indexable like the tuple form."""

    def __new__(cls, prev_sample):
        return super().__new__(cls, (prev_sample,))

    @property
    def prev_sample(self):
        return self[0]


def _from_config_with_hidden(cls, config, kw):
    src = dict(config)
    defaulted = set(src.pop("_use_default_values", ()))
    src = {k: v for k, v in src.items() if k not in defaulted}
    init = cls._known(src)
    init.update(kw)
    s = cls(**init)
    hidden = {k: v for k, v in src.items() if k not in init}
    if "_class_name" in hidden:
        hidden["_class_name"] = cls.__name__
    s.config.update(hidden)
    return s


class DPMSolverMultistepScheduler(_ConfiguredScheduler):
    """Drop-in for diffusers' DPMSolverMultistepScheduler (scheduling_dpmsolver_multistep.py), e.g. "DPM++ 2M Karras" as
    `DPMSolverMultistepScheduler.from_config(pipeline.scheduler.config, use_karras_sigmas=True)`.  Tabulated for data prediction
    ("dpmsolver++", "sde-dpmsolver++") at orders 1-3 (3 without the SDE), midpoint / heun, karras / lu / plain sigmas, the three spacings,
    both final-sigma types and caller `timesteps`; `step(..., generator=, variance_noise=)` draws the SDE noise as :979-986 does."""
    _kind = "dpmsolver"
    _defaults = dict(trained_betas=None, thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0, variance_type=None,
                     rescale_betas_zero_snr=False, **DPM_OPTIONS)

    def __init__(self, **kw):
        if kw.get("algorithm_type") == "deis":                        # the reference re-registers these two (:255-265)
            kw["algorithm_type"] = "dpmsolver++"
        if kw.get("solver_type") in ("logrho", "bh1", "bh2"):
            kw["solver_type"] = "midpoint"
        super().__init__(**kw)
        # diffusers' `_use_default_values`: the __init__ keys the caller did not pass (an explicit None counts as passed)
        self.config["_use_default_values"] = sorted(k for k in self.config if not k.startswith("_") and k not in kw)
        self.table_impl = DPMSolverMultistepTable(num_train_timesteps=self.config["num_train_timesteps"],
                                                  beta_start=self.config["beta_start"], beta_end=self.config["beta_end"],
                                                  **{k: self.config[k] for k in DPM_OPTIONS})

    def _check(self, cfg):
        if cfg["algorithm_type"] in ("dpmsolver", "sde-dpmsolver"):
            raise NotImplementedError(f"algorithm_type {cfg['algorithm_type']!r} (the deprecated noise-prediction form) is not "
                                      "tabulated: use 'dpmsolver++' or 'sde-dpmsolver++'")
        if cfg["algorithm_type"] not in ("dpmsolver++", "sde-dpmsolver++"):
            raise NotImplementedError(f"algorithm_type {cfg['algorithm_type']!r} is not implemented")
        if cfg["thresholding"]:
            raise NotImplementedError("thresholding=True (dynamic thresholding of x0) is not tabulated")
        if cfg["variance_type"] in ("learned", "learned_range"):
            raise NotImplementedError(f"variance_type {cfg['variance_type']!r} (a learned variance) is not supported: the UNet predicts "
                                      "4 channels")
        if cfg["solver_order"] == 3 and cfg["algorithm_type"] == "sde-dpmsolver++":
            raise NotImplementedError("solver_order=3 with algorithm_type 'sde-dpmsolver++': the reference's third-order update has no "
                                      "SDE branch")
        if cfg["solver_order"] not in (1, 2, 3) or cfg["solver_type"] not in ("midpoint", "heun"):
            raise NotImplementedError(f"solver_order {cfg['solver_order']} / solver_type {cfg['solver_type']!r} is not tabulated")
        if cfg["trained_betas"] is not None or cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("trained_betas / rescale_betas_zero_snr are not tabulated")

    @classmethod
    def from_config(cls, config, **kw):
        """diffusers' ConfigMixin.from_config (configuration_utils.py:188-270, 456-549): keys the source left at their defaults are
        dropped, this class's keys are taken, every other key is kept in `.config` as a hidden entry (`_class_name` renamed)."""
        return _from_config_with_hidden(cls, config, kw)

    def table_params(self):
        """(num_train_timesteps, beta_start, beta_end, DPM options as sorted (key, value) pairs): what the engine tabulates."""
        return super().table_params() + (tuple(sorted((k, self.config[k]) for k in DPM_OPTIONS)),)

    @property
    def sigmas(self):
        return self.table_impl.sigmas

    @property
    def num_inference_steps(self):
        return self.table_impl.num_inference_steps

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None):
        self._set_timesteps(device, num_inference_steps, timesteps=timesteps)

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict=True):
        """One DPM-Solver++ update (:920-1007).  The SDE variant draws `randn_tensor(shape, generator, device, float32)` per step unless
        `variance_noise` is given.  Returns `(prev_sample,)` for return_dict=False, else an object with `.prev_sample`."""
        tab = self.table_impl
        if tab.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        noise = None
        if tab.sde:
            noise = variance_noise.to(device=model_output.device, dtype=torch.float32) if variance_noise is not None else \
                randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=torch.float32)
        out = self._apply_row(model_output, sample.to(torch.float32), noise).to(model_output.dtype)
        return _StepOutput(out) if return_dict else (out,)


class _OptionScheduler(_ConfiguredScheduler):
    """What the drop-ins whose table takes options share: the reference's `__init__` keys in `.config`, `from_config` with hidden
    entries, the table built from `_options`, and the step on the current row."""
    _options = {}

    def __init__(self, **kw):
        cfg = self._make_config(kw)
        name = type(self).__name__
        if cfg["beta_schedule"] != "scaled_linear":
            raise NotImplementedError(f"{name}: beta_schedule {cfg['beta_schedule']!r} is not tabulated ('scaled_linear' is)")
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"{name}: prediction_type {cfg['prediction_type']!r} is not tabulated ('epsilon' is)")
        if cfg["trained_betas"] is not None:
            raise NotImplementedError(f"{name}: trained_betas are not tabulated")
        self._check(cfg)
        # diffusers' `_use_default_values`: the __init__ keys the caller did not pass (an explicit None counts as passed)
        cfg["_use_default_values"] = sorted(k for k in cfg if not k.startswith("_") and k not in kw)
        self.config = cfg
        self.timesteps = None
        self.table_impl = table_class(self._kind)(num_train_timesteps=cfg["num_train_timesteps"], beta_start=cfg["beta_start"],
                                                  beta_end=cfg["beta_end"], **{k: cfg[k] for k in self._options})

    @classmethod
    def from_config(cls, config, **kw):
        """diffusers' ConfigMixin.from_config, as DPMSolverMultistepScheduler.from_config above (a PNDM, UniPC or DPM config is fine)."""
        return _from_config_with_hidden(cls, config, kw)

    def table_params(self):
        """(num_train_timesteps, beta_start, beta_end, table options as sorted (key, value) pairs): what the engine tabulates."""
        return super().table_params() + (tuple(sorted((k, self.config[k]) for k in self._options)),)

    @property
    def order(self):
        return self.table_impl.order

    @property
    def num_inference_steps(self):
        return self.table_impl.num_inference_steps

    def set_timesteps(self, num_inference_steps, device=None):
        self._set_timesteps(device, num_inference_steps)

    def _step(self, model_output, sample, noise, return_dict):
        if self.table_impl.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        out = self._apply_row(model_output, sample.to(torch.float32), noise).to(model_output.dtype)
        return _StepOutput(out) if return_dict else (out,)


class _SigmaScheduler(_OptionScheduler):
    """The drop-ins for the sigma-space schedulers: `sigmas` / `init_noise_sigma` of the table, and `scale_model_input` dividing by
    sqrt(sigma^2 + 1) of the current step (TableScheduler)."""

    @property
    def sigmas(self):
        return self.table_impl.sigmas

    @property
    def init_noise_sigma(self):
        return self.table_impl.init_noise_sigma


class EulerDiscreteScheduler(_SigmaScheduler):
    """Drop-in for diffusers' EulerDiscreteScheduler ("Euler"; `EulerDiscreteScheduler.from_config(pipeline.scheduler.config)`).  Tabulated
    for epsilon prediction with linear sigma interpolation, discrete timesteps, the three spacings (`linspace` gives fractional timesteps),
    Karras sigmas, both final-sigma types and caller `timesteps`; s_churn (and with it s_tmin / s_tmax / s_noise) is not."""
    _kind = "euler"
    _options = EULER_OPTIONS
    _defaults = dict(trained_betas=None, sigma_min=None, sigma_max=None, rescale_betas_zero_snr=False, **EULER_OPTIONS)

    def _check(self, cfg):
        if cfg["interpolation_type"] == "log_linear":
            raise NotImplementedError("interpolation_type 'log_linear' is not tabulated ('linear' is)")
        if cfg["timestep_type"] != "discrete":
            raise NotImplementedError(f"timestep_type {cfg['timestep_type']!r} is not tabulated ('discrete' is)")
        if cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("rescale_betas_zero_snr=True is not tabulated")
        if cfg["sigma_min"] is not None or cfg["sigma_max"] is not None:
            raise NotImplementedError("sigma_min / sigma_max (the Karras range) are not tabulated: the range of the schedule is used")

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None):
        self._set_timesteps(device, num_inference_steps, timesteps=timesteps, sigmas=sigmas)

    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, generator=None,
             return_dict=True):
        """One Euler update (:493-599) with gamma = 0.  Returns `(prev_sample,)`, or an object with `.prev_sample` for return_dict=True."""
        if s_churn != 0:
            raise NotImplementedError("s_churn != 0 (stochastic churn) is not tabulated")
        if generator is not None:                                         # the reference draws (and discards) one noise tensor per step (:558)
            randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        return self._step(model_output, sample, None, return_dict)


class EulerAncestralDiscreteScheduler(_SigmaScheduler):
    """Drop-in for diffusers' EulerAncestralDiscreteScheduler ("Euler a"): `step(..., generator=)` draws the step's noise as :427 does;
    `variance_noise=` gives it instead, as this package's DDIM and SDE-DPM-Solver++ steps take it."""
    _kind = "euler_ancestral"
    _options = EULER_ANCESTRAL_OPTIONS
    _defaults = dict(trained_betas=None, rescale_betas_zero_snr=False, **EULER_ANCESTRAL_OPTIONS)

    def _check(self, cfg):
        if cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("rescale_betas_zero_snr=True is not tabulated")

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, variance_noise=None):
        if variance_noise is not None and generator is not None:
            raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                             " `variance_noise` stays `None`.")
        noise = variance_noise.to(device=model_output.device, dtype=torch.float32) if variance_noise is not None else \
            randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        return self._step(model_output, sample, noise, return_dict)


class HeunDiscreteScheduler(_SigmaScheduler):
    """Drop-in for diffusers' HeunDiscreteScheduler ("Heun"): n inference steps are 2n - 1 entries of `timesteps` (order = 2), the
    pipeline's loop runs over all of them.  Tabulated for the three spacings and Karras sigmas."""
    _kind = "heun"
    _options = HEUN_OPTIONS
    _defaults = dict(trained_betas=None, clip_sample=False, clip_sample_range=1.0, **HEUN_OPTIONS)

    def _check(self, cfg):
        if cfg["clip_sample"]:
            raise NotImplementedError("clip_sample=True (clipping of x0) is not tabulated")

    def set_timesteps(self, num_inference_steps=None, device=None, num_train_timesteps=None, timesteps=None):
        if timesteps is not None:
            raise NotImplementedError("custom `timesteps` are not tabulated for Heun: pass num_inference_steps")
        if num_train_timesteps is not None and num_train_timesteps != self.config["num_train_timesteps"]:
            raise NotImplementedError("num_train_timesteps other than the configuration's is not tabulated")
        if num_inference_steps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `custom_timesteps`.")
        self._set_timesteps(device, num_inference_steps)

    def step(self, model_output, timestep, sample, return_dict=True):
        return self._step(model_output, sample, None, return_dict)


class LCMScheduler(_OptionScheduler):
    """Drop-in for diffusers' LCMScheduler (latent-consistency sampling in 1-8 steps, `LCMScheduler.from_config(pipeline.scheduler.config)`
    with LCM-LoRA merged or a distilled LCM UNet).  Tabulated for epsilon prediction on scaled_linear betas: `original_inference_steps`
    (config or `set_timesteps` argument), `timestep_scaling`, caller `timesteps` and `strength`; thresholding and clipping of x0 are not.
    `step(..., generator=)` draws the noise of every step but the last as :578-582 does and returns `(prev_sample, denoised)`;
    `variance_noise=` gives the noise instead, as this package's other stochastic steps take it."""
    _kind = "lcm"
    _options = LCM_OPTIONS
    _defaults = dict(trained_betas=None, clip_sample=False, clip_sample_range=1.0, steps_offset=0, thresholding=False,
                     dynamic_thresholding_ratio=0.995, sample_max_value=1.0, timestep_spacing="leading", rescale_betas_zero_snr=False,
                     **LCM_OPTIONS)

    def _check(self, cfg):
        if cfg["thresholding"]:
            raise NotImplementedError("thresholding=True (dynamic thresholding of x0) is not tabulated")
        if cfg["clip_sample"]:
            raise NotImplementedError("clip_sample=True (clipping of x0) is not tabulated")
        if cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("rescale_betas_zero_snr=True is not tabulated")

    def set_timesteps(self, num_inference_steps=None, device=None, original_inference_steps=None, timesteps=None, strength=1.0):
        self._set_timesteps(device, num_inference_steps, original_inference_steps=original_inference_steps, timesteps=timesteps,
                            strength=strength)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, variance_noise=None):
        tab = self.table_impl
        if tab.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if variance_noise is not None and generator is not None:
            raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                             " `variance_noise` stays `None`.")
        i = self._i
        noise = None
        if tab.draws[i]:
            noise = variance_noise.to(device=model_output.device, dtype=torch.float32) if variance_noise is not None else \
                randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        x = sample.to(torch.float32)
        denoised = tab.c_out[i] * (x * float(tab.coef[i, 0]) - model_output * float(tab.coef[i, 1])) + tab.c_skip[i] * x
        prev = self._apply_row(model_output, x, noise).to(model_output.dtype)
        denoised = denoised.to(model_output.dtype)
        return _LCMStepOutput(prev, denoised) if return_dict else (prev, denoised)


class _LCMStepOutput(tuple):
    """`LCMSchedulerOutput`-like: `.prev_sample`, `.denoised`, and indexable like the tuple form."""

    def __new__(cls, prev_sample, denoised):
        return super().__new__(cls, (prev_sample, denoised))

    @property
    def prev_sample(self):
        return self[0]

    @property
    def denoised(self):
        return self[1]
