"""``GaussianDiffusion`` on HIP kernels — the surface of reference diffusion/gaussian_diffusion.py that the
training and sampling scripts use: ``num_timesteps``, the float64 numpy schedule tables, ``q_sample``,
``training_losses``, ``p_mean_variance``, ``p_sample``, ``p_sample_loop`` (+ ``_progressive``), DDIM, and the likelihood
evaluation (``calc_bpd_loop``, ``_vb_terms_bpd``, ``_prior_bpd``) with its helpers.

What differs by design: the schedule tables are uploaded to the GPU once (the reference uploads a numpy table on
every ``_extract_into_tensor`` call, :861-873), the loss / posterior / sampling pointwise math is one fused kernel
each (``mapdit_loss_fwd`` / ``mapdit_psample_step``), and there is no host synchronisation inside a step.

Built: every objective ``create_diffusion`` can produce — mean type EPSILON / START_X, variance type LEARNED_RANGE /
FIXED_SMALL / FIXED_LARGE, loss MSE / RESCALED_MSE / KL / RESCALED_KL.  The default (EPSILON, LEARNED_RANGE, MSE) runs the
kernels it always ran (``mapdit_loss_fwd`` / ``mapdit_psample_step`` / ``mapdit_ddim_step``); the others run the
generalised ``mapdit_obj_*`` kernels.  ``ModelMeanType.PREVIOUS_X`` and ``ModelVarType.LEARNED`` (never produced by
``create_diffusion``) exist for API parity and raise NotImplementedError when exercised; for PREVIOUS_X there is nothing to match
(the reference's ``p_mean_variance`` has no branch for it and would read the x_{t-1} prediction as eps).

The sampler hooks: every reverse-process method takes ``denoised_fn`` (applied to the raw x0 prediction, before
``clip_denoised``) and, but for ``p_mean_variance``, ``cond_fn(x, t, **model_kwargs)`` (the gradient of a conditional log
probability; under ``SpacedDiffusion`` it sees the timesteps of the base schedule, as the model does).  A hooked step runs
``mapdit_obj_step_guided`` - ``condition_mean`` folded into ``p_sample``, ``condition_score`` into the DDIM steps - after
``mapdit_obj_xstart`` when ``denoised_fn`` has to see the raw prediction: at most two diffusion kernels between the model's output
and the sample, and no torch pointwise op or host synchronisation besides the user's callables.  Without hooks every method runs
the kernel it ran before.  ``condition_mean`` / ``condition_score`` are public, with the reference's semantics.

Not in the reference: ``dpm_solver_sample_loop`` (+ ``_progressive``), the multistep DPM-Solver++ of Lu et al. 2022 (orders 1 and 2) - the
schedule and its coefficients are built here in fp64 (``_dpm_schedule``), a step is one ``mapdit_dpm_step`` launch after the model.
"""
import enum
import math

import numpy as np
import torch

from .. import _lib as L


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()

    def is_vb(self):
        return self in (LossType.KL, LossType.RESCALED_KL)


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    """reference gaussian_diffusion.py:98-122."""
    if schedule_name == "linear":
        scale = 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "squaredcos_cap_v2":
        bar = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
        n = num_diffusion_timesteps
        return np.array([min(1 - bar((i + 1) / n) / bar(i / n), 0.999) for i in range(n)])
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def mean_flat(tensor):
    return tensor.mean(dim=list(range(1, len(tensor.shape))))


class _LossFunction(torch.autograd.Function):
    """mse / vb / loss per sample with the gradient wrt the model output (mapdit_loss_fwd / mapdit_loss_bwd)."""

    @staticmethod
    def forward(ctx, model_output, x_start, x_t, noise, t, tab, nsteps):
        n = model_output.shape[0]
        per = x_start[0].numel()
        mo = model_output.contiguous().float()
        mse, vb, loss = (torch.empty(n, device=mo.device) for _ in range(3))
        G = torch.empty_like(mo)
        with torch.cuda.device(mo.device):
            L.lib().loss_fwd(mo.data_ptr(), x_start.data_ptr(), x_t.data_ptr(), noise.data_ptr(), t.data_ptr(), tab.data_ptr(),
                             nsteps, mse.data_ptr(), vb.data_ptr(), loss.data_ptr(), G.data_ptr(), n, per, L.cur_stream())
        ctx.save_for_backward(G)
        ctx.per = per
        return loss, mse, vb

    @staticmethod
    def backward(ctx, g_loss, g_mse, g_vb):
        (G,) = ctx.saved_tensors
        dout = torch.empty_like(G)
        gl, gm, gv = (None if g is None else g.contiguous().float() for g in (g_loss, g_mse, g_vb))
        with torch.cuda.device(G.device):
            L.lib().loss_bwd(G.data_ptr(), L.ptr(gl), L.ptr(gm), L.ptr(gv), dout.data_ptr(), G.shape[0], ctx.per, L.cur_stream())
        return dout, None, None, None, None, None, None


class _ObjLossFunction(torch.autograd.Function):
    """training_losses of the non-default objectives (mapdit_obj_loss_fwd / mapdit_obj_loss_bwd): loss, mse, vb per sample
    (mse / vb are zeros where the objective has no such key) and the gradient wrt the model output."""

    @staticmethod
    def forward(ctx, model_output, x_start, x_t, noise, t, tab, otab, nsteps, kinds):
        mean_type, var_type, loss_type = kinds
        n = model_output.shape[0]
        per = x_start[0].numel()
        mo = model_output.contiguous().float()
        mse, vb, loss = (torch.zeros(n, device=mo.device) for _ in range(3))
        G = torch.empty_like(mo)
        with torch.cuda.device(mo.device):
            L.lib().obj_loss_fwd(mo.data_ptr(), x_start.data_ptr(), x_t.data_ptr(), noise.data_ptr(), t.data_ptr(), tab.data_ptr(),
                                 otab.data_ptr(), nsteps, mean_type, var_type, loss_type, mse.data_ptr(), vb.data_ptr(),
                                 loss.data_ptr(), G.data_ptr(), n, per, L.cur_stream())
        ctx.save_for_backward(G)
        ctx.per = per
        ctx.groups = 2 if var_type == _VAR_CODE[ModelVarType.LEARNED_RANGE] else 1
        ctx.kl = loss_type >= _LOSS_CODE[LossType.KL]
        return loss, mse, vb

    @staticmethod
    def backward(ctx, g_loss, g_mse, g_vb):
        (G,) = ctx.saved_tensors
        dout = torch.empty_like(G)
        if ctx.kl:                      # the KL losses have no mse / vb keys
            g_mse = g_vb = None
        gl, gm, gv = (None if g is None else g.contiguous().float() for g in (g_loss, g_mse, g_vb))
        with torch.cuda.device(G.device):
            L.lib().obj_loss_bwd(G.data_ptr(), L.ptr(gl), L.ptr(gm), L.ptr(gv), dout.data_ptr(), G.shape[0], ctx.per, ctx.groups,
                                 L.cur_stream())
        return dout, None, None, None, None, None, None, None, None


# kernel codes of the objectives (include/mapdit.h, mapdit_obj_*)
_MEAN_CODE = {ModelMeanType.EPSILON: 0, ModelMeanType.START_X: 1}
_VAR_CODE = {ModelVarType.LEARNED_RANGE: 0, ModelVarType.FIXED_SMALL: 1, ModelVarType.FIXED_LARGE: 2}
_LOSS_CODE = {LossType.MSE: 0, LossType.RESCALED_MSE: 1, LossType.KL: 2, LossType.RESCALED_KL: 3}
_STEP_PSAMPLE, _STEP_DDIM, _STEP_DDIM_REVERSE = 0, 1, 2


class GaussianDiffusion:
    """reference gaussian_diffusion.py:144-201 (constructor and tables)."""

    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type):
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        betas = np.array(betas, dtype=np.float64)
        self.betas = betas
        assert len(betas.shape) == 1, "betas must be 1-D"
        assert (betas > 0).all() and (betas <= 1).all()
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = (np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
                                               if len(self.posterior_variance) > 1 else np.array([]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        self._tab_cache = {}

    # ---- device-resident schedule (layout documented in include/mapdit.h) ------------------------------------------
    def _tables(self, device):
        tab = self._tab_cache.get(device)
        if tab is None:
            rows = [self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, self.sqrt_recip_alphas_cumprod,
                    self.sqrt_recipm1_alphas_cumprod, self.posterior_log_variance_clipped, np.log(self.betas),
                    self.posterior_mean_coef1, self.posterior_mean_coef2]
            tab = torch.from_numpy(np.stack(rows)).float().to(device).contiguous()     # fp32, as _extract_into_tensor
            self._tab_cache[device] = tab
        return tab

    def _ddim_tables(self, device):
        tab = self._tab_cache.get(("ddim", device))
        if tab is None:
            rows = [self.alphas_cumprod, self.alphas_cumprod_prev, self.alphas_cumprod_next]
            tab = torch.from_numpy(np.stack(rows)).float().to(device).contiguous()
            self._tab_cache[("ddim", device)] = tab
        return tab

    def _fixed_large_variance(self):
        """FIXED_LARGE's variance row (reference gaussian_diffusion.py:300-305)."""
        return np.append(self.posterior_variance[1], self.betas[1:])

    def _obj_tables(self, device):
        """The rows the mapdit_obj_* kernels read besides `tab` (layout in include/mapdit.h)."""
        tab = self._tab_cache.get(("obj", device))
        if tab is None:
            rows = [self.alphas_cumprod, self.alphas_cumprod_prev, self.alphas_cumprod_next, np.log(self._fixed_large_variance()),
                    self.log_one_minus_alphas_cumprod]
            tab = torch.from_numpy(np.stack(rows)).float().to(device).contiguous()
            self._tab_cache[("obj", device)] = tab
        return tab

    # ---- DPM-Solver++ (Lu et al. 2022): step selection and coefficients, fp64 on the host ------------------------------
    def _dpm_schedule(self, num_steps=20, order=2, spacing="logsnr", lower_order_final=True):
        """-> (tau int64 [K], coef float64 [K, 3]): the timesteps tau[0] = 0 < ... < tau[K-1] = n - 1 of this diffusion that the solver
        visits and, per solver step i (K-1 down to 0), the (c_x, c_0, c_1) of ``sample = c_x x + c_0 D + c_1 D_prev`` (layout and
        formulas in include/mapdit.h, mapdit_dpm_step).  K <= num_steps: "logsnr" drops the duplicates its rounding produces."""
        n = self.num_timesteps
        if isinstance(num_steps, bool) or not isinstance(num_steps, (int, np.integer)) or not 2 <= num_steps <= n:
            raise ValueError(f"num_steps must be an integer in [2, {n}] (the diffusion's own timesteps); got {num_steps!r}")
        if isinstance(order, bool) or order not in (1, 2):
            raise ValueError(f"order must be 1 or 2 (DPM-Solver++ first order / 2M); got {order!r}")
        num_steps = int(num_steps)
        alpha, sigma = np.sqrt(self.alphas_cumprod), np.sqrt(1.0 - self.alphas_cumprod)
        lam = np.log(alpha / sigma)
        if spacing == "logsnr":
            targets = np.linspace(lam[0], lam[n - 1], num_steps)
            tau = np.unique([int(np.argmin(np.abs(lam - v))) for v in targets])       # argmin: the lowest index on a tie
        elif spacing == "uniform":
            from .respace import space_timesteps
            tau = np.array(sorted(space_timesteps(n, str(num_steps))))
        else:
            raise ValueError(f'spacing must be "logsnr" or "uniform"; got {spacing!r}')
        tau = tau.astype(np.int64)
        K = len(tau)
        assert K >= 2 and tau[0] == 0 and tau[-1] == n - 1 and (np.diff(tau) > 0).all(), tau
        coef = np.zeros((K, 3), dtype=np.float64)
        coef[0] = (0.0, 1.0, 0.0)                                  # the final denoise: the x0 prediction at tau[0]
        for i in range(1, K):
            s, t = tau[i], tau[i - 1]
            h = lam[t] - lam[s]
            b = -alpha[t] * np.expm1(-h)
            c0, c1 = b, 0.0
            if order == 2 and i != K - 1 and not (i == 1 and lower_order_final):
                r = (lam[s] - lam[tau[i + 1]]) / h
                c0, c1 = b * (1.0 + 1.0 / (2.0 * r)), -b / (2.0 * r)
            coef[i] = (sigma[t] / sigma[s], c0, c1)
        return tau, coef

    def _dpm_tables(self, device, num_steps=20, order=2, spacing="logsnr", lower_order_final=True):
        """_dpm_schedule on the device, uploaded once per configuration -> (tau int64 [K], ctab fp32 [K][3], tau as a host list)."""
        key = ("dpm", num_steps, order, spacing, bool(lower_order_final), device)
        tabs = self._tab_cache.get(key)
        if tabs is None:
            tau, coef = self._dpm_schedule(num_steps, order, spacing, lower_order_final)
            tabs = (torch.from_numpy(tau).to(device).contiguous(), torch.from_numpy(coef).float().to(device).contiguous(),
                    [int(v) for v in tau])
            self._tab_cache[key] = tabs
        return tabs

    def _extract(self, name, t, shape):
        """reference _extract_into_tensor (:861-873) with the fp32 row resident on the device (uploaded once per row)."""
        key = ("row", name, t.device)
        row = self._tab_cache.get(key)
        if row is None:
            if name == "fixed_large_variance":
                arr = self._fixed_large_variance()
            elif name == "fixed_large_log_variance":
                arr = np.log(self._fixed_large_variance())
            else:
                arr = getattr(self, name)
            row = torch.from_numpy(np.asarray(arr, dtype=np.float64)).float().to(t.device)
            self._tab_cache[key] = row
        res = row[t]
        return res.view((-1,) + (1,) * (len(shape) - 1)) + torch.zeros(shape, device=t.device)

    def _is_default(self):
        return (self.model_mean_type == ModelMeanType.EPSILON and self.model_var_type == ModelVarType.LEARNED_RANGE
                and self.loss_type == LossType.MSE)

    def _supported(self):
        if self.model_mean_type == ModelMeanType.PREVIOUS_X:
            raise NotImplementedError("ModelMeanType.PREVIOUS_X is not built: the reference's p_mean_variance has no branch for it "
                                      "(it would read the x_{t-1} prediction as eps), so there is no behaviour to match")
        if self.model_mean_type not in _MEAN_CODE or self.model_var_type not in _VAR_CODE or self.loss_type not in _LOSS_CODE:
            raise NotImplementedError("built: mean EPSILON / START_X, variance LEARNED_RANGE / FIXED_SMALL / FIXED_LARGE (every "
                                      "objective create_diffusion() produces); "
                                      f"got {self.model_mean_type}, {self.model_var_type}, {self.loss_type}")

    def _kinds(self):
        return _MEAN_CODE[self.model_mean_type], _VAR_CODE[self.model_var_type], _LOSS_CODE[self.loss_type]

    def _out_channels(self, C):
        return 2 * C if self.model_var_type == ModelVarType.LEARNED_RANGE else C

    def _wrap_model(self, model):
        return model

    def _model_output(self, model, x, t, model_kwargs):
        """model(x, t) through the timestep map, checked against the channel count of the variance type."""
        out = self._wrap_model(model)(x, t, **(model_kwargs or {}))
        B, C = x.shape[:2]
        assert out.shape == (B, self._out_channels(C), *x.shape[2:]), (tuple(out.shape), self.model_var_type)
        return out

    @staticmethod
    def _prep(x):
        # an explicit raise, not an assert: under python -O an assert vanishes and a host pointer would reach a kernel
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            where = f"a tensor on {x.device}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise NotImplementedError(f"the diffusion kernels run on the MI355X only (no CPU path); got {where}")
        return x.contiguous().float()

    # ---- forward process ------------------------------------------------------------------------------------------------
    def q_sample(self, x_start, t, noise=None):
        """reference gaussian_diffusion.py:215-230."""
        x_start = self._prep(x_start)
        if noise is None:
            noise = torch.randn_like(x_start)
        assert noise.shape == x_start.shape
        noise = self._prep(noise)
        t = t.to(device=x_start.device, dtype=torch.int64).contiguous()
        out = torch.empty_like(x_start)
        with torch.cuda.device(x_start.device):
            L.lib().q_sample(x_start.data_ptr(), noise.data_ptr(), t.data_ptr(), self._tables(x_start.device).data_ptr(),
                             self.num_timesteps, out.data_ptr(), x_start.shape[0], x_start[0].numel(), L.cur_stream())
        return out

    def q_mean_variance(self, x_start, t):
        """reference gaussian_diffusion.py:203-213 -> (mean, variance, log_variance), each of x_start's shape."""
        shape = x_start.shape
        mean = self._extract("sqrt_alphas_cumprod", t, shape) * x_start
        return mean, self._extract("one_minus_alphas_cumprod", t, shape), self._extract("log_one_minus_alphas_cumprod", t, shape)

    @property
    def one_minus_alphas_cumprod(self):
        return 1.0 - self.alphas_cumprod

    @property
    def _log_betas(self):
        return np.log(self.betas)

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """reference gaussian_diffusion.py:232-252 -> (posterior mean, variance, clipped log-variance)."""
        assert x_start.shape == x_t.shape
        shape = x_t.shape
        mean = self._extract("posterior_mean_coef1", t, shape) * x_start + self._extract("posterior_mean_coef2", t, shape) * x_t
        return mean, self._extract("posterior_variance", t, shape), self._extract("posterior_log_variance_clipped", t, shape)

    def _predict_xstart_from_eps(self, x_t, t, eps):
        """reference gaussian_diffusion.py:334-339."""
        assert x_t.shape == eps.shape
        return (self._extract("sqrt_recip_alphas_cumprod", t, x_t.shape) * x_t
                - self._extract("sqrt_recipm1_alphas_cumprod", t, x_t.shape) * eps)

    def _predict_eps_from_xstart(self, x_t, t, pred_xstart):
        """reference gaussian_diffusion.py:341-344."""
        return ((self._extract("sqrt_recip_alphas_cumprod", t, x_t.shape) * x_t - pred_xstart)
                / self._extract("sqrt_recipm1_alphas_cumprod", t, x_t.shape))

    # ---- training ----------------------------------------------------------------------------------------------------------
    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None):
        """reference gaussian_diffusion.py:715-787 -> {"loss", "mse", "vb"} (LEARNED_RANGE with an MSE loss), {"loss", "mse"}
        (fixed variance, MSE loss) or {"loss"} (KL losses), each [N]."""
        self._supported()
        if model_kwargs is None:
            model_kwargs = {}
        x_start = self._prep(x_start)
        if noise is None:
            noise = torch.randn_like(x_start)
        noise = self._prep(noise)
        t = t.to(device=x_start.device, dtype=torch.int64).contiguous()
        x_t = self.q_sample(x_start, t, noise=noise)
        if not self._is_default():
            model_output = self._model_output(model, x_t, t, model_kwargs)
            loss, mse, vb = _ObjLossFunction.apply(model_output, x_start, x_t, noise, t, self._tables(x_start.device),
                                                   self._obj_tables(x_start.device), self.num_timesteps, self._kinds())
            if self.loss_type.is_vb():
                return {"loss": loss}
            if self.model_var_type == ModelVarType.LEARNED_RANGE:
                return {"vb": vb, "mse": mse, "loss": loss}
            return {"mse": mse, "loss": loss}
        model_output = model(x_t, t, **model_kwargs)
        B, C = x_t.shape[:2]
        assert model_output.shape == (B, C * 2, *x_t.shape[2:])
        loss, mse, vb = _LossFunction.apply(model_output, x_start, x_t, noise, t, self._tables(x_start.device),
                                            self.num_timesteps)
        return {"vb": vb, "mse": mse, "loss": loss}

    # ---- reverse process ---------------------------------------------------------------------------------------------------
    def _obj_step(self, model_output, x, t, noise, clip_denoised, mode, eta=0.0):
        """mapdit_obj_step: p_mean_variance + p_sample / DDIM / reverse DDIM for any built objective -> (sample, pred_xstart).
        noise None with mode p_sample: the model mean."""
        x = self._prep(x)
        mo = self._prep(model_output)
        mean_type, var_type, _ = self._kinds()
        sample, xstart = torch.empty_like(x), torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.lib().obj_step(mo.data_ptr(), x.data_ptr(), L.ptr(noise), t.data_ptr(), self._tables(x.device).data_ptr(),
                             self._obj_tables(x.device).data_ptr(), self.num_timesteps, mean_type, var_type, int(bool(clip_denoised)),
                             mode, float(eta), sample.data_ptr(), xstart.data_ptr(), x.shape[0], x[0].numel(), L.cur_stream())
        return sample, xstart

    def _hooks(self, model_output, x, t, denoised_fn, cond_fn, model_kwargs):
        """What the hooks hand the guided kernel: denoised_fn(raw x0 prediction) (mapdit_obj_xstart feeds it) and
        cond_fn(x, t, **model_kwargs), t mapped to the base schedule under SpacedDiffusion -> (xstart_in, cond_grad), None where
        the hook is not given."""
        xin = grad = None
        if denoised_fn is not None:
            mean_type, var_type, _ = self._kinds()
            mo = self._prep(model_output)
            raw = torch.empty_like(x)
            with torch.cuda.device(x.device):
                L.lib().obj_xstart(mo.data_ptr(), x.data_ptr(), t.data_ptr(), self._tables(x.device).data_ptr(), self.num_timesteps,
                                   mean_type, var_type, raw.data_ptr(), x.shape[0], x[0].numel(), L.cur_stream())
            xin = self._prep(denoised_fn(raw))
            assert xin.shape == x.shape, (tuple(xin.shape), tuple(x.shape))
        if cond_fn is not None:
            grad = self._cond_grad(cond_fn, x, t, model_kwargs)
        return xin, grad

    def _cond_grad(self, cond_fn, x, t, model_kwargs):
        grad = self._prep(self._wrap_model(cond_fn)(x, t, **(model_kwargs or {})))
        assert grad.shape == x.shape, (tuple(grad.shape), tuple(x.shape))
        return grad

    def _guided_step(self, model_output, x, t, noise, clip_denoised, mode, eta=0.0, xstart_in=None, cond_grad=None, sample=True,
                     mean=False):
        """mapdit_obj_step_guided -> (sample, pred_xstart, mean); sample / mean are None unless asked for.  The default objective
        runs it as mean type 0, variance type 0."""
        mean_type, var_type, _ = self._kinds()
        mo = None if model_output is None else self._prep(model_output)
        out_s = torch.empty_like(x) if sample else None
        out_m = torch.empty_like(x) if mean else None
        xstart = torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.lib().obj_step_guided(L.ptr(mo), x.data_ptr(), L.ptr(noise), t.data_ptr(), self._tables(x.device).data_ptr(),
                                    self._obj_tables(x.device).data_ptr(), self.num_timesteps, mean_type, var_type,
                                    int(bool(clip_denoised)), mode, float(eta), L.ptr(xstart_in), L.ptr(cond_grad), L.ptr(out_s),
                                    xstart.data_ptr(), L.ptr(out_m), x.shape[0], x[0].numel(), L.cur_stream())
        return out_s, xstart, out_m

    def condition_mean(self, cond_fn, p_mean_var, x, t, model_kwargs=None):
        """reference gaussian_diffusion.py:346-356 -> mean + variance * cond_fn(x, t, **model_kwargs) (Sohl-Dickstein et al. 2015).
        p_sample does not come through here: mapdit_obj_step_guided applies the same shift inside the step."""
        x = self._prep(x)
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        grad = self._cond_grad(cond_fn, x, t, model_kwargs)
        return torch.addcmul(p_mean_var["mean"].float(), p_mean_var["variance"], grad)

    def condition_score(self, cond_fn, p_mean_var, x, t, model_kwargs=None):
        """reference gaussian_diffusion.py:358-374 -> a copy of p_mean_var with pred_xstart and mean as they would have been, had the
        model's score been conditioned by cond_fn (Song et al. 2020).  The DDIM steps apply the same in their own launch."""
        self._supported()
        x = self._prep(x)
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        grad = self._cond_grad(cond_fn, x, t, model_kwargs)
        _, xstart, mean = self._guided_step(None, x, t, None, False, _STEP_DDIM, xstart_in=self._prep(p_mean_var["pred_xstart"]),
                                            cond_grad=grad, sample=False, mean=True)
        out = p_mean_var.copy()
        out["pred_xstart"], out["mean"] = xstart, mean
        return out

    def _step_math(self, model_output, x, t, noise, clip_denoised):
        if not self._is_default():
            return self._obj_step(model_output, x, t, noise, clip_denoised, _STEP_PSAMPLE)
        x = self._prep(x)
        mo = self._prep(model_output)
        sample, xstart = torch.empty_like(x), torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.lib().psample_step(mo.data_ptr(), x.data_ptr(), noise.data_ptr(), t.data_ptr(), self._tables(x.device).data_ptr(),
                                 self.num_timesteps, int(bool(clip_denoised)), sample.data_ptr(), xstart.data_ptr(),
                                 x.shape[0], x[0].numel(), L.cur_stream())
        return sample, xstart

    def _counter_step(self, model_output, x, t, rng, index, clip_denoised, mode, eta=0.0):
        """The unhooked stochastic step with its noise generated in the kernel from (rng.seed, index[j], t[j]): the default
        objective's p_sample is mapdit_psample_step_counter, everything else mapdit_obj_step_counter -> (sample, pred_xstart)."""
        x = self._prep(x)
        mo = self._prep(model_output)
        sample, xstart = torch.empty_like(x), torch.empty_like(x)
        with torch.cuda.device(x.device):
            if mode == _STEP_PSAMPLE and self._is_default():
                L.lib().psample_step_counter(mo.data_ptr(), x.data_ptr(), rng.seed, index.data_ptr(), t.data_ptr(),
                                             self._tables(x.device).data_ptr(), self.num_timesteps, int(bool(clip_denoised)),
                                             sample.data_ptr(), xstart.data_ptr(), x.shape[0], x[0].numel(), L.cur_stream())
            else:
                mean_type, var_type, _ = self._kinds()
                L.lib().obj_step_counter(mo.data_ptr(), x.data_ptr(), rng.seed, index.data_ptr(), t.data_ptr(),
                                         self._tables(x.device).data_ptr(), self._obj_tables(x.device).data_ptr(), self.num_timesteps,
                                         mean_type, var_type, int(bool(clip_denoised)), mode, float(eta), sample.data_ptr(),
                                         xstart.data_ptr(), x.shape[0], x[0].numel(), L.cur_stream())
        return sample, xstart

    @staticmethod
    def _rng_rows(rng, index, rows):
        """The loops' rng= / index= pair, checked once, with the index laid out over the batch's rows (sample_rng.rows_index)."""
        from ..sample_rng import pair, rows_index
        rng, index = pair(rng, index)
        return rng, (None if rng is None else rows_index(index, rows))

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        """reference gaussian_diffusion.py:254-332 (mean = the p_sample kernel with zero noise)."""
        self._supported()
        x = self._prep(x)
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        B, C = x.shape[:2]
        assert t.shape == (B,)

        def hooked(model_output):          # pred_xstart = clip(denoised_fn(raw x0)) and the posterior mean built from it
            xin, _ = self._hooks(model_output, x, t, denoised_fn, None, None)
            mean, xstart, _ = self._guided_step(model_output, x, t, None, clip_denoised, _STEP_PSAMPLE, xstart_in=xin)
            return mean, xstart
        if not self._is_default():
            model_output = self._model_output(model, x, t, model_kwargs)
            if denoised_fn is not None:
                mean, xstart = hooked(model_output)
            else:
                mean, xstart = self._obj_step(model_output, x, t, None, clip_denoised, _STEP_PSAMPLE)
            if self.model_var_type == ModelVarType.LEARNED_RANGE:
                frac = (model_output[:, C:].float() + 1) / 2
                log_var = (frac * self._extract("_log_betas", t, x.shape)
                           + (1 - frac) * self._extract("posterior_log_variance_clipped", t, x.shape))
                var = torch.exp(log_var)
            elif self.model_var_type == ModelVarType.FIXED_SMALL:
                var = self._extract("posterior_variance", t, x.shape)
                log_var = self._extract("posterior_log_variance_clipped", t, x.shape)
            else:
                var = self._extract("fixed_large_variance", t, x.shape)
                log_var = self._extract("fixed_large_log_variance", t, x.shape)
            return {"mean": mean, "variance": var, "log_variance": log_var, "pred_xstart": xstart, "extra": None,
                    "model_output": model_output}
        model_output = model(x, t, **(model_kwargs or {}))
        assert model_output.shape == (B, C * 2, *x.shape[2:])
        if denoised_fn is not None:
            mean, xstart = hooked(model_output)
        else:
            mean, xstart = self._step_math(model_output, x, t, torch.zeros_like(x), clip_denoised)
        tab = self._tables(x.device)
        n = self.num_timesteps
        frac = (model_output[:, C:].float() + 1) / 2
        shape = (-1,) + (1,) * (x.dim() - 1)
        log_var = frac * tab[5][t].view(shape) + (1 - frac) * tab[4][t].view(shape)
        return {"mean": mean, "variance": torch.exp(log_var), "log_variance": log_var, "pred_xstart": xstart, "extra": None,
                "model_output": model_output}

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, rng=None, index=None):
        """reference gaussian_diffusion.py:376-417.  rng= (a SampleRNG) with index= (the sample index of every row): the step's noise is
        the contract's noise[index[j]][t[j]] instead of a torch.randn_like draw - generated inside the step kernel, or materialised
        for a hooked step."""
        rng, index = self._rng_rows(rng, index, x.shape[0])
        return self._p_sample(model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, rng, index)

    def _p_sample(self, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, rng, index):
        self._supported()
        x = self._prep(x)
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        model_output = (self._wrap_model(model)(x, t, **(model_kwargs or {})) if self._is_default()
                        else self._model_output(model, x, t, model_kwargs))
        if denoised_fn is not None or cond_fn is not None:
            xin, grad = self._hooks(model_output, x, t, denoised_fn, cond_fn, model_kwargs)
            noise = torch.randn_like(x) if rng is None else rng.noise_checked(index, t, x.shape)
            sample, xstart, _ = self._guided_step(model_output, x, t, noise, clip_denoised, _STEP_PSAMPLE, xstart_in=xin, cond_grad=grad)
            return {"sample": sample, "pred_xstart": xstart}
        if rng is not None:
            sample, xstart = self._counter_step(model_output, x, t, rng, index, clip_denoised, _STEP_PSAMPLE)
            return {"sample": sample, "pred_xstart": xstart}
        noise = torch.randn_like(x)
        sample, xstart = self._step_math(model_output, x, t, noise, clip_denoised)
        return {"sample": sample, "pred_xstart": xstart}

    # ---- DDIM (reference gaussian_diffusion.py:513-680; no reference script uses it) ----------------------------------
    def _ddim_math(self, model_output, x, t, noise, clip_denoised, eta, reverse):
        if not self._is_default():
            return self._obj_step(model_output, x, t, noise, clip_denoised, _STEP_DDIM_REVERSE if reverse else _STEP_DDIM, eta)
        x = self._prep(x)
        mo = self._prep(model_output)
        sample, xstart = torch.empty_like(x), torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.lib().ddim_step(mo.data_ptr(), x.data_ptr(), L.ptr(noise), t.data_ptr(), self._tables(x.device).data_ptr(),
                              self._ddim_tables(x.device).data_ptr(), self.num_timesteps, int(bool(clip_denoised)), float(eta),
                              int(bool(reverse)), sample.data_ptr(), xstart.data_ptr(), x.shape[0], x[0].numel(), L.cur_stream())
        return sample, xstart

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0, rng=None,
                    index=None):
        """reference gaussian_diffusion.py:513-567.  rng= / index= as p_sample takes them: the same noise words, scaled by sigma(eta)."""
        rng, index = self._rng_rows(rng, index, x.shape[0])
        return self._ddim_sample(model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, rng, index)

    def _ddim_sample(self, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, rng, index):
        self._supported()
        x = self._prep(x)
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        model_output = (self._wrap_model(model)(x, t, **(model_kwargs or {})) if self._is_default()
                        else self._model_output(model, x, t, model_kwargs))
        if denoised_fn is not None or cond_fn is not None:
            xin, grad = self._hooks(model_output, x, t, denoised_fn, cond_fn, model_kwargs)
            noise = torch.randn_like(x) if rng is None else rng.noise_checked(index, t, x.shape)
            sample, xstart, _ = self._guided_step(model_output, x, t, noise, clip_denoised, _STEP_DDIM, eta, xstart_in=xin, cond_grad=grad)
            return {"sample": sample, "pred_xstart": xstart}
        if rng is not None:               # (eta = 0: sigma is 0 and the words drop out - the deterministic solver takes only its start)
            sample, xstart = self._counter_step(model_output, x, t, rng, index, clip_denoised, _STEP_DDIM, eta)
            return {"sample": sample, "pred_xstart": xstart}
        noise = torch.randn_like(x)
        sample, xstart = self._ddim_math(model_output, x, t, noise, clip_denoised, eta, False)
        return {"sample": sample, "pred_xstart": xstart}

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
        """reference gaussian_diffusion.py:569-605: x_{t+1} along the deterministic reverse ODE."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        self._supported()
        x = self._prep(x)
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        model_output = (self._wrap_model(model)(x, t, **(model_kwargs or {})) if self._is_default()
                        else self._model_output(model, x, t, model_kwargs))
        if denoised_fn is not None or cond_fn is not None:
            xin, grad = self._hooks(model_output, x, t, denoised_fn, cond_fn, model_kwargs)
            sample, xstart, _ = self._guided_step(model_output, x, t, None, clip_denoised, _STEP_DDIM_REVERSE, xstart_in=xin, cond_grad=grad)
            return {"sample": sample, "pred_xstart": xstart}
        sample, xstart = self._ddim_math(model_output, x, t, None, clip_denoised, 0.0, True)
        return {"sample": sample, "pred_xstart": xstart}

    # ---- likelihood (reference gaussian_diffusion.py:682-713, 789-858) --------------------------------------------------
    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """reference gaussian_diffusion.py:682-713 -> {"output": [N] bits (decoder NLL at t = 0, KL otherwise), "pred_xstart"}."""
        self._supported()
        x_start, x_t = self._prep(x_start), self._prep(x_t)
        t = t.to(device=x_t.device, dtype=torch.int64).contiguous()
        mo = self._prep(self._model_output(model, x_t, t, model_kwargs))
        mean_type, var_type, _ = self._kinds()
        out, xstart = torch.empty(x_t.shape[0], device=x_t.device), torch.empty_like(x_t)
        with torch.cuda.device(x_t.device):
            L.lib().obj_vb_terms(mo.data_ptr(), x_start.data_ptr(), x_t.data_ptr(), None, t.data_ptr(), self._tables(x_t.device).data_ptr(),
                                 self._obj_tables(x_t.device).data_ptr(), self.num_timesteps, mean_type, var_type,
                                 int(bool(clip_denoised)), out.data_ptr(), None, None, xstart.data_ptr(), 1, 0, x_t.shape[0],
                                 x_t[0].numel(), L.cur_stream())
        return {"output": out, "pred_xstart": xstart}

    def _prior_bpd(self, x_start):
        """reference gaussian_diffusion.py:789-803: KL(q(x_T | x_0) || N(0, I)) in bits, [N]."""
        x_start = self._prep(x_start)
        prior = torch.empty(x_start.shape[0], device=x_start.device)
        with torch.cuda.device(x_start.device):
            L.lib().prior_bpd(x_start.data_ptr(), self._tables(x_start.device).data_ptr(), self._obj_tables(x_start.device).data_ptr(),
                              self.num_timesteps, None, prior.data_ptr(), None, x_start.shape[0], x_start[0].numel(), L.cur_stream())
        return prior

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None):
        """reference gaussian_diffusion.py:805-858 -> {"total_bpd", "prior_bpd" [N]; "vb", "xstart_mse", "mse" [N, T]}.

        The whole loop is enqueued without a host synchronisation: per timestep (T-1 down to 0) one N(0,1) draw
        (``torch.randn_like(x_start)``, the reference's order), q_sample, the model forward and one mapdit_obj_vb_terms launch
        that writes column T-1-t of the three [N, T] arrays (the reference stacks them in loop order); then one mapdit_prior_bpd launch for the prior and the total.  Device
        errors (an out-of-range timestep or label) are polled once at the end."""
        self._supported()
        x_start = self._prep(x_start)
        dev, N, T = x_start.device, x_start.shape[0], self.num_timesteps
        per = x_start[0].numel()
        mean_type, var_type, _ = self._kinds()
        tab, otab = self._tables(dev), self._obj_tables(dev)
        vb, xstart_mse, mse = (torch.empty(N, T, device=dev) for _ in range(3))
        for i in range(T)[::-1]:
            t = torch.full((N,), i, device=dev, dtype=torch.int64)
            noise = torch.randn_like(x_start)
            x_t = self.q_sample(x_start, t, noise=noise)
            with torch.no_grad():
                mo = self._prep(self._model_output(model, x_t, t, model_kwargs))
            with torch.cuda.device(dev):
                L.lib().obj_vb_terms(mo.data_ptr(), x_start.data_ptr(), x_t.data_ptr(), noise.data_ptr(), t.data_ptr(), tab.data_ptr(),
                                     otab.data_ptr(), T, mean_type, var_type, int(bool(clip_denoised)), vb.data_ptr(),
                                     xstart_mse.data_ptr(), mse.data_ptr(), None, T, 1, N, per, L.cur_stream())
        prior, total = torch.empty(N, device=dev), torch.empty(N, device=dev)
        with torch.cuda.device(dev):
            L.lib().prior_bpd(x_start.data_ptr(), tab.data_ptr(), otab.data_ptr(), T, vb.data_ptr(), prior.data_ptr(), total.data_ptr(),
                              N, per, L.cur_stream())
            L.lib().device_error_poll(L.cur_stream())
        return {"total_bpd": total, "prior_bpd": prior, "vb": vb, "xstart_mse": xstart_mse, "mse": mse}

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                         device=None, progress=False, eta=0.0, rng=None, index=None):
        """reference gaussian_diffusion.py:607-636.  rng= / index=: as p_sample_loop."""
        final = None
        for sample in self.ddim_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                        denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs,
                                                        device=device, progress=progress, eta=eta, rng=rng, index=index):
            final = sample
        return final["sample"]

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, rng=None, index=None):
        """reference gaussian_diffusion.py:638-680."""
        rng, index = self._rng_rows(rng, index, shape[0])
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else self._start(shape, device, rng, index)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for i in indices:
            t = torch.full((shape[0],), i, device=device, dtype=torch.int64)
            with torch.no_grad():
                if rng is None:
                    out = self.ddim_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                           model_kwargs=model_kwargs, eta=eta)
                else:
                    out = self._ddim_sample(model, img, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, rng, index)
                yield out
                img = out["sample"]

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                      device=None, progress=False, rng=None, index=None):
        """reference gaussian_diffusion.py:419-462.  rng= (a SampleRNG) and index= (one sample index per row, or per row of one half of
        a classifier-free-guidance batch: the two halves then carry the same indices) go together: the initial latent (where noise is
        None) and every step's noise are the contract's draws of those indices, whatever else the process has drawn."""
        final = None
        for sample in self.p_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                     denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs,
                                                     device=device, progress=progress, rng=rng, index=index):
            final = sample
        with torch.cuda.device(final["sample"].device):
            L.lib().device_error_poll(L.cur_stream())      # out-of-range label / timestep anywhere in the loop -> MapditError
        return final["sample"]

    @staticmethod
    def _start(shape, device, rng, index):
        """The loops' initial latent where none is given: torch.randn, or the rng's latents of the rows' sample indices."""
        if rng is None:
            return torch.randn(*shape, device=device)
        return rng.latents(index, tuple(shape[1:]))

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, rng=None, index=None):
        """reference gaussian_diffusion.py:464-511."""
        rng, index = self._rng_rows(rng, index, shape[0])
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else self._start(shape, device, rng, index)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for i in indices:
            t = torch.full((shape[0],), i, device=device, dtype=torch.int64)
            with torch.no_grad():
                if rng is None:
                    out = self.p_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                        model_kwargs=model_kwargs)
                else:                      # (the pair was checked once, above: no host read per step)
                    out = self._p_sample(model, img, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, rng, index)
                yield out
                img = out["sample"]

    # ---- DPM-Solver++ (not in the reference: a high-order solver of the probability-flow ODE, ~20 model evaluations) --------
    def _dpm_step(self, model_output, x, hist, step, tabs, clip_denoised, xstart_in=None, sample=None):
        """mapdit_dpm_step -> (sample, pred_xstart); hist is updated in place.  sample: the tensor to write (may be x itself)."""
        tau, ctab, _ = tabs
        mean_type, var_type, _ = self._kinds()
        mo = None if model_output is None else self._prep(model_output)
        sample = torch.empty_like(x) if sample is None else sample
        xstart = torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.lib().dpm_step(L.ptr(mo), x.data_ptr(), hist.data_ptr(), step.data_ptr(), ctab.data_ptr(), tau.data_ptr(), tau.shape[0],
                             self._tables(x.device).data_ptr(), self.num_timesteps, mean_type, var_type, int(bool(clip_denoised)),
                             L.ptr(xstart_in), sample.data_ptr(), xstart.data_ptr(), x.shape[0], x[0].numel(), L.cur_stream())
        return sample, xstart

    def dpm_solver_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                               device=None, progress=False, rng=None, index=None, num_steps=20, order=2, spacing="logsnr",
                               lower_order_final=True):
        """Deterministic sampling with the multistep DPM-Solver++ (Lu et al. 2022; order 2 = "2M", order 1 = the DDIM eta = 0 update):
        at most ``num_steps`` model evaluations on timesteps of this diffusion chosen by ``spacing`` ("logsnr": nearest to equal steps
        of the log signal-to-noise ratio, duplicates dropped; "uniform": ``space_timesteps``).  Signature and hooks as
        ``ddim_sample_loop``; the variance channels of a learned-range model are ignored.  rng= / index=: the start (where noise is None) is
        the rng's latents of those sample indices; the solver draws nothing else."""
        final = None
        for sample in self.dpm_solver_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                              denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs,
                                                              device=device, progress=progress, num_steps=num_steps, order=order,
                                                              spacing=spacing, lower_order_final=lower_order_final, rng=rng, index=index):
            final = sample
        with torch.cuda.device(final["sample"].device):
            L.lib().device_error_poll(L.cur_stream())      # out-of-range label / timestep / step index anywhere in the loop
        return final["sample"]

    def dpm_solver_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                           model_kwargs=None, device=None, progress=False, rng=None, index=None, num_steps=20, order=2,
                                           spacing="logsnr", lower_order_final=True):
        """Yields {"sample", "pred_xstart"} per solver step.  After the model, an unhooked step is one mapdit_dpm_step launch.
        denoised_fn sees the raw x0 prediction (mapdit_obj_xstart) and its result is clipped inside the step; cond_fn goes through
        condition_score (mapdit_obj_step_guided without a sample: x0 moved by the gradient after the clip, not clipped again), and
        the conditioned x0 is what the solver uses and remembers."""
        self._supported()
        rng, index = self._rng_rows(rng, index, shape[0])
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        tabs = self._dpm_tables(torch.device(device), num_steps, order, spacing, lower_order_final)
        taus = tabs[2]
        img = self._prep(noise if noise is not None else self._start(shape, device, rng, index))
        hist = torch.zeros_like(img)          # c_1 = 0 on the first step, but 0 x NaN of an uninitialised buffer is NaN
        indices = list(range(len(taus)))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for i in indices:
            step = torch.full((shape[0],), i, device=device, dtype=torch.int64)
            t = torch.full((shape[0],), taus[i], device=device, dtype=torch.int64)
            with torch.no_grad():
                model_output = self._model_output(model, img, t, model_kwargs)
                xin, clip = None, clip_denoised
                if denoised_fn is not None or cond_fn is not None:
                    xin, grad = self._hooks(model_output, img, t, denoised_fn, cond_fn, model_kwargs)
                    if grad is not None:
                        _, xin, _ = self._guided_step(model_output, img, t, None, clip_denoised, _STEP_DDIM, xstart_in=xin,
                                                      cond_grad=grad, sample=False)
                        clip = False
                sample, xstart = self._dpm_step(model_output, img, hist, step, tabs, clip, xstart_in=xin)
                out = {"sample": sample, "pred_xstart": xstart}
                yield out
                img = sample
