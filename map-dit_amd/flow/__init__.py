"""Rectified flow on HIP kernels: the linear-interpolant ("flow matching") velocity objective of SiT / SD3 and its Euler / Heun ODE
sampler.  Not in the reference, whose ``diffusion/`` package builds variance-preserving DDPM objectives only.

    x_s = (1 - s) x0 + s eps,      velocity dx/ds = eps - x0,      s = 1: pure noise, s = 0: data

The network is the DiT as it is: it takes integer timesteps, so flow time lives on a grid of ``T`` points.  Index ``k`` in ``[0, T)``
stands for ``s_k = shifted((k + 1) / T)`` with SD3's resolution shift ``shifted(s) = shift s / (1 + (shift - 1) s)``; ``s = 0`` is no
grid index and is never given to the model.  The model's first ``C`` output channels are the velocity; the second ``C`` of a
``learn_sigma`` DiT are ignored and their gradient is exactly zero.

The forward process, the loss with its gradient, the logit-normal timestep map and a sampler evaluation are one launch each
(``mapdit_flow_*``, csrc/flow.hip); the solver plan is built here in fp64 (``_schedule``) and uploaded once per configuration.
Out of scope: stochastic sampling, likelihoods, sampler hooks and clipping, off-grid times.
"""
import collections
import math

import numpy as np
import torch

from .. import _lib as L

MAX_TIMESTEPS = 16384          # csrc/flow.hip FLOW_MAX_T

FlowPlan = collections.namedtuple("FlowPlan", "steps h t coef kind")
FlowPlan.__doc__ = """The evaluation plan of ``RectifiedFlow._schedule``, in execution order.
steps int64 [K']: the grid index each solver step starts at (strictly decreasing, steps[0] = T - 1; the last step ends at s = 0);
h fp64 [K']: the step sizes s_b - s_a < 0, differences of the table values used; t int64 [J]: the timestep of each model evaluation;
coef fp64 [J, 2]: (c_h, c_v) of ``out = base + c_h hist + c_v v``; kind int32 [J]: 1 = predictor row (hist <- v, base kept), 0 =
committing row (base <- out)."""


def shifted(s, shift):
    """SD3's resolution shift of flow time; the identity for shift = 1."""
    return shift * s / (1.0 + (shift - 1.0) * s)


def mean_flat(tensor):
    return tensor.mean(dim=list(range(1, len(tensor.shape))))


class _FlowLossFunction(torch.autograd.Function):
    """mean_flat((v - (eps - x0))^2) per sample with the gradient wrt the model output (mapdit_flow_loss_fwd / mapdit_obj_loss_bwd)."""

    @staticmethod
    def forward(ctx, model_output, x_start, noise):
        n = model_output.shape[0]
        per = x_start[0].numel()
        mo = model_output.contiguous().float()
        groups = mo[0].numel() // per
        loss = torch.empty(n, device=mo.device)
        G = torch.empty_like(mo)
        with torch.cuda.device(mo.device):
            L.lib().flow_loss_fwd(mo.data_ptr(), x_start.data_ptr(), noise.data_ptr(), loss.data_ptr(), G.data_ptr(), n, per, groups,
                                  L.cur_stream())
        ctx.save_for_backward(G)
        ctx.per, ctx.groups = per, groups
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (G,) = ctx.saved_tensors
        dout = torch.empty_like(G)
        gl = g_loss.contiguous().float()
        with torch.cuda.device(G.device):
            L.lib().obj_loss_bwd(G.data_ptr(), L.ptr(gl), None, None, dout.data_ptr(), G.shape[0], ctx.per, ctx.groups, L.cur_stream())
        return dout, None, None


class RectifiedFlow:
    """The rectified-flow process on a ``num_timesteps``-point grid.  ``sigmas`` is the fp64 numpy row [T] of the flow times."""

    def __init__(self, num_timesteps=1000, shift=1.0):
        if isinstance(num_timesteps, bool) or not isinstance(num_timesteps, (int, np.integer)) or not 1 <= num_timesteps <= MAX_TIMESTEPS:
            raise ValueError(f"num_timesteps must be an integer in [1, {MAX_TIMESTEPS}]; got {num_timesteps!r}")
        if isinstance(shift, bool) or not isinstance(shift, (int, float, np.integer, np.floating)) or not math.isfinite(shift) or not shift > 0:
            raise ValueError(f"shift must be finite and positive; got {shift!r}")
        self.num_timesteps = int(num_timesteps)
        self.shift = float(shift)
        T = self.num_timesteps
        sig = shifted((np.arange(T, dtype=np.float64) + 1.0) / T, self.shift)
        sig[-1] = 1.0                                                  # shifted(1) = shift / shift
        if not (sig[0] > 0 and (np.diff(sig) > 0).all() and (np.diff(sig.astype(np.float32)) > 0).all()):
            raise ValueError(f"shift={shift!r} leaves the {T} flow times of the grid indistinct in fp32: use a shift closer to 1 or fewer timesteps")
        self.sigmas = sig
        self._tab_cache = {}

    # ---- device-resident tables -------------------------------------------------------------------------------------------
    def _tables(self, device):
        """sigmas as fp32 [T] on `device`, uploaded once per device."""
        device = torch.device(device)
        tab = self._tab_cache.get(device)
        if tab is None:
            tab = torch.from_numpy(self.sigmas).float().to(device).contiguous()
            self._tab_cache[device] = tab
        return tab

    def _schedule(self, num_steps=50, order=1):
        """The solver plan, fp64 on the host -> FlowPlan.  Target times shifted(1 - j / num_steps), j = 0 .. num_steps; each target above 0
        is replaced by the nearest grid point (the lower index on a tie), duplicates are dropped, the last target is exactly 0.  Every
        step size is the difference of the table values used.  order 1: Euler, one evaluation per step.  order 2: Heun - a predictor
        row at (x, k_a), a corrector row at (x + h v1, k_b); the final step (s_b = 0, no grid point to evaluate at) is an Euler row:
        2 K' - 1 evaluations for K' steps."""
        if isinstance(num_steps, bool) or not isinstance(num_steps, (int, np.integer)) or num_steps < 1:
            raise ValueError(f"num_steps must be an integer >= 1; got {num_steps!r}")
        if isinstance(order, bool) or order not in (1, 2):
            raise ValueError(f"order must be 1 (Euler) or 2 (Heun); got {order!r}")
        K = int(num_steps)
        sig = self.sigmas
        targets = shifted(1.0 - np.arange(K, dtype=np.float64) / K, self.shift)
        steps = []
        for v in targets:
            k = int(np.argmin(np.abs(sig - v)))                        # argmin: the lowest index on a tie
            if not steps or k < steps[-1]:
                steps.append(k)
        steps = np.array(steps, dtype=np.int64)
        assert steps[0] == self.num_timesteps - 1 and (np.diff(steps) < 0).all(), steps
        s_a = sig[steps]
        s_b = np.append(sig[steps[1:]], 0.0)
        h = s_b - s_a
        t, coef, kind = [], [], []
        for i in range(len(steps)):
            last = i == len(steps) - 1
            if order == 1 or last:
                t.append(steps[i]); coef.append((0.0, h[i])); kind.append(0)
            else:
                t.append(steps[i]); coef.append((0.0, h[i])); kind.append(1)
                t.append(steps[i + 1]); coef.append((0.5 * h[i], 0.5 * h[i])); kind.append(0)
        return FlowPlan(steps, h, np.array(t, dtype=np.int64), np.array(coef, dtype=np.float64).reshape(-1, 2),
                        np.array(kind, dtype=np.int32))

    def _plan_tables(self, device, num_steps=50, order=1):
        """_schedule on the device, uploaded once per configuration -> (tau int64 [J], ctab fp32 [J][2], flags int32 [J], the evaluation
        timesteps and the row kinds as host lists).  Row r of the device tables is the evaluation with r more to follow (the layout of
        mapdit_flow_step: the counter runs J - 1 down to 0); the host lists are in execution order."""
        device = torch.device(device)
        key = ("plan", int(num_steps), int(order), device)
        tabs = self._tab_cache.get(key)
        if tabs is None:
            plan = self._schedule(num_steps, order)
            tabs = (torch.from_numpy(plan.t[::-1].copy()).to(device).contiguous(),
                    torch.from_numpy(plan.coef[::-1].copy()).float().to(device).contiguous(),
                    torch.from_numpy(plan.kind[::-1].copy()).to(device).contiguous(),
                    [int(v) for v in plan.t], [int(v) for v in plan.kind])
            self._tab_cache[key] = tabs
        return tabs

    @staticmethod
    def _prep(x):
        # an explicit raise, not an assert: under python -O an assert vanishes and a host pointer would reach a kernel
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            where = f"a tensor on {x.device}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise NotImplementedError(f"the flow kernels run on the MI355X only (no CPU path); got {where}")
        return x.contiguous().float()

    @staticmethod
    def _groups(model_output, x):
        B, C = x.shape[:2]
        if model_output.shape not in ((B, C, *x.shape[2:]), (B, 2 * C, *x.shape[2:])):
            raise ValueError(f"the model output must have C = {C} or 2C channels of x's shape {tuple(x.shape)}; got {tuple(model_output.shape)}")
        return model_output.shape[1] // C

    # ---- forward process --------------------------------------------------------------------------------------------------
    def q_sample(self, x_start, t, noise=None):
        """x_s = (1 - s_t) x_start + s_t noise."""
        x_start = self._prep(x_start)
        if noise is None:
            noise = torch.randn_like(x_start)
        assert noise.shape == x_start.shape
        noise = self._prep(noise)
        t = t.to(device=x_start.device, dtype=torch.int64).contiguous()
        assert t.shape == (x_start.shape[0],)
        out = torch.empty_like(x_start)
        with torch.cuda.device(x_start.device):
            L.lib().flow_q_sample(x_start.data_ptr(), noise.data_ptr(), t.data_ptr(), self._tables(x_start.device).data_ptr(),
                                  self.num_timesteps, out.data_ptr(), x_start.shape[0], x_start[0].numel(), L.cur_stream())
        return out

    def pred_xstart_from_velocity(self, x_t, t, v):
        """x_t - s_t v."""
        x_t, v = self._prep(x_t), self._prep(v)
        assert x_t.shape == v.shape
        t = t.to(device=x_t.device, dtype=torch.int64)
        return x_t - self._tables(x_t.device)[t].view((-1,) + (1,) * (x_t.dim() - 1)) * v

    # ---- training ---------------------------------------------------------------------------------------------------------
    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None):
        """-> {"loss", "mse"}, each [N]: mean_flat((v_pred - (noise - x_start))^2), differentiable with respect to the model output.
        Three launches besides the model: mapdit_flow_q_sample, mapdit_flow_loss_fwd and, in backward, mapdit_obj_loss_bwd."""
        if model_kwargs is None:
            model_kwargs = {}
        x_start = self._prep(x_start)
        if noise is None:
            noise = torch.randn_like(x_start)
        noise = self._prep(noise)
        t = t.to(device=x_start.device, dtype=torch.int64).contiguous()
        x_t = self.q_sample(x_start, t, noise=noise)
        model_output = model(x_t, t, **model_kwargs)
        self._groups(model_output, x_t)
        loss = _FlowLossFunction.apply(model_output, x_start, noise)
        return {"loss": loss, "mse": loss}

    def sample_timesteps(self, n, device, density="uniform", loc=0.0, scale=1.0, generator=None):
        """int64 [n] timestep indices on `device`.  "uniform": torch.randint.  "logit-normal" (SD3): z = torch.randn(n, float64) mapped on
        the device to min(floor(sigmoid(loc + scale z) T), T - 1).  The caller owns the RNG: `generator` is a generator of `device`
        (None: the device's default generator)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError(f"the flow kernels run on the MI355X only (no CPU path); got a tensor on {device}")
        if density == "uniform":
            return torch.randint(0, self.num_timesteps, (int(n),), device=device, generator=generator)
        if density != "logit-normal":
            raise ValueError(f'density must be "uniform" or "logit-normal"; got {density!r}')
        return self.timesteps_from_normals(torch.randn(int(n), dtype=torch.float64, device=device, generator=generator), loc, scale)

    def timesteps_from_normals(self, z, loc=0.0, scale=1.0):
        """The logit-normal map for given standard normal draws z [n] (fp64, on the GPU): mapdit_flow_draw_timesteps."""
        z = self._prep_f64(z)
        t = torch.empty(z.numel(), dtype=torch.int64, device=z.device)
        with torch.cuda.device(z.device):
            L.lib().flow_draw_timesteps(z.data_ptr(), float(loc), float(scale), self.num_timesteps, t.data_ptr(), z.numel(), L.cur_stream())
        return t

    @staticmethod
    def _prep_f64(z):
        if not (isinstance(z, torch.Tensor) and z.is_cuda):
            where = f"a tensor on {z.device}" if isinstance(z, torch.Tensor) else type(z).__name__
            raise NotImplementedError(f"the flow kernels run on the MI355X only (no CPU path); got {where}")
        return z.detach().to(torch.float64).contiguous().view(-1)

    # ---- sampling: the probability-flow ODE from s = 1 to s = 0 --------------------------------------------------------------
    def _flow_step(self, model_output, x_eval, base, hist, step, tabs, sample=None, base_out=None, want_xstart=True):
        """mapdit_flow_step -> (sample, pred_xstart); hist is written on a predictor row.  sample: the tensor to write (may be base on
        a committing row)."""
        tau, ctab, flags = tabs[:3]
        mo = self._prep(model_output)
        groups = self._groups(mo, base)
        sample = torch.empty_like(base) if sample is None else sample
        xstart = torch.empty_like(base) if want_xstart else None
        with torch.cuda.device(base.device):
            L.lib().flow_step(mo.data_ptr(), L.ptr(x_eval), base.data_ptr(), hist.data_ptr(), step.data_ptr(), tau.data_ptr(), ctab.data_ptr(),
                              flags.data_ptr(), tau.shape[0], self._tables(base.device).data_ptr(), self.num_timesteps, sample.data_ptr(),
                              L.ptr(base_out), L.ptr(xstart), base.shape[0], base[0].numel(), groups, L.cur_stream())
        return sample, xstart

    def sample_loop(self, model, shape, noise=None, model_kwargs=None, device=None, progress=False, num_steps=50, order=1, rng=None,
                    index=None):
        """Deterministic sampling along the flow ODE: order 1 Euler (one model evaluation per step), order 2 Heun (2 K' - 1 for K' steps),
        on at most ``num_steps`` steps of the timestep grid (``_schedule``).  ``model(x, t, **model_kwargs)`` returns the velocity on its
        first C channels.  rng= (a SampleRNG) with index= (the rows' sample indices): the start, where noise is None, is the rng's latents
        of those indices; the solver draws nothing else."""
        final = None
        for sample in self.sample_loop_progressive(model, shape, noise=noise, model_kwargs=model_kwargs, device=device, progress=progress,
                                                   num_steps=num_steps, order=order, rng=rng, index=index):
            final = sample
        with torch.cuda.device(final["sample"].device):
            L.lib().device_error_poll(L.cur_stream())      # out-of-range label / timestep / evaluation index anywhere in the loop
        return final["sample"]

    def sample_loop_progressive(self, model, shape, noise=None, model_kwargs=None, device=None, progress=False, num_steps=50, order=1,
                                rng=None, index=None):
        """Yields {"sample", "pred_xstart", "committed"} per model evaluation; after the model an evaluation is one mapdit_flow_step
        launch.  "sample" is the next evaluation point: the solver's state where "committed" is true, Heun's Euler predictor where it
        is false.  "pred_xstart" = x - s v at the evaluation point."""
        from ..sample_rng import pair, rows_index
        rng, index = pair(rng, index)
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        tabs = self._plan_tables(torch.device(device), num_steps, order)
        ts, kinds = tabs[3], tabs[4]
        J = len(ts)
        if noise is None and rng is not None:
            noise = rng.latents(rows_index(index, shape[0]), tuple(shape[1:]))
        img = self._prep(noise if noise is not None else torch.randn(*shape, device=device))
        assert tuple(img.shape) == tuple(shape), (tuple(img.shape), tuple(shape))
        base = img
        hist = torch.empty_like(img)           # written by a predictor row before the corrector row reads it
        indices = list(range(J))
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for j in indices:
            step = torch.full((shape[0],), J - 1 - j, device=device, dtype=torch.int64)
            t = torch.full((shape[0],), ts[j], device=device, dtype=torch.int64)
            with torch.no_grad():
                model_output = model(img, t, **(model_kwargs or {}))
                sample, xstart = self._flow_step(model_output, img, base, hist, step, tabs)
                yield {"sample": sample, "pred_xstart": xstart, "committed": kinds[j] == 0}
                img = sample
                if kinds[j] == 0:
                    base = sample


def create_flow(num_timesteps=1000, shift=1.0):
    return RectifiedFlow(num_timesteps=num_timesteps, shift=shift)


__all__ = ["create_flow", "RectifiedFlow", "FlowPlan", "shifted"]
