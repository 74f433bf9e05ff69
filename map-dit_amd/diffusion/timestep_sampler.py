"""Timestep samplers with the reference's names and signatures (diffusion/timestep_sampler.py), on the device.

    sampler = create_named_schedule_sampler("loss-second-moment", diffusion)
    t, w = sampler.sample(n, device)
    losses = diffusion.training_losses(model, x, t, dict(y=y))
    sampler.update_with_local_losses(t, losses["loss"].detach())
    loss = (losses["loss"] * w).mean()

The reference keeps the loss history in host numpy, reads every timestep and every loss back with ``.item()`` (2 x batch read-backs
per step and rank), gathers three times with a host round trip in between, needs an initialised process group and ``np.int``.  Here
the history, the probability table, the draw and the history update are HIP kernels (csrc/timestep_sampler.hip) on state that lives
on the device: nothing in ``sample()`` or in either update method reads anything back, so the calls queue behind the step like every
other launch of the training loop.

Differences from the reference, all deliberate:
  * ``sample(batch_size, device, generator=None)`` draws its uniforms with ``torch.rand(..., dtype=float64, generator=generator)``: the
    caller owns the RNG, as it does for the noise (the reference draws from numpy's global generator).  ``sample_from_uniforms(u)`` is
    the draw for given uniforms: ``searchsorted(cumsum(p) / cumsum(p)[-1], u, side="right")``, which is what ``np.random.choice(p=p)``
    computes from ``random_sample``.  There is no CPU path.
  * A history entry whose timestep lies outside [0, T) is skipped and reported by ``mapdit_device_error_poll`` (train.py polls at logging
    cadence); the reference indexes numpy with it.
  * A history entry whose loss is inf or NaN is skipped: an fp16 step that overflowed is refused by the optimiser guard and must not
    poison H draws' worth of history (the reference stores it and ``weights()`` turns NaN).
  * A warmed-up history whose weights sum to zero (or to a non-finite value) gives the uniform table; the reference divides by the sum.
  * ``update_with_local_losses`` works without a process group (it is ``update_with_all_losses`` then) and assumes EQUAL local batch
    sizes on every rank (train.py's splits guarantee it): one gather of the timesteps and one of the losses, no size exchange.
"""
from abc import ABC, abstractmethod

import numpy as np
import torch
import torch.distributed as dist

from .. import _lib as L
from .. import parallel


def create_named_schedule_sampler(name, diffusion):
    """
    Create a ScheduleSampler from a library of pre-defined samplers.
    :param name: the name of the sampler.
    :param diffusion: the diffusion object to sample for.
    """
    if name == "uniform":
        return UniformSampler(diffusion)
    elif name == "loss-second-moment":
        return LossSecondMomentResampler(diffusion)
    else:
        raise NotImplementedError(f"unknown schedule sampler: {name}")


def _cuda(device):
    """The device of a draw; a CPU device is refused in the words of GaussianDiffusion._prep."""
    device = torch.device(device)
    if device.type != "cuda":
        raise NotImplementedError(f"the diffusion kernels run on the MI355X only (no CPU path); got a tensor on {device}")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


class ScheduleSampler(ABC):
    """
    A distribution over timesteps in the diffusion process, intended to reduce variance of the objective.
    By default, samplers perform unbiased importance sampling, in which the objective's mean is unchanged.
    """

    @abstractmethod
    def weights(self):
        """
        Get a numpy array of weights, one per diffusion step.
        The weights needn't be normalized, but must be positive (a weight that is not positive and finite is reported by
        ``mapdit_device_error_poll``; the draw then falls back to the uniform table).
        """

    def _table(self, device):
        """(prob, cdf) fp64 [T] on `device`.  The generic path: a subclass's host ``weights()`` is uploaded at every draw."""
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(self.weights(), dtype=np.float64))).to(device)
        prob, cdf = torch.empty_like(w), torch.empty_like(w)
        with torch.cuda.device(device):
            L.lib().tsampler_prepare_weights(L.ptr(w), w.numel(), L.ptr(prob), L.ptr(cdf), L.cur_stream())
        return prob, cdf

    def sample(self, batch_size, device, generator=None):
        """
        Importance-sample timesteps for a batch.
        :param batch_size: the number of timesteps.
        :param device: the torch device to save to (a GPU: there is no CPU path).
        :param generator: the torch generator of `device` the uniforms are drawn from (None: the device's default generator).
        :return: a tuple (timesteps, weights):
                 - timesteps: an int64 tensor of timestep indices.
                 - weights: an fp32 tensor of weights to scale the resulting losses.
        """
        device = _cuda(device)
        return self.sample_from_uniforms(torch.rand(int(batch_size), dtype=torch.float64, device=device, generator=generator))

    def sample_from_uniforms(self, u):
        """The draw for given uniforms u [N] (fp64, in [0, 1), on the GPU): t = searchsorted(cdf, u, side="right"), w = 1 / (T p[t])."""
        if not isinstance(u, torch.Tensor):
            raise NotImplementedError(f"the diffusion kernels run on the MI355X only (no CPU path); got {type(u).__name__}")
        device = _cuda(u.device)
        u = u.detach().to(torch.float64).contiguous().view(-1)
        prob, cdf = self._table(device)
        t = torch.empty(u.numel(), dtype=torch.int64, device=device)
        w = torch.empty(u.numel(), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            L.lib().tsampler_draw(L.ptr(prob), L.ptr(cdf), prob.numel(), L.ptr(u), L.ptr(t), L.ptr(w), u.numel(), L.cur_stream())
        return t, w


class UniformSampler(ScheduleSampler):
    def __init__(self, diffusion):
        self.diffusion = diffusion
        self._weights = np.ones([diffusion.num_timesteps])
        self._tables = {}

    def weights(self):
        return self._weights

    def _table(self, device):          # constant weights: one upload per device
        if device not in self._tables:
            self._tables[device] = super()._table(device)
        return self._tables[device]


class LossAwareSampler(ScheduleSampler):
    def update_with_local_losses(self, local_ts, local_losses):
        """
        Update the reweighting using losses from a model.
        Call this method from each rank with a batch of timesteps and the corresponding losses for each of those timesteps: every
        rank then applies the same entries in the same order (rank 0's, then rank 1's, ...) and holds the same history bits.
        Without an initialised process group, or in a group of one, this is update_with_all_losses.  The local batches must have the
        SAME size on every rank (no size exchange per step).  Over RCCL the two gathers are ordered on the compute stream and nothing
        is read back; under a host-staged gloo group (one-GPU rehearsals) they go through the host.
        :param local_ts: an integer Tensor of timesteps.
        :param local_losses: a 1D Tensor of losses.
        """
        world = parallel._world(None)
        if world == 1:
            return self.update_with_all_losses(local_ts, local_losses)
        ts = local_ts.detach().to(torch.int64).contiguous().view(-1)
        losses = local_losses.detach().to(torch.float32).contiguous().view(-1)
        if parallel._host_staged(None, ts):
            gathered = []
            for x in (ts, losses):
                parts = [torch.empty(x.numel(), dtype=x.dtype) for _ in range(world)]
                dist.all_gather(parts, x.cpu())
                gathered.append(torch.cat(parts).to(ts.device))
            all_ts, all_losses = gathered
        else:
            all_ts = torch.empty(world * ts.numel(), dtype=ts.dtype, device=ts.device)
            all_losses = torch.empty(world * losses.numel(), dtype=losses.dtype, device=losses.device)
            dist.all_gather_into_tensor(all_ts, ts)
            dist.all_gather_into_tensor(all_losses, losses)
        self.update_with_all_losses(all_ts, all_losses)

    @abstractmethod
    def update_with_all_losses(self, ts, losses):
        """
        Update the reweighting using losses from a model.
        This method directly updates the reweighting without synchronizing between workers. It is called by
        update_with_local_losses from all ranks with identical arguments.
        :param ts: timesteps: an integer tensor on the GPU, or a list of ints (uploaded).
        :param losses: losses, one per timestep: a tensor on the GPU, or a list of floats (uploaded).
        """


class LossSecondMomentResampler(LossAwareSampler):
    """p(t) proportional to sqrt(E[loss_t^2]) over the last `history_per_term` losses of each timestep, mixed with `uniform_prob` of
    the uniform distribution; uniform until every timestep has a full history (improved-DDPM's resampler for variational-bound losses).

    The history [T, H] fp64, the counts, the probability table and its cdf live on the device of the first tensors the object sees
    (until then - and for state_dict() / load_state_dict() on a host without a GPU - in host tensors of the same layout).  An update
    marks the table dirty; the next sample() rebuilds it (mapdit_tsampler_prepare) before it draws."""

    def __init__(self, diffusion, history_per_term=10, uniform_prob=0.001):
        self.diffusion = diffusion
        self.history_per_term = int(history_per_term)
        self.uniform_prob = float(uniform_prob)
        T, H = int(diffusion.num_timesteps), self.history_per_term
        if not (1 <= T <= 16384 and 1 <= H <= 64):
            raise ValueError(f"LossSecondMomentResampler: built for 1 <= num_timesteps <= 16384 and 1 <= history_per_term <= 64, got {T}, {H}")
        if not 0.0 <= self.uniform_prob <= 1.0:
            raise ValueError(f"LossSecondMomentResampler: uniform_prob must lie in [0, 1], got {uniform_prob}")
        self._T = T
        self._host = None                              # (hist, counts) loaded before a device is known; None = the empty history
        self._hist = self._counts = self._prob = self._cdf = None
        self._dirty = True

    # ---- state ----------------------------------------------------------------------------------------------------------------------
    @property
    def device(self):
        return None if self._hist is None else self._hist.device

    def _ensure(self, device):
        if self._hist is None:
            if self._host is None:                     # (no upload: nothing of a fresh sampler's first draw waits for the host)
                self._hist = torch.zeros(self._T, self.history_per_term, dtype=torch.float64, device=device)
                self._counts = torch.zeros(self._T, dtype=torch.int32, device=device)
            else:
                self._hist, self._counts = self._host[0].to(device), self._host[1].to(device)
            self._prob = torch.empty(self._T, dtype=torch.float64, device=device)
            self._cdf = torch.empty(self._T, dtype=torch.float64, device=device)
            self._host, self._dirty = None, True
        elif self._hist.device != device:
            raise ValueError(f"LossSecondMomentResampler: its state lives on {self._hist.device}, got a tensor on {device}")

    def _table(self, device):
        self._ensure(device)
        if self._dirty:
            with torch.cuda.device(device):
                L.lib().tsampler_prepare(L.ptr(self._hist), L.ptr(self._counts), self._T, self.history_per_term, self.uniform_prob,
                                         L.ptr(self._prob), L.ptr(self._cdf), L.cur_stream())
            self._dirty = False
        return self._prob, self._cdf

    def update_with_all_losses(self, ts, losses):
        if isinstance(ts, torch.Tensor) and ts.is_cuda:
            device = ts.device
        elif isinstance(losses, torch.Tensor) and losses.is_cuda:
            device = losses.device
        elif self._hist is not None:
            device = self._hist.device
        else:
            device = _cuda("cuda")                     # lists before any tensor: the current GPU
        device = _cuda(device)
        self._ensure(device)
        ts = torch.as_tensor(ts, dtype=torch.int64).detach().to(device).contiguous().view(-1)
        losses = torch.as_tensor(losses, dtype=torch.float32).detach().to(device).contiguous().view(-1)
        if ts.numel() != losses.numel():
            raise ValueError(f"update_with_all_losses: {ts.numel()} timesteps, {losses.numel()} losses")
        if ts.numel() == 0:
            return
        with torch.cuda.device(device):
            L.lib().tsampler_update(L.ptr(self._hist), L.ptr(self._counts), self._T, self.history_per_term, L.ptr(ts), L.ptr(losses),
                                    ts.numel(), L.cur_stream())
        self._dirty = True

    def weights(self):
        """The reference's vector (timestep_sampler.py:130-137): ones until every timestep has a full history, then the normalised
        mixed probabilities.  SYNCHRONISES (it reads the counts and the table back): for logging cadence, not for the step."""
        if self._hist is None or not self._warmed_up():
            return np.ones([self._T], dtype=np.float64)
        return self._table(self._hist.device)[0].cpu().numpy()

    def _host_state(self):
        if self._hist is not None:
            return self._hist.cpu(), self._counts.cpu()
        if self._host is None:
            return torch.zeros(self._T, self.history_per_term, dtype=torch.float64), torch.zeros(self._T, dtype=torch.int32)
        return self._host

    def _warmed_up(self):
        return bool((self._host_state()[1] == self.history_per_term).all().item())

    def state_dict(self):
        """{"loss_history": float64 [T, H], "loss_counts": int64 [T]} (host tensors in the layout of the reference's _loss_history /
        _loss_counts), "history_per_term", "uniform_prob".  Synchronises."""
        hist, counts = self._host_state()
        return {"loss_history": hist.clone(), "loss_counts": counts.to(torch.int64), "history_per_term": self.history_per_term,
                "uniform_prob": self.uniform_prob}

    def load_state_dict(self, state):
        hist = torch.as_tensor(np.asarray(state["loss_history"]), dtype=torch.float64)
        counts = torch.as_tensor(np.asarray(state["loss_counts"]), dtype=torch.int64)
        T, H = self._T, self.history_per_term
        if tuple(hist.shape) != (T, H) or tuple(counts.shape) != (T,):
            raise ValueError(f"load_state_dict: loss_history {tuple(hist.shape)} / loss_counts {tuple(counts.shape)} do not fit "
                             f"[{T}, {H}] / [{T}]")
        if int(state.get("history_per_term", H)) != H:
            raise ValueError(f"load_state_dict: history_per_term {state['history_per_term']} != {H}")
        if bool(((counts < 0) | (counts > H)).any()):
            raise ValueError(f"load_state_dict: loss_counts outside [0, {H}]")
        if "uniform_prob" in state:
            self.uniform_prob = float(state["uniform_prob"])
        counts = counts.to(torch.int32)
        if self._hist is None:
            self._host = (hist.clone().contiguous(), counts.contiguous())
        else:
            self._hist.copy_(hist)
            self._counts.copy_(counts)
        self._dirty = True
