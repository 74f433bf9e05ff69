"""hipGraph-captured sampling (BASELINE config 5; reference sample_fid.py:48-76 + gaussian_diffusion.py:464-511).

One denoise step of ``p_sample_loop`` — timestep map lookup, the classifier-free-guidance DiT forward, the fused
p_mean_variance / p_sample kernel, the N(0,1) draw and the on-device ``t -= 1`` — is captured once into a hipGraph
(torch.cuda.CUDAGraph is hipGraph on ROCm) and replayed ``num_timesteps`` times.  The reference's per-step host work
(``th.tensor([i]*B)``, ~8 numpy table uploads, the timestep_map upload: SURVEY §3.2) disappears: schedule tables,
the map and the step counter live on the device, and a replay is a single graph launch.

``sampler="dpm++"`` captures one step of ``dpm_solver_sample_loop`` instead (the multistep DPM-Solver++, not in the reference):
the lookup of the solver's timestep, the DiT forward, ``mapdit_dpm_step`` and ``step -= 1``, replayed once per solver step.  The
previous x0 prediction, the step index and the solver's tables live on the device; no randomness is drawn.

``sampler="flow"`` takes a ``flow.RectifiedFlow`` in the diffusion's place and captures one model evaluation of its Euler / Heun loop
(``flow.sample_loop``): the lookup of the evaluation's timestep, the DiT forward, ``mapdit_flow_step`` and ``step -= 1``, replayed once
per evaluation.  The solver's state, Heun's first velocity and the evaluation counter live on the device.
"""
from __future__ import annotations

import torch

from . import _lib as L


class GraphedSampler:
    """Captures ``x_{t-1} = p_sample(model_fn(x_t, map[t], **kw), x_t, t)`` for a fixed batch shape.

    model: the DiT module (eval mode); diffusion: a SpacedDiffusion; cfg_scale: None -> model.forward, else
    model.forward_with_cfg (y must then hold [labels, null labels], as sample_fid.py:56-66 builds it).

    sampler: "ancestral" (p_sample, one replay per timestep of the diffusion) or "dpm++" (DPM-Solver++ with num_steps / order / spacing /
    lower_order_final as ``diffusion.dpm_solver_sample_loop`` takes them; one replay per solver step, ``self.num_replays`` of them), or
    "flow": `diffusion` is a ``flow.RectifiedFlow`` and num_steps / order (1 Euler, 2 Heun) are ``flow.sample_loop``'s; one replay per
    model evaluation.  A RectifiedFlow with another sampler, or "flow" with a GaussianDiffusion, is refused; clip_denoised does not apply.

    rng: a ``sample_rng.SampleRNG``.  The sampler then owns an int64 ``index`` buffer (one sample index per row) and the captured
    ancestral step is ``mapdit_psample_step_counter`` / ``mapdit_obj_step_counter``, in place: the noise of row j at step t is the
    contract's ``noise[index[j]][t]``, generated in the kernel - no generator launch, no copy.  ``sample(index=...)`` copies the indices
    in (a guidance batch takes n of them and both halves carry them) and draws the start from them: the same graph, another aim."""

    def __init__(self, model, diffusion, shape, y, cfg_scale=None, clip_denoised=False, sampler="ancestral", num_steps=20, order=2,
                 spacing="logsnr", lower_order_final=True, rng=None):
        assert not model.training, "sampling runs the model in eval mode"
        if sampler not in ("ancestral", "dpm++", "flow"):
            raise ValueError(f'sampler must be "ancestral", "dpm++" or "flow"; got {sampler!r}')
        from .flow import RectifiedFlow
        if isinstance(diffusion, RectifiedFlow) != (sampler == "flow"):
            raise ValueError(f'sampler="flow" runs a flow.RectifiedFlow and "ancestral" / "dpm++" a GaussianDiffusion; got sampler={sampler!r} '
                             f"with a {type(diffusion).__name__}")
        self.flow = None
        self.rng = rng
        # (index 0 in every row is a valid aim for the warm-up and the capture)
        self.index = None if rng is None else torch.zeros(shape[0], device=next(model.parameters()).device, dtype=torch.int64)
        if sampler == "flow":
            return self._init_flow(model, diffusion, shape, y, cfg_scale, num_steps, order)
        diffusion._supported()
        if diffusion.model_var_type.name != "LEARNED_RANGE":
            raise NotImplementedError(f"GraphedSampler drives a DiT, whose output carries learned-range variance channels; a "
                                      f"{diffusion.model_var_type.name} diffusion needs a model with C output channels "
                                      "(DiT(learn_sigma=False) is not built): use diffusion.p_sample_loop")
        self.model, self.diffusion = model, diffusion
        dev = next(model.parameters()).device
        self.dev = dev
        self.img = torch.zeros(*shape, device=dev)
        self.dpm = None
        if sampler == "dpm++":
            self.dpm = diffusion._dpm_tables(dev, num_steps, order, spacing, lower_order_final)
            self.hist = torch.zeros_like(self.img)
        self.num_replays = diffusion.num_timesteps if self.dpm is None else len(self.dpm[2])
        # the warm-up and the capture below each run one real step (t -> t - 1): start high enough to stay inside the schedule
        # (t is the index into the diffusion's schedule for "ancestral", the solver step index for "dpm++")
        self.t = torch.full((shape[0],), max(self.num_replays - 1, 0), device=dev, dtype=torch.int64)
        self.y = y.to(dev).clone()
        self.cfg_scale, self.clip = cfg_scale, bool(clip_denoised)
        self.tab = diffusion._tables(dev)
        # the default objective replays mapdit_psample_step; x0 prediction (START_X) the generalised mapdit_obj_step
        self.otab = None if diffusion._is_default() else diffusion._obj_tables(dev)
        self.tmap = torch.tensor(diffusion.timestep_map, device=dev, dtype=torch.int64)
        self._capture()

    def _capture(self):
        dev = self.dev
        self.graph = None
        with torch.no_grad():
            # eager warm-up on a side stream (allocates the engine workspace, builds the cached bf16 weight images)
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                for _ in range(2):
                    self.t.fill_(max(self.num_replays - 1, 0))
                    self._step()
            torch.cuda.current_stream(dev).wait_stream(s)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            self.t.fill_(max(self.num_replays - 1, 0))
            with torch.cuda.graph(self.graph):
                self._step()

    def _init_flow(self, model, flow, shape, y, cfg_scale, num_steps, order):
        """The "flow" sampler's buffers and capture: img is the evaluation point (and what sample() returns), base the solver's state
        (Euler: img itself), hist Heun's first velocity, t the evaluation counter (J - 1 down to 0)."""
        self.model, self.diffusion = model, flow
        dev = next(model.parameters()).device
        self.dev = dev
        self.dpm = None
        self.flow = flow._plan_tables(dev, num_steps, order)
        self.num_replays = len(self.flow[3])
        self.img = torch.zeros(*shape, device=dev)
        self.base = self.img if order == 1 else torch.zeros_like(self.img)
        self.hist = torch.zeros_like(self.img)
        self.t = torch.full((shape[0],), self.num_replays - 1, device=dev, dtype=torch.int64)
        self.y = y.to(dev).clone()
        self.cfg_scale, self.clip = cfg_scale, False
        self.tab = flow._tables(dev)
        self._capture()

    def _flow_step(self):
        f = self.diffusion
        tau, ctab, flags = self.flow[:3]
        t = tau[self.t.clamp(0, self.num_replays - 1)]
        if self.cfg_scale is None:
            out = self.model.forward(self.img, t, self.y)
        else:
            out = self.model.forward_with_cfg(self.img, t, self.y, self.cfg_scale)
        out = out.contiguous().float()
        # in place: the evaluation point is overwritten by the next one; Heun keeps the state in base (written on committing rows)
        heun = self.base is not self.img
        L.lib().flow_step(out.data_ptr(), None, self.base.data_ptr(), self.hist.data_ptr(), self.t.data_ptr(), tau.data_ptr(), ctab.data_ptr(),
                          flags.data_ptr(), self.num_replays, self.tab.data_ptr(), f.num_timesteps, self.img.data_ptr(),
                          self.base.data_ptr() if heun else None, None, self.img.shape[0], self.img[0].numel(),
                          out[0].numel() // self.img[0].numel(), L.cur_stream())
        self.t.sub_(1)

    def _step(self):
        d = self.diffusion
        if self.flow is not None:
            return self._flow_step()
        if self.dpm is not None:
            return self._dpm_step()
        mapped = self.tmap[self.t.clamp_min(0)]
        if self.cfg_scale is None:
            out = self.model.forward(self.img, mapped, self.y)
        else:
            out = self.model.forward_with_cfg(self.img, mapped, self.y, self.cfg_scale)
        if self.rng is not None:          # in place: the counter kernels' sample may alias x
            if self.otab is None:
                L.lib().psample_step_counter(out.data_ptr(), self.img.data_ptr(), self.rng.seed, self.index.data_ptr(), self.t.data_ptr(),
                                             self.tab.data_ptr(), d.num_timesteps, int(self.clip), self.img.data_ptr(), None,
                                             self.img.shape[0], self.img[0].numel(), L.cur_stream())
            else:
                mean_type, var_type, _ = d._kinds()
                L.lib().obj_step_counter(out.data_ptr(), self.img.data_ptr(), self.rng.seed, self.index.data_ptr(), self.t.data_ptr(),
                                         self.tab.data_ptr(), self.otab.data_ptr(), d.num_timesteps, mean_type, var_type, int(self.clip),
                                         0, 0.0, self.img.data_ptr(), None, self.img.shape[0], self.img[0].numel(), L.cur_stream())
            self.t.sub_(1)
            return
        noise = torch.randn_like(self.img)
        nxt = torch.empty_like(self.img)
        if self.otab is None:
            L.lib().psample_step(out.data_ptr(), self.img.data_ptr(), noise.data_ptr(), self.t.data_ptr(), self.tab.data_ptr(),
                                 d.num_timesteps, int(self.clip), nxt.data_ptr(), None, self.img.shape[0], self.img[0].numel(),
                                 L.cur_stream())
        else:
            mean_type, var_type, _ = d._kinds()
            L.lib().obj_step(out.data_ptr(), self.img.data_ptr(), noise.data_ptr(), self.t.data_ptr(), self.tab.data_ptr(),
                             self.otab.data_ptr(), d.num_timesteps, mean_type, var_type, int(self.clip), 0, 0.0, nxt.data_ptr(), None,
                             self.img.shape[0], self.img[0].numel(), L.cur_stream())
        self.img.copy_(nxt)
        self.t.sub_(1)

    def _dpm_step(self):
        d = self.diffusion
        tau, ctab, taus = self.dpm
        mapped = self.tmap[tau[self.t.clamp(0, len(taus) - 1)]]
        if self.cfg_scale is None:
            out = self.model.forward(self.img, mapped, self.y)
        else:
            out = self.model.forward_with_cfg(self.img, mapped, self.y, self.cfg_scale)
        mean_type, var_type, _ = d._kinds()
        # in place: the kernel's sample may alias x
        L.lib().dpm_step(out.data_ptr(), self.img.data_ptr(), self.hist.data_ptr(), self.t.data_ptr(), ctab.data_ptr(), tau.data_ptr(),
                         len(taus), self.tab.data_ptr(), d.num_timesteps, mean_type, var_type, int(self.clip), None, self.img.data_ptr(),
                         None, self.img.shape[0], self.img[0].numel(), L.cur_stream())
        self.t.sub_(1)

    def refresh_weights(self):
        """After the model's parameters were replaced in place (``load_state_dict``): rebuild the cached weight images
        the captured graph reads (the eager forward does this lazily; a graph replay runs no Python)."""
        rt = self.model._runtime(self.img.shape[0], train=False)
        with torch.cuda.device(self.dev):
            rt.lib.engine_prepare_weights(rt.handle, 0, L.cur_stream())
        rt.weights_key = self.model._weights_key()

    @torch.no_grad()
    def sample(self, noise=None, steps=None, index=None):
        """Run the reverse chain from ``noise`` (or fresh N(0,1)); ``steps`` bounds the prefix (default: all).  A sampler built with an
        rng needs ``index`` (one sample index per row, or per row of one half of a guidance batch) and draws the start from it unless
        ``noise`` is given; without an rng an index is refused."""
        if (index is None) != (self.rng is None):
            raise ValueError("sample(index=...) needs a GraphedSampler built with rng=, and one built with rng= needs index=: "
                             f"got index={'None' if index is None else 'given'}, rng={'None' if self.rng is None else 'given'}")
        if self.rng is not None:                                          # checked here, outside the capture: the kernels read the low 32 bits
            from .sample_rng import rows_index
            self.index.copy_(rows_index(self.rng.check_index(index), self.img.shape[0]))
            if noise is None:
                noise = self.rng.latents(self.index, tuple(self.img.shape[1:]))
        n = self.num_replays
        if self.dpm is not None:
            self.hist.zero_()
        steps = n if steps is None else steps
        if noise is None:
            self.img.normal_()
        else:
            self.img.copy_(noise)
        if self.flow is not None and self.base is not self.img:
            self.base.copy_(self.img)
        self.t.fill_(n - 1)
        for _ in range(steps):
            self.graph.replay()
        out = self.img.clone()
        self.model.check_device_errors()      # a label outside the embedding table (e.g. a null label the model has no row for)
        return out


def p_sample_loop_graphed(diffusion, model, shape, noise=None, clip_denoised=False, model_kwargs=None, device=None, *,
                          denoised_fn=None, cond_fn=None):
    """Drop-in for ``diffusion.p_sample_loop(model.forward[_with_cfg], shape, noise, clip_denoised, model_kwargs=...)``
    with the loop body replayed from a hipGraph.  ``model`` is the DiT module itself.  The sampler hooks are user callables, which
    a captured graph cannot hold: they are refused here and run through ``diffusion.p_sample_loop``."""
    if denoised_fn is not None or cond_fn is not None:
        raise NotImplementedError("denoised_fn / cond_fn are not built for the captured sampler (a user callable cannot run inside "
                                  "a hipGraph): use diffusion.p_sample_loop")
    kw = dict(model_kwargs or {})
    y = kw.pop("y")
    cfg = kw.pop("cfg_scale", None)
    assert not kw, f"unsupported model_kwargs: {sorted(kw)}"
    return GraphedSampler(model, diffusion, shape, y, cfg, clip_denoised).sample(noise)


def dpm_solver_sample_loop_graphed(diffusion, model, shape, noise=None, clip_denoised=False, model_kwargs=None, device=None, *,
                                   denoised_fn=None, cond_fn=None, num_steps=20, order=2, spacing="logsnr", lower_order_final=True):
    """Drop-in for ``diffusion.dpm_solver_sample_loop(model.forward[_with_cfg], shape, noise, clip_denoised, model_kwargs=...,
    num_steps=..., order=..., spacing=...)`` with the solver step replayed from a hipGraph.  ``model`` is the DiT module itself; the
    hooks are refused as ``p_sample_loop_graphed`` refuses them and run through ``diffusion.dpm_solver_sample_loop``."""
    if denoised_fn is not None or cond_fn is not None:
        raise NotImplementedError("denoised_fn / cond_fn are not built for the captured sampler (a user callable cannot run inside "
                                  "a hipGraph): use diffusion.dpm_solver_sample_loop")
    kw = dict(model_kwargs or {})
    y = kw.pop("y")
    cfg = kw.pop("cfg_scale", None)
    assert not kw, f"unsupported model_kwargs: {sorted(kw)}"
    return GraphedSampler(model, diffusion, shape, y, cfg, clip_denoised, sampler="dpm++", num_steps=num_steps, order=order,
                          spacing=spacing, lower_order_final=lower_order_final).sample(noise)


def flow_sample_loop_graphed(flow, model, shape, noise=None, model_kwargs=None, device=None, *, num_steps=50, order=1):
    """Drop-in for ``flow.sample_loop(model.forward[_with_cfg], shape, noise, model_kwargs=..., num_steps=..., order=...)`` with the model
    evaluation and its mapdit_flow_step replayed from a hipGraph.  ``model`` is the DiT module itself."""
    kw = dict(model_kwargs or {})
    y = kw.pop("y")
    cfg = kw.pop("cfg_scale", None)
    assert not kw, f"unsupported model_kwargs: {sorted(kw)}"
    return GraphedSampler(model, flow, shape, y, cfg, sampler="flow", num_steps=num_steps, order=order).sample(noise)


# ---- shared pieces of the sampler CLIs (reference sample.py / sample_fid.py / sample_ema.py) ---------------------------

def str2bool(v) -> bool:
    """argparse type for the reference's ``--use-vae`` style switches (the reference uses ``type=bool``, under which any
    non-empty string - including "False" - is true; here "false"/"0"/"no" mean false)."""
    if isinstance(v, bool):
        return v
    return str(v).strip().lower() not in ("false", "0", "no", "off", "")


def load_train_args(result_dir: str) -> dict:
    """config.yaml written by the training harness (reference train.py:35-40; sample.py:20-24)."""
    import os

    import yaml
    with open(os.path.join(result_dir, "config.yaml"), "r") as f:
        return yaml.safe_load(f)


def load_weights(model, result_dir: str, ema_std: float = 0.05, ckpt: str | None = None, verbose: bool = True):
    """EMA weights reconstructed post hoc from ``<result_dir>/ema`` (default), or a raw checkpoint's ``model`` entry
    when ``ckpt`` names one (without .pt) - reference sample.py:29-37."""
    import os

    from .src.ema import calculate_posthoc_ema
    if ckpt is not None:
        sd = torch.load(os.path.join(result_dir, "checkpoints", f"{ckpt}.pt"), map_location="cpu", weights_only=True)["model"]
    else:
        sd = calculate_posthoc_ema(ema_std, os.path.join(result_dir, "ema"), verbose=verbose)
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    model.eval()
    return model


def denormalize(samples: torch.Tensor, train_args: dict) -> torch.Tensor:
    """Undo the per-channel standardisation of the training latents (reference sample.py:66-69)."""
    mean = torch.tensor(train_args["stats_mean"], device=samples.device).reshape(1, -1, 1, 1)
    std = torch.tensor(train_args["stats_std"], device=samples.device).reshape(1, -1, 1, 1)
    return samples * std + mean


def add_vae_flags(parser):
    """The native decoder's flags, shared by the three CLIs (``load_vae``)."""
    parser.add_argument("--vae-weights", type=str, default=None,
                        help="AutoencoderKL weights (.safetensors, or a torch state dict): decode with the native HIP decoder")
    parser.add_argument("--vae-precision", choices=["f16", "bf16"], default="f16", help="16-bit operand format of the native decoder")
    parser.add_argument("--vae-norm-groups", type=int, default=32, help="norm_num_groups of the VAE config (not recoverable from the weights)")
    return parser


def check_vae_flags(args):
    """Before anything is built: a ``--vae-weights`` that names no file ends the run here, not after sampling."""
    import os
    if getattr(args, "vae_weights", None) and not os.path.isfile(args.vae_weights):
        raise FileNotFoundError(f"--vae-weights {args.vae_weights}: no such file")


def load_vae(vae_path: str | None, device, weights: str | None = None, precision: str = "f16", norm_groups: int = 32):
    """The reference decodes latents with diffusers' AutoencoderKL("stabilityai/sd-vae-ft-mse") fetched from the hub
    (sample.py:72-74).  ``weights`` (``--vae-weights``): the native decoder (map-dit_amd/vae.py) on that weight file - no package,
    no network.  Without it: the ``diffusers`` package on a local copy (``--vae-path``), as before."""
    if weights is not None:
        from .vae import VAEDecoder
        return VAEDecoder.from_file(weights, device, precision=precision, norm_num_groups=norm_groups)
    try:
        from diffusers import AutoencoderKL
    except ImportError as e:
        raise RuntimeError("--use-vae needs the `diffusers` package and a local copy of stabilityai/sd-vae-ft-mse "
                           "(--vae-path); pass `--use-vae false` to write the latents instead") from e
    return AutoencoderKL.from_pretrained(vae_path or "stabilityai/sd-vae-ft-mse").to(device)


SAMPLERS = ("ancestral", "dpm++", "flow-euler", "flow-heun")
FLOW_SAMPLERS = {"flow-euler": 1, "flow-heun": 2}          # -> the order of flow.sample_loop


def add_sampler_flags(parser):
    """The sampler choice shared by the three CLIs.  Under ``dpm++`` ``--num-sampling-steps`` is the solver's num_steps and the
    diffusion is the full schedule, which the solver subsamples itself (``make_diffusion``); under ``flow-euler`` / ``flow-heun`` (a
    run trained with ``--objective flow``) it is the num_steps of ``flow.sample_loop``."""
    parser.add_argument("--sampler", choices=SAMPLERS, default="ancestral",
                        help="ancestral: the reference's p_sample_loop; dpm++: DPM-Solver++ (deterministic, ~20 steps); flow-euler / "
                             "flow-heun: the ODE sampler of a run trained with --objective flow")
    parser.add_argument("--solver-order", type=int, choices=[1, 2], default=2, help="dpm++ only: 1 (DDIM) or 2 (2M)")
    parser.add_argument("--solver-spacing", choices=["logsnr", "uniform"], default="logsnr", help="dpm++ only: how its steps are chosen")
    parser.add_argument("--sample-rng", choices=["torch", "counter"], default="torch",
                        help="torch: every draw from the global torch generator, as the reference; counter: sample i's latent, label and "
                             "step noise are a function of (--seed, i) alone (sample_rng.SampleRNG) - what sample_fid.py's parts, "
                             "shards and resuming rest on")
    return parser


def make_rng(args, device):
    """The SampleRNG of ``--sample-rng counter`` (keyed by ``--seed``), or None."""
    if getattr(args, "sample_rng", "torch") != "counter":
        return None
    if args.seed is None:
        raise ValueError("--sample-rng counter needs a --seed: the seed is the generator's key")
    from .sample_rng import SampleRNG
    return SampleRNG(args.seed, device)


def check_objective(sampler: str, train_args: dict | None):
    """A run directory's objective (config.yaml: "diffusion" where the key is missing, as every run before the key existed) against
    the sampler asked for: a velocity model means nothing to the diffusion samplers, and the reverse."""
    objective = (train_args or {}).get("objective", "diffusion")
    if objective == "flow" and sampler not in FLOW_SAMPLERS:
        raise ValueError(f"this run was trained with --objective flow: its model predicts a velocity, which --sampler {sampler} cannot read; "
                         "pass --sampler flow-euler or --sampler flow-heun")
    if objective != "flow" and sampler in FLOW_SAMPLERS:
        raise ValueError(f"this run was trained with --objective {objective}: its model predicts eps, which --sampler {sampler} cannot read; "
                         "pass --sampler ancestral or --sampler dpm++")


def make_diffusion(args, train_args: dict | None = None):
    """create_diffusion (or create_flow) for a CLI's arguments and the GraphedSampler / run_sampler keywords that select its sampler.
    train_args: the run's config.yaml, whose objective must fit the sampler (check_objective)."""
    from .diffusion import create_diffusion
    check_objective(args.sampler, train_args)
    if args.sampler in FLOW_SAMPLERS:
        from .flow import create_flow
        return (create_flow(shift=float((train_args or {}).get("flow_shift", 1.0))),
                dict(sampler="flow", num_steps=args.num_sampling_steps, order=FLOW_SAMPLERS[args.sampler]))
    if args.sampler == "dpm++":
        return create_diffusion(""), dict(sampler="dpm++", num_steps=args.num_sampling_steps, order=args.solver_order,
                                          spacing=args.solver_spacing)
    return create_diffusion(str(args.num_sampling_steps)), {}


def run_sampler(model, diffusion, z, y, cfg_scale, use_graph: bool = True, progress: bool = False, sampler: str = "ancestral",
                num_steps: int = 20, order: int = 2, spacing: str = "logsnr", rng=None, index=None):
    """``diffusion.p_sample_loop(model.forward[_with_cfg], z.shape, z, clip_denoised=False, ...)`` - through the captured
    hipGraph (default) or the eager loop; with ``sampler="dpm++"``, ``diffusion.dpm_solver_sample_loop`` (num_steps, order,
    spacing) the same two ways; with ``sampler="flow"`` (or the CLI names "flow-euler" / "flow-heun", which fix the order), `diffusion`
    is a RectifiedFlow and the loop is its ``sample_loop(num_steps=, order=1 | 2)``.  rng= / index= (together): the step noise is the
    SampleRNG's for those sample indices; z stays the start."""
    from .sample_rng import pair
    pair(rng, index)
    ctr = {} if rng is None else dict(rng=rng, index=index)
    idx = {} if rng is None else dict(index=index)
    if sampler not in SAMPLERS + ("flow",):
        raise ValueError(f"sampler must be one of {SAMPLERS + ('flow',)}; got {sampler!r}")
    if sampler == "flow" or sampler in FLOW_SAMPLERS:
        order = FLOW_SAMPLERS.get(sampler, order)
        if use_graph:
            return GraphedSampler(model, diffusion, z.shape, y, cfg_scale, sampler="flow", num_steps=num_steps, order=order,
                                  rng=rng).sample(z, **idx)
        from .flow import RectifiedFlow
        if not isinstance(diffusion, RectifiedFlow):
            raise ValueError(f'sampler="flow" runs a flow.RectifiedFlow and "ancestral" / "dpm++" a GaussianDiffusion; got sampler={sampler!r} '
                             f"with a {type(diffusion).__name__}")
        kw = dict(y=y) if cfg_scale is None else dict(y=y, cfg_scale=cfg_scale)
        fn = model.forward if cfg_scale is None else model.forward_with_cfg
        return diffusion.sample_loop(fn, z.shape, z, model_kwargs=kw, progress=progress, device=z.device, num_steps=num_steps, order=order,
                                     **ctr)
    solver = dict(num_steps=num_steps, order=order, spacing=spacing) if sampler == "dpm++" else {}
    if use_graph:
        return GraphedSampler(model, diffusion, z.shape, y, cfg_scale, clip_denoised=False, sampler=sampler, rng=rng, **solver).sample(z, **idx)
    kw = dict(y=y) if cfg_scale is None else dict(y=y, cfg_scale=cfg_scale)
    fn = model.forward if cfg_scale is None else model.forward_with_cfg
    if sampler == "dpm++":
        return diffusion.dpm_solver_sample_loop(fn, z.shape, z, clip_denoised=False, model_kwargs=kw, progress=progress, device=z.device,
                                                **solver, **ctr)
    return diffusion.p_sample_loop(fn, z.shape, z, clip_denoised=False, model_kwargs=kw, progress=progress, device=z.device, **ctr)


def save_image_grid(samples: torch.Tensor, path: str, nrow: int, value_range=(-1.0, 1.0), padding: int = 2):
    """What the reference gets from torchvision.utils.save_image(samples, path, nrow=, normalize=True, value_range=)
    (sample.py:79): min-max scale to [0, 1] over ``value_range``, tile ``nrow`` images per row with a 2-pixel black
    border, write 8-bit.  1/3/4-channel inputs become L / RGB / RGBA."""
    import numpy as np
    from PIL import Image
    x = samples.detach().float().cpu()
    lo, hi = value_range
    x = ((x.clamp(lo, hi) - lo) / max(hi - lo, 1e-5))
    n, c, h, w = x.shape
    cols = min(nrow, n)
    rows = (n + cols - 1) // cols
    grid = torch.zeros(c, rows * (h + padding) + padding, cols * (w + padding) + padding)
    for i in range(n):
        r, q = divmod(i, cols)
        top, left = padding + r * (h + padding), padding + q * (w + padding)
        grid[:, top:top + h, left:left + w] = x[i]
    arr = (grid * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
    mode = {1: "L", 3: "RGB", 4: "RGBA"}.get(c)
    assert mode, f"cannot write a {c}-channel image"
    Image.fromarray(arr[:, :, 0] if c == 1 else np.ascontiguousarray(arr), mode).save(path)


def to_uint8_nhwc(samples: torch.Tensor):
    """[-1,1] float NCHW -> uint8 NHWC as the FID npz stores it (reference sample_fid.py:87-90; .byte() truncates)."""
    s = samples.clamp(-1, 1)
    return (255 * (s + 1) / 2).byte().permute(0, 2, 3, 1).cpu().numpy()
