#!/usr/bin/env python3
"""Training harness with the reference's CLI (train.py:19-141, 225-246) on the MI355X engine.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m mapdit_amd.train \
        --data-path /data/latents --results-dir /results --model DiT-B/2
    python -m mapdit_amd.train --synthetic --results-dir /tmp/res --model DiT-S/2 --num-steps 100

Same arguments, defaults, schedule derivations, experiment directory layout (NNN-DiT-X-p/, config.yaml, log.txt,
checkpoints/NNNNNNN.pt with {"model", "opt"}, ema/{std:.3f}_{t:07d}.pt fp16 snapshots) and log line as the reference.
Added: --synthetic (N(0,1) latents, no dataset), the README's --use-* flags (accepted; the snapshot hard-wires all of
them on, SURVEY F5 — turning one off is refused), data parallelism when launched under torchrun (global batch =
--batch-size, sharded evenly; gradients summed over RCCL and averaged), and --grad-accum-steps K: one optimiser step over K
micro-batches per rank (the activations of --batch-size / (world * K) samples are alive at a time), and --max-grad-norm F: global
gradient-norm clipping on the device, fused into the optimiser step (optim.FusedAdamEMA.max_grad_norm), and --schedule-sampler
loss-second-moment: improved-DDPM's loss-aware timestep resampling with importance weights, state and draw on the device
(diffusion/timestep_sampler.py; the checkpoint then gains a "schedule_sampler" key), and --objective flow: the rectified-flow velocity
objective (flow/__init__.py) in the diffusion objective's place, with --flow-shift and --flow-timestep-density; config.yaml records it
and the sampler CLIs read it, and --data-loader device: the data set lives in HBM and a step's batch is one launch, a function of
(--seed, step) alone (data.py); the default, host, is the reference's DataLoader, and --step-rng counter: a step's timesteps, noise,
label drops and --synthetic batch come from one launch of a counter-based generator (step_rng.py) instead of torch generators, the same
bits for any world size and --grad-accum-steps, and --resume PATH: continue a --step-rng counter run from one of its checkpoints, which
hold the keys "ema" (the fp32 EMA copies) and "train_state" (step, log accumulators, fp16 guard) besides the reference's; with the
device loader or --synthetic the continued run ends with the bits of the run that was never stopped.  A default (--step-rng torch) run
writes the reference's checkpoint, key for key, and cannot be continued: its generators' states are in no checkpoint, and
--repa-features FILE | synthetic:P: representation alignment (REPA, repa.py) - a projector on the hidden state after --repa-depth blocks is
pulled toward the DINOv2 patch tokens of the clean images (`python -m mapdit_amd.dinov2 tokens`); the loss gains --repa-coeff times the
alignment term, the log line `, repa: ...`, the checkpoints "repa_head" and "repa_opt".  Single process, host loader or --synthetic.
"""
import argparse
import contextlib
import math
import os
from glob import glob
from time import time

import torch
import yaml

from . import parallel
from .data import DeviceLatentDataset
from .diffusion import create_diffusion
from .diffusion.timestep_sampler import create_named_schedule_sampler
from .flow import create_flow
from ._lib import MapditError
from .optim import FusedAdamEMA, create_lr_lambda
from .repa import RepaHead
from .src.models import DIT_MODELS
from .step_rng import StepRNG, first_slot

MP_FLAGS = ["cosine-attention", "weight-normalization", "forced-weight-normalization", "mp-residual", "mp-silu",
            "no-layernorm", "mp-pos-enc", "mp-embedding"]          # reference README.md:59-66


# Off forms this engine builds besides --no-use-forced-weight-normalization (DiT(..., mp_silu=False) etc.; src/dit.py).  The other
# three (--no-use-cosine-attention, --no-use-weight-normalization, --no-use-no-layernorm) name layers the snapshot does not contain
# (plain SDPA with learnt scale, biased nn.Linear, LayerNorm) and are refused.
BUILT_OFF_FORMS = ["mp-residual", "mp-silu", "mp-pos-enc", "mp-embedding", "weight-normalization", "cosine-attention", "no-layernorm"]


def get_model(args):
    """reference utils.py:9-17."""
    a = vars(args) if isinstance(args, argparse.Namespace) else args
    kw = dict(rotation_modulation=True) if a.get("use_rotation_modulation") else {}
    if not a.get("use_forced_weight_normalization", True):
        kw["forced_weight_normalization"] = False
    for flag in BUILT_OFF_FORMS:                    # off forms that are built (parity unpinned: README lines, no reference code)
        if not a.get("use_" + flag.replace("-", "_"), True):
            kw[flag.replace("-", "_")] = False
    return DIT_MODELS[a["model"]](in_channels=a["in_channels"], input_size=a["input_size"], num_classes=a["num_classes"], **kw)


def setup_experiment(model_name, results_dir):
    """reference train.py:200-214."""
    os.makedirs(results_dir, exist_ok=True)
    idx = len(glob(os.path.join(results_dir, "*")))
    exp = os.path.join(results_dir, f"{idx:03d}-{model_name.replace('/', '-')}")
    os.makedirs(os.path.join(exp, "checkpoints"), exist_ok=True)
    return exp


class LatentDataset(torch.utils.data.Dataset):
    """reference train.py:144-176: posterior_means.pt / posterior_stds.pt / labels.pt / stats.pt; a sample is
    (mean + randn * std) standardised per channel."""

    def __init__(self, path):
        ld = lambda n: torch.load(os.path.join(path, n), weights_only=True)
        self.means, self.stds, self.labels, self.stats = ld("posterior_means.pt"), ld("posterior_stds.pt"), ld("labels.pt"), ld("stats.pt")
        self.m = torch.as_tensor(self.stats["mean"]).view(-1, 1, 1)
        self.s = torch.as_tensor(self.stats["std"]).view(-1, 1, 1)
        assert self.means.shape[0] == self.labels.shape[0] == self.stds.shape[0]

    channels = property(lambda self: self.means.shape[1])
    data_size = property(lambda self: self.means.shape[2])

    def __len__(self):
        return self.means.shape[0]

    def __getitem__(self, i):
        f = self.means[i] + torch.randn_like(self.means[i]) * self.stds[i]
        return (f - self.m) / self.s, self.labels[i]


class RepaLatentDataset(LatentDataset):
    """--repa-features FILE with --data-path: a sample is (x, y, f), f fp16 [tokens, P] row i of the memory-mapped file (the row order of
    the latents: `dinov2 tokens` over the images `encode_data` read, with --flip-seed where that ran with --flip)."""

    def __init__(self, path, features_path):
        super().__init__(path)
        self.features_path, self._feats = features_path, None

    def __getitem__(self, i):
        import numpy as np
        if self._feats is None:                  # opened in the process that reads it (a loader worker)
            self._feats = np.load(self.features_path, mmap_mode="r")
        x, y = super().__getitem__(i)
        return x, y, torch.from_numpy(np.array(self._feats[i]))


def parse_repa_features(spec):
    """--repa-features: "synthetic:P" -> ("synthetic", P), anything else -> ("file", path).  A bad P is a ValueError naming the flag."""
    if spec.startswith("synthetic:"):
        try:
            P = int(spec[len("synthetic:"):])
        except ValueError:
            P = 0
        if P < 8 or P % 8:
            raise ValueError(f"--repa-features {spec}: the feature width after 'synthetic:' must be a positive multiple of 8")
        return "synthetic", P
    return "file", spec


def check_repa_features_file(path, num_rows, tokens):
    """The features file against the data set, from its header alone (the file is memory-mapped): fp16 [num_rows, tokens, P], P a
    multiple of 8.  Returns P; a misfit is a ValueError naming --repa-features and what does not fit."""
    import numpy as np
    if not os.path.isfile(path):
        raise ValueError(f"--repa-features {path}: no such file (write one with `python -m mapdit_amd.dinov2 tokens`, or pass synthetic:P with --synthetic)")
    try:
        a = np.load(path, mmap_mode="r")
    except Exception as e:
        raise ValueError(f"--repa-features {path}: not a .npy array ({e})") from None
    if a.dtype != np.float16:
        raise ValueError(f"--repa-features {path}: dtype {a.dtype}, expected float16 (what `dinov2 tokens` writes)")
    if a.ndim != 3:
        raise ValueError(f"--repa-features {path}: shape {tuple(a.shape)}, expected [samples, tokens, feature width]")
    if a.shape[0] != num_rows:
        raise ValueError(f"--repa-features {path}: {a.shape[0]} rows, the data set has {num_rows} samples (one row per latent, in the latents' order)")
    if a.shape[1] != tokens:
        raise ValueError(f"--repa-features {path}: {a.shape[1]} tokens per sample, the model has (input_size / patch)^2 = {tokens} "
                         f"(`dinov2 tokens --grid {math.isqrt(tokens)}`)")
    if a.shape[2] < 8 or a.shape[2] % 8:
        raise ValueError(f"--repa-features {path}: feature width {a.shape[2]} must be a positive multiple of 8")
    return int(a.shape[2])


def check_repa_args(args, world):
    """The refusals of --repa-features that need no device: each a ValueError naming the flag that does not fit."""
    if args.repa_features is None:
        return None
    kind, what = parse_repa_features(args.repa_features)
    if args.data_loader == "device":
        raise ValueError("--repa-features is not built for --data-loader device (the device-resident loader gathers latents alone); use the host loader")
    if world > 1:
        raise ValueError(f"--repa-features is single-process: a world size of {world} needs an all-reduce of the head's gradients, which is not built")
    if args.precision == "bf16x3":
        raise ValueError("--repa-features is not built for --precision bf16x3 (the hidden-state gradient is a bf16 / f16 engine feature)")
    if not args.use_no_layernorm:
        raise ValueError("--repa-features is not built for --no-use-no-layernorm (the LayerNorm form)")
    if kind == "synthetic" and not args.synthetic:
        raise ValueError(f"--repa-features {args.repa_features} draws N(0,1) features for --synthetic; a data set needs a features file")
    if kind == "file" and args.synthetic:
        raise ValueError(f"--repa-features {args.repa_features}: --synthetic has no images to have features of; pass synthetic:P")
    if not args.repa_coeff >= 0 or not math.isfinite(args.repa_coeff):
        raise ValueError(f"--repa-coeff {args.repa_coeff} must be finite and >= 0")
    if args.repa_hidden < 8 or args.repa_hidden % 8:
        raise ValueError(f"--repa-hidden {args.repa_hidden} must be a positive multiple of 8")
    if not args.repa_lr > 0:
        raise ValueError(f"--repa-lr {args.repa_lr} must be positive")
    if args.repa_depth is not None and args.repa_depth < 1:
        raise ValueError(f"--repa-depth {args.repa_depth} must be at least 1")
    return kind, what


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--data-path", type=str, default=None)
    p.add_argument("--synthetic", action="store_true", help="N(0,1) 4x32x32 latents and uniform labels instead of a dataset")
    p.add_argument("--synthetic-input-size", type=int, default=32,
                   help="side of the --synthetic latents (64: 512x512 images, 1,024 tokens per sample at patch 2)")
    p.add_argument("--results-dir", type=str, default=None, help="required, except with --resume (the run continues in its own directory)")
    p.add_argument("--model", type=str, choices=list(DIT_MODELS.keys()), default="DiT-XS/2")
    p.add_argument("--num-classes", type=int, default=1000)
    p.add_argument("--num-steps", type=int, default=400_000)
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--lr", type=float, default=1e-2)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--verbose", type=int, choices=[0, 1, 2], default=1)
    p.add_argument("--num-workers", type=int, default=4)
    p.add_argument("--data-loader", choices=["host", "device"], default="host",
                   help="host (default): the reference's DataLoader over --data-path, --num-workers processes per rank; device: the data "
                        "set is uploaded once and every batch - epoch shuffle, gather, posterior draw, standardisation - is one launch, a "
                        "function of (--seed, optimiser step) alone: the same data for any world size and --grad-accum-steps "
                        "(data.DeviceLatentDataset; --num-workers is ignored; the data set must fit HBM)")
    p.add_argument("--log-every", type=int, default=100)
    p.add_argument("--ckpt-every", type=int, default=50_000)
    p.add_argument("--num-lin-warmup", type=int, default=None)
    p.add_argument("--start-decay", type=int, default=None)
    p.add_argument("--ema-snapshot-every", type=int, default=None)
    p.add_argument("--precision", choices=["bf16", "f16", "bf16x3"], default="f16",
                   help="GEMM operand precision: f16 (default: IEEE fp16 operands, logits within 1e-3 of the fp32 reference; power-of-two "
                        "loss scale, steps with non-finite gradients are refused and the scale halved), bf16 (the same engine with bf16 "
                        "operands: 2 %% faster, ~6e-3) or bf16x3 (fp32-accurate forward and backward, the reference's numerics to ~1e-5, "
                        "several times slower)")
    p.add_argument("--grad-comm", choices=["allreduce", "zero1", "zero1w", "zero1w-bf16"], default=None,
                   help="data-parallel gradient exchange: per-stage all-reduce overlapped with backward (default), or "
                        "reduce-scatter + sharded optimiser + all-gather (zero1), or sharded weight passes - forced weight norm, imaging, "
                        "Jacobian, Adam / EMA on 1/world of the rows, 16-bit images all-gathered (zero1w; -bf16: 16-bit gradient exchange)")
    p.add_argument("--activation-recompute", choices=["none", "mlp", "block"], default="none",
                   help="keep fewer activations for the backward and regenerate them block by block (bit-identical gradients): mlp = a "
                        "block's fc1 GEMM is issued again (24 instead of 40 x hidden bytes per token and block), block = the block's whole "
                        "forward (12); f16 / bf16 precisions")
    p.add_argument("--grad-accum-steps", type=int, default=1,
                   help="K > 1: an optimiser step is taken over K micro-batches - each rank's share of --batch-size is cut into K equal "
                        "parts, forward and backward run once per part and the engine adds the gradients up in place (the first K - 1 "
                        "parts without a gradient exchange).  Steps, schedules, checkpoints and steps/sec count optimiser steps; "
                        "activation memory is that of one part.  Not with --grad-comm zero1w / zero1w-bf16 or --precision bf16x3 under "
                        "data parallelism")
    p.add_argument("--max-grad-norm", type=float, default=None,
                   help="clip the global gradient norm (torch.nn.utils.clip_grad_norm_ semantics on the averaged gradient) on the device, "
                        "fused into the optimiser step; `inf` only measures.  The log line gains the norm and the coefficient of the step "
                        "it is written at.  Not with --grad-comm zero1w / zero1w-bf16")
    p.add_argument("--schedule-sampler", choices=["uniform", "loss-second-moment"], default="uniform",
                   help="how a step draws its timesteps: uniform (default: torch.randint, the reference's train.py) or loss-second-moment "
                        "(diffusion/timestep_sampler.py: p(t) follows the second moment of each timestep's last 10 losses once every "
                        "timestep has 10, the loss is weighted by 1 / (T p(t)); history, table and draw stay on the device, ranks share one "
                        "history).  Individual weights reach 1 / uniform_prob = 1000 in the worst case: see INTEGRATION.md on --precision f16")
    p.add_argument("--objective", choices=["diffusion", "flow"], default="diffusion",
                   help="diffusion (default): the reference's eps objective with learned-range variances; flow: the rectified-flow velocity "
                        "objective on the same timestep grid (x_s = (1 - s) x0 + s eps, target eps - x0; the variance channels are ignored). "
                        "Sample such a run with --sampler flow-euler / flow-heun")
    p.add_argument("--flow-shift", type=float, default=1.0, help="--objective flow: SD3's resolution shift of flow time (1: none)")
    p.add_argument("--flow-timestep-density", choices=["uniform", "logit-normal"], default="uniform",
                   help="--objective flow: how the default (uniform) schedule sampler draws timesteps (logit-normal: SD3's, loc 0, scale 1); "
                        "under --schedule-sampler loss-second-moment that sampler draws them and this flag changes nothing")
    for f in MP_FLAGS:
        p.add_argument(f"--use-{f}", dest="use_" + f.replace("-", "_"), action=argparse.BooleanOptionalAction, default=True)
    p.add_argument("--use-rotation-modulation", action=argparse.BooleanOptionalAction, default=False,
                   help="block conditioning by rotation modulation (reference README.md:1-3; not in its code snapshot: this build's "
                        "own restatement, parity unpinned): ~5.4 %% fewer parameters; bf16 and f16 precisions")
    p.add_argument("--step-rng", choices=["torch", "counter"], default="torch",
                   help="where a step's randomness comes from: torch (default: torch.randint / randn_like / rand on per-rank generators, "
                        "as the reference draws) or counter (step_rng.py: timesteps, noise, label drops and the --synthetic batch in one "
                        "launch, a function of (--seed, optimiser step, slot in the global batch): the same draws for any world size and "
                        "--grad-accum-steps, nothing to carry over a --resume.  With --data-loader device or --synthetic the whole step "
                        "is then a function of (--seed, step); with --data-loader host the loader's order is not.  Checkpoints of a "
                        "counter run gain the keys --resume needs; a torch run writes the reference's two)")
    p.add_argument("--repa-features", type=str, default=None, metavar="FILE | synthetic:P",
                   help="representation alignment (REPA): FILE = fp16 [samples, tokens, P] .npy of DINOv2 patch tokens in the latents' order "
                        "(`python -m mapdit_amd.dinov2 tokens`), memory-mapped; synthetic:P = N(0,1) features for --synthetic.  Single "
                        "process, host loader, f16 / bf16")
    p.add_argument("--repa-coeff", type=float, default=0.5, help="weight of the alignment term in the loss")
    p.add_argument("--repa-depth", type=int, default=None, help="align the hidden state after this many blocks (default: 8 for depth >= 24, else 4)")
    p.add_argument("--repa-hidden", type=int, default=2048, help="width of the projector's two inner layers")
    p.add_argument("--repa-lr", type=float, default=1e-4, help="learning rate of the projector's Adam (the run's warm-up and decay apply)")
    p.add_argument("--resume", type=str, default=None, metavar="PATH",
                   help="continue a --step-rng counter run: PATH is one of its checkpoints/NNNNNNN.pt or its experiment directory (the "
                        "latest checkpoint).  "
                        "The run goes on in that directory (log.txt is appended to, config.yaml is left alone); its arguments are read "
                        "from config.yaml and one given here with another value is refused, except --num-steps (may be raised), "
                        "--log-every, --ckpt-every, --ema-snapshot-every, --verbose, --num-workers and --grad-comm (allreduce / zero1).  "
                        "Bit-identical to the unstopped run with --data-loader device or --synthetic; a host loader starts a fresh epoch "
                        "order.  A --step-rng torch run cannot be continued (its checkpoints are the reference's, without the generators)")
    return p


# ---- --resume: host logic (no device work) ------------------------------------------------------------------------------------------
RESUME_FREE = ("num_steps", "log_every", "ckpt_every", "ema_snapshot_every", "verbose", "num_workers", "grad_comm", "resume", "results_dir")
RESUME_KEYS = ("model", "opt", "ema", "train_state")          # what a checkpoint must hold to be continued


def resolve_checkpoint(path):
    """--resume PATH -> the checkpoint file: PATH itself, or the latest checkpoints/NNNNNNN.pt of the experiment directory PATH."""
    if os.path.isdir(path):
        found = sorted(glob(os.path.join(path, "checkpoints", "[0-9]*.pt")), key=lambda f: int(os.path.splitext(os.path.basename(f))[0]))
        if not found:
            raise ValueError(f"--resume {path}: no checkpoints/NNNNNNN.pt in that directory")
        return found[-1]
    if not os.path.isfile(path):
        raise ValueError(f"--resume {path}: neither a checkpoint file nor an experiment directory")
    return path


def explicit_args(argv):
    """The arguments given on the command line (dest -> value), without the defaults of those that were not."""
    p = build_parser()
    for a in p._actions:
        a.default, a.required = argparse.SUPPRESS, False
    return vars(p.parse_args(argv))


def merge_resume_args(args, given, cfg):
    """The arguments a continued run trains with: the run's own (config.yaml) with the command line's for the RESUME_FREE ones.  A
    run-defining argument given with another value is a ValueError naming it.  Schedules that were derived from --num-steps (None in
    the yaml) are derived from the ORIGINAL --num-steps again, so that raising it does not move the learning-rate curve."""
    merged = argparse.Namespace(**vars(args))
    for key, value in vars(args).items():
        if key in RESUME_FREE:
            if key not in given and key in cfg and key not in ("resume", "results_dir"):
                setattr(merged, key, cfg[key])
        elif key in given and key in cfg and given[key] != cfg[key]:
            raise ValueError(f"--resume: --{key.replace('_', '-')} {given[key]!r} differs from the run's {cfg[key]!r} (config.yaml); a "
                             f"continued run keeps its arguments - only {', '.join('--' + k.replace('_', '-') for k in RESUME_FREE[:7])} may change")
        elif key in cfg:
            setattr(merged, key, cfg[key])
    if merged.step_rng != "counter":
        raise ValueError("--resume continues runs trained with --step-rng counter: a --step-rng torch run keeps its randomness in torch "
                         "generators that no checkpoint holds, and its checkpoints are the reference's (\"model\", \"opt\")")
    original = int(cfg["num_steps"])
    if merged.num_lin_warmup is None:
        merged.num_lin_warmup = original // 150
    if merged.start_decay is None:
        merged.start_decay = original // 10
    if merged.ema_snapshot_every is None:
        merged.ema_snapshot_every = original // 250
    return merged


def check_resumable(ckpt, args, path):
    """Refuse a checkpoint that cannot be continued (a reference checkpoint holds only "model" and "opt") or lies behind --num-steps."""
    for key in RESUME_KEYS:
        if key not in ckpt:
            raise ValueError(f"--resume {path}: the checkpoint has no {key!r} key (it holds {sorted(ckpt)}): it was not written by this "
                             f"train.py and cannot be continued bit for bit")
    done = int(ckpt["train_state"]["train_steps"])
    if args.num_steps < done:
        raise ValueError(f"--resume {path}: --num-steps {args.num_steps} lies below the checkpoint's step {done}")
    return done


def micro_batch(batch_size: int, world: int, accum_steps: int) -> int:
    """Samples of one forward: the per-rank share of the global batch (parallel.shard_batch) cut into `accum_steps` equal micro-batches.
    Raises ValueError when either split is ragged."""
    if accum_steps < 1:
        raise ValueError(f"--grad-accum-steps must be >= 1, got {accum_steps}")
    lo, hi = parallel.shard_batch(int(batch_size), 0, world)
    if (hi - lo) % accum_steps:
        raise ValueError(f"--grad-accum-steps {accum_steps} does not divide the per-rank batch {hi - lo} "
                         f"(--batch-size {batch_size} over {world} rank(s)): micro-batches must be equal")
    return (hi - lo) // accum_steps


def main(argv=None):
    args = build_parser().parse_args(argv)
    resume, resume_path = None, None
    if args.resume is not None:
        resume_path = resolve_checkpoint(args.resume)
        resume_exp = os.path.dirname(os.path.dirname(os.path.abspath(resume_path)))
        with open(os.path.join(resume_exp, "config.yaml")) as f:
            args = merge_resume_args(args, explicit_args(argv), yaml.safe_load(f))
        if args.grad_comm in ("zero1w", "zero1w-bf16"):
            raise MapditError("--resume is not built for --grad-comm zero1w / zero1w-bf16 (a rank holds rows of every weight, the checkpoint "
                              "the whole state); continue with allreduce or zero1")
        resume = torch.load(resume_path, map_location="cpu", weights_only=True)
        check_resumable(resume, args, resume_path)
    elif args.results_dir is None:
        raise ValueError("--results-dir is required (except with --resume)")
    K = int(args.grad_accum_steps)
    micro = micro_batch(args.batch_size, int(os.environ.get("WORLD_SIZE", "1")), K)      # (fails here, before any device work)
    if K > 1 and args.grad_comm in ("zero1w", "zero1w-bf16"):
        raise NotImplementedError("--grad-accum-steps is not built for --grad-comm zero1w / zero1w-bf16 (sharded weight passes keep raw "
                                  "gradient sums between the exchange and the Jacobian); use allreduce or zero1")
    # --no-use-forced-weight-normalization is the one off-path the snapshot's code defines (skip the in-place rewrite); the other seven are
    # built as restatements of their README lines (BUILT_OFF_FORMS, parity unpinned: the snapshot hard-wires every feature on)
    off = [f for f in MP_FLAGS if not getattr(args, "use_" + f.replace("-", "_"))
           and f != "forced-weight-normalization" and f not in BUILT_OFF_FORMS]
    if off:
        raise NotImplementedError(f"--no-use-{off[0]}: no off form built; built: --no-use-forced-weight-normalization, "
                                  + ", ".join("--no-use-" + f for f in BUILT_OFF_FORMS))
    if args.precision == "bf16x3" and any(not getattr(args, "use_" + f.replace("-", "_")) for f in BUILT_OFF_FORMS):
        raise NotImplementedError("the --no-use-* off forms are built for the f16 / bf16 engines, not for --precision bf16x3")
    if args.activation_recompute != "none" and (args.precision == "bf16x3" or not args.use_no_layernorm):
        raise NotImplementedError("--activation-recompute is built for the f16 / bf16 engines without the LayerNorm form (--no-use-no-layernorm)")
    if not args.use_no_layernorm and args.use_rotation_modulation:
        raise NotImplementedError("--no-use-no-layernorm (the LayerNorm form) is built for the AdaLN modulation, not with --use-rotation-modulation")
    if args.data_loader == "device" and args.synthetic:
        raise ValueError("--data-loader device draws from the data set under --data-path; --synthetic has none")
    repa = check_repa_args(args, int(os.environ.get("WORLD_SIZE", "1")))      # (None without --repa-features: nothing below changes)
    if repa is not None and resume is not None:
        for key in ("repa_head", "repa_opt"):
            if key not in resume:
                raise ValueError(f"--resume {resume_path}: the checkpoint has no {key!r} key, the run trains with --repa-features {args.repa_features}")
    flow_mode = args.objective == "flow"
    if not flow_mode and (args.flow_shift != 1.0 or args.flow_timestep_density != "uniform"):
        raise ValueError("--flow-shift / --flow-timestep-density belong to --objective flow")
    if flow_mode:
        create_flow(shift=args.flow_shift)                               # (a bad --flow-shift fails here, before any device work)
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    torch.manual_seed(args.seed)
    lo, hi = parallel.shard_batch(int(args.batch_size), rank, world)
    per_rank = hi - lo

    if args.synthetic:
        args.in_channels, args.input_size = 4, int(args.synthetic_input_size)
        args.stats_mean, args.stats_std = [0.0] * 4, [1.0] * 4
        loader = None
    else:
        assert args.data_path, "--data-path or --synthetic"
        if args.data_loader == "device":
            ds, loader = DeviceLatentDataset(args.data_path, dev, seed=args.seed), None
        else:
            ds = LatentDataset(args.data_path) if repa is None else RepaLatentDataset(args.data_path, args.repa_features)
            sampler = torch.utils.data.distributed.DistributedSampler(ds, world, rank, shuffle=True, drop_last=True) if world > 1 else None
            loader = torch.utils.data.DataLoader(ds, batch_size=per_rank, num_workers=args.num_workers, shuffle=sampler is None,
                                                 sampler=sampler, pin_memory=True, drop_last=True)
        args.in_channels, args.input_size = ds.channels, ds.data_size
        args.stats_std = [float(v) for v in ds.stats["std"]]
        args.stats_mean = [float(v) for v in ds.stats["mean"]]
        if repa is not None:                     # (host work: the file's header against the data set, before the model exists)
            patch = int(args.model.split("/")[1])
            repa = ("file", check_repa_features_file(args.repa_features, len(ds), (ds.data_size // patch) ** 2))

    exp = None
    if rank == 0:
        if resume is not None:
            exp = resume_exp                     # the run's own directory: config.yaml stays, log.txt is appended to
        else:
            exp = setup_experiment(args.model, args.results_dir)
            with open(os.path.join(exp, "config.yaml"), "w") as f:
                yaml.dump(vars(args), f)
        os.makedirs(os.path.join(exp, "ema"), exist_ok=True)
        logf = open(os.path.join(exp, "log.txt"), "a")

    def log(msg):
        if rank == 0 and args.verbose:
            print(msg, flush=True)
            logf.write(msg + "\n")
            logf.flush()

    # --objective flow: a RectifiedFlow stands where the diffusion stood (num_timesteps, training_losses); nothing below looks inside
    diffusion = create_flow(shift=args.flow_shift) if flow_mode else create_diffusion(timestep_respacing="")
    model = get_model(args).to(dev).train()
    model.gemm_precision = args.precision
    model.activation_recompute = args.activation_recompute
    log(f"model parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad):,}")
    if args.ema_snapshot_every is None:
        args.ema_snapshot_every = args.num_steps // 250
    if args.num_lin_warmup is None:
        args.num_lin_warmup = args.num_steps // 150
    if args.start_decay is None:
        args.start_decay = args.num_steps // 10
    # Identical parameters on every rank come from the shared seed above (no broadcast needed).  From here on each rank must draw
    # its OWN timesteps, noise and label drops - the reference's single process draws them independently for all 256 samples
    # (train.py:86; gaussian_diffusion.py:735; label_embedder.py:23) - so the default generators are re-seeded per rank.
    torch.manual_seed(args.seed + 1000003 * (rank + 1))
    reducer = parallel.make_reducer(model, args.grad_comm)
    opt = FusedAdamEMA(model, lr=args.lr, betas=(0.9, 0.99), ema_stds=(0.05, 0.1),
                       lr_lambda=create_lr_lambda(args.num_lin_warmup, args.start_decay),
                       # K micro-batches: every micro-loss is the plain mean of its micro-batch (the magnitude the automatic fp16 loss
                       # scale is chosen for) and the gradients are SUMMED over the K backwards - the mean over them is taken here
                       grad_scale=reducer.grad_scale if K == 1 else reducer.grad_scale / K,
                       max_grad_norm=args.max_grad_norm)
    reducer.attach(opt)
    head = head_opt = feats_rng = None
    if repa is not None:
        # REPA: the projector and its own optimiser - outside --max-grad-norm, the model's EMA, state dict and snapshots
        B = args.repa_depth if args.repa_depth is not None else (8 if model.depth >= 24 else 4)
        if not 1 <= B <= model.depth - 1:
            raise ValueError(f"--repa-depth {B}: the tap must lie after 1 .. depth - 1 = {model.depth - 1} blocks of {args.model}")
        model.hidden_tap = B - 1
        repa_tokens, repa_dim = (args.input_size // model.patch_size) ** 2, repa[1]
        head = RepaHead(model.hidden_size, repa_dim, hidden=args.repa_hidden, precision=args.precision, seed=args.seed).to(dev)
        head_opt = FusedAdamEMA(head, lr=args.repa_lr, betas=(0.9, 0.99), ema_stds=(),
                                lr_lambda=create_lr_lambda(args.num_lin_warmup, args.start_decay), grad_scale=1.0 if K == 1 else 1.0 / K)
        log(f"REPA: {sum(p.numel() for p in head.parameters()):,} projector parameters, hidden state after {B} blocks, {repa_tokens} x {repa_dim} features")
    # the default draws with torch.randint below, exactly as before; the sampler object exists only with the flag
    t_sampler = create_named_schedule_sampler(args.schedule_sampler, diffusion) if args.schedule_sampler != "uniform" else None
    # --step-rng counter: one launch per micro-batch draws everything random in it; no torch generator is consumed in a step
    step_rng = StepRNG(args.seed, dev) if args.step_rng == "counter" else None
    if repa is not None and repa[0] == "synthetic" and step_rng is not None:
        feats_rng = StepRNG(args.seed ^ 0x52455041, dev)       # a stream of its own: features of (seed, step, slot in the global batch)
    start_step = 0
    if resume is not None:
        state = resume["train_state"]
        model.load_state_dict(resume["model"])
        opt.load_state_dict(resume["opt"])
        opt.load_resume_state_dict({"ema": resume["ema"], "guard": state["guard"]})      # (ZeRO-1: a rank goes on updating its shard of it)
        if t_sampler is not None:
            if "schedule_sampler" not in resume:
                raise ValueError(f"--resume {resume_path}: the checkpoint has no 'schedule_sampler' key, the run samples with {args.schedule_sampler}")
            t_sampler.load_state_dict(resume["schedule_sampler"])
        if head is not None:
            head.load_state_dict(resume["repa_head"])
            head_opt.load_state_dict(resume["repa_opt"]["opt"])
            head_opt.load_resume_state_dict({"ema": {}, "guard": resume["repa_opt"]["guard"]})
        start_step = int(state["train_steps"])
        log(f"resuming from {resume_path} at step {start_step} (saved by {state['world_size']} rank(s))")
        if loader is not None:
            log("--data-loader host: the loader's position is not in a checkpoint - the continuation starts a fresh epoch order and is not "
                "bit-identical to the run that was never stopped (--data-loader device is)")
        del resume

    def draw_t(n):
        if flow_mode:
            return diffusion.sample_timesteps(n, dev, density=args.flow_timestep_density)
        return torch.randint(0, diffusion.num_timesteps, (n,), device=dev)

    def weighted_loss(xb, yb):
        """Mean over the batch of weight x loss at timesteps drawn by the schedule sampler; the history takes the unweighted losses."""
        t, w = t_sampler.sample(xb.shape[0], dev)
        losses = diffusion.training_losses(model, xb, t, dict(y=yb))
        t_sampler.update_with_local_losses(t, losses["loss"].detach())
        return (losses["loss"] * w).mean()

    def batches():
        if args.data_loader == "device":
            while True:                          # train_steps: optimiser steps taken so far = the 0-based step this batch belongs to
                yield ds.batch(train_steps, args.batch_size, rank, world)
        if loader is None:
            if step_rng is not None:             # the synthetic batch is drawn with the step's other draws (counter_loss)
                while True:
                    yield None, None
            g = torch.Generator(device=dev).manual_seed(args.seed + 1 + rank)
            gf = torch.Generator(device=dev).manual_seed(args.seed + 2 + rank) if head is not None else None
            while True:
                xy = (torch.randn(per_rank, 4, args.input_size, args.input_size, device=dev, generator=g),
                      torch.randint(0, args.num_classes, (per_rank,), device=dev, generator=g))
                yield xy if gf is None else xy + (torch.randn(per_rank, repa_tokens, repa_dim, device=dev, generator=gf),)
        epoch = start_step // max(len(loader), 1)      # (a continued run starts a fresh epoch order: the loader's position is not kept)
        while True:
            if world > 1:
                loader.sampler.set_epoch(epoch)
            for b in loader:
                yield tuple(v.to(dev, non_blocking=True) for v in b)
            epoch += 1

    def counter_loss(xk, yk, k):
        """Micro-batch k of this rank under --step-rng counter: its slots of the global batch are lo + k * micro onwards."""
        want = ["eps"] + (["x_syn", "y_syn"] if xk is None else []) + (["drop"] if model.class_dropout_prob > 0 else [])
        logit_normal = flow_mode and args.flow_timestep_density == "logit-normal"
        want.append("u" if t_sampler is not None else "z" if logit_normal else "t")
        shape = (micro, args.in_channels, args.input_size, args.input_size)
        d = step_rng.draw(train_steps, first_slot(lo, k, micro), micro, per=shape[1] * shape[2] * shape[3], T=diffusion.num_timesteps,
                          num_classes=args.num_classes, drop_prob=model.class_dropout_prob, want=want)
        if xk is None:
            xk, yk = d.x_syn.view(shape), d.y_syn
        kw = dict(y=yk, force_drop_ids=d.drop) if "drop" in want else dict(y=yk)
        if t_sampler is not None:
            t, w = t_sampler.sample_from_uniforms(d.u)
            losses = diffusion.training_losses(model, xk, t, kw, noise=d.eps.view(shape))
            t_sampler.update_with_local_losses(t, losses["loss"].detach())
            return (losses["loss"] * w).mean()
        t = diffusion.timesteps_from_normals(d.z) if logit_normal else d.t
        return diffusion.training_losses(model, xk, t, kw, noise=d.eps.view(shape))["loss"].mean()

    running_repa = torch.zeros((), device=dev)

    def with_repa(base, f, k):
        """base + --repa-coeff x the mean alignment loss of micro-batch k: the projector reads the hidden state the forward behind `base`
        tapped, and its backward hands d loss / d hidden to the engine.  `f`: this rank's features of the step, or None (drawn here)."""
        if head is None:
            return base
        if feats_rng is not None:
            fk = feats_rng.draw(train_steps, first_slot(lo, k, micro), micro, per=repa_tokens * repa_dim, want=["eps"]).eps
            fk = fk.view(micro, repa_tokens, repa_dim)
        else:
            fk = f[k * micro:(k + 1) * micro]
        term = head.loss(model.tapped_hidden, fk).mean()
        running_repa.add_(term.detach() / K)
        return base + args.repa_coeff * term

    train_steps, log_steps, running, start = start_step, 0, torch.zeros((), device=dev), time()
    if resume_path is not None:                  # the log accumulators: a checkpoint may fall between two log lines
        log_steps = int(state["log_steps"])
        running.fill_(float(state["running"]))
        running_repa.fill_(float(state.get("running_repa", 0.0)))
    if train_steps >= args.num_steps:
        log(f"nothing to do: the checkpoint is at step {train_steps}, --num-steps is {args.num_steps}")
        return exp
    log(f"training for {args.num_steps} steps...")
    for batch in batches():
        x, y, f = batch[0], batch[1], (batch[2] if len(batch) > 2 else None)
        if head_opt is not None:
            head_opt.zero_grad()
        if step_rng is not None:
            opt.zero_grad()
            loss = torch.zeros((), device=dev)
            for k in range(K):
                sl = slice(k * micro, (k + 1) * micro)
                part = with_repa(counter_loss(None if x is None else x[sl], None if y is None else y[sl], k), f, k)
                with (reducer.no_sync() if k < K - 1 else contextlib.nullcontext()):
                    part.backward()
                loss = loss + part.detach()
            loss = loss / K
        elif K == 1:
            if t_sampler is None:
                t = draw_t(x.shape[0])
                loss = diffusion.training_losses(model, x, t, dict(y=y))["loss"].mean()
            else:
                loss = weighted_loss(x, y)
            loss = with_repa(loss, f, 0)
            opt.zero_grad()
            loss.backward()
        else:
            # one optimiser step over K micro-batches: a fresh backward, then accumulating ones (p.grad stays set: the engine adds in place);
            # only the last one exchanges gradients - its stages hand over this rank's sums over all K
            opt.zero_grad()
            loss = torch.zeros((), device=dev)
            for k in range(K):
                xk, yk = x[k * micro:(k + 1) * micro], y[k * micro:(k + 1) * micro]
                if t_sampler is None:
                    t = draw_t(micro)                                                            # each micro-batch draws its own
                    part = diffusion.training_losses(model, xk, t, dict(y=yk))["loss"].mean()    # NOT divided by K: see grad_scale above
                else:
                    part = weighted_loss(xk, yk)
                part = with_repa(part, f, k)
                with (reducer.no_sync() if k < K - 1 else contextlib.nullcontext()):
                    part.backward()
                loss = loss + part.detach()
            loss = loss / K
        reducer.finish()
        opt.step()
        if head_opt is not None:
            head_opt.step()
        running += loss.detach()
        log_steps += 1
        train_steps += 1
        if train_steps % args.log_every == 0:
            model.check_device_errors()          # an out-of-range label / timestep raises here (the reference: IndexError)
            refused = opt.poll_overflow()        # fp16: steps refused for non-finite gradients since the last log line
            if refused:
                log(f"(step={train_steps:07d}) {refused} optimiser step(s) refused: non-finite gradients; fp16 loss scale now "
                    f"{model.loss_scale or model.effective_loss_scale():g}")
            avg = running / log_steps
            if world > 1:
                torch.distributed.all_reduce(avg)
                avg /= world
            sps = log_steps / (time() - start)
            clip_msg = ""
            if args.max_grad_norm is not None:   # the values of this step: one read-back per log line
                clip_msg = ", grad norm: {:.4f}, clip: {:.3f}".format(*opt.clip_values())
            repa_msg = ""
            if head is not None:
                if head_opt.poll_overflow():
                    log(f"(step={train_steps:07d}) projector step(s) refused: non-finite gradients; its fp16 loss scale now "
                        f"{head.loss_scale or head.effective_loss_scale():g}")
                repa_msg = ", repa: {:.4f}".format((running_repa / log_steps).item())
                running_repa.zero_()
            log(f"(step={train_steps:07d}) train loss: {avg.item():.4f}, train steps/sec: {sps:.2f}{clip_msg}{repa_msg}")
            running.zero_()
            log_steps, start = 0, time()
        if train_steps % args.ckpt_every == 0 or (args.ema_snapshot_every and train_steps % args.ema_snapshot_every == 0):
            reducer.gather_state()               # ZeRO-1: Adam moments / EMA copies are sharded; complete them (collective)
        if rank == 0 and train_steps % args.ckpt_every == 0:
            ckpt = {"model": model.state_dict(), "opt": opt.state_dict()}                      # reference train.py:125-132
            if t_sampler is not None:
                ckpt["schedule_sampler"] = t_sampler.state_dict()
            if head is not None:
                ckpt["repa_head"] = head.state_dict()
                ckpt["repa_opt"] = {"opt": head_opt.state_dict(), "guard": head_opt.resume_state_dict()["guard"]}
            if step_rng is not None:
                # what --resume needs beyond the reference's keys: the fp32 EMA copies (the snapshots are fp16) and the loop's own state.
                # (The default run's checkpoint stays the reference's, key for key.)
                rs = opt.resume_state_dict()
                ckpt["ema"] = rs["ema"]
                ckpt["train_state"] = {"train_steps": train_steps, "running": running.item(), "log_steps": log_steps, "guard": rs["guard"],
                                       "step_rng": args.step_rng, "seed": args.seed, "world_size": world}
                if head is not None:
                    ckpt["train_state"]["running_repa"] = running_repa.item()
            torch.save(ckpt, os.path.join(exp, "checkpoints", f"{train_steps:07d}.pt"))
        if rank == 0 and args.ema_snapshot_every and train_steps % args.ema_snapshot_every == 0:
            for std in opt.ema_stds:                                   # reference src/ema.py:143-155
                sd = {k: v.cpu().half() for k, v in opt.ema_state_dict(std).items()}
                torch.save({"std": std, "t": train_steps, "state_dict": sd}, os.path.join(exp, "ema", f"{std:.3f}_{train_steps:07d}.pt"))
        if train_steps >= args.num_steps:
            break
    log("done!")
    return exp


if __name__ == "__main__":
    main()
