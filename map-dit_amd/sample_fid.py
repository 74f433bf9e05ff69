"""MI355X counterpart of the reference's ``sample_fid.py``: ``--num-samples`` images in batches of ``--batch-size`` with
random labels (classifier-free guidance when ``--cfg-scale`` > 1), stored as one uint8 NHWC array ``arr_0`` in
``<result-dir>/fid_samples/<output-file>`` (reference sample_fid.py:48-97; flags :100-114).  One hipGraph is captured for
the batch shape and replayed for every batch (``--sampler dpm++``: DPM-Solver++ with ``--num-sampling-steps`` model evaluations).  Without a VAE (``--use-vae false``) the array holds the de-normalised
latents clamped to [-1, 1] and quantised the same way; with ``--vae-weights FILE`` the native VAE decoder (map-dit_amd/vae.py) turns
them into pixels first (``arr_0``: [n, 8S, 8S, 3]).  ``--fid-ref REF.npz --inception-weights FILE`` (together, and with pixels): the
FID of the samples against the reference statistics, accumulated batch by batch on the device (map-dit_amd/fid.py), printed, returned
and written to ``fid_samples/<output-file>.fid.json``; the array is written as before.  ``--metrics fid,pr,kid`` (default ``fid``)
adds precision / recall / density / coverage and KID (map-dit_amd/metrics.py) to that file (under its key ``metrics``) and to the output: ``--fid-ref`` must then
be a file of ``python -m mapdit_amd.fid features`` (it holds ``pool_3``); the samples' features stay on the device.  ``fid_s`` (sFID)
needs ``mu_s`` / ``sigma_s`` in ``--fid-ref`` (``fid stats --spatial``) and accumulates the spatial statistics in the same pass of the
network; ``isc`` (the samples' Inception Score, stored as ``isc`` and ``isc_std``) reads the classifier head of ``--inception-weights``.

``--sample-rng counter``: sample i - its latent, its label, the noise of every step - is a function of (``--seed``, i) alone
(map-dit_amd/sample_rng.py), batch b holds the sample indices [b n, (b + 1) n) (n = ``--batch-size``), and every finished batch is
written as ``fid_samples/<output-file>.parts/<first>-<end>.npy`` beside a ``manifest.json`` of everything the bytes depend on.  Running
the same command again skips the batches whose part exists (that is resuming); ``--shard R/W`` takes the batches with b % W == R, so W
processes on W GPUs share a run; whichever process finds every part present assembles ``arr_0`` in index order and computes the
metrics from the assembled bytes.  The finished file has the same bits whatever history produced it.  A manifest that differs in any
key is refused before any model is built.

``--dinov2-ref REF.npz --dinov2-weights FILE`` (together, and with pixels): FD-DINOv2, the Fréchet distance on the CLS features of the
DINOv2 ViT (map-dit_amd/dinov2.py) against the reference's ``mu_dinov2`` / ``sigma_dinov2`` - one more pass over the same uint8 bytes
the FID pass reads (under ``--sample-rng counter``: over the assembled array), printed as ``fd_dinov2:`` and written to
``fid_samples/<output-file>.fd_dinov2.json``.  The flags have no bearing on the array, the manifest or ``.fid.json``."""
from __future__ import annotations

import argparse
import math
import os

import numpy as np
import torch

from . import sampling as S
from .train import get_model


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--result-dir", type=str, required=True)
    p.add_argument("--use-vae", type=S.str2bool, default=True)
    p.add_argument("--cfg-scale", type=float, default=1.5)
    p.add_argument("--num-classes", type=int, default=None,
                   help="default: the trained model's num_classes from config.yaml (the reference defaults to 1000 whatever "
                        "the model was trained with; a mismatch would index past its label table)")
    p.add_argument("--num-samples", type=int, default=10_000)
    p.add_argument("--batch-size", type=int, default=128)
    p.add_argument("--num-sampling-steps", type=int, default=250)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--output-file", type=str, default="samples.npz", help="Filename in which to store samples.")
    p.add_argument("--ema-std", type=float, default=0.05)
    p.add_argument("--ckpt", type=str, default=None, help="Checkpoint to load instead of EMA (should not include .pt extension).")
    p.add_argument("--vae-path", type=str, default=None, help="local copy of stabilityai/sd-vae-ft-mse (no network here)")
    p.add_argument("--no-graph", action="store_true", help="eager p_sample_loop instead of the captured hipGraph")
    p.add_argument("--precision", choices=["bf16", "f16", "bf16x3"], default="f16")
    S.add_sampler_flags(p)
    S.add_vae_flags(p)
    p.add_argument("--fid-ref", type=str, default=None, help="reference statistics (.npz with mu and sigma): compute the FID of the samples")
    p.add_argument("--inception-weights", type=str, default=None,
                   help="pt_inception-2015-12-05 weights (.safetensors, or a torch state dict) for --fid-ref")
    p.add_argument("--inception-precision", choices=["f16", "bf16"], default="f16", help="16-bit operand format of the feature network")
    from .metrics import add_metric_flags
    add_metric_flags(p)                                                   # --metrics fid,pr,kid (default fid): pr and kid need pool_3 in --fid-ref
    p.add_argument("--dinov2-ref", type=str, default=None, help="reference statistics (.npz with mu_dinov2 and sigma_dinov2): compute FD-DINOv2")
    p.add_argument("--dinov2-weights", type=str, default=None,
                   help="dinov2_vitl14_pretrain weights (.safetensors, or a torch state dict) for --dinov2-ref")
    p.add_argument("--dinov2-precision", choices=["f16", "bf16"], default="f16", help="16-bit operand format of the DINOv2 network")
    p.add_argument("--shard", type=str, default="0/1",
                   help="R/W with --sample-rng counter: this process takes the batches b with b %% W == R (start W processes by hand or from a job script)")
    return p


# ---- --sample-rng counter: the host logic of parts, shards and resuming (pure functions: no GPU, no model) -----------------------

def parse_shard(text: str):
    """"R/W" -> (R, W); W >= 1 and 0 <= R < W."""
    try:
        r, w = (int(v) for v in str(text).split("/"))
    except ValueError:
        raise ValueError(f"--shard {text}: expected R/W, two integers") from None
    if w < 1 or not 0 <= r < w:
        raise ValueError(f"--shard {text}: needs W >= 1 and 0 <= R < W")
    return r, w


def plan_batches(num_samples: int, batch_size: int, shard=(0, 1)):
    """[(b, first, end)]: the batches b with b % W == R of a run of `num_samples` samples in batches of `batch_size`.  Batch b holds the
    sample indices [first, end) = [b n, min((b + 1) n, num_samples)): the last one is cut where the array is cut."""
    if num_samples < 1 or batch_size < 1:
        raise ValueError(f"--num-samples {num_samples} and --batch-size {batch_size} must both be >= 1")
    r, w = shard
    return [(b, b * batch_size, min((b + 1) * batch_size, num_samples))
            for b in range(-(-num_samples // batch_size)) if b % w == r]


def check_shard_flags(args):
    """Before anything is built: --shard is R/W with R < W, and means something under --sample-rng counter only -> (R, W)."""
    shard = parse_shard(args.shard)
    if args.sample_rng == "counter" and args.seed is None:
        raise ValueError("--sample-rng counter needs a --seed: the seed is the generator's key")
    if shard != (0, 1) and args.sample_rng != "counter":
        raise ValueError(f"--shard {args.shard} needs --sample-rng counter: under the torch generator a sample depends on everything its "
                         "process drew before it, so a run cannot be split")
    return shard


MANIFEST_KEYS = ("sample_rng", "seed", "num_samples", "batch_size", "sampler", "num_sampling_steps", "solver_order", "solver_spacing",
                 "cfg_scale", "precision", "ema_std", "ckpt", "num_classes", "use_vae", "vae_weights", "vae_path", "vae_precision",
                 "vae_norm_groups", "objective", "flow_shift", "graph")


def make_manifest(args, train_args: dict) -> dict:
    """Everything the bytes of a part depend on (the shard is not among them: a part is the same whoever makes it)."""
    vae = bool(args.use_vae)
    return {"sample_rng": "counter/1",                                     # the layout of mapdit.h, "Counter-based sampler draws"
            "seed": args.seed, "num_samples": args.num_samples, "batch_size": args.batch_size, "sampler": args.sampler,
            "num_sampling_steps": args.num_sampling_steps,
            "solver_order": args.solver_order if args.sampler == "dpm++" else None,
            "solver_spacing": args.solver_spacing if args.sampler == "dpm++" else None,
            "cfg_scale": float(args.cfg_scale), "precision": args.precision,
            "ema_std": float(args.ema_std) if args.ckpt is None else None, "ckpt": args.ckpt,
            "num_classes": int(args.num_classes), "use_vae": vae,
            "vae_weights": os.path.abspath(args.vae_weights) if vae and args.vae_weights else None,
            "vae_path": args.vae_path if vae and not args.vae_weights else None,
            "vae_precision": args.vae_precision if vae and args.vae_weights else None,
            "vae_norm_groups": args.vae_norm_groups if vae and args.vae_weights else None,
            "objective": (train_args or {}).get("objective", "diffusion"),
            "flow_shift": float((train_args or {}).get("flow_shift", 1.0)) if args.sampler in S.FLOW_SAMPLERS else None,
            "graph": not args.no_graph}


def check_manifest(old: dict, new: dict):
    """A parts directory holds the batches of ONE run: any key that differs (or is missing on one side) is refused, named with both
    values."""
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new or old[k] != new[k]:
            raise ValueError(f"the parts directory was written by a run with {k} = {old.get(k, '<absent>')!r}; this run has "
                             f"{k} = {new.get(k, '<absent>')!r}.  Parts of two runs do not mix: use another --output-file, or remove the directory")


def parts_dir(result_dir: str, output_file: str) -> str:
    return os.path.join(result_dir, "fid_samples", output_file + ".parts")


def part_path(pdir: str, first: int, end: int) -> str:
    return os.path.join(pdir, f"{first}-{end}.npy")


def _replace_into(path: str, write):
    """Atomic write: `write(file)` into a temporary name beside `path`, then os.replace - a reader sees the old file or the whole new one,
    and two processes writing the same bytes do no harm."""
    tmp = f"{path}.tmp.{os.getpid()}"
    with open(tmp, "wb") as f:
        write(f)
    os.replace(tmp, path)


def part_done(path: str, rows: int, tail) -> bool:
    """A finished part: a readable uint8 array of `rows` images of shape `tail`."""
    if not os.path.isfile(path):
        return False
    try:
        a = np.load(path, mmap_mode="r")
    except (OSError, ValueError):
        return False
    return a.dtype == np.uint8 and a.shape == (rows, *tail)


def open_manifest(pdir: str, manifest: dict):
    """Compare with the directory's manifest.json, or write it (atomically: shards may start together)."""
    import json
    os.makedirs(pdir, exist_ok=True)
    path = os.path.join(pdir, "manifest.json")
    if os.path.isfile(path):
        with open(path) as f:
            check_manifest(json.load(f), manifest)
    else:
        _replace_into(path, lambda f: f.write(json.dumps(manifest, indent=1, sort_keys=True).encode()))


class FidPass:
    """--fid-ref: the one pass of the feature network over the samples (fid.FeaturePass) - the pool statistics, with ``fid_s`` the
    spatial statistics from the same walk, and the ``pool_3`` rows themselves where a metric needs them (isc, pr, kid) - and the
    record made of it.  With the default --metrics it reads, computes and keeps what the FID alone needs.  What can be refused
    (the reference's dimensions, a weight file without the classifier head) was refused by check_fid_flags, before any model."""

    def __init__(self, args, device):
        from . import fid as FID
        from .vae import load_state_dict_file
        self.FID, self.args, self.device = FID, args, device
        self.names = FID.parse_metrics(args.metrics)
        self.spatial = "fid_s" in self.names
        self.ref = FID.load_stats(args.fid_ref, spatial=self.spatial)
        if self.ref[0].shape != (FID.FEATURE_DIM,):
            raise ValueError(f"--fid-ref {args.fid_ref}: statistics of {self.ref[0].shape[0]} dimensions, the pool features have {FID.FEATURE_DIM}")
        sd = getattr(args, "inception_sd", None)                          # (check_fid_flags read it for isc: the file is read once)
        if sd is None and "isc" in self.names:
            sd = load_state_dict_file(args.inception_weights)
        if sd is None:
            net = FID.InceptionFeatures.from_file(args.inception_weights, device, args.inception_precision)
        else:
            net = FID.InceptionFeatures.from_state_dict(sd, device, args.inception_precision)
        self.head = FID.classifier_head(sd) if "isc" in self.names else None
        keep = any(m in self.names for m in FID.FEATURE_METRICS)           # their features stay on the device
        self.run = FID.FeaturePass(net, device, self.spatial, keep)

    @property
    def n(self):
        return self.run.stats.n

    def update(self, images):
        """uint8 [n, H, W, 3] (numpy): the stored bytes."""
        self.run.update(images)

    def record(self, path) -> dict:
        FID, args = self.FID, self.args
        value = FID.frechet_distance(*self.run.stats.mean_cov(), *self.ref[:2])
        record = {"fid": value, "n": self.run.stats.n, "ref": args.fid_ref, "precision": args.inception_precision, "samples": path}
        if self.names != ("fid",):
            extra = {}
            if self.spatial:
                extra["fid_s"] = FID.frechet_distance(*self.run.stats_s.mean_cov(), *self.ref[2:])
            if self.run.feats is not None:
                both = "pr" in self.names or "kid" in self.names
                ref_feat = torch.from_numpy(FID.load_features(args.fid_ref)).to(self.device) if both else None
                extra.update(FID.extra_metrics(ref_feat, torch.cat(self.run.feats), self.names, args, self.head))
            record["metrics"] = extra                                      # (its "precision" is not the record's: that is the operand format)
        return record

    def report(self, record):
        print(f"fid: {record['fid']:.6f}")
        self.FID.print_metrics(record.get("metrics", {}))
        return record["fid"]


def fid_record(args, path, out, device):
    """--fid-ref under --sample-rng counter: the FID and --metrics in one pass over the assembled bytes, in batches of --batch-size from
    index 0 - a function of the stored array alone -> the FID."""
    import json
    fid_pass = FidPass(args, device)
    for i in range(0, len(out), args.batch_size):
        fid_pass.update(out[i:i + args.batch_size])
    record = fid_pass.record(path)
    _replace_into(path + ".fid.json", lambda f: f.write(json.dumps(record).encode()))
    return fid_pass.report(record)


class DinoPass:
    """--dinov2-ref: one pass of the DINOv2 network over the samples' bytes and the record made of it.  What can be refused (half
    of the flag pair, latents, a reference of another dimension) was refused by check_dinov2_flags, before any model."""

    def __init__(self, args, device):
        from . import dinov2 as DINO
        self.DINO, self.args = DINO, args
        self.ref = DINO.load_stats(args.dinov2_ref)
        net = DINO.DinoV2Features.from_state_dict(args.dinov2_sd, device, args.dinov2_precision)
        args.dinov2_sd = None                                              # (the host copy of the weights is not needed again)
        self.run = DINO.FeaturePass(net, device)

    @property
    def n(self):
        return self.run.stats.n

    def update(self, images):
        self.run.update(images)

    def finish(self, path) -> float:
        """Writes ``<samples>.fd_dinov2.json`` and prints ``fd_dinov2:`` -> the value."""
        import json
        value = self.DINO.fd_dinov2(*self.run.stats.mean_cov(), *self.ref)
        record = {"fd_dinov2": value, "n": self.run.stats.n, "ref": self.args.dinov2_ref, "precision": self.args.dinov2_precision, "samples": path}
        _replace_into(path + ".fd_dinov2.json", lambda f: f.write(json.dumps(record).encode()))
        print(f"fd_dinov2: {value:.6f}")
        return value


def dinov2_record(args, path, out, device):
    """--dinov2-ref under --sample-rng counter: FD-DINOv2 of the assembled bytes, in batches of --batch-size from index 0."""
    dino_pass = DinoPass(args, device)
    for i in range(0, len(out), args.batch_size):
        dino_pass.update(out[i:i + args.batch_size])
    return dino_pass.finish(path)


def check_dinov2_flags(args) -> bool:
    """Before anything is built: --dinov2-ref and --dinov2-weights go together, name files, need pixels, and agree on the dimension."""
    if args.dinov2_ref is None and args.dinov2_weights is None:
        return False
    if args.dinov2_ref is None or args.dinov2_weights is None:
        raise ValueError("--dinov2-ref and --dinov2-weights go together: FD-DINOv2 needs the reference statistics and the feature network")
    for flag, path in (("--dinov2-ref", args.dinov2_ref), ("--dinov2-weights", args.dinov2_weights)):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{flag} {path}: no such file")
    if not args.use_vae:
        raise ValueError("--dinov2-ref needs pixels: the feature network reads 3-channel images, --use-vae false writes latents")
    from . import dinov2 as DINO
    from .vae import load_state_dict_file
    mu, _ = DINO.load_stats(args.dinov2_ref)
    args.dinov2_sd = load_state_dict_file(args.dinov2_weights)             # (read once: DinoPass builds the network from it)
    dim = DINO.feature_dim(args.dinov2_sd)
    if mu.shape[0] != dim:
        raise ValueError(f"--dinov2-ref {args.dinov2_ref}: statistics of {mu.shape[0]} dimensions, --dinov2-weights {args.dinov2_weights} is a "
                         f"network of dim {dim}")
    return True


def run_counter(args, train_args, device, want_fid, shard, want_dino=False):
    """main() under --sample-rng counter, from the manifest on.  Returns the parts directory while parts are missing, else what main()
    returns: the FID with --fid-ref, the .npz path without."""
    n = args.batch_size
    pdir = parts_dir(args.result_dir, args.output_file)
    open_manifest(pdir, make_manifest(args, train_args))                  # a differing run is refused here, before any model is built
    size, chans = int(train_args["input_size"]), int(train_args["in_channels"])
    tail = (8 * size, 8 * size, 3) if args.use_vae else (size, size, chans)
    todo = [(b, first, end) for b, first, end in plan_batches(args.num_samples, n, shard)
            if not part_done(part_path(pdir, first, end), end - first, tail)]
    if todo:
        rng = S.make_rng(args, device)
        model = get_model(train_args).to(device)
        S.load_weights(model, args.result_dir, args.ema_std, args.ckpt, verbose=False)
        model.gemm_precision = args.precision
        vae = S.load_vae(args.vae_path, device, args.vae_weights, args.vae_precision, args.vae_norm_groups) if args.use_vae else None
        diffusion, solver = S.make_diffusion(args, train_args)
        use_cfg = args.cfg_scale > 1.0
        shape = (2 * n if use_cfg else n, chans, size, size)
        null = torch.full((n,), args.num_classes, device=device, dtype=torch.int64)
        graphed = None
        for b, first, end in todo:
            index = list(range(b * n, (b + 1) * n))                       # the whole batch: indices beyond --num-samples are drawn and dropped
            z, y = rng.latents(index, shape[1:]), rng.labels(index, args.num_classes)
            if use_cfg:
                z, y = torch.cat([z, z], dim=0), torch.cat([y, null], dim=0)
            if args.no_graph:
                samples = S.run_sampler(model, diffusion, z, y, args.cfg_scale if use_cfg else None, use_graph=False, rng=rng, index=index,
                                        **solver)
            else:
                if graphed is None:
                    graphed = S.GraphedSampler(model, diffusion, shape, y, args.cfg_scale if use_cfg else None, rng=rng, **solver)
                graphed.y.copy_(y)
                samples = graphed.sample(z, index=index)
            if use_cfg:
                samples, _ = samples.chunk(2, dim=0)
            samples = S.denormalize(samples, train_args)
            if vae is not None:
                samples = vae.decode(samples).sample
            arr = np.ascontiguousarray(S.to_uint8_nhwc(samples)[: end - first])
            assert arr.shape == (end - first, *tail), (arr.shape, tail)
            _replace_into(part_path(pdir, first, end), lambda f: np.save(f, arr))
    every = plan_batches(args.num_samples, n)
    missing = [(first, end) for _, first, end in every if not part_done(part_path(pdir, first, end), end - first, tail)]
    if missing:
        print(f"{len(every) - len(missing)} of {len(every)} parts in {pdir}; missing sample ranges: " + ", ".join(f"{a}-{e}" for a, e in missing))
        return pdir
    out = np.concatenate([np.load(part_path(pdir, first, end)) for _, first, end in every], axis=0)
    path = os.path.join(args.result_dir, "fid_samples", args.output_file)
    if not path.endswith(".npz"):
        path += ".npz"                                                     # (np.savez appends it to a name; a file object takes none)
    _replace_into(path, lambda f: np.savez(f, arr_0=out))
    result = fid_record(args, path, out, device) if want_fid else path
    if want_dino:
        dinov2_record(args, path, out, device)
    return result


def check_fid_flags(args) -> bool:
    """Before anything is built: --fid-ref and --inception-weights go together, name files, and need pixels."""
    from .metrics import parse_metrics
    metrics = getattr(args, "metrics", None)
    names = parse_metrics(metrics)                                        # (an unknown name is refused here too)
    if args.fid_ref is None and args.inception_weights is None:
        if metrics is not None:
            raise ValueError(f"--metrics {metrics} needs --fid-ref and --inception-weights: the metrics compare the samples with a reference")
        return False
    if args.fid_ref is None or args.inception_weights is None:
        raise ValueError("--fid-ref and --inception-weights go together: the FID needs the reference statistics and the feature network")
    for flag, path in (("--fid-ref", args.fid_ref), ("--inception-weights", args.inception_weights)):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{flag} {path}: no such file")
    if not args.use_vae:
        raise ValueError("--fid-ref needs pixels: the feature network reads 3-channel images, --use-vae false writes latents")
    if "fid_s" in names:
        from .fid import has_spatial
        if not has_spatial(args.fid_ref):
            raise ValueError(f"--metrics {metrics}: fid_s needs the reference's spatial statistics: --fid-ref {args.fid_ref} holds no 'mu_s' / "
                             "'sigma_s'; write them with `python -m mapdit_amd.fid stats --spatial --images A.npz --inception-weights FILE "
                             "--output ref.npz`")
    if "pr" in names or "kid" in names:                                   # (isc is the samples' own: it reads the head of --inception-weights)
        from .fid import features_rows
        rows = features_rows(args.fid_ref)
        if rows is None:
            raise ValueError(f"--metrics {metrics} needs the reference's features: --fid-ref {args.fid_ref} holds no 'pool_3'; write one with "
                             "`python -m mapdit_amd.fid features --images A.npz --inception-weights FILE --output feats.npz`")
        if "kid" in names and args.kid_subset_size > min(rows, args.num_samples):
            raise ValueError(f"--metrics {metrics}: --kid-subset-size {args.kid_subset_size} exceeds the smaller set (--num-samples "
                             f"{args.num_samples}, {rows} reference features)")
    if "fid_s" in names:
        from .fid import spatial_dim
        with np.load(args.fid_ref) as z:
            got = z["mu_s"].shape
        if got != (spatial_dim(),):
            raise ValueError(f"--metrics {metrics}: --fid-ref {args.fid_ref} holds spatial statistics of shape {got}, the spatial features have "
                             f"{spatial_dim()} dimensions")
    if "isc" in names:                                                    # a file without fc.weight is a KeyError here, not after the sampling
        from .fid import classifier_head
        from .vae import load_state_dict_file
        args.inception_sd = load_state_dict_file(args.inception_weights)
        classifier_head(args.inception_sd)
    return True


@torch.no_grad()          # the reference switches autograd off globally (torch.set_grad_enabled(False)); scoped here
def main(argv=None):
    args = build_parser().parse_args(argv)
    S.check_vae_flags(args)                                               # a missing --vae-weights file ends the run before any model is built
    want_fid = check_fid_flags(args)                                      # (so does half of the FID flag pair)
    want_dino = check_dinov2_flags(args)                                  # (and half of the FD-DINOv2 pair, or a reference of another dimension)
    shard = check_shard_flags(args)                                       # (and a --shard that is no R/W with R < W, or has no counter rng)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    device = torch.device("cuda")
    train_args = S.load_train_args(args.result_dir)
    S.check_objective(args.sampler, train_args)                           # a velocity model and a diffusion sampler (or the reverse): refused here
    if args.num_classes is None:
        args.num_classes = int(train_args["num_classes"])
    elif args.num_classes != int(train_args["num_classes"]):
        raise ValueError(f"--num-classes {args.num_classes} != the trained model's num_classes {train_args['num_classes']} "
                         "(config.yaml): labels and the null label would fall outside its embedding table")
    if args.sample_rng == "counter":
        return run_counter(args, train_args, device, want_fid, shard, want_dino)
    model = get_model(train_args).to(device)
    S.load_weights(model, args.result_dir, args.ema_std, args.ckpt, verbose=False)
    model.gemm_precision = args.precision
    vae = S.load_vae(args.vae_path, device, args.vae_weights, args.vae_precision, args.vae_norm_groups) if args.use_vae else None
    diffusion, solver = S.make_diffusion(args, train_args)
    fid_pass = FidPass(args, device) if want_fid else None
    dino_pass = DinoPass(args, device) if want_dino else None

    n = args.batch_size
    use_cfg = args.cfg_scale > 1.0
    shape = (2 * n if use_cfg else n, train_args["in_channels"], train_args["input_size"], train_args["input_size"])
    graphed = None
    gathered = []
    for _ in range(math.ceil(args.num_samples / n)):
        z = torch.randn(n, *shape[1:], device=device)
        y = torch.randint(0, args.num_classes, (n,), device=device)
        if use_cfg:                                                       # sample_fid.py:56-62
            z = torch.cat([z, z], dim=0)
            y = torch.cat([y, torch.tensor([args.num_classes] * n, device=device)], dim=0)
        if args.no_graph:
            samples = S.run_sampler(model, diffusion, z, y, args.cfg_scale if use_cfg else None, use_graph=False, **solver)
        else:
            if graphed is None:
                graphed = S.GraphedSampler(model, diffusion, shape, y, args.cfg_scale if use_cfg else None, **solver)
            graphed.y.copy_(y)
            samples = graphed.sample(z)
        if use_cfg:
            samples, _ = samples.chunk(2, dim=0)
        samples = S.denormalize(samples, train_args)
        if vae is not None:
            samples = vae.decode(samples).sample
        gathered.append(S.to_uint8_nhwc(samples))
        if want_fid:                                                      # the stored bytes, cut where the array is cut
            keep = min(len(gathered[-1]), args.num_samples - fid_pass.n)
            if keep > 0:
                fid_pass.update(gathered[-1][:keep])
        if want_dino:                                                     # one more pass over the same bytes
            keep = min(len(gathered[-1]), args.num_samples - dino_pass.n)
            if keep > 0:
                dino_pass.update(gathered[-1][:keep])
    out = np.concatenate(gathered, axis=0)[: args.num_samples]
    os.makedirs(os.path.join(args.result_dir, "fid_samples"), exist_ok=True)
    path = os.path.join(args.result_dir, "fid_samples", args.output_file)
    np.savez(path, arr_0=out)
    if want_dino:
        dino_pass.finish(path)
    if want_fid:
        import json
        record = fid_pass.record(path)
        with open(path + ".fid.json", "w") as f:
            json.dump(record, f)
        return fid_pass.report(record)
    return path


if __name__ == "__main__":
    main()
