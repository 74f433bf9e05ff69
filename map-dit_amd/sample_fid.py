"""MI355X counterpart of the reference's ``sample_fid.py``: ``--num-samples`` images in batches of ``--batch-size`` with
random labels (classifier-free guidance when ``--cfg-scale`` > 1), stored as one uint8 NHWC array ``arr_0`` in
``<result-dir>/fid_samples/<output-file>`` (reference sample_fid.py:48-97; flags :100-114).  One hipGraph is captured for
the batch shape and replayed for every batch (``--sampler dpm++``: DPM-Solver++ with ``--num-sampling-steps`` model evaluations).  Without a VAE (``--use-vae false``) the array holds the de-normalised
latents clamped to [-1, 1] and quantised the same way; with ``--vae-weights FILE`` the native VAE decoder (map-dit_amd/vae.py) turns
them into pixels first (``arr_0``: [n, 8S, 8S, 3]).  ``--fid-ref REF.npz --inception-weights FILE`` (together, and with pixels): the
FID of the samples against the reference statistics, accumulated batch by batch on the device (map-dit_amd/fid.py), printed, returned
and written to ``fid_samples/<output-file>.fid.json``; the array is written as before.  ``--metrics fid,pr,kid`` (default ``fid``)
adds precision / recall / density / coverage and KID (map-dit_amd/metrics.py) to that file (under its key ``metrics``) and to the output: ``--fid-ref`` must then
be a file of ``python -m mapdit_amd.fid features`` (it holds ``pool_3``); the samples' features stay on the device."""
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
    return p


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
    if names != ("fid",):
        from .fid import features_rows
        rows = features_rows(args.fid_ref)
        if rows is None:
            raise ValueError(f"--metrics {metrics} needs the reference's features: --fid-ref {args.fid_ref} holds no 'pool_3'; write one with "
                             "`python -m mapdit_amd.fid features --images A.npz --inception-weights FILE --output feats.npz`")
        if "kid" in names and args.kid_subset_size > min(rows, args.num_samples):
            raise ValueError(f"--metrics {metrics}: --kid-subset-size {args.kid_subset_size} exceeds the smaller set (--num-samples "
                             f"{args.num_samples}, {rows} reference features)")
    return True


@torch.no_grad()          # the reference switches autograd off globally (torch.set_grad_enabled(False)); scoped here
def main(argv=None):
    args = build_parser().parse_args(argv)
    S.check_vae_flags(args)                                               # a missing --vae-weights file ends the run before any model is built
    want_fid = check_fid_flags(args)                                      # (so does half of the FID flag pair)
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
    model = get_model(train_args).to(device)
    S.load_weights(model, args.result_dir, args.ema_std, args.ckpt, verbose=False)
    model.gemm_precision = args.precision
    vae = S.load_vae(args.vae_path, device, args.vae_weights, args.vae_precision, args.vae_norm_groups) if args.use_vae else None
    diffusion, solver = S.make_diffusion(args, train_args)
    if want_fid:
        from . import fid as FID
        ref_mu, ref_sigma = FID.load_stats(args.fid_ref)
        if ref_mu.shape != (FID.FEATURE_DIM,):
            raise ValueError(f"--fid-ref {args.fid_ref}: statistics of {ref_mu.shape[0]} dimensions, the pool features have {FID.FEATURE_DIM}")
        fid_net = FID.InceptionFeatures.from_file(args.inception_weights, device, args.inception_precision)
        fid_stats = FID.FeatureStats(FID.FEATURE_DIM, device)
        metric_names = FID.parse_metrics(args.metrics)
        keep_feats = metric_names != ("fid",)                             # pr / kid: the samples' features stay on the device
        feats = []

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
            keep = min(len(gathered[-1]), args.num_samples - fid_stats.n)
            if keep > 0:
                feat = fid_net.features(torch.from_numpy(gathered[-1][:keep]).to(device))
                fid_stats.update(feat)
                if keep_feats:
                    feats.append(feat)
    out = np.concatenate(gathered, axis=0)[: args.num_samples]
    os.makedirs(os.path.join(args.result_dir, "fid_samples"), exist_ok=True)
    path = os.path.join(args.result_dir, "fid_samples", args.output_file)
    np.savez(path, arr_0=out)
    if want_fid:
        import json
        value = FID.frechet_distance(*fid_stats.mean_cov(), ref_mu, ref_sigma)
        record = {"fid": value, "n": fid_stats.n, "ref": args.fid_ref, "precision": args.inception_precision, "samples": path}
        extra = {}
        if keep_feats:
            ref_feat = torch.from_numpy(FID.load_features(args.fid_ref)).to(device)
            extra = FID.extra_metrics(ref_feat, torch.cat(feats), metric_names, args)
            record["metrics"] = extra                                      # (its "precision" is not the record's: that is the operand format)
        with open(path + ".fid.json", "w") as f:
            json.dump(record, f)
        print(f"fid: {value:.6f}")
        for k, v in extra.items():
            print(f"{k}: {v:.6f}")
        return value
    return path


if __name__ == "__main__":
    main()
