"""Child-process worker of tests/test_grad_clip_gpu.py: one data-parallel rank (gloo collectives, the ranks share one GPU) of ONE clipped
optimiser step on the fixture tiny_a.

    python -m torch.distributed.run ... tests/grad_clip_worker.py OUT_DIR MODE        (MODE: allreduce | zero1)

Each rank runs forward and backward on its half of the batch; after the exchange the flat gradient buffer holds the sum over the ranks
(under gloo the ZeRO-1 reducer all-reduces whole stage slices too).  max_grad_norm is set to half of that gradient's norm, computed on
the host from the same bits on every rank, so the coefficient is about 0.5.  Writes parameters (gathered), the summed gradients and the
device's {norm, coef} to OUT_DIR/rank{r}.pt.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(out_dir, mode):
    import mapdit_amd  # noqa: F401
    from grad_accum_worker import fixture_model, mean_loss
    from grad_clip_reference import clip64, f32
    from mapdit_amd import parallel
    from mapdit_amd.optim import FusedAdamEMA
    rank, world, _ = parallel.init_from_env()
    torch.cuda.set_device(0)
    # (train mode without the forced in-place rewrite, as tests/grad_accum_worker.py: the forwards must see the same weights)
    m, _, (x, t, y, noise) = fixture_model("tiny_a", "bf16", train=True, forced_weight_normalization=False)
    red = parallel.make_reducer(m, mode)
    opt = FusedAdamEMA(m, lr=1e-2, betas=(0.9, 0.99), ema_stds=(0.05, 0.1), grad_scale=red.grad_scale, max_grad_norm=1.0)
    red.attach(opt)
    assert (opt.norm_sync is not None) == (mode == "zero1" and world > 1)
    lo, hi = parallel.shard_batch(x.shape[0], rank, world)
    opt.zero_grad()
    mean_loss(m, (x[lo:hi], t[lo:hi], y[lo:hi], noise[lo:hi])).backward()
    red.finish()
    torch.cuda.synchronize()
    summed = m._gflat.cpu()
    norm, _ = clip64(summed.numpy(), f32(opt.grad_scale), np.inf)
    opt.max_grad_norm = f32(0.5 * norm)
    opt.step()
    red.gather_state()
    torch.cuda.synchronize()
    assert torch.equal(m._gflat.cpu(), summed)                     # the step does not rewrite the gradients
    torch.save({"p": m._pflat.cpu(), "g": summed, "clip": opt._clip.cpu(), "norm": opt.grad_norm(), "coef": opt.clip_coef(),
                "max_norm": opt.max_grad_norm, "grad_scale": f32(opt.grad_scale), "shards": list(opt.shards)},
               os.path.join(out_dir, f"rank{rank}.pt"))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
