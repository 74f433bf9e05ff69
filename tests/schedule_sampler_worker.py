"""Child-process worker of tests/test_schedule_sampler_gpu.py: one data-parallel rank (gloo collectives, the ranks share one GPU) feeding
a LossSecondMomentResampler through update_with_local_losses.

    python -m torch.distributed.run ... tests/schedule_sampler_worker.py OUT_DIR

T = 37, H = 3.  In each of ROUNDS rounds every rank feeds its OWN entries (rank_batch below: a permutation of all timesteps and three
repeats, so two rounds fill every row and the third shifts every row), then draws.  Writes the history, the counts and the probability
table of the last draw to OUT_DIR/rank{r}.pt.  Imported, it provides rank_batch for the test's replay through the restatement.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

T, H, ROUNDS, DRAWS = 37, 3, 3, 8


def rank_batch(rank, rnd):
    """(ts int64 [40], losses fp32 [40]) of one rank in one round."""
    rng = np.random.default_rng([7, rank, rnd])
    ts = np.concatenate([rng.permutation(T), rng.integers(0, T, size=3)]).astype(np.int64)
    return ts, rng.lognormal(-1.0 + rank, 1.0, size=ts.size).astype(np.float32)


def main(out_dir):
    import mapdit_amd  # noqa: F401
    from mapdit_amd import parallel
    from mapdit_amd.diffusion.timestep_sampler import LossSecondMomentResampler
    rank, world, _ = parallel.init_from_env()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    s = LossSecondMomentResampler(types.SimpleNamespace(num_timesteps=T), history_per_term=H)
    gen = torch.Generator(device=dev).manual_seed(100 + rank)
    for rnd in range(ROUNDS):
        ts, losses = rank_batch(rank, rnd)
        s.update_with_local_losses(torch.from_numpy(ts).to(dev), torch.from_numpy(losses).to(dev))
        t, w = s.sample(DRAWS, dev, generator=gen)
    torch.cuda.synchronize()
    sd = s.state_dict()
    torch.save({"hist": sd["loss_history"], "counts": sd["loss_counts"], "prob": s._prob.cpu(), "cdf": s._cdf.cpu(), "t": t.cpu(), "w": w.cpu(),
                "world": world}, os.path.join(out_dir, f"rank{rank}.pt"))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
