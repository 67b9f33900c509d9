"""Worker for tests/test_hip_ema.py: python _ema_dp_worker.py RANK WORLD INIT_METHOD OUTFILE.
Both ranks share cuda:0 (one-GPU box), so the collectives run over gloo, as in _step_guard_dp_worker.py, whose three guarded steps
these are (step 2 carries a NaN pixel on rank 0 and is skipped on both ranks), here with the weight average on.  The average is a
function of the parameters alone, so no collective carries it: every rank records its averaged weights, its update count, its
guard counts and its final parameters."""
import faulthandler
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, init, outfile = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    faulthandler.dump_traceback_later(300, exit=True)        # a stall leaves every thread's stack on stderr
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    from transformerupscaler_amd import harness
    from transformerupscaler_amd.dp import DataParallel
    from transformerupscaler_amd.weights import deterministic_state_dict
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "train_mixed_step.npz"), allow_pickle=False))
    model = importlib.import_module("models.FastTransformer.model").TransformerModel()
    model.load_state_dict(deterministic_state_dict(0), strict=False)
    model = model.cuda().eval()
    dp = DataParallel(model, scales=(2, 3, 4, 6), bucket_mb=2.0)
    opt = harness.make_ema_optimizer(model, 0.9, ema_warmup=True, lr=1e-4, max_grad_norm=1e-3, skip_nonfinite=True)
    mine = [[0, 1, 2], [4]][rank]
    lrs, hrs = ([torch.from_numpy(d[f"{k}_u8_{i}"]).float().div(255.0).unsqueeze(0).cuda() for i in mine] for k in ("lr", "hr"))
    bad = [t.clone() for t in lrs]
    if rank == 0:
        bad[0][0, 2, 3, 5] = float("nan")
    for batch in (lrs, bad, lrs):
        harness.train_step_samples(model, opt, batch, hrs, group=False, b_global=4)
    params = dict(model.named_parameters())
    rec = {"updates": opt.ema_updates, "stats": opt.guard_stats(),
           "ema": {k: v.cpu() for k, v in opt.ema_state_dict(model).items() if k in params},
           "params": {k: p.detach().cpu().clone() for k, p in params.items()}}
    torch.save(rec, f"{outfile}.{rank}.pt")
    dist.barrier()
    dp.detach()
    dist.destroy_process_group()
    print(f"RANK{rank} OK", flush=True)


if __name__ == "__main__":
    main()
