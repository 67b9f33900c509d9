"""Worker for tests/test_hip_mixed_step.py: python _mixed_dp_worker.py RANK WORLD INIT_METHOD OUTFILE.
Both ranks share cuda:0 (one-GPU box), so the collectives run over gloo; the accumulator, the per-step reduction and the
bucket order are the ones the RCCL path uses.  Step 1: rank 0 holds fixture samples 0, 1 (x2) and 2 (x3), rank 1 sample 4 (x6).
Step 2: rank 0 holds samples 0 and 1, rank 1 none."""
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
    episodes = []
    begin = dp.reducer.begin
    dp.reducer.begin = lambda *a, **k: (episodes.append(1), begin(*a, **k))[1]
    opt = harness.make_optimizer(model, 1e-4)
    mine = [[0, 1, 2], [4]][rank]
    lrs, hrs = ([torch.from_numpy(d[f"{k}_u8_{i}"]).float().div(255.0).unsqueeze(0).cuda() for i in mine] for k in ("lr", "hr"))
    loss = harness.train_step_samples(model, opt, lrs, hrs, group=False, b_global=4)
    rec = {"grads": {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None},
           "loss": loss.item(), "launched_order": list(dp.reducer.launched_order), "nbuckets": len(dp.reducer.bucket_ranges),
           "reducer_restored": model._grad_reducer is dp.reducer}
    mine = [[0, 1], []][rank]
    harness.train_step_samples(model, opt, lrs[:len(mine)], hrs[:len(mine)], b_global=2)
    rec["step2_launched_order"] = list(dp.reducer.launched_order)
    rec["step2_grad_names"] = [k for k, p in model.named_parameters() if p.grad is not None]
    rec["episodes"] = len(episodes)
    torch.save(rec, f"{outfile}.{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()
    print(f"RANK{rank} OK", flush=True)


if __name__ == "__main__":
    main()
