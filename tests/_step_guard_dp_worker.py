"""Worker for tests/test_hip_step_guard.py: python _step_guard_dp_worker.py RANK WORLD INIT_METHOD OUTFILE.
Both ranks share cuda:0 (one-GPU box), so the collectives run over gloo, as in _mixed_dp_worker.py.  Three guarded steps
(clipping + skip_nonfinite): step 1, rank 0 holds fixture samples 0, 1 (x2) and 2 (x3), rank 1 sample 4 (x6); step 2, rank 0's
first sample carries a NaN pixel (rank 1's is clean: it learns of the NaN through the reduced gradients only); step 3 is step 1
again.  Every rank records the bits of `optimizer.grad_norm` after each step, its guard counts and its final parameters."""
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
    initial = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    dp = DataParallel(model, scales=(2, 3, 4, 6), bucket_mb=2.0)
    opt = harness.make_optimizer(model, 1e-4, max_grad_norm=1e-3, skip_nonfinite=True)
    mine = [[0, 1, 2], [4]][rank]
    lrs, hrs = ([torch.from_numpy(d[f"{k}_u8_{i}"]).float().div(255.0).unsqueeze(0).cuda() for i in mine] for k in ("lr", "hr"))
    bad = [t.clone() for t in lrs]
    if rank == 0:
        bad[0][0, 2, 3, 5] = float("nan")
    norm_bits, norms, unchanged = [], [], True
    for step, batch in enumerate([lrs, bad, lrs]):
        if step == 1:
            opt.guard_stats()                                # settle, so that `step` counts are comparable
            before = {k: p.detach().clone() for k, p in model.named_parameters()}
            before_state = {k: {n: v.clone() for n, v in opt.state[p].items()} for k, p in model.named_parameters() if p in opt.state}
        harness.train_step_samples(model, opt, batch, hrs, group=False, b_global=4)
        norm = opt.grad_norm.clone()
        norm_bits.append(int(norm.view(torch.int32).item()))
        norms.append(float(norm.item()))
        if step == 1:
            opt.guard_stats()
            for k, p in model.named_parameters():
                unchanged &= bool(torch.equal(p.detach(), before[k]))
                if k in before_state:
                    unchanged &= all(bool(torch.equal(opt.state[p][n], v)) for n, v in before_state[k].items())
    rec = {"norm_bits": norm_bits, "norms": norms, "stats": opt.guard_stats(), "skipped_step_unchanged": unchanged, "initial": initial,
           "params": {k: p.detach().cpu().clone() for k, p in model.named_parameters()}}
    torch.save(rec, f"{outfile}.{rank}.pt")
    dist.barrier()
    dp.detach()
    dist.destroy_process_group()
    print(f"RANK{rank} OK", flush=True)


if __name__ == "__main__":
    main()
