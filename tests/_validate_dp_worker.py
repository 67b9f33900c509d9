"""Worker for tests/test_hip_validate.py: python _validate_dp_worker.py RANK WORLD INIT_METHOD -- <train.py arguments>.
Both ranks share cuda:0 (one-GPU box), so the process group is gloo, set up here; the driver then runs in this process (it takes a
group that already exists) as rank RANK of WORLD.  Rank 0 writes the driver's --json record."""
import faulthandler
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, init = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    argv = sys.argv[sys.argv.index("--") + 1:]
    faulthandler.dump_traceback_later(300, exit=True)        # a stall leaves every thread's stack on stderr
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    import train
    train.main(argv)
    print(f"RANK{rank} OK", flush=True)


if __name__ == "__main__":
    main()
