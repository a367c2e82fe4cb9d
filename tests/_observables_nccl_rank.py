"""One rank of an RCCL (backend "nccl") group that all-reduces hand-made observables.Totals -- the child process of
tests/test_gpu_observables.py::test_all_reduce_under_rccl.  Usage: python _observables_nccl_rank.py PORT [RANK WORLD]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
from waveflow_amd import observables as obs  # noqa: E402


def totals(seed):
    g = np.random.default_rng(seed)
    return obs.Totals(3, 7, 5, -2.0, 1.5, sums=g.normal(size=(5, 2)) * 1e3, counts=g.integers(0, 1 << 40, size=4),
                      density=g.integers(0, 1 << 40, size=(3, 7)), pair=g.integers(0, 1 << 40, size=5))


def main():
    port = int(sys.argv[1])
    rank, world = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (0, 1)
    torch.cuda.set_device(rank % torch.cuda.device_count())
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        got = totals(10 + rank).all_reduce()
        want = totals(10)
        for r in range(1, world):
            want.merge(totals(10 + r))
        for k in ("sums", "counts", "density", "pair"):
            a, b = getattr(got, k), getattr(want, k)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
        print(f"__ALL_REDUCE_OK__ rank {rank} of {world}, backend {dist.get_backend()}", flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
