"""One rank of test_cgrad_multislice_gpu's two-rank test:

    _cgrad_multislice_child.py RANK WORLD STORE OUT

joins a gloo group of WORLD ranks on one GPU (WORLD > 1) and reconstructs the
two-slice 32^2 problem of tests/cgrad_multislice.py (gaussian, masked, object
and probe) with cgrad in two minibatches of 1 and 8 positions: with two ranks
the second rank's share of the first minibatch is empty.  Writes psi, probe
and costs to OUT (.npz)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cgrad_multislice as ms  # noqa: E402
import fly_scan as fs  # noqa: E402
import tike_amd.ptycho as tp  # noqa: E402
from test_cgrad_multislice_gpu import parameters  # noqa: E402


def main():
    rank, world, store, out = (int(sys.argv[1]), int(sys.argv[2]),
                               sys.argv[3], sys.argv[4])
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"file://{store}",
                                rank=rank, world_size=world)
    K = ms.SOLVER_CASES["general32_d2"]
    P = ms.problem(**K)
    mask = fs.block_mask(K["pw"])
    data = fs.masked(P["data"], mask)
    N = len(P["scan"])
    params = parameters(tp, P, "gaussian", mask, True, epochs=2)
    with tp.Reconstruction(data, params, order=np.arange(N),
                           batches=[np.arange(0, 1), np.arange(1, N)],
                           spatial_sort=False) as ctx:
        shares = [len(b) for b in ctx.batches]
        ctx.iterate(2)
        r = ctx.get_result()
    np.savez(out, psi=r.psi, probe=r.probe,
             costs=np.array(r.algorithm_options.costs), shares=shares,
             scan=r.scan)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
