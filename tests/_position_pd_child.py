"""One rank of test_position_pd_gpu's two-rank tests:

    _position_pd_child.py RANK WORLD STORE STEP

joins a gloo group of WORLD ranks on one GPU (WORLD > 1), opens a
Reconstruction over the (128, 128, 2, 10) problem of tests/position_pd.py and
calls `update_positions_pd(step=STEP)`.  Prints one JSON line: the scan of the
whole job before and after, the cost, and the message of a ValueError."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import position_pd as pp  # noqa: E402
import tike_amd.ptycho as tp  # noqa: E402
from test_position_pd_gpu import _parameters  # noqa: E402


def main():
    rank, world, store, step = (int(sys.argv[1]), int(sys.argv[2]),
                                sys.argv[3], float(sys.argv[4]))
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"file://{store}",
                                rank=rank, world_size=world)
    N = 10
    P = pp.problem(128, 128, 2, N)
    out = dict(raised=None, cost=None)
    with tp.Reconstruction(P["data"], _parameters(tp, P), order=np.arange(N),
                           batches=np.array_split(np.arange(N), 2)) as ctx:
        out["scan0"] = ctx.get_scan().tolist()
        try:
            out["cost"] = ctx.update_positions_pd(step=step)
        except ValueError as e:
            out["raised"] = str(e)
        out["scan"] = ctx.get_scan().tolist()
    print("RESULT " + json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
