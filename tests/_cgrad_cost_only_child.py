"""Child process of tests/test_cgrad_cost_only_gpu.py: two cgrad epochs with
nothing recovered on every case of that module; the iterates, the costs and
the reference cost go into the .npz named on the command line.  The parent
runs it under TIKE_DETERMINISTIC=1."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import tike_amd.ptycho as tp  # noqa: E402
from test_cgrad_cost_only_gpu import CASES, run  # noqa: E402

out = {}
for case in sorted(CASES):
    got, want = run(tp, CASES[case](tp))
    out.update({f"{case}_psi": got.psi, f"{case}_probe": got.probe,
                f"{case}_scan": got.scan, f"{case}_want": want,
                f"{case}_costs": np.ravel(got.algorithm_options.costs)})
np.savez(sys.argv[1], **out)
