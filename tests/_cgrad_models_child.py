"""Child process of test_cgrad_poisson_mask_deterministic_children_bit_identical:
two poisson + mask cgrad epochs at 256^2 (all-at-once device line search),
the iterates and costs saved to the .npz named on the command line."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import cgrad_models as cm  # noqa: E402
import tike_amd.ptycho as tp  # noqa: E402
from test_cgrad_models_gpu import _problem, _run, _start  # noqa: E402

det, N = 256, 10
mask = cm.detector_mask(det)
scan, psi_true, probe, data = _problem(tp, det, det, 2, N, 21, mask)
r = _run(tp, data, scan, _start(psi_true), probe, "poisson", mask)
np.savez(sys.argv[1], psi=r.psi, probe=r.probe,
         costs=np.array(r.algorithm_options.costs))
