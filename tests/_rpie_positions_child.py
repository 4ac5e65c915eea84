"""Child process of test_deterministic_mode_gives_bit_identical_positions:
two rpie epochs with position correction at 256^2 x 8 modes with eigen
weights, then on a two-slice object; prints one JSON line with a hash of
every result.  The parent runs it twice under TIKE_DETERMINISTIC=1."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import tike_amd.ptycho as tp  # noqa: E402
import tike_amd.random  # noqa: E402
from test_rpie_positions_gpu import ADAM, _parameters, _problem  # noqa: E402


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out = {}
    for tag, depth, S, N, eigen in (("", 1, 8, 12, True), ("2", 2, 3, 10, False)):
        det = 256
        true, scan0, psi0, probe0, ep, ew, data = _problem(
            tp, det, S, N, 17 + depth, eigen, depth)
        params = _parameters(tp, scan0, psi0, probe0, ep, ew, num_batch=2,
                             method="compact", popts=ADAM)
        tike_amd.random.randomizer_np = np.random.default_rng(11)
        with tp.Reconstruction(data, params, order=np.arange(N),
                               batches=np.array_split(np.arange(N), 2)) as ctx:
            ctx.iterate(2)
            r = ctx.get_result()
        out["scan" + tag] = digest(r.scan)
        out["psi" + tag] = digest(r.psi)
        out["probe" + tag] = digest(r.probe)
        out["moved" + tag] = float(np.abs(r.scan - scan0).max())
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
