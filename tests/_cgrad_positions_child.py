"""Child process of test_cgrad_positions_gpu.test_deterministic_mode: two
cgrad epochs at 256^2 x 2 modes (poisson, a mask, ADAM) with position
correction, with an update_start beyond the run and with no position_options;
then the new chunk entry next to the old one.  Prints one JSON line with a
hash of every result.  The parent runs it under TIKE_DETERMINISTIC=1."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import cgrad_positions as cp  # noqa: E402
import rpie_positions as rp  # noqa: E402
import tike_amd.ptycho as tp  # noqa: E402
import tike_amd.random  # noqa: E402
from test_cgrad_positions_gpu import _parameters  # noqa: E402


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    det, S, N = 256, 2, 8
    true, psi_true, probe, data, mask, rng = cp.problem(det, det, S, N, 23,
                                                        masked=True)
    scan0 = (true + rp.jitter(rng, true.shape)).astype(np.float32)
    psi0 = cp.start(psi_true)
    batches = np.array_split(np.arange(N), 2)
    moment = dict(use_adaptive_moment=True, update_magnitude_limit=1.0)
    out = {}
    for tag, popts, positions in (("", moment, True),
                                  ("_late", dict(update_start=5, **moment),
                                   True), ("_off", {}, False)):
        params = _parameters(tp, scan0, psi0, probe, mask, "poisson",
                             popts=popts, positions=positions)
        tike_amd.random.randomizer_np = np.random.default_rng(11)
        with tp.Reconstruction(data, params, order=np.arange(N),
                               batches=batches) as ctx:
            ctx.iterate(2)
            r = ctx.get_result()
        out["scan" + tag] = digest(r.scan)
        out["psi" + tag] = digest(r.psi)
        out["probe" + tag] = digest(r.probe)
        out["costs" + tag] = digest(np.array(r.algorithm_options.costs))
        if tag == "":
            out["moved"] = float(np.abs(r.scan - scan0).max())
    old = cp.entry_run(psi0, scan0, probe, data, mask, "poisson",
                       positions=False)
    new = cp.entry_run(psi0, scan0, probe, data, mask, "poisson")
    out["entry_equal"] = {k: bool(np.array_equal(old[k], new[k]))
                          for k in ("costs", "mpu", "acc")}
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
