"""Child process of test_products_deterministic_mode: tike_pfa_inv_products at
96^2, 17 positions under tike_set_deterministic (process-wide, hence a fresh
process) with scratch of three sizes, and prints one JSON line."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import pfa_cases as pc  # noqa: E402
import pfa_model as pm  # noqa: E402
from devbuf import Dev, dev, dptr  # noqa: E402
from util import OP_MAXABS, OP_NORMWISE, maxerr, relerr  # noqa: E402


def main():
    import tike_amd._arrays as A
    from tike_amd._lib import lib
    det = pw = 96
    S, nscan = 3, 17
    g = pm.Geom(det)
    rng = np.random.default_rng(17)
    sub = pc.rc(rng, nscan, S, g.p, g.p, g.M, g.M)
    patches = pc.rc(rng, nscan, pw, pw)
    mpu0 = pc.rc(rng, S, pw, pw)
    pr = pc.probe_case("eigen", nscan, S, pw, 23, C=1, Sm=1)
    inv_scale, scale = 0.7, 0.25
    want = pm.inv_products(sub, patches, pr["probes"], det, inv_scale, scale,
                           mpu0)[:3]
    keep = [dev(pr[k]) for k in ("probe", "eigen", "weights")]
    sub_d, patches_d = dev(sub), dev(patches)
    nmpu = 2 * S * pw * pw  # floats of one set of partial sums
    # the launcher's chunks: about eight positions each, at most 2048 / pw rows
    nchunk = min((2048 + pw - 1) // pw, (nscan + 7) // 8)
    out = dict(nchunk=nchunk)

    def run(scratch_floats):
        scratch = Dev(scratch_floats, init=np.zeros(scratch_floats, np.float32))
        assert lib.tike_set_deterministic(1, scratch.ptr(),
                                          4 * scratch_floats) == 0
        bufs = (Dev((nscan, pw, pw), cplx=True), Dev((nscan, pw, pw), cplx=True),
                Dev((S, pw, pw), cplx=True, init=mpu0))
        rc = lib.tike_pfa_inv_products(
            dptr(sub_d), dptr(patches_d), dptr(keep[0]), 0, None, dptr(keep[1]),
            dptr(keep[2]), 1, 1, bufs[0].ptr(), bufs[1].ptr(), bufs[2].ptr(),
            scale, nscan, S, pw, det, inv_scale, A.stream_ptr())
        scratch.get()  # (the guards: a failure ends the child)
        return rc, [b.get() for b in bufs], bufs

    def ok(got):
        return all(relerr(a, b) <= OP_NORMWISE and maxerr(a, b) <= OP_MAXABS
                   for a, b in zip(got, want))

    digests, good = [], True
    for _ in range(2):
        rc, got, _ = run(4 * nmpu * nchunk)
        good = good and rc == 0 and ok(got)
        h = hashlib.sha256()
        for a in got:
            h.update(a.tobytes())
        digests.append(h.hexdigest())
    out["ample_digests"], out["ample_ok"] = digests, bool(good)
    rc, got, _ = run(nmpu)  # one set, not nchunk: the one-chunk fallback
    out["one_set_ok"] = bool(rc == 0 and ok(got))
    rc, got, bufs = run(nmpu - 1)
    out["too_small_rc"] = int(rc)
    out["too_small_untouched"] = bool(all(b.untouched() for b in bufs))
    lib.tike_set_deterministic(0, None, 0)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
