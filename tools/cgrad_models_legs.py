"""Epoch rate of cgrad (bench.py's c2 problem: 256^2, 1 mode, 10 000
positions, 10 minibatches, cg_iter = 4) under the four cost models it
supports -- gaussian, gaussian + mask, poisson, poisson + mask -- in one
process, each leg after two untimed epochs, and how many CG calls left the
device line search for the host-side one.

The mask is a beamstop disc around the zero frequency plus a dead row and a
dead column; the counts there are NaN.

    python tools/cgrad_models_legs.py [positions=10000] [detector=256] [epochs=3]
                                      [legs, e.g. gaussian,poisson+mask]

One JSON line per leg, then the rate of each leg relative to gaussian."""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import tike_amd._arrays as A  # noqa: E402
import tike_amd.ptycho as tp  # noqa: E402

C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")

LEGS = (("gaussian", False), ("gaussian", True), ("poisson", False),
        ("poisson", True))


def beamstop_mask(det):
    """True = measured: a disc of radius det / 24 around the zero frequency
    (corner-centred layout), one dead row and one dead column."""
    f = np.fft.fftfreq(det) * det
    mask = f[:, None]**2 + f[None, :]**2 > (det / 24.0)**2
    mask[det // 3, :] = False
    mask[:, (2 * det) // 5] = False
    return mask


class Fallbacks:
    """Counts the CG calls the host-side search made (opt.conjugate_gradient
    inside cgrad) and the all-at-once searches that found no step."""

    def __init__(self):
        self.host = self.linear_failed = 0
        self._cg, self._dev = C.opt.conjugate_gradient, C._cg_device

        def host(*a, **k):
            self.host += 1
            return self._cg(*a, **k)

        def dev(*a, **k):
            r = self._dev(*a, **k)
            if k.get("linear") and r is None:
                self.linear_failed += 1
            return r

        C.opt.conjugate_gradient, C._cg_device = host, dev

    def close(self):
        C.opt.conjugate_gradient, C._cg_device = self._cg, self._dev


def leg(p, data, model, masked, num_batch, epochs):
    det, N = p["det"], len(p["scan"])
    mask = beamstop_mask(det) if masked else np.ones((det, det), bool)
    d = data.copy()
    if masked:
        d[:, ~mask] = np.nan
    np.random.seed(1234)
    params = tp.PtychoParameters(
        probe=p["probe"].copy(), psi=np.full_like(p["psi"], 0.5 + 0j),
        scan=p["scan"].copy(),
        algorithm_options=tp.CgradOptions(num_batch=num_batch, cg_iter=4),
        probe_options=tp.ProbeOptions(force_orthogonality=True),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(measured_pixels=mask,
                                            noise_model=model))
    count = Fallbacks()
    ctx = tp.Reconstruction(A.to_device(d, np.float32), params,
                            presharded=True, order=np.arange(N),
                            batches=np.array_split(np.arange(N), num_batch))
    ctx.__enter__()
    try:
        ctx.iterate(2)
        torch.cuda.synchronize()
        warm = (count.host, count.linear_failed)
        t0 = time.perf_counter()
        ctx.iterate(epochs)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        cost = float(ctx.parameters.algorithm_options.costs[-1][0])
    finally:
        ctx.__exit__(None, None, None)
        count.close()
    return dict(model=model, mask=masked, measured_pixels=int(mask.sum()),
                positions=N, detector=det, modes=p["probe"].shape[-3],
                num_batch=num_batch, cg_iter=4, epochs=epochs,
                ms_per_epoch=dt / epochs * 1e3, value=N * epochs / dt,
                unit="patterns/s", last_cost=cost,
                host_search_calls=count.host - warm[0],
                host_search_calls_warmup=warm[0],
                linear_search_failures=count.linear_failed - warm[1],
                linear_search_failures_warmup=warm[1])


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    det = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    names = {m + ("+mask" if k else ""): (m, k) for m, k in LEGS}
    legs = ([names[n] for n in sys.argv[4].split(",")] if len(sys.argv) > 4
            else LEGS)
    num_batch = 10
    p = bench.synthetic(N, 1, det, 0, N)
    data = tp.simulate(det, p["probe"], p["scan"], p["psi"]).astype(np.float32)
    rows = []
    for model, masked in legs:
        r = leg(p, data, model, masked, num_batch, epochs)
        rows.append(r)
        print(json.dumps(r), flush=True)
    base = rows[0]["value"]
    for r in rows:
        name = r["model"] + (" + mask" if r["mask"] else "")
        print(f"{name:16s} {r['value'] / 1e3:8.1f} k patterns/s  "
              f"{r['value'] / base:5.3f} x gaussian  host searches "
              f"{r['host_search_calls']} (warm-up {r['host_search_calls_warmup']})",
              flush=True)


if __name__ == "__main__":
    main()
