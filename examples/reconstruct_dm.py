#!/usr/bin/env python3
"""Start a reconstruction from a poor probe with the difference map, then
refine its result with lstsq_grad: simulate a small ptychography data set,
blur and dim the probe, run 30 epochs of `dm` and 10 of `lstsq_grad` from
what they leave.

    python examples/reconstruct_dm.py

The first history is the Fourier error of the difference map's reflected
estimate (`DmOptions`); the second is the model cost of object x probe, which
is what `lstsq_grad` reports.  The exit waves of `dm` live in its
`Reconstruction` only: the second call starts from the object and the probe.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tike_amd.ptycho as tike_ptycho  # noqa: E402


def blurred(probe, passes):
    """`passes` of the (1, 2, 1) / 4 filter along both axes, periodic."""
    for _ in range(passes):
        for axis in (-2, -1):
            probe = (np.roll(probe, 1, axis) + 2 * probe
                     + np.roll(probe, -1, axis)) / 4
    return probe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=144)
    ap.add_argument("--width", type=int, default=64, help="probe = detector width")
    ap.add_argument("--dm-epochs", type=int, default=30)
    ap.add_argument("--lstsq-epochs", type=int, default=10)
    a = ap.parse_args()

    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(a.positions)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:a.positions]
    scan = (2 + 5.0 * ij + rng.random((a.positions, 2))).astype(np.float32)
    width = a.width
    extent = 5 * (side - 1) + width + 8
    smooth = lambda x: blurred(x, 4)
    psi = ((0.6 + 0.4 * smooth(rng.random((1, extent, extent)))) * np.exp(
        1j * np.pi * (smooth(rng.random((1, extent, extent))) - 0.5))).astype(
            np.complex64)
    probe = (100 * tike_ptycho.gaussian(width)[None, None, None] * np.exp(
        0.3j * np.pi * smooth(rng.random((1, 1, 1, width, width))))).astype(
            np.complex64)
    data = tike_ptycho.simulate(width, probe, scan, psi)

    poor = (0.8 * blurred(probe, 2)).astype(np.complex64)
    options = dict(
        probe_options=tike_ptycho.ProbeOptions(
            init_rescale_from_measurements=False),
        object_options=tike_ptycho.ObjectOptions())
    first = tike_ptycho.reconstruct(data, tike_ptycho.PtychoParameters(
        probe=poor, psi=np.full_like(psi, np.abs(psi).mean()), scan=scan,
        algorithm_options=tike_ptycho.DmOptions(num_iter=a.dm_epochs),
        **options))
    second = tike_ptycho.reconstruct(data, tike_ptycho.PtychoParameters(
        probe=first.probe, psi=first.psi, scan=scan,
        algorithm_options=tike_ptycho.LstsqOptions(
            num_batch=4, num_iter=a.lstsq_epochs), **options))
    dm_costs = [float(np.mean(c)) for c in first.algorithm_options.costs]
    costs = [float(np.mean(c)) for c in second.algorithm_options.costs]
    print("dm, Fourier error of the reflected estimate per epoch:",
          " ".join(f"{c:.4g}" for c in dm_costs))
    print("lstsq_grad from its result, cost per epoch:",
          " ".join(f"{c:.4g}" for c in costs))
    # (the first dm epoch starts from waves = P O: its error IS the model cost
    # of the poor start)
    return 0 if dm_costs[-1] < dm_costs[0] and costs[-1] < dm_costs[0] else 1


if __name__ == "__main__":
    sys.exit(main())
