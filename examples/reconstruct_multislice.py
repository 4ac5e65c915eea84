#!/usr/bin/env python3
"""A thick sample as two object slices a Fresnel step apart: simulate such a
data set and reconstruct both slices and the probe with cgrad under the Poisson
noise model -- the exact gradient through every slice, with a line search:

    python examples/reconstruct_multislice.py [--positions 144] [--width 64]
                                              [--epochs 8]

The optics of the step between the slices travel in the options:
`ProbeOptions(probe_wavelength, probe_FOV_lengths)` and
`ObjectOptions(multislice_propagation_distance)`; the probe window must equal
the detector width (the wave that leaves a slice is the next slice's probe).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tike_amd.ptycho as tike_ptycho  # noqa: E402

SLICES = 2
PIXEL = 1e-8  # 10 nm
WAVELENGTH = 1e-10
DISTANCE = 2e-6  # between the slices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=144)
    ap.add_argument("--width", type=int, default=64, help="probe = detector width")
    ap.add_argument("--modes", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=8)
    a = ap.parse_args()

    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(a.positions)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:a.positions]
    scan = (2 + 8.0 * ij + rng.random((a.positions, 2))).astype(np.float32)
    width = a.width
    extent = 8 * (side - 1) + width + 8
    psi = ((0.8 + 0.2 * rng.random((SLICES, extent, extent))) * np.exp(
        0.3j * rng.standard_normal((SLICES, extent, extent)))).astype(np.complex64)
    # a few thousand photons per pattern: the Poisson model's regime
    probe = 2.0 * np.stack([
        tike_ptycho.gaussian(width, rin=0.6)
        * np.exp(0.3j * np.pi * rng.random((width, width))) / (m + 1)
        for m in range(a.modes)])[None, None].astype(np.complex64)
    optics = dict(probe_wavelength=WAVELENGTH,
                  probe_FOV_lengths=(width * PIXEL, width * PIXEL))
    exact = tike_ptycho.simulate(width, probe, scan, psi,
                                 multislice_propagation_distance=DISTANCE,
                                 **optics)
    data = rng.poisson(exact).astype(np.uint16)

    parameters = tike_ptycho.PtychoParameters(
        probe=probe, psi=np.full_like(psi, 0.9), scan=scan,
        algorithm_options=tike_ptycho.CgradOptions(num_batch=2, cg_iter=2,
                                                   num_iter=a.epochs),
        probe_options=tike_ptycho.ProbeOptions(
            init_rescale_from_measurements=False, **optics),
        object_options=tike_ptycho.ObjectOptions(
            multislice_propagation_distance=DISTANCE),
        exitwave_options=tike_ptycho.ExitWaveOptions(
            measured_pixels=np.ones((width, width), bool),
            noise_model="poisson"))
    result = tike_ptycho.reconstruct(data, parameters)
    costs = [float(np.mean(c)) for c in result.algorithm_options.costs]
    print("cost per epoch:", " ".join(f"{c:.4g}" for c in costs))
    print(f"{data.shape[0]} patterns: psi {result.psi.shape}, "
          f"probe {result.probe.shape}")
    return 0 if costs[-1] < costs[0] else 1


if __name__ == "__main__":
    sys.exit(main())
