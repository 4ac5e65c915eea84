#!/usr/bin/env python3
"""Detector binning: the beam is too large (or the detector too close) for the
illumination to fit into a window as wide as the diffraction patterns, so the
far field is modelled on a grid `binning` times finer than the detector and
every measured pixel is the sum of binning x binning model pixels.  Simulate
such a data set (`simulate(..., binning=2)`) and reconstruct it with cgrad,
the solver that takes `binning`:

    python examples/reconstruct_binned.py [--positions 144] [--width 64]
                                          [--epochs 8]

`--width` is the far-plane (and probe-window) width; the patterns are
width / 2 wide and the beam below does not fit into a window of that width:
without `binning` the data-shape rule (probe window <= data width) refuses the
problem.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tike_amd.ptycho as tike_ptycho  # noqa: E402

BINNING = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=144)
    ap.add_argument("--width", type=int, default=64,
                    help="far-plane = probe-window width")
    ap.add_argument("--modes", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=8)
    a = ap.parse_args()

    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(a.positions)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:a.positions]
    scan = (2 + 8.0 * ij + rng.random((a.positions, 2))).astype(np.float32)
    width = a.width
    data_width = width // BINNING
    extent = 8 * (side - 1) + width + 8
    psi = ((0.75 + 0.25 * rng.random((1, extent, extent))) * np.exp(
        1j * np.pi * (rng.random((1, extent, extent)) - 0.5))).astype(np.complex64)
    # a beam that fills the far-plane window: its 1/e^2 diameter is 0.7 of the
    # window, 1.4 times the width of the patterns
    probe = np.stack([
        tike_ptycho.gaussian(width, rin=0.7)
        * np.exp(0.3j * np.pi * rng.random((width, width))) / (m + 1)
        for m in range(a.modes)])[None, None].astype(np.complex64)
    power = np.abs(probe[0, 0, 0])**2
    inside = slice((width - data_width) // 2, (width + data_width) // 2)
    print(f"probe window {width}, patterns {data_width} wide: "
          f"{1 - power[inside, inside].sum() / power.sum():.0%} of the beam "
          "lies outside a window of the patterns' width")
    data = tike_ptycho.simulate(width, probe, scan, psi, binning=BINNING)
    assert data.shape == (a.positions, data_width, data_width)

    parameters = tike_ptycho.PtychoParameters(
        probe=probe, psi=np.full_like(psi, 0.5), scan=scan,
        algorithm_options=tike_ptycho.CgradOptions(num_batch=2, cg_iter=2,
                                                   num_iter=a.epochs),
        probe_options=tike_ptycho.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tike_ptycho.ObjectOptions(),
        exitwave_options=tike_ptycho.ExitWaveOptions(
            measured_pixels=np.ones((data_width, data_width), bool)))
    try:
        tike_ptycho.reconstruct(data, parameters)
    except ValueError as e:
        print("without binning:", str(e)[:96], "...")
    result = tike_ptycho.reconstruct(data, parameters, binning=BINNING)
    costs = [float(np.mean(c)) for c in result.algorithm_options.costs]
    print("cost per epoch:", " ".join(f"{c:.4g}" for c in costs))
    print(f"{data.shape[0]} patterns {data.shape[1:]} x binning {BINNING}: "
          f"psi {result.psi.shape}, probe {result.probe.shape}")
    return 0 if costs[-1] < costs[0] else 1


if __name__ == "__main__":
    sys.exit(main())
