#!/usr/bin/env python3
"""Fly-scan data: the stage moves while the detector integrates, so every
diffraction pattern is the incoherent sum of `fly` consecutive scan positions.
Simulate such a data set (`simulate(..., fly=4)`) and reconstruct it with
cgrad, the solver that takes `fly`:

    python examples/reconstruct_fly.py [--frames 144] [--width 64] [--epochs 8]

`parameters.scan` holds frames * fly positions, `data` holds frames patterns;
pattern f belongs to the scan rows f * fly ... f * fly + fly - 1.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tike_amd.ptycho as tike_ptycho  # noqa: E402

FLY = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=144)
    ap.add_argument("--width", type=int, default=64, help="probe = detector width")
    ap.add_argument("--modes", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=8)
    a = ap.parse_args()

    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(a.frames)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:a.frames]
    # a frame starts on a jittered grid and sweeps 1.5 pixels per position
    start = 2 + 8.0 * ij + rng.random((a.frames, 2))
    sweep = np.arange(FLY)[None, :, None] * np.array([0.0, 1.5])[None, None]
    scan = (start[:, None] + sweep).reshape(-1, 2).astype(np.float32)
    width = a.width
    extent = 8 * (side - 1) + width + 8 + int(1.5 * FLY)
    psi = ((0.75 + 0.25 * rng.random((1, extent, extent))) * np.exp(
        1j * np.pi * (rng.random((1, extent, extent)) - 0.5))).astype(np.complex64)
    probe = np.stack([
        tike_ptycho.gaussian(width, rin=0.6)
        * np.exp(0.3j * np.pi * rng.random((width, width))) / (m + 1)
        for m in range(a.modes)])[None, None].astype(np.complex64)
    data = tike_ptycho.simulate(width, probe, scan, psi, fly=FLY)
    assert data.shape[0] * FLY == scan.shape[0]

    parameters = tike_ptycho.PtychoParameters(
        probe=probe, psi=np.full_like(psi, 0.5), scan=scan,
        algorithm_options=tike_ptycho.CgradOptions(num_batch=2, cg_iter=2,
                                                   num_iter=a.epochs),
        probe_options=tike_ptycho.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tike_ptycho.ObjectOptions(),
        exitwave_options=tike_ptycho.ExitWaveOptions(
            measured_pixels=np.ones((width, width), bool)))
    result = tike_ptycho.reconstruct(data, parameters, fly=FLY)
    costs = [float(np.mean(c)) for c in result.algorithm_options.costs]
    print("cost per epoch:", " ".join(f"{c:.4g}" for c in costs))
    print(f"{data.shape[0]} frames x fly {FLY}: psi {result.psi.shape}, "
          f"probe {result.probe.shape}, scan {result.scan.shape}")
    return 0 if costs[-1] < costs[0] else 1


if __name__ == "__main__":
    sys.exit(main())
