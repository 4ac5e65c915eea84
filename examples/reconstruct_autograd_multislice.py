#!/usr/bin/env python3
"""The differentiable MULTISLICE intensity model: a thick sample with
uncertain positions, the combination `cgrad` refuses (it reconstructs an
object of several slices only with fixed positions), in a few lines of
`torch.optim.Adam`.  Data is simulated from a two-slice object and known
positions; the positions handed to the optimiser are off by up to 0.3 pixels.
`tike_amd.autograd.multislice_intensity` gives any PyTorch loss exact
gradients with respect to every slice, the probe and the scan positions, so
Adam first refines the positions alone, then both slices and the positions
together:

    python examples/reconstruct_autograd_multislice.py [--frames 100]
                                                       [--width 64]
                                                       [--epochs 40] [--fly 1]

Printed per epoch: the gaussian amplitude cost mean((sqrt(I) - sqrt(d))^2)
and the RMS distance of the positions from the true ones, in pixels.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tike_amd.operators as operators  # noqa: E402
import tike_amd.ptycho as tike_ptycho  # noqa: E402
from tike_amd.autograd import multislice_intensity  # noqa: E402

PIXEL, WAVELENGTH, DISTANCE = 1e-8, 1e-10, 2e-6  # 10 nm, 1 A, 2 um apart


def smooth(rng, shape, sigma):
    """White noise under a gaussian filter, scaled to [-1, 1]."""
    from scipy.ndimage import gaussian_filter
    a = gaussian_filter(rng.standard_normal(shape), sigma)
    return a / np.abs(a).max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--width", type=int, default=64, help="probe = detector width")
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--fly", type=int, default=1, help="positions per frame")
    a = ap.parse_args()

    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(a.frames)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:a.frames]
    # a frame starts on a jittered grid and sweeps 1.5 pixels per position
    start = 4 + 6.0 * ij + rng.random((a.frames, 2))
    sweep = np.arange(a.fly)[None, :, None] * np.array([0.0, 1.5])[None, None]
    truth = (start[:, None] + sweep).reshape(-1, 2).astype(np.float32)
    width = a.width
    extent = 6 * (side - 1) + width + 12 + int(1.5 * a.fly)
    # two mutually different smooth slices
    psi_true = np.stack([
        (0.7 + 0.3 * smooth(rng, (extent, extent), 3.0)) * np.exp(
            0.8j * np.pi * smooth(rng, (extent, extent), 3.0)),
        (0.85 + 0.15 * smooth(rng, (extent, extent), 4.0)) * np.exp(
            0.5j * np.pi * smooth(rng, (extent, extent), 4.0))
    ]).astype(np.complex64)
    probe_true = tike_ptycho.gaussian(width, rin=0.6)[None, None, None].astype(
        np.complex64)

    dev = torch.device("cuda")
    truth_d = torch.from_numpy(truth).to(dev)
    scan = (truth_d + 0.6 * (torch.rand(truth_d.shape, device=dev) - 0.5)
            ).requires_grad_(True)
    psi = torch.from_numpy(psi_true).to(dev).requires_grad_(True)
    probe = torch.from_numpy(probe_true).to(dev)

    def rms():
        return float((scan.detach() - truth_d).square().sum(dim=1).mean().sqrt())

    def run(title, optimiser):
        print(title)
        for epoch in range(a.epochs):
            optimiser.zero_grad()
            cost = ((multislice_intensity(op, psi, probe, scan,
                                          fly=a.fly).sqrt() - d.sqrt())**2
                    ).mean()
            cost.backward()
            optimiser.step()
            print(f"  epoch {epoch:3d}: cost {float(cost.detach()):.4e}, "
                  f"position error {rms():.4f} px")

    with operators.Ptycho(
            detector_shape=width, probe_shape=width, nz=extent, n=extent,
            probe_wavelength=WAVELENGTH,
            probe_FOV_lengths=(width * PIXEL, width * PIXEL),
            multislice_propagation_distance=DISTANCE) as op:
        with torch.no_grad():  # the data: the model at the true positions
            d = multislice_intensity(op, psi, probe, truth_d, fly=a.fly)
        assert d.shape[0] * a.fly == truth.shape[0]
        first = rms()
        run(f"positions alone ({truth.shape[0]} positions, {d.shape[0]} "
            f"frames x fly {a.fly}, {psi.shape[0]} slices; position error "
            f"{first:.4f} px)", torch.optim.Adam([scan], lr=0.05))
        alone = rms()
        # both slices start 1 % off: while Adam repairs them the positions
        # give way a little, then go on falling
        with torch.no_grad():
            psi.mul_(0.99).add_(0.005)
        run("both slices and the positions together", torch.optim.Adam([
            dict(params=[psi], lr=1e-3), dict(params=[scan], lr=0.03)]))
        print(f"position error {first:.4f} -> {alone:.4f} (positions alone) -> "
              f"{rms():.4f} px (together)")
    return 0 if alone < first else 1


if __name__ == "__main__":
    sys.exit(main())
