#!/usr/bin/env python3
"""An incoherent background: air scatter, fluorescence and dark current add a
count to every detector pixel that does not move with the scan.  Simulate a
data set with a flat offset plus a smooth blob around the beam
(`simulate(..., background=b)`), then reconstruct it with cgrad twice: without
`background_options`, where the background leaks into the object, and with
them, where a third conjugate-gradient block per minibatch fits it.  Both
object errors are printed:

    python examples/reconstruct_background.py [--positions 100] [--width 64]
                                              [--epochs 12]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tike_amd.ptycho as tike_ptycho  # noqa: E402


def object_error(psi, truth, lo, hi):
    """Normwise error over the scanned field of view after the best global
    complex factor."""
    a = psi[0, lo:hi, lo:hi].astype(np.complex128)
    t = truth[0, lo:hi, lo:hi].astype(np.complex128)
    a = a * (np.vdot(a, t) / np.vdot(a, a))
    return float(np.linalg.norm(a - t) / np.linalg.norm(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=100)
    ap.add_argument("--width", type=int, default=64,
                    help="detector = probe-window width")
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--flat", type=float, default=0.3)
    ap.add_argument("--blob", type=float, default=1.5)
    a = ap.parse_args()

    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(a.positions)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:a.positions]
    scan = (2 + 6.0 * ij + rng.random((a.positions, 2))).astype(np.float32)
    width = a.width
    extent = 6 * (side - 1) + width + 8
    psi = ((0.75 + 0.25 * rng.random((1, extent, extent))) * np.exp(
        1j * np.pi * (rng.random((1, extent, extent)) - 0.5))).astype(np.complex64)
    probe = (tike_ptycho.gaussian(width, rin=0.6) * np.exp(
        1j * np.pi * rng.random((width, width))))[None, None, None].astype(
            np.complex64)
    # a flat offset plus a smooth blob around the beam, in the stored
    # (FFT-shifted) layout of the patterns
    y, x = np.meshgrid(np.linspace(-1, 1, width), np.linspace(-1, 1, width),
                       indexing="ij")
    background = np.fft.ifftshift(a.flat + a.blob * np.exp(
        -(x * x + y * y) / (2 * 0.35**2))).astype(np.float32)
    data = tike_ptycho.simulate(width, probe, scan, psi, background=background)
    clean = tike_ptycho.simulate(width, probe, scan, psi)
    print(f"{a.positions} patterns of {width}^2: the background is "
          f"{background.sum() / clean.mean(axis=0).sum():.0%} of a pattern's "
          "counts")

    def parameters():
        return tike_ptycho.PtychoParameters(
            probe=probe.copy(), psi=np.full_like(psi, 0.5), scan=scan.copy(),
            algorithm_options=tike_ptycho.CgradOptions(
                num_batch=1, cg_iter=2, num_iter=a.epochs),
            probe_options=None, object_options=tike_ptycho.ObjectOptions(),
            exitwave_options=tike_ptycho.ExitWaveOptions(
                measured_pixels=np.ones((width, width), bool)))

    lo, hi = 2, int(scan.max()) + width
    without = tike_ptycho.reconstruct(data, parameters())
    options = tike_ptycho.BackgroundOptions(
        np.full((width, width), 0.1, np.float32))  # a first guess: a constant
    fitted = tike_ptycho.reconstruct(data, parameters(),
                                     background_options=options)
    e0 = object_error(without.psi, psi, lo, hi)
    e1 = object_error(fitted.psi, psi, lo, hi)
    b_err = np.linalg.norm(options.background - background) / np.linalg.norm(
        background)
    print(f"object error without background_options: {e0:.4f}")
    print(f"object error with background_options:    {e1:.4f}")
    print(f"fitted background: normwise error {b_err:.3f} "
          f"(first guess {np.linalg.norm(0.1 - background) / np.linalg.norm(background):.3f})")
    return 0 if e1 < e0 else 1


if __name__ == "__main__":
    sys.exit(main())
