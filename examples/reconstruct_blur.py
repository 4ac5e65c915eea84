#!/usr/bin/env python3
"""Far-field blur: a source of finite size (partial spatial coherence) and the
detector's point-spread function both convolve the recorded intensity with a
small kernel.  Simulate a data set whose patterns are blurred by a Gaussian
(`simulate(..., blur=K)`), then reconstruct it with cgrad and ONE probe mode
twice: without `blur_options`, where the blur ends up in the object, and with
them, where a third conjugate-gradient block per minibatch fits the kernel
from a first guess that is mostly a delta.  Both object errors and the fitted
kernel's distance to the true one are printed:

    python examples/reconstruct_blur.py [--positions 100] [--width 64]
                                        [--epochs 12] [--sigma 0.8]
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
    ap.add_argument("--sigma", type=float, default=0.8,
                    help="width of the Gaussian blur, in detector pixels")
    ap.add_argument("--taps", type=int, default=5, choices=(3, 5, 7))
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
    # the kernel: centre at [taps // 2, taps // 2]; `simulate` normalises it
    x = np.arange(a.taps) - a.taps // 2
    kernel = np.exp(-(x[:, None]**2 + x[None, :]**2)
                    / (2 * a.sigma**2)).astype(np.float32)
    kernel /= kernel.sum()
    data = tike_ptycho.simulate(width, probe, scan, psi, blur=kernel)
    print(f"{a.positions} patterns of {width}^2, blurred by a Gaussian of "
          f"sigma {a.sigma} px on {a.taps} x {a.taps} taps (centre tap "
          f"{kernel[a.taps // 2, a.taps // 2]:.3f})")

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
    # a first guess: mostly a delta
    guess = np.full((a.taps, a.taps), 0.48 / (a.taps**2 - 1), np.float32)
    guess[a.taps // 2, a.taps // 2] = 0.52
    options = tike_ptycho.BlurOptions(guess.copy())
    fitted = tike_ptycho.reconstruct(data, parameters(), blur_options=options)
    e0 = object_error(without.psi, psi, lo, hi)
    e1 = object_error(fitted.psi, psi, lo, hi)
    print(f"object error, one mode, without blur_options: {e0:.4f}")
    print(f"object error, one mode, with blur_options:    {e1:.4f}")
    print(f"fitted kernel: L1 distance to the true one "
          f"{np.abs(options.kernel - kernel).sum():.4f} "
          f"(first guess {np.abs(guess - kernel).sum():.4f})")
    return 0 if e1 < e0 else 1


if __name__ == "__main__":
    sys.exit(main())
