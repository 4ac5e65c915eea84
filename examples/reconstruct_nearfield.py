#!/usr/bin/env python3
"""Near-field (Fresnel, holographic) ptychography: the detector sits a finite
distance behind the sample, a diffuser structures the beam and the probe fills
the whole frame.  Simulate such a data set (`simulate(..., nearfield=H)`: a
speckled full-frame probe, a weak-phase object, a propagator with a few pi of
phase at Nyquist), then reconstruct it with cgrad twice: with
`nearfield_options`, and as if the frames were far-field patterns, to show
that the model matters.  Both object errors are printed:

    python examples/reconstruct_nearfield.py [--positions 64] [--width 128]
                                             [--epochs 10] [--nyquist-pi 3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tike_amd.ptycho as tike_ptycho  # noqa: E402


def smooth(shape, rng, sigma):
    """A smooth real field of unit maximum: white noise under a Gaussian
    low-pass, by the transform."""
    f = [np.fft.fftfreq(n) for n in shape]
    low = np.exp(-2 * (np.pi * sigma)**2 * (f[0][:, None]**2 + f[1][None]**2))
    x = np.fft.ifft2(np.fft.fft2(rng.standard_normal(shape)) * low).real
    return x / np.abs(x).max()


def propagator(width, nyquist_pi):
    """The paraxial transfer function exp(-i pi lambda z (fy^2 + fx^2)) on the
    FFT's own frequency order, its phase nyquist_pi * pi / 2 per axis at the
    Nyquist frequency.  With a distance, a pixel size and a wavelength it is
    `NearFieldOptions.from_geometry(width, pixel_size, distance,
    wavelength)`."""
    f = np.fft.fftfreq(width)
    q = (f[:, None]**2 + f[None, :]**2) / 0.25
    return np.exp(-0.5j * np.pi * nyquist_pi * q).astype(np.complex64)


def make_problem(positions=64, width=128, nyquist_pi=3.0, seed=0):
    """dict(psi, probe, scan, H, data): the frames in the natural, unshifted
    layout of the detector."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(positions)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:positions]
    scan = (2 + 5.0 * ij + 3 * rng.random((positions, 2))).astype(np.float32)
    extent = int(scan.max()) + width + 4
    # a weak-phase object with a little absorption
    psi = ((1 - 0.1 * np.abs(smooth((extent, extent), rng, 2.0))) * np.exp(
        0.4j * smooth((extent, extent), rng, 1.5)))[None].astype(np.complex64)
    # a diffuser: amplitude near 1, a strong smooth random phase -> speckle
    probe = ((1 + 0.1 * smooth((width, width), rng, 3.0)) * np.exp(
        3j * smooth((width, width), rng, 2.5)))[None, None, None].astype(
            np.complex64)
    H = propagator(width, nyquist_pi)
    data = tike_ptycho.simulate(width, probe, scan, psi, nearfield=H)
    return dict(psi=psi, probe=probe, scan=scan, H=H, data=data)


def object_error(psi, truth, scan, width):
    """Normwise error over the scanned field of view after the best global
    complex factor."""
    lo, hi = int(scan.min()), int(scan.max()) + width
    a = psi[0, lo:hi, lo:hi].astype(np.complex128)
    t = truth[0, lo:hi, lo:hi].astype(np.complex128)
    a = a * (np.vdot(a, t) / np.vdot(a, a))
    return float(np.linalg.norm(a - t) / np.linalg.norm(t))


def reconstruct(P, epochs, nearfield):
    """cgrad from a flat object with the probe known: with the near-field
    model (nearfield True) or as if the frames were far-field patterns."""
    width = P["probe"].shape[-1]
    parameters = tike_ptycho.PtychoParameters(
        probe=P["probe"].copy(), psi=np.ones_like(P["psi"]),
        scan=P["scan"].copy(),
        algorithm_options=tike_ptycho.CgradOptions(num_batch=1, cg_iter=2,
                                                   num_iter=epochs),
        probe_options=None, object_options=tike_ptycho.ObjectOptions(),
        exitwave_options=tike_ptycho.ExitWaveOptions(
            measured_pixels=np.ones((width, width), bool)))
    options = (tike_ptycho.NearFieldOptions(P["H"].copy()) if nearfield
               else None)
    return tike_ptycho.reconstruct(P["data"], parameters,
                                   nearfield_options=options)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=64)
    ap.add_argument("--width", type=int, default=128,
                    help="detector = probe-window width")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--nyquist-pi", type=float, default=3.0,
                    help="phase of the propagator at Nyquist, in units of pi")
    a = ap.parse_args()
    P = make_problem(a.positions, a.width, a.nyquist_pi)
    print(f"{a.positions} near-field frames of {a.width}^2, {a.nyquist_pi} pi "
          "of propagator phase at Nyquist")
    near = reconstruct(P, a.epochs, True)
    far = reconstruct(P, a.epochs, False)
    e_near = object_error(near.psi, P["psi"], P["scan"], a.width)
    e_far = object_error(far.psi, P["psi"], P["scan"], a.width)
    print(f"object error with nearfield_options: {e_near:.4f}")
    print(f"object error, as if far-field:       {e_far:.4f}")
    return 0 if e_near < e_far else 1


if __name__ == "__main__":
    sys.exit(main())
