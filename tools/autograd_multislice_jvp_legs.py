#!/usr/bin/env python3
"""Legs of the forward-mode derivative of the differentiable MULTISLICE
intensity model on the GPU (not a test, not part of bench.py):

    python tools/autograd_multislice_jvp_legs.py [--repeats 5] [--frames 4000]
                                                 [--once]

At 256^2 x 8 modes x 2 slices and 128^2 x 4 modes x 3 slices, `frames` frames
of `fly` = 1 and 4 positions each (the shapes of autograd_multislice_legs.py),
it times with device events (2 warm-up calls, median of the repeats), all in
one process
  * `tike_slice_wave_tangent` alone on one chunk of positions, three tangents:
    the form of the slices behind the first (a beam per position, de written
    over a dbeam per position) and the form of slice 0 (shared probe and
    d_probe), each as a time and as a share of the 8 TB/s roofline on its
    byte model (csrc/autograd_jvp.hip; the object taps, which come mostly from
    cache, left out), the latter alternating with `tike_conv_fwd_tangent` at
    det == pw on the same planes and with ITSELF (new, old, new: the
    difference of the two medians of the same launch is the spread);
  * the Fresnel step of the tangent on the same chunk: `tike_fresnel_spect_prop`
    in place against `tike_fft2_pass1` -> `tike_fresnel_colpass` ->
    `tike_fft2_pass2_inplace`, alternating;
  * one forward of `multislice_intensity`, one forward + backward with all
    three gradients (loss = sum(g * I), a random signed g),
    `multislice_intensity_jvp` with all three tangents -- with the default
    levers, with `TANGENT_FRESNEL_TWO_PASS` flipped and with
    `FIRST_SLICE_BY_CONV_TANGENT` flipped, the three alternating -- and with
    `d_scan` alone, and `multislice_gauss_newton_product` with all three
    tangents and all three parts.
`--once` runs everything exactly once after one warm-up call (for a
`rocprofv3 --kernel-trace --stats` run).  One line per shape, then one JSON
line with the library's build id."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import tike_amd.operators as ops  # noqa: E402
from autograd_multislice_legs import (DISTANCE, HBM_PEAK, PIXEL,  # noqa: E402
                                      WAVELENGTH, problem, timed,
                                      timed_alternating)
from tike_amd import _arrays as A  # noqa: E402
from tike_amd import autograd  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402
from tike_amd.operators.propagation import fft_scales  # noqa: E402


def legs(det, S, D, frames, fly, repeats, warm):
    dev = torch.device("cuda")
    psi_h, probe_h, scan_h = problem(det, S, D, frames, fly)
    N = frames * fly
    H, W = psi_h.shape[-2:]
    row = dict(det=det, modes=S, slices=D, frames=frames, fly=fly,
               positions=N)
    psi, probe, scan = (torch.from_numpy(x).to(dev).requires_grad_(True)
                        for x in (psi_h, probe_h, scan_h))
    gen = torch.Generator(device=dev).manual_seed(det + S + fly)
    rc = lambda *shape: torch.view_as_complex(torch.randn(
        tuple(shape) + (2,), generator=gen, device=dev))
    d_psi, d_probe = rc(*psi.shape), rc(*probe.shape)
    d_scan = torch.randn(scan.shape, generator=gen, device=dev)
    g = torch.randn((frames, det, det), generator=gen, device=dev)
    f, jvp = autograd.multislice_intensity, autograd.multislice_intensity_jvp
    tangents = dict(d_psi=d_psi, d_probe=d_probe, d_scan=d_scan)
    with ops.Ptycho(probe_shape=det, detector_shape=det, nz=H, n=W,
                    probe_wavelength=WAVELENGTH,
                    probe_FOV_lengths=(det * PIXEL, det * PIXEL),
                    multislice_propagation_distance=DISTANCE) as op:

        def forward():
            with torch.no_grad():
                f(op, psi, probe, scan, fly=fly)

        def both():
            for x in (psi, probe, scan):
                x.grad = None
            (f(op, psi, probe, scan, fly=fly) * g).sum().backward()

        def flipped(lever):
            def run():
                old = getattr(autograd, lever)
                setattr(autograd, lever, not old)
                try:
                    jvp(op, psi, probe, scan, fly=fly, **tangents)
                finally:
                    setattr(autograd, lever, old)
            return run

        row["forward_ms"] = timed(forward, repeats, warm)
        row["forward_backward_ms"] = timed(both, repeats, warm)
        row["tangent_fresnel_two_pass"] = bool(
            autograd.TANGENT_FRESNEL_TWO_PASS)
        row["first_slice_by_conv_tangent"] = bool(
            autograd.FIRST_SLICE_BY_CONV_TANGENT)
        (row["jvp_three_tangents_ms"], row["jvp_fresnel_lever_flipped_ms"],
         row["jvp_first_slice_lever_flipped_ms"]) = timed_alternating(
             [lambda: jvp(op, psi, probe, scan, fly=fly, **tangents),
              flipped("TANGENT_FRESNEL_TWO_PASS"),
              flipped("FIRST_SLICE_BY_CONV_TANGENT")], repeats, warm)
        row["jvp_scan_tangent_ms"] = timed(
            lambda: jvp(op, psi, probe, scan, d_scan=d_scan, fly=fly),
            repeats, warm)
        row["gauss_newton_product_ms"] = timed(
            lambda: autograd.multislice_gauss_newton_product(
                op, psi, probe, scan, fly=fly, **tangents), repeats, warm)
        # the route and the chunk of the model (ptycho/solvers/_multislice.py)
        route = autograd._SlicesForward(op, fly, psi, probe, scan, extra=1)
        row["fused_route"] = route.fused
        n = row["chunk_positions"] = min(route.chunk, N)
        # ------------------------------------- the launches on one chunk
        st = A.stream_ptr()
        P, Q, Sc = psi.detach(), probe.detach(), scan.detach()[:n]
        dsc = d_scan[:n]
        beam, dwave = rc(n, S, det, det), rc(n, S, det, det)
        scratch = torch.empty_like(dwave)

        def chain():  # a slice behind the first: de over dbeam
            check(lib.tike_slice_wave_tangent(
                A.ptr(P[1]), A.ptr(d_psi[1]), A.ptr(Sc), A.ptr(dsc),
                A.ptr(beam), 1, A.ptr(dwave), 1, A.ptr(dwave), n, S, det, H,
                W, st), "tike_slice_wave_tangent")

        def first():  # slice 0: shared probe and d_probe
            check(lib.tike_slice_wave_tangent(
                A.ptr(P[0]), A.ptr(d_psi[0]), A.ptr(Sc), A.ptr(dsc), A.ptr(Q),
                0, A.ptr(d_probe), 0, A.ptr(scratch), n, S, det, H, W, st),
                "tike_slice_wave_tangent")

        def conv():  # the same planes by the single-slice entry
            check(lib.tike_conv_fwd_tangent(
                A.ptr(P[0]), A.ptr(d_psi[0]), A.ptr(Sc), A.ptr(dsc), A.ptr(Q),
                A.ptr(d_probe), A.ptr(scratch), n, S, det, det, H, W, st),
                "tike_conv_fwd_tangent")

        row["slice_wave_tangent_chain_ms"] = timed(chain, repeats, warm)
        (row["slice_wave_tangent_first_ms"], row["conv_fwd_tangent_ms"],
         again) = timed_alternating([first, conv, first], repeats, warm)
        row["slice_wave_tangent_first_again_ms"] = again
        fresnel = op.diffraction.propagation
        fwd_scale, inv_scale = fft_scales(det, op.norm)
        torch.view_as_real(dwave).normal_()  # (finite values)

        def one_launch():
            fresnel.fwd(dwave, overwrite=True)

        legs_ = [one_launch]
        if row["fused_route"]:
            prop = fresnel._propagator((det, det), dev)

            def two_pass():
                check(lib.tike_fft2_pass1(A.ptr(dwave), A.ptr(scratch), n * S,
                                          det, 0, st), "tike_fft2_pass1")
                check(lib.tike_fresnel_colpass(
                    A.ptr(scratch), A.ptr(prop), 0, A.ptr(dwave), n * S, det,
                    fwd_scale * inv_scale, st), "tike_fresnel_colpass")
                check(lib.tike_fft2_pass2_inplace(A.ptr(dwave), n * S, det, 1,
                                                  1.0, st),
                      "tike_fft2_pass2_inplace")

            legs_.append(two_pass)
        times = timed_alternating(legs_, repeats, warm)
        row["fresnel_spect_prop_ms"] = times[0]
        row["fresnel_two_pass_ms"] = times[1] if len(times) > 1 else None
    planes = n * S * det * det * 8
    row["slice_wave_tangent_chain_model_bytes"] = 3 * planes + n * 16
    row["slice_wave_tangent_first_model_bytes"] = planes + n * 16
    for name in ("slice_wave_tangent_chain", "slice_wave_tangent_first"):
        rate = row[name + "_model_bytes"] / (row[name + "_ms"] * 1e-3)
        row[name + "_TB_per_s"] = rate / 1e12
        row[name + "_share_of_8TBps"] = rate / HBM_PEAK
    row["jvp_over_forward"] = row["jvp_three_tangents_ms"] / row["forward_ms"]
    row["jvp_over_forward_backward"] = (row["jvp_three_tangents_ms"]
                                        / row["forward_backward_ms"])
    del beam, dwave, scratch
    torch.cuda.empty_cache()
    two = row["fresnel_two_pass_ms"]
    print(f"{det}^2 x {S} x {D} slices x {frames} frames x fly {fly} "
          f"({'fused' if row['fused_route'] else 'general'} route, chunks of "
          f"{n}): forward {row['forward_ms']:.2f} ms, forward + backward "
          f"{row['forward_backward_ms']:.2f} ms; multislice_intensity_jvp "
          f"{row['jvp_three_tangents_ms']:.2f} ms "
          f"({row['jvp_over_forward']:.2f} forwards; Fresnel lever flipped "
          f"{row['jvp_fresnel_lever_flipped_ms']:.2f} ms, first-slice lever "
          f"flipped {row['jvp_first_slice_lever_flipped_ms']:.2f} ms; d_scan "
          f"alone {row['jvp_scan_tangent_ms']:.2f} ms), "
          f"multislice_gauss_newton_product "
          f"{row['gauss_newton_product_ms']:.2f} ms; on one chunk: "
          f"tike_slice_wave_tangent behind the first slice "
          f"{row['slice_wave_tangent_chain_ms']:.3f} ms "
          f"({row['slice_wave_tangent_chain_share_of_8TBps']:.2f} of 8 TB/s), "
          f"slice 0 {row['slice_wave_tangent_first_ms']:.3f} / "
          f"{row['slice_wave_tangent_first_again_ms']:.3f} ms "
          f"({row['slice_wave_tangent_first_share_of_8TBps']:.2f} of 8 TB/s) "
          f"against tike_conv_fwd_tangent {row['conv_fwd_tangent_ms']:.3f} ms; "
          f"Fresnel step of the tangent: tike_fresnel_spect_prop "
          f"{row['fresnel_spect_prop_ms']:.3f} ms, three two-pass launches "
          + ("none (general route)" if two is None else f"{two:.3f} ms"),
          flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    repeats, warm = (1, 1) if args.once else (args.repeats, 2)
    rows = []
    for det, S, D in ((256, 8, 2), (128, 4, 3)):
        for fly in (1, 4):
            rows.append(legs(det, S, D, args.frames, fly, repeats, warm))
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0),
        rows=rows)))


if __name__ == "__main__":
    main()
