#!/usr/bin/env python3
"""Legs of the forward-mode derivative of the differentiable intensity model
on the GPU (not a test, not part of bench.py):

    python tools/autograd_jvp_legs.py [--repeats 10] [--frames 4000] [--once]

At 256^2 x 1 mode and 128^2 x 4 modes, `frames` frames of `fly` = 1 and 4
positions each, it times with device events (2 warm-up calls, median of the
repeats), all in one process
  * one forward of `tike_amd.autograd.intensity` and one forward + backward
    with all three gradients (loss = sum(g * I), a random signed g);
  * `intensity_jvp` with all three tangents and with `d_scan` alone;
  * `gauss_newton_product` with all three tangents and all three parts;
  * each launch of `intensity_jvp` alone on arrays of the same shape:
    `tike_ptycho_fwd`, `tike_conv_fwd_tangent` (three tangents, and `d_scan`
    alone), `tike_fft2` in place, `tike_intensity_tangent` -- the two new
    entries also as a share of the 8 TB/s roofline on their byte models
    (csrc/autograd_jvp.hip).
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
from autograd_legs import HBM_PEAK, problem, timed  # noqa: E402
from tike_amd import _arrays as A  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402
from tike_amd.autograd import (gauss_newton_product, intensity,  # noqa: E402
                               intensity_jvp)
from tike_amd.operators.propagation import fft_scales  # noqa: E402


def legs(det, S, frames, fly, repeats, warm):
    dev = torch.device("cuda")
    psi_h, probe_h, scan_h = problem(det, S, frames, fly)
    N = frames * fly
    H, W = psi_h.shape[-2:]
    row = dict(det=det, modes=S, frames=frames, fly=fly, positions=N)
    psi, probe, scan = (torch.from_numpy(x).to(dev).requires_grad_(True)
                        for x in (psi_h, probe_h, scan_h))
    gen = torch.Generator(device=dev).manual_seed(det + S + fly)
    rc = lambda x: torch.view_as_complex(torch.randn(
        tuple(x.shape) + (2,), generator=gen, device=dev))
    d_psi, d_probe = rc(psi), rc(probe)
    d_scan = torch.randn(scan.shape, generator=gen, device=dev)
    g = torch.randn((frames, det, det), generator=gen, device=dev)
    with ops.Ptycho(probe_shape=det, detector_shape=det, nz=H, n=W) as op:

        def forward():
            with torch.no_grad():
                intensity(op, psi, probe, scan, fly=fly)

        def both():
            for x in (psi, probe, scan):
                x.grad = None
            (intensity(op, psi, probe, scan, fly=fly) * g).sum().backward()

        row["forward_ms"] = timed(forward, repeats, warm)
        row["forward_backward_ms"] = timed(both, repeats, warm)
        row["jvp_three_tangents_ms"] = timed(lambda: intensity_jvp(
            op, psi, probe, scan, d_psi=d_psi, d_probe=d_probe, d_scan=d_scan,
            fly=fly), repeats, warm)
        row["jvp_scan_tangent_ms"] = timed(lambda: intensity_jvp(
            op, psi, probe, scan, d_scan=d_scan, fly=fly), repeats, warm)
        row["gauss_newton_product_ms"] = timed(lambda: gauss_newton_product(
            op, psi, probe, scan, d_psi=d_psi, d_probe=d_probe, d_scan=d_scan,
            fly=fly), repeats, warm)
        # every launch of intensity_jvp alone
        st = A.stream_ptr()
        P, D, Sc = psi.detach(), probe.detach(), scan.detach()
        far = torch.empty((N, 1, S, det, det), dtype=torch.complex64,
                          device=dev)
        dfar = torch.empty_like(far)
        inten = torch.empty((frames, det, det), dtype=torch.float32,
                            device=dev)
        tangent = torch.empty_like(inten)
        row["ptycho_fwd_ms"] = timed(
            lambda: op.fwd_device(D, Sc, P, out=far), repeats, warm)

        def conv(dp, ds, dq):
            check(lib.tike_conv_fwd_tangent(
                A.ptr(P), A.ptr(dp), A.ptr(Sc), A.ptr(ds), A.ptr(D), A.ptr(dq),
                A.ptr(dfar), N, S, det, det, H, W, st),
                "tike_conv_fwd_tangent")

        row["conv_fwd_tangent_scan_ms"] = timed(
            lambda: conv(None, d_scan, None), repeats, warm)
        row["conv_fwd_tangent_ms"] = timed(
            lambda: conv(d_psi, d_scan, d_probe), repeats, warm)
        scale = fft_scales(det, op.norm)[0]
        row["fft2_ms"] = timed(lambda: check(lib.tike_fft2(
            A.ptr(dfar), A.ptr(dfar), N * S, det, 0, scale, st), "tike_fft2"),
            repeats, warm)
        conv(d_psi, d_scan, d_probe)  # (finite values for the last leg)
        row["intensity_tangent_ms"] = timed(
            lambda: check(lib.tike_intensity_tangent(
                A.ptr(far), A.ptr(dfar), A.ptr(inten), A.ptr(tangent), frames,
                S * fly, det * det, st), "tike_intensity_tangent"),
            repeats, warm)
    plane = N * S * det * det * 8
    # written once; object and probe reads come from cache (csrc/autograd_jvp.hip)
    row["conv_fwd_tangent_model_bytes"] = plane + N * 16
    row["intensity_tangent_model_bytes"] = 2 * plane + 2 * frames * det * det * 4
    for name in ("conv_fwd_tangent", "intensity_tangent"):
        rate = row[name + "_model_bytes"] / (row[name + "_ms"] * 1e-3)
        row[name + "_TB_per_s"] = rate / 1e12
        row[name + "_share_of_8TBps"] = rate / HBM_PEAK
    del far, dfar
    torch.cuda.empty_cache()
    print(f"{det}^2 x {S} x {frames} frames x fly {fly}: forward "
          f"{row['forward_ms']:.2f} ms, forward + backward "
          f"{row['forward_backward_ms']:.2f} ms; intensity_jvp "
          f"{row['jvp_three_tangents_ms']:.2f} ms (d_scan alone "
          f"{row['jvp_scan_tangent_ms']:.2f} ms), gauss_newton_product "
          f"{row['gauss_newton_product_ms']:.2f} ms; tike_ptycho_fwd "
          f"{row['ptycho_fwd_ms']:.3f} ms, tike_conv_fwd_tangent "
          f"{row['conv_fwd_tangent_ms']:.3f} ms (d_scan alone "
          f"{row['conv_fwd_tangent_scan_ms']:.3f} ms; "
          f"{row['conv_fwd_tangent_share_of_8TBps']:.2f} of 8 TB/s), tike_fft2 "
          f"{row['fft2_ms']:.3f} ms, tike_intensity_tangent "
          f"{row['intensity_tangent_ms']:.3f} ms "
          f"({row['intensity_tangent_share_of_8TBps']:.2f} of 8 TB/s)",
          flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    repeats, warm = (1, 1) if args.once else (args.repeats, 2)
    rows = []
    for det, S in ((256, 1), (128, 4)):
        for fly in (1, 4):
            rows.append(legs(det, S, args.frames, fly, repeats, warm))
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0), rows=rows)))


if __name__ == "__main__":
    main()
