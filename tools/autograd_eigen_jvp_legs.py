#!/usr/bin/env python3
"""Legs of the forward-mode derivative of the differentiable intensity model
with eigen probes on the GPU (not a test, not part of bench.py):

    python tools/autograd_eigen_jvp_legs.py [--repeats 10] [--frames 4000]
                                            [--shape 0|1] [--fly N] [--once]

Shapes (those of tools/autograd_eigen_legs.py): 0 = 256^2 x 8 modes with one
eigen probe on mode 0, 1 = 128^2 x 4 modes with 2 eigen probes on all 4;
`frames` frames of `fly` = 1 and 4 positions each (all four without --shape /
--fly).  For every shape it times with device events (2 warm-up calls, median
of the repeats)
  * `tike_eigen_wave_tangent` with all five tangents next to
    `tike_conv_fwd_tangent` with its three on the same S, pw and det, the two
    ALTERNATING call by call, on ONE chunk of positions as `eigen_intensity_jvp`
    cuts them (half of `chunk_positions`) -- the two write identical bytes --,
    the new entry also as a share of the 8 TB/s roofline on the S det^2 8
    bytes per position it writes, and with `d_scan` and `d_eigen_weights`
    alone (the tangents of the joint refinement);
  * `eigen_intensity_jvp` with all five tangents next to the forward of
    `intensity(..., eigen_probe=, eigen_weights=)` alone, and to forward +
    backward with all five gradients (loss = sum(g * I), a random signed g);
  * `eigen_gauss_newton_product` with all five tangents and all five parts.
`--once` runs the two entries exactly once after one warm-up call and skips
the end-to-end legs (for a `rocprofv3 --kernel-trace --stats` run, which gives
the kernels' own times).  One line per shape, then one JSON line with the
library's build id."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import tike_amd.operators as ops  # noqa: E402
from autograd_eigen_legs import SHAPES, problem, timed_pair  # noqa: E402
from autograd_legs import HBM_PEAK, timed  # noqa: E402
from tike_amd import _arrays as A  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402
from tike_amd.autograd import (eigen_gauss_newton_product,  # noqa: E402
                               eigen_intensity_jvp, intensity)
from tike_amd.ptycho.solvers.lstsq import chunk_positions  # noqa: E402


def legs(det, S, C, M, frames, fly, repeats, warm, once):
    dev = torch.device("cuda")
    psi, probe, scan, eigen, weights = (torch.from_numpy(a).to(dev) for a in
                                        problem(det, S, C, M, frames, fly))
    N, pw = frames * fly, det
    H, W = psi.shape[-2:]
    row = dict(det=det, modes=S, eigen=C, eigen_modes=M, frames=frames,
               fly=fly, positions=N)
    st = A.stream_ptr()
    A.current_device()
    gen = torch.Generator(device=dev).manual_seed(det + S + fly)
    rc = lambda x: torch.view_as_complex(torch.randn(
        tuple(x.shape) + (2,), generator=gen, device=dev))
    d_psi, d_probe, d_eigen = rc(psi), rc(probe), rc(eigen)
    d_scan = torch.randn(scan.shape, generator=gen, device=dev)
    d_weights = torch.randn(weights.shape, generator=gen, device=dev)
    # ---- the two entries on one chunk of positions, as the JVP cuts them
    chunk = max(1, chunk_positions(S, det) // 2 // fly) * fly
    rows = min(chunk, N)
    row["chunk_positions"] = rows
    near = torch.empty((rows, S, det, det), dtype=torch.complex64, device=dev)

    def new(dp, ds, dq, de, dw):
        check(lib.tike_eigen_wave_tangent(
            A.ptr(psi), A.ptr(dp), A.ptr(scan), A.ptr(ds), A.ptr(probe),
            A.ptr(dq), A.ptr(eigen), A.ptr(de), A.ptr(weights), A.ptr(dw), C,
            M, A.ptr(near), rows, S, pw, det, H, W, st),
            "tike_eigen_wave_tangent")

    def old():
        check(lib.tike_conv_fwd_tangent(
            A.ptr(psi), A.ptr(d_psi), A.ptr(scan), A.ptr(d_scan), A.ptr(probe),
            A.ptr(d_probe), A.ptr(near), rows, S, pw, det, H, W, st),
            "tike_conv_fwd_tangent")

    five = lambda: new(d_psi, d_scan, d_probe, d_eigen, d_weights)
    (row["eigen_wave_tangent_ms"],
     row["conv_fwd_tangent_ms"]) = timed_pair(five, old, repeats, warm)
    row["eigen_wave_tangent_scan_weights_ms"] = timed(
        lambda: new(None, d_scan, None, None, d_weights), repeats, warm)
    row["new_over_old"] = (row["eigen_wave_tangent_ms"]
                           / row["conv_fwd_tangent_ms"])
    # written once; the planes and the object taps come from cache
    row["model_bytes"] = rows * S * det * det * 8
    rate = row["model_bytes"] / (row["eigen_wave_tangent_ms"] * 1e-3)
    row["eigen_wave_tangent_TB_per_s"] = rate / 1e12
    row["eigen_wave_tangent_share_of_8TBps"] = rate / HBM_PEAK
    row["conv_fwd_tangent_share_of_8TBps"] = (
        row["model_bytes"] / (row["conv_fwd_tangent_ms"] * 1e-3) / HBM_PEAK)
    del near
    torch.cuda.empty_cache()
    line = (f"{det}^2 x {S} + {C} eigen on {M} x {frames} frames x fly {fly}: "
            f"tike_eigen_wave_tangent ({rows} positions, five tangents) "
            f"{row['eigen_wave_tangent_ms']:.3f} ms "
            f"({row['eigen_wave_tangent_share_of_8TBps']:.2f} of 8 TB/s), "
            f"tike_conv_fwd_tangent {row['conv_fwd_tangent_ms']:.3f} ms "
            f"({row['conv_fwd_tangent_share_of_8TBps']:.2f}), new / old "
            f"{row['new_over_old']:.2f}; d_scan + d_eigen_weights alone "
            f"{row['eigen_wave_tangent_scan_weights_ms']:.3f} ms")
    if once:
        print(line, flush=True)
        return row
    # ---- end to end
    leaves = [x.requires_grad_(True) for x in (psi, probe, scan, eigen,
                                               weights)]
    g = torch.randn((frames, det, det), generator=gen, device=dev)
    kw = dict(eigen_probe=eigen, eigen_weights=weights, fly=fly)
    t = dict(d_psi=d_psi, d_probe=d_probe, d_scan=d_scan,
             d_eigen_probe=d_eigen, d_eigen_weights=d_weights)
    with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:

        def forward():
            with torch.no_grad():
                intensity(op, psi, probe, scan, **kw)

        def both():
            for x in leaves:
                x.grad = None
            (intensity(op, psi, probe, scan, **kw) * g).sum().backward()

        jvp = lambda: eigen_intensity_jvp(op, psi, probe, scan, **kw, **t)
        row["jvp_five_tangents_ms"], row["forward_ms"] = timed_pair(
            jvp, forward, repeats, warm)
        row["forward_backward_ms"] = timed(both, repeats, warm)
        row["jvp_scan_weights_ms"] = timed(lambda: eigen_intensity_jvp(
            op, psi, probe, scan, d_scan=d_scan, d_eigen_weights=d_weights,
            **kw), repeats, warm)
        row["gauss_newton_product_ms"] = timed(
            lambda: eigen_gauss_newton_product(op, psi, probe, scan, **kw,
                                               **t), repeats, warm)
    row["jvp_over_forward"] = row["jvp_five_tangents_ms"] / row["forward_ms"]
    row["jvp_over_forward_backward"] = (row["jvp_five_tangents_ms"]
                                        / row["forward_backward_ms"])
    print(line + f"; eigen_intensity_jvp {row['jvp_five_tangents_ms']:.2f} ms "
          f"(d_scan + d_eigen_weights alone {row['jvp_scan_weights_ms']:.2f} "
          f"ms), forward {row['forward_ms']:.2f} ms "
          f"(x {row['jvp_over_forward']:.2f}), forward + backward "
          f"{row['forward_backward_ms']:.2f} ms "
          f"(x {row['jvp_over_forward_backward']:.2f}), "
          f"eigen_gauss_newton_product {row['gauss_newton_product_ms']:.2f} ms",
          flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--shape", type=int, choices=(0, 1))
    ap.add_argument("--fly", type=int)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    repeats, warm = (1, 1) if args.once else (args.repeats, 2)
    rows = []
    for k, (det, S, C, M) in enumerate(SHAPES):
        if args.shape not in (None, k):
            continue
        for fly in ((1, 4) if args.fly is None else (args.fly,)):
            rows.append(legs(det, S, C, M, args.frames, fly, repeats, warm,
                             args.once))
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0), rows=rows)))


if __name__ == "__main__":
    main()
