#!/usr/bin/env python3
"""Legs of the differentiable MULTISLICE intensity model on the GPU (not a
test, not part of bench.py):

    python tools/autograd_multislice_legs.py [--repeats 5] [--frames 4000]
                                             [--once] [--no-cgrad]

At 256^2 x 8 modes x 2 slices and 128^2 x 4 modes x 3 slices, `frames` frames
of `fly` = 1 and 4 positions each, it times with device events (2 warm-up
calls, median of the repeats)
  * one forward of `tike_amd.autograd.multislice_intensity` and one forward +
    backward with all three gradients (loss = sum(g * I), a random signed g),
    the latter also with `PASS1_TAKES_TABLE` off (the upstream gradient by
    `tike_farplane_scale` + `tike_fft2_pass1` instead of
    `tike_ifft2_pass1_scaled`), the two alternating;
  * in the same process, one cgrad gradient evaluation of the same object,
    probe and positions with both gradients (`_multislice_cost_and_grad`, one
    pattern per position: the yardstick; cgrad has no multislice fly scans);
  * `tike_scan_gradient_slices` alone, launched chunk by chunk as the backward
    launches it, as a time, as a share of the forward + backward, and as a
    share of the 8 TB/s roofline on its byte model (csrc/autograd.hip).
`--once` runs everything exactly once after one warm-up call (for a
`rocprofv3 --kernel-trace --stats` run, which gives the kernels' own times);
`--no-cgrad` skips the cgrad leg.  One line per shape, then one JSON line with
the library's build id."""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tike_amd.ptycho as tp  # noqa: E402
from tike_amd import _arrays as A  # noqa: E402
from tike_amd import autograd  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402

# (the package exports the solver function under the module's name)
C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")

HBM_PEAK = 8.0e12
PIXEL, WAVELENGTH, DISTANCE = 1e-8, 1e-10, 2e-6  # 10 nm, 1 A, 2 um


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return statistics.median(ms)


def timed_alternating(fns, repeats, warmup=2):
    """Medians of several callables timed in turn, a b a b ...: what drifts
    over the run (clocks, neighbours) falls on all alike."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ms[k].append(start.elapsed_time(stop))
    return [statistics.median(m) for m in ms]


def problem(det, S, D, frames, fly):
    """Host arrays of a raster of `frames` frames, `fly` positions each, over
    D slices."""
    rng = np.random.default_rng(det + fly)
    side = int(np.ceil(np.sqrt(frames)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:frames]
    start = 2 + 6.0 * ij + rng.random((frames, 2))
    along = np.arange(fly)[None, :, None] * np.array([0.0, 1.25])[None, None]
    scan = (start[:, None] + along).reshape(-1, 2).astype(np.float32)
    extent = int(6 * (side - 1) + det + 8 + 1.25 * fly)
    psi = ((0.8 + 0.2 * rng.random((D, extent, extent))) * np.exp(
        0.3j * rng.standard_normal((D, extent, extent)))).astype(np.complex64)
    probe = np.stack([
        tp.gaussian(det, rin=0.6) * np.exp(1j * np.pi * rng.random((det, det)))
        / (m + 1) for m in range(S)])[None, None].astype(np.complex64)
    return psi, probe, scan


def legs(det, S, D, frames, fly, repeats, warm, with_cgrad):
    dev = torch.device("cuda")
    psi_h, probe_h, scan_h = problem(det, S, D, frames, fly)
    N = frames * fly
    H, W = psi_h.shape[-2:]
    row = dict(det=det, modes=S, slices=D, frames=frames, fly=fly,
               positions=N)
    # cgrad's yardstick reads one pattern per position; the counts do not
    # change what is launched
    data = np.ones((N, det, det), np.float32)
    params = tp.PtychoParameters(
        probe=probe_h, psi=psi_h, scan=scan_h,
        algorithm_options=tp.CgradOptions(num_batch=1, cg_iter=1, num_iter=1),
        probe_options=tp.ProbeOptions(
            init_rescale_from_measurements=False, probe_wavelength=WAVELENGTH,
            probe_FOV_lengths=(det * PIXEL, det * PIXEL)),
        object_options=tp.ObjectOptions(
            multislice_propagation_distance=DISTANCE),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((det, det), bool)))
    with tp.Reconstruction(data, params) as ctx:
        p, op = ctx.parameters, ctx.operator
        psi, probe, scan = (x.detach().clone().requires_grad_(True)
                            for x in (p.psi, p.probe, p.scan))
        g = torch.randn((frames, det, det), device=dev)
        f = autograd.multislice_intensity

        def forward():
            with torch.no_grad():
                f(op, psi, probe, scan, fly=fly)

        def both(table=True):
            autograd.PASS1_TAKES_TABLE = table
            for x in (psi, probe, scan):
                x.grad = None
            (f(op, psi, probe, scan, fly=fly) * g).sum().backward()
            autograd.PASS1_TAKES_TABLE = True

        row["forward_ms"] = timed(forward, repeats, warm)
        (row["forward_backward_ms"],
         row["forward_backward_two_launch_table_ms"]) = timed_alternating(
             [both, lambda: both(False)], repeats, warm)
        row["pass1_takes_table"] = bool(autograd.PASS1_TAKES_TABLE)
        # the route and the chunk of the model (ptycho/solvers/_multislice.py)
        route = autograd._SlicesForward(op, fly, psi.detach(), probe.detach(),
                                        scan.detach())
        row["fused_route"] = route.fused
        row["chunk_positions"] = min(route.chunk, N)
        if with_cgrad:
            cm = C._cost_model(p.exitwave_options, det)
            one = lambda: C._multislice_cost_and_grad(  # noqa: E731
                op, ctx.comm, ctx.data, p.psi, p.scan, p.probe, 0, N,
                want_psi=True, want_probe=True, want_grad=True, cm=cm)
            row["cgrad_gradient_ms"] = timed(one, repeats, warm)
            row["forward_backward_over_cgrad"] = (
                row["forward_backward_ms"] / row["cgrad_gradient_ms"])
        scan_d = p.scan.detach().clone()
        psi_d = p.psi.detach().clone()
    torch.cuda.empty_cache()
    # the new entry alone, chunk by chunk as the backward launches it
    st = A.stream_ptr()
    nmax = row["chunk_positions"]
    gen = torch.Generator(device=dev).manual_seed(det + S + fly)
    objproj = torch.view_as_complex(
        torch.randn((D, nmax, det, det, 2), generator=gen, device=dev))
    grad = torch.empty((N, 2), dtype=torch.float32, device=dev)

    def slices():
        for lo in range(0, N, nmax):
            n = min(N, lo + nmax) - lo
            check(
                lib.tike_scan_gradient_slices(
                    A.ptr(objproj), nmax * det * det, A.ptr(scan_d[lo:]),
                    A.ptr(psi_d), A.ptr(grad[lo:]), n, D, det, H, W, st),
                "tike_scan_gradient_slices")

    row["scan_gradient_slices_ms"] = timed(slices, repeats, warm)
    row["scan_gradient_slices_share_of_forward_backward"] = (
        row["scan_gradient_slices_ms"] / row["forward_backward_ms"])
    row["scan_gradient_slices_model_bytes"] = (
        N * D * (det * det + (det + 1)**2) * 8)
    rate = (row["scan_gradient_slices_model_bytes"]
            / (row["scan_gradient_slices_ms"] * 1e-3))
    row["scan_gradient_slices_TB_per_s"] = rate / 1e12
    row["scan_gradient_slices_share_of_8TBps"] = rate / HBM_PEAK
    del objproj
    torch.cuda.empty_cache()
    cg = (f"; cgrad gradient {row['cgrad_gradient_ms']:.2f} ms (forward + "
          f"backward / cgrad {row['forward_backward_over_cgrad']:.2f})"
          if with_cgrad else "")
    print(f"{det}^2 x {S} x {D} slices x {frames} frames x fly {fly} "
          f"({'fused' if row['fused_route'] else 'general'} route, chunks of "
          f"{nmax}): forward {row['forward_ms']:.2f} ms, forward + backward "
          f"{row['forward_backward_ms']:.2f} ms (table by two launches "
          f"{row['forward_backward_two_launch_table_ms']:.2f} ms){cg}; "
          f"tike_scan_gradient_slices {row['scan_gradient_slices_ms']:.3f} ms "
          f"({row['scan_gradient_slices_share_of_forward_backward']:.3f} of "
          f"forward + backward, "
          f"{row['scan_gradient_slices_share_of_8TBps']:.2f} of 8 TB/s)",
          flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no-cgrad", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    repeats, warm = (1, 1) if args.once else (args.repeats, 2)
    rows = []
    for det, S, D in ((256, 8, 2), (128, 4, 3)):
        for fly in (1, 4):
            rows.append(legs(det, S, D, args.frames, fly, repeats, warm,
                             not args.no_cgrad))
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0),
        rows=rows)))


if __name__ == "__main__":
    main()
