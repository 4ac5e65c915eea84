#!/usr/bin/env python3
"""Legs of the differentiable intensity model on the GPU (not a test, not part
of bench.py):

    python tools/autograd_legs.py [--repeats 10] [--frames 4000] [--once]
                                  [--no-cgrad]

At 256^2 x 1 mode and 128^2 x 4 modes, `frames` frames of `fly` = 1 and 4
positions each, it times with device events (2 warm-up calls, median of the
repeats)
  * one forward of `tike_amd.autograd.intensity` and one forward + backward
    with all three gradients (loss = sum(g * I), a random signed g);
  * in the same process, one cgrad gradient evaluation of the same shape with
    both gradients (`_cost_and_grad`; `_fly_cost_and_grad` for fly > 1);
  * the two new entries alone on arrays of the same shape,
    `tike_farplane_scale` and `tike_scan_gradient`, as a time and as a share
    of the 8 TB/s roofline on their byte models (csrc/autograd.hip).
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
from tike_amd._lib import build_id, check, lib  # noqa: E402
from tike_amd.autograd import intensity  # noqa: E402

# (the package exports the solver function under the module's name)
C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")

HBM_PEAK = 8.0e12


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


def problem(det, S, frames, fly):
    """Host arrays of a raster of `frames` frames, `fly` positions each."""
    rng = np.random.default_rng(det + fly)
    side = int(np.ceil(np.sqrt(frames)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:frames]
    start = 2 + 6.0 * ij + rng.random((frames, 2))
    along = np.arange(fly)[None, :, None] * np.array([0.0, 1.25])[None, None]
    scan = (start[:, None] + along).reshape(-1, 2).astype(np.float32)
    extent = int(6 * (side - 1) + det + 8 + 1.25 * fly)
    psi = ((0.75 + 0.25 * rng.random((1, extent, extent))) * np.exp(
        1j * np.pi * (rng.random((1, extent, extent)) - 0.5))).astype(
            np.complex64)
    probe = np.stack([
        tp.gaussian(det, rin=0.6) * np.exp(1j * np.pi * rng.random((det, det)))
        / (m + 1) for m in range(S)])[None, None].astype(np.complex64)
    return psi, probe, scan


def legs(det, S, frames, fly, repeats, warm, with_cgrad):
    dev = torch.device("cuda")
    psi_h, probe_h, scan_h = problem(det, S, frames, fly)
    N = frames * fly
    H, W = psi_h.shape[-2:]
    row = dict(det=det, modes=S, frames=frames, fly=fly, positions=N)
    data = tp.simulate(det, probe_h, scan_h, psi_h, fly=fly)
    params = tp.PtychoParameters(
        probe=probe_h, psi=(0.8 * psi_h + 0.1).astype(np.complex64),
        scan=scan_h,
        algorithm_options=tp.CgradOptions(num_batch=1, cg_iter=1, num_iter=1),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((det, det), bool)))
    with tp.Reconstruction(data, params, fly=fly) as ctx:
        p, op = ctx.parameters, ctx.operator
        psi, probe, scan = (x.detach().clone().requires_grad_(True)
                            for x in (p.psi, p.probe, p.scan))
        g = torch.randn((frames, det, det), device=dev)

        def forward():
            with torch.no_grad():
                intensity(op, psi, probe, scan, fly=fly)

        def both():
            for x in (psi, probe, scan):
                x.grad = None
            (intensity(op, psi, probe, scan, fly=fly) * g).sum().backward()

        row["forward_ms"] = timed(forward, repeats, warm)
        row["forward_backward_ms"] = timed(both, repeats, warm)
        if with_cgrad:
            cm = C._cost_model(p.exitwave_options, det)
            want = dict(want_psi=True, want_probe=True, want_grad=True, cm=cm)
            if fly > 1:
                one = lambda: C._fly_cost_and_grad(  # noqa: E731
                    op, ctx.comm, ctx.data, p.psi, p.scan, p.probe, 0, N, fly,
                    **want)
            else:
                one = lambda: C._cost_and_grad(  # noqa: E731
                    op, ctx.comm, ctx.data, p.psi, p.scan, p.probe, 0, N,
                    **want)
            row["cgrad_gradient_ms"] = timed(one, repeats, warm)
            row["forward_backward_over_cgrad"] = (
                row["forward_backward_ms"] / row["cgrad_gradient_ms"])
        scan_d = p.scan.detach()
        psi_d = p.psi.detach()
    torch.cuda.empty_cache()
    # the two new entries alone, on arrays of this shape
    st = A.stream_ptr()
    gen = torch.Generator(device=dev).manual_seed(det + S + fly)
    far = torch.view_as_complex(
        torch.randn((N, 1, S, det, det, 2), generator=gen, device=dev))
    row["farplane_scale_ms"] = timed(lambda: check(lib.tike_farplane_scale(
        A.ptr(far), A.ptr(g), frames, fly * S, det * det, 1.0, st),
        "tike_farplane_scale"), repeats, warm)
    row["farplane_scale_model_bytes"] = (2 * N * S * det * det * 8
                                         + frames * det * det * 4)
    del far
    objproj = torch.view_as_complex(
        torch.randn((N, det, det, 2), generator=gen, device=dev))
    grad = torch.empty((N, 2), dtype=torch.float32, device=dev)
    row["scan_gradient_ms"] = timed(lambda: check(lib.tike_scan_gradient(
        A.ptr(objproj), A.ptr(scan_d), A.ptr(psi_d), A.ptr(grad), N, det, H, W,
        st), "tike_scan_gradient"), repeats, warm)
    row["scan_gradient_model_bytes"] = N * (det * det + (det + 1)**2) * 8
    for name in ("farplane_scale", "scan_gradient"):
        rate = row[name + "_model_bytes"] / (row[name + "_ms"] * 1e-3)
        row[name + "_TB_per_s"] = rate / 1e12
        row[name + "_share_of_8TBps"] = rate / HBM_PEAK
    del objproj
    torch.cuda.empty_cache()
    cg = (f"; cgrad gradient {row['cgrad_gradient_ms']:.2f} ms (forward + "
          f"backward / cgrad {row['forward_backward_over_cgrad']:.2f})"
          if with_cgrad else "")
    print(f"{det}^2 x {S} x {frames} frames x fly {fly}: forward "
          f"{row['forward_ms']:.2f} ms, forward + backward "
          f"{row['forward_backward_ms']:.2f} ms{cg}; tike_farplane_scale "
          f"{row['farplane_scale_ms']:.3f} ms "
          f"({row['farplane_scale_share_of_8TBps']:.2f} of 8 TB/s), "
          f"tike_scan_gradient {row['scan_gradient_ms']:.3f} ms "
          f"({row['scan_gradient_share_of_8TBps']:.2f} of 8 TB/s)", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no-cgrad", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    repeats, warm = (1, 1) if args.once else (args.repeats, 2)
    rows = []
    for det, S in ((256, 1), (128, 4)):
        for fly in (1, 4):
            rows.append(legs(det, S, args.frames, fly, repeats, warm,
                             not args.no_cgrad))
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0),
        rows=rows)))


if __name__ == "__main__":
    main()
