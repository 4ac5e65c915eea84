#!/usr/bin/env python3
"""Legs of fly-scan reconstruction on the GPU (not a test, not part of
bench.py):

    python tools/fly_legs.py [--repeats 10] [--frames 4000] [--fly 4]
                             [--kernel-only] [--once]

At 256^2 x 1 mode and 128^2 x 4 modes, `frames` frames of `fly` positions each,
it times with device events (warm-up first, median of the repeats)
  * `tike_fly_farplane_gradient` alone, with the gradient and costs only, as a
    time, as a rate on its byte model (the far plane read once and, with the
    gradient, written once, plus the counts) and as a fraction of the 8 TB/s
    HBM peak;
  * `tike_farplane_gradient` in the same process on the same frames * fly far
    planes (one pattern per position), and the ratio of the two per far-plane
    byte;
  * one cgrad epoch of `reconstruct(..., fly=fly)` on simulated data, in ms
    and in frames per second.
`--kernel-only` skips the epoch; `--once` runs every kernel exactly once after
the warm-up (for a counter collection run).  One line per shape, then one JSON
line with the library's build id."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tike_amd.ptycho as tp  # noqa: E402
from tike_amd import _arrays as A  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, reset, repeats, warmup=2):
    for _ in range(warmup):
        reset()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        reset()
        start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return statistics.median(ms)


def kernel_legs(det, S, frames, fly, repeats, once):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(det + S)
    N = frames * fly
    far0 = torch.view_as_complex(
        torch.randn((N, 1, S, det, det, 2), generator=gen, device=dev))
    far = torch.empty_like(far0)
    data = torch.poisson(torch.full((frames, det, det), 2.0 * fly * S,
                                    device=dev), generator=gen)
    data_each = data.repeat_interleave(fly, dim=0).contiguous()
    costs = torch.empty(N, dtype=torch.float32, device=dev)
    st = A.stream_ptr()
    reset = lambda: far.copy_(far0)  # noqa: E731

    def fly_kernel(grad):
        check(lib.tike_fly_farplane_gradient(
            A.ptr(far), A.ptr(data), 0, None, None, A.ptr(costs), frames, fly,
            S, det, 0, grad, 1.0, det * det, st), "tike_fly_farplane_gradient")

    def each_kernel(grad):
        check(lib.tike_farplane_gradient(
            A.ptr(far), A.ptr(data_each), None, None, A.ptr(costs), N, S, det,
            0, grad, 1.0, det * det, st), "tike_farplane_gradient")

    if once:
        repeats, warm = 1, 1
    else:
        warm = 2
    t = {name: timed(fn, reset, repeats, warm) for name, fn in (
        ("fly_gradient", lambda: fly_kernel(1)),
        ("fly_costs", lambda: fly_kernel(0)),
        ("each_gradient", lambda: each_kernel(1)),
        ("each_costs", lambda: each_kernel(0)))}
    plane = N * S * det * det * 8
    counts = frames * det * det * 4
    row = dict(det=det, modes=S, frames=frames, fly=fly,
               farplane_bytes=plane,
               fly_gradient_ms=t["fly_gradient"], fly_costs_ms=t["fly_costs"],
               each_gradient_ms=t["each_gradient"],
               each_costs_ms=t["each_costs"],
               fly_gradient_model_bytes=2 * plane + counts,
               fly_costs_model_bytes=plane + counts)
    row["fly_gradient_TB_per_s"] = (2 * plane + counts) / (
        t["fly_gradient"] * 1e-3) / 1e12
    row["fly_costs_TB_per_s"] = (plane + counts) / (
        t["fly_costs"] * 1e-3) / 1e12
    row["fly_gradient_fraction_of_8TBps"] = (
        row["fly_gradient_TB_per_s"] * 1e12 / HBM_PEAK)
    # the same far-plane bytes in both: the ratio of times is the ratio per byte
    row["fly_over_each_gradient"] = t["fly_gradient"] / t["each_gradient"]
    row["fly_over_each_costs"] = t["fly_costs"] / t["each_costs"]
    print(f"{det}^2 x {S} x {frames} frames x fly {fly}: fly kernel "
          f"{t['fly_gradient']:.3f} ms with the gradient "
          f"({row['fly_gradient_TB_per_s']:.2f} TB/s of its byte model, "
          f"{row['fly_gradient_fraction_of_8TBps']:.2f} of 8 TB/s), "
          f"{t['fly_costs']:.3f} ms costs only "
          f"({row['fly_costs_TB_per_s']:.2f} TB/s); per-position kernel on the "
          f"same planes {t['each_gradient']:.3f} / {t['each_costs']:.3f} ms; "
          f"fly / per-position {row['fly_over_each_gradient']:.3f} / "
          f"{row['fly_over_each_costs']:.3f}")
    return row


def epoch_leg(det, S, frames, fly, num_batch=4):
    rng = np.random.default_rng(det)
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
    data = tp.simulate(det, probe, scan, psi, fly=fly)
    params = tp.PtychoParameters(
        probe=probe, psi=(0.8 * psi + 0.1).astype(np.complex64), scan=scan,
        algorithm_options=tp.CgradOptions(num_batch=num_batch, cg_iter=2,
                                          num_iter=1),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((det, det), bool)))
    with tp.Reconstruction(data, params, fly=fly) as ctx:
        ctx.iterate(1)  # warm-up: workspaces, tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.iterate(1)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        costs = [float(c[0]) for c in ctx.get_convergence()[0]]
    print(f"{det}^2 x {S} x {frames} frames x fly {fly}: cgrad epoch "
          f"{ms:.1f} ms = {frames / ms * 1e3:.0f} frames/s "
          f"({num_batch} minibatches, 2 CG iterations each for object and "
          f"probe); costs {costs}")
    return dict(epoch_ms=ms, epoch_frames_per_s=frames / ms * 1e3,
                epoch_costs=costs, epoch_num_batch=num_batch)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--fly", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    rows = []
    for det, S in ((256, 1), (128, 4)):
        row = kernel_legs(det, S, args.frames, args.fly, args.repeats,
                          args.once)
        torch.cuda.empty_cache()
        if not args.kernel_only:
            row.update(epoch_leg(det, S, args.frames, args.fly))
            torch.cuda.empty_cache()
        rows.append(row)
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0),
        rows=rows)))


if __name__ == "__main__":
    main()
