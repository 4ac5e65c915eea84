#!/usr/bin/env python3
"""Legs of the differentiable intensity model with eigen probes on the GPU
(not a test, not part of bench.py):

    python tools/autograd_eigen_legs.py [--repeats 10] [--frames 4000]
                                        [--shape 0|1] [--fly N] [--once]

Shapes: 0 = 256^2 x 8 modes with one eigen probe on mode 0 (S = 8, C = 1,
M = 1: the c3 configuration; the kernel compiled for 8 modes + one eigen
probe), 1 = 128^2 x 4 modes with C = 2, M = 4 (the general kernel); `frames`
frames of `fly` = 1 and 4 positions each (all four without --shape / --fly).
For every shape it times with device events (2 warm-up calls, median of the
repeats), the two runs of a pair ALTERNATING call by call:
  * `tike_eigen_probe_gradients` with all four outputs next to
    `tike_lstsq_gradients` with both outputs and the shared probe, on the same
    chi, launched chunk by chunk as the backward launches them;
  * forward + backward of `tike_amd.autograd.intensity` with eigen probes and
    all five gradients next to the shared-probe forward + backward with its
    three (loss = sum(g * I), a random signed g), and the two forwards alone.
`--once` runs the two entries exactly once after one warm-up call and skips
the end-to-end leg (for a `rocprofv3 --kernel-trace --stats` run, which gives
the kernels' own times).  One line per shape, then one JSON line with the
library's build id."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tike_amd.operators as ops  # noqa: E402
import tike_amd.ptycho as tp  # noqa: E402
from tike_amd import _arrays as A  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402
from tike_amd.autograd import intensity  # noqa: E402
from tike_amd.ptycho.solvers.lstsq import chunk_positions  # noqa: E402

SHAPES = ((256, 8, 1, 1), (128, 4, 2, 4))  # det = pw, S, C, M


def timed_pair(fa, fb, repeats, warmup=2):
    """Medians (ms) of fa and fb, called in turn."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(repeats):
        for k, fn in enumerate((fa, fb)):
            start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ms[k].append(start.elapsed_time(stop))
    return statistics.median(ms[0]), statistics.median(ms[1])


def problem(det, S, C, M, frames, fly):
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
    window = tp.gaussian(det, rin=0.6)
    phase = lambda: np.exp(1j * np.pi * rng.random((det, det)))
    probe = np.stack([window * phase() / (m + 1)
                      for m in range(S)])[None, None].astype(np.complex64)
    eigen = 0.3 * np.stack([[window * phase() / (m + 1) for m in range(M)]
                            for _ in range(C)])[None].astype(np.complex64)
    N = frames * fly
    weights = 0.1 * rng.standard_normal((N, C + 1, S))
    weights[:, 0] += 1
    return psi, probe, scan, eigen, weights.astype(np.float32)


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
    # ---- the two entries on the same chi, chunk by chunk as the backward
    chunk = max(1, chunk_positions(S, det) // fly) * fly
    rows = min(chunk, N)
    gen = torch.Generator(device=dev).manual_seed(det + S + fly)
    chi = torch.view_as_complex(
        torch.randn((rows, S, pw, pw, 2), generator=gen, device=dev))
    objproj = torch.empty((rows, pw, pw), dtype=torch.complex64, device=dev)
    gprobe, geigen = torch.zeros_like(probe), torch.zeros_like(eigen)
    gweights = torch.empty_like(weights)
    work = torch.empty((-(-pw * pw // 256), rows, S + C * M),
                       dtype=torch.float64, device=dev)

    def eigen_entry():
        for lo in range(0, N, chunk):
            n = min(N, lo + chunk) - lo
            check(lib.tike_eigen_probe_gradients(
                A.ptr(chi), A.ptr(scan[lo:]), A.ptr(psi), A.ptr(probe),
                A.ptr(eigen), A.ptr(weights[lo:]), C, M, A.ptr(gprobe),
                A.ptr(geigen), A.ptr(gweights[lo:]), A.ptr(objproj),
                A.ptr(work), n, S, pw, H, W, st),
                "tike_eigen_probe_gradients")

    def lstsq_entry():
        for lo in range(0, N, chunk):
            n = min(N, lo + chunk) - lo
            check(lib.tike_lstsq_gradients(
                A.ptr(chi), A.ptr(scan[lo:]), A.ptr(psi), A.ptr(probe), None,
                None, 0, 0, None, None, A.ptr(gprobe), A.ptr(objproj), n, S,
                pw, H, W, st), "tike_lstsq_gradients")

    row["chunk"] = chunk
    row["eigen_gradients_ms"], row["lstsq_gradients_ms"] = timed_pair(
        eigen_entry, lstsq_entry, repeats, warm)
    row["entry_ratio"] = row["eigen_gradients_ms"] / row["lstsq_gradients_ms"]
    row["chi_bytes"] = N * S * pw * pw * 8
    row["eigen_gradients_chi_TB_per_s"] = (
        row["chi_bytes"] / (row["eigen_gradients_ms"] * 1e-3) / 1e12)
    line = (f"{det}^2 x {S} modes, C = {C}, M = {M}, {frames} frames x fly "
            f"{fly}: tike_eigen_probe_gradients "
            f"{row['eigen_gradients_ms']:.3f} ms, tike_lstsq_gradients "
            f"{row['lstsq_gradients_ms']:.3f} ms (ratio "
            f"{row['entry_ratio']:.3f})")
    del chi, objproj, work
    torch.cuda.empty_cache()
    if not once:
        # ---- end to end, all five gradients against the shared probe's three
        g = torch.randn((frames, det, det), device=dev)
        leaves = [x.detach().clone().requires_grad_(True)
                  for x in (psi, probe, scan, eigen, weights)]
        with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:

            def with_eigen():
                for x in leaves:
                    x.grad = None
                (intensity(op, *leaves[:3], eigen_probe=leaves[3],
                           eigen_weights=leaves[4], fly=fly) * g).sum(
                               ).backward()

            def shared():
                for x in leaves:
                    x.grad = None
                (intensity(op, *leaves[:3], fly=fly) * g).sum().backward()

            def forward_eigen():
                with torch.no_grad():
                    intensity(op, *leaves[:3], eigen_probe=leaves[3],
                              eigen_weights=leaves[4], fly=fly)

            def forward_shared():
                with torch.no_grad():
                    intensity(op, *leaves[:3], fly=fly)

            (row["eigen_forward_backward_ms"],
             row["shared_forward_backward_ms"]) = timed_pair(
                 with_eigen, shared, repeats, warm)
            row["eigen_forward_ms"], row["shared_forward_ms"] = timed_pair(
                forward_eigen, forward_shared, repeats, warm)
        row["forward_backward_ratio"] = (row["eigen_forward_backward_ms"]
                                         / row["shared_forward_backward_ms"])
        line += (f"; forward + backward with eigen probes (five gradients) "
                 f"{row['eigen_forward_backward_ms']:.2f} ms, shared probe "
                 f"(three) {row['shared_forward_backward_ms']:.2f} ms (ratio "
                 f"{row['forward_backward_ratio']:.3f}); forward alone "
                 f"{row['eigen_forward_ms']:.2f} / "
                 f"{row['shared_forward_ms']:.2f} ms")
    print(line, flush=True)
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
    for k, shape in enumerate(SHAPES):
        for fly in (1, 4):
            if args.shape in (None, k) and args.fly in (None, fly):
                rows.append(legs(*shape, args.frames, fly, repeats, warm,
                                 args.once))
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0),
        rows=rows)))


if __name__ == "__main__":
    main()
