#!/usr/bin/env python3
"""Legs of `tike_amd.ptycho.position_pd_shifts` on the GPU (not a test, not
part of bench.py):

    python tools/position_pd_legs.py [--repeats 20] [--positions 1000]

At 256^2 x 8 modes and 128^2 x 1 mode, 1000 positions each, it times with
device events (warm-up first, median of the repeats)
  * the whole call, in ms per 1000 positions;
  * its stacked forward alone and `tike_position_pd_sums` alone, the latter
    also as a rate on its byte model (3 S npix 8 + npix 4 bytes read per
    position) and as a fraction of the 8 TB/s HBM peak;
  * the same `grad` formed from the SAME three far planes with plain torch
    expressions -- the reference's decomposition (position.py:654-689), the
    baseline: the commit before this one has nothing to time.
One line per shape, then one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tike_amd import _arrays as A  # noqa: E402
from tike_amd._lib import check, lib  # noqa: E402
from tike_amd.operators import Ptycho  # noqa: E402
from tike_amd.ptycho import position  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, repeats, warmup=3):
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


def torch_grad(far0, far_dx, far_dy, data, dx):
    """position.py:654-689 as array expressions, mode by mode."""
    n = far0.shape[0]
    inten = torch.sum(far0.real**2 + far0.imag**2, dim=1)
    residual = (data - inten).reshape(n, -1)
    d_dx = d_dy = 0
    for m in range(far0.shape[1]):
        f = far0[:, m]
        d_dx = d_dx + 2 * torch.real((f - far_dx[:, m]) / dx * f.conj())
        d_dy = d_dy + 2 * torch.real((f - far_dy[:, m]) / dx * f.conj())
    design = torch.stack((d_dy.reshape(n, -1), d_dx.reshape(n, -1)), dim=-1)
    normal = design.transpose(-1, -2) @ design
    rhs = design.transpose(-1, -2) @ residual[..., None]
    return torch.linalg.solve(normal, rhs)[..., 0]


def legs(det, S, N, repeats):
    rng = np.random.default_rng(det + S)
    side = det + 40
    dev = torch.device("cuda")
    cplx = lambda *s: torch.from_numpy(  # noqa: E731
        (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(
            np.complex64)).to(dev)
    psi, probe = cplx(1, side, side), cplx(1, 1, S, det, det) / det
    scan = torch.from_numpy(rng.uniform(4, 34, (N, 2)).astype(
        np.float32)).to(dev)
    dx = -1.0
    with Ptycho(det, det, nz=side, n=side) as op:
        moves = torch.tensor([[0, 0], [0, dx], [dx, 0]], dtype=torch.float32,
                             device=dev)
        stacked = (scan[None] + moves[:, None]).reshape(3 * N, 2).contiguous()
        work = torch.empty((3 * N, 1, S, det, det), dtype=torch.complex64,
                           device=dev)
        forward = lambda: op.fwd_device(probe, stacked, psi, out=work)  # noqa: E731
        forward()
        far = work.reshape(3, N, S, det, det)
        # patterns of positions half a pixel away: a residual worth fitting
        data = torch.sum(op.fwd_device(probe, scan + 0.5, psi).abs()**2,
                         dim=(1, 2)).contiguous()
        sums = torch.empty((N, 5), dtype=torch.float32, device=dev)
        costs = torch.empty((N,), dtype=torch.float32, device=dev)

        def kernel():
            check(lib.tike_position_pd_sums(
                A.ptr(far[0]), A.ptr(far[1]), A.ptr(far[2]), A.ptr(data), 0,
                1.0 / dx, A.ptr(sums), A.ptr(costs), N, S, det * det,
                A.stream_ptr()), "tike_position_pd_sums")

        whole = lambda: position.position_pd_shifts(  # noqa: E731
            op, data, psi, probe, scan, dx)
        flat = far.reshape(3, N, S, det * det)
        plain = lambda: torch_grad(flat[0], flat[1], flat[2],  # noqa: E731
                                   data.reshape(N, -1), dx)
        t_whole = timed(whole, repeats)
        t_forward = timed(forward, repeats)
        t_kernel = timed(kernel, repeats)
        t_plain = timed(plain, max(3, repeats // 4), warmup=2)
        grad = whole()
        miss = float(torch.linalg.norm(grad - plain()) /
                     torch.linalg.norm(grad))
    model = N * (3 * S * det * det * 8 + det * det * 4 + 24)
    rate = model / (t_kernel * 1e-3)
    per_k = 1000.0 / N
    row = dict(det=det, modes=S, positions=N,
               whole_ms_per_1000=t_whole * per_k,
               forward_ms_per_1000=t_forward * per_k,
               sums_ms_per_1000=t_kernel * per_k,
               sums_bytes=model, sums_TB_per_s=rate / 1e12,
               sums_fraction_of_8TBps=rate / HBM_PEAK,
               torch_sums_ms_per_1000=t_plain * per_k,
               torch_over_kernel=t_plain / t_kernel,
               grad_normwise_vs_torch=miss)
    print(f"{det}^2 x {S} x {N}: whole {row['whole_ms_per_1000']:.3f} ms / "
          f"1000 positions (forward {row['forward_ms_per_1000']:.3f}, sums "
          f"{row['sums_ms_per_1000']:.3f}); sums {rate / 1e12:.2f} TB/s = "
          f"{rate / HBM_PEAK:.2f} of 8 TB/s; torch expressions on the same "
          f"far planes {row['torch_sums_ms_per_1000']:.3f} ms "
          f"({row['torch_over_kernel']:.1f} x the kernel); grad normwise "
          f"difference {miss:.1e}")
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--positions", type=int, default=1000)
    args = ap.parse_args()
    A.require_gpu()
    rows = [legs(256, 8, args.positions, args.repeats),
            legs(128, 1, args.positions, args.repeats)]
    print("RESULT " + json.dumps(rows))


if __name__ == "__main__":
    main()
