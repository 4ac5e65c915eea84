#!/usr/bin/env python3
"""Timings of the difference map on the GPU (not a test, not part of bench.py;
what profiles/dm.md quotes):

    python tools/dm_timing.py [--repeats 7] [--positions 10000] [--epochs 3]
                              [--skip-epochs]

1. At 256^2 x 8 modes (819 positions) and 128^2 x 4 modes (4000 positions):
   `tike_dm_reflect` (with waves and with waves = NULL), `tike_dm_update`
   (without and with `change`) and, on the same planes, the streaming form of
   `tike_slice_wave_tangent` (a beam per position, dwave written over a dbeam
   per position), alternating, device events, 2 warm-up calls, median of the
   repeats: time per 1000 positions and the share of the 8 TB/s roofline on
   the algorithmic bytes of each (the planes written and read once; the
   object taps and the shared probe, which come from cache, left out).
2. One epoch of `dm` at bench.py's c3 shapes (256^2, 8 modes, `positions`
   positions, its generator; object and probe recovered, no eigen probes) on
   both routes of the exit-wave step, beside one epoch of `rpie` (10
   minibatches, the same problem, no eigen probes): 2 warm-up epochs, then
   `epochs` epochs under a host clock that ends in a synchronise.
3. The bytes of the waves at that shape and the allocator's peak.
One line per row, then one JSON line with the library's build id."""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from autograd_multislice_legs import HBM_PEAK, timed_alternating  # noqa: E402
from tike_amd import _arrays as A  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402


def entries(det, S, n, repeats):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(det + S)
    rc = lambda *shape: torch.view_as_complex(torch.randn(
        tuple(shape) + (2,), generator=gen, device=dev))
    side = int(np.ceil(np.sqrt(n)))
    H = W = 8 * side + det + 4
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side),
                              indexing="ij"), -1).reshape(-1, 2)[:n]
    scan = torch.from_numpy((1 + 8.0 * ij + np.random.default_rng(det).random(
        (n, 2))).astype(np.float32)).to(dev)
    psi, probe = rc(H, W), rc(S, det, det)
    waves, chi, near = rc(n, S, det, det), rc(n, S, det, det), rc(n, S, det,
                                                                  det)
    change = torch.empty(n, dtype=torch.float64, device=dev)
    st = A.stream_ptr()

    def reflect(w):
        return lambda: check(lib.tike_dm_reflect(
            A.ptr(psi), A.ptr(scan), A.ptr(probe), A.ptr(w), A.ptr(near), 0.8,
            n, S, det, det, H, W, st), "tike_dm_reflect")

    def update(c):
        return lambda: check(lib.tike_dm_update(
            A.ptr(waves), A.ptr(chi), A.ptr(psi), A.ptr(scan), A.ptr(probe),
            0.0625, A.ptr(c), n, S, det, det, H, W, st), "tike_dm_update")

    def tangent():  # the streaming form: three planes
        check(lib.tike_slice_wave_tangent(
            A.ptr(psi), None, A.ptr(scan), None, A.ptr(chi), 1, A.ptr(near),
            1, A.ptr(near), n, S, det, H, W, st), "tike_slice_wave_tangent")

    names = ("dm_reflect", "dm_reflect_null", "dm_update", "dm_update_change",
             "slice_wave_tangent")
    planes = dict(dm_reflect=2, dm_reflect_null=1, dm_update=3,
                  dm_update_change=3, slice_wave_tangent=3)
    ms = timed_alternating([reflect(waves), reflect(None), update(None),
                            update(change), tangent], repeats, 2)
    plane = n * S * det * det * 8
    row = dict(det=det, modes=S, positions=n)
    for name, t in zip(names, ms):
        nbytes = planes[name] * plane + n * 8
        row[name] = dict(ms=t, ms_per_1000=t * 1000 / n, model_bytes=nbytes,
                         TB_per_s=nbytes / (t * 1e-3) / 1e12,
                         share_of_8TBps=nbytes / (t * 1e-3) / HBM_PEAK)
    ref = row["slice_wave_tangent"]["share_of_8TBps"]
    for name in names[:-1]:
        row[name]["share_over_slice_wave_tangent"] = (
            row[name]["share_of_8TBps"] / ref)
    print(f"{det}^2 x {S} x {n} positions: " + "; ".join(
        f"{name} {row[name]['ms_per_1000']:.3f} ms per 1000 "
        f"({row[name]['share_of_8TBps']:.2f} of 8 TB/s)" for name in names),
          flush=True)
    return row


def epochs(positions, nepochs):
    import bench
    import tike_amd.ptycho as tp
    solver = importlib.import_module("tike_amd.ptycho.solvers.dm")
    det, S, N = 256, 8, positions
    p = bench.synthetic(N, S, det, 0, N)
    data = A.to_device(tp.simulate(det, p["probe"], p["scan"], p["psi"]),
                       np.float32)
    psi0 = np.full_like(p["psi"], 0.5 + 0j)
    row = dict(det=det, modes=S, positions=N,
               waves_bytes=N * S * det * det * 8)

    def run(options, num_batch, fused=True):
        solver.FUSED = fused
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        params = tp.PtychoParameters(
            probe=p["probe"].copy(), psi=psi0.copy(), scan=p["scan"],
            algorithm_options=options,
            probe_options=tp.ProbeOptions(force_orthogonality=True),
            object_options=tp.ObjectOptions())
        with tp.Reconstruction(
                data, params, presharded=True, order=np.arange(N),
                batches=np.array_split(np.arange(N), num_batch)) as ctx:
            ctx.iterate(2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.iterate(nepochs)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / nepochs
            costs = [c[0] for c in ctx.get_convergence()[0]]
        solver.FUSED = True
        return dict(ms_per_epoch=wall * 1e3, patterns_per_s=N / wall,
                    peak_allocated_bytes=torch.cuda.max_memory_allocated(),
                    costs=costs)

    row["dm_far_plane_free"] = run(tp.DmOptions(), 1, True)
    row["dm_stored"] = run(tp.DmOptions(), 1, False)
    row["rpie"] = run(tp.RpieOptions(num_batch=10,
                                     batch_method="wobbly_center"), 10)
    for name in ("dm_far_plane_free", "dm_stored", "rpie"):
        r = row[name]
        print(f"{name}: {r['ms_per_epoch']:.1f} ms per epoch, "
              f"{r['patterns_per_s'] / 1e3:.1f} k patterns/s, allocator peak "
              f"{r['peak_allocated_bytes'] / 2**30:.1f} GiB, costs "
              + " ".join(f"{c:.4g}" for c in r["costs"]), flush=True)
    print(f"waves: {row['waves_bytes'] / 2**30:.1f} GiB", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--positions", type=int, default=10000)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--skip-epochs", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    result = dict(build_id=build_id(), device=torch.cuda.get_device_name(0),
                  entries=[entries(256, 8, 819, args.repeats),
                           entries(128, 4, 4000, args.repeats)])
    if not args.skip_epochs:
        result["epochs"] = epochs(args.positions, args.epochs)
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main()
