#!/usr/bin/env python3
"""Legs of reconstruction under detector binning on the GPU (not a test, not
part of bench.py):

    python tools/binned_legs.py [--repeats 10] [--gib 8] [--epoch-frames 4000]
                                [--kernel-only]

Kernel legs, at 256^2 x 8 modes with binning 2 and at 128^2 x 4 modes x fly 2
with binning 4, on `gib` GiB of far plane: `tike_binned_farplane_gradient`
against `tike_fly_farplane_gradient` ON THE SAME FAR PLANES (the fly entry
reads counts at far-plane resolution, the binned entry B^2 times fewer), with
the gradient and costs only, and `tike_binned_cost_factor` with its table
against `tike_cost_factor`.  Device events, warm-up first, the two entries
alternating inside every repeat, median of the repeats; the far plane is
restored before every timed call, outside the timed region.  Times, rates on
each entry's byte model, fractions of the 8 TB/s HBM peak, and the ratio
binned / fly.

Epoch legs, at 256^2 x 1 mode: one cgrad epoch of `reconstruct` (4 minibatches,
2 CG iterations each for object and probe, the second epoch timed) with
(fly, binning) = (4, 1) -- the leg of profiles/fly_scan.md, the yardstick on
this box --, (4, 2) and (1, 2).

One line per leg, then one JSON line with the library's build id."""
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


def timed_alternating(legs, reset, repeats, warmup=2):
    """{name: median ms} of the legs, run one after the other inside every
    repeat so that drift of the box hits all of them alike."""
    for _ in range(warmup):
        for fn in legs.values():
            reset()
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            reset()
            start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ms[name].append(start.elapsed_time(stop))
    return {name: statistics.median(v) for name, v in ms.items()}


def kernel_legs(det, S, fly, B, gib, repeats):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(det + S + B)
    P, w = fly * S, det // B
    frames = max(1, int(gib * 2**30) // (P * det * det * 8))
    N = frames * fly
    far0 = torch.view_as_complex(
        torch.randn((N, 1, S, det, det, 2), generator=gen, device=dev))
    far = torch.empty_like(far0)
    fine = torch.poisson(torch.full((frames, det, det), 2.0 * P, device=dev),
                         generator=gen)
    coarse = torch.poisson(torch.full((frames, w, w), 2.0 * P * B * B,
                                      device=dev), generator=gen)
    costs = torch.empty(frames, dtype=torch.float32, device=dev)
    table = torch.empty((frames, det, det), dtype=torch.float32, device=dev)
    st = A.stream_ptr()
    reset = lambda: far.copy_(far0)  # noqa: E731

    def fly_kernel(grad):
        check(lib.tike_fly_farplane_gradient(
            A.ptr(far), A.ptr(fine), 0, None, None, A.ptr(costs), frames, fly,
            S, det, 0, grad, 1.0, det * det, st), "tike_fly_farplane_gradient")

    def binned_kernel(grad):
        check(lib.tike_binned_farplane_gradient(
            A.ptr(far), A.ptr(coarse), 0, None, None, A.ptr(costs), frames,
            fly, S, det, B, 0, grad, 1.0, w * w, st),
            "tike_binned_farplane_gradient")

    def factor():
        check(lib.tike_cost_factor(
            A.ptr(far), A.ptr(fine), 0, None, None, None, A.ptr(table), frames,
            P, det * det, 0, det * det, st), "tike_cost_factor")

    def binned_factor():
        check(lib.tike_binned_cost_factor(
            A.ptr(far), A.ptr(coarse), 0, None, None, None, A.ptr(table),
            frames, P, det * det, 0, w * w, det, B, st),
            "tike_binned_cost_factor")

    t = timed_alternating(dict(
        fly_gradient=lambda: fly_kernel(1),
        binned_gradient=lambda: binned_kernel(1),
        fly_costs=lambda: fly_kernel(0),
        binned_costs=lambda: binned_kernel(0),
        factor_table=factor, binned_factor_table=binned_factor), reset, repeats)
    plane = N * S * det * det * 8
    nfine, ncoarse = frames * det * det * 4, frames * w * w * 4
    model = dict(fly_gradient=2 * plane + nfine,
                 binned_gradient=2 * plane + ncoarse,
                 fly_costs=plane + nfine, binned_costs=plane + ncoarse,
                 factor_table=plane + 2 * nfine,
                 binned_factor_table=plane + ncoarse + nfine)
    row = dict(det=det, modes=S, fly=fly, binning=B, frames=frames,
               farplane_bytes=plane,
               rows_in_registers=bool(B * P <= 32))
    for name, ms in t.items():
        row[name + "_ms"] = ms
        row[name + "_model_bytes"] = model[name]
        row[name + "_TB_per_s"] = model[name] / (ms * 1e-3) / 1e12
        row[name + "_fraction_of_8TBps"] = model[name] / (ms * 1e-3) / HBM_PEAK
    for kind in ("gradient", "costs", "factor_table"):
        f = "fly_" + kind if kind != "factor_table" else kind
        row["binned_over_fly_" + kind] = t["binned_" + kind] / t[f]
    print(f"{det}^2 x {S} modes x fly {fly}, binning {B}, {frames} frames "
          f"({plane / 2**30:.2f} GiB of far plane, B * P = {B * P}): gradient "
          f"binned {t['binned_gradient']:.3f} ms "
          f"({row['binned_gradient_TB_per_s']:.2f} TB/s of its byte model) / "
          f"fly {t['fly_gradient']:.3f} ms "
          f"({row['fly_gradient_TB_per_s']:.2f} TB/s) = "
          f"{row['binned_over_fly_gradient']:.3f}; costs only "
          f"{t['binned_costs']:.3f} / {t['fly_costs']:.3f} ms = "
          f"{row['binned_over_fly_costs']:.3f}; cost factor with its table "
          f"{t['binned_factor_table']:.3f} / {t['factor_table']:.3f} ms = "
          f"{row['binned_over_fly_factor_table']:.3f}")
    return row


def epoch_leg(det, S, frames, fly, B, num_batch=4):
    """One timed cgrad epoch; the problem of tools/fly_legs.py, the counts
    binned by `simulate`."""
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
    data = tp.simulate(det, probe, scan, psi, fly=fly, binning=B)
    w = det // B
    params = tp.PtychoParameters(
        probe=probe, psi=(0.8 * psi + 0.1).astype(np.complex64), scan=scan,
        algorithm_options=tp.CgradOptions(num_batch=num_batch, cg_iter=2,
                                          num_iter=1),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((w, w), bool)))
    with tp.Reconstruction(data, params, fly=fly, binning=B) as ctx:
        ctx.iterate(1)  # warm-up: workspaces, tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.iterate(1)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        costs = [float(c[0]) for c in ctx.get_convergence()[0]]
    print(f"{det}^2 x {S} x {frames} frames x fly {fly}, binning {B}: cgrad "
          f"epoch {ms:.1f} ms = {frames / ms * 1e3:.0f} frames/s "
          f"({num_batch} minibatches, 2 CG iterations each for object and "
          f"probe); costs {costs}")
    return dict(det=det, modes=S, frames=frames, fly=fly, binning=B,
                epoch_ms=ms, epoch_frames_per_s=frames / ms * 1e3,
                epoch_costs=costs, epoch_num_batch=num_batch)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--epoch-frames", type=int, default=4000)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    rows, epochs = [], []
    for det, S, fly, B in ((256, 8, 1, 2), (128, 4, 2, 4)):
        rows.append(kernel_legs(det, S, fly, B, args.gib, args.repeats))
        torch.cuda.empty_cache()
    if not args.kernel_only:
        for fly, B in ((4, 1), (4, 2), (1, 2)):
            epochs.append(epoch_leg(256, 1, args.epoch_frames, fly, B))
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0),
        rows=rows, epochs=epochs)))


if __name__ == "__main__":
    main()
