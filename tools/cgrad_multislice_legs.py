#!/usr/bin/env python3
"""Legs of multislice cgrad on the GPU (not a test, not part of bench.py):

    python tools/cgrad_multislice_legs.py [--positions 4000] [--chunk 1000]
        [--repeats 7] [--kernel-only] [--markdown FILE]

At 256^2 x 8 modes x 2 slices it measures

  (a) per `chunk` positions, with device events, `tike_slice_step_back`
      against the pair of launches it replaces on the same tiles:
      `tike_ifft2_pass2_products(keep_chi=1)` followed by `tike_fft2_pass1`.
      The pair has no conj(patch) multiply, so it does strictly less
      arithmetic; it moves 4 T (T = the chunk's waves) where the one launch
      moves 2 T + the incident probes.  Three alternations new / pair in one
      process, each the median of `repeats` calls after a warm-up; the figure
      of a side is the median of its three.  The hand-off the pair overwrites
      is restored before every call, outside the timed region.
  (b) one cgrad epoch of `Reconstruction` on simulated two-slice data, Poisson
      model, in patterns per second, on the fused route and on the general
      route (`cgrad.MULTISLICE_FUSED = False`), and on the fused route with
      the three-launch step back (`cgrad.MULTISLICE_STEP_BACK_FUSED = False`).

One line per figure, then one JSON line with the library's build id; with
--markdown the two tables are written to FILE."""
import argparse
import importlib
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
from tike_amd.operators.propagation import fft_scales  # noqa: E402

# (the package exports the solver function under the module's name)
C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
DET, MODES, SLICES = 256, 8, 2
PIXEL, WAVELENGTH, DISTANCE = 1e-8, 1e-10, 2e-6


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


def kernel_leg(n, repeats):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    det, S = DET, MODES
    H = W = det + 200
    rand = lambda *shape: torch.view_as_complex(
        torch.randn((*shape, 2), generator=gen, device=dev))
    work0, beam, psi = rand(n, S, det, det), rand(n, S, det, det), rand(H, W)
    work, far1 = torch.empty_like(work0), torch.empty_like(work0)
    objproj = torch.empty((n, det, det), dtype=torch.complex64, device=dev)
    side = int(np.ceil(np.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:n]
    scan = torch.from_numpy(
        (2 + ij * (190.0 / side) + np.random.default_rng(0).random((n, 2))
         ).astype(np.float32)).to(dev)
    inv_scale = fft_scales(det, "ortho")[1]
    st = A.stream_ptr()
    reset = lambda: work.copy_(work0)  # noqa: E731

    def fused():
        check(lib.tike_slice_step_back(
            A.ptr(work), A.ptr(psi), A.ptr(scan), A.ptr(beam), A.ptr(objproj),
            A.ptr(far1), n, S, det, H, W, inv_scale, st),
            "tike_slice_step_back")

    def pair():
        check(lib.tike_ifft2_pass2_products(
            A.ptr(work), A.ptr(psi), A.ptr(scan), A.ptr(beam), 1,
            A.ptr(objproj), None, 1.0, None, 1, n, S, det, H, W, inv_scale,
            st), "tike_ifft2_pass2_products")
        check(lib.tike_fft2_pass1(A.ptr(work), A.ptr(far1), n * S, det, 0,
                                  st), "tike_fft2_pass1")

    rounds = []
    for _ in range(3):
        rounds.append((timed(fused, reset, repeats),
                       timed(pair, reset, repeats)))
    t_fused = statistics.median(r[0] for r in rounds)
    t_pair = statistics.median(r[1] for r in rounds)
    T = n * S * det * det * 8
    print(f"{det}^2 x {S} modes, {n} positions: tike_slice_step_back "
          f"{t_fused:.3f} ms (rounds {[round(r[0], 3) for r in rounds]}), "
          f"pair {t_pair:.3f} ms (rounds {[round(r[1], 3) for r in rounds]}); "
          f"T = {T / 1e9:.2f} GB")
    return dict(positions=n, fused_ms=t_fused, pair_ms=t_pair,
                fused_rounds_ms=[r[0] for r in rounds],
                pair_rounds_ms=[r[1] for r in rounds], wave_bytes=T)


def problem(N):
    det, S, D = DET, MODES, SLICES
    rng = np.random.default_rng(det)
    side = int(np.ceil(np.sqrt(N)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:N]
    scan = (2 + 6.0 * ij + rng.random((N, 2))).astype(np.float32)
    extent = int(6 * (side - 1) + det + 8)
    psi = ((0.8 + 0.2 * rng.random((D, extent, extent))) * np.exp(
        0.3j * rng.standard_normal((D, extent, extent)))).astype(np.complex64)
    probe = np.stack([
        tp.gaussian(det, rin=0.6) * np.exp(1j * np.pi * rng.random((det, det)))
        / (m + 1) for m in range(S)])[None, None].astype(np.complex64)
    optics = dict(probe_wavelength=WAVELENGTH,
                  probe_FOV_lengths=(det * PIXEL, det * PIXEL))
    data = tp.simulate(det, probe, scan, psi,
                       multislice_propagation_distance=DISTANCE, **optics)
    params = lambda: tp.PtychoParameters(  # noqa: E731
        probe=probe.copy(), psi=(0.8 * psi + 0.1).astype(np.complex64),
        scan=scan.copy(),
        algorithm_options=tp.CgradOptions(num_batch=4, cg_iter=2, num_iter=1),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False,
                                      **optics),
        object_options=tp.ObjectOptions(
            multislice_propagation_distance=DISTANCE),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((det, det), bool), noise_model="poisson"))
    return data, params


def epoch_leg(data, params, name, fused, one_launch):
    C.MULTISLICE_FUSED, C.MULTISLICE_STEP_BACK_FUSED = fused, one_launch
    N = data.shape[0]
    with tp.Reconstruction(data, params()) as ctx:
        ctx.iterate(1)  # warm-up: workspaces, tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.iterate(1)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        costs = [float(c[0]) for c in ctx.get_convergence()[0]]
    print(f"cgrad epoch, {name}: {ms:.1f} ms = {N / ms * 1e3:.0f} patterns/s; "
          f"costs {costs}")
    return dict(route=name, epoch_ms=ms, patterns_per_s=N / ms * 1e3,
                costs=costs)


def markdown(path, result):
    k = result["kernel"]
    per = 1000.0 / k["positions"]
    lines = [
        "# Multislice cgrad: the step back through a slice and an epoch",
        "",
        f"One {result['device']}, `tools/cgrad_multislice_legs.py`; library "
        f"build id `{result['build_id']}`.",
        f"{DET}^2 x {MODES} modes x {SLICES} slices.",
        "",
        "## (a) The step back, per 1000 positions",
        "",
        f"Device events, {k['positions']} positions per call, three "
        "alternations new / pair in one process, each the median of "
        f"{result['repeats']} calls; scaled to 1000 positions.  The pair does "
        "no conj(patch) multiply.",
        "",
        "| launches | round 1 | round 2 | round 3 | median |",
        "|---|---|---|---|---|",
        "| `tike_slice_step_back` | " + " | ".join(
            f"{v * per:.3f} ms" for v in k["fused_rounds_ms"])
        + f" | {k['fused_ms'] * per:.3f} ms |",
        "| `tike_ifft2_pass2_products(keep_chi=1)` + `tike_fft2_pass1` | "
        + " | ".join(f"{v * per:.3f} ms" for v in k["pair_rounds_ms"])
        + f" | {k['pair_ms'] * per:.3f} ms |",
        "",
    ]
    if result["epochs"]:
        lines += [
            "## (b) One cgrad epoch",
            "",
            f"{result['positions']} positions, Poisson model, 4 minibatches, 2 "
            "CG iterations each for the object (both slices at once) and the "
            "probe, host-side line searches; the second epoch of a context, "
            "host clock around a device synchronise.",
            "",
            "| route | epoch | patterns/s |",
            "|---|---|---|",
        ] + [f"| {e['route']} | {e['epoch_ms']:.1f} ms | "
             f"{e['patterns_per_s']:.0f} |" for e in result["epochs"]] + [""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--positions", type=int, default=4000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--markdown")
    args = ap.parse_args()
    A.require_gpu()
    result = dict(build_id=build_id(), device=torch.cuda.get_device_name(0),
                  positions=args.positions, repeats=args.repeats,
                  kernel=kernel_leg(args.chunk, args.repeats), epochs=[])
    torch.cuda.empty_cache()
    if not args.kernel_only:
        data, params = problem(args.positions)
        for name, fused, one_launch in (
                ("fused, one-launch step back", True, True),
                ("fused, three-launch step back", True, False),
                ("general operators", False, True)):
            result["epochs"].append(
                epoch_leg(data, params, name, fused, one_launch))
            torch.cuda.empty_cache()
    if args.markdown:
        markdown(args.markdown, result)
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main()
