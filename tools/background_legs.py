#!/usr/bin/env python3
"""Legs of a reconstruction with a fitted background on the GPU (not a test,
not part of bench.py):

    python tools/background_legs.py [--repeats 10] [--frames 4000]
                                    [--kernel-only]

At 256^2 x 1 mode and 128^2 x 4 modes, `frames` frames, fly 1 and 4, it times
with device events (warm-up first, median of the repeats)
  * `tike_background_farplane_gradient` with the gradient against
    `tike_fly_farplane_gradient` on the same planes in the same process;
  * `tike_background_sums` (both outputs) as a time, as a rate on its byte
    model (intensity and counts read once) and as a fraction of the 8 TB/s
    HBM peak;
  * one cgrad epoch of `reconstruct(..., background_options=)` with `update`
    on and off against the same epoch without `background_options`.
One line per leg, then one JSON line with the library's build id."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tike_amd.ptycho as tp  # noqa: E402
from tike_amd import _arrays as A  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402

from fly_legs import HBM_PEAK, timed  # noqa: E402


def kernel_legs(det, S, frames, fly, repeats):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(det + S)
    N = frames * fly
    far0 = torch.view_as_complex(
        torch.randn((N, 1, S, det, det, 2), generator=gen, device=dev))
    far = torch.empty_like(far0)
    data = torch.poisson(torch.full((frames, det, det), 2.0 * fly * S,
                                    device=dev), generator=gen)
    b = torch.rand((det, det), generator=gen, device=dev) + 0.5
    costs = torch.empty(frames, dtype=torch.float32, device=dev)
    inten = torch.empty((frames, det, det), dtype=torch.float32, device=dev)
    st = A.stream_ptr()
    reset = lambda: far.copy_(far0)  # noqa: E731

    def fly_kernel():
        check(lib.tike_fly_farplane_gradient(
            A.ptr(far), A.ptr(data), 0, None, None, A.ptr(costs), frames, fly,
            S, det, 0, 1, 1.0, det * det, st), "tike_fly_farplane_gradient")

    def background_kernel():
        check(lib.tike_background_farplane_gradient(
            A.ptr(far), A.ptr(data), 0, None, A.ptr(b), None, A.ptr(costs),
            frames, fly, S, det, 0, 1, 1.0, det * det, st),
            "tike_background_farplane_gradient")

    t_fly = timed(fly_kernel, reset, repeats)
    t_bg = timed(background_kernel, reset, repeats)
    t_fly2 = timed(fly_kernel, reset, repeats)
    far.copy_(far0)
    check(lib.tike_background_farplane_gradient(
        A.ptr(far), A.ptr(data), 0, None, A.ptr(b), A.ptr(inten), None,
        frames, fly, S, det, 0, 0, 1.0, det * det, st), "intensity")
    del far, far0
    torch.cuda.empty_cache()
    npix = det * det
    partials = torch.empty(lib.tike_background_sums_partials(npix),
                           dtype=torch.float64, device=dev)
    bgrad = torch.empty_like(b)

    def sums():
        check(lib.tike_background_sums(
            A.ptr(inten), A.ptr(data), 0, None, A.ptr(b), None,
            A.ptr(partials), A.ptr(bgrad), frames, npix, 0, npix, st),
            "tike_background_sums")

    t_sums = timed(sums, lambda: None, repeats)
    model = frames * npix * 8
    row = dict(det=det, modes=S, frames=frames, fly=fly,
               fly_gradient_ms=t_fly, fly_gradient_again_ms=t_fly2,
               background_gradient_ms=t_bg,
               background_over_fly=t_bg / min(t_fly, t_fly2),
               sums_ms=t_sums, sums_model_bytes=model,
               sums_TB_per_s=model / (t_sums * 1e-3) / 1e12,
               sums_fraction_of_8TBps=model / (t_sums * 1e-3) / HBM_PEAK)
    print(f"{det}^2 x {S} x {frames} frames x fly {fly}: background entry "
          f"{t_bg:.3f} ms with the gradient, fly entry {t_fly:.3f} / "
          f"{t_fly2:.3f} ms (before / after), ratio "
          f"{row['background_over_fly']:.3f}; tike_background_sums "
          f"{t_sums:.3f} ms = {row['sums_TB_per_s']:.2f} TB/s of its byte "
          f"model ({row['sums_fraction_of_8TBps']:.2f} of 8 TB/s)")
    return row


def epoch_legs(det, S, frames, fly, num_batch=4):
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
    truth = np.full((det, det), 0.5, np.float32)
    data = tp.simulate(det, probe, scan, psi, fly=fly, background=truth)
    out = {}
    for name, bo in (
            ("none", None),
            ("fixed", tp.BackgroundOptions(truth.copy(), update=False)),
            ("fitted", tp.BackgroundOptions(0.5 * truth))):
        params = tp.PtychoParameters(
            probe=probe, psi=(0.8 * psi + 0.1).astype(np.complex64), scan=scan,
            algorithm_options=tp.CgradOptions(num_batch=num_batch, cg_iter=2,
                                              num_iter=1),
            probe_options=tp.ProbeOptions(
                init_rescale_from_measurements=False),
            object_options=tp.ObjectOptions(),
            exitwave_options=tp.ExitWaveOptions(
                measured_pixels=np.ones((det, det), bool)))
        # (fly == 1 without background_options: the plain route with device
        # line searches, what such a call runs today)
        with tp.Reconstruction(data, params, fly=fly,
                               background_options=bo) as ctx:
            ctx.iterate(1)  # warm-up: workspaces, tables
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.iterate(1)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        out[f"epoch_{name}_ms"] = ms
        torch.cuda.empty_cache()
    print(f"{det}^2 x {S} x {frames} frames x fly {fly}: cgrad epoch "
          f"{out['epoch_none_ms']:.1f} ms without background_options, "
          f"{out['epoch_fixed_ms']:.1f} ms with update off, "
          f"{out['epoch_fitted_ms']:.1f} ms with update on (third block "
          f"{out['epoch_fitted_ms'] - out['epoch_fixed_ms']:.1f} ms; "
          f"{num_batch} minibatches, 2 CG iterations per block)")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    rows = []
    for det, S in ((256, 1), (128, 4)):
        for fly in (1, 4):
            row = kernel_legs(det, S, args.frames, fly, args.repeats)
            torch.cuda.empty_cache()
            if not args.kernel_only:
                row.update(epoch_legs(det, S, args.frames, fly))
            rows.append(row)
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0),
        rows=rows)))


if __name__ == "__main__":
    main()
