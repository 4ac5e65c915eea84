#!/usr/bin/env python3
"""Legs of a reconstruction with a far-field blur on the GPU (not a test, not
part of bench.py):

    python tools/blur_legs.py [--repeats 10] [--frames 4000] [--kernel-only]
                              [--no-pitch]

With device events (warm-up first, median of the repeats) it times
  * `tike_blur_cost_factor` (costs and table) at 256^2 and 128^2, k = 3, 5, 7,
    as a time, as a rate on its byte model (intensity 4 B + counts 4 B + mask
    1 B read, table 4 B written per pixel and frame) and as a fraction of the
    8 TB/s HBM peak, beside `tike_cost_factor` on a far plane of the same
    frames at fly * S = 1; and `tike_blur_kernel_sums` with and without kgrad;
  * one gradient evaluation of cgrad's whole-frames route with a blur (k = 5),
    split into forward / intensities / blur / scale / adjoint on a chunk,
    against the same evaluation with a zero background
    (`tike_background_farplane_gradient`: the whole-frames route at fly = 1
    before blur_options existed), at 256^2 x 1 mode and 128^2 x 4 modes x
    fly 2;
  * one cgrad epoch at 256^2 with 1 mode and blur_options (update on and off)
    against the 8-mode epoch on the same positions without.
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

NOTHING = lambda: None  # noqa: E731


def gaussian_kernel(k, sigma=0.8):
    x = np.arange(k) - k // 2
    g = np.exp(-(x[:, None]**2 + x[None, :]**2) / (2 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def kernel_legs(det, frames, repeats):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(det)
    npix = det * det
    far = torch.view_as_complex(
        torch.randn((frames, 1, npix, 2), generator=gen, device=dev))
    data = torch.poisson(torch.full((frames, det, det), 2.0, device=dev),
                         generator=gen)
    mask = torch.ones((det, det), dtype=torch.uint8, device=dev)
    mask[det // 3] = 0
    nm = int(mask.sum())
    inten = torch.empty((frames, det, det), dtype=torch.float32, device=dev)
    costs = torch.empty(frames, dtype=torch.float32, device=dev)
    table = torch.empty_like(inten)
    st = A.stream_ptr()
    check(lib.tike_intensity(A.ptr(far), A.ptr(inten), frames, 1, npix, st),
          "tike_intensity")

    def plain():
        check(lib.tike_cost_factor(
            A.ptr(far), A.ptr(data), 0, A.ptr(mask), None, A.ptr(costs),
            A.ptr(table), frames, 1, npix, 0, nm, st), "tike_cost_factor")

    rows = []
    t_plain = timed(plain, NOTHING, repeats)
    for k in (3, 5, 7):
        K = torch.from_numpy(gaussian_kernel(k)).to(dev)
        n = lib.tike_blur_kernel_sums_partials(det, k)
        partials = torch.empty(n, dtype=torch.float64, device=dev)
        kgrad = torch.empty((k, k), dtype=torch.float64, device=dev)

        def blur(want_table=True):
            check(lib.tike_blur_cost_factor(
                A.ptr(inten), A.ptr(K), k, A.ptr(data), 0, A.ptr(mask), None,
                A.ptr(costs), A.ptr(table) if want_table else None, None,
                frames, det, 0, nm, st), "tike_blur_cost_factor")

        def sums(want_grad=True):
            check(lib.tike_blur_kernel_sums(
                A.ptr(inten), A.ptr(K), k, A.ptr(data), 0, A.ptr(mask), None,
                A.ptr(partials), A.ptr(kgrad) if want_grad else None, frames,
                det, 0, nm, st), "tike_blur_kernel_sums")

        t_blur = timed(blur, NOTHING, repeats)
        t_costs = timed(lambda: blur(False), NOTHING, repeats)
        t_sums = timed(sums, NOTHING, repeats)
        t_trial = timed(lambda: sums(False), NOTHING, repeats)
        model = frames * npix * (4 + 4 + 1 + 4)
        sums_model = frames * npix * (4 + 4)
        rows.append(dict(
            det=det, k=k, frames=frames, cost_factor_ms=t_plain,
            blur_cost_factor_ms=t_blur, blur_costs_only_ms=t_costs,
            model_bytes=model,
            fraction_of_8TBps=model / (t_blur * 1e-3) / HBM_PEAK,
            lds_taps_per_s=2.0 * k * k * frames * npix / (t_blur * 1e-3),
            kernel_sums_ms=t_sums, kernel_sums_trial_ms=t_trial,
            kernel_sums_fraction_of_8TBps=sums_model / (t_sums * 1e-3)
            / HBM_PEAK,
            trial_fraction_of_8TBps=sums_model / (t_trial * 1e-3) / HBM_PEAK))
        r = rows[-1]
        print(f"{det}^2 x {frames} frames, k = {k}: tike_blur_cost_factor "
              f"{t_blur:.3f} ms with the table ({r['fraction_of_8TBps']:.3f} "
              f"of 8 TB/s on 13 B per pixel; {r['lds_taps_per_s'] / 1e12:.2f} "
              f"T taps/s), {t_costs:.3f} ms costs only; tike_cost_factor at "
              f"fly * S = 1 {t_plain:.3f} ms; tike_blur_kernel_sums "
              f"{t_sums:.3f} ms with kgrad "
              f"({r['kernel_sums_fraction_of_8TBps']:.3f} of 8 TB/s on 8 B "
              f"per pixel), {t_trial:.3f} ms without "
              f"({r['trial_fraction_of_8TBps']:.3f})")
    return rows


def _problem(det, S, frames, fly, blur=None):
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
    data = tp.simulate(det, probe, scan, psi, fly=fly, blur=blur)
    return scan, psi, probe, data


def _parameters(scan, psi, probe, det, num_batch):
    return tp.PtychoParameters(
        probe=probe, psi=(0.8 * psi + 0.1).astype(np.complex64), scan=scan,
        algorithm_options=tp.CgradOptions(num_batch=num_batch, cg_iter=2,
                                          num_iter=1),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((det, det), bool)))


def gradient_legs(det, S, frames, fly, repeats, k=5):
    """One gradient evaluation (object) of a minibatch of all frames, blur
    against zero background, and the legs of a chunk of the blur route."""
    import importlib
    cg = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    from tike_amd.operators.detector import Detector
    from tike_amd.ptycho import background as B
    from tike_amd.ptycho import blur as U
    K = gaussian_kernel(k)
    scan, psi, probe, data = _problem(det, S, frames, fly, blur=K)
    params = _parameters(scan, psi, probe, det, 1)
    N = scan.shape[0]
    out = dict(det=det, modes=S, frames=frames, fly=fly, k=k)
    with tp.Reconstruction(data, params, fly=fly, order=np.arange(N),
                           batches=[np.arange(N)]) as ctx:
        op, comm, p = ctx.operator, ctx.comm, ctx.parameters
        cm = cg._cost_model(p.exitwave_options, det)
        dev = p.psi.device
        states = dict(
            blur=U.State(tp.BlurOptions(K), K),
            background=B.State(
                tp.BackgroundOptions(np.zeros((det, det), np.float32)),
                np.zeros((det, det), np.float32)))
        for name, state in states.items():
            mb = cg._Minibatch(op, comm, ctx.data, p.psi, p.scan, p.probe, 0,
                               N, cm, fly, Detector(name), state)
            out[f"{name}_gradient_ms"] = timed(
                lambda: mb.evaluate(p.psi, p.probe, 0, True), NOTHING,
                repeats)
            out[f"{name}_trial_ms"] = timed(
                lambda: mb.evaluate(p.psi, p.probe, None, False), NOTHING,
                repeats)
        # the legs of one chunk of the blur route
        chunk = max(1, cg.chunk_positions(S, det) // fly) * fly
        n = min(N, chunk)
        nf = n // fly
        far = torch.empty((n, 1, S, det, det), dtype=torch.complex64,
                          device=dev)
        inten = torch.empty((nf, det, det), dtype=torch.float32, device=dev)
        table = torch.empty_like(inten)
        costs = torch.empty(nf, dtype=torch.float32, device=dev)
        unit = torch.full((nf,), float(cm.nmeasured), device=dev)
        K_d = torch.from_numpy(K).to(dev)
        d = ctx.data[:nf]
        sc = p.scan[:n]
        fwd = lambda: op.fwd_device(p.probe, sc, p.psi, out=far)  # noqa: E731
        legs = dict(
            forward=fwd,
            intensities=lambda: op.fly_farplane_gradient(far, d, fly,
                                                         intensity=inten),
            blur=lambda: op.blur_cost_factor(
                inten, K_d, d, model=cm.model, measured=cm.mask,
                num_measured=cm.nmeasured, upstream=unit, costs=costs,
                table=table),
            scale=lambda: check(lib.tike_farplane_scale(
                A.ptr(far), A.ptr(table), nf, S * fly, det * det, -1.0,
                A.stream_ptr()), "tike_farplane_scale"),
            adjoint=lambda: cg._fly_adjoint(op, far, p.probe, sc, p.psi, True,
                                            False),
            background=lambda: op.background_farplane_gradient(
                far, d, fly, states["background"].value,
                model=cm.model, measured=cm.mask, num_measured=cm.nmeasured,
                costs=costs, apply_gradient=True))
        fwd()
        for name, fn in legs.items():
            # (every leg on a far plane the forward has just written)
            out[f"leg_{name}_ms"] = timed(
                fn, NOTHING if name == "forward" else fwd, repeats)
        out["chunk_frames"] = nf
    torch.cuda.empty_cache()
    print(f"{det}^2 x {S} x {frames} frames x fly {fly}, k = {k}: gradient "
          f"evaluation {out['blur_gradient_ms']:.2f} ms with a blur, "
          f"{out['background_gradient_ms']:.2f} ms with a zero background; "
          f"line-search trial {out['blur_trial_ms']:.2f} / "
          f"{out['background_trial_ms']:.2f} ms; legs of a chunk of "
          f"{out['chunk_frames']} frames: "
          + ", ".join(f"{name} {out[f'leg_{name}_ms']:.2f}"
                      for name in ("forward", "intensities", "blur", "scale",
                                   "adjoint", "background")) + " ms")
    return out


def pitch(det, frames, num_batch=4, k=5):
    """An epoch with 1 mode and a blur against an epoch with 8 modes."""
    K = gaussian_kernel(k)
    out = dict(det=det, frames=frames, k=k, num_batch=num_batch)
    scan, psi, probe8, _ = _problem(det, 8, 4, 1)
    scan, psi, probe1, data = _problem(det, 1, frames, 1, blur=K)
    for name, probe, bo in (
            ("modes8", probe8, None),
            ("modes1", probe1, None),
            ("modes1_blur_fixed", probe1, tp.BlurOptions(K, update=False)),
            ("modes1_blur_fitted", probe1, tp.BlurOptions(K))):
        params = _parameters(scan, psi, probe, det, num_batch)
        with tp.Reconstruction(data, params, blur_options=bo) as ctx:
            ctx.iterate(1)  # warm-up: workspaces, tables
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.iterate(1)
            torch.cuda.synchronize()
            out[f"epoch_{name}_ms"] = (time.perf_counter() - t0) * 1e3
        torch.cuda.empty_cache()
    print(f"{det}^2 x {frames} frames, {num_batch} minibatches, 2 CG "
          f"iterations per block: cgrad epoch {out['epoch_modes8_ms']:.1f} ms "
          f"with 8 modes, {out['epoch_modes1_ms']:.1f} ms with 1 mode, "
          f"{out['epoch_modes1_blur_fixed_ms']:.1f} ms with 1 mode and a "
          f"fixed blur, {out['epoch_modes1_blur_fitted_ms']:.1f} ms with 1 "
          "mode and a fitted blur")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--no-pitch", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    result = dict(build_id=build_id(), device=torch.cuda.get_device_name(0),
                  kernels=[], gradients=[])
    for det in (256, 128):
        result["kernels"] += kernel_legs(det, args.frames, args.repeats)
        torch.cuda.empty_cache()
    if not args.kernel_only:
        for det, S, fly in ((256, 1, 1), (128, 4, 2)):
            result["gradients"].append(
                gradient_legs(det, S, args.frames, fly, args.repeats))
        if not args.no_pitch:
            result["pitch"] = pitch(256, args.frames)
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main()
