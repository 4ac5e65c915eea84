#!/usr/bin/env python3
"""Legs of a near-field reconstruction on the GPU (not a test, not part of
bench.py):

    python tools/nearfield_legs.py [--repeats 10] [--gib 8] [--frames 4000]
                                   [--kernel-only]

With device events (warm-up first, median of the repeats) it times
  * `tike_nearfield_plane_gradient` against the three launches it replaces --
    `tike_fft2_pass2_inplace` + `tike_fly_farplane_gradient` +
    `tike_fft2_pass1` -- on the same planes in the same run, alternating, at
    256^2 x 8 modes and 128^2 x 4 modes x fly 2 (about `--gib` GiB of planes),
    with `out` and cost-only: times, their ratio, and the entry's rate on its
    own byte model (P planes x 8 B read, twice past 3 planes, and written,
    counts 4 B, mask 1 B) as a fraction of the 8 TB/s HBM peak;
  * every launch of one near-field gradient evaluation of cgrad on a chunk
    (pass 1, column passes, entry, adjoint column passes, products, scatter);
  * one cgrad epoch with `nearfield_options` against the far-field epoch of
    the same shape, at 256^2 x 1 mode and 128^2 x 4 modes.
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
from tike_amd.operators import nearfield as NF  # noqa: E402

from fly_legs import HBM_PEAK, timed  # noqa: E402

NOTHING = lambda: None  # noqa: E731


def propagator(det, nyquist_pi=3.0):
    f = np.fft.fftfreq(det)
    q = (f[:, None]**2 + f[None, :]**2) / 0.25
    return np.exp(-0.5j * np.pi * nyquist_pi * q).astype(np.complex64)


def kernel_legs(det, S, fly, gib, repeats):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(det + S)
    P = S * fly
    frames = max(1, int(gib * 2**30) // (P * det * det * 8))
    N = frames * fly
    work0 = torch.view_as_complex(
        torch.randn((N, S, det, det, 2), generator=gen, device=dev))
    work = work0.clone()
    out = torch.empty_like(work0)
    data = torch.poisson(torch.full((frames, det, det), 2.0 * P * det * det,
                                    device=dev), generator=gen)
    mask = torch.ones((det, det), dtype=torch.uint8, device=dev)
    mask[det // 2 - 1:det // 2 + 1] = 0
    nm = int(mask.sum())
    costs = torch.empty(frames, dtype=torch.float32, device=dev)
    unit = torch.full((frames,), float(nm), dtype=torch.float32, device=dev)
    st = A.stream_ptr()

    def entry(grad):
        NF.plane_gradient(work0, data, fly, model=0, measured=mask,
                          num_measured=nm, upstream=unit, costs=costs,
                          out=out if grad else None, scale=-1.0)

    def three(grad):
        check(lib.tike_fft2_pass2_inplace(A.ptr(work), N * S, det, 1, 1.0, st),
              "pass 2")
        check(lib.tike_fly_farplane_gradient(
            A.ptr(work), A.ptr(data), 0, A.ptr(mask), None, A.ptr(costs),
            frames, fly, S, det, 0, int(grad), 1.0, nm, st), "fly gradient")
        if grad:
            check(lib.tike_fft2_pass1(A.ptr(work), A.ptr(out), N * S, det, 0,
                                      st), "pass 1")

    reset = lambda: work.copy_(work0)  # noqa: E731
    row = dict(det=det, S=S, fly=fly, frames=frames,
               plane_gib=N * S * det * det * 8 / 2**30)
    # alternate the two sides: same run, same planes
    t = {k: [] for k in ("entry", "three", "entry_cost", "three_cost")}
    for _ in range(3):
        t["entry"].append(timed(lambda: entry(True), NOTHING, repeats))
        t["three"].append(timed(lambda: three(True), reset, repeats))
        t["entry_cost"].append(timed(lambda: entry(False), NOTHING, repeats))
        t["three_cost"].append(timed(lambda: three(False), reset, repeats))
    # (the reset of the in-place side runs in front of the timed window)
    med = {k: float(np.median(v)) for k, v in t.items()}
    plane = N * S * det * det * 8
    reads = 2 if P > 3 else 1
    side = frames * det * det * (4 + 1)
    model = plane * (reads + 1) + side
    model_cost = plane + side
    row.update(
        entry_ms=med["entry"], three_launches_ms=med["three"],
        ratio=med["three"] / med["entry"], entry_cost_only_ms=med["entry_cost"],
        three_launches_cost_only_ms=med["three_cost"],
        ratio_cost_only=med["three_cost"] / med["entry_cost"],
        spread_entry_ms=[min(t["entry"]), max(t["entry"])],
        spread_three_ms=[min(t["three"]), max(t["three"])],
        model_bytes=model,
        fraction_of_8TBps=model / (med["entry"] * 1e-3) / HBM_PEAK,
        cost_only_fraction_of_8TBps=model_cost / (med["entry_cost"] * 1e-3)
        / HBM_PEAK)
    print(f"{det}^2 x {S} modes x fly {fly}, {frames} frames "
          f"({row['plane_gib']:.2f} GiB of planes): entry {med['entry']:.3f} ms"
          f" against {med['three']:.3f} ms of three launches (x"
          f"{row['ratio']:.2f}; {row['fraction_of_8TBps']:.3f} of 8 TB/s on "
          f"{reads + 1} crossings); cost only {med['entry_cost']:.3f} ms "
          f"against {med['three_cost']:.3f} ms (x{row['ratio_cost_only']:.2f}; "
          f"{row['cost_only_fraction_of_8TBps']:.3f} of 8 TB/s)")
    return row


def problem(det, S, frames, fly=1, seed=0):
    rng = np.random.default_rng(seed)
    N = frames * fly
    side = int(np.ceil(np.sqrt(N)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:N]
    scan = (2 + 4.0 * ij + rng.random((N, 2))).astype(np.float32)
    extent = int(scan.max()) + det + 4
    psi = np.exp(0.3j * rng.random((1, extent, extent))).astype(np.complex64)
    probe = np.stack([
        np.exp(2j * np.pi * rng.random((det, det))) / (m + 1)
        for m in range(S)])[None, None].astype(np.complex64)
    return psi, probe, scan


def gradient_legs(det, S, fly, frames, repeats):
    """Every launch of one gradient evaluation of the fused route on a chunk."""
    import tike_amd.operators as tops
    from tike_amd.operators.propagation import fft_scales
    dev = torch.device("cuda")
    psi_h, probe_h, scan_h = problem(det, S, frames, fly)
    psi, probe, scan = (torch.from_numpy(x).to(dev)
                        for x in (psi_h, probe_h, scan_h))
    H = torch.from_numpy(propagator(det)).to(dev)
    n, (Hh, W) = scan.shape[0], psi.shape[-2:]
    a = torch.empty((n, S, det, det), dtype=torch.complex64, device=dev)
    b = torch.empty_like(a)
    data = torch.ones((frames, det, det), dtype=torch.float32, device=dev)
    costs = torch.empty(frames, dtype=torch.float32, device=dev)
    unit = torch.full((frames,), float(det * det), device=dev)
    objproj = torch.empty((n, det, det), dtype=torch.complex64, device=dev)
    acc = torch.zeros((2, Hh, W), dtype=torch.float32, device=dev)
    pacc = torch.zeros((S, det, det), dtype=torch.complex64, device=dev)
    st = A.stream_ptr()
    fs_, is_ = fft_scales(det, "ortho")
    legs = [
        ("tike_fwd_pass1", lambda: check(lib.tike_fwd_pass1(
            A.ptr(psi[0]), A.ptr(scan), A.ptr(probe), 0, None, None, None, 0,
            0, A.ptr(a), None, n, S, det, det, Hh, W, st), "pass 1")),
        ("tike_fresnel_colpass(H)", lambda: check(lib.tike_fresnel_colpass(
            A.ptr(a), A.ptr(H), 0, A.ptr(b), n * S, det, fs_ * is_, st), "c")),
        ("tike_nearfield_plane_gradient", lambda: NF.plane_gradient(
            b, data, fly, upstream=unit, costs=costs, out=a, scale=-1.0)),
        ("tike_nearfield_plane_gradient (cost only)",
         lambda: NF.plane_gradient(b, data, fly, upstream=unit, costs=costs)),
        ("tike_fresnel_colpass(conj H)", lambda: check(
            lib.tike_fresnel_colpass(A.ptr(a), A.ptr(H), 1, A.ptr(b), n * S,
                                     det, fs_, st), "c")),
        ("tike_ifft2_pass2_products", lambda: check(
            lib.tike_ifft2_pass2_products(
                A.ptr(b), A.ptr(psi[0]), A.ptr(scan), A.ptr(probe), 0,
                A.ptr(objproj), A.ptr(pacc), 1.0, None, 0, n, S, det, Hh, W,
                is_, st), "products")),
        ("tike_scatter_patches", lambda: check(lib.tike_scatter_patches(
            A.ptr(objproj), A.ptr(scan), A.ptr(acc), n, det, Hh, W, st), "s")),
    ]
    rows = []
    for name, fn in legs:
        ms = timed(fn, NOTHING, repeats)
        rows.append(dict(det=det, S=S, fly=fly, frames=frames, leg=name, ms=ms))
        print(f"{det}^2 x {S} modes x fly {fly}, {frames} frames: {name} "
              f"{ms:.3f} ms")
    with tops.Ptycho(det, det, nz=Hh, n=W) as op:
        far = torch.empty((n, 1, S, det, det), dtype=torch.complex64,
                          device=dev)
        ms = timed(lambda: op.fwd_device(probe, scan, psi, out=far), NOTHING,
                   repeats)
        print(f"{det}^2 x {S} modes: the far-field forward operator "
              f"{ms:.3f} ms")
        rows.append(dict(det=det, S=S, fly=fly, frames=frames,
                         leg="tike_ptycho_fwd (far field)", ms=ms))
    return rows


def epoch_legs(det, S, frames, epochs=2):
    """Wall time of a cgrad epoch in the near field against the far-field one
    of the same shape (the second of two epochs: the first warms up)."""
    psi, probe, scan = problem(det, S, frames)
    H = propagator(det)
    data = tp.simulate(det, probe, scan, psi, nearfield=H)
    out = {}
    for name, options in (("far", None), ("near", tp.NearFieldOptions(H))):
        params = tp.PtychoParameters(
            probe=probe.copy(), psi=np.ones_like(psi), scan=scan.copy(),
            algorithm_options=tp.CgradOptions(num_batch=1, cg_iter=2,
                                              num_iter=1),
            probe_options=None, object_options=tp.ObjectOptions(),
            exitwave_options=tp.ExitWaveOptions(
                measured_pixels=np.ones((det, det), bool)))
        with tp.Reconstruction(data, params,
                               nearfield_options=options) as ctx:
            times = []
            for _ in range(epochs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.iterate(1)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
        out[name] = times[-1]
    print(f"{det}^2 x {S} modes, {frames} frames: cgrad epoch near field "
          f"{out['near']:.3f} s, far field {out['far']:.3f} s "
          f"(x{out['near'] / out['far']:.2f})")
    return dict(det=det, S=S, frames=frames, near_epoch_s=out["near"],
                far_epoch_s=out["far"], ratio=out["near"] / out["far"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    A.current_device()
    rows = dict(kernel=[], gradient=[], epoch=[])
    for det, S, fly in ((256, 8, 1), (128, 4, 2), (256, 1, 1), (256, 3, 1)):
        rows["kernel"].append(kernel_legs(det, S, fly, a.gib, a.repeats))
    if not a.kernel_only:
        for det, S, fly in ((256, 1, 1), (128, 4, 1)):
            rows["gradient"] += gradient_legs(det, S, fly,
                                              min(a.frames, 4000), a.repeats)
        for det, S in ((256, 1), (128, 4)):
            rows["epoch"].append(epoch_legs(det, S, a.frames))
    print(json.dumps(dict(build_id=build_id(), **rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
