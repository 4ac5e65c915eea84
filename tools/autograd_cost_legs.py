#!/usr/bin/env python3
"""Legs of the differentiable noise-model cost on the GPU (not a test, not
part of bench.py):

    python tools/autograd_cost_legs.py [--repeats 10] [--frames 4000]
                                       [--entries-once]

At 256^2 x 1 mode and 128^2 x 4 modes, `frames` frames of `fly` = 1 and 4
positions each, and at 256^2 x 8 modes + one eigen probe (fly 1), with Poisson
counts and a module-gap mask, it times with device events (2 warm-up calls
each; the two variants of a pair ALTERNATE inside the timed loop; median and
min ... max of the repeats), all in one process
  (a) `tike_amd.autograd.cost` forward + backward with every gradient against
      the composition it replaces -- `intensity`, the loss in torch, torch's
      backward -- with `torch.cuda.max_memory_allocated` of one call of each;
  (b) `cost_gauss_newton_product` (every tangent, every part) against
      `*_gauss_newton_product(weight=W)` including the formation of W from
      `intensity` in torch;
  (c) the two new entries against their closest existing ones on the same
      planes: `tike_cost_curvature` (table alone, as the product calls it, and
      with costs and dcosts, as `cost_jvp` does) against
      `tike_intensity_tangent` (I and dI), and `tike_cost_factor` (table
      alone, costs alone) against `tike_fly_farplane_gradient(apply_gradient
      =0)` writing costs and intensity -- each as a share of the 8 TB/s
      roofline on the bytes its contract implies.
`--entries-once` runs the launches of (c) exactly once after one warm-up
launch each, for a `rocprofv3 --kernel-trace --stats` run of its own.  One
line per shape, then one JSON line with the library's build id."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tike_amd.operators as ops  # noqa: E402
from autograd_legs import HBM_PEAK, problem  # noqa: E402
from tike_amd import _arrays as A  # noqa: E402
from tike_amd import autograd  # noqa: E402
from tike_amd._lib import build_id, check, lib  # noqa: E402

CURVATURE = {"gaussian": 0.5, "poisson": 1.0}
MODEL = "poisson"


def alternate(fns, repeats, warm=2):
    """[(median, min, max) ms per function]: after `warm` calls of each, the
    functions take turns inside the timed loop, one device-event pair per
    call."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ms[k].append(start.elapsed_time(stop))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def peak_of(fn):
    """torch.cuda.max_memory_allocated over one call, above what is resident
    before it (bytes)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def torch_loss(inten, data, mask, nm):
    """The per-frame poisson cost in torch: the mask by torch.where on the
    counts and on the terms, the guard of the project."""
    zero = torch.zeros_like(inten)
    d = torch.where(mask, data, zero)
    terms = torch.where(mask, inten - d * torch.log(inten + 1e-9), zero)
    return terms.sum(dim=(1, 2)) / nm


def gap_mask(det, dev):
    mask = torch.ones((det, det), dtype=torch.bool, device=dev)
    mask[det // 2 - det // 16:det // 2] = False
    return mask


def legs(det, S, frames, fly, repeats, warm, eigen, entries_once):
    dev = torch.device("cuda")
    psi_h, probe_h, scan_h = problem(det, S, frames, fly)
    N = frames * fly
    H, W = psi_h.shape[-2:]
    row = dict(det=det, modes=S, frames=frames, fly=fly, positions=N,
               eigen=int(eigen))
    leaves = dict(zip(("psi", "probe", "scan"),
                      (torch.from_numpy(x).to(dev).requires_grad_(True)
                       for x in (psi_h, probe_h, scan_h))))
    gen = torch.Generator(device=dev).manual_seed(det + S + fly)
    rc = lambda x: torch.view_as_complex(torch.randn(
        tuple(x.shape) + (2,), generator=gen, device=dev))
    extra = {}
    if eigen:
        extra["eigen_probe"] = (0.1 * rc(leaves["probe"][:, :, :1])
                                ).requires_grad_(True)
        w = torch.zeros((N, 2, S), device=dev)
        w[:, 0] = 1 + 0.05 * torch.randn((N, S), generator=gen, device=dev)
        w[:, 1] = 0.3 * torch.randn((N, S), generator=gen, device=dev)
        extra["eigen_weights"] = w.requires_grad_(True)
    leaves.update(extra)
    tangents = {"d_" + k: (rc(v) if v.is_complex() else torch.randn(
        v.shape, generator=gen, device=dev)) for k, v in leaves.items()}
    names = tuple(leaves)
    mask = gap_mask(det, dev)
    nm = int(mask.sum())
    up = 0.5 + torch.rand(frames, generator=gen, device=dev)
    with ops.Ptycho(probe_shape=det, detector_shape=det, nz=H, n=W) as op:
        args = (leaves["psi"], leaves["probe"], leaves["scan"])
        with torch.no_grad():
            clean = autograd.intensity(op, *args, fly=fly, **extra)
            data = torch.poisson(200.0 * clean / clean.mean()) * (
                clean.mean() / 200.0)
            data = torch.where(mask, data, torch.full_like(data, float("nan")))
            del clean
        common = dict(fly=fly, check_positions=False, **extra)

        def zero_grads():
            for x in leaves.values():
                x.grad = None

        def cost_both():
            zero_grads()
            (autograd.cost(op, data, *args, model=MODEL, measured_pixels=mask,
                           **common) * up).sum().backward()

        def composition_both():
            zero_grads()
            inten = autograd.intensity(op, *args, **common)
            (torch_loss(inten, data, mask, nm) * up).sum().backward()

        def product():
            autograd.cost_gauss_newton_product(
                op, data, *args, model=MODEL, measured_pixels=mask,
                upstream=up, wrt=names, **common, **tangents)

        composed = (autograd.eigen_gauss_newton_product if eigen else
                    autograd.gauss_newton_product)

        def composition_product():
            with torch.no_grad():
                inten = autograd.intensity(op, *args, **common)
                weight = torch.where(
                    mask, up[:, None, None] * CURVATURE[MODEL]
                    / (nm * (inten + 1e-9)), torch.zeros_like(inten))
                del inten
            composed(op, *args, weight=weight, wrt=names, **common,
                     **tangents)

        if not entries_once:
            (a, b), (c, d) = (alternate([cost_both, composition_both],
                                        repeats, warm),
                              alternate([product, composition_product],
                                        repeats, warm))
            for key, t in (("cost_fwd_bwd", a), ("composition_fwd_bwd", b),
                           ("cost_gn_product", c), ("composition_gn_product",
                                                    d)):
                row[key + "_ms"], row[key + "_min_ms"], row[key + "_max_ms"] = t
            for key, fn in (("cost_fwd_bwd", cost_both),
                            ("composition_fwd_bwd", composition_both),
                            ("cost_gn_product", product),
                            ("composition_gn_product", composition_product)):
                row[key + "_peak_bytes"] = peak_of(fn)
            zero_grads()
        # (c) the entries alone on one chunk of planes of the same shape
        st = A.stream_ptr()
        nf = min(frames, max(1, (1 << 31) // (S * fly * det * det * 8)))
        n, P, npix = nf * fly, S * fly, det * det
        far = torch.empty((n, 1, S, det, det), dtype=torch.complex64,
                          device=dev)
        with torch.no_grad():
            w = extra.get("eigen_weights")
            op.fwd_device(leaves["probe"].detach(), leaves["scan"][:n].detach(),
                          leaves["psi"].detach(),
                          *((extra["eigen_probe"].detach(), w[:n].detach())
                            if eigen else ()), out=far)
        dfar = torch.view_as_complex(torch.randn(
            tuple(far.shape) + (2,), generator=gen, device=dev))
        m8 = mask.to(torch.uint8).contiguous()
        d = data[:nf].contiguous()
        table = torch.empty((nf, det, det), dtype=torch.float32, device=dev)
        inten = torch.empty_like(table)
        costs = torch.empty(nf, dtype=torch.float32, device=dev)
        dcosts = torch.empty_like(costs)
        u = up[:nf].contiguous()

        def curvature(sums, tab=True):
            check(lib.tike_cost_curvature(
                A.ptr(far), A.ptr(dfar), A.ptr(d) if sums else None, 0,
                A.ptr(m8), A.ptr(u), A.ptr(costs) if sums else None,
                A.ptr(dcosts) if sums else None, A.ptr(table) if tab else None,
                nf, P, npix, 1, 1e-9, nm, st), "tike_cost_curvature")

        def factor(with_costs, tab):
            check(lib.tike_cost_factor(
                A.ptr(far), A.ptr(d), 0, A.ptr(m8), A.ptr(u),
                A.ptr(costs) if with_costs else None,
                A.ptr(table) if tab else None, nf, P, npix, 1, nm, st),
                "tike_cost_factor")

        entries = dict(
            cost_curvature_table=lambda: curvature(False),
            cost_curvature_sums=lambda: curvature(True, False),
            intensity_tangent=lambda: check(lib.tike_intensity_tangent(
                A.ptr(far), A.ptr(dfar), A.ptr(inten), A.ptr(table), nf, P,
                npix, st), "tike_intensity_tangent"),
            cost_factor_table=lambda: factor(False, True),
            cost_factor_costs=lambda: factor(True, False),
            fly_farplane_gradient=lambda: check(
                lib.tike_fly_farplane_gradient(
                    A.ptr(far), A.ptr(d), 0, A.ptr(m8), A.ptr(inten),
                    A.ptr(costs), nf, P, 1, det, 1, 0, 1.0, nm, st),
                "tike_fly_farplane_gradient"))
        times = alternate(list(entries.values()), 1 if entries_once else
                          repeats, 1 if entries_once else warm)
        plane, frame = n * S * npix * 8, nf * npix
        model_bytes = dict(
            cost_curvature_table=2 * plane + frame * (1 + 4),
            cost_curvature_sums=2 * plane + frame * (4 + 1),
            intensity_tangent=2 * plane + frame * 8,
            cost_factor_table=plane + frame * (4 + 1 + 4),
            cost_factor_costs=plane + frame * (4 + 1),
            fly_farplane_gradient=plane + frame * (4 + 1 + 4))
        row["entry_frames"] = nf
        for key, t in zip(entries, times):
            row[key + "_ms"], row[key + "_min_ms"], row[key + "_max_ms"] = t
            row[key + "_model_bytes"] = model_bytes[key]
            row[key + "_share_of_8TBps"] = model_bytes[key] / (t[0] * 1e-3) \
                / HBM_PEAK
        del far, dfar
    torch.cuda.empty_cache()
    f = lambda k: (f"{row[k + '_ms']:.2f} ms ({row[k + '_min_ms']:.2f} ... "
                   f"{row[k + '_max_ms']:.2f})")
    gib = lambda k: f"{row[k + '_peak_bytes'] / 2**30:.2f} GiB"
    head = (f"{det}^2 x {S}{' + eigen' if eigen else ''} x {frames} frames x "
            f"fly {fly}: ")
    if not entries_once:
        head += (f"cost fwd+bwd {f('cost_fwd_bwd')} peak "
                 f"{gib('cost_fwd_bwd')}, composition "
                 f"{f('composition_fwd_bwd')} peak "
                 f"{gib('composition_fwd_bwd')}; cost_gauss_newton_product "
                 f"{f('cost_gn_product')} peak {gib('cost_gn_product')}, "
                 f"composition {f('composition_gn_product')} peak "
                 f"{gib('composition_gn_product')}; ")
    print(head + f"entries on {nf} frames: " + ", ".join(
        f"{k} {row[k + '_ms']:.3f} ms ({row[k + '_share_of_8TBps']:.2f} of "
        "8 TB/s)" for k in entries), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--entries-once", action="store_true")
    args = ap.parse_args()
    A.require_gpu()
    np.random.seed(0)
    rows = []
    for det, S, eigen in ((256, 1, False), (128, 4, False), (256, 8, True)):
        for fly in ((1,) if eigen else (1, 4)):
            rows.append(legs(det, S, args.frames, fly, args.repeats, 2, eigen,
                             args.entries_once))
    print("RESULT " + json.dumps(dict(
        build_id=build_id(), device=torch.cuda.get_device_name(0), rows=rows)))


if __name__ == "__main__":
    main()
