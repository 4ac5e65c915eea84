"""What position correction costs cgrad, at the shapes of BASELINE configs[0]
(c1: 256 positions, 128^2, 1 mode, one minibatch) and configs[1] (c2: 10 000
positions, 256^2, 1 mode), cg_iter = 4:

  * patterns/s of whole epochs with and without `position_options`, object
    and probe recovered, and with the object not recovered (where the sums
    cost one extra gradient pass per minibatch);
  * the time of one chunk through `tike_lstsq_chunk_gradients_positions` with
    the sums (numerator / denominator given) next to the same call without
    them (both NULL: the gradient pass alone).

    python tools/cgrad_positions_legs.py [c1|c2|both] [positions of c2]

The problems carry 12 px of object around the scan so that corrected
positions stay inside it (bench.py's generator starts at pixel 1).
(test infrastructure: imports tests/, like tools/fuzz_vs_oracle.py)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tike_amd._arrays as A  # noqa: E402
import tike_amd.ptycho as tp  # noqa: E402
import tike_amd.random  # noqa: E402
from rpie_positions import jitter, smooth_object  # noqa: E402
from tike_amd._lib import check, lib  # noqa: E402
from tike_amd.operators.propagation import fft_scales  # noqa: E402
from tike_amd.ptycho.position import gaussian_derivative_taps  # noqa: E402
from tike_amd.ptycho.solvers.lstsq import chunk_positions  # noqa: E402

SHAPES = {"c1": (128, 1, 256, 1, 20, 10), "c2": (256, 1, 10000, 10, 3, 2)}
"""workload: detector, modes, positions, minibatches, timed / warm-up epochs"""


def problem(det, S, N, seed=1234):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(N)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side),
                              indexing="ij"), -1).reshape(-1, 2)[:N]
    true = (12 + 8.0 * ij + rng.random((N, 2))).astype(np.float32)
    rng.shuffle(true, axis=0)
    HW = 8 * (side - 1) + det + 26
    psi = smooth_object(rng, 1, HW)
    w = tp.gaussian(det, rin=0.6)
    probe = np.stack([w * np.exp(1j * np.pi * rng.random((det, det))) / (m + 1)
                      for m in range(S)])[None, None].astype(np.complex64)
    data = tp.simulate(det, probe, true, psi).astype(np.float32)
    scan0 = (true + jitter(rng, true.shape, 0.5)).astype(np.float32)
    return scan0, psi, probe, data


def epochs(workload, scan0, psi, probe, data, *, positions, recover_psi):
    det, S, N, num_batch, timed, warm = SHAPES[workload]
    N = len(scan0)
    params = tp.PtychoParameters(
        probe=probe.copy(), psi=(0.8 * psi + 0.1).astype(np.complex64),
        scan=scan0.copy(),
        algorithm_options=tp.CgradOptions(num_batch=num_batch, cg_iter=4),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions() if recover_psi else None,
        position_options=tp.PositionOptions(
            scan0.copy(), use_adaptive_moment=True,
            update_magnitude_limit=0.25) if positions else None)
    tike_amd.random.randomizer_np = np.random.default_rng(4321)
    with tp.Reconstruction(A.to_device(data, np.float32), params,
                           presharded=True, order=np.arange(N),
                           batches=np.array_split(np.arange(N),
                                                  num_batch)) as ctx:
        ctx.iterate(warm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.iterate(timed)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return N * timed / dt


def chunk_times(workload, scan0, psi, probe, data, repeats=20):
    """ms of one chunk: gradient pass alone, gradient pass + sums."""
    det, S = SHAPES[workload][:2]
    n = min(len(scan0), chunk_positions(S, det, det in (256, 512)))
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W = psi.shape[-2:]
    t = dict(psi=A.to_device(psi), scan=A.to_device(scan0[:n]),
             probe=A.to_device(probe), data=A.to_device(data[:n], np.float32))
    c64 = lambda *s: torch.empty(*s, dtype=torch.complex64, device=dev)
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    far, mid = c64(n, 1, S, det, det), c64(n, 1, S, det, det)
    gscale, patches, objproj = f32(2 * n, det, det), c64(n, det, det), c64(
        n, det, det)
    costs, inten = f32(n), f32(det, det)
    acc = torch.zeros(2, H, W, device=dev)
    num, den = f32(n, 2), f32(n, 2)
    taps, r = gaussian_derivative_taps(0.333)
    fwd_scale, inv_scale = fft_scales(det, "ortho")
    args = (A.ptr(t["psi"]), A.ptr(t["scan"]), A.ptr(t["probe"]), None, None,
            0, 0, A.ptr(t["data"]), 0, None, 0, 1.0, det * det, A.ptr(far),
            A.ptr(mid), A.ptr(gscale), A.ptr(patches), A.ptr(costs),
            A.ptr(objproj), None, None, 1.0, A.ptr(acc), n, S, det, H, W,
            fwd_scale, inv_scale, taps.ctypes.data, r, A.ptr(inten))
    out = {}
    for name, sums in (("gradient pass", (None, None)),
                       ("gradient pass + sums", (A.ptr(num), A.ptr(den)))):
        best = np.inf
        for _ in range(repeats):
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            check(lib.tike_lstsq_chunk_gradients_positions(
                *args, *sums, A.stream_ptr()), name)
            b.record()
            b.synchronize()
            best = min(best, a.elapsed_time(b))
        out[name] = best
    return n, out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    for workload in (("c1", "c2") if which == "both" else (which,)):
        det, S, N = SHAPES[workload][:3]
        if workload == "c2" and len(sys.argv) > 2:
            N = int(sys.argv[2])
        built = problem(det, S, N)
        result = dict(workload=workload, positions=N)
        for recover_psi in (True, False):
            for positions in (False, True):
                key = (("object + probe" if recover_psi else "probe only") +
                       (", positions" if positions else ""))
                result[key + " [patterns/s]"] = round(
                    epochs(workload, *built, positions=positions,
                           recover_psi=recover_psi), 1)
        n, times = chunk_times(workload, *built)
        result["chunk positions"] = n
        for name, ms in times.items():
            result[name + " [ms]"] = round(ms, 4)
        print("LEGS " + json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
