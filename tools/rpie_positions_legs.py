"""The rpie workloads of bench.py (c3rpie: 10 000 positions, 256^2, 8 modes +
eigen weights, 10 minibatches; c3rpie2: the same on a two-slice object) with
and without position correction.  Prints k patterns/s per leg; under
`rocprofv3 --kernel-trace --stats` the kernel table of the run shows
`rpie_position_sums_kernel` next to the gradient pass and the scatter.

    python tools/rpie_positions_legs.py [--only with|without] [workload ...]
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def leg(workload, positions, torch, tp, A, bench, epochs=3):
    built = bench.epoch_problem(workload, 0, 1, 0, tp, A)
    ctx = built["ctx"]
    try:
        if positions:
            # (shifts clipped to 0.05 px: the cost of the correction does not
            # depend on how far the positions move, and the bench's scan has
            # little room around it)
            scan = A.to_host(ctx.parameters.scan)
            ctx.parameters.position_options = tp.PositionOptions(
                scan.copy(), update_magnitude_limit=0.05).copy_to_device()
        ctx.iterate(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.iterate(epochs)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        ctx.__exit__(None, None, None)
    return built["N"] * epochs / dt


def main(argv):
    import torch
    import bench
    import tike_amd._arrays as A
    import tike_amd.ptycho as tp
    only = None
    if argv[:1] == ["--only"]:
        only, argv = argv[1], argv[2:]
    for w in argv or ("c3rpie", "c3rpie2"):
        row = []
        for label, positions in (("without", False), ("with", True)):
            if only in (None, label):
                rate = leg(w, positions, torch, tp, A, bench)
                row.append(f"{label} position correction: {rate / 1e3:.1f}")
                torch.cuda.empty_cache()
        print(f"{w}: " + " | ".join(row) + "  (k patterns/s)", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
