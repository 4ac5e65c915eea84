"""The GPU work of tests/test_dm_gpu.py in a process of its own:

    _dm_child.py SECTION OUT

runs one of the sections `entries`, `routes`, `solver`, `resume` on cuda:0
and writes every figure the tests set a bar on, and every exact comparison as
a bool, to OUT (.json); `ranks` (see there) writes one rank's result.  The
float64 model is tests/dm_model.py."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dm_model as dm  # noqa: E402
from util import relerr  # noqa: E402

from tike_amd import _arrays as A  # noqa: E402
from tike_amd._lib import ERR_ARG, lib  # noqa: E402

DEV = torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(a, b):
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return bool(torch.equal(a, b))


def rc(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(
        np.complex64)


def c128(x):
    return x.cpu().numpy().astype(np.complex128)


# ------------------------------------------------------------------ entries
ENTRY_SHAPES = {"padded": (64, 48, 3, 5), "plain": (32, 32, 1, 5),
                "odd": (45, 35, 2, 5)}


def entry_positions(H, pw):
    """The smallest allowed position, the largest, a whole-pixel one and two
    with fractions."""
    last = float(H - pw - 1)
    return np.array([[1.0, 1.0], [last, last], [5.0, 7.0], [3.3, 9.7],
                     [8.25, 2.5]], np.float32)


def reflect(psi, scan, probe, waves, near, a, det):
    n, S, pw = scan.shape[0], probe.shape[0], probe.shape[-1]
    return lib.tike_dm_reflect(A.ptr(psi), A.ptr(scan), A.ptr(probe),
                               A.ptr(waves), A.ptr(near), a, n, S, pw, det,
                               psi.shape[0], psi.shape[1], A.stream_ptr())


def update(waves, chi, psi, scan, probe, a, change):
    n, S, pw = scan.shape[0], probe.shape[0], probe.shape[-1]
    return lib.tike_dm_update(A.ptr(waves), A.ptr(chi), A.ptr(psi),
                              A.ptr(scan), A.ptr(probe), a, A.ptr(change), n,
                              S, pw, chi.shape[-1], psi.shape[0],
                              psi.shape[1], A.stream_ptr())


def entries():
    out = {}
    for name, (det, pw, S, N) in ENTRY_SHAPES.items():
        rng = np.random.default_rng(det + S)
        H = pw + 21
        scan_h = entry_positions(H, pw)[:N]
        psi_h, probe_h = rc(rng, H, H), rc(rng, S, pw, pw)
        waves_h, chi_h = rc(rng, N, S, pw, pw), rc(rng, N, S, det, det)
        psi, probe, scan = t(psi_h), t(probe_h), t(scan_h)
        waves, chi = t(waves_h), t(chi_h)
        m = [x.astype(np.complex128) for x in (psi_h, probe_h, waves_h, chi_h)]
        window = np.zeros((det, det), bool)
        p = (det - pw) // 2
        window[p:p + pw, p:p + pw] = True
        # waves == NULL against waves = P O, the very products: the same bits
        null = torch.full((N, S, det, det), 7.0, dtype=torch.complex64,
                          device=DEV)
        assert reflect(psi, scan, probe, None, null, 0.6, det) == 0
        po = null[..., p:p + pw, p:p + pw].contiguous()
        explicit = torch.full_like(null, 7.0)
        assert reflect(psi, scan, probe, po, explicit, 0.6, det) == 0
        res = {"null_equals_explicit": same(null, explicit),
               "null_err": relerr(c128(null), dm.reflect(m[0], scan_h, m[1],
                                                         None, 0.6, det)),
               "null_padding_zero": bool(
                   (null.cpu().numpy()[..., ~window] == 0).all())}
        for a in (1.0, 0.6):
            near = torch.full((N, S, det, det), 7.0, dtype=torch.complex64,
                              device=DEV)
            assert reflect(psi, scan, probe, waves, near, a, det) == 0
            again = torch.full_like(near, 3.0)
            assert reflect(psi, scan, probe, waves, again, a, det) == 0
            got = near.cpu().numpy()
            want = dm.reflect(m[0], scan_h, m[1], m[2], a, det)
            new = waves.clone()
            change = torch.full((N,), -1.0, dtype=torch.float64, device=DEV)
            assert update(new, chi, psi, scan, probe, a, change) == 0
            plain = waves.clone()
            assert update(plain, chi, psi, scan, probe, a, None) == 0
            want_new, want_change = dm.update(m[2], m[3], m[0], scan_h, m[1],
                                              a)
            res[f"a={a}"] = {
                "reflect_err": relerr(got.astype(np.complex128), want),
                "reflect_worst": max(relerr(got[n].astype(np.complex128),
                                            want[n]) for n in range(N)),
                "padding_zero": bool((got[..., ~window] == 0).all()),
                "finite": bool(np.isfinite(got).all()),
                "reflect_repeats": same(near, again),
                "inputs_kept": same(waves, t(waves_h)) and same(chi, t(chi_h))
                and same(psi, t(psi_h)) and same(probe, t(probe_h)),
                "update_err": relerr(c128(new), want_new),
                "update_worst": max(relerr(c128(new[n]), want_new[n])
                                    for n in range(N)),
                "change_err": float(np.max(np.abs(
                    change.cpu().numpy() - want_change) / want_change)),
                "change_grid_waves": relerr(c128(plain), c128(new)),
            }
        # bad arguments, and no positions: nothing is written
        near = torch.full((N, S, det, det), 7.0, dtype=torch.complex64,
                          device=DEV)
        ok = [A.ptr(psi), A.ptr(scan), A.ptr(probe), A.ptr(waves),
              A.ptr(near), 0.6, N, S, pw, det, H, H, A.stream_ptr()]
        bad = []
        for change in ({0: None}, {1: None}, {2: None}, {4: None},
                       {5: float("nan")}, {5: float("inf")}, {7: 0},
                       {8: det + 1}, {6: -1}):
            args = list(ok)
            for k, v in change.items():
                args[k] = v
            bad.append(lib.tike_dm_reflect(*args) == ERR_ARG)
        kept = waves.clone()
        ok2 = [A.ptr(kept), A.ptr(chi), A.ptr(psi), A.ptr(scan),
               A.ptr(probe), 0.6, None, N, S, pw, det, H, H, A.stream_ptr()]
        for change in ({0: None}, {1: None}, {2: None}, {3: None},
                       {4: None}, {5: float("nan")}, {8: 0}, {9: det + 1},
                       {7: -1}):
            args = list(ok2)
            for k, v in change.items():
                args[k] = v
            bad.append(lib.tike_dm_update(*args) == ERR_ARG)
        ok[6] = ok2[7] = 0
        res["bad_arguments"] = all(bad)
        res["no_positions"] = (lib.tike_dm_reflect(*ok) == 0
                               and lib.tike_dm_update(*ok2) == 0)
        torch.cuda.synchronize()
        res["nothing_written"] = bool((near == 7).all()) and same(kept, waves)
        out[name] = res
    return out


# ------------------------------------------------------------------- routes
ROUTE_SHAPES = {"256": (256, 2, 3), "512": (512, 1, 2)}


def routes():
    """One exit-wave step of the solver on both routes, from waves that are
    not P O, relaxation 0.6, float32 counts."""
    import tike_amd.operators as ops
    from tike_amd.ptycho.exitwave import ExitWaveOptions
    solver = importlib.import_module("tike_amd.ptycho.solvers.dm")
    out = {}
    for name, (det, S, N) in ROUTE_SHAPES.items():
        obj, probe, scan_h, data = dm.problem(det=det, pw=det, S=S,
                                              grid=(N, 1), step=7.0,
                                              seed=det, smooth=2)
        rng = np.random.default_rng(det)
        waves_h = (dm.products(obj, scan_h, probe)
                   * (1 + 0.3 * rng.standard_normal((N, S, det, det)))
                   ).astype(np.complex64)
        data = (1.2 * data).astype(np.float32)
        psi_h, probe_h = obj.astype(np.complex64), probe.astype(np.complex64)
        want, want_cost = dm.exit_wave_step(
            psi_h.astype(np.complex128), probe_h.astype(np.complex128),
            waves_h.astype(np.complex128), scan_h, data.astype(np.float64),
            relaxation=0.6)
        eo = ExitWaveOptions(measured_pixels=np.ones((det, det), bool))
        got = {}
        with ops.Ptycho(detector_shape=det, probe_shape=det, nz=obj.shape[0],
                        n=obj.shape[1]) as op:
            for fused in (True, False):
                solver.FUSED = fused
                assert solver.fused_route(op, S, det, t(data)) == fused
                waves = t(waves_h)
                costs = torch.zeros(N, dtype=torch.float32, device=DEV)
                solver.exit_wave_step(
                    op, t(data), t(psi_h)[None], t(scan_h), t(probe_h)[None,
                                                                       None],
                    waves, False, 0, N, costs, relaxation=0.6,
                    exitwave_options=eo)
                got[fused] = (c128(waves), costs.cpu().numpy().astype(
                    np.float64))
        solver.FUSED = True
        out[name] = {
            "routes_waves": relerr(got[True][0], got[False][0]),
            "routes_costs": relerr(got[True][1], got[False][1]),
            "fused_waves": relerr(got[True][0], want),
            "stored_waves": relerr(got[False][0], want),
            "fused_costs": float(np.max(np.abs(got[True][1] - want_cost)
                                        / want_cost)),
            "stored_costs": float(np.max(np.abs(got[False][1] - want_cost)
                                         / want_cost)),
            "step": relerr(want, waves_h.astype(np.complex128)),
        }
    return out


# ------------------------------------------------------------------- solver
def solver_problem():
    """det = pw = 64, two modes, 6 x 6 positions; a flat object and a blurred,
    dimmed probe to start from; counts scaled to peak at 60000 and rounded,
    so that float32 and uint16 carry the same values."""
    obj, probe, scan, data = dm.problem(det=64, pw=64, S=2, grid=(6, 6),
                                        step=5.0, seed=7, smooth=3)
    k = 60000.0 / data.max()
    counts = np.rint(k * data)
    probe = probe * np.sqrt(k)
    start = (0.8 * dm.binomial(dm.binomial(probe))).astype(np.complex64)
    flat = np.full_like(obj, np.abs(obj).mean()).astype(np.complex64)
    return flat, start, scan, counts


def gap_mask(det):
    """The gaps between the modules of a detector: a cross of dead rows and
    columns."""
    mask = np.ones((det, det), bool)
    mask[det // 2 - 2:det // 2 + 2, :] = False
    mask[:, det // 3:det // 3 + 3] = False
    return mask


def model_epochs(flat, start, scan, counts, epochs, mask=None, unmeasured=1.0,
                 batches=None):
    o, p = flat[0].astype(np.complex128), start.astype(np.complex128)
    w = dm.products(o, scan, p)
    costs = []
    for _ in range(epochs):
        o, p, w, c = dm.epoch(o, p, w, scan, counts, mask=mask,
                              unmeasured=unmeasured, batches=batches)
        costs.append(c)
    return o, p, np.array(costs)


def parameters(tp, psi, probe, scan, mask=None, unmeasured=1.0, num_batch=1,
               epochs=3):
    det = probe.shape[-1]
    return tp.PtychoParameters(
        probe=probe.copy(), psi=psi.copy(), scan=scan.copy(),
        algorithm_options=tp.DmOptions(num_batch=num_batch, num_iter=epochs),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=(mask if mask is not None else np.ones(
                (det, det), bool)), unmeasured_pixels_scaling=unmeasured))


def solver():
    import tike_amd.ptycho as tp
    flat, start, scan, counts = solver_problem()
    flat = flat[None]
    N, det = len(scan), 64
    mask = gap_mask(det)
    masked = counts.astype(np.float32)
    masked[:, ~mask] = np.nan

    def run(data, num_batch=1, **kw):
        batches = [np.asarray(b) for b in np.array_split(np.arange(N),
                                                         num_batch)]
        return tp.reconstruct(data, parameters(tp, flat, start[None, None],
                                               scan, num_batch=num_batch,
                                               **kw),
                              order=np.arange(N), batches=batches)

    def against(r, want):
        o, p, costs = want
        return {"psi": relerr(r.psi[0], o), "probe": relerr(r.probe[0, 0], p),
                "costs": float(np.max(np.abs(np.ravel(
                    r.algorithm_options.costs) - costs) / costs)),
                "epochs": len(r.algorithm_options.costs)}

    out = {}
    want = model_epochs(flat, start, scan, counts, 3)
    plain = run(counts.astype(np.float32))
    out["float32"] = against(plain, want)
    out["float32"]["moved"] = relerr(plain.probe[0, 0], start)
    out["uint16"] = against(run(counts.astype(np.uint16)), want)
    out["masked"] = against(
        run(masked, mask=mask, unmeasured=0.95),
        model_epochs(flat, start, scan, counts, 3, mask=mask,
                     unmeasured=0.95))
    three = run(counts.astype(np.float32), num_batch=3)
    out["three_batches"] = against(
        three, model_epochs(flat, start, scan, counts, 3,
                            batches=np.array_split(np.arange(N), 3)))
    out["three_vs_one"] = {
        "psi": relerr(three.psi, plain.psi),
        "probe": relerr(three.probe, plain.probe),
        "costs": float(np.max(np.abs(
            np.ravel(three.algorithm_options.costs)
            - np.ravel(plain.algorithm_options.costs))
            / np.ravel(plain.algorithm_options.costs)))}
    return out


def resume():
    """A second Reconstruction on a result starts again from waves = P O.
    The caller sets TIKE_DETERMINISTIC=1: the overlap sums are float atomics
    otherwise, and two runs of the same epoch differ in their last bits."""
    import copy

    import tike_amd.ptycho as tp
    from tike_amd._lib import DETERMINISTIC
    flat, start, scan, counts = solver_problem()
    N = len(scan)
    data = counts.astype(np.float32)
    kw = dict(order=np.arange(N), batches=[np.arange(N)])
    with tp.Reconstruction(data, parameters(tp, flat[None], start[None, None],
                                            scan), **kw) as ctx:
        ctx.iterate(2)
        # (the options object of a result is the context's own)
        two = copy.deepcopy(ctx.get_result())
        ctx.iterate(1)
        kept = ctx.get_result()
    with tp.Reconstruction(data, two, **kw) as ctx:
        ctx.iterate(1)
        resumed = ctx.get_result()
    with tp.Reconstruction(data, parameters(tp, two.psi, two.probe, scan),
                           **kw) as ctx:
        ctx.iterate(1)
        fresh = ctx.get_result()
    return {
        "deterministic": bool(DETERMINISTIC),
        "psi_equals_fresh": bool(np.array_equal(resumed.psi, fresh.psi)),
        "probe_equals_fresh": bool(np.array_equal(resumed.probe,
                                                  fresh.probe)),
        "cost_equals_fresh": (resumed.algorithm_options.costs[-1]
                              == fresh.algorithm_options.costs[-1]),
        "differs_from_kept_waves": relerr(resumed.psi, kept.psi),
        "epochs_on_record": len(resumed.algorithm_options.costs)}


def ranks():
    """`_dm_child.py ranks OUT RANK WORLD STORE`: one rank of a gloo group of
    WORLD ranks on one GPU (WORLD > 1) runs three epochs of the solver's
    problem in two minibatches of 1 and 35 positions -- with two ranks the
    second rank's share of the first minibatch is empty."""
    import tike_amd.ptycho as tp
    rank, world, store = int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"file://{store}",
                                rank=rank, world_size=world)
    flat, start, scan, counts = solver_problem()
    N = len(scan)
    with tp.Reconstruction(
            counts.astype(np.float32),
            parameters(tp, flat[None], start[None, None], scan, num_batch=2),
            order=np.arange(N), batches=[np.arange(0, 1), np.arange(1, N)],
            spatial_sort=False) as ctx:
        shares = [len(b) for b in ctx.batches]
        ctx.iterate(3)
        r = ctx.get_result()
    if world > 1:
        dist.destroy_process_group()
    return {"shares": shares, "costs": np.ravel(
        r.algorithm_options.costs).tolist(),
        "psi": np.stack([r.psi.real, r.psi.imag]).tolist(),
        "probe": np.stack([r.probe.real, r.probe.imag]).tolist()}


if __name__ == "__main__":
    torch.cuda.set_device(0)
    result = {"entries": entries, "routes": routes, "solver": solver,
              "resume": resume, "ranks": ranks}[sys.argv[1]]()
    torch.cuda.synchronize()
    with open(sys.argv[2], "w") as f:
        json.dump(result, f, indent=1)
    if sys.argv[1] != "ranks":  # (its arrays go to the file only)
        print(json.dumps(result, indent=1))
