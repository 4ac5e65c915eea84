"""Fly scans on the GPU: `tike_fly_farplane_gradient` against the float64 model
(tests/fly_scan.py), the operator and `simulate` against the reference's
results (tests/golden/fly_scan.npz), cgrad on fly-scan data against the model's
cgrad, and the host plumbing (host-kept data, injected orders, two ranks)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fly_scan as fs
from util import OP_NORMWISE, assert_close, relerr

pytestmark = pytest.mark.gpu

RECON_NORMWISE = 1e-3  # the project's reconstruction bar


@pytest.fixture(scope="module")
def tp():
    import tike_amd.ptycho as m
    return m


@pytest.fixture(scope="module")
def fx(golden):
    return golden("fly_scan.npz")


# ------------------------------------------------------------------ the kernel
def _kernel_case(nframe, fly, S, det, seed=0):
    """Random far planes and integer counts (the same values as float32 and
    as uint16), and the float64 model's results for both noise models, with
    and without the mask -- computed once per case."""
    rng = np.random.default_rng(seed + det)
    N = nframe * fly
    far = (rng.standard_normal((N, 1, S, det, det))
           + 1j * rng.standard_normal((N, 1, S, det, det))).astype(np.complex64)
    counts = rng.poisson(2.0 * fly * S, (nframe, det, det)).astype(np.uint16)
    mask = fs.block_mask(det)
    want = {}
    inten = fs.frame_intensity(far, fly)
    for model in ("gaussian", "poisson"):
        for m in (None, mask):
            d = counts.astype(np.float64)
            want[model, m is not None] = (
                fs.cost_each(model, d, inten, m),
                fs.farplane_gradient(model, fs.masked(d, m) if m is not None
                                     else d, far, fly, m))
    return far, counts, mask, inten, want


def _call(torch, lib, far, data, mask, intensity, costs, nframe, fly, S, det,
          model, grad, ums, nmeasured):
    from tike_amd import _arrays as A
    from tike_amd._lib import check
    check(lib.tike_fly_farplane_gradient(
        A.ptr(far), A.ptr(data), int(data.dtype == torch.uint16), A.ptr(mask),
        A.ptr(intensity), A.ptr(costs), nframe, fly, S, det, model, int(grad),
        ums, nmeasured, A.stream_ptr()), "tike_fly_farplane_gradient")


KERNEL_CASES = [(3, 1, 1, 16), (2, 2, 1, 32), (3, 3, 2, 33), (2, 4, 8, 64),
                (1, 5, 3, 128)]


@pytest.mark.parametrize("nframe,fly,S,det", KERNEL_CASES)
def test_kernel_vs_float64_model(nframe, fly, S, det):
    """gaussian and Poisson, with and without the NaN mask, float32 and
    uint16 counts, costs only and with the gradient, intensity NULL and
    given; two calls give the same bits; a costs-only call leaves the far
    plane as it was."""
    import torch

    from tike_amd._lib import lib
    far_h, counts, mask_h, inten, want = _kernel_case(nframe, fly, S, det)
    dev = torch.device("cuda")
    far0 = torch.from_numpy(far_h).to(dev)
    mask_d = torch.from_numpy(mask_h.astype(np.uint8)).to(dev)
    f32 = counts.astype(np.float32)
    f32_nan = fs.masked(f32, mask_h)
    junk = counts.copy()
    junk[:, ~mask_h] = 65535  # uint16 has no NaN: counts that must not be read
    UMS = 0.75
    worst = dict(cost=0.0, grad=0.0, intensity=0.0)
    for model, name in enumerate(("gaussian", "poisson")):
        for masked in (False, True):
            mask = mask_d if masked else None
            nmeas = int(mask_h.sum()) if masked else det * det
            cost_want, grad_want = want[name, masked]
            expect = -grad_want
            if masked:  # (unmeasured_scaling - 1) * farplane elsewhere
                expect = np.where(mask_h, expect, (UMS - 1.0) * far_h)
            for u16 in (False, True):
                if u16:
                    data = torch.from_numpy(
                        (junk if masked else counts).view(np.int16)).to(
                            dev).view(torch.uint16)
                else:
                    data = torch.from_numpy(f32_nan if masked else f32).to(dev)
                for grad in (False, True):
                    for with_intensity in (False, True):
                        runs = []
                        for _ in range(2):
                            far = far0.clone()
                            costs = torch.full((nframe,), -1.0, device=dev)
                            out_i = (torch.full((nframe, det, det), -1.0,
                                                device=dev)
                                     if with_intensity else None)
                            _call(torch, lib, far, data, mask, out_i, costs,
                                  nframe, fly, S, det, model, grad, UMS, nmeas)
                            runs.append((far, costs, out_i))
                        (far, costs, out_i), again = runs
                        tag = (name, masked, u16, grad, with_intensity)
                        assert torch.equal(far.view(torch.int64),
                                           again[0].view(torch.int64)), tag
                        assert torch.equal(costs.view(torch.int32),
                                           again[1].view(torch.int32)), tag
                        c = costs.cpu().numpy().astype(np.float64)
                        assert np.all(np.isfinite(c)), tag
                        worst["cost"] = max(worst["cost"], np.max(
                            np.abs(c - cost_want) / np.abs(cost_want)))
                        np.testing.assert_allclose(c, cost_want,
                                                   rtol=OP_NORMWISE,
                                                   err_msg=str(tag))
                        if with_intensity:
                            assert torch.equal(out_i, again[2]), tag
                            worst["intensity"] = max(
                                worst["intensity"],
                                relerr(out_i.cpu().numpy(), inten))
                            assert_close(out_i.cpu().numpy(), inten,
                                         what=f"intensity {tag}")
                        if grad:
                            got = far.cpu().numpy()
                            assert np.all(np.isfinite(got)), tag
                            worst["grad"] = max(worst["grad"],
                                                relerr(got, expect))
                            assert_close(got, expect,
                                         what=f"far-plane gradient {tag}")
                        else:
                            assert torch.equal(far.view(torch.int64),
                                               far0.view(torch.int64)), tag
    print(f"{(nframe, fly, S, det)}: worst cost rel {worst['cost']:.2e}, "
          f"gradient normwise {worst['grad']:.2e}, intensity normwise "
          f"{worst['intensity']:.2e}")


def test_kernel_at_fly_1_agrees_with_the_per_position_kernel():
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    nframe, fly, S, det = KERNEL_CASES[0]
    far_h, counts, mask_h, _, _ = _kernel_case(nframe, fly, S, det)
    dev = torch.device("cuda")
    data = torch.from_numpy(fs.masked(counts.astype(np.float32), mask_h)).to(dev)
    mask = torch.from_numpy(mask_h.astype(np.uint8)).to(dev)
    nmeas = int(mask_h.sum())
    for model in (0, 1):
        a = torch.from_numpy(far_h).to(dev)
        b = a.clone()
        ca, cb = torch.empty(nframe, device=dev), torch.empty(nframe, device=dev)
        ia = torch.empty((nframe, det, det), device=dev)
        ib = torch.empty_like(ia)
        _call(torch, lib, a, data, mask, ia, ca, nframe, 1, S, det, model,
              True, 0.5, nmeas)
        check(lib.tike_farplane_gradient(
            A.ptr(b), A.ptr(data), A.ptr(mask), A.ptr(ib), A.ptr(cb), nframe,
            S, det, model, 1, 0.5, nmeas, A.stream_ptr()),
            "tike_farplane_gradient")
        assert_close(a.cpu().numpy(), b.cpu().numpy(), what="far plane")
        assert_close(ia.cpu().numpy(), ib.cpu().numpy(), what="intensity")
        np.testing.assert_allclose(ca.cpu().numpy(), cb.cpu().numpy(),
                                   rtol=OP_NORMWISE)


def test_kernel_without_frames_and_bad_arguments():
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import ERR_ARG, lib
    dev = torch.device("cuda")
    far = torch.ones((2, 1, 1, 4, 4), dtype=torch.complex64, device=dev)
    data = torch.ones((1, 4, 4), device=dev)
    costs = torch.full((1,), -1.0, device=dev)
    st = A.stream_ptr()
    fn = lib.tike_fly_farplane_gradient
    assert fn(A.ptr(far), A.ptr(data), 0, None, None, A.ptr(costs), 0, 2, 1,
              4, 0, 1, 1.0, 16, st) == 0
    torch.cuda.synchronize()
    assert float(costs[0]) == -1.0 and bool((far == 1).all())
    assert fn(None, A.ptr(data), 0, None, None, None, 1, 2, 1, 4, 0, 1, 1.0,
              16, st) == ERR_ARG
    assert fn(A.ptr(far), None, 0, None, None, None, 1, 2, 1, 4, 0, 1, 1.0,
              16, st) == ERR_ARG
    assert fn(A.ptr(far), A.ptr(data), 0, None, None, None, 1, 0, 1, 4, 0, 1,
              1.0, 16, st) == ERR_ARG
    assert fn(A.ptr(far), A.ptr(data), 0, None, None, None, 1, 2, 0, 4, 0, 1,
              1.0, 16, st) == ERR_ARG


# ---------------------------------------------------------------- the operator
def test_operator_and_simulate_vs_reference(tp, fx):
    import tike_amd.operators as tops
    K = fs.FIXTURE
    fly, det = K["fly"], K["det"]
    scan, psi, probe, data = fx["scan"], fx["psi"], fx["probe"], fx["data"]
    P = fs.problem(**K)
    sim = tp.simulate(det, probe, scan, P["psi"], fly=fly)
    assert sim.shape == fx["simulated"].shape
    assert_close(sim, fx["simulated"], what="simulate(fly=3)")
    with tops.Ptycho(det, K["pw"], nz=K["obj"], n=K["obj"]) as op:
        inten, far = op._compute_intensity(data, psi, scan, probe, fly=fly)
        assert far.shape == (len(scan), 1, K["S"], det, det)
        assert_close(inten, fx["intensity"], what="_compute_intensity(fly=3)")
        for model in ("gaussian", "poisson"):
            c = float(op.cost(data, psi, scan, probe, model=model, fly=fly))
            want = float(fx[f"cost_{model}"])
            assert abs(c - want) <= OP_NORMWISE * abs(want), (model, c, want)
        # fly == 1 is today's path
        one, _ = op._compute_intensity(None, psi, scan, probe)
        assert one.shape == (len(scan), det, det)
        assert_close(one.reshape(-1, fly, det, det).sum(axis=1),
                     fx["intensity"], what="fly=1 intensities summed")


# ------------------------------------------------------------------ the solver
def parameters(tp, P, model, mask, recover_probe, epochs=2, cg_iter=2,
               num_batch=1):
    pw = P["probe"].shape[-1]
    det = P["data"].shape[-1]
    eo = tp.ExitWaveOptions(
        measured_pixels=mask if mask is not None else np.ones((det, det), bool),
        noise_model=model)
    return tp.PtychoParameters(
        probe=P["probe0"].copy(), psi=P["psi0"].copy(), scan=P["scan"].copy(),
        algorithm_options=tp.CgradOptions(num_batch=num_batch, cg_iter=cg_iter,
                                          num_iter=epochs, step_length=1.0,
                                          batch_method="contiguous"),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False)
        if recover_probe else None,
        object_options=tp.ObjectOptions(), exitwave_options=eo)


@pytest.mark.parametrize("model,use_mask,recover_probe", fs.SOLVER_VARIANTS)
@pytest.mark.parametrize("case", sorted(fs.SOLVER_CASES))
def test_cgrad_fly_vs_float64_model(tp, case, model, use_mask, recover_probe):
    """Two epochs of reconstruct(..., fly=3) on the fixture problem (unfused
    adjoint) and on 64^2 with a 64^2 probe window; every line-search decision
    of the model is clear (test_fly_scan_cpu.py)."""
    state, P, mask = fs.run_model(case, model, use_mask, recover_probe)
    assert min(state["margins"]) >= fs.MIN_MARGIN
    fly = fs.SOLVER_CASES[case]["fly"]
    N = len(P["scan"])
    got = tp.reconstruct(P["data"], parameters(tp, P, model, mask,
                                               recover_probe), fly=fly,
                         order=np.arange(N), batches=[np.arange(N)])
    costs = np.array(got.algorithm_options.costs)
    print(case, model, use_mask, recover_probe,
          f"psi {relerr(got.psi, state['psi']):.2e} probe "
          f"{relerr(got.probe, state['probe']):.2e} costs",
          np.ravel(costs), "vs", np.ravel(state["costs"]))
    np.testing.assert_allclose(costs, np.array(state["costs"]),
                               rtol=RECON_NORMWISE)
    assert relerr(got.psi, state["psi"]) <= RECON_NORMWISE
    assert relerr(got.probe, state["probe"]) <= RECON_NORMWISE
    if not recover_probe:
        assert np.array_equal(got.probe, P["probe0"])
    assert np.array_equal(got.scan, P["scan"])


def _fixture_run(tp, epochs=2, model="gaussian", **kw):
    K = fs.FIXTURE
    P = fs.problem(**K)
    mask = fs.block_mask(K["det"])
    data = fs.masked(P["data"], mask)
    params = parameters(tp, P, model, mask, True, epochs=epochs)
    with tp.Reconstruction(data, params, fly=K["fly"], **kw) as ctx:
        ctx.iterate(epochs)
        return ctx.get_result(), ctx, P, data


def test_costs_do_not_increase(tp):
    r, _, _, _ = _fixture_run(tp, epochs=4)
    costs = np.ravel(r.algorithm_options.costs)
    print("costs", costs)
    assert len(costs) == 4 and np.all(np.diff(costs) <= 0)
    r, _, _, _ = _fixture_run(tp, epochs=4, model="poisson")
    costs = np.ravel(r.algorithm_options.costs)
    assert len(costs) == 4 and np.all(np.diff(costs) <= 0)


def test_data_on_host_equals_resident(tp):
    a, _, _, _ = _fixture_run(tp)
    b, _, _, _ = _fixture_run(tp, data_on_host=True)
    assert relerr(b.psi, a.psi) <= 1e-6 and relerr(b.probe, a.probe) <= 1e-6
    np.testing.assert_allclose(b.algorithm_options.costs,
                               a.algorithm_options.costs, rtol=1e-6)
    # 16-bit counts stay 16-bit
    K = fs.FIXTURE
    P = fs.problem(**K)
    counts = np.round(P["data"]).astype(np.uint16)
    for kw in ({}, dict(data_on_host=True)):
        with tp.Reconstruction(counts, parameters(tp, P, "poisson", None, True),
                               fly=K["fly"], **kw) as ctx:
            import torch
            assert ctx.data.dtype == torch.uint16
            ctx.iterate(1)
            assert np.isfinite(ctx.get_result().algorithm_options.costs[-1][0])


def test_orders_and_batches(tp):
    """Injected `order` / `batches` are honoured (the data rows follow the
    frame order; the result equals that of the hand-permuted problem), bad
    ones are refused; the default order keeps every frame's positions
    together."""
    K = fs.FIXTURE
    fly, F = K["fly"], K["nframe"]
    N = F * fly
    from tike_amd.ptycho.ptycho import expand_frames
    frame_order = np.random.default_rng(5).permutation(F)
    order, batches = expand_frames(frame_order,
                                   [np.arange(0, 5), np.arange(5, F)], fly)
    a, ctx, P, data = _fixture_run(tp, order=order, batches=batches,
                                   spatial_sort=False)
    assert np.array_equal(ctx.order, order)
    assert [len(b) for b in ctx.batches] == [15, 21]
    assert np.array_equal(ctx.local_frame_order, frame_order)
    # the same problem, permuted by hand
    mask = fs.block_mask(K["det"])
    Q = dict(P, scan=P["scan"][order], data=data[frame_order])
    b = tp.reconstruct(Q["data"], parameters(tp, Q, "gaussian", mask, True),
                       fly=fly, order=np.arange(N), batches=batches,
                       spatial_sort=False)
    assert relerr(a.psi, b.psi) <= 1e-6 and relerr(a.probe, b.probe) <= 1e-6
    assert np.array_equal(a.scan, P["scan"])  # results come back in input order
    bad = order.copy()
    bad[[0, 1]] = bad[[1, 0]]
    with pytest.raises(ValueError):
        _fixture_run(tp, order=bad, batches=batches)
    with pytest.raises(ValueError):
        _fixture_run(tp, order=order, batches=[np.arange(0, 4),
                                               np.arange(4, N)])
    # clustering and spatial sorting act on frames
    params = parameters(tp, P, "gaussian", mask, True, num_batch=3)
    with tp.Reconstruction(data, params, fly=fly) as ctx:
        rows = ctx.order.reshape(F, fly)
        assert np.array_equal(np.sort(ctx.order), np.arange(N))
        assert np.array_equal(rows, rows[:, :1] + np.arange(fly))
        assert np.all(rows[:, 0] % fly == 0)
        assert len(ctx.batches) == 3
        assert all(len(b) % fly == 0 for b in ctx.batches)
        assert ctx.data.shape[0] == F
        ctx.iterate(2)
        costs = np.ravel(ctx.get_result().algorithm_options.costs)
        assert np.all(np.isfinite(costs)) and costs[1] < costs[0]


# ------------------------------------------------------------------- two ranks
def _ranks(tmp_path, world):
    """Fresh child processes, one per rank (gloo, one GPU)."""
    here = os.path.dirname(os.path.abspath(__file__))
    store = tmp_path / f"store_{world}"
    outs = [str(tmp_path / f"out_{world}_{rank}.npz") for rank in range(world)]
    procs = [subprocess.Popen(
        [sys.executable, os.path.join(here, "_fly_scan_child.py"), str(rank),
         str(world), str(store), outs[rank]],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for rank in range(world)]
    for proc in procs:
        out, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, out[-2000:] + err[-4000:]
    return [np.load(o) for o in outs]


def test_two_ranks_match_one_rank(tmp_path):
    one, = _ranks(tmp_path, 1)
    two = _ranks(tmp_path, 2)
    fly = fs.FIXTURE["fly"]
    assert list(one["shares"]) == [fly, 11 * fly]
    assert list(two[0]["shares"]) == [fly, 6 * fly]
    assert list(two[1]["shares"]) == [0, 5 * fly]  # an empty share
    for r in two:
        print(f"two ranks: psi {relerr(r['psi'], one['psi']):.2e} probe "
              f"{relerr(r['probe'], one['probe']):.2e}")
        assert relerr(r["psi"], one["psi"]) <= 1e-4
        assert relerr(r["probe"], one["probe"]) <= 1e-4
        np.testing.assert_allclose(r["costs"], one["costs"], rtol=1e-4)
        assert np.array_equal(r["scan"], one["scan"])
        assert np.array_equal(r["psi"], two[0]["psi"])
