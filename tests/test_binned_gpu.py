"""Detector binning on the GPU: `tike_binned_farplane_gradient` and
`tike_binned_cost_factor` against the float64 model (tests/binned.py) on the
smallest shapes that reach every path of the kernel, the operator and
`simulate` against block sums of their own unbinned results, cgrad on binned
data against the model's cgrad, and `autograd.cost(binning=2)` against
`Ptycho.cost` and against `intensity` + `avg_pool2d` + the loss in torch."""
import numpy as np
import pytest

import binned as bn
import fly_scan as fs
from util import OP_NORMWISE, assert_close, relerr

pytestmark = pytest.mark.gpu

RECON_NORMWISE = 1e-3  # the project's reconstruction bar


@pytest.fixture(scope="module")
def tp():
    import tike_amd.ptycho as m
    return m


# ----------------------------------------------------------------- the kernel
# (nframe, fly, S, det, B)
KERNEL_CASES = [
    (3, 1, 1, 16, 2),  # smallest register-resident case
    (2, 2, 1, 32, 4),  # register-resident, fly 2
    (2, 1, 3, 33, 3),  # general path; odd w; rows not a multiple of 4
    (1, 1, 5, 64, 2),  # next register class
    (1, 3, 3, 24, 4),  # B * P past 16 while P is not: second read of the rows
    (2, 2, 2, 48, 8),  # cross-lane bins; B * P = 32: two pixels per lane
    (2, 1, 17, 16, 2),  # P past 16
    # (beyond the issue's list: paths the kernel grew)
    (2, 1, 2, 48, 8),  # cross-lane bins, four pixels per lane, in registers
    (1, 2, 3, 24, 4),  # B * P = 24: two pixels per lane, two lanes per bin
    (1, 1, 9, 16, 2),  # B * P = 18: two pixels per lane, one lane per bin
]

_CASES = {}


def _kernel_case(nframe, fly, S, det, B):
    """Random far planes and integer counts (the same values as float32 and
    as uint16) and the float64 model's results for both noise models, with
    and without the mask at data resolution -- computed once per case, shared
    by the tests, left unchanged."""
    key = (nframe, fly, S, det, B)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(det + 7 * B)
    N, w = nframe * fly, det // B
    far = (rng.standard_normal((N, 1, S, det, det))
           + 1j * rng.standard_normal((N, 1, S, det, det))).astype(np.complex64)
    counts = rng.poisson(2.0 * fly * S * B * B, (nframe, w, w)).astype(
        np.uint16)
    mask = fs.block_mask(w)
    inten = bn.frame_intensity(far, fly, B)
    want = {}
    for model in ("gaussian", "poisson"):
        for m in (None, mask):
            d = counts.astype(np.float64)
            dm = fs.masked(d, m) if m is not None else d
            want[model, m is not None] = (
                bn.cost_each(model, d, inten, m),
                bn.farplane_gradient(model, dm, far, fly, B, m))
    _CASES[key] = far, counts, mask, inten, want
    return _CASES[key]


def _call(torch, lib, far, data, mask, intensity, costs, nframe, fly, S, det,
          B, model, grad, ums, nmeasured):
    from tike_amd import _arrays as A
    from tike_amd._lib import check
    check(lib.tike_binned_farplane_gradient(
        A.ptr(far), A.ptr(data), int(data.dtype == torch.uint16), A.ptr(mask),
        A.ptr(intensity), A.ptr(costs), nframe, fly, S, det, B, model,
        int(grad), ums, nmeasured, A.stream_ptr()),
        "tike_binned_farplane_gradient")


def _counts_on_device(torch, counts, mask_h, masked, u16):
    """float32 counts NaN under the mask, uint16 counts 65535 under it."""
    dev = torch.device("cuda")
    if u16:
        c = counts.copy()
        if masked:
            c[:, ~mask_h] = 65535  # uint16 has no NaN: must not be read
        return torch.from_numpy(c.view(np.int16)).to(dev).view(torch.uint16)
    f32 = counts.astype(np.float32)
    return torch.from_numpy(fs.masked(f32, mask_h) if masked else f32).to(dev)


@pytest.mark.parametrize("nframe,fly,S,det,B", KERNEL_CASES)
def test_kernel_vs_float64_model(nframe, fly, S, det, B):
    """gaussian and Poisson, with and without the block mask at data
    resolution, float32 and uint16 counts, costs only and with the gradient,
    intensity NULL and given; two calls give the same bits; a costs-only call
    leaves the far plane as it was; the costs of all four kinds of call carry
    the same bits; everything finite."""
    import torch

    from tike_amd._lib import lib
    far_h, counts, mask_h, inten, want = _kernel_case(nframe, fly, S, det, B)
    w = det // B
    dev = torch.device("cuda")
    far0 = torch.from_numpy(far_h).to(dev)
    mask_d = torch.from_numpy(mask_h.astype(np.uint8)).to(dev)
    fine_mask = bn.spread(mask_h, B)
    UMS = 0.75
    worst = dict(cost=0.0, grad=0.0, intensity=0.0)
    for model, name in enumerate(("gaussian", "poisson")):
        for masked in (False, True):
            mask = mask_d if masked else None
            nmeas = int(mask_h.sum()) if masked else w * w
            cost_want, grad_want = want[name, masked]
            expect = -grad_want
            if masked:  # (unmeasured_scaling - 1) * farplane elsewhere
                expect = np.where(fine_mask, expect, (UMS - 1.0) * far_h)
            for u16 in (False, True):
                data = _counts_on_device(torch, counts, mask_h, masked, u16)
                bits = None  # of the costs: one set for every kind of call
                for grad in (False, True):
                    for with_intensity in (False, True):
                        runs = []
                        for _ in range(2):
                            far = far0.clone()
                            costs = torch.full((nframe,), -1.0, device=dev)
                            out_i = (torch.full((nframe, w, w), -1.0,
                                                device=dev)
                                     if with_intensity else None)
                            _call(torch, lib, far, data, mask, out_i, costs,
                                  nframe, fly, S, det, B, model, grad, UMS,
                                  nmeas)
                            runs.append((far, costs, out_i))
                        (far, costs, out_i), again = runs
                        tag = (name, masked, u16, grad, with_intensity)
                        assert torch.equal(far.view(torch.int64),
                                           again[0].view(torch.int64)), tag
                        assert torch.equal(costs.view(torch.int32),
                                           again[1].view(torch.int32)), tag
                        bits = costs if bits is None else bits
                        assert torch.equal(costs.view(torch.int32),
                                           bits.view(torch.int32)), tag
                        c = costs.cpu().numpy().astype(np.float64)
                        assert np.all(np.isfinite(c)), tag
                        worst["cost"] = max(worst["cost"], np.max(
                            np.abs(c - cost_want) / np.abs(cost_want)))
                        if with_intensity:
                            assert torch.equal(out_i, again[2]), tag
                            worst["intensity"] = max(
                                worst["intensity"],
                                relerr(out_i.cpu().numpy(), inten))
                        if grad:
                            got = far.cpu().numpy()
                            assert np.all(np.isfinite(got)), tag
                            worst["grad"] = max(worst["grad"],
                                                relerr(got, expect))
                        else:
                            assert torch.equal(far.view(torch.int64),
                                               far0.view(torch.int64)), tag
                        np.testing.assert_allclose(c, cost_want,
                                                   rtol=OP_NORMWISE,
                                                   err_msg=str(tag))
                        if with_intensity:
                            assert_close(out_i.cpu().numpy(), inten,
                                         what=f"intensity {tag}")
                        if grad:
                            assert_close(got, expect,
                                         what=f"far-plane gradient {tag}")
    print(f"{(nframe, fly, S, det, B)}: worst cost rel {worst['cost']:.2e}, "
          f"gradient normwise {worst['grad']:.2e}, intensity normwise "
          f"{worst['intensity']:.2e}")


@pytest.mark.parametrize("nframe,fly,S,det", [(3, 1, 1, 16), (2, 3, 2, 33),
                                              (2, 2, 9, 32)])
def test_binning_1_has_the_bits_of_the_fly_entry(nframe, fly, S, det):
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    far_h, counts, mask_h, _, _ = _kernel_case(nframe, fly, S, det, 1)
    dev = torch.device("cuda")
    mask = torch.from_numpy(mask_h.astype(np.uint8)).to(dev)
    nmeas = int(mask_h.sum())
    for model in (0, 1):
        for u16 in (False, True):
            for grad in (False, True):
                data = _counts_on_device(torch, counts, mask_h, True, u16)
                a = torch.from_numpy(far_h).to(dev)
                b = a.clone()
                ca = torch.empty(nframe, device=dev)
                cb = torch.empty_like(ca)
                ia = torch.empty((nframe, det, det), device=dev)
                ib = torch.empty_like(ia)
                _call(torch, lib, a, data, mask, ia, ca, nframe, fly, S, det,
                      1, model, grad, 0.5, nmeas)
                check(lib.tike_fly_farplane_gradient(
                    A.ptr(b), A.ptr(data), int(u16), A.ptr(mask), A.ptr(ib),
                    A.ptr(cb), nframe, fly, S, det, model, int(grad), 0.5,
                    nmeas, A.stream_ptr()), "tike_fly_farplane_gradient")
                tag = (model, u16, grad)
                assert torch.equal(a.view(torch.int64),
                                   b.view(torch.int64)), tag
                assert torch.equal(ia.view(torch.int32),
                                   ib.view(torch.int32)), tag
                assert torch.equal(ca.view(torch.int32),
                                   cb.view(torch.int32)), tag


@pytest.mark.parametrize("nframe,fly,S,det,B", KERNEL_CASES)
def test_cost_factor(nframe, fly, S, det, B):
    """Costs with the bits of `tike_binned_farplane_gradient`; the table
    against the model at the operator bar, exactly constant over every bin and
    exactly 0 on unmeasured bins; costs alone and table alone give the same;
    the far plane is not written; two calls give the same bits."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    far_h, counts, mask_h, _, _ = _kernel_case(nframe, fly, S, det, B)
    w, P = det // B, fly * S
    dev = torch.device("cuda")
    far = torch.from_numpy(far_h).to(dev)
    mask_d = torch.from_numpy(mask_h.astype(np.uint8)).to(dev)
    up_h = (np.linspace(0.5, 1.5, nframe)
            * np.where(np.arange(nframe) % 2, -1, 1)).astype(np.float32)
    up = torch.from_numpy(up_h).to(dev)
    st = A.stream_ptr()
    worst = 0.0

    def factor(data, mask, upstream, costs, table, nmeas, model):
        check(lib.tike_binned_cost_factor(
            A.ptr(far), A.ptr(data), int(data.dtype == torch.uint16),
            A.ptr(mask), A.ptr(upstream), A.ptr(costs), A.ptr(table), nframe,
            P, det * det, model, nmeas, det, B, st), "tike_binned_cost_factor")

    for model, name in enumerate(("gaussian", "poisson")):
        for masked in (False, True):
            mask = mask_d if masked else None
            m = mask_h if masked else None
            nmeas = int(mask_h.sum()) if masked else w * w
            d64 = counts.astype(np.float64)
            want = bn.cost_factor_table(
                name, fs.masked(d64, m) if masked else d64, far_h, fly, B, m,
                up_h)
            for u16 in (False, True):
                data = _counts_on_device(torch, counts, mask_h, masked, u16)
                ref = torch.empty(nframe, device=dev)
                _call(torch, lib, far, data, mask, None, ref, nframe, fly, S,
                      det, B, model, False, 1.0, nmeas)
                outs = []
                for _ in range(2):
                    costs = torch.full((nframe,), -1.0, device=dev)
                    table = torch.full((nframe, det, det), -1.0, device=dev)
                    factor(data, mask, up, costs, table, nmeas, model)
                    outs.append((costs, table))
                (costs, table), again = outs
                tag = (name, masked, u16)
                assert torch.equal(costs.view(torch.int32),
                                   ref.view(torch.int32)), tag
                assert torch.equal(costs, again[0]), tag
                assert torch.equal(table.view(torch.int32),
                                   again[1].view(torch.int32)), tag
                alone = torch.full((nframe,), -1.0, device=dev)
                factor(data, mask, None, alone, None, nmeas, model)
                assert torch.equal(alone, costs), tag
                only = torch.full((nframe, det, det), -1.0, device=dev)
                factor(data, mask, up, None, only, nmeas, model)
                assert torch.equal(only.view(torch.int32),
                                   table.view(torch.int32)), tag
                t = table.cpu().numpy()
                assert np.all(np.isfinite(t)), tag
                blocks = t.reshape(nframe, w, B, w, B)
                assert np.all(blocks == blocks[:, :, :1, :, :1]), tag
                if masked:
                    assert np.all(t[:, ~bn.spread(mask_h, B)] == 0.0), tag
                worst = max(worst, relerr(t, want))
                assert_close(t, want, what=f"table {tag}")
    assert torch.equal(far.cpu().view(torch.int64),
                       torch.from_numpy(far_h).view(torch.int64))
    print(f"cost factor {(nframe, fly, S, det, B)}: table normwise "
          f"{worst:.2e}")


def test_kernel_without_frames_and_bad_arguments():
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import ERR_ARG, lib
    dev = torch.device("cuda")
    far = torch.ones((2, 1, 1, 4, 4), dtype=torch.complex64, device=dev)
    data = torch.ones((1, 2, 2), device=dev)
    costs = torch.full((1,), -1.0, device=dev)
    table = torch.full((1, 4, 4), -1.0, device=dev)
    st = A.stream_ptr()
    fn = lib.tike_binned_farplane_gradient
    f, d, c = A.ptr(far), A.ptr(data), A.ptr(costs)
    assert fn(f, d, 0, None, None, c, 0, 2, 1, 4, 2, 0, 1, 1.0, 4, st) == 0
    torch.cuda.synchronize()
    assert float(costs[0]) == -1.0 and bool((far == 1).all())
    assert fn(None, d, 0, None, None, None, 1, 2, 1, 4, 2, 0, 1, 1.0, 4,
              st) == ERR_ARG
    assert fn(f, None, 0, None, None, None, 1, 2, 1, 4, 2, 0, 1, 1.0, 4,
              st) == ERR_ARG
    assert fn(f, d, 0, None, None, None, 1, 0, 1, 4, 2, 0, 1, 1.0, 4,
              st) == ERR_ARG  # fly
    assert fn(f, d, 0, None, None, None, 1, 2, 0, 4, 2, 0, 1, 1.0, 4,
              st) == ERR_ARG  # S
    assert fn(f, d, 0, None, None, None, 1, 2, 1, 4, 3, 0, 1, 1.0, 4,
              st) == ERR_ARG  # det % binning
    assert fn(f, d, 0, None, None, None, 1, 2, 1, 4, 0, 0, 1, 1.0, 4,
              st) == ERR_ARG  # binning < 1
    assert fn(f, d, 0, None, None, None, 1, 2, 1, 4, 2, 0, 1, 1.0, 0,
              st) == ERR_ARG  # num_measured
    fn = lib.tike_binned_cost_factor
    t = A.ptr(table)
    assert fn(f, d, 0, None, None, c, t, 0, 2, 16, 0, 4, 4, 2, st) == 0
    torch.cuda.synchronize()
    assert float(costs[0]) == -1.0 and bool((table == -1).all())
    assert fn(None, d, 0, None, None, c, t, 1, 2, 16, 0, 4, 4, 2, st) == ERR_ARG
    assert fn(f, None, 0, None, None, c, t, 1, 2, 16, 0, 4, 4, 2, st) == ERR_ARG
    assert fn(f, d, 0, None, None, c, t, 1, 2, 16, 0, 4, 4, 3, st) == ERR_ARG
    assert fn(f, d, 0, None, None, c, t, 1, 2, 16, 0, 4, 4, 0, st) == ERR_ARG
    assert fn(f, d, 0, None, None, c, t, 1, 2, 12, 0, 4, 4, 2, st) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((far == 1).all())


# ---------------------------------------------------------------- the operator
@pytest.mark.parametrize("fly", [1, 2])
@pytest.mark.parametrize("B", [2, 4])
def test_operator_and_simulate_vs_block_sums(tp, B, fly):
    """`_compute_intensity(binning=B)` and `simulate(binning=B)` against the
    block sum of the binning = 1 result of the same operator; `Ptycho.cost`
    against the float64 model."""
    import tike_amd.operators as tops
    K = dict(fs.FIXTURE, fly=fly, nframe=6)
    P = fs.problem(**K)
    det, w = K["det"], K["det"] // B
    assert det == 32
    scan, psi, probe = P["scan"], P["psi0"], P["probe"]
    fine = tp.simulate(det, probe, scan, psi, fly=fly)
    sim = tp.simulate(det, probe, scan, psi, fly=fly, binning=B)
    assert sim.shape == (K["nframe"], w, w) and sim.dtype == np.float32
    assert_close(sim, bn.block_sum(fine.astype(np.float64), B),
                 what=f"simulate(binning={B})")
    assert np.array_equal(tp.simulate(det, probe, scan, psi, fly=fly,
                                      binning=1), fine)
    data = bn.block_sum(P["data"].astype(np.float64), B).astype(np.float32)
    data = data * 1.2 + 0.5  # (away from the minimum)
    with tops.Ptycho(det, K["pw"], nz=K["obj"], n=K["obj"]) as op:
        one, far1 = op._compute_intensity(None, psi, scan, probe, fly=fly)
        inten, far = op._compute_intensity(None, psi, scan, probe, fly=fly,
                                           binning=B)
        assert inten.shape == (K["nframe"], w, w)
        assert far.shape == (len(scan), 1, K["S"], det, det)
        assert np.array_equal(far, far1)
        assert_close(inten, bn.block_sum(one.astype(np.float64), B),
                     what=f"_compute_intensity(binning={B})")
        for model in ("gaussian", "poisson"):
            c = float(op.cost(data, psi, scan, probe, model=model, fly=fly,
                              binning=B))
            want = bn.cost(model, data, psi, scan, probe, det, fly, B)
            assert abs(c - want) <= OP_NORMWISE * abs(want), (model, c, want)
            # binning == 1 is today's call
            c1 = float(op.cost(P["data"], psi, scan, probe, model=model,
                               fly=fly, binning=1))
            assert c1 == float(op.cost(P["data"], psi, scan, probe,
                                       model=model, fly=fly))
        with pytest.raises(ValueError, match="does not divide"):
            op._compute_intensity(None, psi, scan, probe, fly=fly, binning=5)


# ------------------------------------------------------------------ the solver
def parameters(tp, P, model, mask, epochs=2, cg_iter=2):
    return tp.PtychoParameters(
        probe=P["probe0"].copy(), psi=P["psi0"].copy(), scan=P["scan"].copy(),
        algorithm_options=tp.CgradOptions(num_batch=1, cg_iter=cg_iter,
                                          num_iter=epochs, step_length=1.0,
                                          batch_method="contiguous"),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(measured_pixels=mask,
                                            noise_model=model))


@pytest.mark.parametrize("model", ["gaussian", "poisson"])
@pytest.mark.parametrize("fly", bn.SOLVER_FLY)
def test_cgrad_binned_vs_float64_model(tp, fly, model):
    """Two epochs of reconstruct(..., binning=2) on a 6 x 6 scan (18 frames at
    fly = 2), a 32^2 far plane and probe window under 16^2 counts, 2 modes,
    with the mask: object, probe and cost history against the model's cgrad;
    every line-search decision of the model is clear (test_binned_cpu.py)."""
    state, P, mask = bn.run_model(fly, model)
    assert min(state["margins"]) >= bn.MIN_MARGIN
    B, N = bn.SOLVER["B"], len(P["scan"])
    assert P["data"].shape[-1] * B == P["probe0"].shape[-1] == 32
    got = tp.reconstruct(P["data"], parameters(tp, P, model, mask), fly=fly,
                         binning=B, order=np.arange(N), batches=[np.arange(N)])
    costs = np.array(got.algorithm_options.costs)
    print(fly, model, f"psi {relerr(got.psi, state['psi']):.2e} probe "
          f"{relerr(got.probe, state['probe']):.2e} costs", np.ravel(costs),
          "vs", np.ravel(state["costs"]))
    np.testing.assert_allclose(costs, np.array(state["costs"]),
                               rtol=RECON_NORMWISE)
    assert relerr(got.psi, state["psi"]) <= RECON_NORMWISE
    assert relerr(got.probe, state["probe"]) <= RECON_NORMWISE
    assert np.array_equal(got.scan, P["scan"])


def test_data_on_host_and_uint16_counts(tp):
    """Host-kept patterns go through the frame-unit plumbing of fly scans: the
    result of the resident run; 16-bit counts stay 16-bit."""
    import torch
    fly, B = 2, bn.SOLVER["B"]
    _, P, mask = bn.run_model(fly, "gaussian")
    runs = []
    for kw in ({}, dict(data_on_host=True)):
        with tp.Reconstruction(P["data"], parameters(tp, P, "gaussian", mask),
                               fly=fly, binning=B, **kw) as ctx:
            assert ctx.operator.detector_shape == 32
            assert tuple(ctx.data.shape[1:]) == (16, 16)
            ctx.iterate(2)
            runs.append(ctx.get_result())
    a, b = runs
    assert relerr(b.psi, a.psi) <= 1e-6 and relerr(b.probe, a.probe) <= 1e-6
    np.testing.assert_allclose(b.algorithm_options.costs,
                               a.algorithm_options.costs, rtol=1e-6)
    counts = np.round(40 * np.nan_to_num(P["data"])).astype(np.uint16)
    for kw in ({}, dict(data_on_host=True)):
        with tp.Reconstruction(counts, parameters(tp, P, "poisson", mask),
                               fly=fly, binning=B, **kw) as ctx:
            assert ctx.data.dtype == torch.uint16
            ctx.iterate(1)
            assert np.isfinite(ctx.get_result().algorithm_options.costs[-1][0])


def test_probe_rescale_reads_binned_patterns(tp):
    """`init_rescale_from_measurements` compares the patterns with the BINNED
    intensity of the first iterate on the measured data pixels."""
    fly, B, det = 2, bn.SOLVER["B"], bn.SOLVER["det"]
    _, P, mask = bn.run_model(fly, "gaussian")
    params = parameters(tp, P, "gaussian", mask)
    params.probe_options = tp.ProbeOptions(init_rescale_from_measurements=True)
    with tp.Reconstruction(P["data"], params, fly=fly, binning=B) as ctx:
        got = ctx.get_result().probe
    inten = bn.simulate(det, P["probe0"], P["scan"], P["psi0"], fly, B)
    want = P["probe0"] * np.sqrt(
        np.nan_to_num(P["data"])[:, mask].sum(dtype=np.float64)
        / inten[:, mask].sum())
    assert_close(got, want, what="rescaled probe")


# ------------------------------------------------------------------- autograd
import autograd_cost as ac  # noqa: E402

AUTOGRAD_CASES = [ac.CASES[0],  # plain, fly 2, det 16
                  ("eigen", ac.EIGEN_CASES[1]),  # eigen weights, det 20, fly 2
                  ("multislice", ac.MULTISLICE_CASES[0])]  # two slices, det 32
# the bars of test_autograd_cost_gpu.py's comparison with the composition on
# the device: twice those of its comparison with the model (both routes are
# float32 against the same model)
BARS = dict(psi=2 * OP_NORMWISE, probe=2 * OP_NORMWISE,
            eigen_probe=2 * OP_NORMWISE, scan=2e-6, eigen_weights=2e-6)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def _binned_inputs(c, B):
    """Counts at data resolution with no dark bin (the block sums of
    `well_conditioned_counts`), the module-gap mask at data resolution, NaN
    under it, and a signed upstream."""
    fine = ac.well_conditioned_counts(c["form"], c["m"]).astype(np.float64)
    data = bn.block_sum(fine, B).astype(np.float32)
    assert data.min() > 0
    mask = ac.module_gap_mask(c["det"] // B)
    data = np.where(mask, data, np.float32("nan")).astype(np.float32)
    up = ac.frame_weights(data.shape[0])
    return data, mask, up


def _model_scales(c, data, mask, up, model, B):
    """The float64 model's gradients (for A_scan / A_weights, the sums of
    absolute values the position and weight gradients are measured in): the
    binned table spread over the far plane, then the form's own backward."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        I = c["form"].intensity(c["m"])
        Ib = F.avg_pool2d(I[:, None], B)[:, 0] * (B * B)
        table = ac.table_of(Ib, torch.from_numpy(data.astype(np.float64)),
                            torch.from_numpy(mask), model,
                            torch.from_numpy(up))
        fine = table.repeat_interleave(B, dim=-2).repeat_interleave(B, dim=-1)
        return c["form"].grads(c["m"], fine)


@pytest.mark.parametrize("model", ac.MODELS)
@pytest.mark.parametrize("kind,shape", AUTOGRAD_CASES)
def test_autograd_cost_binned(kind, shape, model):
    """`cost(binning=2)`: the costs against `Ptycho.cost` (one slice, shared
    probe) and, with the gradients with respect to every input of the form,
    against `intensity` + `avg_pool2d * B^2` + the same loss written in torch,
    float32 both."""
    import torch
    import torch.nn.functional as F

    import tike_amd.operators as ops
    from tike_amd import autograd
    B = 2
    c = ac.case(kind, shape)
    fly, det = c["fly"], c["det"]
    data, mask, up = _binned_inputs(c, B)
    want = _model_scales(c, data, mask, up, model, B)
    names = [k for k in c["form"].names if c["host"].get(k) is not None]
    kw = {k: _dev(c["host"][k]).requires_grad_(True) for k in names}
    eigen = {k: kw[k] for k in ("eigen_probe", "eigen_weights") if k in kw}
    data_d, mask_d, up_d = _dev(data), _dev(mask), _dev(up)
    nm = int(mask.sum())
    with ops.Ptycho(**c["operator"]) as op:
        costs = autograd.cost(op, data_d, kw["psi"], kw["probe"], kw["scan"],
                              model=model, measured_pixels=mask_d, fly=fly,
                              binning=B, **eigen)
        assert costs.shape == (data.shape[0],)
        grads = torch.autograd.grad((costs * up_d).sum(),
                                    [kw[k] for k in names])
        many = kw["psi"].shape[0] > 1
        run = autograd.multislice_intensity if many else autograd.intensity
        inten = run(op, kw["psi"], kw["probe"], kw["scan"], fly=fly, **eigen)
        binned = F.avg_pool2d(inten[:, None], B)[:, 0] * (B * B)
        zero = torch.zeros_like(binned)
        d = torch.where(mask_d, data_d, zero)
        terms = ((torch.sqrt(binned) - torch.sqrt(d))**2 if model == "gaussian"
                 else binned - d * torch.log(binned + 1e-9))
        ccosts = torch.where(mask_d, terms, zero).sum(dim=(1, 2)) / nm
        cgrads = torch.autograd.grad((ccosts * up_d).sum(),
                                     [kw[k] for k in names])
        if kind == "plain":
            # (no mask in Ptycho.cost: the same call without one)
            plain = autograd.cost(op, torch.nan_to_num(data_d), kw["psi"],
                                  kw["probe"], kw["scan"], model=model,
                                  fly=fly, binning=B)
            mean = float(op.cost(torch.nan_to_num(data_d),
                                 kw["psi"].detach(), kw["scan"].detach(),
                                 kw["probe"].detach(), model=model, fly=fly,
                                 binning=B))
            got = float(plain.detach().mean())
            assert abs(got - mean) <= 1e-6 * abs(mean), (got, mean)
    h = lambda x: x.detach().cpu().numpy()
    cerr = np.abs(h(costs) - h(ccosts)) / np.abs(h(ccosts))
    what = f"{kind} {shape} {model} binning={B}"
    errors = {}
    for name, g, cg in zip(names, grads, cgrads):
        g, cg = h(g), h(cg)
        assert np.all(np.isfinite(g)), name
        if name in ("scan", "eigen_weights"):
            A = want["A_" + ("scan" if name == "scan" else "weights")].numpy()
            live = A > 0
            errors[name] = float((np.abs(g - cg)[live] / A[live]).max())
        else:
            errors[name] = relerr(g, cg)
    print(f"{what}: costs max rel {cerr.max():.2e}; "
          + ", ".join(f"{k} {v:.2e}" for k, v in errors.items()))
    assert np.all(np.isfinite(h(costs))) and np.all(cerr <= 2e-5), cerr
    for k, v in errors.items():
        assert v <= BARS[k], (what, k, v)
