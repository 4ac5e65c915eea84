"""A fitted incoherent background on the GPU: the three entries of
background.hip against the float64 model (tests/background.py) and against
the entries they extend, bit for bit where they must agree; cgrad with
`background_options` against the model's three-block cgrad;
`autograd.cost(background=)` against `intensity + b` with the loss written in
torch; the demonstration.

Every figure a bar is set on is printed before it is asserted."""
import numpy as np
import pytest

import autograd_cost as ac
import background as bg
import fly_scan as fs
import test_autograd_cost_gpu as tc
from test_binned_gpu import BARS
from util import OP_NORMWISE, assert_close, relerr

pytestmark = pytest.mark.gpu

RECON_NORMWISE = 1e-3  # the project's reconstruction bar
MODEL_ID = {"gaussian": 0, "poisson": 1}


@pytest.fixture(scope="module")
def tp():
    import tike_amd.ptycho as m
    return m


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(
        np.ascontiguousarray(a)).to("cuda")


def _u16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(
        "cuda").view(torch.uint16)


def _bits(x):
    import torch
    return x.view(torch.int64 if x.dtype == torch.complex64 else torch.int32)


# ------------------------------------------------------------ the first entry
# (nframe, fly, S, det): smallest; fly 2; npix % 4 != 0; the next register
# class; exactly 16 planes; the second read
FIRST_CASES = [(3, 1, 1, 16), (2, 2, 1, 32), (2, 1, 3, 33), (1, 1, 5, 64),
               (1, 4, 4, 16), (2, 1, 17, 16)]


def _first(far, data, mask, background, intensity, costs, nframe, fly, S, det,
           model, grad, ums, nmeasured, entry="background"):
    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    u16 = int(str(data.dtype) == "torch.uint16")
    if entry == "fly":
        check(lib.tike_fly_farplane_gradient(
            A.ptr(far), A.ptr(data), u16, A.ptr(mask), A.ptr(intensity),
            A.ptr(costs), nframe, fly, S, det, model, int(grad), ums,
            nmeasured, A.stream_ptr()), "tike_fly_farplane_gradient")
        return
    check(lib.tike_background_farplane_gradient(
        A.ptr(far), A.ptr(data), u16, A.ptr(mask), A.ptr(background),
        A.ptr(intensity), A.ptr(costs), nframe, fly, S, det, model, int(grad),
        ums, nmeasured, A.stream_ptr()), "tike_background_farplane_gradient")


@pytest.mark.parametrize("nframe,fly,S,det", FIRST_CASES)
def test_farplane_gradient(nframe, fly, S, det):
    """Both models, with and without the block mask (NaN under it, in the
    counts and in the background), float32 and uint16 counts.  With a
    background of zeros and with NULL: far plane, costs and intensity have the
    bits of tike_fly_farplane_gradient.  With a positive random b: costs
    (rtol OP_NORMWISE) and far plane (normwise, `assert_close`) against the
    float64 model -- the bars of test_binned_gpu.py's kernel test --, the
    intensity has the fly entry's bits, a costs-only call leaves the far plane
    untouched, two calls give the same bits."""
    import torch
    rng = np.random.default_rng(det + 7 * S)
    N = nframe * fly
    far_h = (rng.standard_normal((N, 1, S, det, det))
             + 1j * rng.standard_normal((N, 1, S, det, det))).astype(
                 np.complex64)
    counts = rng.poisson(2.0 * fly * S + 1.0, (nframe, det, det)).astype(
        np.uint16)
    b_h = rng.uniform(0.2, 2.0, (det, det)).astype(np.float32)
    mask_h = fs.block_mask(det)
    inten = fs.frame_intensity(far_h, fly)
    far0 = _dev(far_h)
    mask_d = _dev(mask_h.astype(np.uint8))
    junk = counts.copy()
    junk[:, ~mask_h] = 65535  # uint16 has no NaN: counts that must not be read
    UMS = 0.75
    worst = dict(cost=0.0, grad=0.0)
    for name, model in MODEL_ID.items():
        for masked in (False, True):
            m = mask_h if masked else None
            mask = mask_d if masked else None
            nmeas = int(mask_h.sum()) if masked else det * det
            d64 = counts.astype(np.float64)
            cost_want = fs.cost_each(name, d64, inten + b_h.astype(np.float64),
                                     m)
            expect = -bg.farplane_gradient(
                name, fs.masked(d64, m) if masked else d64, far_h, fly, m,
                b_h.astype(np.float64))
            if masked:
                expect = np.where(mask_h, expect, (UMS - 1.0) * far_h)
            b_pos = _dev(np.where(mask_h, b_h, np.float32("nan"))
                         if masked else b_h)
            zeros = torch.zeros((det, det), device="cuda")
            for u16 in (False, True):
                data = (_u16(junk if masked else counts) if u16 else _dev(
                    fs.masked(counts.astype(np.float32), mask_h) if masked
                    else counts.astype(np.float32)))
                tag = (name, masked, u16)

                def run(background, grad, entry="background"):
                    far = far0.clone()
                    costs = torch.full((nframe,), -1.0, device="cuda")
                    out_i = torch.full((nframe, det, det), -1.0, device="cuda")
                    _first(far, data, mask, background, out_i, costs, nframe,
                           fly, S, det, model, grad, UMS, nmeas, entry)
                    return far, costs, out_i

                for grad in (False, True):
                    ref = run(None, grad, "fly")
                    for background in (zeros, None):
                        got = run(background, grad)
                        for g, r in zip(got, ref):
                            assert torch.equal(_bits(g), _bits(r)), (tag, grad)
                    got, again = run(b_pos, grad), run(b_pos, grad)
                    for g, r in zip(got, again):
                        assert torch.equal(_bits(g), _bits(r)), (tag, grad)
                    far, costs, out_i = got
                    assert torch.equal(_bits(out_i), _bits(ref[2])), tag
                    c = costs.cpu().numpy().astype(np.float64)
                    assert np.all(np.isfinite(c)), tag
                    worst["cost"] = max(worst["cost"], np.max(
                        np.abs(c - cost_want) / np.abs(cost_want)))
                    np.testing.assert_allclose(c, cost_want, rtol=OP_NORMWISE,
                                               err_msg=str(tag))
                    if grad:
                        g = far.cpu().numpy()
                        assert np.all(np.isfinite(g)), tag
                        worst["grad"] = max(worst["grad"], relerr(g, expect))
                        assert_close(g, expect,
                                     what=f"far-plane gradient {tag}")
                    else:
                        assert torch.equal(_bits(far), _bits(far0)), tag
    print(f"{(nframe, fly, S, det)}: worst cost rel {worst['cost']:.2e}, "
          f"gradient normwise {worst['grad']:.2e}")


# ----------------------------------------------------------- the second entry
def _second(far_d, data_d, u16, mask_d, b_d, up_d, costs, table, nframe, P,
            npix, model, nm):
    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    check(lib.tike_background_cost_factor(
        A.ptr(far_d), A.ptr(data_d), int(u16), A.ptr(mask_d), A.ptr(b_d),
        A.ptr(up_d), A.ptr(costs), A.ptr(table), nframe, P, npix,
        MODEL_ID[model], nm, A.stream_ptr()), "tike_background_cost_factor")


def _background_for(npix, mask, seed):
    """A positive float32 background of npix pixels, NaN under the mask."""
    b = np.random.default_rng(seed).uniform(0.5, 4.0, npix).astype(np.float32)
    return b if mask is None else np.where(mask, b, np.float32("nan"))


@pytest.mark.parametrize("model,masked,u16", tc.ENTRY_VARIANTS)
@pytest.mark.parametrize("nframe,P,npix", tc.ENTRY_CASES)
def test_cost_factor(nframe, P, npix, model, masked, u16):
    """costs: the bits of tike_background_farplane_gradient on the same far
    plane (where that entry can be asked: npix a square).  The table: the
    bits of tike_cost_factor at b = 0 (zeros and NULL); exactly 0 under the
    mask; on measured pixels |err| <= 1e-6 |upstream_f| (1 + sqrt(d) /
    (sqrt(Ib) + 1e-9)) / num_measured (poisson: d / (Ib + 1e-9)) against the
    float64 factor at the FLOAT32 Ib = I + b."""
    import torch
    far, _, data, mask, upstream = tc._entry_inputs(nframe, P, npix, masked,
                                                    u16)
    nm = npix if mask is None else int(mask.sum())
    far_d, up_d = _dev(far), _dev(upstream)
    data_d = _u16(data) if u16 else _dev(data)
    mask_d = None if mask is None else _dev(mask.astype(np.uint8))
    b = _background_for(npix, mask, npix + P)
    b_d = _dev(b)

    def run(background, entry=_second):
        costs = torch.full((nframe,), 7.0, device="cuda")
        table = torch.full((nframe, npix), 7.0, device="cuda")
        if entry is _second:
            _second(far_d, data_d, u16, mask_d, background, up_d, costs,
                    table, nframe, P, npix, model, nm)
        else:
            tc._launch_factor(far_d, data_d, u16, mask_d, up_d, costs, table,
                              nframe, P, npix, model, nm)
        return costs, table

    plain = run(None, entry="tike_cost_factor")
    for background in (torch.zeros(npix, device="cuda"), None):
        got = run(background)
        assert torch.equal(_bits(got[0]), _bits(plain[0]))
        assert torch.equal(_bits(got[1]), _bits(plain[1]))
    costs, table = run(b_d)
    again = run(b_d)
    assert torch.equal(_bits(costs), _bits(again[0]))
    assert torch.equal(_bits(table), _bits(again[1]))
    assert np.array_equal(far_d.cpu().numpy(), far)
    square = int(round(np.sqrt(npix)))**2 == npix
    if square:
        det = int(round(np.sqrt(npix)))
        first = torch.empty(nframe, device="cuda")
        _first(far_d, data_d, mask_d, b_d.view(det, det), None, first, nframe,
               P, 1, det, MODEL_ID[model], False, 1.0, nm)
        assert torch.equal(_bits(costs), _bits(first)), (costs, first)
    I32 = tc._intensity32(far_d, nframe, P, npix)
    sel = np.ones(npix, bool) if mask is None else mask
    Ib32 = I32 + np.where(sel, b, np.float32(0))[None]  # (one float32 add)
    assert Ib32.dtype == np.float32
    lp, scale = tc._model_factor(Ib32, data, mask, model)
    table = table.cpu().numpy()
    want = upstream[:, None].astype(np.float64) * lp / nm
    ratio = np.abs(table - want)[:, sel] / (
        np.abs(upstream[:, None]) * scale / nm)[:, sel]
    print(f"background cost factor ({nframe}, {P}, {npix}) {model} "
          f"masked={masked} u16={u16}: costs "
          f"{'= first entry bits, ' if square else ''}table max |err| / "
          f"bound scale {ratio.max():.2e}")
    assert np.all(table[:, ~sel] == 0.0)
    assert np.all(np.isfinite(table))
    assert np.all(np.isfinite(costs.cpu().numpy()))
    assert np.all(ratio <= 1e-6), ratio.max()


# ------------------------------------------------------------ the third entry
# (nframe, npix): npix % 4 of 1, 0, 3, 3; one lane group and several; fewer
# frames than the unroll, a multiple of it and neither
SUMS_CASES = [(1, 169), (5, 256), (37, 1027), (300, 403)]


def _sums(inten_d, data_d, u16, mask_d, b_d, up_d, want_partials, want_bgrad,
          nframe, npix, model, nm):
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    n = lib.tike_background_sums_partials(npix)
    partials = torch.full((n + 2,), 7.0, dtype=torch.float64, device="cuda")
    bgrad = torch.full((npix + 2,), 7.0, device="cuda")
    check(lib.tike_background_sums(
        A.ptr(inten_d), A.ptr(data_d), int(u16), A.ptr(mask_d), A.ptr(b_d),
        A.ptr(up_d), A.ptr(partials[1:]) if want_partials else None,
        A.ptr(bgrad[1:]) if want_bgrad else None, nframe, npix,
        MODEL_ID[model], nm, A.stream_ptr()), "tike_background_sums")
    return partials, bgrad


@pytest.mark.parametrize("model,masked,u16", tc.ENTRY_VARIANTS)
@pytest.mark.parametrize("nframe,npix", SUMS_CASES)
def test_background_sums(nframe, npix, model, masked, u16):
    """bgrad: exactly 0 under the mask; |err| <= 1e-6 sum_f |upstream_f|
    (1 + sqrt(d) / (sqrt(Ib) + 1e-9)) / num_measured (poisson: d / (Ib +
    1e-9)) against the float64 sum with l' at the float32 Ib.  The sum of the
    partials against the float64 cost sum at 1e-6 relative (of the sum of the
    terms' absolute parts, |upstream_f| (Ib + d) or |upstream_f| (Ib +
    d |log Ib|), what the terms are differences of).  Each output alone equals
    what both give; NULL upstream equals ones; two calls give the same bits;
    nothing in front of or behind the outputs is written."""
    import torch
    rng = np.random.default_rng(nframe + npix)
    I32 = rng.uniform(5.0, 60.0, (nframe, npix)).astype(np.float32)
    counts = I32 * rng.uniform(0.1, 0.4, I32.shape)
    mask = None
    if masked:
        mask = rng.random(npix) < 0.75
        mask[rng.integers(npix)] = False
        mask[(rng.integers(npix) + 1) % npix] = True
    if u16:
        data = np.minimum(np.rint(counts), 65535).astype(np.uint16)
        data_d = _u16(data)
    else:
        data = counts.astype(np.float32)
        if masked:
            data[:, ~mask] = np.nan
        data_d = _dev(data)
    upstream = ac.frame_weights(nframe, seed=npix)
    nm = npix if mask is None else int(mask.sum())
    b = _background_for(npix, mask, npix + nframe)
    inten_d, b_d, up_d = _dev(I32), _dev(b), _dev(upstream)
    mask_d = None if mask is None else _dev(mask.astype(np.uint8))
    args = (nframe, npix, model, nm)
    both = _sums(inten_d, data_d, u16, mask_d, b_d, up_d, True, True, *args)
    again = _sums(inten_d, data_d, u16, mask_d, b_d, up_d, True, True, *args)
    only_p = _sums(inten_d, data_d, u16, mask_d, b_d, up_d, True, False, *args)
    only_g = _sums(inten_d, data_d, u16, mask_d, b_d, up_d, False, True, *args)
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])
    assert torch.equal(only_p[0], both[0]) and bool((only_p[1] == 7.0).all())
    assert torch.equal(only_g[1], both[1]) and bool((only_g[0] == 7.0).all())
    for out in both:
        assert float(out[0]) == 7.0 == float(out[-1])
    ones = _sums(inten_d, data_d, u16, mask_d, b_d,
                 torch.ones(nframe, device="cuda"), True, True, *args)
    null = _sums(inten_d, data_d, u16, mask_d, b_d, None, True, True, *args)
    assert torch.equal(ones[0], null[0]) and torch.equal(ones[1], null[1])
    partials = both[0][1:-1].cpu().numpy()
    bgrad = both[1][1:-1].cpu().numpy()
    sel = np.ones(npix, bool) if mask is None else mask
    Ib32 = I32 + np.where(sel, b, np.float32(0))[None]
    assert Ib32.dtype == np.float32
    lp, scale = tc._model_factor(Ib32, data, mask, model)
    up = upstream[:, None].astype(np.float64)
    want = (up * lp).sum(axis=0) / nm
    bound = (np.abs(up) * scale).sum(axis=0) / nm
    ratio = (np.abs(bgrad - want) / bound)[sel]
    clean = np.where(sel, data, 0).astype(np.float64)
    Ib = Ib32.astype(np.float64)
    terms = ac.terms(torch.from_numpy(Ib), torch.from_numpy(clean),
                     model).numpy()
    cost_want = (up * terms)[:, sel].sum() / nm
    parts = np.abs(up) * (Ib + clean * (1 if model == "gaussian" else
                                       np.abs(np.log(Ib + 1e-9))))
    cost_err = abs(partials.sum() - cost_want) / (parts[:, sel].sum() / nm)
    print(f"background sums ({nframe}, {npix}) {model} masked={masked} "
          f"u16={u16}: bgrad max |err| / bound scale {ratio.max():.2e}; cost "
          f"|err| / sum parts {cost_err:.2e}")
    assert np.all(bgrad[~sel] == 0.0)
    assert np.all(np.isfinite(bgrad)) and np.all(np.isfinite(partials))
    assert np.all(ratio <= 1e-6), ratio.max()
    assert cost_err <= 1e-6, cost_err


# ------------------------------------------------------------------ the solver
def _parameters(tp, P, model, mask, epochs=2, cg_iter=2, recover_probe=True,
                step_length=bg.STEP_LENGTH, probe=None):
    det = P["data"].shape[-1]
    eo = tp.ExitWaveOptions(
        measured_pixels=mask if mask is not None else np.ones((det, det), bool),
        noise_model=model)
    return tp.PtychoParameters(
        probe=(P["probe0"] if probe is None else probe).copy(),
        psi=P["psi0"].copy(), scan=P["scan"].copy(),
        algorithm_options=tp.CgradOptions(num_batch=1, cg_iter=cg_iter,
                                          num_iter=epochs,
                                          step_length=step_length,
                                          batch_method="contiguous"),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False)
        if recover_probe else None,
        object_options=tp.ObjectOptions(), exitwave_options=eo)


def _reconstruct(tp, P, data, params, fly, bo):
    N = len(P["scan"])
    return tp.reconstruct(data, params, fly=fly, order=np.arange(N),
                          batches=[np.arange(N)], background_options=bo)


@pytest.mark.parametrize("model,use_mask,update", bg.SOLVER_VARIANTS)
@pytest.mark.parametrize("case", sorted(bg.SOLVER_CASES))
def test_cgrad_vs_float64_model(tp, case, model, use_mask, update):
    """Two epochs of cgrad with background_options, cg_iter 2, det 32, fly 1
    and 2: psi, probe, the background left in the options and the cost
    history against the model's three-block cgrad at RECON_NORMWISE; every
    line-search decision of the model is clear (test_background_cpu.py)."""
    state, P, mask = bg.run_model(case, model, use_mask, update)
    assert min(state["margins"]) >= fs.MIN_MARGIN
    fly = bg.SOLVER_CASES[case][0]["fly"]
    bo = tp.BackgroundOptions(P["b0"].copy(), update=update)
    got = _reconstruct(tp, P, P["data"], _parameters(tp, P, model, mask), fly,
                       bo)
    costs = np.array(got.algorithm_options.costs)
    want_b = state["a"]**2
    sel = np.ones_like(want_b, bool) if mask is None else mask
    b_err = relerr(np.where(sel, bo.background, 0), np.where(sel, want_b, 0))
    print(case, model, use_mask, update,
          f"psi {relerr(got.psi, state['psi']):.2e} probe "
          f"{relerr(got.probe, state['probe']):.2e} background {b_err:.2e} "
          "costs", np.ravel(costs), "vs", np.ravel(state["costs"]))
    np.testing.assert_allclose(costs, np.array(state["costs"]),
                               rtol=RECON_NORMWISE)
    assert relerr(got.psi, state["psi"]) <= RECON_NORMWISE
    assert relerr(got.probe, state["probe"]) <= RECON_NORMWISE
    assert isinstance(bo.background, np.ndarray)
    assert bo.background.dtype == np.float32 and np.all(bo.background >= 0)
    assert b_err <= RECON_NORMWISE
    if not update:
        np.testing.assert_allclose(bo.background, P["b0"], rtol=1e-6)
    elif use_mask:  # nothing pulls on a pixel that is not measured
        np.testing.assert_allclose(bo.background[~mask], P["b0"][~mask],
                                   rtol=1e-6)


@pytest.mark.parametrize("model", ["gaussian", "poisson"])
def test_cgrad_uint16_counts_equal_float32_counts(tp, model):
    P = bg.solver_problem("fly2")
    mask = fs.block_mask(32)
    counts = np.rint(P["data"] * 20).astype(np.uint16)  # (some tens)
    out = []
    for data in (counts, fs.masked(counts.astype(np.float32), mask)):
        bo = tp.BackgroundOptions(20 * P["b0"])
        got = _reconstruct(tp, P, data, _parameters(tp, P, model, mask), 2, bo)
        out.append((got, bo.background))
    (a, ba), (b, bb) = out
    print(f"uint16 vs float32 {model}: psi {relerr(a.psi, b.psi):.2e} probe "
          f"{relerr(a.probe, b.probe):.2e} background {relerr(ba, bb):.2e}")
    assert relerr(a.psi, b.psi) <= 1e-6 and relerr(a.probe, b.probe) <= 1e-6
    assert relerr(ba, bb) <= 1e-6
    np.testing.assert_allclose(a.algorithm_options.costs,
                               b.algorithm_options.costs, rtol=1e-6)


@pytest.mark.parametrize("fly", [1, 2])
def test_cgrad_zero_background_is_the_whole_frames_route(tp, fly, monkeypatch):
    """background_options with a zero background and update=False gives the
    iterates of the same call without it on the whole-frames route
    (`_fly_cost_and_grad`; at fly 1 the call without background_options takes
    the plain route, whose line searches the device decides: it is sent the
    whole-frames way here), to 1e-6 normwise."""
    import importlib
    # (the package exports the solver function under the module's name)
    cg = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    P = bg.solver_problem(f"fly{fly}")
    mask = fs.block_mask(32)
    data = fs.masked(P["data"], mask)
    bo = tp.BackgroundOptions(np.zeros((32, 32), np.float32), update=False)
    with_bo = _reconstruct(tp, P, data, _parameters(tp, P, "gaussian", mask),
                           fly, bo)
    assert np.array_equal(bo.background, np.zeros((32, 32), np.float32))
    if fly == 1:
        # the route a plain minibatch would not take
        monkeypatch.setattr(cg, "PLAIN_ROUTE", False)
    without = _reconstruct(tp, P, data, _parameters(tp, P, "gaussian", mask),
                           fly, None)
    print(f"fly {fly}: psi {relerr(with_bo.psi, without.psi):.2e} probe "
          f"{relerr(with_bo.probe, without.probe):.2e}")
    assert relerr(with_bo.psi, without.psi) <= 1e-6
    assert relerr(with_bo.probe, without.probe) <= 1e-6
    np.testing.assert_allclose(with_bo.algorithm_options.costs,
                               without.algorithm_options.costs, rtol=1e-6)


def test_operator_and_simulate(tp):
    """simulate(background=) adds b to every frame; Ptycho.cost and
    _compute_intensity with a background against the model."""
    import tike_amd.operators as tops
    kw = bg.SOLVER_CASES["fly2"][0]
    P = bg.solver_problem("fly2")
    det, fly = kw["det"], kw["fly"]
    b = P["background"]
    sim = tp.simulate(det, P["probe"], P["scan"], P["psi"], fly=fly,
                      background=b)
    assert_close(sim, P["data"], what="simulate(background=)")
    plain = tp.simulate(det, P["probe"], P["scan"], P["psi"], fly=fly)
    assert_close(sim - plain, np.broadcast_to(b, sim.shape), what="b")
    with tops.Ptycho(det, kw["pw"], nz=kw["obj"], n=kw["obj"]) as op:
        inten, _ = op._compute_intensity(None, P["psi0"], P["scan"],
                                         P["probe0"], fly=fly, background=b)
        assert_close(inten, bg.intensity(P["probe0"], P["scan"], P["psi0"],
                                         det, fly, b), what="intensity + b")
        for model in ("gaussian", "poisson"):
            c = float(op.cost(P["data"], P["psi0"], P["scan"], P["probe0"],
                              model=model, fly=fly, background=b))
            want = bg.cost(model, P["data"], P["psi0"], P["scan"], P["probe0"],
                           det, fly, None, b.astype(np.float64))
            assert abs(c - want) <= OP_NORMWISE * abs(want), (model, c, want)


# ----------------------------------------------------- autograd.cost(background=)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("model", ac.MODELS)
def test_autograd_cost_background(model, masked):
    """The plain fly-2 case of autograd_cost.CASES: costs and the gradients
    with respect to psi, probe, scan and b against `intensity + b` with the
    same loss written in torch, float32 both, at the BARS of
    test_binned_gpu.py; b.grad normwise at 2 * OP_NORMWISE."""
    import torch

    import tike_amd.operators as ops
    from tike_amd import autograd
    kind, shape = ac.CASES[0]
    c = ac.case(kind, shape)
    fly, det = c["fly"], c["det"]
    data, mask, up = ac.counts_of(c, masked)
    b_h = _background_for(det * det, None, 5).reshape(det, det) * 0.2
    data = (data + b_h).astype(np.float32)
    with torch.no_grad():
        I = c["form"].intensity(c["m"]) + torch.from_numpy(
            b_h.astype(np.float64))
        table = ac.table_of(I, torch.from_numpy(
            np.nan_to_num(data).astype(np.float64)),
            None if mask is None else torch.from_numpy(mask), model,
            torch.from_numpy(up))
        want = c["form"].grads(c["m"], table)
    names = ["psi", "probe", "scan"]
    kw = {k: _dev(c["host"][k]).requires_grad_(True) for k in names}
    b_d = _dev(b_h).requires_grad_(True)
    data_d, up_d = _dev(data), _dev(up)
    mask_d = None if mask is None else _dev(mask)
    nm = det * det if mask is None else int(mask.sum())
    wrt = [kw[k] for k in names] + [b_d]
    with ops.Ptycho(**c["operator"]) as op:
        costs = autograd.cost(op, data_d, kw["psi"], kw["probe"], kw["scan"],
                              model=model, measured_pixels=mask_d, fly=fly,
                              background=b_d)
        grads = torch.autograd.grad((costs * up_d).sum(), wrt)
        inten = autograd.intensity(op, kw["psi"], kw["probe"], kw["scan"],
                                   fly=fly) + b_d
        sel = (torch.ones((det, det), dtype=torch.bool, device="cuda")
               if mask_d is None else mask_d)
        zero = torch.zeros_like(inten)
        d = torch.where(sel, data_d, zero)
        terms = ((torch.sqrt(inten) - torch.sqrt(d))**2 if model == "gaussian"
                 else inten - d * torch.log(inten + 1e-9))
        ccosts = torch.where(sel, terms, zero).sum(dim=(1, 2)) / nm
        cgrads = torch.autograd.grad((ccosts * up_d).sum(), wrt)
        # b alone
        alone = torch.autograd.grad((autograd.cost(
            op, data_d, kw["psi"].detach(), kw["probe"].detach(),
            kw["scan"].detach(), model=model, measured_pixels=mask_d, fly=fly,
            background=b_d) * up_d).sum(), [b_d])[0]
    h = lambda x: x.detach().cpu().numpy()
    cerr = np.abs(h(costs) - h(ccosts)) / np.abs(h(ccosts))
    errors = {}
    for name, g, cg in zip(names + ["background"], grads, cgrads):
        g, cg = h(g), h(cg)
        assert np.all(np.isfinite(g)), name
        if name == "scan":
            A = want["A_scan"].numpy()
            live = A > 0
            errors[name] = float((np.abs(g - cg)[live] / A[live]).max())
        else:
            errors[name] = relerr(g, cg)
    print(f"cost(background=) {model} masked={masked}: costs max rel "
          f"{cerr.max():.2e}; "
          + ", ".join(f"{k} {v:.2e}" for k, v in errors.items()))
    assert np.all(np.isfinite(h(costs))) and np.all(cerr <= 2e-5), cerr
    for k, v in errors.items():
        assert v <= dict(BARS, background=2 * OP_NORMWISE)[k], (k, v)
    assert torch.equal(alone, grads[3])
    if masked:
        assert np.all(h(grads[3])[~mask] == 0.0)


# ------------------------------------------------------------- demonstration
def test_demonstration(tp):
    """The GPU reaches the object errors of the model's demonstration
    (test_background_cpu.py: 0.8091 ignored, 0.6554 fitted), with and without
    the fit, within RECON_NORMWISE."""
    D = bg.DEMO
    P = bg.demo_problem()
    pw = D["problem"]["pw"]
    for fit in (False, True):
        want, state = bg.run_demo(fit)
        bo = tp.BackgroundOptions(P["b0"].copy()) if fit else None
        params = _parameters(tp, P, "gaussian", None, epochs=D["epochs"],
                             cg_iter=D["cg_iter"], recover_probe=False,
                             step_length=1.0, probe=P["probe"])
        got = _reconstruct(tp, P, P["data"], params, 1, bo)
        err = bg.object_error(got.psi, P["psi"], P["scan"], pw)
        print(f"demonstration fit={fit}: object error {err:.4f}, model "
              f"{want:.4f}; psi vs model {relerr(got.psi, state['psi']):.2e}")
        assert abs(err - want) <= RECON_NORMWISE * want
