"""Near-field ptychography without a GPU: the float64 model (tests/nearfield.py)
against itself -- adjointness, finite differences, the two passes of the
transform -- and the host side of the interface: options, refusals, the ABI."""
import numpy as np
import pytest
import scipy.fft

import fly_scan as fs
import nearfield as nf


def _small(det=16, S=2, fly=2, nframe=4, seed=5):
    P = nf.problem(det, S, fly, nframe, seed, step=2.0)
    rng = np.random.default_rng(seed)
    inten = nf.simulate(det, P["probe"], P["scan"], P["psi"], fly, P["H"])
    data = rng.poisson(30 * inten) / 30.0
    mask = np.ones((det, det), bool)
    mask[det // 2 - 1:det // 2 + 1, :] = False
    mask[:, 3] = False
    return P, data, mask


# ------------------------------------------------------------------ the model
def test_dot_product_of_the_operator_and_its_adjoint():
    """<A x, y> = <x, A^H y> to 1e-12, in the object and in the probe."""
    P, _, _ = _small()
    det, rng = 16, np.random.default_rng(0)
    psi = P["psi"].astype(np.complex128)
    probe = P["probe"].astype(np.complex128)
    scan = P["scan"]
    N, S = len(scan), probe.shape[2]
    y = rng.standard_normal((N, 1, S, det, det)) + 1j * rng.standard_normal(
        (N, 1, S, det, det))
    x = rng.standard_normal(psi.shape) + 1j * rng.standard_normal(psi.shape)
    lhs = np.vdot(y, nf.fwd(probe, scan, x, det, P["H"]))
    rhs = np.vdot(nf.adj(y, probe, scan, psi, P["H"])[0], x)
    print("object", abs(lhs - rhs) / abs(lhs))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    q = rng.standard_normal(probe.shape) + 1j * rng.standard_normal(probe.shape)
    lhs = np.vdot(y, nf.fwd(q, scan, psi, det, P["H"]))
    rhs = np.vdot(nf.adj(y, probe, scan, psi, P["H"])[1].sum(axis=0), q[0])
    print("probe", abs(lhs - rhs) / abs(lhs))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    # the propagator alone
    u = rng.standard_normal((3, det, det)) + 1j * rng.standard_normal(
        (3, det, det))
    v = rng.standard_normal((3, det, det)) + 1j * rng.standard_normal(
        (3, det, det))
    lhs = np.vdot(v, nf.propagate(u, P["H"]))
    rhs = np.vdot(nf.propagate(v, P["H"], adjoint=True), u)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("model", nf.MODELS)
def test_gradients_against_central_finite_differences(model, masked):
    """d cost / d Re, Im of object and probe pixels is 2 Re, 2 Im of the
    gradient over (measured pixels x frames); the scan's is
    `autograd_gradients`' directly."""
    P, data, mask = _small()
    mask = mask if masked else None
    d = fs.masked(data, mask).astype(np.float64) if masked else data
    det, fly, H = 16, 2, P["H"]
    psi = P["psi"].astype(np.complex128)
    probe = P["probe"].astype(np.complex128)
    scan = P["scan"]
    G = nf.autograd_gradients(model, d, psi, scan, probe, det, fly, H, mask)
    c = lambda **kw: nf.cost(model, d, kw.get("psi", psi),
                             kw.get("scan", scan), kw.get("probe", probe),
                             det, fly, H, mask)
    h = 1e-5
    rng = np.random.default_rng(3)
    lo = int(np.floor(scan.min())) + 2
    for _ in range(4):
        y, x = rng.integers(lo, lo + det - 4, 2)
        for unit in (1.0, 1j):
            e = np.zeros_like(psi)
            e[0, y, x] = unit
            fd = (c(psi=psi + h * e) - c(psi=psi - h * e)) / (2 * h)
            want = (G["psi"][0, y, x].real if unit == 1.0 else
                    G["psi"][0, y, x].imag)
            assert abs(fd - want) <= 1e-6 * max(abs(want), 1e-6), (fd, want)
        s, y, x = rng.integers(0, 2), *rng.integers(0, det, 2)
        for unit in (1.0, 1j):
            e = np.zeros_like(probe)
            e[0, 0, s, y, x] = unit
            fd = (c(probe=probe + h * e) - c(probe=probe - h * e)) / (2 * h)
            want = (G["probe"][0, 0, s, y, x].real if unit == 1.0 else
                    G["probe"][0, 0, s, y, x].imag)
            assert abs(fd - want) <= 1e-6 * max(abs(want), 1e-6), (fd, want)
    # positions: steps that stay inside a pixel (the integer part is
    # constant).  The gather's weights are float32 (as the kernels' are): a
    # difference over 2 hs carries up to 4 u / hs of the absolute-term sum A,
    # u = 2^-24; the truncation of the central difference is O(hs^2) of it
    frac = scan - np.floor(scan)
    hs = 1e-3
    bound = 4 * 2.0**-24 / hs + 10 * hs**2
    for n in range(len(scan)):
        for axis in (0, 1):
            if not hs < frac[n, axis] < 1 - hs:
                continue
            e = np.zeros_like(scan, dtype=np.float64)
            e[n, axis] = hs
            # (float32 positions: the step must be representable)
            up = (scan.astype(np.float64) + e).astype(np.float32)
            dn = (scan.astype(np.float64) - e).astype(np.float32)
            step = float(up[n, axis]) - float(dn[n, axis])
            fd = (c(scan=up) - c(scan=dn)) / step
            assert abs(fd - G["scan"][n, axis]) <= bound * G["A"][n, axis], (
                n, axis, fd, G["scan"][n, axis])


@pytest.mark.parametrize("N", [128, 256])
def test_two_pass_model_is_the_transform(N):
    """pass2(pass1(x)) is the unnormalised transform, either direction: what
    holds the entry's hand-off to the model."""
    rng = np.random.default_rng(N)
    x = rng.standard_normal((2, N, N)) + 1j * rng.standard_normal((2, N, N))
    want = scipy.fft.fft2(x)
    assert np.abs(nf.pass2(nf.pass1(x)) - want).max() <= 1e-12 * np.abs(
        want).max()
    want = scipy.fft.ifft2(x, norm="forward")
    got = nf.pass2(nf.pass1(x, inverse=True), inverse=True)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_entry_model_is_the_chain_of_the_model():
    """`entry` on the model's own hand-off gives the model's intensity, costs
    and, finished by the adjoint's remaining passes, the plane gradient."""
    det, S, fly = 128, 2, 2
    P = nf.problem(det, S, fly, 2, seed=1)
    rng = np.random.default_rng(1)
    near = nf.exit_waves(P["probe"], P["scan"], P["psi"], det)
    Hc = P["H"].astype(np.complex128)
    spectrum = scipy.fft.fft2(near) * Hc / (det * det)
    work = nf.pass1(spectrum, inverse=True)
    inten = nf.simulate(det, P["probe"], P["scan"], P["psi"], fly, P["H"])
    data = rng.poisson(20 * inten) / 20.0
    mask = np.ones((det, det), bool)
    mask[60:63] = False
    R = nf.entry(work, data, "poisson", fly, S, mask, None, scale=float(
        mask.sum()))
    assert np.abs(R["intensity"] - inten).max() <= 1e-12 * inten.max()
    np.testing.assert_allclose(R["costs"], fs.cost_each("poisson", data, inten,
                                                        mask), rtol=1e-12)
    g = nf.plane_gradient("poisson", data, P["psi"], P["scan"], P["probe"],
                          det, fly, P["H"], mask)[:, 0]
    got = scipy.fft.ifft2(nf.pass2(R["out"]) * Hc.conj(), norm="forward") / (
        det * det)
    want = nf.propagate(g, P["H"], adjoint=True)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_well_conditioned_problem_and_solver_margins():
    """The problem of the GPU solver test: every comparison of the float64
    line searches is decided by a clear relative margin, the cost falls."""
    for fly in (1, 2):
        state, P = nf.run_model(fly)
        print(fly, f"{min(state['margins']):.2e}", np.ravel(state["costs"]))
        assert min(state["margins"]) >= 1e-4
        costs = np.ravel(state["costs"])
        assert costs[1] < costs[0]


# --------------------------------------------------------- the host interface
def test_from_geometry_is_the_fresnel_spectrum_propagator():
    import tike_amd.ptycho as tp
    from tike_amd.operators.fresnelspectprop import fresnel_spectrum_propagator
    det, px, z, lam = 32, 50e-9, 2e-4, 1.2e-10
    o = tp.NearFieldOptions.from_geometry(det, px, z, lam)
    want = fresnel_spectrum_propagator((det, det), (det * px, det * px), z, lam)
    assert o.propagator.dtype == np.complex64
    assert o.propagator.shape == (det, det)
    np.testing.assert_array_equal(o.propagator, want)
    np.testing.assert_allclose(np.abs(o.propagator), 1, rtol=1e-6)


def test_nearfield_is_part_of_the_public_interface():
    """Fails on the parent commit: there is no `nearfield`."""
    import dataclasses
    import inspect

    import tike_amd.autograd as ag
    import tike_amd.operators as tops
    import tike_amd.ptycho as tp
    assert "NearFieldOptions" in tp.__all__
    assert [f.name for f in dataclasses.fields(tp.NearFieldOptions)] == [
        "propagator"]
    for fn in (tp.Reconstruction.__init__, tp.reconstruct,
               tp.reconstruct_multigrid):
        p = inspect.signature(fn).parameters["nearfield_options"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for fn in (ag.cost, tops.Ptycho.cost):
        p = inspect.signature(fn).parameters["nearfield"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for fn in (tp.simulate, tops.Ptycho._compute_intensity):
        assert inspect.signature(fn).parameters["nearfield"].default is None
    for fn in (ag.cost_jvp, ag.cost_gauss_newton_product):
        assert "nearfield" not in inspect.signature(fn).parameters


def test_abi_prototypes_are_present():
    import tike_amd._lib as L
    assert len(L._PROTOTYPES["tike_nearfield_plane_gradient"]) == 18
    assert len(L._PROTOTYPES["tike_nearfield_cost_partials"]) == 1
    for name in ("tike_nearfield_plane_gradient",
                 "tike_nearfield_cost_partials"):
        assert hasattr(L.lib, name)
        assert name in L.declared_symbols()
    assert L.lib.tike_abi_version() == L.ABI_VERSION == 25
    # host only: the float64 partials of the costs of n frames
    assert L.lib.tike_nearfield_cost_partials(5) >= 5 * 16
    assert L.lib.tike_nearfield_cost_partials(0) == 0
    assert L.lib.tike_nearfield_cost_partials(-1) < 0


def test_routes():
    from tike_amd.operators import nearfield as NF
    assert NF.route(128, 128, 8, True) == "entry"
    assert NF.route(256, 256, 1, True) == "entry"
    assert NF.route(256, 256, 9, True) == "general"
    assert NF.route(512, 512, 4, True) == "chain"
    assert NF.route(512, 512, 5, True) == "general"
    assert NF.route(64, 64, 1, True) == "general"
    assert NF.route(256, 256, 1, False) == "general"
    assert NF.route(512, 512, 1, False) == "general"
    with pytest.raises(ValueError, match="probe window = detector"):
        NF.route(64, 128, 1, True)


def test_option_validation():
    from tike_amd.ptycho import nearfield as N
    H = nf.propagator(16)
    got = N.checked_propagator(H, 16)
    assert got.dtype == np.complex64 and got.shape == (16, 16)
    np.testing.assert_array_equal(got, H)  # used as given
    for bad, match in ((nf.propagator(8), "has shape"),
                       (H[None], "has shape"),
                       (H[:, :8], "has shape"),
                       (H.astype(np.complex128), "expected complex64"),
                       (np.abs(H), "expected complex64"),
                       (H * np.float32("nan"), "must be finite"),
                       (H * np.float32("inf"), "must be finite")):
        with pytest.raises(ValueError, match=match):
            N.checked_propagator(bad, 16)
    import torch
    t = torch.from_numpy(H.copy()).requires_grad_(True)
    with pytest.raises(ValueError, match="requires a gradient"):
        N.checked_propagator(t, 16)


def test_every_refusal(monkeypatch):
    import tike_amd.autograd as ag
    import tike_amd.ptycho as tp
    from test_background_cpu import _parameters, _scan
    data = np.zeros((12, 16, 16), np.float32)
    scan = _scan(12)
    H = nf.propagator(16)
    good = lambda: tp.NearFieldOptions(H.copy())

    def refused(match, params=None, no=None, error=NotImplementedError, **kw):
        with pytest.raises(error, match=match):
            tp.Reconstruction(kw.pop("data", data),
                              params or _parameters(tp, scan),
                              nearfield_options=good() if no is None else no,
                              **kw)

    for options in (tp.LstsqOptions, tp.RpieOptions, tp.DmOptions):
        refused(f"nearfield_options with {options(num_batch=1).name}",
                _parameters(tp, scan, options=options(num_batch=1)))
    refused("nearfield_options with binning=2",
            data=np.zeros((12, 8, 8), np.float32), binning=2)
    refused("nearfield_options with background_options",
            background_options=tp.BackgroundOptions(
                np.zeros((16, 16), np.float32)))
    from blur import first_guess
    refused("nearfield_options with blur_options",
            blur_options=tp.BlurOptions(first_guess()))
    refused("nearfield_options with several slices",
            _parameters(tp, scan, slices=2))
    refused("nearfield_options with eigen probes", _parameters(
        tp, scan, eigen_probe=np.ones((1, 1, 1, 16, 16), np.complex64),
        eigen_weights=np.ones((12, 2, 1), np.float32)))
    refused("nearfield_options with position_options", _parameters(
        tp, scan, position_options=tp.PositionOptions(scan.copy())))
    refused("nearfield_options with data_on_host", data_on_host=True)
    refused("nearfield_options with local_data", local_data=object())
    refused("nearfield_options with probe window 8 != detector 16",
            _parameters(tp, scan, pw=8, mask=np.ones((16, 16), bool)))
    # the wrong shape, dtype or value
    refused("has shape", no=tp.NearFieldOptions(nf.propagator(8)),
            error=ValueError)
    refused("expected complex64",
            no=tp.NearFieldOptions(H.astype(np.complex128)), error=ValueError)
    refused("must be finite", no=tp.NearFieldOptions(H * np.float32("nan")),
            error=ValueError)
    refused("must be a tike_amd.ptycho.NearFieldOptions", no=H,
            error=TypeError)
    # update_positions_pd of a near-field context
    ctx = tp.Reconstruction.__new__(tp.Reconstruction)
    from tike_amd.operators.detector import Detector
    ctx._detector = Detector("nearfield", 1, H)
    with pytest.raises(NotImplementedError,
                       match="nearfield_options with update_positions_pd"):
        ctx.update_positions_pd()
    # reconstruct_multigrid; reconstruct(num_gpu=N) from a plain process
    with pytest.raises(NotImplementedError,
                       match="nearfield_options with reconstruct_multigrid"):
        tp.reconstruct_multigrid(data, _parameters(tp, scan),
                                 nearfield_options=good())
    with pytest.raises(NotImplementedError, match=r"nearfield_options with "
                       r"reconstruct\(num_gpu=2\)"):
        tp.reconstruct(data, _parameters(tp, scan), num_gpu=2,
                       nearfield_options=good())
    # simulate
    probe = np.ones((1, 1, 1, 16, 16), np.complex64)
    one = np.ones((1, 64, 64), np.complex64)
    with pytest.raises(NotImplementedError, match="nearfield with binning=2"):
        tp.simulate(16, probe, scan, one, binning=2, nearfield=H)
    with pytest.raises(NotImplementedError,
                       match="nearfield with a background"):
        tp.simulate(16, probe, scan, one, nearfield=H,
                    background=np.zeros((16, 16), np.float32))
    with pytest.raises(NotImplementedError, match="nearfield with a blur"):
        tp.simulate(16, probe, scan, one, nearfield=H, blur=first_guess())
    with pytest.raises(NotImplementedError,
                       match="nearfield with several slices"):
        tp.simulate(16, probe, scan, np.ones((2, 64, 64), np.complex64),
                    nearfield=H)
    with pytest.raises(NotImplementedError,
                       match="nearfield with eigen probes"):
        tp.simulate(16, probe, scan, one, nearfield=H,
                    eigen_weights=np.ones((12, 1, 1), np.float32))
    with pytest.raises(NotImplementedError,
                       match="nearfield with probe window 8 != detector 16"):
        tp.simulate(16, probe[..., :8, :8], scan, one, nearfield=H)
    with pytest.raises(ValueError, match="nearfield has shape"):
        tp.simulate(16, probe, scan, one, nearfield=nf.propagator(8))
    # the differentiable cost

    class Op:
        detector_shape = 16
        probe_shape = 16

    import torch
    t = torch.from_numpy(H.copy())
    psi = torch.ones((1, 64, 64), dtype=torch.complex64)
    check = lambda *a: ag._checked_nearfield("cost", Op(), *a)
    with pytest.raises(NotImplementedError, match="requires a gradient"):
        check(t.clone().requires_grad_(True), psi, None, None, 1, None, None)
    with pytest.raises(NotImplementedError,
                       match="nearfield with eigen probes"):
        check(t, psi, None, torch.ones(12, 1, 1), 1, None, None)
    with pytest.raises(NotImplementedError,
                       match="nearfield with several slices"):
        check(t, torch.ones((2, 64, 64), dtype=torch.complex64), None, None, 1,
              None, None)
    with pytest.raises(NotImplementedError, match="nearfield with binning=2"):
        check(t, psi, None, None, 2, None, None)
    with pytest.raises(NotImplementedError,
                       match="nearfield with a background"):
        check(t, psi, None, None, 1, torch.zeros(16, 16), None)
    with pytest.raises(NotImplementedError, match="nearfield with a blur"):
        check(t, psi, None, None, 1, None, torch.ones(3, 3))
    with pytest.raises(TypeError, match="nearfield must be a torch"):
        check(H, psi, None, None, 1, None, None)
    with pytest.raises(TypeError, match="must be torch.complex64"):
        check(t.to(torch.complex128), psi, None, None, 1, None, None)
    with pytest.raises(ValueError, match=r"nearfield must be \(16, 16\)"):
        check(t[:8, :8], psi, None, None, 1, None, None)
    Op.probe_shape = 8
    with pytest.raises(NotImplementedError, match="probe window 8"):
        check(t, psi, None, None, 1, None, None)
    Op.probe_shape = 16
    with pytest.raises(TypeError, match="no CPU fallback"):
        check(t, psi, None, None, 1, None, None)
    # the ranks of a torch.distributed job
    from tike_amd.ptycho import _spawn
    monkeypatch.setattr(_spawn, "world_size", lambda: 2)
    refused("nearfield_options with the ranks of a torch.distributed job")
