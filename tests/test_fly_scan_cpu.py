"""Fly scans without a GPU: the float64 model (tests/fly_scan.py) against the
reference's own results (tests/golden/fly_scan.npz) and against
tests/cgrad_models.py at fly = 1, the frame-order expansion, the data-shape
rule, every refusal, the ABI, and how clearly the model's line searches are
decided on the problems the GPU test compares."""
import inspect

import numpy as np
import pytest

import cgrad_models as cm
import fly_scan as fs
from util import OP_NORMWISE, assert_close, relerr


@pytest.fixture(scope="module")
def fx(golden):
    return golden("fly_scan.npz")


# ------------------------------------------------- the model vs the reference
def test_model_matches_the_reference_fixture(fx):
    K = fs.FIXTURE
    fly, det = K["fly"], K["det"]
    P = fs.problem(**K)
    # the file's inputs are the seeded problem's
    assert np.array_equal(fx["scan"], P["scan"])
    assert np.array_equal(fx["psi"], P["psi0"])
    assert np.array_equal(fx["probe"], P["probe"])
    scan, psi, probe, data = fx["scan"], fx["psi"], fx["probe"], fx["data"]
    mask = fx["mask"]
    assert fx["simulated"].shape == (K["nframe"], det, det)
    assert_close(fs.simulate(det, probe, scan, P["psi"], fly), fx["simulated"],
                 what="simulate(fly=3)")
    far = fs.fwd(probe, scan, psi, det)
    inten = fs.frame_intensity(far, fly)
    assert_close(inten, fx["intensity"], what="_compute_intensity(fly=3)")
    nan_data = fs.masked(data, mask)
    for model in ("gaussian", "poisson"):
        for tag, m, d in (("", None, data), ("_masked", mask, nan_data)):
            c = fs.cost(model, d, psi, scan, probe, det, fly, m)
            want = float(fx[f"cost_{model}{tag}"])
            assert abs(c - want) <= OP_NORMWISE * abs(want), (model, tag, c,
                                                              want)
            g = fs.farplane_gradient(model, d, far, fly, m)
            assert np.all(np.isfinite(g))
            assert_close(g[:fly], fx[f"grad_far_{model}{tag}"],
                         what=f"far-plane gradient {model}{tag}")
            assert_close(fs.grad_probe(model, d, psi, scan, probe, det, fly, m),
                         fx[f"grad_probe_{model}{tag}"],
                         what=f"probe gradient {model}{tag}")
            key = f"grad_psi_{model}{tag}"
            if key in fx.files:
                assert_close(fs.grad_psi(model, d, psi, scan, probe, det, fly,
                                         m), fx[key],
                             what=f"object gradient {model}{tag}")
    assert "grad_psi_gaussian_masked" in fx.files
    assert "grad_psi_poisson" in fx.files


@pytest.mark.parametrize("model", ["gaussian", "poisson"])
def test_model_at_fly_1_is_the_cgrad_model(model):
    K = dict(fs.FIXTURE, fly=1, nframe=9)
    P = fs.problem(**K)
    det = K["det"]
    mask = fs.block_mask(det)
    data = fs.masked(P["data"], mask)
    args = (data, P["psi0"], P["scan"], P["probe"], det)
    a = fs.cost(model, *args, 1, mask)
    b = cm.cost(model, *args, mask)
    assert abs(a - b) <= OP_NORMWISE * abs(b)
    assert_close(fs.grad_psi(model, *args, 1, mask),
                 cm.grad_psi(model, *args, mask), what="object gradient")
    assert_close(fs.grad_probe(model, *args, 1, mask),
                 cm.grad_probe(model, *args, mask), what="probe gradient")
    # one epoch of each solver model
    N = len(P["scan"])
    s1 = dict(psi=P["psi0"].copy(), probe=P["probe0"].copy(), scan=P["scan"],
              costs=[])
    s2 = dict(s1, costs=[])
    s1 = fs.cgrad(s1, data, [np.arange(N)], detector_shape=det, fly=1,
                  model=model, mask=mask)
    s2 = cm.cgrad(s2, data, [np.arange(N)], detector_shape=det, model=model,
                  mask=mask)
    assert min(s1["margins"]) > 1e-4  # (both models decide alike)
    assert_close(s1["psi"], s2["psi"], normwise=1e-4, maxabs=1e-3, what="psi")
    assert_close(s1["probe"], s2["probe"], normwise=1e-4, maxabs=1e-3,
                 what="probe")
    np.testing.assert_allclose(s1["costs"], s2["costs"], rtol=1e-5)


@pytest.mark.parametrize("case", sorted(fs.SOLVER_CASES))
def test_line_searches_of_the_solver_cases_are_clearly_decided(case):
    """Every comparison `cost(x + step d) <= cost(x)` of the float64 model,
    over both epochs of every variant the GPU test runs, is decided by a
    relative margin of at least 1e-3: float32 rounding of the product's costs
    (~1e-7 relative) cannot turn a decision."""
    for variant in fs.SOLVER_VARIANTS:
        state, _, _ = fs.run_model(case, *variant)
        margin = min(state["margins"])
        print(case, variant, f"min margin {margin:.2e} over "
              f"{len(state['margins'])} comparisons, costs "
              f"{np.ravel(state['costs'])}")
        assert margin >= fs.MIN_MARGIN, (case, variant, margin)
        assert len(state["costs"]) == 2


# ------------------------------------------------------------ frames, orders
def test_frame_order_expansion():
    from tike_amd.ptycho.ptycho import (collapse_to_frames, expand_frames,
                                        frame_centroids, rank_share)
    fly, F = 3, 11
    rng = np.random.default_rng(0)
    frame_order = rng.permutation(F)
    frame_batches = [np.arange(0, 4), np.arange(4, 4), np.arange(4, 11)]
    order, batches = expand_frames(frame_order, frame_batches, fly)
    N = F * fly
    assert np.array_equal(np.sort(order), np.arange(N))
    rows = order.reshape(F, fly)
    assert np.array_equal(rows[:, 0], frame_order * fly)
    assert np.array_equal(rows, rows[:, :1] + np.arange(fly))
    assert np.array_equal(np.concatenate(batches), np.arange(N))
    assert [len(b) for b in batches] == [12, 0, 21]
    o2, b2 = collapse_to_frames(order, batches, fly)
    assert np.array_equal(o2, frame_order)
    assert all(np.array_equal(x, y) for x, y in zip(b2, frame_batches))
    # ranks share frames: sizes that do not divide evenly, empty shares
    world = 4
    seen = []
    for rank in range(world):
        local, local_batches = rank_share(frame_order,
                                          [np.arange(0, 3), np.arange(3, 11)],
                                          world, rank)
        lo, lb = expand_frames(local, local_batches, fly)
        assert len(lo) == fly * len(local)
        assert np.array_equal(lo.reshape(-1, fly),
                              lo.reshape(-1, fly)[:, :1] + np.arange(fly))
        assert np.array_equal(np.concatenate(lb) if len(lo) else
                              np.zeros(0, int), np.arange(len(lo)))
        assert all(len(b) % fly == 0 for b in lb)
        seen.append(lo)
        if rank == 3:
            assert len(lb[0]) == 0  # 3 frames over 4 ranks
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(N))
    # centroids
    scan = rng.random((N, 2)).astype(np.float32)
    assert np.allclose(frame_centroids(scan, fly)[2], scan[6:9].mean(axis=0))
    # injected orders that split or reorder a frame are refused
    bad = order.copy()
    bad[[0, 1]] = bad[[1, 0]]
    with pytest.raises(ValueError, match="consecutively"):
        collapse_to_frames(bad, batches, fly)
    with pytest.raises(ValueError, match="whole frames"):
        collapse_to_frames(order, [np.arange(0, 4), np.arange(4, N)], fly)
    shifted = (order + 1) % N
    with pytest.raises(ValueError):
        collapse_to_frames(shifted, batches, fly)


def _parameters(tp, scan, pw=16, obj=64, options=None, **kw):
    rng = np.random.default_rng(1)
    return tp.PtychoParameters(
        probe=np.ones((1, 1, 1, pw, pw), np.complex64),
        psi=np.ones((kw.pop("slices", 1), obj, obj), np.complex64),
        scan=scan,
        algorithm_options=options or tp.CgradOptions(num_batch=1),
        probe_options=tp.ProbeOptions(), object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((pw, pw), bool)), **kw)


def _scan(n):
    rng = np.random.default_rng(2)
    return (2 + 40 * rng.random((n, 2))).astype(np.float32)


def test_data_shape_rule():
    import tike_amd.ptycho as tp
    from tike_amd.ptycho.ptycho import _check_data_shape
    params = _parameters(tp, _scan(12))
    _check_data_shape(np.zeros((6, 16, 16), np.float32), params, fly=2)
    _check_data_shape(np.zeros((12, 16, 16), np.float32), params)
    with pytest.raises(ValueError, match="fly=2"):
        _check_data_shape(np.zeros((5, 16, 16), np.float32), params, fly=2)
    with pytest.raises(ValueError, match="fly=2"):
        _check_data_shape(np.zeros((12, 16, 16), np.float32), params, fly=2)
    # fly == 1: the reference's rule and message
    with pytest.raises(ValueError,
                       match="They should have the same leading dimension"):
        _check_data_shape(np.zeros((6, 16, 16), np.float32), params)
    with pytest.raises(ValueError,
                       match="They should have the same leading dimension"):
        _check_data_shape(np.zeros((6, 16, 16), np.float32), params, fly=1)


def test_fly_is_a_keyword_of_the_public_interface():
    """Fails on the parent commit: there is no `fly`."""
    import tike_amd.ptycho as tp
    for fn in (tp.Reconstruction.__init__, tp.reconstruct):
        p = inspect.signature(fn).parameters["fly"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1
    assert "fly" not in [f for f in vars(_parameters(tp, _scan(4)))]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="fly="):
            tp.Reconstruction(np.zeros((4, 16, 16), np.float32),
                              _parameters(tp, _scan(4)), fly=bad)


def test_every_refusal():
    import tike_amd.ptycho as tp
    data = np.zeros((4, 16, 16), np.float32)
    scan = _scan(12)

    def refused(match, params=None, **kw):
        with pytest.raises(NotImplementedError, match=match):
            tp.Reconstruction(data, params or _parameters(tp, scan), fly=3,
                              **kw)

    refused("fly=3 with position_options", _parameters(
        tp, scan, position_options=tp.PositionOptions(scan.copy())))
    refused("fly=3 with eigen probes", _parameters(
        tp, scan, eigen_probe=np.ones((1, 1, 1, 16, 16), np.complex64),
        eigen_weights=np.ones((12, 2, 1), np.float32)))
    refused("fly=3 with lstsq_grad",
            _parameters(tp, scan, options=tp.LstsqOptions(num_batch=1)))
    refused("fly=3 with rpie",
            _parameters(tp, scan, options=tp.RpieOptions(num_batch=1)))
    refused("fly=3 with several slices", _parameters(tp, scan, slices=2))
    # the solver refuses by itself too
    from tike_amd.ptycho.solvers.cgrad import _refuse_fly
    _refuse_fly(_parameters(tp, scan), 3)
    _refuse_fly(_parameters(
        tp, scan, position_options=tp.PositionOptions(scan.copy())), 1)
    with pytest.raises(NotImplementedError, match="position_options"):
        _refuse_fly(_parameters(
            tp, scan, position_options=tp.PositionOptions(scan.copy())), 3)
    # update_positions_pd of a fly context
    ctx = tp.Reconstruction.__new__(tp.Reconstruction)
    ctx.fly = 3
    with pytest.raises(NotImplementedError,
                       match="fly=3 with update_positions_pd"):
        ctx.update_positions_pd()
    # reconstruct(num_gpu=N) from a plain process
    with pytest.raises(NotImplementedError, match=r"fly=3 with reconstruct\("
                       r"num_gpu=2\)"):
        tp.reconstruct(data, _parameters(tp, scan), num_gpu=2, fly=3)
    with pytest.raises(NotImplementedError, match="num_gpu"):
        tp.reconstruct(data, _parameters(tp, scan), num_gpu=(0, 1), fly=3)


# ------------------------------------------------------------------- the ABI
def test_abi_has_the_new_entry():
    """Fails on the parent commit: the symbol does not exist."""
    import ctypes

    import tike_amd._lib as L
    name = "tike_fly_farplane_gradient"
    assert name in L.declared_symbols()
    assert len(L._PROTOTYPES[name]) == 15
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert L.ABI_VERSION >= 17
    assert "fly.hip" in open(
        L.LIB_PATH.replace("libtike_amd.so", "Makefile")).read()
    # argument checks come before any launch: no GPU needed
    fn = L.lib.tike_fly_farplane_gradient
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = (p, p, 0, None, None, None, 1, 2, 1, 2, 0, 0, 1.0, 4, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return fn(*args)

    assert call(a0=None) == L.ERR_ARG  # farplane
    assert call(a1=None) == L.ERR_ARG  # data
    assert call(a7=0) == L.ERR_ARG  # fly
    assert call(a8=0) == L.ERR_ARG  # S
    assert call(a10=2) == L.ERR_ARG  # model
    assert call(a6=0) == 0  # no frame: no launch
