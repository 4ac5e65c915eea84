"""Detector binning without a GPU: the float64 model (tests/binned.py) against
central differences of its own cost and against tests/fly_scan.py at B = 1,
the fftshift identity of the block sum, the ABI, the data-shape rule, every
refusal, the values `binning` may take, and how clearly the model's line
searches are decided on the problem the GPU test compares."""
import ctypes
import inspect

import numpy as np
import pytest

import binned as bn
import fly_scan as fs
from util import OP_NORMWISE, assert_close


# ------------------------------------------------------------------ the model
def _small(fly, B=2, seed=0):
    """A problem small enough for central differences: 4 positions, a 16^2
    far plane, 2 modes."""
    K = dict(obj=40, pw=16, det=16, S=2, B=B, side=2, seed=seed, amp=1.0,
             mix=0.3, dim=0.5)
    return K, bn.problem(fly, **K)


@pytest.mark.parametrize("fly", [1, 2])
@pytest.mark.parametrize("model", ["gaussian", "poisson"])
def test_model_gradient_is_the_derivative_of_its_cost(model, fly):
    """d cost / d Re, Im of object and probe pixels by central differences in
    float64 equals 2 / (frames * num_measured) * the model's gradient (the
    unnormalised adjoint; the cost is the mean over frames of a mean over the
    measured data pixels, real, of a complex variable), with the block mask at
    data resolution and NaN under it."""
    K, P = _small(fly)
    det, B = K["det"], K["B"]
    mask = fs.block_mask(det // B)
    data = fs.masked(P["data"] * 1.3 + 0.2, mask)  # (away from the minimum)
    psi = P["psi0"].astype(np.complex128)
    probe = P["probe0"].astype(np.complex128)
    scan = P["scan"]
    frames = len(scan) // fly * int(mask.sum())  # (times the pixels)
    c = lambda ps, pr: bn.cost(model, data, ps, scan, pr, det, fly, B, mask)
    g_psi = bn.grad_psi(model, data, psi, scan, probe, det, fly, B, mask)
    g_probe = bn.grad_probe(model, data, psi, scan, probe, det, fly, B, mask)
    assert np.all(np.isfinite(g_psi)) and np.all(np.isfinite(g_probe))
    rng = np.random.default_rng(4)
    h = 1e-6
    lo = int(np.floor(scan.min())) + 2
    for _ in range(6):
        y, x = rng.integers(lo, lo + 10, 2)
        for unit in (1.0, 1j):
            e = np.zeros_like(psi)
            e[0, y, x] = unit
            fd = (c(psi + h * e, probe) - c(psi - h * e, probe)) / (2 * h)
            want = 2.0 / frames * (g_psi[0, y, x].real if unit == 1.0
                                   else g_psi[0, y, x].imag)
            assert abs(fd - want) <= 1e-6 * max(abs(want), 1e-3), (
                "psi", y, x, unit, fd, want)
        m, y, x = rng.integers(0, 2), *rng.integers(4, 12, 2)
        for unit in (1.0, 1j):
            e = np.zeros_like(probe)
            e[0, 0, m, y, x] = unit
            fd = (c(psi, probe + h * e) - c(psi, probe - h * e)) / (2 * h)
            g = g_probe[0, 0, m, y, x]
            want = 2.0 / frames * (g.real if unit == 1.0 else g.imag)
            assert abs(fd - want) <= 1e-6 * max(abs(want), 1e-3), (
                "probe", m, y, x, unit, fd, want)


@pytest.mark.parametrize("fly", [1, 3])
@pytest.mark.parametrize("model", ["gaussian", "poisson"])
def test_model_at_binning_1_is_the_fly_scan_model(model, fly):
    K = dict(fs.FIXTURE, fly=fly, nframe=6)
    P = fs.problem(**K)
    det = K["det"]
    mask = fs.block_mask(det)
    data = fs.masked(P["data"], mask)
    far = fs.fwd(P["probe"], P["scan"], P["psi0"], det)
    assert np.array_equal(bn.frame_intensity(far, fly, 1),
                          fs.frame_intensity(far, fly))
    assert np.array_equal(bn.farplane_gradient(model, data, far, fly, 1, mask),
                          fs.farplane_gradient(model, data, far, fly, mask))
    args = (data, P["psi0"], P["scan"], P["probe"], det, fly)
    assert bn.cost(model, *args, 1, mask) == fs.cost(model, *args, mask)
    assert np.array_equal(bn.grad_psi(model, *args, 1, mask),
                          fs.grad_psi(model, *args, mask))
    assert np.array_equal(bn.grad_probe(model, *args, 1, mask),
                          fs.grad_probe(model, *args, mask))
    N = len(P["scan"])
    s1 = dict(psi=P["psi0"].copy(), probe=P["probe0"].copy(), scan=P["scan"],
              costs=[])
    s2 = dict(s1, costs=[])
    s1 = bn.cgrad(s1, data, [np.arange(N)], detector_shape=det, fly=fly,
                  binning=1, model=model, mask=mask)
    s2 = fs.cgrad(s2, data, [np.arange(N)], detector_shape=det, fly=fly,
                  model=model, mask=mask)
    assert np.array_equal(s1["psi"], s2["psi"])
    assert np.array_equal(s1["probe"], s2["probe"])
    assert s1["costs"] == s2["costs"]


@pytest.mark.parametrize("det,B", [(16, 2), (32, 4), (48, 8), (24, 3)])
def test_block_sum_commutes_with_fftshift_for_even_data_width(det, B):
    """fftshift(I) == blocksum(fftshift(fine)) when w = det / B is even: the
    shift by det / 2 = (w / 2) B moves whole blocks, so binning the stored
    (corner-peaked) far plane is binning the centred detector."""
    assert (det // B) % 2 == 0
    fine = np.random.default_rng(det).random((3, det, det))
    stored = bn.block_sum(fine, B)
    centred = bn.block_sum(np.fft.fftshift(fine, axes=(-2, -1)), B)
    assert np.array_equal(np.fft.fftshift(stored, axes=(-2, -1)), centred)
    # ... and not for odd w: the blocks straddle the shift
    odd = np.random.default_rng(1).random((9 * B, 9 * B))
    a = np.fft.fftshift(bn.block_sum(odd, B))
    b = bn.block_sum(np.fft.fftshift(odd), B)
    assert not np.allclose(a, b)


def test_spread_and_table():
    K, P = _small(2)
    det, B, fly = K["det"], K["B"], 2
    far = fs.fwd(P["probe0"], P["scan"], P["psi0"], det)
    mask = fs.block_mask(det // B)
    data = fs.masked(P["data"], mask)
    up = np.array([0.5, -2.0])
    t = bn.cost_factor_table("poisson", data, far, fly, B, mask, up)
    assert t.shape == (2, det, det)
    blocks = t.reshape(2, det // B, B, det // B, B)
    assert np.all(blocks == blocks[:, :, :1, :, :1])
    assert np.all(t[:, ~bn.spread(mask, B)] == 0)
    # the gradient is far * table * num_measured / upstream
    g = bn.farplane_gradient("poisson", data, far, fly, B, mask)
    want = far * np.repeat(t * mask.sum() / up[:, None, None], fly,
                           axis=0)[:, None, None]
    assert_close(g, want, what="gradient from the table")


@pytest.mark.parametrize("fly", bn.SOLVER_FLY)
def test_line_searches_of_the_solver_problem_are_clearly_decided(fly):
    """As tests/test_fly_scan_cpu.py asks of its cases: every comparison of
    the float64 line searches over both epochs is decided by a relative margin
    of at least 1e-3, out of reach of float32 rounding of the costs."""
    for model in ("gaussian", "poisson"):
        state, P, mask = bn.run_model(fly, model)
        margin = min(state["margins"])
        print(fly, model, f"min margin {margin:.2e} over "
              f"{len(state['margins'])} comparisons, costs "
              f"{np.ravel(state['costs'])}")
        assert margin >= bn.MIN_MARGIN, (fly, model, margin)
        assert len(state["costs"]) == 2
        w = bn.SOLVER["det"] // bn.SOLVER["B"]
        assert P["data"].shape == (36 // fly, w, w) and mask.shape == (w, w)
        assert P["probe"].shape[-1] > w  # no window of the data's width holds it


# -------------------------------------------------------------------- the ABI
NAMES = {"tike_binned_farplane_gradient": 16, "tike_binned_cost_factor": 15}


def test_abi_has_the_new_entries():
    """Fails on the parent commit: the symbols do not exist."""
    import tike_amd._lib as L
    header = open(L.HEADER_PATH).read()
    so = ctypes.CDLL(L.LIB_PATH)
    for name, arity in NAMES.items():
        assert name in L.declared_symbols()
        assert f"int {name}(" in header
        assert len(L._PROTOTYPES[name]) == arity
        assert hasattr(so, name)
    assert "binned.hip" in open(
        L.LIB_PATH.replace("libtike_amd.so", "Makefile")).read()


def test_entries_refuse_bad_arguments_before_any_launch():
    import tike_amd._lib as L
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def caller(fn, ok):
        def call(**change):
            args = list(ok)
            for k, v in change.items():
                args[int(k[1:])] = v
            return fn(*args)
        return call

    # farplane data u16 mask intensity costs nframe fly S det binning model
    # apply_gradient unmeasured_scaling num_measured stream
    call = caller(L.lib.tike_binned_farplane_gradient,
                  (p, p, 0, None, None, None, 1, 2, 1, 4, 2, 0, 0, 1.0, 4, None))
    assert call(a0=None) == L.ERR_ARG  # farplane
    assert call(a1=None) == L.ERR_ARG  # data
    assert call(a7=0) == L.ERR_ARG  # fly
    assert call(a8=0) == L.ERR_ARG  # S
    assert call(a9=0) == L.ERR_ARG  # det
    assert call(a10=0) == L.ERR_ARG  # binning < 1
    assert call(a10=-2) == L.ERR_ARG
    assert call(a10=3) == L.ERR_ARG  # 4 % 3 != 0
    assert call(a11=2) == L.ERR_ARG  # model
    assert call(a14=0) == L.ERR_ARG  # num_measured
    assert call(a6=0) == 0  # no frame: no launch
    # binning == 1 forwards: the fly entry's own refusals
    assert call(a10=1, a0=None) == L.ERR_ARG
    assert call(a10=1, a6=0) == 0
    # farplane data u16 mask upstream costs table nframe P npix model
    # num_measured det binning stream
    call = caller(L.lib.tike_binned_cost_factor,
                  (p, p, 0, None, None, None, None, 1, 2, 16, 0, 4, 4, 2, None))
    assert call(a0=None) == L.ERR_ARG
    assert call(a1=None) == L.ERR_ARG
    assert call(a8=0) == L.ERR_ARG  # P
    assert call(a9=15) == L.ERR_ARG  # npix != det * det
    assert call(a10=2) == L.ERR_ARG  # model
    assert call(a11=0) == L.ERR_ARG  # num_measured
    assert call(a13=0) == L.ERR_ARG  # binning < 1
    assert call(a13=3) == L.ERR_ARG  # 4 % 3 != 0
    assert call(a7=-1) == L.ERR_ARG
    assert call(a7=0) == 0
    assert call(a13=1, a7=0) == 0
    assert call(a13=1, a0=None) == L.ERR_ARG


# --------------------------------------------------------- the host interface
def _parameters(tp, scan, pw=16, obj=64, options=None, mask=None, **kw):
    return tp.PtychoParameters(
        probe=np.ones((1, 1, 1, pw, pw), np.complex64),
        psi=np.ones((kw.pop("slices", 1), obj, obj), np.complex64),
        scan=scan,
        algorithm_options=options or tp.CgradOptions(num_batch=1),
        probe_options=tp.ProbeOptions(), object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((pw, pw), bool) if mask is None else mask),
        **kw)


def _scan(n):
    rng = np.random.default_rng(2)
    return (2 + 40 * rng.random((n, 2))).astype(np.float32)


def test_binning_is_a_keyword_of_the_public_interface():
    """Fails on the parent commit: there is no `binning`."""
    import tike_amd.autograd as ag
    import tike_amd.operators as tops
    import tike_amd.ptycho as tp
    for fn in (tp.Reconstruction.__init__, tp.reconstruct,
               tp.reconstruct_multigrid, ag.cost, ag.cost_jvp,
               ag.cost_gauss_newton_product, tops.Ptycho.cost):
        p = inspect.signature(fn).parameters["binning"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1, fn
    for fn in (tp.simulate, tops.Ptycho._compute_intensity):
        assert inspect.signature(fn).parameters["binning"].default == 1
    assert hasattr(tops.Ptycho, "binned_farplane_gradient")


def test_values_binning_may_take():
    import tike_amd.ptycho as tp
    scan = _scan(4)
    data = np.zeros((4, 8, 8), np.float32)
    for bad in (0, -1, 1.5, True, "2", None):
        with pytest.raises(ValueError, match="binning="):
            tp.Reconstruction(data, _parameters(tp, scan), binning=bad)
        with pytest.raises(ValueError, match="binning="):
            tp.reconstruct(data, _parameters(tp, scan), binning=bad)
        with pytest.raises(ValueError, match="binning="):
            tp.simulate(16, np.ones((1, 1, 1, 16, 16), np.complex64), scan,
                        np.ones((1, 64, 64), np.complex64), binning=bad)
    # a binning that does not divide the far-plane width
    for det, B in ((16, 3), (33, 2), (16, 32)):
        with pytest.raises(ValueError, match="does not divide"):
            tp.simulate(det, np.ones((1, 1, 1, 16, 16), np.complex64), scan,
                        np.ones((1, 64, 64), np.complex64), binning=B)
    import tike_amd.autograd as ag

    class Op:
        detector_shape = 16

    for bad in (0, 1.5, True):
        with pytest.raises(ValueError, match="binning="):
            ag.cost(Op(), None, None, None, None, binning=bad)
    with pytest.raises(ValueError, match="does not divide"):
        ag.cost(Op(), None, None, None, None, binning=3)


def test_data_shape_rule():
    import tike_amd.ptycho as tp
    from tike_amd.ptycho.ptycho import _check_data_shape
    scan = _scan(12)
    # a 16^2 probe window over 8^2 data: only with binning
    params = _parameters(tp, scan, pw=16)
    data = np.zeros((12, 8, 8), np.float32)
    _check_data_shape(data, params, binning=2)
    _check_data_shape(data, params, binning=4)
    _check_data_shape(np.zeros((6, 8, 8), np.float32), params, fly=2,
                      binning=2)
    with pytest.raises(ValueError, match="times binning"):
        _check_data_shape(np.zeros((12, 5, 5), np.float32), params, binning=3)
    with pytest.raises(ValueError, match="binning=3"):
        _check_data_shape(np.zeros((12, 5, 5), np.float32), params, binning=3)
    # binning == 1: the reference's rule and message
    with pytest.raises(ValueError, match="The probe width/height must be <= "
                       "the data width/height ."):
        _check_data_shape(data, params)
    with pytest.raises(ValueError, match="The probe width/height must be <= "
                       "the data width/height ."):
        _check_data_shape(data, params, binning=1)
    # a mask with unmeasured pixels is at data resolution
    mask = np.ones((8, 8), bool)
    mask[2, 3] = False
    _check_data_shape(data, _parameters(tp, scan, mask=mask), binning=2)
    fine = np.ones((16, 16), bool)
    fine[2, 3] = False
    with pytest.raises(ValueError, match="measured_pixels shape"):
        _check_data_shape(data, _parameters(tp, scan, mask=fine), binning=2)


def test_every_refusal(monkeypatch):
    import tike_amd.ptycho as tp
    data = np.zeros((12, 8, 8), np.float32)
    scan = _scan(12)

    def refused(match, params=None, **kw):
        with pytest.raises(NotImplementedError, match=match):
            tp.Reconstruction(data, params or _parameters(tp, scan), binning=2,
                              **kw)

    refused("binning=2 with position_options", _parameters(
        tp, scan, position_options=tp.PositionOptions(scan.copy())))
    refused("binning=2 with eigen probes", _parameters(
        tp, scan, eigen_probe=np.ones((1, 1, 1, 16, 16), np.complex64),
        eigen_weights=np.ones((12, 2, 1), np.float32)))
    refused("binning=2 with lstsq_grad",
            _parameters(tp, scan, options=tp.LstsqOptions(num_batch=1),
                        mask=np.ones((8, 8), bool)))
    refused("binning=2 with rpie",
            _parameters(tp, scan, options=tp.RpieOptions(num_batch=1),
                        mask=np.ones((8, 8), bool)))
    refused("binning=2 with dm",
            _parameters(tp, scan, options=tp.DmOptions(num_batch=1),
                        mask=np.ones((8, 8), bool)))
    refused("binning=2 with several slices", _parameters(tp, scan, slices=2))
    refused("binning=2 with local_data", local_data=object())
    # the solver refuses by itself too
    from tike_amd.ptycho.solvers.cgrad import _refuse, _refuse_binning
    _refuse_binning(_parameters(tp, scan), 2)
    _refuse_binning(_parameters(
        tp, scan, position_options=tp.PositionOptions(scan.copy())), 1)
    with pytest.raises(NotImplementedError, match="binning=4 with position"):
        _refuse(_parameters(
            tp, scan, position_options=tp.PositionOptions(scan.copy())), 1,
            binning=4)
    # update_positions_pd of a binned context
    ctx = tp.Reconstruction.__new__(tp.Reconstruction)
    ctx.binning = 2
    with pytest.raises(NotImplementedError,
                       match="binning=2 with update_positions_pd"):
        ctx.update_positions_pd()
    # reconstruct_multigrid
    with pytest.raises(NotImplementedError,
                       match="binning=2 with reconstruct_multigrid"):
        tp.reconstruct_multigrid(data, _parameters(tp, scan), binning=2)
    # reconstruct(num_gpu=N) from a plain process
    with pytest.raises(NotImplementedError, match=r"binning=2 with "
                       r"reconstruct\(num_gpu=2\)"):
        tp.reconstruct(data, _parameters(tp, scan), num_gpu=2, binning=2)
    with pytest.raises(NotImplementedError, match="num_gpu"):
        tp.reconstruct(data, _parameters(tp, scan), num_gpu=(0, 1), binning=2)
    # the forward-mode functions of the differentiable cost
    import tike_amd.autograd as ag
    for fn in (ag.cost_jvp, ag.cost_gauss_newton_product):
        with pytest.raises(NotImplementedError,
                           match=fn.__name__ + " with binning=2"):
            fn(None, None, None, None, None, binning=2)
    # the ranks of a torch.distributed job
    from tike_amd.ptycho import _spawn
    monkeypatch.setattr(_spawn, "world_size", lambda: 2)
    refused("binning=2 with the ranks of a torch.distributed job")
