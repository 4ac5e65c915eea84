"""Far-field blur without a GPU: the float64 model (tests/blur.py) against
finite differences and its own adjoint, the chain of the kernel's
parametrisation, option validation, the refusals and the ABI prototypes."""
import numpy as np
import pytest

import blur as bl
import fly_scan as fs

MODELS = ("gaussian", "poisson")


def _fd_close(f, x, dx, got, h=1e-6, rtol=1e-7):
    """A central difference of f at x along dx against `got`: rtol (the
    difference's own third-order term at these sizes) plus the rounding of the
    two float64 values it subtracts, 8 x 2^-52 |f| / h."""
    fd = (f(x + h * dx) - f(x - h * dx)) / (2 * h)
    tol = rtol * max(abs(fd), abs(got)) + 8 * 2.0**-52 * abs(f(x)) / h
    assert abs(fd - got) <= tol, (fd, got, tol)


def _frames(nframe, det, k, seed, masked):
    rng = np.random.default_rng(seed)
    inten = rng.uniform(2.0, 30.0, (nframe, det, det))
    K = bl.gaussian_kernel(k, 0.9).astype(np.float64) * rng.uniform(
        0.5, 1.5, (k, k))
    K /= K.sum()
    data = rng.poisson(bl.blur(K, inten)).astype(np.float64) + 1.0
    mask = fs.block_mask(det) if masked else None
    if masked:
        data[:, ~mask] = np.nan
    up = rng.uniform(0.5, 1.5, nframe) * np.where(np.arange(nframe) % 2, -1, 1)
    return inten, K, data, mask, up


def test_blur_is_the_cyclic_convolution_by_index():
    """The np.roll sums are the formula of the issue, index by index, at a
    size where the halo wraps almost twice (det 5, k 5)."""
    rng = np.random.default_rng(0)
    det, k = 5, 5
    r = k // 2
    x, K = rng.random((det, det)), rng.random((k, k))
    want = np.zeros((det, det))
    corr = np.zeros((det, det))
    for y in range(det):
        for xx in range(det):
            for u in range(k):
                for v in range(k):
                    want[y, xx] += K[u, v] * x[(y - u + r) % det,
                                               (xx - v + r) % det]
                    corr[y, xx] += K[u, v] * x[(y + u - r) % det,
                                               (xx + v - r) % det]
    np.testing.assert_allclose(bl.blur(K, x), want, rtol=1e-13)
    np.testing.assert_allclose(bl.correlate(K, x), corr, rtol=1e-13)


@pytest.mark.parametrize("det,k", [(5, 5), (8, 7), (13, 3)])
def test_correlation_is_the_adjoint_of_the_blur(det, k):
    rng = np.random.default_rng(det)
    K = rng.random((k, k))
    x, y = rng.standard_normal((2, 3, det, det))
    lhs, rhs = np.sum(bl.blur(K, x) * y), np.sum(x * bl.correlate(K, y))
    assert abs(lhs - rhs) <= 1e-12 * np.sum(np.abs(bl.blur(K, np.abs(x)) * y))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_table_and_kgrad_against_finite_differences(model, masked):
    """Central differences of sum_f up_f cost_f in float64: along a random
    direction of the intensities (the table) and of the kernel (kgrad)."""
    inten, K, data, mask, up = _frames(3, 9, 5, 11, masked)
    rng = np.random.default_rng(5)
    f = lambda I, KK: bl.cost_from_intensity(model, data, I, KK, mask, up)
    dI = rng.standard_normal(inten.shape)
    _fd_close(lambda I: f(I, K), inten, dI,
              np.sum(bl.table(model, data, inten, K, mask, up) * dI))
    dK = rng.standard_normal(K.shape)
    _fd_close(lambda KK: f(inten, KK), K, dK,
              np.sum(bl.kgrad(model, data, inten, K, mask, up) * dK))


@pytest.mark.parametrize("model", MODELS)
def test_the_chain_of_the_parametrisation(model):
    """d / d a through K = a^2 / sum a^2 against central differences; it
    annihilates the direction a itself (the scale of a does not move K), and
    an entry of a that is 0 has gradient 0."""
    inten, K, data, mask, up = _frames(2, 8, 3, 3, True)
    rng = np.random.default_rng(9)
    a = rng.uniform(0.2, 1.0, (3, 3))
    a[0, 2] = 0.0
    f = lambda x: bl.cost_from_intensity(model, data, inten, bl.kernel_of(x),
                                         mask, up)
    ga = bl.grad_a(a, bl.kgrad(model, data, inten, bl.kernel_of(a), mask, up))
    da = rng.standard_normal(a.shape)
    # (a^2 is even around the entry at 0: the central difference sees the 0
    # the chain gives there)
    _fd_close(f, a, da, np.sum(ga * da), rtol=1e-6)
    assert abs(np.sum(ga * a)) <= 1e-13 * np.sum(np.abs(ga * a))
    assert ga[0, 2] == 0.0
    np.testing.assert_allclose(bl.kernel_of(3.7 * a), bl.kernel_of(a),
                               rtol=1e-14)


def test_abi_prototypes_are_present():
    import tike_amd._lib as L
    for name, nargs in (("tike_blur_cost_factor", 15),
                        ("tike_blur_kernel_sums_partials", 2),
                        ("tike_blur_kernel_sums", 14)):
        assert len(L._PROTOTYPES[name]) == nargs
        assert hasattr(L.lib, name)
    # host only: the length of the partials for a plane and a kernel
    n = L.lib.tike_blur_kernel_sums_partials(33, 5)
    assert n > 0 and n % 26 == 0
    assert L.lib.tike_blur_kernel_sums_partials(33, 4) == 0
    assert L.lib.tike_blur_kernel_sums_partials(4, 5) == 0


# ------------------------------------------------------ the solver's problems
MIN_MARGIN = 1e-4
"""Every comparison of the model's line searches on the problems the GPU test
compares is decided by at least this relative margin.  The device's float32
costs carry about 1e-6 of relative error -- a few u per term, (k^2 + 1) u
through I_model, float64 sums --, a hundredth of it.  (fly_scan.MIN_MARGIN is
1e-3; the poisson cost of these low-count patterns, I - d log I, is mostly a
constant that no step moves, so its relative steps are smaller.)"""


@pytest.mark.parametrize("model,use_mask,update", bl.SOLVER_VARIANTS)
@pytest.mark.parametrize("case", sorted(bl.SOLVER_CASES))
def test_line_searches_of_the_solver_problems_are_clearly_decided(
        case, model, use_mask, update):
    state, P, mask = bl.run_model(case, model, use_mask, update)
    print(case, model, use_mask, update, f"{min(state['margins']):.2e}")
    assert min(state["margins"]) >= MIN_MARGIN
    costs = np.ravel(state["costs"])
    assert costs[1] < costs[0]
    K = bl.kernel_of(state["a"])
    assert abs(K.sum() - 1) <= 1e-12 and np.all(K >= 0)
    if not update:
        np.testing.assert_allclose(K, bl.normalised(P["k0"]), rtol=1e-6)


def test_demonstration_modelling_the_blur_helps():
    """One mode and the true kernel against one mode alone on blurred
    patterns; and the fit from 0.52 / 0.02 finds the kernel."""
    none, _ = bl.run_demo("none")
    true, _ = bl.run_demo("true")
    fit, state = bl.run_demo("fit")
    l1_0 = float(np.abs(bl.first_guess() - bl.TRUE_KERNEL).sum())
    l1 = float(np.abs(bl.kernel_of(state["a"]) - bl.TRUE_KERNEL).sum())
    print(f"object error: no blur {none:.4f}, true kernel {true:.4f}, fitted "
          f"{fit:.4f}; L1 distance of the kernel {l1_0:.3f} -> {l1:.4f}")
    assert true < 0.7 * none and fit < 0.7 * none
    assert l1 < 0.1 * l1_0


# --------------------------------------------------------- the host interface
def test_blur_is_part_of_the_public_interface():
    """Fails on the parent commit: there is no `blur`."""
    import dataclasses
    import inspect

    import tike_amd.autograd as ag
    import tike_amd.operators as tops
    import tike_amd.ptycho as tp
    assert "BlurOptions" in tp.__all__
    fields = {f.name: f.default for f in dataclasses.fields(tp.BlurOptions)}
    assert list(fields) == ["kernel", "update", "update_start"]
    assert fields["update"] is True and fields["update_start"] == 0
    for fn in (tp.Reconstruction.__init__, tp.reconstruct,
               tp.reconstruct_multigrid):
        p = inspect.signature(fn).parameters["blur_options"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for fn in (ag.cost, tops.Ptycho.cost):
        p = inspect.signature(fn).parameters["blur"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for fn in (tp.simulate, tops.Ptycho._compute_intensity):
        assert inspect.signature(fn).parameters["blur"].default is None
    assert hasattr(tops.Ptycho, "blur_cost_factor")
    assert hasattr(tops.Ptycho, "blur_kernel_sums")
    for fn in (ag.cost_jvp, ag.cost_gauss_newton_product):
        assert "blur" not in inspect.signature(fn).parameters


def test_option_validation_and_normalisation():
    from tike_amd.ptycho import blur as B
    K = np.full((5, 5), 2.0, np.float32)
    K[2, 2] = 50.0
    got = B.checked_kernel(K, 16)
    assert got.dtype == np.float32 and got.shape == (5, 5)
    assert abs(float(got.sum(dtype=np.float64)) - 1) <= 25 * 2.0**-24
    np.testing.assert_allclose(got, K / K.sum(dtype=np.float64), rtol=1e-7)
    assert K[2, 2] == 50.0  # (the caller's array is left as it is)
    zero = K.copy()
    zero[0, 4] = 0
    assert B.checked_kernel(zero, 16)[0, 4] == 0
    for bad, match in ((np.ones((4, 4), np.float32), "has shape"),
                       (np.ones((9, 9), np.float32), "has shape"),
                       (np.ones((3, 5), np.float32), "has shape"),
                       (np.ones((2, 3, 3), np.float32), "has shape"),
                       (np.ones((3, 3)), "expected float32"),
                       (np.ones((7, 7), np.float32), "wider than the detector"),
                       (-K, "finite and >= 0"),
                       (K * np.float32("nan"), "finite and >= 0"),
                       (K * np.float32("inf"), "finite and >= 0"),
                       (0 * K, "positive sum")):
        with pytest.raises(ValueError, match=match):
            B.checked_kernel(bad, 6)
    # the chain on the device tensors' CPU twins is the model's
    import torch
    rng = np.random.default_rng(1)
    a = rng.uniform(0.1, 1, (5, 5)).astype(np.float32)
    g = rng.standard_normal((5, 5))
    np.testing.assert_allclose(
        B.chain(torch.from_numpy(a), torch.from_numpy(g)).numpy(),
        bl.grad_a(a, g), rtol=1e-6)
    np.testing.assert_allclose(B.kernel_of(torch.from_numpy(a)).numpy(),
                               bl.kernel_of(a), rtol=1e-6)


def test_every_refusal(monkeypatch):
    import tike_amd.autograd as ag
    import tike_amd.operators as tops
    import tike_amd.ptycho as tp
    from test_background_cpu import _parameters, _scan
    data = np.zeros((12, 16, 16), np.float32)
    scan = _scan(12)
    good = lambda: tp.BlurOptions(bl.first_guess())

    def refused(match, params=None, bo=None, error=NotImplementedError, **kw):
        with pytest.raises(error, match=match):
            tp.Reconstruction(kw.pop("data", data),
                              params or _parameters(tp, scan),
                              blur_options=good() if bo is None else bo, **kw)

    for options in (tp.LstsqOptions, tp.RpieOptions, tp.DmOptions):
        refused(f"blur_options with {options(num_batch=1).name}",
                _parameters(tp, scan, options=options(num_batch=1)))
    refused("blur_options with binning=2",
            data=np.zeros((12, 8, 8), np.float32), binning=2)
    refused("blur_options with background_options",
            background_options=tp.BackgroundOptions(
                np.zeros((16, 16), np.float32)))
    refused("blur_options with several slices",
            _parameters(tp, scan, slices=2))
    refused("blur_options with eigen probes", _parameters(
        tp, scan, eigen_probe=np.ones((1, 1, 1, 16, 16), np.complex64),
        eigen_weights=np.ones((12, 2, 1), np.float32)))
    refused("blur_options with position_options", _parameters(
        tp, scan, position_options=tp.PositionOptions(scan.copy())))
    refused("blur_options with data_on_host", data_on_host=True)
    refused("blur_options with local_data", local_data=object())
    # the wrong shape, dtype or sign
    refused("has shape", bo=tp.BlurOptions(np.ones((4, 4), np.float32)),
            error=ValueError)
    refused("expected float32", bo=tp.BlurOptions(np.ones((3, 3))),
            error=ValueError)
    negative = bl.first_guess()
    negative[2, 3] = -1e-3
    refused("finite and >= 0", bo=tp.BlurOptions(negative), error=ValueError)
    negative[2, 3] = np.nan
    refused("finite and >= 0", bo=tp.BlurOptions(negative), error=ValueError)
    refused("must be a tike_amd.ptycho.BlurOptions", bo=negative,
            error=TypeError)
    # update_positions_pd of a context with a blur
    ctx = tp.Reconstruction.__new__(tp.Reconstruction)
    from tike_amd.operators.detector import Detector
    ctx._detector = Detector("blur", 1, bl.first_guess())
    with pytest.raises(NotImplementedError,
                       match="blur_options with update_positions_pd"):
        ctx.update_positions_pd()
    # reconstruct_multigrid; reconstruct(num_gpu=N) from a plain process
    with pytest.raises(NotImplementedError,
                       match="blur_options with reconstruct_multigrid"):
        tp.reconstruct_multigrid(data, _parameters(tp, scan),
                                 blur_options=good())
    with pytest.raises(NotImplementedError, match=r"blur_options with "
                       r"reconstruct\(num_gpu=2\)"):
        tp.reconstruct(data, _parameters(tp, scan), num_gpu=2,
                       blur_options=good())
    # simulate
    probe = np.ones((1, 1, 1, 16, 16), np.complex64)
    K = bl.first_guess()
    one = np.ones((1, 64, 64), np.complex64)
    with pytest.raises(NotImplementedError, match="blur with binning=2"):
        tp.simulate(16, probe, scan, one, binning=2, blur=K)
    with pytest.raises(NotImplementedError, match="blur with a background"):
        tp.simulate(16, probe, scan, one, blur=K,
                    background=np.zeros((16, 16), np.float32))
    with pytest.raises(NotImplementedError, match="blur with several slices"):
        tp.simulate(16, probe, scan, np.ones((2, 64, 64), np.complex64),
                    blur=K)
    with pytest.raises(NotImplementedError, match="blur with eigen probes"):
        tp.simulate(16, probe, scan, one, blur=K,
                    eigen_weights=np.ones((12, 1, 1), np.float32))
    with pytest.raises(ValueError, match="blur has shape"):
        tp.simulate(16, probe, scan, one, blur=np.ones((4, 4), np.float32))
    with pytest.raises(ValueError, match="finite and >= 0"):
        tp.simulate(16, probe, scan, one, blur=-K)
    # the differentiable cost

    class Op:
        detector_shape = 16

    import torch
    t = torch.from_numpy(K)
    with pytest.raises(NotImplementedError, match="blur with binning=2"):
        ag._checked_blur("cost", Op(), t, 2, None)
    with pytest.raises(NotImplementedError, match="blur with a background"):
        ag._checked_blur("cost", Op(), t, 1, torch.zeros(16, 16))
    with pytest.raises(TypeError, match="blur must be a torch"):
        ag._checked_blur("cost", Op(), K, 1, None)
    with pytest.raises(TypeError, match="blur must be torch.float32"):
        ag._checked_blur("cost", Op(), t.double(), 1, None)
    with pytest.raises(ValueError, match=r"blur must be \(k, k\)"):
        ag._checked_blur("cost", Op(), torch.zeros(4, 4), 1, None)
    with pytest.raises(ValueError, match="wider than the detector"):
        Op.detector_shape = 4
        ag._checked_blur("cost", Op(), t, 1, None)
    Op.detector_shape = 16
    with pytest.raises(TypeError, match="no CPU fallback"):
        ag._checked_blur("cost", Op(), t, 1, None)
    # the ranks of a torch.distributed job
    from tike_amd.ptycho import _spawn
    monkeypatch.setattr(_spawn, "world_size", lambda: 2)
    refused("blur_options with the ranks of a torch.distributed job")
