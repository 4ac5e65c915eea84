"""A fitted incoherent background without a GPU: the float64 model
(tests/background.py) against central differences of its own cost, how clearly
the model's line searches are decided on the problems the GPU test compares,
the demonstration, the ABI, the public interface and every refusal."""
import ctypes
import inspect

import numpy as np
import pytest

import background as bg
import fly_scan as fs


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("fly", [1, 2])
@pytest.mark.parametrize("model", ["gaussian", "poisson"])
def test_model_background_gradients_are_derivatives_of_its_cost(model, fly):
    """d (sum_f cost_f) / d b[p] and / d a[p] by central differences in
    float64, with the block mask and NaN under it (counts and background):
    the model's grad_b and grad_a, exactly 0 under the mask; a pixel with
    a = 0 is stationary."""
    K = dict(obj=40, pw=16, det=16, S=2, fly=fly, nframe=4, seed=1, amp=1.0,
             mix=0.3, dim=0.5)
    P = fs.problem(**K)
    det = K["det"]
    mask = fs.block_mask(det)
    rng = np.random.default_rng(3)
    data = fs.masked(P["data"] * 1.3 + 0.2, mask)
    psi = P["psi0"].astype(np.complex128)
    probe = P["probe0"].astype(np.complex128)
    scan = P["scan"]
    frames = len(scan) // fly
    a = (0.2 + rng.random((det, det)))
    a[3, 5] = 0.0  # pinned
    a_nan = np.where(mask, a, np.nan)
    total = lambda b: frames * bg.cost(model, data, psi, scan, probe, det,
                                       fly, mask, b)
    gb = bg.grad_b(model, data, psi, scan, probe, det, fly, mask, a_nan**2)
    ga = bg.grad_a(model, data, psi, scan, probe, det, fly, mask, a_nan)
    assert np.all(np.isfinite(gb)) and np.all(np.isfinite(ga))
    assert np.all(gb[~mask] == 0) and np.all(ga[~mask] == 0)
    assert ga[3, 5] == 0.0
    h = 1e-6
    for _ in range(12):
        y, x = rng.integers(0, det, 2)
        if not mask[y, x]:
            continue
        e = np.zeros((det, det))
        e[y, x] = 1.0
        fd = (total((a + h * e)**2) - total((a - h * e)**2)) / (2 * h)
        assert abs(fd - ga[y, x]) <= 1e-6 * max(abs(ga[y, x]), 1e-3), (
            "a", y, x, fd, ga[y, x])
        fd = (total(a**2 + h * e) - total(a**2 - h * e)) / (2 * h)
        assert abs(fd - gb[y, x]) <= 1e-6 * max(abs(gb[y, x]), 1e-3), (
            "b", y, x, fd, gb[y, x])


def test_model_without_background_is_fly_scan():
    K = fs.FIXTURE
    P = fs.problem(**K)
    args = (P["data"], P["psi0"], P["scan"], P["probe0"], K["det"], K["fly"])
    for model in ("gaussian", "poisson"):
        assert bg.cost(model, *args) == fs.cost(model, *args)
        assert np.array_equal(bg.grad_psi(model, *args),
                              fs.grad_psi(model, *args))
        assert np.array_equal(bg.grad_probe(model, *args),
                              fs.grad_probe(model, *args))


@pytest.mark.parametrize("model,use_mask,update", bg.SOLVER_VARIANTS)
@pytest.mark.parametrize("case", sorted(bg.SOLVER_CASES))
def test_line_searches_of_the_solver_problems_are_clearly_decided(
        case, model, use_mask, update):
    """Every comparison of the model's line searches, over two epochs of
    three blocks, has a relative margin >= fly_scan.MIN_MARGIN: float32
    rounding on the GPU cannot decide one differently."""
    state, P, mask = bg.run_model(case, model, use_mask, update)
    margins = np.array(state["margins"])
    print(case, model, use_mask, update, f"{len(margins)} comparisons, "
          f"smallest margin {margins.min():.2e}; costs",
          np.ravel(state["costs"]))
    assert margins.min() >= fs.MIN_MARGIN
    b0 = P["b0"]
    moved = not np.array_equal(state["a"].astype(np.float32),
                               np.sqrt(b0).astype(np.float32))
    assert moved == update
    assert len(state["costs"]) == 2


def test_demonstration_fitting_the_background_helps():
    """The model's object error on the demonstration problem
    (background.DEMO: a flat offset of 0.3 plus a smooth blob of 1.5 on
    patterns whose tails are below 1; six epochs, gaussian model, known
    probe): 0.8091 with the background ignored, 0.6554 with it fitted from a
    constant first guess of 0.1."""
    without, _ = bg.run_demo(False)
    with_fit, state = bg.run_demo(True)
    print(f"object error: background ignored {without:.4f}, fitted "
          f"{with_fit:.4f}")
    assert with_fit < without
    assert abs(without - 0.8091) < 5e-4 and abs(with_fit - 0.6554) < 5e-4
    assert min(state["margins"]) >= fs.MIN_MARGIN


# -------------------------------------------------------------------- the ABI
NAMES = {"tike_background_farplane_gradient": 16,
         "tike_background_cost_factor": 14,
         "tike_background_sums_partials": 1,
         "tike_background_sums": 13}


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
    assert "background.hip" in open(
        L.LIB_PATH.replace("libtike_amd.so", "Makefile")).read()
    assert L.ABI_VERSION == 25 and L.lib.tike_abi_version() == 25
    assert "#define TIKE_ABI_VERSION 25" in header


def test_partials_query():
    """One partial per workgroup of 64 lanes; a lane owns four pixels, the
    last npix % 4 pixels one lane each."""
    import tike_amd._lib as L
    q = L.lib.tike_background_sums_partials
    assert q(0) == 0 and q(-5) == 0
    for npix in (1, 3, 4, 169, 256, 257, 403, 1027, 128 * 128, 512 * 512):
        items = npix // 4 + npix % 4
        assert q(npix) == -(-items // 64), npix


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

    # farplane data u16 mask background intensity costs nframe fly S det
    # model apply_gradient unmeasured_scaling num_measured stream
    call = caller(L.lib.tike_background_farplane_gradient,
                  (p, p, 0, None, p, None, None, 1, 2, 1, 4, 0, 0, 1.0, 4,
                   None))
    for background in (p, None):  # (NULL forwards: the fly entry's refusals)
        assert call(a4=background, a0=None) == L.ERR_ARG  # farplane
        assert call(a4=background, a1=None) == L.ERR_ARG  # data
        assert call(a4=background, a8=0) == L.ERR_ARG  # fly
        assert call(a4=background, a9=0) == L.ERR_ARG  # S
        assert call(a4=background, a10=0) == L.ERR_ARG  # det
        assert call(a4=background, a11=2) == L.ERR_ARG  # model
        assert call(a4=background, a14=0) == L.ERR_ARG  # num_measured
        assert call(a4=background, a7=-1) == L.ERR_ARG
        assert call(a4=background, a7=0) == 0  # no frame: no launch
    # farplane data u16 mask background upstream costs table nframe P npix
    # model num_measured stream
    call = caller(L.lib.tike_background_cost_factor,
                  (p, p, 0, None, p, None, None, None, 1, 2, 16, 0, 4, None))
    for background in (p, None):
        assert call(a4=background, a0=None) == L.ERR_ARG
        assert call(a4=background, a1=None) == L.ERR_ARG
        assert call(a4=background, a9=0) == L.ERR_ARG  # P
        assert call(a4=background, a10=0) == L.ERR_ARG  # npix
        assert call(a4=background, a11=2) == L.ERR_ARG  # model
        assert call(a4=background, a12=0) == L.ERR_ARG  # num_measured
        assert call(a4=background, a8=-1) == L.ERR_ARG
        assert call(a4=background, a8=0) == 0
    # intensity data u16 mask background upstream partials bgrad nframe npix
    # model num_measured stream
    call = caller(L.lib.tike_background_sums,
                  (p, p, 0, None, p, None, None, None, 1, 16, 0, 4, None))
    assert call(a0=None) == L.ERR_ARG
    assert call(a1=None) == L.ERR_ARG
    assert call(a4=None) == L.ERR_ARG
    assert call(a9=0) == L.ERR_ARG  # npix
    assert call(a10=2) == L.ERR_ARG  # model
    assert call(a11=0) == L.ERR_ARG  # num_measured
    assert call(a8=-1) == L.ERR_ARG
    assert call(a8=0) == 0


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


def test_background_is_part_of_the_public_interface():
    """Fails on the parent commit: there is no `background`."""
    import dataclasses

    import tike_amd.autograd as ag
    import tike_amd.operators as tops
    import tike_amd.ptycho as tp
    assert "BackgroundOptions" in tp.__all__
    fields = {f.name: f.default for f in dataclasses.fields(
        tp.BackgroundOptions)}
    assert list(fields) == ["background", "update", "update_start"]
    assert fields["update"] is True and fields["update_start"] == 0
    for fn in (tp.Reconstruction.__init__, tp.reconstruct):
        p = inspect.signature(fn).parameters["background_options"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for fn in (ag.cost, tops.Ptycho.cost):
        p = inspect.signature(fn).parameters["background"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for fn in (tp.simulate, tops.Ptycho._compute_intensity):
        assert inspect.signature(fn).parameters["background"].default is None
    assert hasattr(tops.Ptycho, "background_farplane_gradient")
    for fn in (ag.cost_jvp, ag.cost_gauss_newton_product):
        assert "background" not in inspect.signature(fn).parameters


def test_every_refusal(monkeypatch):
    import tike_amd.autograd as ag
    import tike_amd.operators as tops
    import tike_amd.ptycho as tp
    data = np.zeros((12, 16, 16), np.float32)
    scan = _scan(12)
    good = lambda: tp.BackgroundOptions(np.zeros((16, 16), np.float32))

    def refused(match, params=None, bo=None, error=NotImplementedError, **kw):
        with pytest.raises(error, match=match):
            tp.Reconstruction(kw.pop("data", data),
                              params or _parameters(tp, scan),
                              background_options=good() if bo is None else bo,
                              **kw)

    for options in (tp.LstsqOptions, tp.RpieOptions, tp.DmOptions):
        refused(f"background_options with {options(num_batch=1).name}",
                _parameters(tp, scan, options=options(num_batch=1)))
    refused("background_options with binning=2",
            data=np.zeros((12, 8, 8), np.float32), binning=2)
    refused("background_options with several slices",
            _parameters(tp, scan, slices=2))
    refused("background_options with eigen probes", _parameters(
        tp, scan, eigen_probe=np.ones((1, 1, 1, 16, 16), np.complex64),
        eigen_weights=np.ones((12, 2, 1), np.float32)))
    refused("background_options with position_options", _parameters(
        tp, scan, position_options=tp.PositionOptions(scan.copy())))
    refused("background_options with data_on_host", data_on_host=True)
    refused("background_options with local_data", local_data=object())
    # the wrong shape, dtype or sign
    refused("has shape", bo=tp.BackgroundOptions(np.zeros((8, 8), np.float32)),
            error=ValueError)
    refused("expected float32", bo=tp.BackgroundOptions(np.zeros((16, 16))),
            error=ValueError)
    negative = np.zeros((16, 16), np.float32)
    negative[2, 3] = -1e-3
    refused("finite and >= 0", bo=tp.BackgroundOptions(negative),
            error=ValueError)
    negative[2, 3] = np.nan
    refused("finite and >= 0", bo=tp.BackgroundOptions(negative),
            error=ValueError)
    refused("must be a tike_amd.ptycho.BackgroundOptions", bo=negative,
            error=TypeError)
    # reconstruct(num_gpu=N) from a plain process
    with pytest.raises(NotImplementedError, match=r"background_options with "
                       r"reconstruct\(num_gpu=2\)"):
        tp.reconstruct(data, _parameters(tp, scan), num_gpu=2,
                       background_options=good())
    # simulate and the operator
    probe = np.ones((1, 1, 1, 16, 16), np.complex64)
    b = np.zeros((16, 16), np.float32)
    with pytest.raises(NotImplementedError, match="background with binning=2"):
        tp.simulate(16, probe, scan, np.ones((1, 64, 64), np.complex64),
                    binning=2, background=b)
    with pytest.raises(NotImplementedError,
                       match="background with several slices"):
        tp.simulate(16, probe, scan, np.ones((2, 64, 64), np.complex64),
                    background=b)
    with pytest.raises(NotImplementedError,
                       match="background with eigen probes"):
        tp.simulate(16, probe, scan, np.ones((1, 64, 64), np.complex64),
                    eigen_weights=np.ones((12, 1, 1), np.float32),
                    background=b)
    with pytest.raises(ValueError, match="background has shape"):
        tp.simulate(16, probe, scan, np.ones((1, 64, 64), np.complex64),
                    background=np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError, match="finite and >= 0"):
        tp.simulate(16, probe, scan, np.ones((1, 64, 64), np.complex64),
                    background=b - 1)
    # the differentiable cost

    class Op:
        detector_shape = 16

    import torch
    with pytest.raises(NotImplementedError,
                       match="background with binning=2"):
        ag._checked_background("cost", Op(), torch.zeros(16, 16), 2)
    with pytest.raises(TypeError, match="background must be a torch"):
        ag._checked_background("cost", Op(), b, 1)
    with pytest.raises(TypeError, match="background must be torch.float32"):
        ag._checked_background("cost", Op(),
                               torch.zeros(16, 16, dtype=torch.float64), 1)
    with pytest.raises(ValueError, match=r"background must be \(16, 16\)"):
        ag._checked_background("cost", Op(), torch.zeros(8, 8), 1)
    with pytest.raises(TypeError, match="no CPU fallback"):
        ag._checked_background("cost", Op(), torch.zeros(16, 16), 1)
    # the ranks of a torch.distributed job
    from tike_amd.ptycho import _spawn
    monkeypatch.setattr(_spawn, "world_size", lambda: 2)
    refused("background_options with the ranks of a torch.distributed job")
