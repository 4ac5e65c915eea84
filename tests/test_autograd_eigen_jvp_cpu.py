"""The forward-mode derivative of the intensity model with eigen probes
without a GPU: the float64 formulas (tests/autograd_eigen_jvp.py) against
`torch.autograd.functional.jvp` of the model, central differences and the
reverse mode (the adjoint identity), what float32 alone costs, every refusal
of `eigen_intensity_jvp` and `eigen_gauss_newton_product`, the new ABI entry,
and joint Levenberg-Marquardt recovery of positions and eigen weights on the
model.

Every figure a bar is set on is printed before it is asserted."""
import ctypes
import os

import numpy as np
import pytest
import torch

import autograd_eigen as ae
import autograd_eigen_jvp as ej
import autograd_jvp as aj
import autograd_model as am

# END_TO_END_CASES of autograd_eigen.py, and C = 0 (eigen_probe None)
CASES = ae.END_TO_END_CASES + [ae.END_TO_END_CASES_MORE[1]]


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _subsets(c):
    """Each tangent the case has alone, and all of them together."""
    have = tuple(k for k in ej.TANGENT_NAMES if c[k] is not None)
    return [(k,) for k in have] + [have]


@pytest.mark.parametrize("shape", CASES)
def test_hand_jvp_equals_torch_jvp_of_the_model(shape):
    """`torch.autograd.functional.jvp` of `autograd_eigen.intensity` in
    complex128 (torch differentiates the model itself; the integer part of a
    position is a constant of the model) against `hand_jvp`: 1e-10 normwise,
    each tangent alone and all five together.  The primal of `hand_jvp` is the
    model's intensity."""
    N, S, M, C, pw, det, H, fly = shape
    c = ej.case(*shape)
    m = ae.model_of(c)
    live = [i for i, x in enumerate(m) if x is not None]

    def f(*given):
        full = [None] * 5
        for i, x in zip(live, given):
            full[i] = x
        return ae.intensity(*full, det, fly)

    for names in _subsets(c):
        t = ej.model_tangents(c, names)
        v = tuple(torch.zeros_like(m[i]) if t[ej.TANGENT_NAMES[i]] is None
                  else t[ej.TANGENT_NAMES[i]] for i in live)
        inten, want = torch.autograd.functional.jvp(
            f, tuple(m[i] for i in live), v)
        got_i, got = ej.hand_jvp(*m, det, fly=fly, **t)
        err = rel(got, want.detach())
        print(f"{shape} {names}: {err:.2e}")
        assert float(want.abs().max()) > 0
        assert rel(got_i, inten.detach()) < 1e-14
        assert err < 1e-10, (names, err)


@pytest.mark.parametrize("norm", ["ortho", "forward", "backward"])
@pytest.mark.parametrize("shape", [CASES[0], CASES[4]])
def test_hand_jvp_equals_central_differences(shape, norm):
    """A sanity check that does not go through torch's autograd:
    (I(x + eps v) - I(x - eps v)) / (2 eps) with eps = 1e-6 on the float64
    model, to 1e-7 normwise (the model is a polynomial of degree four in its
    inputs; the truncation error is eps^2, the rounding error 1e-16 / eps),
    all tangents together."""
    N, S, M, C, pw, det, H, fly = shape
    eps = 1e-6
    c = ej.case(*shape, norm)
    m = ae.model_of(c)
    t = ej.model_tangents(c)
    step = [t[k] for k in ej.TANGENT_NAMES]
    # (the step crosses no integer)
    frac = m[2] - torch.floor(m[2])
    assert float((frac - eps * step[2].abs()).min()) > 0
    assert float((frac + eps * step[2].abs()).max()) < 1
    move = lambda sign: [None if x is None else x + sign * eps * d
                         for x, d in zip(m, step)]
    with torch.no_grad():
        up = ae.intensity(*move(+1), det, fly, norm)
        dn = ae.intensity(*move(-1), det, fly, norm)
    _, got = ej.hand_jvp(*m, det, fly=fly, norm=norm, **t)
    err = rel(got, (up - dn) / (2 * eps))
    print(f"{shape} {norm}: {err:.2e}")
    assert err < 1e-7, err


@pytest.mark.parametrize("shape", CASES)
def test_what_float32_alone_costs(shape):
    """The same formulas in float32 on the CPU stay an order of magnitude
    inside the bar the GPU tests hold the kernels to (normwise 1e-5)."""
    N, S, M, C, pw, det, H, fly = shape
    c = ej.case(*shape)
    m, t = ae.model_of(c), ej.model_tangents(c)
    _, want = ej.hand_jvp(*m, det, fly=fly, **t)
    inten, got = ej.hand_jvp_float32(*m, det, fly=fly, **t)
    assert got.dtype == inten.dtype == torch.float32
    err = rel(got.to(am.F64), want)
    print(f"{shape}: float32 restatement {err:.2e}")
    assert err < 1e-6


@pytest.mark.parametrize("norm", ["ortho", "forward"])
@pytest.mark.parametrize("shape", CASES)
def test_adjoint_identity_on_the_model(shape, norm):
    """<u, J v> = <J^T u, v> to 1e-12 relative, J v by `hand_jvp` and J^T u
    by `autograd_eigen.hand_gradients`, both float64, over the five inputs."""
    N, S, M, C, pw, det, H, fly = shape
    c = ej.case(*shape, norm)
    m, t = ae.model_of(c), ej.model_tangents(c)
    u = ae.t128(c["u"])
    _, dI = ej.hand_jvp(*m, det, fly=fly, norm=norm, **t)
    g = ae.hand_gradients(*m, det, u, fly, norm)
    left = aj.inner(u, dI)
    right = sum(aj.inner(g[k], t["d_" + k])
                for k in ("psi", "probe", "scan", "eigen", "weights")
                if t["d_" + k] is not None)
    print(f"{shape} {norm}: {left:.15e} {right:.15e}")
    assert abs(left - right) <= 1e-12 * abs(left)


def test_weight_rows_of_modes_without_an_eigen_probe_count_for_nothing():
    """M < S: rows c + 1 of the weights and of their tangent in the modes
    s >= M may hold anything."""
    shape = CASES[0]
    N, S, M, C, pw, det, H, fly = shape
    assert 0 < M < S
    c = ej.case(*shape)
    m, t = list(ae.model_of(c)), ej.model_tangents(c)
    want = ej.hand_jvp(*m, det, fly=fly, **t)
    m[4] = m[4].clone()
    t["d_weights"] = t["d_weights"].clone()
    m[4][:, 1:, M:] = 1e30
    t["d_weights"][:, 1:, M:] = -1e30
    got = ej.hand_jvp(*m, det, fly=fly, **t)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------ refusals
def test_every_refusal():
    """The argument checks come before any device work: CPU tensors reach
    every one of them, and are themselves refused last."""
    import tike_amd.operators as ops
    from tike_amd.autograd import (MAX_EIGEN_PLANES, MAX_MODES,
                                   eigen_gauss_newton_product,
                                   eigen_intensity_jvp)
    pw, det, H, W, N, S, C, M = 8, 12, 24, 31, 6, 2, 2, 1
    c64 = torch.complex64
    psi = torch.zeros((1, H, W), dtype=c64)
    probe = torch.zeros((1, 1, S, pw, pw), dtype=c64)
    scan = torch.full((N, 2), 3.5)
    eigen = torch.zeros((1, C, M, pw, pw), dtype=c64)
    w = torch.ones((N, C + 1, S))
    weight = torch.ones((N, det, det))
    with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:
        for fn, name in ((eigen_intensity_jvp, "eigen_intensity_jvp"),
                         (eigen_gauss_newton_product,
                          "eigen_gauss_newton_product")):
            kw = dict(eigen_probe=eigen, eigen_weights=w)
            # (without an eigen probe the product's `wrt` must not name one)
            c0 = {} if fn is eigen_intensity_jvp else dict(
                wrt=("psi", "probe", "scan", "eigen_weights"))
            # eigen_weights is a required keyword
            with pytest.raises(TypeError, match="eigen_weights"):
                fn(op, psi, probe, scan)
            with pytest.raises(TypeError, match="eigen_weights"):
                fn(op, psi, probe, scan, eigen_probe=eigen)
            with pytest.raises(TypeError, match="eigen_weights is required"):
                fn(op, psi, probe, scan, eigen_probe=eigen, eigen_weights=None)
            # what `_checked` raises for the eigen form, under the new name
            with pytest.raises(NotImplementedError, match="several slices"):
                fn(op, psi.expand(2, H, W), probe, scan, **kw)
            with pytest.raises(NotImplementedError, match="probe per position"):
                fn(op, psi, probe.expand(N, 1, S, pw, pw), scan, **kw)
            with pytest.raises(TypeError, match="psi must be a torch"):
                fn(op, psi.numpy(), probe, scan, **kw)
            with pytest.raises(TypeError,
                               match="eigen_probe must be a torch"):
                fn(op, psi, probe, scan, eigen_probe=eigen.numpy(),
                   eigen_weights=w)
            with pytest.raises(TypeError,
                               match="eigen_weights must be a torch"):
                fn(op, psi, probe, scan, eigen_probe=eigen,
                   eigen_weights=w.numpy())
            with pytest.raises(TypeError,
                               match=name + ": probe must be torch.complex64"):
                fn(op, psi, probe.to(torch.complex128), scan, **kw)
            with pytest.raises(
                    TypeError,
                    match=name + ": eigen_weights must be torch.float32"):
                fn(op, psi, probe, scan, eigen_probe=eigen,
                   eigen_weights=w.double())
            with pytest.raises(
                    TypeError,
                    match=name + ": eigen_probe must be torch.complex64"):
                fn(op, psi, probe, scan, eigen_probe=eigen.to(torch.complex128),
                   eigen_weights=w)
            with pytest.raises(ValueError, match="not a multiple of fly=4"):
                fn(op, psi, probe, scan, fly=4, **kw)
            many = torch.zeros((1, 1, MAX_MODES + 1, pw, pw), dtype=c64)
            with pytest.raises(ValueError, match=f"at most {MAX_MODES}"):
                fn(op, psi, many, scan, eigen_weights=torch.ones(
                    (N, 1, MAX_MODES + 1)), **c0)
            with pytest.raises(ValueError,
                               match=name + ": eigen_weights must be"):
                fn(op, psi, probe, scan, eigen_probe=eigen,
                   eigen_weights=w[:, :2])  # C + 1 = 2 rows for C = 2
            with pytest.raises(ValueError,
                               match=name + ": eigen_weights must be"):
                fn(op, psi, probe, scan, eigen_weights=w, **c0)  # C = 0: one row
            with pytest.raises(ValueError,
                               match=name + ": eigen_probe must be"):
                fn(op, psi, probe, scan,
                   eigen_probe=torch.zeros((1, C, S + 1, pw, pw), dtype=c64),
                   eigen_weights=w)  # M > S
            with pytest.raises(ValueError, match="eigen_probe .* expected"):
                fn(op, psi, probe, scan, eigen_probe=eigen[0],
                   eigen_weights=w)
            wide_probe = torch.zeros((1, 1, 9, pw, pw), dtype=c64)
            planes = torch.zeros((1, 2, 9, pw, pw), dtype=c64)
            with pytest.raises(ValueError,
                               match=f"at most {MAX_EIGEN_PLANES}"):
                fn(op, psi, wide_probe, scan, eigen_probe=planes,
                   eigen_weights=torch.ones((N, 3, 9)))
            outside = scan.clone()
            outside[2] = torch.tensor((0.5, 3.0))
            with pytest.raises(ValueError, match="Scan positions must be >= 1"):
                fn(op, psi, probe, outside, d_scan=scan, **kw)
            with pytest.raises(TypeError, match="no CPU fallback"):
                fn(op, psi, probe, outside, check_positions=False, **kw)
            # a tangent matches its primal
            with pytest.raises(TypeError, match="d_psi must be a torch"):
                fn(op, psi, probe, scan, d_psi=psi.numpy(), **kw)
            with pytest.raises(TypeError,
                               match="d_eigen_probe must be a torch"):
                fn(op, psi, probe, scan, d_eigen_probe=eigen.numpy(), **kw)
            with pytest.raises(TypeError,
                               match="d_eigen_weights must be a torch"):
                fn(op, psi, probe, scan, d_eigen_weights=w.numpy(), **kw)
            with pytest.raises(TypeError, match="d_psi must be torch.complex64"):
                fn(op, psi, probe, scan, d_psi=psi.to(torch.complex128), **kw)
            with pytest.raises(TypeError,
                               match="d_eigen_probe must be torch.complex64"):
                fn(op, psi, probe, scan,
                   d_eigen_probe=eigen.to(torch.complex128), **kw)
            with pytest.raises(TypeError,
                               match="d_eigen_weights must be torch.float32"):
                fn(op, psi, probe, scan, d_eigen_weights=w.double(), **kw)
            with pytest.raises(ValueError, match="d_probe must have the shape"):
                fn(op, psi, probe, scan, d_probe=probe[:, :, :1], **kw)
            with pytest.raises(ValueError,
                               match="d_eigen_probe must have the shape"):
                fn(op, psi, probe, scan, d_eigen_probe=eigen[:, :1], **kw)
            with pytest.raises(ValueError,
                               match="d_eigen_weights must have the shape"):
                fn(op, psi, probe, scan, d_eigen_weights=w[:, :1], **kw)
            with pytest.raises(ValueError, match="d_eigen_weights lives on"):
                fn(op, psi, probe, scan, d_eigen_weights=w.to("meta"), **kw)
            with pytest.raises(ValueError, match="d_eigen_probe lives on"):
                fn(op, psi, probe, scan, d_eigen_probe=eigen.to("meta"), **kw)
            with pytest.raises(ValueError,
                               match="d_eigen_probe without eigen_probe"):
                fn(op, psi, probe, scan, eigen_weights=w[:, :1],
                   d_eigen_probe=eigen, **c0)
            with pytest.raises(TypeError, match="no CPU fallback"):
                fn(op, psi, probe, scan, d_psi=psi, d_probe=probe, d_scan=scan,
                   d_eigen_probe=eigen, d_eigen_weights=w, **kw)
            with pytest.raises(TypeError, match="no CPU fallback"):  # C = 0
                fn(op, psi, probe, scan, eigen_weights=w[:, :1],
                   d_eigen_weights=w[:, :1], **c0)
        fn = eigen_gauss_newton_product
        for bad in ((), ("psi", "psi"), ("scan", "weights"), ("eigen",)):
            with pytest.raises(ValueError, match="wrt must name"):
                fn(op, psi, probe, scan, d_scan=scan, wrt=bad, **kw)
        with pytest.raises(ValueError,
                           match='"eigen_probe" in wrt with eigen_probe=None'):
            fn(op, psi, probe, scan, eigen_weights=w[:, :1], d_scan=scan)
        with pytest.raises(ValueError,
                           match='"eigen_probe" in wrt with eigen_probe=None'):
            fn(op, psi, probe, scan, eigen_weights=w[:, :1], d_scan=scan,
               wrt=("eigen_probe",))
        with pytest.raises(TypeError, match="weight must be a torch"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight.numpy(), **kw)
        with pytest.raises(TypeError, match="weight must be torch.float32"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight.double(), **kw)
        with pytest.raises(ValueError, match="weight must be"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight[:-1], **kw)
        with pytest.raises(ValueError, match="weight must be"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight, fly=2, **kw)
        with pytest.raises(ValueError, match="weight lives on"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight.to("meta"),
               **kw)
        with pytest.raises(TypeError, match="no CPU fallback"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight, **kw)
        with pytest.raises(TypeError, match="no CPU fallback"):  # C = 0
            fn(op, psi, probe, scan, eigen_weights=w[:, :1], d_scan=scan,
               wrt=("scan", "eigen_weights"))


def test_the_shared_probe_functions_still_take_no_eigen_parameter():
    """`intensity_jvp` and `gauss_newton_product` are unchanged: the eigen
    form has its own functions."""
    import tike_amd.operators as ops
    from tike_amd.autograd import gauss_newton_product, intensity_jvp
    pw, det, H, W, N = 8, 12, 24, 31, 6
    psi = torch.zeros((1, H, W), dtype=torch.complex64)
    probe = torch.zeros((1, 1, 2, pw, pw), dtype=torch.complex64)
    scan = torch.full((N, 2), 3.5)
    with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:
        for fn in (intensity_jvp, gauss_newton_product):
            with pytest.raises(TypeError, match="eigen_weights"):
                fn(op, psi, probe, scan, eigen_weights=torch.ones((N, 1, 2)))
            with pytest.raises(TypeError, match="d_eigen_weights"):
                fn(op, psi, probe, scan, d_eigen_weights=torch.ones((N, 1, 2)))


# ------------------------------------------------------------------- the ABI
def test_abi_has_the_new_entry():
    """Fails on the parent commit: the symbol does not exist."""
    import tike_amd._lib as L
    name = "tike_eigen_wave_tangent"
    assert name in L.declared_symbols()
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert L._PROTOTYPES[name] == [p] * 10 + [i, i, p, l, i, i, i, i, i, p]
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert L.ABI_VERSION >= 24
    assert "autograd_eigen_jvp.hip" in open(os.path.join(
        os.path.dirname(os.path.abspath(L.__file__)), "csrc",
        "Makefile")).read()


def test_abi_entry_checks_its_arguments_without_a_gpu():
    """Argument checks come before any launch.  Fails on the parent commit."""
    import tike_amd._lib as L
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (psi, dpsi, scan, dscan, probe, dprobe, eigen_probe, deigen_probe,
    #  eigen_weights, deigen_weights, C, M, nearplane, nscan, S, pw, det, H,
    #  W, stream)
    ok = (p, p, p, p, p, p, p, p, p, p, 1, 1, p, 1, 2, 2, 4, 4, 4, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return L.lib.tike_eigen_wave_tangent(*args)

    for k in (0, 2, 4, 8, 12):
        assert call(**{f"a{k}": None}) == L.ERR_ARG  # a NULL required array
    assert call(a6=None) == L.ERR_ARG  # eigen_probe NULL with C > 0
    assert call(a11=0) == L.ERR_ARG  # M < 1 with C > 0
    assert call(a11=3) == L.ERR_ARG  # M > S with C > 0
    assert call(a10=-1) == L.ERR_ARG  # C
    assert call(a11=-1) == L.ERR_ARG  # M
    assert call(a13=-1) == L.ERR_ARG  # nscan
    assert call(a13=1 << 31) == L.ERR_ARG  # more than grid.x holds
    assert call(a14=0) == L.ERR_ARG  # S
    assert call(a15=0) == L.ERR_ARG  # pw
    assert call(a15=5) == L.ERR_ARG  # pw > det
    assert call(a17=0) == L.ERR_ARG  # H
    assert call(a18=0) == L.ERR_ARG  # W
    assert call(a14=17) == L.ERR_UNSUPPORTED  # S
    assert call(a14=16, a10=2, a11=9) == L.ERR_UNSUPPORTED  # C * M = 18
    assert call(a14=16, a10=17, a11=1) == L.ERR_UNSUPPORTED  # C * M = 17
    # a detector of more items than one launch holds (no device: none at all)
    assert call(a15=1 << 30, a16=1 << 30) == L.ERR_ARG
    assert call(a13=0) == 0  # no position: no launch
    assert call(a13=0, a14=16, a10=1, a11=16) == 0  # the limits themselves
    # the five tangents may be NULL, and eigen_probe with C = 0 (M ignored)
    assert call(a13=0, a1=None, a3=None, a5=None, a7=None, a9=None) == 0
    assert call(a13=0, a6=None, a7=None, a10=0, a11=0) == 0
    assert call(a13=0, a6=None, a10=0, a11=7) == 0


# ------------------------------------------- joint recovery: scan and weights
def test_joint_levenberg_marquardt_on_the_model():
    """`recovery_problem()` (196 positions, one eigen probe, a frame per
    position; positions from scan_start, +- 0.3 px, weights from row 1 = 0):
    four Levenberg-Marquardt steps on (scan, eigen weights) jointly, each at
    most 20 CG iterations with J v by `hand_jvp` and J^T u by
    `autograd_eigen.hand_gradients` in float64.  Required: finite costs that
    fall with every step, and both errors falling with every step.  Measured
    when the test was written: position RMS 0.2433 -> 0.2295, 0.2166, 0.1966,
    0.1629 px, weights RMS 0.1210 -> 0.0337, 0.0181, 0.0151, 0.0104, cost
    177.6 -> 0.391.  The same iteration through `hand_jvp_float32` (float32
    parameters, residuals and products; float64 inner products) is printed
    next to it: 0.162854100 px and 0.010376345, 1.27e-7 px and 6.07e-8 from
    the float64 result; that deviation, doubled, is the margin of the GPU test
    (`autograd_eigen_jvp.JOINT_RECOVERY`, which this test reproduces)."""
    p = ej.recovery_problem()
    r0 = am.rms(p["scan_start"], p["scan_true"])
    w0 = ae.weights_rms(p["weights_start"], p["weights_true"])
    out = {}
    for single in (False, True):
        after, costs = ej.joint_recovery_model(p, single=single)
        r = [am.rms(a[0], p["scan_true"]) for a in after]
        w = [ae.weights_rms(a[1], p["weights_true"]) for a in after]
        out[single] = r[-1], w[-1]
        print(f"joint LM on the model, float{32 if single else 64}: rms "
              f"{r0:.4f} -> " + ", ".join(f"{x:.9f}" for x in r)
              + f"; weights rms {w0:.4f} -> "
              + ", ".join(f"{x:.9f}" for x in w) + "; cost "
              + " -> ".join(f"{x:.6e}" for x in costs))
        assert np.isfinite(costs).all()
        assert all(b < a for a, b in zip(costs, costs[1:])), costs
        assert all(b < a for a, b in zip([r0] + r, r)), r
        assert all(b < a for a, b in zip([w0] + w, w)), w
    j = ej.JOINT_RECOVERY
    # the float64 figures the GPU test is bounded by are those of this run
    # (1e-9: the order of a sum is the library's); the float32 figures were
    # measured once and are printed, not asserted: another CPU's float32
    # transform rounds differently, by as much as the deviation itself
    assert abs(out[False][0] - j["rms64"]) <= 1e-9
    assert abs(out[False][1] - j["wrms64"]) <= 1e-9
    print(f"float32 deviates by {abs(out[True][0] - out[False][0]):.3e} px "
          f"and {abs(out[True][1] - out[False][1]):.3e} in the weights")
