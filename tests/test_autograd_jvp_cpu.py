"""The forward-mode derivative of the intensity model without a GPU: the
float64 formulas (tests/autograd_jvp.py) against central differences and
against the reverse mode (the adjoint identity), what float32 alone costs,
every refusal of `intensity_jvp` and `gauss_newton_product`, the two new ABI
entries, and Gauss-Newton position recovery on the model."""
import ctypes

import numpy as np
import pytest
import torch

import autograd_jvp as aj
import autograd_model as am

# (N, S, pw, det, H, W, fly): probe window < detector and = detector
SHAPES = [(6, 2, 8, 12, 24, 31, 1), (8, 3, 16, 16, 40, 37, 2)]
TANGENTS = [("d_psi",), ("d_probe",), ("d_scan",), ("d_psi", "d_probe", "d_scan")]


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("norm", ["ortho", "forward", "backward"])
@pytest.mark.parametrize("shape", SHAPES)
def test_hand_jvp_equals_central_differences(shape, norm):
    """(I(x + eps v) - I(x - eps v)) / (2 eps) with eps = 1e-6 on the float64
    model, to 1e-7 normwise: each tangent alone and all together.  The primal
    of `hand_jvp` is the model's intensity."""
    det, fly = shape[3], shape[6]
    eps = 1e-6
    c = aj.case(*shape)
    for names in TANGENTS:
        (psi, probe, scan), t = aj.as_model(c, names)
        zero = lambda x: torch.zeros_like(x)
        dpsi, dprobe, dscan = (
            zero(x) if t[k] is None else t[k]
            for k, x in (("d_psi", psi), ("d_probe", probe), ("d_scan", scan)))
        # (the step crosses no integer)
        frac = scan - torch.floor(scan)
        assert float((frac - eps * dscan.abs()).min()) > 0
        assert float((frac + eps * dscan.abs()).max()) < 1
        with torch.no_grad():
            up = am.intensity(psi + eps * dpsi, probe + eps * dprobe,
                              scan + eps * dscan, det, fly, norm)
            dn = am.intensity(psi - eps * dpsi, probe - eps * dprobe,
                              scan - eps * dscan, det, fly, norm)
            want = am.intensity(psi, probe, scan, det, fly, norm)
        inten, got = aj.hand_jvp(psi, probe, scan, det, fly=fly, norm=norm, **t)
        err = rel(got, (up - dn) / (2 * eps))
        print(f"{shape} {norm} {names}: {err:.2e}")
        assert rel(inten, want) < 1e-14
        assert err < 1e-7, (names, err)


@pytest.mark.parametrize("norm", ["ortho", "forward", "backward"])
@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint_identity_on_the_model(shape, norm):
    """<u, J v> = <J^T u, v> to 1e-12 relative, J v by `hand_jvp` and J^T u by
    torch.autograd on the model."""
    N, S, pw, det, H, W, fly = shape
    c = aj.case(*shape)
    (psi, probe, scan), t = aj.as_model(c)
    u = torch.from_numpy(np.random.default_rng(3).standard_normal(
        (N // fly, det, det)))
    _, dI = aj.hand_jvp(psi, probe, scan, det, fly=fly, norm=norm, **t)
    _, gpsi, gprobe, gscan = am.autograd_gradients(psi, probe, scan, det, u,
                                                   fly, norm)
    left = aj.inner(u, dI)
    right = (aj.inner(gpsi, t["d_psi"]) + aj.inner(gprobe, t["d_probe"])
             + aj.inner(gscan, t["d_scan"]))
    print(f"{shape} {norm}: {left:.15e} {right:.15e}")
    assert abs(left - right) <= 1e-12 * abs(left)


@pytest.mark.parametrize("shape", SHAPES)
def test_what_float32_alone_costs(shape):
    """The same formulas in float32 on the CPU stay an order of magnitude
    inside the bar the GPU tests hold the kernels to (normwise 1e-5)."""
    det, fly = shape[3], shape[6]
    (psi, probe, scan), t = aj.as_model(aj.case(*shape))
    _, want = aj.hand_jvp(psi, probe, scan, det, fly=fly, **t)
    _, got = aj.hand_jvp_float32(psi, probe, scan, det, fly=fly, **t)
    err = rel(got.to(am.F64), want)
    print(f"{shape}: float32 restatement {err:.2e}")
    assert err < 1e-6


# ------------------------------------------------------------------ refusals
def test_every_refusal():
    """The argument checks come before any device work: CPU tensors reach
    every one of them, and are themselves refused last."""
    import tike_amd.operators as ops
    from tike_amd.autograd import (MAX_MODES, gauss_newton_product,
                                   intensity_jvp)
    pw, det, H, W, N = 8, 12, 24, 31, 6
    psi = torch.zeros((1, H, W), dtype=torch.complex64)
    probe = torch.zeros((1, 1, 2, pw, pw), dtype=torch.complex64)
    scan = torch.full((N, 2), 3.5)
    weight = torch.ones((N, det, det))
    with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:
        for fn, name in ((intensity_jvp, "intensity_jvp"),
                         (gauss_newton_product, "gauss_newton_product")):
            with pytest.raises(NotImplementedError, match="several slices"):
                fn(op, psi.expand(2, H, W), probe, scan)
            with pytest.raises(NotImplementedError, match="probe per position"):
                fn(op, psi, probe.expand(N, 1, 2, pw, pw), scan)
            with pytest.raises(TypeError, match="psi must be a torch"):
                fn(op, psi.numpy(), probe, scan)
            with pytest.raises(TypeError, match="scan must be a torch"):
                fn(op, psi, probe, scan.numpy())
            with pytest.raises(TypeError,
                               match=name + ": probe must be torch.complex64"):
                fn(op, psi, probe.to(torch.complex128), scan)
            with pytest.raises(TypeError, match="scan must be torch.float32"):
                fn(op, psi, probe, scan.to(torch.float64))
            with pytest.raises(ValueError, match="not a multiple of fly=4"):
                fn(op, psi, probe, scan, fly=4)
            many = torch.zeros((1, 1, MAX_MODES + 1, pw, pw),
                               dtype=torch.complex64)
            with pytest.raises(ValueError, match=f"at most {MAX_MODES}"):
                fn(op, psi, many, scan)
            with pytest.raises(TypeError):  # eigen probes are no parameter
                fn(op, psi, probe, scan, eigen_weights=torch.ones((N, 1, 2)))
            outside = scan.clone()
            outside[2] = torch.tensor((0.5, 3.0))
            with pytest.raises(ValueError, match="Scan positions must be >= 1"):
                fn(op, psi, probe, outside, d_scan=scan)
            with pytest.raises(TypeError, match="no CPU fallback"):
                fn(op, psi, probe, outside, check_positions=False)
            # a tangent matches its primal
            with pytest.raises(TypeError, match="d_psi must be a torch"):
                fn(op, psi, probe, scan, d_psi=psi.numpy())
            with pytest.raises(TypeError, match="d_psi must be torch.complex64"):
                fn(op, psi, probe, scan, d_psi=psi.to(torch.complex128))
            with pytest.raises(TypeError, match="d_scan must be torch.float32"):
                fn(op, psi, probe, scan, d_scan=scan.to(torch.float64))
            with pytest.raises(ValueError, match="d_probe must have the shape"):
                fn(op, psi, probe, scan, d_probe=probe[:, :, :1])
            with pytest.raises(ValueError, match="d_scan must have the shape"):
                fn(op, psi, probe, scan, d_scan=scan[:-1])
            with pytest.raises(ValueError, match="d_psi lives on"):
                fn(op, psi, probe, scan, d_psi=psi.to("meta"))
            with pytest.raises(TypeError, match="no CPU fallback"):
                fn(op, psi, probe, scan, d_psi=psi, d_probe=probe, d_scan=scan)
        fn = gauss_newton_product
        for bad in ((), ("psi", "psi"), ("scan", "weights")):
            with pytest.raises(ValueError, match="wrt must name"):
                fn(op, psi, probe, scan, d_scan=scan, wrt=bad)
        with pytest.raises(TypeError, match="weight must be a torch"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight.numpy())
        with pytest.raises(TypeError, match="weight must be torch.float32"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight.double())
        with pytest.raises(ValueError, match="weight must be"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight[:-1])
        with pytest.raises(ValueError, match="weight must be"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight, fly=2)
        with pytest.raises(ValueError, match="weight lives on"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight.to("meta"))
        with pytest.raises(TypeError, match="no CPU fallback"):
            fn(op, psi, probe, scan, d_scan=scan, weight=weight)


def test_dual_tensors_on_the_cpu_are_refused_by_name():
    """`intensity` on forward_ad dual tensors still reaches its own refusals
    (the dual of a CPU tensor is a CPU tensor)."""
    import torch.autograd.forward_ad as fwad

    import tike_amd.operators as ops
    from tike_amd.autograd import intensity
    pw, det, H, W, N = 8, 12, 24, 31, 6
    psi = torch.zeros((1, H, W), dtype=torch.complex64)
    probe = torch.zeros((1, 1, 2, pw, pw), dtype=torch.complex64)
    scan = torch.full((N, 2), 3.5)
    with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:
        with fwad.dual_level():
            dual = fwad.make_dual(scan, torch.ones_like(scan))
            with pytest.raises(TypeError, match="no CPU fallback"):
                intensity(op, psi, probe, dual)


# ------------------------------------------------------------------- the ABI
def test_abi_has_the_new_entries():
    """Fails on the parent commit: the symbols do not exist."""
    import tike_amd._lib as L
    for name, arity in (("tike_conv_fwd_tangent", 14),
                        ("tike_intensity_tangent", 8)):
        assert name in L.declared_symbols()
        assert len(L._PROTOTYPES[name]) == arity
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert L.ABI_VERSION >= 22
    import os
    assert "autograd_jvp.hip" in open(os.path.join(
        os.path.dirname(os.path.abspath(L.__file__)), "csrc",
        "Makefile")).read()


def _calls(fn, ok):
    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return fn(*args)
    return call


def test_abi_entries_check_their_arguments_without_a_gpu():
    """Argument checks come before any launch.  Fails on the parent commit."""
    import tike_amd._lib as L
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (psi, dpsi, scan, dscan, probe, dprobe, nearplane, nscan, S, pw, det, H,
    #  W, stream)
    call = _calls(L.lib.tike_conv_fwd_tangent,
                  (p, p, p, p, p, p, p, 1, 1, 2, 4, 4, 4, None))
    for k in (0, 2, 4, 6):
        assert call(**{f"a{k}": None}) == L.ERR_ARG  # a NULL required array
    assert call(a7=-1) == L.ERR_ARG  # nscan
    assert call(a7=1 << 31) == L.ERR_ARG  # more than grid.x holds
    assert call(a8=0) == L.ERR_ARG  # S
    assert call(a8=17) == L.ERR_UNSUPPORTED  # S
    assert call(a9=0) == L.ERR_ARG  # pw
    assert call(a9=5) == L.ERR_ARG  # pw > det
    assert call(a11=0) == L.ERR_ARG  # H
    assert call(a12=0) == L.ERR_ARG  # W
    assert call(a7=0) == 0  # no position: no launch
    assert call(a7=0, a1=None, a3=None, a5=None) == 0  # NULL tangents are fine
    # (farplane, dfarplane, intensity, dintensity, nframe, P, npix, stream)
    call = _calls(L.lib.tike_intensity_tangent, (p, p, p, p, 1, 2, 4, None))
    for k in (0, 1, 3):
        assert call(**{f"a{k}": None}) == L.ERR_ARG  # a NULL required array
    assert call(a4=-1) == L.ERR_ARG  # nframe
    assert call(a5=0) == L.ERR_ARG  # P
    assert call(a6=0) == L.ERR_ARG  # npix
    assert call(a4=1 << 40, a6=1 << 40) == L.ERR_ARG  # more than grid.x holds
    assert call(a4=0) == 0  # no frame: no launch
    assert call(a4=0, a2=None) == 0  # the intensity is optional


# --------------------------------------------------------- position recovery
def test_gauss_newton_recovers_the_positions_on_the_model():
    """`problem()` (196 positions, fly 2, start +- 0.3 px): four damped
    Gauss-Newton steps on the positions alone, each at most 20 CG iterations
    with J v by `hand_jvp` and J^T u by torch.autograd on the float64 model,
    bring the RMS position error to 0.05 of its start or less (0.0204 measured
    when the bar was set; 40 steps of Adam reach 0.09)."""
    p = am.problem()
    psi, probe, _ = am.as_model(p["psi"], p["probe"], p["scan_true"])
    det, fly = p["det"], p["fly"]
    data = torch.from_numpy(p["data"]).to(am.F64)
    start = torch.from_numpy(p["scan_start"]).to(am.F64)

    def forward(scan):
        with torch.no_grad():
            return am.intensity(psi, probe, scan, det, fly)

    jv = lambda scan, v: aj.hand_jvp(psi, probe, scan, det, d_scan=v,
                                     fly=fly)[1]
    jtu = lambda scan, u: am.autograd_gradients(psi, probe, scan, det, u,
                                                fly)[3]
    after, costs = aj.gauss_newton(forward, jv, jtu, data, start)
    r0 = am.rms(p["scan_start"], p["scan_true"])
    r = [am.rms(s, p["scan_true"]) for s in after]
    print(f"rms {r0:.4f} -> " + ", ".join(f"{x:.4f}" for x in r)
          + f" ({r[-1] / r0:.4f}); cost {costs[0]:.3e} -> {costs[-1]:.3e}")
    assert np.isfinite(costs).all()
    assert r[-1] <= 0.05 * r0, (r0, r)
