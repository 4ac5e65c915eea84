"""The forward-mode derivative of the multislice intensity model without a
GPU: the float64 formulas (tests/autograd_multislice_jvp.py) against
`torch.func.jvp` of the model, against central differences and against the
reverse mode (the adjoint identity), what float32 alone costs, every refusal of
`multislice_intensity_jvp` and `multislice_gauss_newton_product`, the new ABI
entry, and Levenberg-Marquardt position recovery on the two-slice model."""
import ctypes

import numpy as np
import pytest
import torch

import autograd_jvp as aj
import autograd_model as am
import autograd_multislice as mm
import autograd_multislice_jvp as mj

NORMS = ["ortho", "backward"]


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape", mm.END_TO_END_CASES)
def test_hand_jvp_equals_torch_func_jvp(shape, norm):
    """`hand_jvp` with all three tangents against `torch.func.jvp` of
    `autograd_multislice.intensity`, to 1e-12 normwise (4e-16 - 6e-16 when the
    bar was set); its primal is the model's intensity."""
    c = mj.case(*shape, norm=norm)
    (psi, probe, scan, Hprop), t = mj.as_model(c)
    fly = c["fly"]
    want_i, want = torch.func.jvp(
        lambda a, b, s: mm.intensity(a, b, s, Hprop, fly, norm),
        (psi, probe, scan), (t["d_psi"], t["d_probe"], t["d_scan"]))
    inten, got = mj.hand_jvp(psi, probe, scan, Hprop, fly=fly, norm=norm, **t)
    err = rel(got, want)
    print(f"{shape} {norm}: hand_jvp against torch.func.jvp {err:.2e}")
    assert rel(inten, want_i) < 1e-14
    assert err <= 1e-12


def test_hand_jvp_equals_central_differences():
    """(I(x + eps v) - I(x - eps v)) / (2 eps), eps = 1e-6, on the smallest
    case: each tangent alone and all together, to 1e-7 normwise."""
    shape, eps = mm.END_TO_END_CASES[0], 1e-6
    c = mj.case(*shape)
    fly = c["fly"]
    for names in [("d_psi",), ("d_probe",), ("d_scan",), mj.TANGENT_NAMES]:
        (psi, probe, scan, Hprop), t = mj.as_model(c, names)
        dpsi, dprobe, dscan = (
            torch.zeros_like(x) if t[k] is None else t[k]
            for k, x in (("d_psi", psi), ("d_probe", probe), ("d_scan", scan)))
        # (the step crosses no integer)
        frac = scan - torch.floor(scan)
        assert float((frac - eps * dscan.abs()).min()) > 0
        assert float((frac + eps * dscan.abs()).max()) < 1
        with torch.no_grad():
            up = mm.intensity(psi + eps * dpsi, probe + eps * dprobe,
                              scan + eps * dscan, Hprop, fly)
            dn = mm.intensity(psi - eps * dpsi, probe - eps * dprobe,
                              scan - eps * dscan, Hprop, fly)
        got = mj.hand_jvp(psi, probe, scan, Hprop, fly=fly, **t)[1]
        err = rel(got, (up - dn) / (2 * eps))
        print(f"{shape} {names}: central differences {err:.2e}")
        assert err < 1e-7, (names, err)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape", mm.END_TO_END_CASES)
def test_adjoint_identity_on_the_model(shape, norm):
    """<u, J v> = <J^T u, v> to 1e-12 relative, J v by `hand_jvp` and J^T u by
    torch.autograd on the model (1.6e-15 at most when the bar was set)."""
    c = mj.case(*shape, norm=norm)
    m, t = mj.as_model(c)
    u = mj.f64(c["u"])
    dI = mj.hand_jvp(*m, fly=c["fly"], norm=norm, **t)[1]
    _, gpsi, gprobe, gscan = mm.autograd_gradients(*m, u, c["fly"], norm)
    left = aj.inner(u, dI)
    right = (aj.inner(gpsi, t["d_psi"]) + aj.inner(gprobe, t["d_probe"])
             + aj.inner(gscan, t["d_scan"]))
    print(f"{shape} {norm}: {left:.15e} {right:.15e} "
          f"({abs(left - right) / abs(left):.1e})")
    assert abs(left - right) <= 1e-12 * abs(left)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape", mm.END_TO_END_CASES)
def test_what_float32_alone_costs(shape, norm):
    """The same formulas in complex64 / float32 on the CPU: within 2e-6
    normwise of the float64 dI (6.8e-7 the worst measured when the bar was
    set, the margin for other FFT builds) -- the GPU tests hold the kernels to
    1e-5."""
    c = mj.case(*shape, norm=norm)
    m, t = mj.as_model(c)
    want = mj.hand_jvp(*m, fly=c["fly"], norm=norm, **t)[1]
    got = mj.hand_jvp_float32(*m, fly=c["fly"], norm=norm, **t)[1]
    assert got.dtype == torch.float32
    err = rel(got.to(am.F64), want)
    worst = float((got.to(am.F64) - want).abs().max() / want.abs().max())
    print(f"{shape} {norm}: float32 restatement normwise {err:.2e}, max-abs "
          f"{worst:.2e} of max |dI|")
    assert err <= 2e-6


# ------------------------------------------------------------------ refusals
def test_every_refusal():
    """Fails on the parent commit: the functions do not exist.  The argument
    checks come before any device work: CPU tensors reach every one of them,
    and are themselves refused last."""
    import tike_amd.operators as ops
    from tike_amd.autograd import (MAX_MODES, multislice_gauss_newton_product,
                                   multislice_intensity_jvp)
    pw, H, W, N, D = 8, 24, 31, 6, 2
    psi = torch.zeros((D, H, W), dtype=torch.complex64)
    probe = torch.zeros((1, 1, 2, pw, pw), dtype=torch.complex64)
    scan = torch.full((N, 2), 3.5)
    weight = torch.ones((N, pw, pw))
    functions = ((multislice_intensity_jvp, "multislice_intensity_jvp"),
                 (multislice_gauss_newton_product,
                  "multislice_gauss_newton_product"))
    with ops.Ptycho(probe_shape=pw, detector_shape=pw, nz=H, n=W,
                    **mm.optics(pw)) as op:
        for fn, name in functions:
            with pytest.raises(TypeError, match="psi must be a torch"):
                fn(op, psi.numpy(), probe, scan)
            with pytest.raises(TypeError, match="scan must be a torch"):
                fn(op, psi, probe, scan.numpy())
            with pytest.raises(TypeError,
                               match=name + ": probe must be torch.complex64"):
                fn(op, psi, probe.to(torch.complex128), scan)
            with pytest.raises(TypeError, match="scan must be torch.float32"):
                fn(op, psi, probe, scan.to(torch.float64))
            with pytest.raises(ValueError, match=r"psi \(D, H, W\)"):
                fn(op, psi[0], probe, scan)
            with pytest.raises(NotImplementedError, match="probe per position"):
                fn(op, psi, probe.expand(N, 1, 2, pw, pw), scan)
            with pytest.raises(ValueError, match=f"psi must be .D, {H}, {W}."):
                fn(op, psi[:, :, :30], probe, scan)
            with pytest.raises(ValueError, match="not a multiple of fly=4"):
                fn(op, psi, probe, scan, fly=4)
            many = torch.zeros((1, 1, MAX_MODES + 1, pw, pw),
                               dtype=torch.complex64)
            with pytest.raises(ValueError, match=f"at most {MAX_MODES}"):
                fn(op, psi, many, scan)
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
            # (one slice's tangent for an object of D)
            with pytest.raises(ValueError, match="d_psi must have the shape"):
                fn(op, psi, probe, scan, d_psi=psi[:1])
            with pytest.raises(ValueError, match="d_probe must have the shape"):
                fn(op, psi, probe, scan, d_probe=probe[:, :, :1])
            with pytest.raises(ValueError, match="d_scan must have the shape"):
                fn(op, psi, probe, scan, d_scan=scan[:-1])
            with pytest.raises(ValueError, match="d_psi lives on"):
                fn(op, psi, probe, scan, d_psi=psi.to("meta"))
            with pytest.raises(TypeError, match=name + ": psi lives"):
                fn(op, psi, probe, scan, d_psi=psi, d_probe=probe, d_scan=scan)
            # one slice is taken too, and refused as late
            with pytest.raises(TypeError, match="no CPU fallback"):
                fn(op, psi[:1], probe, scan, d_psi=psi[:1])
        fn = multislice_gauss_newton_product
        for bad in ((), ("psi", "psi"), ("scan", "weights")):
            with pytest.raises(ValueError,
                               match="multislice_gauss_newton_product: wrt "
                               "must name"):
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
    # several slices need probe window = detector; one slice does not
    with ops.Ptycho(probe_shape=pw, detector_shape=12, nz=H, n=W) as op:
        for fn, name in functions:
            with pytest.raises(ValueError,
                               match="detector_shape == probe_shape"):
                fn(op, psi, probe, scan, d_scan=scan)
            with pytest.raises(TypeError, match="no CPU fallback"):
                fn(op, psi[:1], probe, scan, d_scan=scan)


def test_single_slice_functions_keep_refusing_several_slices():
    """`intensity_jvp` and `gauss_newton_product` are unchanged."""
    import tike_amd.operators as ops
    from tike_amd.autograd import gauss_newton_product, intensity_jvp
    pw, H, W, N = 8, 24, 31, 6
    psi = torch.zeros((2, H, W), dtype=torch.complex64)
    probe = torch.zeros((1, 1, 2, pw, pw), dtype=torch.complex64)
    scan = torch.full((N, 2), 3.5)
    with ops.Ptycho(probe_shape=pw, detector_shape=pw, nz=H, n=W,
                    **mm.optics(pw)) as op:
        for fn in (intensity_jvp, gauss_newton_product):
            with pytest.raises(NotImplementedError, match="several slices"):
                fn(op, psi, probe, scan)


# ------------------------------------------------------------------- the ABI
def test_abi_has_the_new_entry():
    """Fails on the parent commit: the symbol does not exist."""
    import tike_amd._lib as L
    name = "tike_slice_wave_tangent"
    assert name in L.declared_symbols()
    assert len(L._PROTOTYPES[name]) == 15
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert L.ABI_VERSION >= 23


def test_abi_entry_checks_its_arguments_without_a_gpu():
    """Argument checks come before any launch.  Fails on the parent commit."""
    import tike_amd._lib as L
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (psi, dpsi, scan, dscan, beam, beam_per_scan, dbeam, dbeam_per_scan,
    #  dwave, nscan, S, pw, H, W, stream)
    ok = (p, p, p, p, p, 1, p, 1, p, 1, 1, 2, 4, 4, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return L.lib.tike_slice_wave_tangent(*args)
    for k in (0, 2, 4, 8):
        assert call(**{f"a{k}": None}) == L.ERR_ARG  # a NULL required array
    assert call(a9=-1) == L.ERR_ARG  # nscan
    assert call(a9=1 << 31) == L.ERR_ARG  # more than grid.x holds
    assert call(a10=0) == L.ERR_ARG  # S
    assert call(a10=17) == L.ERR_UNSUPPORTED  # S
    assert call(a11=0) == L.ERR_ARG  # pw
    assert call(a12=0) == L.ERR_ARG  # H
    assert call(a13=0) == L.ERR_ARG  # W
    # a plane of more items than one launch holds (no device: none at all)
    assert call(a11=1 << 30) == L.ERR_ARG
    assert call(a9=0) == 0  # no position: no launch
    assert call(a9=0, a1=None, a3=None, a6=None) == 0  # NULL tangents are fine
    assert call(a9=0, a5=0, a7=0) == 0  # shared operands


# --------------------------------------------------------- position recovery
def test_levenberg_marquardt_recovers_the_positions_on_the_model():
    """`autograd_multislice.problem(seed=RECOVERY["seed"])`, the two-slice
    problem on which 80 steps of Adam end at 0.43 of the starting error: four
    Levenberg-Marquardt steps on the positions alone (at most 20 CG
    iterations, damping 1e-3) on the float64 model end at 0.2 of the start or
    less with the cost 0.5 |r|^2 at 0.005 of its start or less (0.139 and
    0.00145 when the bars were set).  These are the margins of the GPU test's
    conditions."""
    p = mm.problem(seed=mm.RECOVERY["seed"])
    after, costs = mj.lm_on_model(p)
    r0 = am.rms(p["scan_start"], p["scan_true"])
    r = [am.rms(s, p["scan_true"]) for s in after]
    print(f"rms {r0:.4f} -> " + ", ".join(f"{x:.4f}" for x in r)
          + f" ({r[-1] / r0:.4f}); cost {costs[0]:.3e} -> {costs[-1]:.3e} "
          f"({costs[-1] / costs[0]:.5f})")
    assert np.isfinite(costs).all()
    assert r[-1] <= 0.2 * r0, (r0, r)
    assert costs[-1] <= 0.005 * costs[0], costs
