"""`tike_amd.autograd.cost`, `cost_jvp` and `cost_gauss_newton_product` without
a GPU: the float64 model of tests/autograd_cost.py against torch.autograd,
central differences and the algebra of a Gauss-Newton matrix; the ABI of the
two new entries; every refusal of `cost`; what float32 alone costs on the
end-to-end inputs of the GPU tests; and the Levenberg-Marquardt iteration on
Poisson-noisy fly-scan data whose result the GPU test is held against."""
import ctypes

import numpy as np
import pytest
import torch

import autograd_cost as ac
import autograd_eigen as ae
import autograd_eigen_jvp as aej
import autograd_jvp as aj
import autograd_model as am
import autograd_multislice_jvp as msj

rel = ae.rel

# (N, S, pw, det, H, W, fly) of the plain end-to-end GPU cases
PLAIN_SHAPES = [(8, 3, 16, 16, 40, 40, 2), (6, 2, 48, 64, 120, 120, 1),
                (4, 2, 100, 128, 240, 250, 2)]
SMALL = (6, 2, 8, 12, 24, 26, 2)


def _plain_case(shape, seed=0):
    """(form, m, tangents by name) of a plain shape."""
    N, S, pw, det, H, W, fly = shape
    c = aj.case(N, S, pw, det, H, W, fly, seed)
    (m, t) = aj.as_model(c)
    return ac.plain(det, fly), m, t


def _eigen_case():
    N, S, M, C, pw, det, H, fly = 6, 3, 2, 2, 8, 12, 26, 2
    c = dict(ae.inputs(N, S, M, C, pw, H, H, seed=3))
    c.update(aej.tangents(c, seed=5))
    t = aej.model_tangents(c)
    t = dict(d_psi=t["d_psi"], d_probe=t["d_probe"], d_scan=t["d_scan"],
             d_eigen_probe=t["d_eigen"], d_eigen_weights=t["d_weights"])
    return ac.eigen(det, fly), ae.model_of(c), t


def _multislice_case():
    c = msj.case(4, 2, 16, 40, 2, 2)
    m, t = msj.as_model(c)
    return ac.multislice(c["fly"]), m, t


FORMS = {"plain": lambda: _plain_case(SMALL), "eigen": _eigen_case,
         "multislice": _multislice_case}


def _counts_mask(form, m, masked):
    d = torch.from_numpy(ac.well_conditioned_counts(form, m)).to(ac.F64)
    det = d.shape[-1]
    mask = torch.from_numpy(ac.module_gap_mask(det)) if masked else None
    if masked:  # NaN under the mask: selected away
        d = torch.where(mask, d, torch.full_like(d, float("nan")))
    up = torch.from_numpy(ac.frame_weights(d.shape[0]))
    return d, mask, up


# ------------------------------------------------------------- the model
@pytest.mark.parametrize("model", ac.MODELS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("which", sorted(FORMS))
def test_hand_gradients_agree_with_torch_autograd(which, masked, model):
    """The table (the project's factor, guard included) followed by the
    form's hand-written backward against torch.autograd on the cost formula
    itself, in float64, NaN under the mask: 1e-8 normwise (the guard 1e-9 in
    the gaussian factor is what separates the two)."""
    form, m, _ = FORMS[which]()
    d, mask, up = _counts_mask(form, m, masked)
    costs, hand = ac.hand_gradients(form, m, d, mask, model, up)
    costs2, auto = ac.autograd_gradients(form, m, d, mask, model, up)
    assert torch.equal(costs, costs2) and bool(torch.isfinite(costs).all())
    for name in form.names:
        if auto[name] is None:
            continue
        err = rel(hand[name].numpy(), auto[name].numpy())
        print(f"{which} {model} masked={masked} {name}: {err:.2e}")
        assert err <= 1e-8, (name, err)


@pytest.mark.parametrize("model", ac.MODELS)
@pytest.mark.parametrize("which", sorted(FORMS))
def test_dcosts_agree_with_a_central_difference(which, model):
    """dcosts along all tangents against (cost(x + h v) - cost(x - h v)) / 2h
    of the model's cost, h = 1e-6 (the positions' fractions lie in [0.05,
    0.95]: no integer is crossed): 1e-6 of max |dcosts|."""
    form, m, t = FORMS[which]()
    d, mask, _ = _counts_mask(form, m, True)
    _, dcosts = ac.hand_jvp(form, m, t, d, mask, model)
    h = 1e-6
    frac = m[2] - torch.floor(m[2])
    assert 10 * h < float(frac.min()) and float(frac.max()) < 1 - 10 * h
    tangent = [t.get("d_" + name) for name in form.names]
    move = lambda s: tuple(
        x if k >= len(tangent) or tangent[k] is None else x + s * tangent[k]
        for k, x in enumerate(m))
    with torch.no_grad():
        fd = (ac.cost(form, move(h), d, mask, model)
              - ac.cost(form, move(-h), d, mask, model)) / (2 * h)
    err = float((dcosts - fd).abs().max() / dcosts.abs().max())
    print(f"{which} {model}: dcosts against a central difference {err:.2e}")
    assert err <= 1e-6


@pytest.mark.parametrize("model", ac.MODELS)
@pytest.mark.parametrize("which", sorted(FORMS))
def test_gauss_newton_product_is_symmetric_and_positive(which, model):
    """<u, G v> = <G u, v> to 1e-12 of its size, and <v, G v> >= 0, for random
    tangents of every input with a positive upstream and a mask."""
    form, m, v = FORMS[which]()
    det = (m[1].shape[-1] if which == "multislice" else
           ac.well_conditioned_counts(form, m).shape[-1])
    mask = torch.from_numpy(ac.module_gap_mask(det))
    frames = m[2].shape[0] // 2
    up = torch.from_numpy(np.abs(ac.frame_weights(frames)))
    rng = np.random.default_rng(8)
    u = {k: None if x is None else torch.from_numpy(
        rng.standard_normal(x.shape) + (1j * rng.standard_normal(x.shape)
                                        if x.is_complex() else 0)).to(x.dtype)
         for k, x in v.items()}
    Gv = ac.gauss_newton_product(form, m, v, mask, model, up)
    Gu = ac.gauss_newton_product(form, m, u, mask, model, up)
    pair = lambda G, w: sum(aj.inner(G[name], w["d_" + name])
                            for name in form.names
                            if w.get("d_" + name) is not None)
    uGv, vGu, vGv, uGu = pair(Gv, u), pair(Gu, v), pair(Gv, v), pair(Gu, u)
    print(f"{which} {model}: <u,Gv> {uGv:.12e} <Gu,v> {vGu:.12e} <v,Gv> "
          f"{vGv:.3e} <u,Gu> {uGu:.3e}")
    assert abs(uGv - vGu) <= 1e-12 * np.sqrt(vGv * uGu)
    assert vGv > 0 and uGu > 0


@pytest.mark.parametrize("shape", PLAIN_SHAPES)
@pytest.mark.parametrize("model", ac.MODELS)
def test_float32_alone_stays_inside_the_gpu_bars(shape, model):
    """On the end-to-end inputs of the GPU tests (masked, NaN under the mask,
    a signed upstream) the float32 restatement of the cost's backward stays
    within half of the GPU bars against the float64 model: 1e-5 normwise for
    the object and the probe, 1e-6 A_n for the positions.  The inputs, not
    the bars, were chosen for that: sqrt(d / I) is printed."""
    N, S, pw, det, H, W, fly = shape
    form, m, _ = _plain_case(shape)
    d, mask, up = _counts_mask(form, m, True)
    with torch.no_grad():
        ratio = torch.sqrt(ac._clean(d, mask) / form.intensity(m))[:, mask]
    _, hand = ac.hand_gradients(form, m, d, mask, model, up)
    low = ac.float32_gradients(m, det, fly, d, mask, model, up)
    epsi, eprobe = (rel(low[k].numpy(), hand[k].numpy())
                    for k in ("psi", "probe"))
    escan = float(((low["scan"] - hand["scan"]).abs() / hand["A_scan"]).max())
    q = np.quantile(ratio.numpy(), [0.01, 0.5, 0.99])
    print(f"{shape} {model}: sqrt(d/I) 1% {q[0]:.2f} median {q[1]:.2f} 99% "
          f"{q[2]:.2f}; float32 alone: psi {epsi:.2e} probe {eprobe:.2e} "
          f"scan / A_n {escan:.2e}")
    assert epsi <= 5e-6 and eprobe <= 5e-6 and escan <= 5e-7


# --------------------------------------------------------------- the ABI
def test_abi_has_the_new_entries():
    """Fails on the parent commit: the symbols do not exist."""
    import tike_amd._lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, arity in (("tike_cost_factor", 13), ("tike_cost_curvature", 16)):
        assert name in L.declared_symbols()
        assert len(L._PROTOTYPES[name]) == arity
        assert hasattr(lib, name)
    lib.tike_abi_version.restype = ctypes.c_int
    assert lib.tike_abi_version() == 25 == L.ABI_VERSION
    makefile = open(L.LIB_PATH.replace("libtike_amd.so", "Makefile")).read()
    assert "autograd_cost.hip" in makefile and "noise_model.h" in makefile


def _calls(fn, ok):
    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return fn(*args)
    return call


def test_abi_entries_check_their_arguments_without_a_gpu():
    """Argument checks come before any launch."""
    import tike_amd._lib as L
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (farplane, data, data_u16, measured, upstream, costs, table, nframe, P,
    #  npix, model, num_measured, stream)
    call = _calls(L.lib.tike_cost_factor,
                  (p, p, 0, None, None, p, p, 1, 2, 4, 0, 4, None))
    assert call(a0=None) == L.ERR_ARG  # farplane
    assert call(a1=None) == L.ERR_ARG  # data
    assert call(a7=-1) == L.ERR_ARG  # nframe
    assert call(a7=1 << 31) == L.ERR_ARG  # more than one launch holds
    assert call(a8=0) == L.ERR_ARG  # P
    assert call(a9=0) == L.ERR_ARG  # npix
    assert call(a10=2) == L.ERR_ARG and call(a10=-1) == L.ERR_ARG  # model
    assert call(a11=0) == L.ERR_ARG  # num_measured
    assert call(a7=0) == 0  # no frame: no launch
    # (farplane, dfarplane, data, data_u16, measured, upstream, costs, dcosts,
    #  table, nframe, P, npix, model, floor, num_measured, stream)
    call = _calls(L.lib.tike_cost_curvature,
                  (p, p, p, 0, None, None, p, p, p, 1, 2, 4, 1, 1e-9, 4, None))
    assert call(a0=None) == L.ERR_ARG and call(a1=None) == L.ERR_ARG
    assert call(a2=None) == L.ERR_ARG  # costs / dcosts without counts
    assert call(a2=None, a6=None) == L.ERR_ARG
    assert call(a9=-1) == L.ERR_ARG and call(a9=1 << 31) == L.ERR_ARG
    assert call(a10=0) == L.ERR_ARG and call(a11=0) == L.ERR_ARG
    assert call(a12=2) == L.ERR_ARG  # model
    for bad in (-1e-9, float("inf"), float("nan")):
        assert call(a13=bad) == L.ERR_ARG  # floor
    assert call(a14=0) == L.ERR_ARG  # num_measured
    assert call(a9=0) == 0 and call(a9=0, a2=None, a6=None, a7=None) == 0


# ---------------------------------------------------------------- refusals
def test_every_refusal_of_cost():
    """Raised before any device use: CPU tensors reach every refusal and are
    themselves refused last."""
    import tike_amd.operators as ops
    from tike_amd.autograd import (cost, cost_gauss_newton_product, cost_jvp)
    pw, det, H, W, N, S = 8, 12, 24, 31, 6, 2
    psi = torch.zeros((1, H, W), dtype=torch.complex64)
    probe = torch.zeros((1, 1, S, pw, pw), dtype=torch.complex64)
    scan = torch.full((N, 2), 3.5)
    data = torch.ones((N // 2, det, det))
    mask = torch.ones((det, det), dtype=torch.bool)
    with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:
        run = lambda **k: cost(op, k.pop("data", data), k.pop("psi", psi),
                               k.pop("probe", probe), scan,
                               **dict(dict(fly=2), **k))
        with pytest.raises(TypeError, match="data must be a torch"):
            run(data=data.numpy())
        with pytest.raises(TypeError, match="data must be torch.float32 or"):
            run(data=data.double())
        with pytest.raises(ValueError, match="data must be"):
            run(data=data[:, :-1])
        with pytest.raises(ValueError, match="data must be"):
            run(data=data[:-1])
        with pytest.raises(ValueError, match="data must be"):
            run(data=data[0])
        with pytest.raises(ValueError, match="measured_pixels must be"):
            run(measured_pixels=mask[:-1])
        with pytest.raises(TypeError, match="measured_pixels must be torch"):
            run(measured_pixels=mask.float())
        with pytest.raises(ValueError, match="measures no pixel"):
            run(measured_pixels=torch.zeros_like(mask))
        with pytest.raises(ValueError, match="unknown noise model"):
            run(model="laplace")
        weights = torch.ones((N, 1, S))
        with pytest.raises(NotImplementedError,
                           match="several slices .* with eigen probes"):
            run(psi=psi.expand(2, H, W), eigen_weights=weights)
        # the refusals of the form go on unchanged
        with pytest.raises(ValueError, match="not a multiple of fly=4"):
            cost(op, data, psi, probe, scan, fly=4)
        with pytest.raises(NotImplementedError, match="probe per position"):
            run(probe=probe.expand(N, 1, S, pw, pw))
        with pytest.raises(ValueError, match="needs detector_shape == probe"):
            run(psi=psi.expand(2, H, W))  # probe window != detector
        with pytest.raises(ValueError, match="eigen_probe without"):
            run(eigen_probe=torch.zeros((1, 1, 1, pw, pw),
                                        dtype=torch.complex64))
        with pytest.raises(TypeError, match="no CPU fallback"):
            run(measured_pixels=mask, model="poisson")
        # the two other functions share the checks, and add their own
        with pytest.raises(ValueError, match="unknown noise model"):
            cost_jvp(op, data, psi, probe, scan, model="x", fly=2)
        with pytest.raises(ValueError, match="d_scan must have the shape"):
            cost_jvp(op, data, psi, probe, scan, d_scan=scan[:-1], fly=2)
        with pytest.raises(ValueError, match="without eigen_weights"):
            cost_jvp(op, data, psi, probe, scan, d_eigen_weights=weights,
                     fly=2)
        gn = lambda **k: cost_gauss_newton_product(
            op, data, psi, probe, scan, d_scan=scan, fly=2, **k)
        with pytest.raises(ValueError, match="wrt must name"):
            gn(wrt=("eigen_weights",))
        with pytest.raises(ValueError, match="floor must be"):
            gn(floor=-1.0)
        with pytest.raises(ValueError, match="upstream must be"):
            gn(upstream=torch.ones(N))
        with pytest.raises(TypeError, match="upstream must be torch.float32"):
            gn(upstream=torch.ones(N // 2, dtype=torch.float64))
        with pytest.raises(TypeError, match="no CPU fallback"):
            gn()


# ------------------------------------------------------ position recovery
def test_levenberg_marquardt_on_the_model():
    """`noisy_problem()`: 196 positions, fly = 2, start off by up to 0.3 px,
    Poisson counts (gain 1e4: up to 3e5 counts in a pixel, 89 % of the pixels
    empty).  Four Levenberg-Marquardt steps of at most 20 CG iterations on the
    poisson cost, entirely in the float64 model: the RMS position error goes
    0.2433 -> 0.0850, 0.0612, 0.0588, 0.0583 px and the cost falls at every
    step.  (The noise sets the floor: at gain 1e3 the same iteration ends at
    0.156 px with a cost BELOW that of the true positions.)"""
    p = ac.noisy_problem()
    after, costs = ac.lm_on_model(p)
    r0 = am.rms(p["scan_start"], p["scan_true"])
    r = [am.rms(s, p["scan_true"]) for s in after]
    print(f"LM on the float64 model: rms {r0:.4f} -> "
          + ", ".join(f"{x:.4f}" for x in r) + "; F "
          + ", ".join(f"{c:.4f}" for c in costs))
    assert np.isfinite(costs).all()
    assert all(b < a for a, b in zip(costs, costs[1:]))
    assert abs(r[-1] - ac.LM_MODEL_RMS) <= 5e-5, r
