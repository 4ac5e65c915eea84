"""`tike_amd.autograd.cost`, `cost_jvp` and `cost_gauss_newton_product` on the
GPU: the two new entries on their own, the three functions end to end against
the float64 model (tests/autograd_cost.py) for every form of the model and
against the composition they replace (`intensity` + a loss in torch,
`*_gauss_newton_product(weight=)`), detector-like counts, a dark frame,
chunking, and Levenberg-Marquardt position recovery on Poisson-noisy fly-scan
data.

Every figure a bar is set on is printed before it is asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import autograd_cost as ac
import autograd_model as am
from util import OP_NORMWISE, relerr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_ID = {"gaussian": 0, "poisson": 1}


def _rc(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(
        np.complex64)


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(
        "cuda")


def _host(x):
    return None if x is None else x.detach().cpu().numpy()


# ------------------------------------------------------------ the entries
# nframe, P, npix: P of 1, 3, 8 and 17 (the entries keep no plane in
# registers: there is no limit for P to straddle); npix % 4 of 1, 0, 3, 3, 0,
# 3; npix < 4; one and many sweeps of the frame's workgroup
ENTRY_CASES = [(3, 1, 169), (2, 3, 256), (2, 8, 403), (2, 3, 1027),
               (1, 8, 16384), (2, 1, 3), (2, 17, 403)]
ENTRY_VARIANTS = [(model, masked, u16) for model in ac.MODELS
                  for masked in (False, True) for u16 in (False, True)]


def _entry_inputs(nframe, P, npix, masked, u16):
    """far, dfar (3 x complex normal: I of some tens), counts = I x uniform
    (0.1, 0.4) -- the factor l' stays away from 0, so that its own rounding
    does not outweigh the bar of dcosts, which is stated in |l'| -- rounded
    for uint16, NaN under the mask for float32; a mask that leaves about
    three pixels in four (and at least one); a signed upstream."""
    rng = np.random.default_rng(nframe + 3 * P + npix)
    far = (3 * _rc(rng, nframe, P, npix)).astype(np.complex64)
    dfar = _rc(rng, nframe, P, npix)
    inten = (np.abs(far.astype(np.complex128))**2).sum(axis=1)
    counts = inten * rng.uniform(0.1, 0.4, inten.shape)
    mask = None
    if masked:
        mask = rng.random(npix) < 0.75
        mask[rng.integers(npix)] = False
        mask[(rng.integers(npix) + 1) % npix] = True
    if u16:
        data = np.minimum(np.rint(counts), 65535).astype(np.uint16)
    else:
        data = counts.astype(np.float32)
        if masked:
            data[:, ~mask] = np.nan
    upstream = ac.frame_weights(nframe, seed=P)
    return far, dfar, data, mask, upstream


def _model_factor(I32, data, mask, model):
    """(l', |.| scale 1 + ratio) in float64 at the float32 intensity."""
    import torch
    I = torch.from_numpy(I32.astype(np.float64))
    m = None if mask is None else torch.from_numpy(mask)
    d = ac._clean(torch.from_numpy(data.astype(np.float64)), m)
    lp = ac.lprime(I, d, model).numpy()
    return lp, 2 - lp  # 1 + sqrt(d) / (sqrt(I) + 1e-9), or with d / (I + 1e-9)


def _launch_factor(far_d, data_d, u16, mask_d, up_d, costs, table, nframe, P,
                   npix, model, nm):
    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    check(lib.tike_cost_factor(
        A.ptr(far_d), A.ptr(data_d), int(u16), A.ptr(mask_d), A.ptr(up_d),
        A.ptr(costs), A.ptr(table), nframe, P, npix, MODEL_ID[model], nm,
        A.stream_ptr()), "tike_cost_factor")


def _fly_costs(far_d, data_d, u16, mask_d, nframe, P, npix, model, nm):
    """costs of tike_fly_farplane_gradient(apply_gradient=0), and its
    intensity, on the same far plane; npix must be a square (the entry takes
    det)."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    det = int(round(np.sqrt(npix)))
    assert det * det == npix
    costs = torch.empty(nframe, dtype=torch.float32, device="cuda")
    inten = torch.empty((nframe, npix), dtype=torch.float32, device="cuda")
    check(lib.tike_fly_farplane_gradient(
        A.ptr(far_d), A.ptr(data_d), int(u16), A.ptr(mask_d), A.ptr(inten),
        A.ptr(costs), nframe, P, 1, det, MODEL_ID[model], 0, 1.0, nm,
        A.stream_ptr()), "tike_fly_farplane_gradient")
    return costs.cpu().numpy(), inten.cpu().numpy()


def _intensity32(far_d, nframe, P, npix):
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    inten = torch.empty((nframe, npix), dtype=torch.float32, device="cuda")
    check(lib.tike_intensity(A.ptr(far_d), A.ptr(inten), nframe, P, npix,
                             A.stream_ptr()), "tike_intensity")
    return inten.cpu().numpy()


@pytest.mark.parametrize("model,masked,u16", ENTRY_VARIANTS)
@pytest.mark.parametrize("nframe,P,npix", ENTRY_CASES)
def test_cost_factor(nframe, P, npix, model, masked, u16):
    """costs: the bits of tike_fly_farplane_gradient(apply_gradient=0) on the
    same far plane where that entry can be asked (it takes det: npix a
    square -- 169, 256, 16384; its intensity is also that of tike_intensity
    there), and within 1e-6 of the float64 sum of the terms' absolute
    parts (I + d, or I + d |log I|: what the terms are differences of)
    everywhere.  The table: exactly 0 under the mask; on measured pixels
    |err| <= 1e-6 |upstream_f| (1 + sqrt(d) / (sqrt(I) + 1e-9)) / num_measured
    (poisson: d / (I + 1e-9)) against the float64 factor at the FLOAT32
    intensity.  Two calls give the same bits; a NULL output leaves the other
    as it is; the rows in front of and behind the outputs and the far plane
    are untouched."""
    import torch
    far, _, data, mask, upstream = _entry_inputs(nframe, P, npix, masked, u16)
    nm = npix if mask is None else int(mask.sum())
    far_d, data_d, up_d = _dev(far), _dev(data), _dev(upstream)
    mask_d = None if mask is None else _dev(mask.astype(np.uint8))
    out = []
    for which in ("both", "both", "costs", "table"):
        costs = torch.full((nframe + 2,), 7.0, dtype=torch.float32,
                           device="cuda")
        table = torch.full((nframe + 2, npix), 7.0, dtype=torch.float32,
                           device="cuda")
        _launch_factor(far_d, data_d, u16, mask_d, up_d,
                       costs[1:] if which != "table" else None,
                       table[1:] if which != "costs" else None, nframe, P,
                       npix, model, nm)
        out.append((costs.cpu().numpy(), table.cpu().numpy()))
        assert out[-1][0][0] == 7.0 == out[-1][0][-1]
        assert np.all(out[-1][1][[0, -1]] == 7.0)
    assert np.array_equal(far_d.cpu().numpy(), far)
    for k in (0, 1):  # two calls; NULL outputs
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True)
    assert np.array_equal(out[2][0], out[0][0]) and np.all(out[2][1] == 7.0)
    assert np.array_equal(out[3][1], out[0][1]) and np.all(out[3][0] == 7.0)
    costs, table = out[0][0][1:-1], out[0][1][1:-1]
    I32 = _intensity32(far_d, nframe, P, npix)
    square = int(round(np.sqrt(npix)))**2 == npix
    if square:
        fly_costs, fly_inten = _fly_costs(far_d, data_d, u16, mask_d, nframe,
                                          P, npix, model, nm)
        assert np.array_equal(fly_inten, I32)
        assert np.array_equal(costs, fly_costs), (costs, fly_costs)
    lp, scale = _model_factor(I32, data, mask, model)
    sel = np.ones(npix, bool) if mask is None else mask
    terms = ac.terms(torch.from_numpy(I32.astype(np.float64)),
                     torch.from_numpy(np.where(sel, data, 0).astype(
                         np.float64)), model).numpy()
    want_costs = terms[:, sel].sum(axis=1) / nm
    clean = np.where(sel, data, 0).astype(np.float64)
    parts = I32 + clean * (1 if model == "gaussian" else
                           np.abs(np.log(I32.astype(np.float64) + 1e-9)))
    cost_err = np.abs(costs - want_costs) / (parts[:, sel].sum(axis=1) / nm)
    want = upstream[:, None].astype(np.float64) * lp / nm
    ratio = np.abs(table - want)[:, sel] / (
        np.abs(upstream[:, None]) * scale / nm)[:, sel]
    print(f"cost factor ({nframe}, {P}, {npix}) {model} masked={masked} "
          f"u16={u16}: costs {'= fly bits, ' if square else ''}|err| / sum "
          f"parts {cost_err.max():.2e}; table max |err| / bound scale "
          f"{ratio.max():.2e}")
    assert np.all(table[:, ~sel] == 0.0)
    assert np.all(np.isfinite(table)) and np.all(np.isfinite(costs))
    assert np.all(cost_err <= 1e-6), cost_err
    assert np.all(ratio <= 1e-6), ratio.max()


@pytest.mark.parametrize("model,masked,u16", ENTRY_VARIANTS)
@pytest.mark.parametrize("nframe,P,npix", ENTRY_CASES)
def test_cost_curvature(nframe, P, npix, model, masked, u16):
    """The table: exactly 0 under the mask, and |err| <= 1e-6 w sum_j |far_j|
    |dfar_j| with w = |upstream_f| c / (num_measured (I + floor)) in float64 at
    the FLOAT32 intensity -- the bar of `test_intensity_tangent` carried
    through one more multiply.  costs: the bits of tike_cost_factor.  dcosts:
    |err| <= 1e-6 sum_p |l'| sum_j |far_j| |dfar_j| / num_measured against
    the float64 sum with l' at the float32 intensity.  NULL outputs are not
    written and change nothing else (without costs and dcosts the counts may
    be NULL too); two calls give the same bits; neither far plane is
    written."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    far, dfar, data, mask, upstream = _entry_inputs(nframe, P, npix, masked,
                                                    u16)
    nm = npix if mask is None else int(mask.sum())
    floor = 1e-9
    far_d, dfar_d, data_d, up_d = (_dev(far), _dev(dfar), _dev(data),
                                   _dev(upstream))
    mask_d = None if mask is None else _dev(mask.astype(np.uint8))
    ref_costs = torch.empty(nframe, dtype=torch.float32, device="cuda")
    _launch_factor(far_d, data_d, u16, mask_d, up_d, ref_costs, None, nframe,
                   P, npix, model, nm)
    out = []
    for which in ("all", "all", "table", "table-nodata", "sums"):
        costs = torch.full((nframe + 2,), 7.0, dtype=torch.float32,
                           device="cuda")
        dcosts = torch.full((nframe + 2,), 7.0, dtype=torch.float32,
                            device="cuda")
        table = torch.full((nframe + 2, npix), 7.0, dtype=torch.float32,
                           device="cuda")
        sums = which in ("all", "sums")
        check(lib.tike_cost_curvature(
            A.ptr(far_d), A.ptr(dfar_d),
            None if which == "table-nodata" else A.ptr(data_d), int(u16),
            A.ptr(mask_d), A.ptr(up_d), A.ptr(costs[1:]) if sums else None,
            A.ptr(dcosts[1:]) if sums else None,
            None if which == "sums" else A.ptr(table[1:]), nframe, P, npix,
            MODEL_ID[model], floor, nm, A.stream_ptr()),
            "tike_cost_curvature")
        out.append(tuple(x.cpu().numpy() for x in (costs, dcosts, table)))
        for x in out[-1]:
            assert np.all(x[[0, -1]] == 7.0)
    assert np.array_equal(far_d.cpu().numpy(), far)
    assert np.array_equal(dfar_d.cpu().numpy(), dfar)
    for k in range(3):
        assert np.array_equal(out[0][k], out[1][k])
    for k in (2, 3):  # table alone, with and without the counts
        assert np.array_equal(out[k][2], out[0][2])
        assert np.all(out[k][0] == 7.0) and np.all(out[k][1] == 7.0)
    assert np.array_equal(out[4][0], out[0][0])
    assert np.array_equal(out[4][1], out[0][1]) and np.all(out[4][2] == 7.0)
    costs, dcosts, table = (x[1:-1] for x in out[0])
    assert np.array_equal(costs, ref_costs.cpu().numpy())
    I32 = _intensity32(far_d, nframe, P, npix).astype(np.float64)
    f, d = far.astype(np.complex128), dfar.astype(np.complex128)
    dI = 2 * (f.conj() * d).real.sum(axis=1)
    scale = (np.abs(f) * np.abs(d)).sum(axis=1)
    sel = np.ones(npix, bool) if mask is None else mask
    w = (np.abs(upstream[:, None]).astype(np.float64) * ac.CURVATURE[model]
         / (nm * (I32 + floor)))
    want = np.sign(upstream[:, None]) * w * dI
    ratio = np.abs(table - want)[:, sel] / (w * scale)[:, sel]
    lp, _ = _model_factor(I32.astype(np.float32), data, mask, model)
    want_d = (lp * dI)[:, sel].sum(axis=1) / nm
    bound_d = 1e-6 * (np.abs(lp) * scale)[:, sel].sum(axis=1) / nm
    err_d = np.abs(dcosts - want_d)
    print(f"cost curvature ({nframe}, {P}, {npix}) {model} masked={masked} "
          f"u16={u16}: table max |err| / (w sum |far||dfar|) "
          f"{ratio.max():.2e}; dcosts max |err| / bound "
          f"{(err_d / bound_d).max():.2e} of 1")
    assert np.all(table[:, ~sel] == 0.0) and np.all(np.isfinite(table))
    assert np.all(ratio <= 1e-6), ratio.max()
    assert np.all(err_d <= bound_d), (err_d, bound_d)


# ------------------------------------------------------------- end to end
def _operator(c, norm="ortho"):
    import tike_amd.operators as ops
    return ops.Ptycho(norm=norm, **c["operator"])


def _inputs(c, masked, u16=False):
    """(data, mask, upstream host arrays; device keyword arguments of `cost`
    with leaves that require a gradient; device tangents)."""
    data, mask, up = ac.counts_of(c, masked)
    if u16:
        data = np.minimum(np.rint(np.nan_to_num(data)), 65535).astype(
            np.uint16)
    leaves = {k: None if v is None else _dev(v).requires_grad_(True)
              for k, v in c["host"].items()}
    kw = dict(leaves, fly=c["fly"])
    if mask is not None:
        kw["measured_pixels"] = _dev(mask)
    tangents = {k: _dev(v) for k, v in c["host_t"].items()}
    return data, mask, up, kw, tangents


def _model_of(c, data, mask, up, model):
    """The float64 model's (costs, gradients, dcosts, sum |l'| |dI| / nm,
    Gauss-Newton product) of a case."""
    import torch
    form, m, t = c["form"], c["m"], c["t"]
    d = torch.from_numpy(data.astype(np.float64))
    mk = None if mask is None else torch.from_numpy(mask)
    upt = torch.from_numpy(up)
    costs, grads = ac.hand_gradients(form, m, d, mk, model, upt)
    with torch.no_grad():
        I, dI = form.jvp(m, t)
        dcosts = ac.dcosts_of(I, dI, d, mk, model)
        scale = ac._select(
            mk, ac.lprime(I, ac._clean(d, mk), model).abs() * dI.abs()).sum(
                dim=(1, 2)) / ac.num_measured(mk, c["det"])
    gn = ac.gauss_newton_product(form, m, t, mk, model, upt)
    return costs.numpy(), grads, dcosts.numpy(), scale.numpy(), gn


def _grad_errors(got, want, names):
    """{name: error figure}: normwise for the complex inputs, max |err| / A
    for the positions and the weights."""
    out = {}
    for name in names:
        if want.get(name) is None or got.get(name) is None:
            continue
        g, w = got[name], want[name].numpy()
        if name in ("scan", "eigen_weights"):
            A = want["A_" + ("scan" if name == "scan" else "weights")].numpy()
            live = A > 0
            assert np.all(g[~live] == w[~live]), name  # (nothing to sum)
            out[name] = float((np.abs(g - w)[live] / A[live]).max())
        else:
            out[name] = relerr(g, w)
    return out


BARS = dict(psi=OP_NORMWISE, probe=OP_NORMWISE, eigen_probe=OP_NORMWISE,
            scan=1e-6, eigen_weights=1e-6)


def _assert_grads(errors, what, factor=1.0):
    print(what + ": " + ", ".join(f"{k} {v:.2e}" for k, v in errors.items()))
    for k, v in errors.items():
        assert v <= factor * BARS[k], (what, k, v)


def _run_all(c, data, kw, tangents, up, model):
    """(costs, gradients by name, dcosts, Gauss-Newton product by name) of the
    three functions on the device, host arrays."""
    import torch

    from tike_amd import autograd
    data_d, up_d = _dev(data), _dev(up)
    names = c["form"].names
    with _operator(c) as op:
        args = (op, data_d, kw["psi"], kw["probe"], kw["scan"])
        rest = {k: v for k, v in kw.items()
                if k not in ("psi", "probe", "scan")}
        costs = autograd.cost(*args, model=model, **rest)
        assert costs.dtype == torch.float32 and costs.ndim == 1
        leaves = [kw[k] for k in names if kw.get(k) is not None]
        grads = torch.autograd.grad((costs * up_d).sum(), leaves)
        grads = dict(zip([k for k in names if kw.get(k) is not None], grads))
        costs2, dcosts = autograd.cost_jvp(*args, model=model, **rest,
                                           **tangents)
        assert torch.equal(costs2, costs.detach())
        wrt = tuple(k for k in names if kw.get(k) is not None)
        gn = autograd.cost_gauss_newton_product(
            *args, model=model, upstream=up_d, wrt=wrt, **rest, **tangents)
    return (_host(costs), {k: _host(v) for k, v in grads.items()},
            _host(dcosts), dict(zip(wrt, map(_host, gn))))


@pytest.mark.parametrize("model", ac.MODELS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind,shape", ac.CASES)
def test_cost_vs_model(kind, shape, masked, model):
    """Every form, both noise models, with and without a module-gap mask (NaN
    under it), a signed non-uniform upstream ((cost * weights).sum()): costs
    within 1e-5 relative; psi, probe and eigen_probe gradients normwise 1e-5;
    scan and weight gradients 1e-6 A per entry; dcosts within 1e-5 of
    sum |l'| |dI| / num_measured; the Gauss-Newton product at the bars of the
    gradients (A for its own table).  The costs of `cost_jvp` have the bits of
    `cost`."""
    c = ac.case(kind, shape)
    data, mask, up, kw, tangents = _inputs(c, masked)
    costs, grads, dcosts, gn = _run_all(c, data, kw, tangents, up, model)
    want_costs, want, want_d, scale_d, want_gn = _model_of(c, data, mask, up,
                                                           model)
    cerr = np.abs(costs - want_costs) / np.abs(want_costs)
    derr = np.abs(dcosts - want_d) / scale_d
    what = f"{kind} {shape} {model} masked={masked}"
    print(f"{what}: costs max rel {cerr.max():.2e}; dcosts max |err| / sum "
          f"|l'||dI| {derr.max():.2e}")
    assert np.all(np.isfinite(costs)) and np.all(cerr <= 1e-5), cerr
    assert np.all(derr <= 1e-5), derr
    _assert_grads(_grad_errors(grads, want, c["form"].names),
                  what + " gradients")
    _assert_grads(_grad_errors(gn, want_gn, c["form"].names),
                  what + " Gauss-Newton product")


@pytest.mark.parametrize("model", ac.MODELS)
def test_uint16_counts_and_every_norm(model):
    """uint16 counts give the bits of the same counts in float32; the
    operator's norm is honoured ("forward" and "backward" against the model
    at the bars of `test_cost_vs_model`)."""
    import torch

    from tike_amd import autograd
    kind, shape = ac.CASES[0]
    c = ac.case(kind, shape)
    data, mask, up, kw, _ = _inputs(c, True, u16=True)
    as_float = np.where(mask, data.astype(np.float32), np.float32("nan"))
    got = []
    with _operator(c) as op:
        for d in (data, as_float):
            costs = autograd.cost(op, _dev(d), kw["psi"], kw["probe"],
                                  kw["scan"], model=model, fly=c["fly"],
                                  measured_pixels=kw["measured_pixels"])
            got.append([_host(costs)] + [_host(g) for g in torch.autograd.grad(
                (costs * _dev(up)).sum(), [kw["scan"], kw["probe"]])])
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])  # scan: no atomics
    assert relerr(got[0][2], got[1][2]) <= 1e-6  # probe: float atomics
    N, S, pw, det, H, W, fly = shape
    for norm in ("forward", "backward"):
        form = ac.plain(det, fly, norm)
        cn = dict(c, form=form)
        d, mk, upn, kwn, t = _inputs(cn, True)
        data_d, up_d = _dev(d), _dev(upn)
        with _operator(c, norm) as op:
            costs = autograd.cost(op, data_d, kwn["psi"], kwn["probe"],
                                  kwn["scan"], model=model, fly=fly,
                                  measured_pixels=kwn["measured_pixels"])
            grads = torch.autograd.grad(
                (costs * up_d).sum(),
                [kwn["psi"], kwn["probe"], kwn["scan"]])
        want_costs, want = ac.hand_gradients(
            form, c["m"], torch.from_numpy(d.astype(np.float64)),
            torch.from_numpy(mk), model, torch.from_numpy(upn))
        cerr = np.abs(_host(costs) - want_costs.numpy()) / np.abs(
            want_costs.numpy())
        print(f"norm={norm} {model}: costs max rel {cerr.max():.2e}")
        assert np.all(cerr <= 1e-5)
        _assert_grads(_grad_errors(dict(zip(form.names, map(_host, grads))),
                                   want, form.names), f"norm={norm} {model}")


# ----------------------------------- against the composition, on the device
def _torch_loss(inten, data, mask, model, nm):
    """The per-frame cost written in torch on an intensity: the mask by
    torch.where on the counts AND on the terms, the guard 1e-9 where the
    formula has one (the poisson logarithm; the gaussian (sqrt(I) -
    sqrt(d))^2 is the line of examples/reconstruct_autograd.py)."""
    import torch
    zero = torch.zeros_like(inten)
    d = data.to(torch.float32)
    d = d if mask is None else torch.where(mask, d, zero)
    if model == "gaussian":
        terms = (torch.sqrt(inten) - torch.sqrt(d))**2
    else:
        terms = inten - d * torch.log(inten + 1e-9)
    terms = terms if mask is None else torch.where(mask, terms, zero)
    return terms.sum(dim=(1, 2)) / nm


def _composition(c, op, data_d, kw, up_d, model, tangents=None, floor=1e-9):
    """(costs, gradients by name[, product by name]) of the parent's route:
    the form's `intensity`, a torch loss, torch's backward; and the form's
    `*_gauss_newton_product(weight=W)` with W formed in torch."""
    import torch

    from tike_amd import autograd
    names = [k for k in c["form"].names if kw.get(k) is not None]
    mask = kw.get("measured_pixels")
    nm = c["det"]**2 if mask is None else int(mask.sum())
    eigen = {k: kw[k] for k in ("eigen_probe", "eigen_weights") if k in kw}
    many = kw["psi"].shape[0] > 1
    run = autograd.multislice_intensity if many else autograd.intensity
    inten = run(op, kw["psi"], kw["probe"], kw["scan"], fly=c["fly"], **eigen)
    costs = _torch_loss(inten, data_d, mask, model, nm)
    grads = torch.autograd.grad((costs * up_d).sum(), [kw[k] for k in names])
    out = [_host(costs), dict(zip(names, map(_host, grads)))]
    if tangents is not None:
        with torch.no_grad():
            W = (up_d[:, None, None] * ac.CURVATURE[model]
                 / (nm * (inten.detach() + floor)))
            if mask is not None:
                W = torch.where(mask, W, torch.zeros_like(W))
        product = (autograd.multislice_gauss_newton_product if many else
                   autograd.eigen_gauss_newton_product if eigen else
                   autograd.gauss_newton_product)
        gn = product(op, kw["psi"], kw["probe"], kw["scan"], weight=W,
                     fly=c["fly"], wrt=tuple(names), **eigen, **tangents)
        out.append(dict(zip(names, map(_host, gn))))
    return out


def _pair_errors(a, b, want, names):
    """Error figures of a against b in the units of `_grad_errors` (A from
    the model)."""
    out = {}
    for name in names:
        if name not in a:
            continue
        if name in ("scan", "eigen_weights"):
            A = want["A_" + ("scan" if name == "scan" else "weights")].numpy()
            live = A > 0
            out[name] = float((np.abs(a[name] - b[name])[live]
                               / A[live]).max())
        else:
            out[name] = relerr(a[name], b[name])
    return out


@pytest.mark.parametrize("model", ac.MODELS)
@pytest.mark.parametrize("kind,shape", [ac.CASES[0], ac.CASES[1], ac.CASES[2],
                                        ac.CASES[4], ac.CASES[5]])
def test_cost_vs_the_composition_on_the_device(kind, shape, model,
                                               monkeypatch):
    """`cost` and its gradients against `intensity` followed by the same loss
    in torch, and `cost_gauss_newton_product` against
    `*_gauss_newton_product(weight=W)` with W from `intensity` in torch, masked
    with NaN under the mask: twice the bars of `test_cost_vs_model` (both
    routes are float32 against the same model).  wrt=("scan",) launches no
    object scatter and gives the bits of the scan part of the full
    product."""
    from tike_amd import autograd
    c = ac.case(kind, shape)
    data, mask, up, kw, tangents = _inputs(c, True)
    costs, grads, _, gn = _run_all(c, data, kw, tangents, up, model)
    _, want, _, _, want_gn = _model_of(c, data, mask, up, model)
    data_d, up_d = _dev(data), _dev(up)
    scatters = []
    scatter = autograd.lib.tike_scatter_patches
    with _operator(c) as op:
        ccosts, cgrads, cgn = _composition(c, op, data_d, kw, up_d, model,
                                           tangents)
        monkeypatch.setattr(autograd.lib, "tike_scatter_patches",
                            lambda *a: scatters.append(1) or scatter(*a))
        rest = {k: v for k, v in kw.items()
                if k not in ("psi", "probe", "scan")}
        (only,) = autograd.cost_gauss_newton_product(
            op, data_d, kw["psi"], kw["probe"], kw["scan"], model=model,
            upstream=up_d, wrt=("scan",), **rest, **tangents)
        assert not scatters
        autograd.cost_gauss_newton_product(
            op, data_d, kw["psi"], kw["probe"], kw["scan"], model=model,
            upstream=up_d, wrt=("psi",), **rest, **tangents)
        assert scatters
    assert np.array_equal(_host(only), gn["scan"])
    cerr = np.abs(costs - ccosts) / np.abs(ccosts)
    what = f"{kind} {shape} {model} against the composition"
    print(f"{what}: costs max rel {cerr.max():.2e}")
    assert np.all(cerr <= 2e-5)
    names = c["form"].names
    _assert_grads(_pair_errors(grads, cgrads, want, names),
                  what + ", gradients", 2.0)
    _assert_grads(_pair_errors(gn, cgn, want_gn, names),
                  what + ", Gauss-Newton product", 2.0)


# ------------------------------------------------------ detector-like counts
def _detector_case():
    """16 positions (8 frames, fly = 2) of `autograd_model.problem()` with a
    probe of sqrt(2000) times the amplitude: the model's intensities span six
    decades and more (1e-2 ... 6e4), the Poisson counts drawn from them are
    mostly zero and fit uint16; the model is evaluated at the START positions
    (off by up to 0.3 px), so d / I is far from 1 where either is small.
    pw = det = 32."""
    p = ac.noisy_problem(gain=2000.0)
    N, fly, det = 16, p["fly"], p["det"]
    H = p["psi"].shape[-1]
    host = dict(psi=p["psi"], probe=p["probe"],
                scan=np.ascontiguousarray(p["scan_start"][:N]))
    data = p["data"][:N // fly]
    assert data.max() <= 65535 and (data == 0).mean() > 0.5
    form = ac.plain(det, fly)
    return dict(form=form, m=am.as_model(host["psi"], host["probe"],
                                         host["scan"]), t={}, host=host,
                host_t={}, det=det, fly=fly,
                operator=dict(probe_shape=det, detector_shape=det, nz=H, n=H)
                ), data.astype(np.uint16)


@pytest.mark.parametrize("model", ac.MODELS)
def test_detector_like_counts(model):
    """uint16 counts over the range a detector delivers, mostly zero, a
    module gap (the float32 copy with NaN under the gap gives the same bits).
    The error against the float64 model is MEASURED: the bound of every figure
    is the larger of the bar of `test_cost_vs_model` and twice the error of
    the composition (`intensity` + the loss in torch) against the same model
    on the same inputs.  Both are printed; profiles/autograd_cost.md records
    them."""
    import torch

    from tike_amd import autograd
    c, data = _detector_case()
    mask = ac.module_gap_mask(c["det"])
    up = ac.frame_weights(data.shape[0])
    leaves = {k: _dev(v).requires_grad_(True) for k, v in c["host"].items()}
    kw = dict(leaves, fly=c["fly"], measured_pixels=_dev(mask))
    as_float = np.where(mask, data.astype(np.float32), np.float32("nan"))
    names = c["form"].names
    up_d = _dev(up)
    with _operator(c) as op:
        both = []
        for d in (data, as_float):
            costs = autograd.cost(op, _dev(d), *(kw[k] for k in names),
                                  model=model, fly=c["fly"],
                                  measured_pixels=kw["measured_pixels"])
            grads = torch.autograd.grad((costs * up_d).sum(),
                                        [kw[k] for k in names])
            both.append((_host(costs), dict(zip(names, map(_host, grads)))))
        ccosts, cgrads = _composition(c, op, _dev(as_float), kw, up_d, model)
    assert np.array_equal(both[0][0], both[1][0])
    assert np.array_equal(both[0][1]["scan"], both[1][1]["scan"])
    costs, grads = both[0]
    want_costs, want = ac.hand_gradients(
        c["form"], c["m"], torch.from_numpy(data.astype(np.float64)),
        torch.from_numpy(mask), model, torch.from_numpy(up))
    want_costs = want_costs.numpy()
    mine = _grad_errors(grads, want, names)
    mine["costs"] = float((np.abs(costs - want_costs)
                           / np.abs(want_costs)).max())
    with np.errstate(invalid="ignore"):
        theirs = {k: relerr(cgrads[k], want[k].numpy())
                  for k in ("psi", "probe")}
        theirs["scan"] = float((np.abs(cgrads["scan"] - want["scan"].numpy())
                                / want["A_scan"].numpy()).max())
        theirs["costs"] = float((np.abs(ccosts - want_costs)
                                 / np.abs(want_costs)).max())
    print(f"detector-like counts {model}: counts up to {data.max()}, "
          f"{(data == 0).mean():.0%} zero; error against the float64 model, "
          "cost | composition: " + "; ".join(
              f"{k} {mine[k]:.2e} | {theirs[k]:.2e}" for k in mine))
    bars = dict(BARS, costs=1e-5)
    for k, v in mine.items():
        other = theirs[k] if np.isfinite(theirs[k]) else np.inf
        assert np.isfinite(v) and v <= max(bars[k], 2 * other), (k, v, other)


# ------------------------------------------------------------ a dark frame
@pytest.mark.parametrize("model", ac.MODELS)
def test_dark_frame(model):
    """Frame 0 lies over a region where psi is exactly zero, with counts > 0
    there: I = 0, the factor is -sqrt(d) / 1e-9 (or -d / 1e-9), finite.  Every
    gradient of `cost` is finite and meets the model at the bars of
    `test_cost_vs_model`.  Whether the composition's gradients are finite is
    printed, not asserted."""
    import torch

    from tike_amd import autograd
    kind, shape = ac.CASES[0]
    N, S, pw, det, H, W, fly = shape
    base = ac.case(kind, shape)
    host = {k: v.copy() for k, v in base["host"].items()}
    host["scan"][:fly] = np.array([[3.3, 4.6], [5.4, 3.7]], np.float32)[:fly]
    host["psi"][0, :pw + 8, :pw + 8] = 0
    c = dict(base, host=host,
             m=am.as_model(host["psi"], host["probe"], host["scan"]))
    data, mask, up = ac.counts_of(c, False)
    data[0] = 2.0 + np.arange(det * det, dtype=np.float32).reshape(det, det) % 5
    leaves = {k: _dev(v).requires_grad_(True) for k, v in host.items()}
    kw = dict(leaves, fly=fly)
    names = base["form"].names
    up_d = _dev(up)
    with _operator(c) as op:
        costs = autograd.cost(op, _dev(data), *(kw[k] for k in names),
                              model=model, fly=fly)
        grads = dict(zip(names, map(_host, torch.autograd.grad(
            (costs * up_d).sum(), [kw[k] for k in names]))))
        _, cgrads = _composition(c, op, _dev(data), kw, up_d, model)
    want_costs, want = ac.hand_gradients(
        base["form"], c["m"], torch.from_numpy(data.astype(np.float64)), None,
        model, torch.from_numpy(up))
    finite = {k: bool(np.isfinite(v).all()) for k, v in cgrads.items()}
    print(f"dark frame {model}: the composition's gradients finite: {finite}")
    costs = _host(costs)
    assert np.all(np.isfinite(costs))
    assert all(np.isfinite(v).all() for v in grads.values())
    cerr = np.abs(costs - want_costs.numpy()) / np.abs(want_costs.numpy())
    print(f"dark frame {model}: costs max rel {cerr.max():.2e}")
    assert np.all(cerr <= 1e-5)
    _assert_grads(_grad_errors(grads, want, names), f"dark frame {model}")


# ---------------------------------------------------------------- chunking
CHUNK_CASES = [("plain", (12, 2, 16, 20, 40, 44, 2)),
               ("eigen", (12, 3, 2, 2, 16, 20, 48, 2)),
               ("multislice", (12, 2, 32, 72, 2, 2))]


def _chunked_outputs(kind, shape, override):
    """Every output of the three functions with `chunk_positions` forced to
    `override` (cost) and 2 x override (the forward mode's half chunks):
    dict of host arrays.  Importable by the deterministic-mode child."""
    from tike_amd.ptycho.solvers import lstsq
    c = ac.case(kind, shape)
    data, mask, up, kw, tangents = _inputs(c, True)
    saved = lstsq.CHUNK_POSITIONS_OVERRIDE
    out = {}
    try:
        for name, value in (("cost", override),
                            ("tangent", override and 2 * override)):
            lstsq.CHUNK_POSITIONS_OVERRIDE = value
            costs, grads, dcosts, gn = _run_all(c, data, kw, tangents, up,
                                                "poisson")
            if name == "cost":
                out.update(costs=costs,
                           **{"grad_" + k: v for k, v in grads.items()})
            else:
                out.update(dcosts=dcosts,
                           **{"gn_" + k: v for k, v in gn.items()})
    finally:
        lstsq.CHUNK_POSITIONS_OVERRIDE = saved
    return out


EXACT = ("costs", "dcosts", "grad_scan", "grad_eigen_weights", "gn_scan",
         "gn_eigen_weights")


def _compare_chunked(whole, cut):
    """{name: 0.0 where the bits agree, else the normwise difference}."""
    return {k: 0.0 if np.array_equal(whole[k], cut[k]) else
            max(relerr(cut[k], whole[k]), 1e-300) for k in whole}


@pytest.mark.parametrize("kind,shape", CHUNK_CASES)
def test_three_chunks(kind, shape):
    """12 positions, fly = 2, cut into three chunks of whole frames (the
    forward mode and the product of several slices: 8 + 4): costs, dcosts,
    the scan and the weight gradients and products have the bits of the
    one-chunk run (no float atomics); the others agree normwise at 1e-5."""
    whole = _chunked_outputs(kind, shape, 0)
    cut = _chunked_outputs(kind, shape, 4)
    diff = _compare_chunked(whole, cut)
    print(f"three chunks {kind}: " + ", ".join(f"{k} {v:.1e}"
                                               for k, v in diff.items()))
    for k, v in diff.items():
        assert v == 0.0 if k in EXACT else v <= OP_NORMWISE, (k, v)


def test_three_chunks_in_deterministic_mode():
    """The same under TIKE_DETERMINISTIC=1, in a fresh child process (the
    switch is read when the library is bound)."""
    env = dict(os.environ, TIKE_DETERMINISTIC="1")
    run = subprocess.run(
        [sys.executable, os.path.join(HERE, "_autograd_cost_child.py")],
        env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    diff = json.loads(run.stdout.strip().splitlines()[-1])
    print(f"three chunks, deterministic mode: {diff}")
    for k, v in diff.items():
        assert v == 0.0 if k in EXACT else v <= OP_NORMWISE, (k, v)


# ---------------------------------------------------------------- recovery
def test_levenberg_marquardt_recovers_fly_scan_positions():
    """`noisy_problem()` -- 196 positions, fly = 2, start off by up to
    0.3 px (RMS 0.2433), Poisson counts -- with the poisson model: four
    Levenberg-Marquardt steps of at most 20 CG iterations
    (`autograd_cost.levenberg_marquardt`), every product
    `cost_gauss_newton_product`, the right-hand side from `cost`'s backward,
    the step accepted by `cost_jvp`'s slope and a cost decrease.  Finite
    costs, and a final RMS position error of at most 1.5 times the 0.0583 px
    the float64 model reaches (`LM_MODEL_RMS`, test_autograd_cost_cpu.py); the
    margin is for float32 products inside CG."""
    import torch

    from tike_amd import autograd
    p = ac.noisy_problem()
    fly, det, H = p["fly"], p["det"], p["psi"].shape[-1]
    psi, probe, data, start = (_dev(p[k]) for k in ("psi", "probe", "data",
                                                    "scan_start"))
    import tike_amd.operators as ops
    with ops.Ptycho(probe_shape=det, detector_shape=det, nz=H, n=H) as op:
        args = lambda scan: (op, data, psi, probe, scan)
        kw = dict(model="poisson", fly=fly)

        def cost_of(scan):
            with torch.no_grad():
                return float(autograd.cost(*args(scan), **kw).double().sum())

        def grad_of(scan):
            s = scan.detach().requires_grad_(True)
            return torch.autograd.grad(autograd.cost(*args(s), **kw).sum(),
                                       s)[0]

        product_of = lambda scan, v: autograd.cost_gauss_newton_product(
            *args(scan), d_scan=v, wrt=("scan",), **kw)[0]
        slope_of = lambda scan, v: float(autograd.cost_jvp(
            *args(scan), d_scan=v, **kw)[1].double().sum())
        after, costs = ac.levenberg_marquardt(cost_of, grad_of, product_of,
                                              slope_of, start, **ac.LM)
    r0 = am.rms(p["scan_start"], p["scan_true"])
    r = [am.rms(s, p["scan_true"]) for s in after]
    print(f"Levenberg-Marquardt position recovery: rms {r0:.4f} -> "
          + ", ".join(f"{x:.4f}" for x in r) + f"; F "
          + ", ".join(f"{c:.3f}" for c in costs)
          + f"; the float64 model: {ac.LM_MODEL_RMS}")
    assert np.isfinite(costs).all()
    assert r[-1] <= 1.5 * ac.LM_MODEL_RMS, r
