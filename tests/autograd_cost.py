"""Float64 model of `tike_amd.autograd.cost`, `cost_jvp` and
`cost_gauss_newton_product` (test infrastructure), on the models of the three
forms: tests/autograd_model.py + autograd_jvp.py (plain), autograd_eigen.py +
autograd_eigen_jvp.py (eigen probes), autograd_multislice.py +
autograd_multislice_jvp.py (several slices).

Per measured pixel, with the project's guards (1e-9) and the mask applied by
SELECTION (a count under the mask may be NaN):

    gaussian: term (sqrt(I) - sqrt(d))^2,  l' = 1 - sqrt(d) / (sqrt(I) + 1e-9)
    poisson:  term I - d log(I + 1e-9),    l' = 1 - d / (I + 1e-9)
    cost_f   = sum_p term / num_measured
    table_f  = upstream_f l' / num_measured             (the backward's dL/dI)
    dcost_f  = sum_p l' dI / num_measured
    curv_f   = upstream_f c / (num_measured (I + floor)) dI,  c = 1/2 | 1

A `Form` holds the three callables of a model form -- intensity (by torch, so
torch.autograd differentiates the cost), its hand-written forward mode and its
hand-written backward -- so that every function below is written once.
`levenberg_marquardt` is the iteration the CPU test, the GPU test and the
example run; `noisy_problem` its Poisson-noisy fly-scan data.
"""
import collections

import numpy as np
import torch

import autograd_eigen as ae
import autograd_eigen_jvp as aej
import autograd_jvp as aj
import autograd_model as am
import autograd_multislice as mm
import autograd_multislice_jvp as msj

F64 = am.F64
GUARD = 1e-9
MODELS = ("gaussian", "poisson")
CURVATURE = {"gaussian": 0.5, "poisson": 1.0}

Form = collections.namedtuple("Form", "intensity jvp grads names")
"""intensity(m) -> I (frames, det, det), differentiable; jvp(m, t) -> (I, dI)
with t a dict of tangents by the form's names ("d_" + name; missing: zero);
grads(m, g) -> dict by name plus "A_scan" (and "A_weights") for an upstream
g = dL/dI; names: the inputs in the order of the model tuple m."""


def plain(det, fly=1, norm="ortho"):
    """m = (psi, probe, scan)."""
    def grads(m, g):
        h = am.hand_gradients(*m, det, g, fly, norm)
        return dict(psi=h["psi"], probe=h["probe"], scan=h["scan"],
                    A_scan=h["A"])
    return Form(
        lambda m: am.intensity(*m, det, fly, norm),
        lambda m, t: aj.hand_jvp(*m, det, t.get("d_psi"), t.get("d_probe"),
                                 t.get("d_scan"), fly, norm),
        grads, ("psi", "probe", "scan"))


def eigen(det, fly=1, norm="ortho"):
    """m = (psi, probe, scan, eigen_probe or None, eigen_weights)."""
    def grads(m, g):
        h = ae.hand_gradients(*m, det, g, fly, norm)
        return dict(psi=h["psi"], probe=h["probe"], scan=h["scan"],
                    eigen_probe=h["eigen"], eigen_weights=h["weights"],
                    A_scan=h["A_scan"], A_weights=h["A"])
    return Form(
        lambda m: ae.intensity(*m, det, fly, norm),
        lambda m, t: aej.hand_jvp(
            *m, det, t.get("d_psi"), t.get("d_probe"), t.get("d_scan"),
            t.get("d_eigen_probe"), t.get("d_eigen_weights"), fly, norm),
        grads, ("psi", "probe", "scan", "eigen_probe", "eigen_weights"))


def multislice(fly=1, norm="ortho"):
    """m = (psi (D, H, W), probe, scan, Hprop); Hprop is no input."""
    def grads(m, g):
        h = mm.hand_gradients(*m, g, fly, norm)
        return dict(psi=h["psi"], probe=h["probe"], scan=h["scan"],
                    A_scan=h["A"])
    return Form(
        lambda m: mm.intensity(*m, fly, norm),
        lambda m, t: msj.hand_jvp(*m, t.get("d_psi"), t.get("d_probe"),
                                  t.get("d_scan"), fly, norm),
        grads, ("psi", "probe", "scan"))


# ------------------------------------------------------------- per pixel
def _clean(d, mask):
    """The counts as float64 with what lies under the mask selected away."""
    d = torch.as_tensor(d).to(F64)
    return d if mask is None else torch.where(mask, d, torch.zeros_like(d))


def _select(mask, x):
    return x if mask is None else torch.where(mask, x, torch.zeros_like(x))


def num_measured(mask, det):
    return det * det if mask is None else int(mask.sum())


def terms(I, d, model):
    if model == "gaussian":
        return (torch.sqrt(I) - torch.sqrt(d))**2
    return I - d * torch.log(I + GUARD)


def lprime(I, d, model):
    """The project's gradient factor, guard included."""
    if model == "gaussian":
        return 1 - torch.sqrt(d) / (torch.sqrt(I) + GUARD)
    return 1 - d / (I + GUARD)


def costs_of(I, d, mask, model):
    """(frames,) from an intensity; differentiable through I."""
    d = _clean(d, mask)
    nm = num_measured(mask, I.shape[-1])
    return _select(mask, terms(I, d, model)).sum(dim=(1, 2)) / nm


def table_of(I, d, mask, model, upstream=None):
    """dL/dI (frames, det, det) of sum_f upstream_f cost_f, exactly 0 under
    the mask."""
    d = _clean(d, mask)
    nm = num_measured(mask, I.shape[-1])
    up = 1.0 if upstream is None else upstream.to(F64)[:, None, None]
    return _select(mask, up * lprime(I, d, model) / nm)


def dcosts_of(I, dI, d, mask, model):
    d = _clean(d, mask)
    nm = num_measured(mask, I.shape[-1])
    return _select(mask, lprime(I, d, model) * dI).sum(dim=(1, 2)) / nm


def curvature_of(I, dI, mask, model, upstream=None, floor=GUARD):
    nm = num_measured(mask, I.shape[-1])
    up = 1.0 if upstream is None else upstream.to(F64)[:, None, None]
    return _select(mask, up * CURVATURE[model] / (nm * (I + floor)) * dI)


# ------------------------------------------------------------ whole model
def cost(form, m, d, mask, model):
    """(frames,) costs, differentiable by torch.autograd."""
    return costs_of(form.intensity(m), d, mask, model)


def autograd_gradients(form, m, d, mask, model, upstream=None):
    """(costs, dict by name) of sum_f upstream_f cost_f by torch.autograd."""
    leaves = [x.detach().clone().requires_grad_(True) if k < len(form.names)
              and x is not None else x for k, x in enumerate(m)]
    c = cost(form, leaves, d, mask, model)
    (c if upstream is None else c * upstream.to(F64)).sum().backward()
    return c.detach(), {name: None if x is None else x.grad
                        for name, x in zip(form.names, leaves)}


def hand_gradients(form, m, d, mask, model, upstream=None):
    """(costs, dict by name + A_scan ...) with no autograd: the table, then
    the form's hand-written backward -- what the HIP route implements."""
    with torch.no_grad():
        I = form.intensity(m)
        return (costs_of(I, d, mask, model),
                form.grads(m, table_of(I, d, mask, model, upstream)))


def hand_jvp(form, m, t, d, mask, model):
    """(costs, dcosts) with no autograd."""
    with torch.no_grad():
        I, dI = form.jvp(m, t)
        return costs_of(I, d, mask, model), dcosts_of(I, dI, d, mask, model)


def gauss_newton_product(form, m, t, mask, model, upstream=None, floor=GUARD):
    """J^T diag(upstream c / (num_measured (I + floor))) J v: dict by name
    (+ A_scan ... for that upstream table)."""
    with torch.no_grad():
        I, dI = form.jvp(m, t)
        return form.grads(m, curvature_of(I, dI, mask, model, upstream, floor))


def module_gap_mask(det):
    """A detector of two modules: a horizontal gap of max(1, det // 16) rows
    just above the middle and one dead pixel.  (det, det) bool, True =
    measured."""
    mask = np.ones((det, det), dtype=bool)
    gap = max(1, det // 16)
    mask[det // 2 - gap:det // 2] = False
    mask[min(3, det - 1), min(5, det - 1)] = False
    return mask


# ------------------------------------------------- Levenberg-Marquardt
LM = dict(steps=4, cg_iters=20, damping=1e-3)


def levenberg_marquardt(cost_of, grad_of, product_of, slope_of, start, steps=4,
                        cg_iters=20, damping=1e-3):
    """Levenberg-Marquardt on the positions alone for F = sum_f cost_f:
    `steps` times solve (G + lam) delta = -grad F by at most `cg_iters`
    conjugate-gradient iterations from zero, G v = product_of(scan, v) the
    Gauss-Newton product, lam = damping * mean|G 1|.  The step is taken when
    the exact slope along it, slope_of(scan, delta) = sum_f dcost_f, is
    negative AND the cost decreases; otherwise it is halved (twice at the
    most) and, failing that, dropped with the damping ten times larger for
    the next step.  cost_of(scan) -> float F; grad_of(scan) -> grad F; tensors
    of one dtype and device.  Returns ([positions after every step, host
    arrays], [F before every step and after the last])."""
    dot = lambda a, b: float((a.double() * b.double()).sum())
    scan = start.detach().clone()
    after, costs = [], [cost_of(scan)]
    for _ in range(steps):
        hess = lambda v: product_of(scan, v)
        lam = damping * float(hess(torch.ones_like(scan)).abs().mean())
        b = -grad_of(scan)
        delta = torch.zeros_like(scan)
        res, p = b.clone(), b.clone()
        rs0 = rs = dot(res, res)
        for _ in range(cg_iters):
            if rs <= 1e-24 * rs0:
                break
            hp = hess(p) + lam * p
            alpha = rs / dot(p, hp)
            delta = delta + alpha * p
            res = res - alpha * hp
            rs_new = dot(res, res)
            p = res + (rs_new / rs) * p
            rs = rs_new
        taken = False
        if slope_of(scan, delta) < 0:
            for t in (1.0, 0.5, 0.25):
                trial = scan + t * delta
                f = cost_of(trial)
                if np.isfinite(f) and f < costs[-1]:
                    scan, taken = trial, True
                    costs.append(f)
                    break
        if not taken:
            damping *= 10.0
            costs.append(costs[-1])
        after.append(scan.detach().cpu().numpy().copy())
    return after, costs


NOISY_GAIN = 1e4


def noisy_problem(seed=0, gain=NOISY_GAIN):
    """`autograd_model.problem()` (196 positions, fly = 2, start off by up to
    0.3 px) with a probe of sqrt(gain) times the amplitude and Poisson counts
    drawn from its intensities (gain: the mean of the brightest pixel goes
    from a few counts to a few thousand).  data float32 holding the integer
    counts."""
    p = dict(am.problem(seed=seed))
    p["probe"] = (p["probe"] * np.float32(np.sqrt(gain))).astype(np.complex64)
    with torch.no_grad():
        clean = am.intensity(*am.as_model(p["psi"], p["probe"],
                                          p["scan_true"]), p["det"],
                             p["fly"]).numpy()
    rng = np.random.default_rng(seed + 500)
    p["data"] = rng.poisson(clean).astype(np.float32)
    return p


def lm_on_model(p, model="poisson"):
    """`levenberg_marquardt` on the float64 model of `noisy_problem()`:
    (positions after every step, F before every step and after the last)."""
    form = plain(p["det"], p["fly"])
    psi, probe, _ = am.as_model(p["psi"], p["probe"], p["scan_true"])
    d = torch.from_numpy(p["data"]).to(F64)
    start = torch.from_numpy(p["scan_start"]).to(F64)
    m = lambda scan: (psi, probe, scan)

    def cost_of(s):
        with torch.no_grad():
            return float(cost(form, m(s), d, None, model).sum())

    grad_of = lambda s: hand_gradients(form, m(s), d, None, model)[1]["scan"]
    product_of = lambda s, v: gauss_newton_product(
        form, m(s), dict(d_scan=v), None, model)["scan"]
    slope_of = lambda s, v: float(hand_jvp(form, m(s), dict(d_scan=v), d, None,
                                           model)[1].sum())
    return levenberg_marquardt(cost_of, grad_of, product_of, slope_of, start,
                               **LM)


# ------------------------------------------------------------ the inputs
def well_conditioned_counts(form, m, seed=0):
    """float32 counts (frames, det, det): the model's intensity of perturbed
    inputs -- the probe 0.8 times as large, every position moved by up to
    0.04 px (kept inside the object) -- so that sqrt(d / I) stays near 0.8:
    the gradient factor 1 - sqrt(d / I) is then neither dominated by dark
    pixels (a large ratio) nor a difference of nearly equal numbers (a ratio
    of 1.08 costs float32 alone 9.6e-7 A_n in the scan gradient at det = 64:
    the factor is -0.08 with the rounding of 1.08)."""
    rng = np.random.default_rng(seed + 900)
    psi, probe, scan = m[0], m[1], m[2]
    pw = probe.shape[-1]
    moved = scan + torch.from_numpy(rng.uniform(-0.04, 0.04, scan.shape))
    hi = torch.tensor([psi.shape[-2] - pw - 1e-3, psi.shape[-1] - pw - 1e-3],
                      dtype=F64)
    moved = torch.minimum(torch.clamp(moved, min=1.0), hi)
    with torch.no_grad():
        inten = form.intensity((psi, 0.8 * probe, moved) + tuple(m[3:]))
    return inten.numpy().astype(np.float32)


def frame_weights(frames, seed=0):
    """A non-uniform signed upstream (frames,) float32: d(sum w_f cost_f)."""
    rng = np.random.default_rng(seed + 40)
    return (0.5 + rng.random(frames)).astype(np.float32) * np.where(
        np.arange(frames) % 3 == 2, -1, 1).astype(np.float32)


def float32_gradients(m, det, fly, d, mask, model, upstream=None,
                      norm="ortho"):
    """The plain form's cost gradients restated in float32 / complex64 on the
    CPU (the weight and scan sums in float64, as the kernels have them): what
    float32 alone costs against `hand_gradients`.  m = (psi, probe, scan)
    float64 model tensors; dict(psi, probe, scan)."""
    psi, probe, scan = m
    ones = torch.ones((scan.shape[0], 1, probe.shape[2]), dtype=F64)
    low = lambda x: x.to(torch.complex64 if x.is_complex() else torch.float32)
    with torch.no_grad():
        I = ae.intensity(low(psi), low(probe), low(scan), None, low(ones),
                         det, fly, norm)
        assert I.dtype == torch.float32
        d32 = low(_clean(d, mask))
        nm = num_measured(mask, det)
        g = torch.float32
        if model == "gaussian":
            lp = 1 - torch.sqrt(d32) / (torch.sqrt(I) + torch.tensor(GUARD, dtype=g))
        else:
            lp = 1 - d32 / (I + torch.tensor(GUARD, dtype=g))
        up = (torch.ones(I.shape[0], dtype=g) if upstream is None
              else upstream.to(g)) / nm
        table = _select(mask, up[:, None, None] * lp)
        assert table.dtype == torch.float32
    h = ae.hand_gradients(psi, probe, scan, None, ones, det, table, fly, norm,
                          single=True)
    return dict(psi=h["psi"], probe=h["probe"], scan=h["scan"])


LM_MODEL_RMS = 0.05834
"""The RMS position error (px) the float64 model reaches on `noisy_problem()`
after four Levenberg-Marquardt steps, from 0.2433
(test_autograd_cost_cpu.py reproduces it): the GPU test is held to 1.5 times
this."""


# ------------------------------------------------- the end-to-end cases
# (N, S, pw, det, H, W, fly): fly scan at the smallest size; pw < det at a
# detector without the scaled inverse (tike_farplane_scale); the scaled inverse
PLAIN_CASES = [(8, 3, 16, 16, 40, 40, 2), (6, 2, 48, 64, 120, 120, 1),
               (4, 2, 100, 128, 240, 250, 2)]
# (N, S, M, C, pw, det, H, fly): the two smallest of autograd_eigen's
EIGEN_CASES = [(5, 1, 1, 1, 15, 15, 40, 1), (6, 3, 2, 2, 16, 20, 48, 2)]
# (N, S, pw, obj, D, fly): general with two and three slices, fused with two
# and three
MULTISLICE_CASES = [(6, 2, 32, 72, 2, 1), (8, 2, 64, 104, 3, 2),
                    (6, 2, 128, 170, 2, 2), (4, 8, 128, 170, 3, 1)]
CASES = ([("plain", s) for s in PLAIN_CASES]
         + [("eigen", s) for s in EIGEN_CASES]
         + [("multislice", s) for s in MULTISLICE_CASES])

_CACHE = {}


def case(kind, shape):
    """dict(form, m (float64 model tuple), t (model tangents by d_name), host
    (float32 / complex64 arrays by the names of `cost`'s arguments), host_t
    (tangents by d_name), det, fly, operator (keyword arguments of
    tike_amd.operators.Ptycho)) -- computed once, shared, left unchanged."""
    if (kind, shape) in _CACHE:
        return _CACHE[kind, shape]
    if kind == "plain":
        N, S, pw, det, H, W, fly = shape
        c = aj.case(N, S, pw, det, H, W, fly)
        m, t = aj.as_model(c)
        out = dict(form=plain(det, fly), m=m, t=t, det=det, fly=fly,
                   host={k: c[k] for k in ("psi", "probe", "scan")},
                   host_t={k: c[k] for k in ("d_psi", "d_probe", "d_scan")},
                   operator=dict(probe_shape=pw, detector_shape=det, nz=H,
                                 n=W))
    elif kind == "eigen":
        N, S, M, C, pw, det, H, fly = shape
        c = dict(ae.inputs(N, S, M, C, pw, H, H, seed=N + 3 * S + 5 * det))
        c.update(aej.tangents(c, seed=17 + N + 3 * S + 5 * det))
        rename = dict(eigen="eigen_probe", weights="eigen_weights",
                      d_eigen="d_eigen_probe", d_weights="d_eigen_weights")
        host = {rename.get(k, k): c[k]
                for k in ("psi", "probe", "scan", "eigen", "weights")}
        host_t = {rename.get(k, k): c[k] for k in aej.TANGENT_NAMES}
        out = dict(form=eigen(det, fly), m=ae.model_of(c),
                   t={k: ae.t128(v) for k, v in host_t.items()}, det=det,
                   fly=fly, host=host, host_t=host_t,
                   operator=dict(probe_shape=pw, detector_shape=det, nz=H,
                                 n=H))
    else:
        N, S, pw, obj, D, fly = shape
        c = msj.case(N, S, pw, obj, D, fly)
        m, t = msj.as_model(c)
        out = dict(form=multislice(fly), m=m, t=t, det=pw, fly=fly,
                   host={k: c[k] for k in ("psi", "probe", "scan")},
                   host_t={k: c[k] for k in ("d_psi", "d_probe", "d_scan")},
                   operator=dict(probe_shape=pw, detector_shape=pw, nz=obj,
                                 n=obj, **mm.optics(pw)))
    _CACHE[kind, shape] = out
    return out


def counts_of(c, masked, seed=0):
    """(data float32 host array with NaN under the mask, mask (det, det) bool
    host array or None, upstream (frames,) float32) of a case."""
    d = well_conditioned_counts(c["form"], c["m"], seed)
    mask = module_gap_mask(c["det"]) if masked else None
    if masked:
        d = np.where(mask, d, np.float32("nan")).astype(np.float32)
    return d, mask, frame_weights(d.shape[0], seed)
