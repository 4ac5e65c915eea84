"""float64 NumPy model of ptychography with an incoherent background per
detector pixel, on top of tests/fly_scan.py:

    I_f = sum_{j < fly} sum_{m < S} |far[f * fly + j, m]|^2 + b,   b = a * a
    cost = mean over frames of each frame's mean over its measured pixels of
           the noise model's term at I_f
    d (sum_f cost_f) / d b[p] = sum_f l'(I_f[p], d_f[p]) / num_measured on the
           measured pixels, 0 elsewhere;  d / d a = 2 a d / d b

and a cgrad epoch of THREE blocks per minibatch: the object, the probe, the
root a of the background (real; float32 between iterations), each `cg_iter`
conjugate-gradient iterations with fly_scan's backtracking search.  Gradients
are, as in fly_scan, those of the SUM of the frames' costs.  A count or a
background value under the mask may be NaN: selected away, never multiplied.
"""
import numpy as np

import fly_scan as fs


def intensity(probe, scan, psi, det, fly, b):
    return fs.frame_intensity(fs.fwd(probe, scan, psi, det), fly) + b


def cost(model, data, psi, scan, probe, det, fly, mask=None, b=0.0):
    inten = intensity(probe, scan, psi, det, fly, b)
    return float(np.mean(fs.cost_each(model, data, inten, mask)))


def factor(model, data, inten, mask=None):
    """l'(I, d), 0 at unmeasured pixels."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return fs._select(mask, fs._FACTORS[model](
            np.asarray(data, np.float64), np.asarray(inten, np.float64)))


def farplane_gradient(model, data, far, fly, mask=None, b=0.0):
    f = factor(model, data, fs.frame_intensity(far, fly) + b, mask)
    return far * np.repeat(f, fly, axis=0)[:, None, None, :, :]


def grad_psi(model, data, psi, scan, probe, det, fly, mask=None, b=0.0):
    g = farplane_gradient(model, data, fs.fwd(probe, scan, psi, det), fly,
                          mask, b)
    return fs.adj(g, probe, scan, psi)[0]


def grad_probe(model, data, psi, scan, probe, det, fly, mask=None, b=0.0):
    g = farplane_gradient(model, data, fs.fwd(probe, scan, psi, det), fly,
                          mask, b)
    return np.sum(fs.adj(g, probe, scan, psi)[1], axis=0, keepdims=True)


def grad_b_from_intensity(model, data, inten_without_b, mask, b,
                          upstream=None):
    """sum_f upstream_f l'(I_f + b, d_f) / num_measured, 0 under the mask."""
    det = inten_without_b.shape[-1]
    n = det * det if mask is None else int(mask.sum())
    f = factor(model, data, inten_without_b + b, mask)
    if upstream is not None:
        f = f * np.asarray(upstream, np.float64)[:, None, None]
    return f.sum(axis=0) / n


def cost_from_intensity(model, data, inten_without_b, mask, b):
    return float(np.mean(fs.cost_each(model, data, inten_without_b + b, mask)))


def grad_b(model, data, psi, scan, probe, det, fly, mask=None, b=0.0):
    inten = fs.frame_intensity(fs.fwd(probe, scan, psi, det), fly)
    return grad_b_from_intensity(model, data, inten, mask, b)


def grad_a(model, data, psi, scan, probe, det, fly, mask, a):
    with np.errstate(invalid="ignore"):
        a = np.where(True if mask is None else mask, a, 0.0)
    return 2 * a * grad_b(model, data, psi, scan, probe, det, fly, mask,
                          a * a)


# --------------------------------------------------------------- the solver
def _line_search_real(f, x, d, step, margins, fx=None):
    """fly_scan._line_search for a real float32 variable."""
    fx = f(x) if fx is None else fx
    while True:
        xsd = (x + np.float32(step) * d).astype(np.float32).astype(np.float64)
        fxsd = f(xsd)
        margins.append(abs(fxsd - fx) / abs(fx))
        if fxsd <= fx:
            return step, fxsd, xsd
        step *= 0.5
        if step < 1e-32:
            return 0, fx, x


def conjugate_gradient_real(x, cost_function, grad, num_iter, step_length,
                            margins):
    dir_ = grad0 = fx = None
    for i in range(num_iter):
        grad1 = grad(x)
        dir_ = (fs._direction(grad1) if i == 0 else
                fs._direction(grad1, grad0, dir_))
        grad0 = grad1
        step_length, fx, x = _line_search_real(cost_function, x, dir_,
                                               step_length, margins, fx)
    return x, fx


def cgrad(state, data, batches, *, detector_shape, fly, model, mask=None,
          cg_iter=2, step_length=1.0, recover_probe=True, update=True):
    """One epoch: per minibatch the object, the probe and -- with `update` --
    the root of the background (state["a"], (det, det)).  The third block
    forms the intensity of the minibatch once: it does not depend on a."""
    det = detector_shape
    psi = np.asarray(state["psi"], np.complex128)
    probe = np.asarray(state["probe"], np.complex128)
    a = np.asarray(state["a"], np.float64)
    scan = state["scan"]
    margins = state.setdefault("margins", [])
    batch_cost = []
    for bt in batches:
        lo, hi = int(bt[0]), int(bt[0]) + len(bt)
        assert lo % fly == 0 and hi % fly == 0
        d, s = data[lo // fly:hi // fly], scan[lo:hi]
        b = a * a
        psi, c = fs.conjugate_gradient(
            psi, lambda p: cost(model, d, p, s, probe, det, fly, mask, b),
            lambda p: grad_psi(model, d, p, s, probe, det, fly, mask, b),
            cg_iter, step_length, margins)
        if recover_probe:
            probe, c = fs.conjugate_gradient(
                probe, lambda q: cost(model, d, psi, s, q, det, fly, mask, b),
                lambda q: grad_probe(model, d, psi, s, q, det, fly, mask, b),
                cg_iter, step_length, margins)
        if update:
            inten = fs.frame_intensity(fs.fwd(probe, s, psi, det), fly)
            a, c = conjugate_gradient_real(
                a, lambda x: cost_from_intensity(model, d, inten, mask, x * x),
                lambda x: 2 * x * grad_b_from_intensity(model, d, inten, mask,
                                                        x * x),
                cg_iter, step_length, margins)
        batch_cost.append(c)
    state["costs"].append([float(np.mean(batch_cost))])
    state["psi"], state["probe"], state["a"] = psi, probe, a
    return state


# ------------------------------------------------------------- the problems
def blob(det, flat, peak, width=0.35):
    """A flat offset plus a smooth bump around the beam (centred detector
    coordinates), in the STORED (FFT-shifted) layout: float32 (det, det)."""
    y, x = np.meshgrid(np.linspace(-1, 1, det), np.linspace(-1, 1, det),
                       indexing="ij")
    centred = flat + peak * np.exp(-(x * x + y * y) / (2 * width * width))
    return np.fft.ifftshift(centred).astype(np.float32)


SOLVER_CASES = {
    # name: (fly_scan.problem keywords, flat, peak, first guess of b); det 32.
    # The background is a few counts on patterns of a few counts, the first
    # guess a quarter of its flat part, and the searches start from
    # STEP_LENGTH: the gradient with respect to a carries the 1 / num_measured
    # of the cost, so that a block on a moves the cost by little at step
    # length 1.  Seed, sizes and step length chosen so that every comparison
    # of the float64 line searches, over both epochs and every
    # SOLVER_VARIANTS entry, is decided by a relative margin >=
    # fly_scan.MIN_MARGIN (test_background_cpu.py asserts it; the smallest is
    # 2.3e-3)
    "fly1": (dict(obj=96, pw=32, det=32, S=2, fly=1, nframe=16, seed=4,
                  amp=1.0, mix=0.6, dim=0.5), 3.0, 1.0, 0.75),
    "fly2": (dict(obj=96, pw=32, det=32, S=2, fly=2, nframe=12, seed=4,
                  amp=1.0, mix=0.6, dim=0.5), 3.0, 1.0, 0.75),
}
STEP_LENGTH = 16.0
SOLVER_VARIANTS = [(model, use_mask, update)
                   for model in ("gaussian", "poisson")
                   for use_mask in (False, True)
                   for update in (False, True)]

_CACHE = {}


def solver_problem(case):
    """fly_scan.problem with the background added to its data: dict(...,
    background the true one, b0 the first guess (a small constant))."""
    kw, flat, peak, guess = SOLVER_CASES[case]
    P = fs.problem(**kw)
    b = blob(kw["det"], flat, peak)
    return dict(P, data=(P["data"] + b).astype(np.float32), background=b,
                b0=np.full_like(b, guess))


def run_model(case, model, use_mask, update, epochs=2, cg_iter=2):
    """The float64 three-block cgrad on a named problem, one minibatch,
    computed once per variant.  Returns (state, problem, mask)."""
    key = (case, model, use_mask, update, epochs, cg_iter)
    if key in _CACHE:
        return _CACHE[key]
    kw = SOLVER_CASES[case][0]
    P = solver_problem(case)
    mask = fs.block_mask(kw["det"]) if use_mask else None
    data = fs.masked(P["data"], mask) if use_mask else P["data"]
    N = len(P["scan"])
    a0 = np.sqrt(P["b0"]).astype(np.float32)
    state = dict(psi=P["psi0"].copy(), probe=P["probe0"].copy(),
                 scan=P["scan"], a=a0, costs=[])
    for _ in range(epochs):
        state = cgrad(state, data, [np.arange(N)], detector_shape=kw["det"],
                      fly=kw["fly"], model=model, mask=mask, cg_iter=cg_iter,
                      step_length=STEP_LENGTH, update=update)
    _CACHE[key] = state, dict(P, data=data), mask
    return _CACHE[key]


# ----------------------------------------------------------- demonstration
DEMO = dict(problem=dict(obj=96, pw=32, det=32, S=1, fly=1, nframe=25, seed=3,
                         amp=1.0, mix=0.3, dim=1.0),
            flat=0.3, peak=1.5, guess=0.1, epochs=6, cg_iter=2)
"""A flat offset plus a smooth blob of the size of the signal's tails; the
probe is known (dim = 1, not recovered), the object starts blurred."""


def object_error(psi, truth, scan, pw):
    """Normwise error of the object over the scanned field of view, after the
    best global complex factor."""
    lo = int(np.floor(scan.min(axis=0)).min())
    hi = int(np.ceil(scan.max(axis=0)).max()) + pw
    a = np.asarray(psi, np.complex128)[0, lo:hi, lo:hi]
    t = np.asarray(truth, np.complex128)[0, lo:hi, lo:hi]
    factor_ = np.vdot(a, t) / np.vdot(a, a)
    return float(np.linalg.norm(factor_ * a - t) / np.linalg.norm(t))


def demo_problem():
    D = DEMO
    P = fs.problem(**D["problem"])
    b = blob(D["problem"]["det"], D["flat"], D["peak"])
    return dict(P, data=(P["data"] + b).astype(np.float32), background=b,
                b0=np.full_like(b, D["guess"]))


def run_demo(fit):
    """The model's object error on the demonstration problem, with the
    background fitted (three blocks from the first guess) or ignored (b = 0,
    two blocks): (error, state)."""
    key = ("demo", fit)
    if key in _CACHE:
        return _CACHE[key]
    D = DEMO
    kw = D["problem"]
    P = demo_problem()
    N = len(P["scan"])
    a0 = np.sqrt(P["b0"]) if fit else np.zeros_like(P["b0"])
    state = dict(psi=P["psi0"].copy(), probe=P["probe"].copy(),
                 scan=P["scan"], a=a0.astype(np.float32), costs=[])
    for _ in range(D["epochs"]):
        state = cgrad(state, P["data"], [np.arange(N)],
                      detector_shape=kw["det"], fly=kw["fly"],
                      model="gaussian", cg_iter=D["cg_iter"],
                      recover_probe=False, update=fit)
    _CACHE[key] = (object_error(state["psi"], P["psi"], P["scan"], kw["pw"]),
                   state)
    return _CACHE[key]
