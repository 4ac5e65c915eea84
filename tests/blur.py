"""float64 NumPy model of ptychography with a blurred far field, on top of
tests/fly_scan.py:

    I_f     = sum_{j < fly} sum_{m < S} |far[f * fly + j, m]|^2
    I_model = K (*) I_f        cyclic over the (det, det) plane in the stored
                               (FFT-shifted) layout, K (k, k), centre [r, r]:
              I_model[y, x] = sum_{u,v} K[u, v] I[(y-u+r) % det, (x-v+r) % det]
    cost    = mean over frames of each frame's mean over its measured pixels of
              the noise model's term at I_model
    table   = K (star) (upstream_f mask l'(I_model, d) / num_measured): the
              cyclic correlation, the adjoint of the blur; far * table is the
              gradient with respect to the far plane
    kgrad[u, v] = sum_f sum_{p measured} upstream_f l'(p) / num_measured
                  I_f[p - (u - r, v - r)]

Blur and correlation are explicit np.roll sums, so the cyclic indexing is the
definition's own.  The kernel is fitted through a real a (k, k) with
K = a^2 / sum a^2; d / d a = 2 a / sum a^2 (g - sum(g K)), g = kgrad.  A cgrad
epoch has THREE blocks per minibatch: the object, the probe and a, with
tests/background.py's real CG and line search.  Gradients are, as in fly_scan,
those of the SUM of the frames' costs.  A count under the mask may be NaN:
selected away, never multiplied."""
import numpy as np

import background as bg
import fly_scan as fs


def _taps(K):
    K = np.asarray(K, np.float64)
    k = K.shape[0]
    assert K.shape == (k, k) and k % 2 == 1
    r = k // 2
    return K, [(u, v, u - r, v - r) for u in range(k) for v in range(k)]


def blur(K, x):
    """K (*) x over the last two axes: out[p] = sum K[u, v] x[p - (u-r, v-r)]
    (np.roll by s moves x[p - s] to p)."""
    K, taps = _taps(K)
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    for u, v, du, dv in taps:
        out = out + K[u, v] * np.roll(x, (du, dv), axis=(-2, -1))
    return out


def correlate(K, y):
    """K (star) y: out[p] = sum K[u, v] y[p + (u-r, v-r)], the adjoint of
    `blur`."""
    K, taps = _taps(K)
    y = np.asarray(y, np.float64)
    out = np.zeros_like(y)
    for u, v, du, dv in taps:
        out = out + K[u, v] * np.roll(y, (-du, -dv), axis=(-2, -1))
    return out


def num_measured(mask, det):
    return det * det if mask is None else int(mask.sum())


def cost_each(model, data, inten, K, mask=None):
    return fs.cost_each(model, data, blur(K, inten), mask)


def cost_from_intensity(model, data, inten, K, mask=None, upstream=None):
    """sum_f upstream_f cost_f (upstream None: the mean over the frames)."""
    c = cost_each(model, data, inten, K, mask)
    if upstream is None:
        return float(np.mean(c))
    return float(np.sum(np.asarray(upstream, np.float64) * c))


def factor(model, data, inten, K, mask=None, upstream=None):
    """g = upstream_f l'(I_model, d) / num_measured, 0 at unmeasured pixels."""
    g = bg.factor(model, data, blur(K, inten), mask)
    g = g / num_measured(mask, inten.shape[-1])
    if upstream is not None:
        g = g * np.asarray(upstream, np.float64)[:, None, None]
    return g


def table(model, data, inten, K, mask=None, upstream=None):
    return correlate(K, factor(model, data, inten, K, mask, upstream))


def kgrad(model, data, inten, K, mask=None, upstream=None):
    K, taps = _taps(K)
    g = factor(model, data, inten, K, mask, upstream)
    inten = np.asarray(inten, np.float64)
    out = np.zeros_like(K)
    for u, v, du, dv in taps:
        out[u, v] = np.sum(g * np.roll(inten, (du, dv), axis=(-2, -1)))
    return out


# ----------------------------------------------------------------- the chain
def kernel_of(a):
    a = np.asarray(a, np.float64)
    return a * a / np.sum(a * a)


def grad_a(a, g):
    """d / d a of a function of K = a^2 / sum a^2 whose gradient in K is g."""
    a = np.asarray(a, np.float64)
    K = kernel_of(a)
    return 2 * a / np.sum(a * a) * (g - np.sum(g * K))


def normalised(K):
    K = np.asarray(K, np.float64)
    return (K / K.sum()).astype(np.float32)


def root_of(K):
    """The float32 a the fit starts from: sqrt of the normalised kernel."""
    return np.sqrt(normalised(K).astype(np.float64)).astype(np.float32)


def gaussian_kernel(k, sigma):
    x = np.arange(k) - k // 2
    g = np.exp(-(x[:, None]**2 + x[None, :]**2) / (2 * sigma * sigma))
    return normalised(g)


def delta_kernel(k):
    K = np.zeros((k, k), np.float32)
    K[k // 2, k // 2] = 1
    return K


# --------------------------------------------------- the ptychographic model
def intensity(probe, scan, psi, det, fly, K):
    return blur(K, fs.frame_intensity(fs.fwd(probe, scan, psi, det), fly))


def cost(model, data, psi, scan, probe, det, fly, mask=None, K=None):
    inten = fs.frame_intensity(fs.fwd(probe, scan, psi, det), fly)
    return cost_from_intensity(model, data, inten, K, mask)


def farplane_gradient(model, data, far, fly, mask=None, K=None):
    """far * T with T the table of the SUM of the frames' costs."""
    inten = fs.frame_intensity(far, fly)
    t = table(model, data, inten, K, mask) * num_measured(mask, far.shape[-1])
    return far * np.repeat(t, fly, axis=0)[:, None, None, :, :]


def grad_psi(model, data, psi, scan, probe, det, fly, mask=None, K=None):
    g = farplane_gradient(model, data, fs.fwd(probe, scan, psi, det), fly,
                          mask, K)
    return fs.adj(g, probe, scan, psi)[0]


def grad_probe(model, data, psi, scan, probe, det, fly, mask=None, K=None):
    g = farplane_gradient(model, data, fs.fwd(probe, scan, psi, det), fly,
                          mask, K)
    return np.sum(fs.adj(g, probe, scan, psi)[1], axis=0, keepdims=True)


def cgrad(state, data, batches, *, detector_shape, fly, model, mask=None,
          cg_iter=2, step_length=1.0, recover_probe=True, update=True):
    """One epoch: per minibatch the object, the probe and -- with `update` --
    the root a of the kernel (state["a"], (k, k) float32 between iterations).
    The third block forms the intensity of the minibatch once: it does not
    depend on a.  Its gradient is that of the SUM of the frames' costs (kgrad
    with upstream ones), as the background's block takes it."""
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
        K = kernel_of(a)
        psi, c = fs.conjugate_gradient(
            psi, lambda p: cost(model, d, p, s, probe, det, fly, mask, K),
            lambda p: grad_psi(model, d, p, s, probe, det, fly, mask, K),
            cg_iter, step_length, margins)
        if recover_probe:
            probe, c = fs.conjugate_gradient(
                probe, lambda q: cost(model, d, psi, s, q, det, fly, mask, K),
                lambda q: grad_probe(model, d, psi, s, q, det, fly, mask, K),
                cg_iter, step_length, margins)
        if update:
            inten = fs.frame_intensity(fs.fwd(probe, s, psi, det), fly)
            a, c = bg.conjugate_gradient_real(
                a, lambda x: cost_from_intensity(model, d, inten,
                                                 kernel_of(x), mask),
                lambda x: grad_a(x, kgrad(model, d, inten, kernel_of(x),
                                          mask)),
                cg_iter, step_length, margins)
        batch_cost.append(c)
    state["costs"].append([float(np.mean(batch_cost))])
    state["psi"], state["probe"], state["a"] = psi, probe, a
    return state


# ---------------------------------------------------- detector-like intensities
def detector_intensity(nframe, det, rng):
    """Stored intensities that look like a detector: a peak of 1e6 at the
    stored corner falling over six decades to the farthest (cyclic) pixel,
    times uniform(0.2, 1.8), plus 1e-3: float32 (nframe, det, det)."""
    y = np.minimum(np.arange(det), det - np.arange(det)).astype(np.float64)
    dist = np.hypot(y[:, None], y[None, :])
    decay = 1e6 * 10.0**(-6.0 * dist / dist.max())
    return (decay[None] * rng.uniform(0.2, 1.8, (nframe, det, det))
            + 1e-3).astype(np.float32)


# ------------------------------------------------------------- the problems
TRUE_KERNEL = gaussian_kernel(5, 0.8)
"""What the solver and demonstration data are blurred with: a Gaussian of
sigma = 0.8 pixels on 5 x 5 taps."""


def first_guess(k=5):
    """0.52 at the centre and 0.02 elsewhere (sum 1 at k = 5)."""
    K = np.full((k, k), 0.02, np.float32)
    K[k // 2, k // 2] = 0.52
    return K


SOLVER_CASES = {name: case[0] for name, case in bg.SOLVER_CASES.items()}
"""The shapes of the background's solver problems (det 32, fly 1 and 2)."""
STEP_LENGTH = 1.0
SOLVER_VARIANTS = bg.SOLVER_VARIANTS

_CACHE = {}


def solver_problem(case):
    """fly_scan.problem with its data blurred by TRUE_KERNEL: dict(...,
    kernel the true one, k0 the first guess)."""
    P = fs.problem(**SOLVER_CASES[case])
    return dict(P, data=blur(TRUE_KERNEL, P["data"]).astype(np.float32),
                kernel=TRUE_KERNEL, k0=first_guess())


def run_model(case, model, use_mask, update, epochs=2, cg_iter=2):
    """The float64 three-block cgrad on a named problem, one minibatch,
    computed once per variant.  Returns (state, problem, mask)."""
    key = (case, model, use_mask, update, epochs, cg_iter)
    if key in _CACHE:
        return _CACHE[key]
    kw = SOLVER_CASES[case]
    P = solver_problem(case)
    mask = fs.block_mask(kw["det"]) if use_mask else None
    data = fs.masked(P["data"], mask) if use_mask else P["data"]
    N = len(P["scan"])
    state = dict(psi=P["psi0"].copy(), probe=P["probe0"].copy(),
                 scan=P["scan"], a=root_of(P["k0"]), costs=[])
    for _ in range(epochs):
        state = cgrad(state, data, [np.arange(N)], detector_shape=kw["det"],
                      fly=kw["fly"], model=model, mask=mask, cg_iter=cg_iter,
                      step_length=STEP_LENGTH, update=update)
    _CACHE[key] = state, dict(P, data=data), mask
    return _CACHE[key]


# ----------------------------------------------------------- demonstration
DEMO = dict(problem=bg.DEMO["problem"], epochs=6, cg_iter=2)
"""The background demonstration's geometry (obj 96, pw 32, det 32, 25 frames,
1 mode); the probe is known (not recovered), the object starts blurred."""


def demo_problem():
    P = fs.problem(**DEMO["problem"])
    return dict(P, data=blur(TRUE_KERNEL, P["data"]).astype(np.float32),
                kernel=TRUE_KERNEL, k0=first_guess())


def run_demo(how):
    """The model on the demonstration problem.  how: "none" (no blur in the
    model: two blocks of fly_scan's cgrad), "true" (the true kernel, fixed) or
    "fit" (from the first guess): (object error, state)."""
    key = ("demo", how)
    if key in _CACHE:
        return _CACHE[key]
    D, kw = DEMO, DEMO["problem"]
    P = demo_problem()
    N = len(P["scan"])
    state = dict(psi=P["psi0"].copy(), probe=P["probe"].copy(),
                 scan=P["scan"], costs=[])
    if how != "none":
        state["a"] = root_of(P["kernel"] if how == "true" else P["k0"])
    for _ in range(D["epochs"]):
        if how == "none":
            state = fs.cgrad(state, P["data"], [np.arange(N)],
                             detector_shape=kw["det"], fly=kw["fly"],
                             model="gaussian", cg_iter=D["cg_iter"],
                             recover_probe=False)
        else:
            state = cgrad(state, P["data"], [np.arange(N)],
                          detector_shape=kw["det"], fly=kw["fly"],
                          model="gaussian", cg_iter=D["cg_iter"],
                          recover_probe=False, update=how == "fit")
    _CACHE[key] = (bg.object_error(state["psi"], P["psi"], P["scan"],
                                   kw["pw"]), state)
    return _CACHE[key]
