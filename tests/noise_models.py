"""A float64 / complex128 model of the noise-model entries -- the gaussian and
poisson gradient factor, the per-pattern costs, the far-plane gradient, the
poisson step lengths and the exit-wave update chi -- on detector-like counts,
and the table of cases both test files walk.  NumPy only: it imports without
torch or a GPU.

The model restates include/tike_amd.h, not the kernels: for a far plane F
(N, S, det, det), counts d (N, det, det), an optional measured-pixel mask,
`unmeasured_scaling`, `step_start` and `weight`,

  I        = sum_s |F_s|^2
  factor   = -(1 - sqrt d / (sqrt I + 1e-9))   gaussian, measured pixels
             -(1 - d / (I + 1e-9))             poisson,  measured pixels
             unmeasured_scaling - 1            elsewhere, exactly
  costs    = mean over the measured pixels of (sqrt I - sqrt d)^2 or
             I - d log(I + 1e-9)
  gradient = F_s factor
  steps    = exitwave.py:122-184 (all modes) and :187-234 (dominant mode): the
             denominator and two fixed-point updates from step_start
  chi      = IFFT2(F_s factor [step_s on measured pixels]) scale

tests/test_noise_models_cpu.py pins the model and the preconditions of every
case; tests/test_noise_models_gpu.py holds the HIP entries to it.

Inputs.  The far plane is designed, not an object: F_s = 0.5^s envelope x a
complex normal, the envelope falling `decades` decades in intensity from the DC
pixel to the corner (FFT order), the peak model intensity 6e4.  Counts are
min(Poisson(I u), 65535) with u uniform in (0.5, 1.5) per pixel; the patterns
of a case are PATTERNS[N]: six and nine decades, a dim-data pattern (u = 1e-3:
d << I at every bright pixel) and a hot pixel (one count forced to 65535 where
the model intensity is nearest 1).  No model intensity is exactly zero: there
the reference formulas give 0 / 0 as well (sqrt d / (0 + 1e-9) with d = 0 is
0, but d / (I + 1e-9) of a dark count and the dominant-mode step are
undefined), so such a pixel says nothing about an implementation.

Hand-off cases (256^2, 512^2): the kernels read the forward hand-off of
tike_fwd_pass1, built from an object identically 1, whole-number positions and
per-position probes complex64(IFFT2(F_design) / scale).  The model's far plane
is scale x FFT2 of THAT complex64 probe in complex128: exact for what the
kernel was given.

Bounds (margin 4 over a float32 restatement, the rule of cgrad_search.widened;
never from a kernel's output).  The restatement is the oracle's complex64
transform of the same probe (stored-input cases: the stored complex64 far
plane), float32 pixel formulas WITH the counts as given, float64 sums.
  e[n,s]   = 4 max_p |F32 - F64|  (0 for stored-input entries)
  dI       = sum_s (2 |F_s| e + e^2) + (S + 2) 2^-23 I
  a pixel quantity q(I), monotone in I: max(|q(I + dI) - q(I)|,
             |q(max(I - dI, 0)) - q(I)|) + 4 x 2^-23 (1 + |q|); unmeasured
             pixels must hold the stated value exactly
  gradient = |F_s| (factor's bound) + e (|factor| + its bound)
             + 4 x 2^-23 |F_s factor|   (a product of two bounded factors)
  a sum    = 1e-5 x the sum of the absolute terms + 4 x the restatement's error;
             through to alpha by the first-order propagation of `_alpha_bound`,
             each update adding 4 x 2^-23 (|alpha| + |w n / D|) for its own
             float32 arithmetic
  chi      = per tile, in the 2-norm: the 2-norm of its input's per-entry
             bounds + 4 x the 2-norm error of a complex64 transform."""
import collections
import functools

import numpy as np
import scipy.fft

from oracle import operators as ops

MODELS = ("gaussian", "poisson")
EPS = 1e-9
RTOL = 1e-5  # cgrad_search.RTOL
MARGIN = 4.0
U = 2.0**-23
PEAK = 6e4
STEP_START, WEIGHT = 0.7, 0.4
UNMEASURED = 0.7
# the patterns of a case with N positions
PATTERNS = {3: ("six+hot", "nine", "dim"), 2: ("nine+hot", "dim")}


# ---------------------------------------------------------------- the model
def intensity(F):
    return np.sum(np.abs(np.asarray(F, np.complex128))**2, axis=1)


def unmeasured_value(ums):
    """unmeasured_scaling - 1 as a float32 subtraction of float32 operands."""
    return float(np.float32(ums) - np.float32(1.0))


def _measured(mask, values, other=0.0):
    if mask is None:
        return values
    with np.errstate(invalid="ignore"):
        return np.where(mask, values, other)


def pixel_factor(model, I, d, eps=EPS):
    """The factor of a measured pixel."""
    with np.errstate(invalid="ignore", divide="ignore"):
        if model == 0:
            return -(1.0 - np.sqrt(d) / (np.sqrt(I) + eps))
        return -(1.0 - d / (I + eps))


def factor(model, I, d, mask=None, ums=1.0, eps=EPS):
    return _measured(mask, pixel_factor(model, I, d, eps),
                     unmeasured_value(ums))


def cost_terms(model, I, d, eps=EPS):
    with np.errstate(invalid="ignore", divide="ignore"):
        if model == 0:
            return (np.sqrt(I) - np.sqrt(d))**2
        return I - d * np.log(I + eps)


def count_measured(mask, det):
    return det * det if mask is None else int(mask.sum())


def costs(model, I, d, mask=None, eps=EPS):
    """(N,): the mean term over the measured pixels; also the mean |term|."""
    t = _measured(mask, cost_terms(model, I, d, eps))
    n = count_measured(mask, I.shape[-1])
    return t.sum(axis=(-2, -1)) / n, np.abs(t).sum(axis=(-2, -1)) / n


def gradient(F, fac):
    return np.asarray(F, np.complex128) * fac[:, None]


def _steps(F, I, d, mask, start, w, dominant, eps=EPS, detail=False):
    """exitwave.py:122-184 / :187-234 in float64: (N, S) step lengths.
    xi = 1 - d / (I + 1e-9);
      all modes, a = |F_s|^2:  D = sum xi^2 a,
          n(alpha) = sum xi a (1 + d (xi alpha - 1) / (a (xi alpha - 1)^2 + I - a))
      dominant:                D = sum xi^2 I,
          n(alpha) = sum xi (I - d / (1 - alpha xi))
      alpha <- (1 - w) alpha + w n(alpha) / D, twice from `start`."""
    N, S = F.shape[:2]
    with np.errstate(invalid="ignore", divide="ignore"):
        xi = (1.0 - d / (I + eps))[:, None]
    Ie, Im = I[:, None], d[:, None]
    a = Ie if dominant else np.abs(np.asarray(F, np.complex128))**2

    def total(t):
        t = _measured(mask, t)
        return t.sum(axis=(-2, -1)), np.abs(t).sum(axis=(-2, -1))

    def numer(alpha):
        al = alpha[..., None, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            if dominant:
                return total(xi * (Ie - Im / (1.0 - al * xi)))
            xam1 = xi * al - 1.0
            return total(xi * a * (1.0 + Im * xam1 /
                                   (a * xam1 * xam1 + Ie - a)))

    with np.errstate(invalid="ignore"):
        D, Dabs = total(xi * xi * a)
    alpha = np.full(D.shape, float(start))
    trail = []
    for _ in range(2):
        n, nabs = numer(alpha)
        h = 1e-6
        slope = (numer(alpha + h)[0] - numer(alpha - h)[0]) / (2 * h)
        trail.append((alpha, n, nabs, slope))
        alpha = alpha * (1.0 - w) + (n / D) * w
    if dominant:
        alpha = np.broadcast_to(alpha, (N, S)).copy()
    if detail:
        return alpha, D, Dabs, trail
    return alpha


def steps_all_modes(F, I, d, mask=None, start=STEP_START, w=WEIGHT, eps=EPS):
    return _steps(F, I, d, mask, start, w, False, eps)


def steps_dominant_mode(F, I, d, mask=None, start=STEP_START, w=WEIGHT,
                        eps=EPS):
    return _steps(F, I, d, mask, start, w, True, eps)


def scaled_gradient(F, fac, steps=None, mask=None):
    """F_s factor [step_s on measured pixels]: the input of chi's transform."""
    G = gradient(F, fac)
    if steps is not None:
        s = steps[:, :, None, None]
        G = G * (s if mask is None else np.where(mask, s, 1.0))
    return G


def chi(G, scale):
    """IFFT2(G) scale, the transform unnormalised."""
    return scipy.fft.ifft2(G, axes=(-2, -1), norm="forward") * scale


def model_outputs(model, F, I, d, mask, ums, scale, eps=EPS):
    """Every output of the model for one noise model: what `reference` holds
    the entries to, and what the CPU test perturbs."""
    fac = factor(model, I, d, mask, ums, eps)
    out = dict(factor=fac, gradient=gradient(F, fac),
               costs=costs(model, I, d, mask, eps)[0])
    steps = None
    if model == 1:
        steps = out["steps_all"] = steps_all_modes(F, I, d, mask, eps=eps)
        out["steps_dominant"] = steps_dominant_mode(F, I, d, mask, eps=eps)
    out["chi"] = chi(scaled_gradient(F, fac, steps, mask), scale)
    return out


# ------------------------------------------------------------------ bounds
def delta_intensity(F, I, e):
    """dI: (N, det, det); e (N, S)."""
    e = np.asarray(e, np.float64)[:, :, None, None]
    S = F.shape[1]
    return np.sum(2.0 * np.abs(F) * e + e * e, axis=1) + (S + 2) * U * I


def factor_bound(model, I, dI, d, mask=None, eps=EPS):
    """The bound of a pixel quantity for q = the factor; 0 where unmeasured."""
    q = pixel_factor(model, I, d, eps)
    up = np.abs(pixel_factor(model, I + dI, d, eps) - q)
    dn = np.abs(pixel_factor(model, np.maximum(I - dI, 0.0), d, eps) - q)
    with np.errstate(invalid="ignore"):
        b = np.maximum(up, dn) + MARGIN * U * (1.0 + np.abs(q))
    return _measured(mask, b)


def gradient_bound(F, fac, fbound, e):
    e = np.asarray(e, np.float64)[:, :, None, None]
    aF = np.abs(F)
    fb, af = fbound[:, None], np.abs(fac)[:, None]
    return aF * fb + e * (af + fb) + MARGIN * U * aF * af


def sum_bound(abs_terms, restated, want):
    return RTOL * abs_terms + MARGIN * np.abs(restated - want)


def _alpha_bound(D, Dabs, trail, w, restated, want):
    """alpha_{k+1} = (1 - w) alpha_k + w n(alpha_k) / D to first order in the
    errors of the sums (1e-5 of their absolute terms) and of alpha_k (the
    slope of n, by a central difference in the model), + 4 x the
    restatement's error in the step length."""
    dD = RTOL * Dabs
    b = np.zeros_like(D)
    for alpha, n, nabs, slope in trail:
        dn = RTOL * nabs + np.abs(slope) * b
        b = (1.0 - w) * b + w * (dn / np.abs(D) + np.abs(n) * dD / D**2)
        # the update itself is float32 arithmetic on a float32 step length:
        # the rounding term of a pixel quantity, on its two summands
        b = b + MARGIN * U * (np.abs(alpha) + np.abs(w * n / D))
    return b + MARGIN * np.abs(restated - want)


# -------------------------------------- the formulas in float32 (restatement)
def _f4(x):
    return np.asarray(x).astype(np.float32)


def intensity_float32(F32):
    a = np.asarray(F32, np.complex64)
    t = a.real * a.real + a.imag * a.imag
    out = np.zeros(t.shape[:1] + t.shape[2:], np.float32)
    for s in range(t.shape[1]):
        out = out + t[:, s]
    return out


def factor_float32(model, I32, d):
    f4 = np.float32
    I32, dv = _f4(I32), _f4(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        if model == 0:
            return -(f4(1) - np.sqrt(dv) / (np.sqrt(I32) + f4(EPS)))
        return -(f4(1) - dv / (I32 + f4(EPS)))


def cost_terms_float32(model, I32, d):
    f4 = np.float32
    I32, dv = _f4(I32), _f4(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        if model == 0:
            diff = np.sqrt(I32) - np.sqrt(dv)
            return diff * diff
        return I32 - dv * np.log(I32 + f4(EPS))


def costs_float32(model, I32, d, mask=None):
    t = _measured(mask, cost_terms_float32(model, I32, d)).astype(np.float64)
    return t.sum(axis=(-2, -1)) / count_measured(mask, I32.shape[-1])


def steps_float32(F32, I32, d, mask, start, w, dominant):
    """The step lengths with float32 pixel terms (the counts as given) and
    float64 sums."""
    f4 = np.float32
    I32, dv = _f4(I32), _f4(d)
    N, S = F32.shape[:2]
    with np.errstate(invalid="ignore", divide="ignore"):
        xi = (f4(1) - dv / (I32 + f4(EPS)))[:, None]
    Ie, Im = I32[:, None], dv[:, None]
    if dominant:
        a = Ie
    else:
        c = np.asarray(F32, np.complex64)
        a = c.real * c.real + c.imag * c.imag

    def total(t):
        return _measured(mask, t).astype(np.float64).sum(axis=(-2, -1))

    with np.errstate(invalid="ignore"):
        D = total(xi * xi * a)
    alpha = np.full(D.shape, f4(start), np.float32)
    for _ in range(2):
        al = alpha[..., None, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            if dominant:
                n = total(xi * (Ie - Im / (f4(1) - al * xi)))
            else:
                xam1 = xi * al - f4(1)
                n = total(xi * a * (f4(1) + Im * xam1 /
                                    (a * xam1 * xam1 + Ie - a)))
        alpha = (alpha * (f4(1) - f4(w)) + (n / D).astype(f4) * f4(w)).astype(
            f4)
    alpha = alpha.astype(np.float64)
    return np.broadcast_to(alpha, (N, S)).copy() if dominant else alpha


def transform_error(G, scale):
    """(N, S): the 2-norm error of a complex64 inverse transform of G."""
    g4 = scipy.fft.ifft2(G.astype(np.complex64), axes=(-2, -1),
                         norm="forward") * np.float32(scale)
    return np.linalg.norm(g4 - chi(G, scale), axis=(-2, -1))


# ---------------------------------------------------------------------- cases
# kind "stored": the entries read a stored far plane / intensity (e = 0);
# "handoff": the forward hand-off of tike_fwd_pass1.  masked: the module-gap
# mask; u16: 16-bit counts (unmeasured pixels 65535; float32: NaN).
Case = collections.namedtuple("Case", "name kind det S N masked u16")


def _c(kind, det, S, N, masked, u16=False):
    name = "{}-{}x{}n{}-{}{}".format(kind, det, S, N,
                                     "mask" if masked else "all",
                                     "-u16" if u16 else "")
    return Case(name, kind, det, S, N, masked, u16)


STORED_DETS = (24, 48, 15)
STORED_MODES = (1, 3, 8, 9)
HANDOFF_SHAPES = ((256, 1, 3), (256, 3, 3), (256, 6, 3), (256, 7, 3),
                  (256, 8, 3), (512, 1, 2), (512, 4, 2))
CASES = [_c("stored", det, S, 3, m) for det in STORED_DETS
         for S in STORED_MODES for m in (False, True)] + [
             _c("handoff", det, S, N, m, u) for det, S, N in HANDOFF_SHAPES
             for m in (False, True) for u in (False, True)]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def scale_of(det):
    return 1.0 / det  # "ortho"


def envelope(det, decades):
    """Intensity envelope in FFT order: 1 at the DC pixel, log-linear in the
    distance from it, 10^-decades at the Nyquist frequency of either axis and
    in the corners beyond (a radial fall-off, as a detector sees)."""
    f = np.minimum(np.arange(det), det - np.arange(det)) / (det // 2)
    r = np.sqrt(np.add.outer(f**2, f**2))
    return 10.0**(-decades * np.minimum(r, 1.0))


def detector_gap_mask(det, rng):
    """About 10 % random pixels, a full row and a full column unmeasured."""
    mask = rng.random((det, det)) >= 0.1
    mask[det // 3, :] = False
    mask[:, (2 * det) // 3 + 1] = False
    mask[0, 0] = True  # (the DC pixel carries the peak)
    return mask


@functools.lru_cache(maxsize=4)
def _design(kind, det, S, N):
    """What the cases of a shape share: the far plane as the kernels are given
    it, the model's and the restatement's far planes, the counts."""
    rng = np.random.default_rng([det, S, N, kind == "handoff"])
    scale = scale_of(det)
    kinds = PATTERNS[N]
    F = np.empty((N, S, det, det), np.complex128)
    for n, kind_n in enumerate(kinds):
        env = np.sqrt(envelope(det, 9 if kind_n.startswith("nine") else 6))
        z = (rng.standard_normal((S, det, det)) +
             1j * rng.standard_normal((S, det, det))) / np.sqrt(2.0)
        F[n] = env * z * 0.5**np.arange(S)[:, None, None]
        F[n] *= np.sqrt(PEAK / intensity(F[n:n + 1]).max())
    out = {}
    if kind == "handoff":
        probe = (scipy.fft.ifft2(F, axes=(-2, -1)) / scale).astype(
            np.complex64)
        F64 = scale * scipy.fft.fft2(probe.astype(np.complex128),
                                     axes=(-2, -1))
        F32 = ops.propagation_fwd(probe)
        assert F32.dtype == np.complex64
        e = MARGIN * np.abs(F32 - F64).max(axis=(-2, -1))
        out["probe"] = probe
    else:
        F32 = F.astype(np.complex64)
        F64 = F32.astype(np.complex128)
        e = np.zeros((N, S))
    I = intensity(F64)
    mask = detector_gap_mask(det, rng)
    u = rng.uniform(0.5, 1.5, I.shape)
    hot = {}
    for n, kind_n in enumerate(kinds):
        # the brightest pixel is measured, and counted at its expectation
        # (u = 1) so that the peak count of a bright pattern is near 6e4
        y, x = np.unravel_index(np.argmax(I[n]), I[n].shape)
        mask[y, x] = True
        u[n, y, x] = 1.0
        if kind_n == "dim":
            u[n] = 1e-3
    counts = np.minimum(rng.poisson(I * u), 65535).astype(np.float64)
    for n, kind_n in enumerate(kinds):
        if kind_n.endswith("+hot"):
            cand = np.where(mask, np.abs(np.log(I[n])), np.inf)
            y, x = np.unravel_index(np.argmin(cand), cand.shape)
            counts[n, y, x] = 65535.0
            hot[n] = (int(y), int(x))
    out.update(F=F64, F32=F32, e=e, I=I, counts=counts, gap=mask, hot=hot,
               kinds=kinds)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=8)
def inputs(name):
    """The inputs of a case: what the GPU test sends and the CPU test checks.
    Arrays are read-only (they are shared)."""
    c = BY_NAME[name]
    D = _design(c.kind, c.det, c.S, c.N)
    mask = D["gap"] if c.masked else None
    counts = D["counts"]
    if c.u16:
        data = counts.astype(np.uint16)
        if mask is not None:
            data[:, ~mask] = 65535
    else:
        data = counts.astype(np.float32)
        if mask is not None:
            data[:, ~mask] = np.nan
    # the stored intensity of the stored-input entries: the float32 nearest the
    # model's; the model then reads THAT value
    I32 = D["I"].astype(np.float32)
    out = dict(D, case=c, mask=mask, data=data,
               model_data=data.astype(np.float64), I32=I32,
               scale=scale_of(c.det),
               num_measured=count_measured(mask, c.det))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=8)
def reference(name, model, ums=UNMEASURED, stored_intensity=False,
              eps=EPS):
    """The model's answers for a case under a noise model, with their bounds.
    stored_intensity: the entry reads the float32 intensity `I32` instead of
    forming it from the far plane."""
    P = inputs(name)
    c = P["case"]
    F, F32, e, d, mask = P["F"], P["F32"], P["e"], P["model_data"], P["mask"]
    I = P["I32"].astype(np.float64) if stored_intensity else P["I"]
    I4 = P["I32"] if stored_intensity else intensity_float32(F32)
    dI = delta_intensity(F, I, e)
    out = dict(I=I, dI=dI)
    fac = factor(model, I, d, mask, ums, eps)
    fb = factor_bound(model, I, dI, d, mask, eps)
    out.update(factor=fac, factor_bound=fb, gradient=gradient(F, fac),
               gradient_bound=gradient_bound(F, fac, fb, e))
    cost, cabs = costs(model, I, d, mask, eps)
    c4 = costs_float32(model, I4, d, mask)
    out.update(costs=cost, costs_float32=c4,
               costs_bound=sum_bound(cabs, c4, cost))
    if model == 1:
        for dom, key in ((False, "steps_all"), (True, "steps_dominant")):
            alpha, D, Dabs, trail = _steps(F, I, d, mask, STEP_START, WEIGHT,
                                           dom, eps, detail=True)
            a4 = steps_float32(F32, I4, d, mask, STEP_START, WEIGHT, dom)
            b = _alpha_bound(D, Dabs, trail, WEIGHT, a4 if not dom else
                             a4[:, :1], alpha if not dom else alpha[:, :1])
            out[key] = alpha
            out[key + "_float32"] = a4
            out[key + "_bound"] = np.broadcast_to(b, alpha.shape).copy()
            out[key + "_denominator"] = D
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def chi_reference(name, model, ums, with_steps):
    """chi (N, S, det, det) of a case and its per-tile 2-norm bound (N, S);
    with_steps: the factor times the all-modes step lengths on measured pixels
    (poisson)."""
    P, R = inputs(name), reference(name, model, ums)
    mask, scale = P["mask"], P["scale"]
    steps = R["steps_all"] if with_steps else None
    G = scaled_gradient(P["F"], R["factor"], steps, mask)
    gb = np.array(R["gradient_bound"])
    if with_steps:
        s = np.abs(steps)[:, :, None, None]
        sb = R["steps_all_bound"][:, :, None, None]
        on = 1.0 if mask is None else mask
        gb = np.where(on, gb * (s + sb) + np.abs(R["gradient"]) * sb, gb)
    det = P["case"].det
    # (the unnormalised inverse of a det x det tile has 2-norm det)
    bound = (np.linalg.norm(gb, axis=(-2, -1)) * det * scale +
             MARGIN * transform_error(G, scale))
    want = chi(G, scale)
    want.setflags(write=False)
    return want, bound
