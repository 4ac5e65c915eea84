"""A float64 / complex128 model of the conjugate-gradient search entries
(tike_cgrad_line_search{,_masked}, tike_cgrad_line_search_linear{,_masked}) and
the table of cases both test files walk.  NumPy only: it imports without torch
or a GPU.

The model restates include/tike_amd.h, not the kernels: the far planes come
from a complex128 forward pass (oracle.operators' gather and probe product, then
a float64 FFT), the intensity of a trial is |A + s B|^2 formed directly (no
expansion into a quadratic in s), the costs are those of tests/cgrad_models.py,
and the decisions are a dozen lines of Python.
tests/test_cgrad_search_cpu.py pins the model and the preconditions of every
case; tests/test_cgrad_search_gpu.py holds the HIP entries to it.

Shapes: object (1, H, W), probe (1, 1, S, det, det), scan (N, 2), data
(N, det, det), far planes (N, S, det, det), cost rows (17, N)."""
import collections
import functools

import numpy as np
import scipy.fft

import cgrad_models as cm
from oracle import operators as ops

STEPS = 8  # step lengths per pass
ROWS = 2 * STEPS + 1  # cost rows: x, then every step length of the two passes
MODELS = ("gaussian", "poisson")

# the bound of a cost row (test_linear_masked_entry_row_sums_vs_numpy holds
# the row sums to it), applied per pattern, to the means and to `fx`
RTOL, FLOOR = 1e-5, 2e-10
CLEAR = 100.0  # a decision is clear at this many bounds from the bar


def row_bound(want, row0):
    """|got - want| may be 1e-5 |want| + 2e-10 |row 0|."""
    return RTOL * np.abs(want) + FLOOR * np.abs(row0)


# ------------------------------------------------------------ the forward model
def forward(psi, scan, probe, det):
    """F = FFT2(patch_n(psi) probe_s), ortho, in complex128: (N, S, det, det).
    (The gather weights are the float32 fractions of the scan positions, as
    they are for every implementation of the operator.)"""
    near = ops.convolution_fwd(
        np.asarray(psi, np.complex128)[0], np.asarray(scan, np.float32),
        np.asarray(probe, np.complex128)[..., 0, :, :, :], det)
    return scipy.fft.fft2(near, axes=(-2, -1), norm="ortho")


def far_planes(variable, x, d, other, scan, det):
    """A = F(x) and B = F(d): the direction in place of the object
    (variable 0) or of the probe (variable 1)."""
    if variable == 0:
        return forward(x, scan, other, det), forward(d, scan, other, det)
    return forward(other, scan, x, det), forward(other, scan, d, det)


def intensity(A, B, s):
    """sum_m |A_m + s B_m|^2: (N, det, det) float64."""
    return np.sum(np.abs(A + float(s) * B)**2, axis=1)


def step_lengths(step0):
    """The 16 candidates step0 / 2^k, halved in float32 as the entries do."""
    s, out = np.float32(step0), []
    for _ in range(ROWS - 1):
        out.append(float(s))
        s = np.float32(s * np.float32(0.5))
    return out


def _measured(mask, values):
    if mask is None:
        return values
    with np.errstate(invalid="ignore"):
        return np.where(mask, values, 0.0)


def plain_rows(A, B, data, mask, model, step0):
    """(17, N): each pattern's mean plain term over its measured pixels at x
    (row 0) and at x + step0 / 2^k d (rows 1..16)."""
    name = MODELS[model]
    return np.stack([cm.cost_each(name, data, intensity(A, B, s), mask)
                     for s in [0.0] + step_lengths(step0)])


def cost_rows(A, B, data, mask, model, step0):
    """(17, N) as the linear entries leave `costs_k`: row 0 the plain term at
    x; rows 1..16 at step0 / 2^k the plain gaussian cost, or the poisson
    difference from x, per pixel (I(s) - I0) - d log1p((I(s) - I0) / (I0 +
    1e-9)), summed over the measured pixels."""
    if model == 0:
        return plain_rows(A, B, data, mask, model, step0)
    d64 = np.asarray(data, np.float64)
    n = d64.shape[-1] * d64.shape[-2] if mask is None else int(mask.sum())
    I0 = intensity(A, B, 0.0)
    rows = [cm.cost_each("poisson", d64, I0, mask)]
    for s in step_lengths(step0):
        dI = intensity(A, B, s) - I0
        with np.errstate(invalid="ignore"):
            t = dI - d64 * np.log1p(dI / (I0 + 1e-9))
        rows.append(_measured(mask, t).sum(axis=(-2, -1)) / n)
    return np.stack(rows)


# ------------------------------------- the entries' formulas in float32 NumPy
def _fma(a, b, c):
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def far_planes_float32(variable, x, d, other, scan, det):
    """A and B as a float32 implementation holds them: the oracle's
    complex64 forward pass (float32 gather, probe product and FFT), returned
    as complex128 (N, S, det, det)."""
    def fwd(psi, probe):
        return ops.ptycho_fwd(probe, scan, psi, det)[:, 0].astype(
            np.complex128)
    if variable == 0:
        return fwd(x, other), fwd(d, other)
    return fwd(other, x), fwd(other, d)


def plain_rows_float32(A, B, data, mask, model, step0):
    """plain_rows in float32 (the trial entries form I of x + s d itself)."""
    f4 = np.float32
    with np.errstate(invalid="ignore"):
        dv = np.asarray(data).astype(f4)
    n = f4(dv.shape[-1] * dv.shape[-2] if mask is None else int(mask.sum()))
    rows = []
    for s in [0.0] + step_lengths(step0):
        I = np.sum(np.abs((A + s * B).astype(np.complex64))**2, axis=1,
                   dtype=f4)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = ((np.sqrt(I) - np.sqrt(dv))**2 if model == 0 else
                 _fma(-dv, np.log(I + f4(1e-9)), I))
        rows.append(_measured(mask, t).astype(f4).sum(axis=(-2, -1),
                                                      dtype=f4) / n)
    return np.stack(rows).astype(np.float64)


def cost_rows_float32(A, B, data, mask, model, step0):
    """cost_rows by the per-pixel formulas the header gives for the linear
    entries, evaluated in float32 from the float64 far planes: the quadratic
    I0 + s (s I1 + 2 C) of the three per-pixel sums, clamped at 0; the poisson
    difference dI - d log1p(dI / (I0 + 1e-9)) with dI = s (s I1 + 2 C) clamped
    at -I0 and log1p(r) = log(u) + (r - (u - 1)) max(2 - u, 0) for u the
    rounded 1 + r.  Sums are NumPy's pairwise float32 sums.  With the far
    planes of far_planes_float32: what float32 rounding alone does to a row --
    the measure a bound is widened by (`widened`), never a reference."""
    f4 = np.float32
    I0 = np.sum(np.abs(A)**2, axis=1).astype(f4)
    C = np.sum((np.conj(A) * B).real, axis=1).astype(f4)
    I1 = np.sum(np.abs(B)**2, axis=1).astype(f4)
    with np.errstate(invalid="ignore"):
        dv = np.asarray(data).astype(f4)
    n = f4(dv.shape[-1] * dv.shape[-2] if mask is None else int(mask.sum()))
    c2 = f4(2) * C

    def total(t):
        return _measured(mask, t).astype(f4).sum(axis=(-2, -1), dtype=f4) / n

    with np.errstate(invalid="ignore", divide="ignore"):
        if model == 0:
            sd = np.sqrt(dv)
            rows = [total((np.sqrt(I0) - sd)**2)]
            for s in step_lengths(step0):
                s = f4(s)
                I = np.maximum(_fma(s, _fma(s, I1, c2), I0), f4(0))
                rows.append(total((np.sqrt(I) - sd)**2))
            return np.stack(rows).astype(np.float64)
        e0 = I0 + f4(1e-9)
        inv0 = f4(1) / e0
        rows = [total(_fma(-dv, np.log(e0), I0))]
        for s in step_lengths(step0):
            s = f4(s)
            dI = np.maximum(s * _fma(s, I1, c2), -I0)
            I = I0 + dI
            r = dI * inv0
            u = (I + f4(1e-9)) * inv0
            lp = _fma(r - (u - f4(1)), np.maximum(f4(2) - u, f4(0)), np.log(u))
            rows.append(total(_fma(-dv, lp, dI)))
    return np.stack(rows).astype(np.float64)


def widened(want, float32_rows):
    """The bound of every entry of `want` (17, N).  Where the float32
    restatement of a row itself misses the row bound, on any pattern, float32
    rounding and not an implementation sets the error: that row's bound is 4 x
    the restatement's largest error in the row (it sums in another order than
    wave reductions and atomics do, and the size of a row's rounding error
    goes with the magnitude of the terms summed, which the patterns share).
    Returns (bound, the restatement's error / row bound)."""
    base = row_bound(want, want[0])
    err = np.abs(float32_rows - want)
    ratio = err / base
    wide = 4.0 * err.max(axis=1, keepdims=True) * np.ones_like(base)
    return np.where(ratio.max(axis=1, keepdims=True) > 1.0,
                    np.maximum(base, wide), base), ratio


# ------------------------------------------------------------------ decisions
def decide(means, fx_in, step0, first, last, relative, trials=0.0,
           failures=0.0):
    """The rule of ls_pick_kernel / ls_pick_sums_kernel on one pass: `means`
    are the 17 row means, of which the pass reads rows 1..8 (first) or 9..16
    and, on a first pass, row 0 for fx.  Returns { fx, step, done, trials,
    failures }."""
    row1 = 1 if first else 1 + STEPS
    fx = float(means[0]) if first else float(fx_in)
    bar = 0.0 if relative else fx
    s = np.float32(step0)
    for k in range(STEPS):
        m = float(means[row1 + k])
        if m <= bar:  # (NaN: never)
            return np.array([fx + m if relative else m, float(s), 1.0,
                             trials + k + 1, failures])
        s = np.float32(s * np.float32(0.5))
    return np.array([fx, float(s), 0.0, trials + STEPS,
                     failures + (1.0 if last else 0.0)])


def search_linear(means, state, relative):
    """Two passes of `decide` from state { fx, step, done, trials, failures }
    (fx on entry is not read; the second pass returns at once when the first
    accepted).  Returns the state afterwards."""
    st = decide(means, state[0], state[1], True, False, relative, state[3],
                state[4])
    if st[2] == 0.0:
        st = decide(means, st[0], st[1], False, True, relative, st[3], st[4])
    return st


def apply_step(x, d, state):
    """xs of the linear entries: x + step d when a step was accepted, else x
    (complex128; the step is the float32 the entries multiply with)."""
    a = float(np.float32(state[1])) if state[2] != 0.0 else 0.0
    return np.asarray(x, np.complex128) + a * np.asarray(d, np.complex128)


def xs_bound(x, d, a):
    """One multiply-add per component: 2^-23 (|x| + |a d|), on the real and
    on the imaginary parts (returned as a complex array of the two bounds)."""
    x, d = np.asarray(x, np.complex128), np.asarray(d, np.complex128)
    return 2.0**-23 * ((np.abs(x.real) + abs(a) * np.abs(d.real)) + 1j *
                       (np.abs(x.imag) + abs(a) * np.abs(d.imag)))


def search_trials(cost_of_step, fx, step, nslots, trials=0.0, failures=0.0):
    """The protocol of ls_decide_kernel: step lengths step / 2^k, one at a
    time, accepted when the mean cost is no larger than fx.  Returns (state,
    the last step length tried): xs = x + that d."""
    s = np.float32(step)
    for k in range(nslots):
        tried = float(s)
        f = float(cost_of_step(tried))
        trials += 1.0
        if f <= fx:
            return np.array([f, tried, 1.0, trials, failures]), tried
        s = np.float32(s * np.float32(0.5))
    return np.array([fx, float(s), 0.0, trials, failures + 1.0]), tried


def table_means(row0, first8=None, second8=None):
    """17 row means: row 0, rows 1..8, rows 9..16 (1e30 where not given)."""
    m = np.full(ROWS, 1e30)
    m[0] = row0
    if first8 is not None:
        m[1:1 + STEPS] = first8
    if second8 is not None:
        m[1 + STEPS:] = second8
    return m


_NAN = float("nan")
# The decision rule, written out by hand: (means of the pass's 8 rows, fx,
# step0, first pass (else the second, which is the last), relative, trials and
# failures on entry, { fx, step, done, trials, failures } afterwards).  fx is
# row 0's mean on a first pass and state[0] on the second.
DECIDE_TABLE = [
    # an accept at k = 0
    ([3.0, 9, 9, 9, 9, 9, 9, 9], 4.0, 2.0, True, 0, 0.0, 0.0,
     [3.0, 2.0, 1.0, 1.0, 0.0]),
    # an accept in the middle (k = 3), counters carried
    ([9, 9, 9, 3.5, 1, 1, 1, 1], 4.0, 2.0, True, 0, 5.0, 2.0,
     [3.5, 0.25, 1.0, 9.0, 2.0]),
    # a tie, mean == bar, is accepted
    ([9, 4.0, 1, 1, 1, 1, 1, 1], 4.0, 1.0, True, 0, 0.0, 0.0,
     [4.0, 0.5, 1.0, 2.0, 0.0]),
    # a tie on the second pass
    ([9, 9, 9, 9, 9, 9, 9, 4.0], 4.0, 1.0, False, 0, 8.0, 0.0,
     [4.0, 2.0**-7, 1.0, 16.0, 0.0]),
    # a NaN row is never accepted; the next finite one is
    ([_NAN, _NAN, 2.0, 1, 1, 1, 1, 1], 4.0, 1.0, True, 0, 0.0, 0.0,
     [2.0, 0.25, 1.0, 3.0, 0.0]),
    # nothing accepted, not the last pass: no failure, step / 2^8
    ([5, 5, 5, 5, 5, 5, 5, _NAN], 4.0, 1.0, True, 0, 1.0, 1.0,
     [4.0, 2.0**-8, 0.0, 9.0, 1.0]),
    # nothing accepted, the last pass: one failure
    ([5, 5, 5, 5, 5, 5, 5, 5], 4.0, 2.0**-8, False, 0, 8.0, 1.0,
     [4.0, 2.0**-16, 0.0, 16.0, 2.0]),
    # a second pass that accepts at k = 7
    ([5, 5, 5, 5, 5, 5, 5, 3.0], 4.0, 2.0**-8, False, 0, 8.0, 0.0,
     [3.0, 2.0**-15, 1.0, 16.0, 0.0]),
    # relative: a mean of exactly 0 is accepted; fx = fx + mean
    ([1e-3, 0.0, -1, -1, -1, -1, -1, -1], 4.0, 1.0, True, 1, 0.0, 0.0,
     [4.0, 0.5, 1.0, 2.0, 0.0]),
    # relative: a negative difference, fx moves by it
    ([0.5, 0.25, -0.125, -1, -1, -1, -1, -1], 4.0, 1.0, True, 1, 0.0, 0.0,
     [3.875, 0.25, 1.0, 3.0, 0.0]),
    # relative, second pass: fx = state[0] + the difference
    ([0.5, _NAN, -0.25, -1, -1, -1, -1, -1], 4.0, 2.0**-8, False, 1, 8.0, 0.0,
     [3.75, 2.0**-10, 1.0, 11.0, 0.0]),
    # relative: values below fx but above 0 are NOT accepted
    ([3, 3, 3, 3, 3, 3, 3, 3], 4.0, 1.0, False, 1, 0.0, 0.0,
     [4.0, 2.0**-8, 0.0, 8.0, 1.0]),
    ([3, 3, 3, 3, 3, 3, 3, 3], 4.0, 1.0, True, 1, 0.0, 0.0,
     [4.0, 2.0**-8, 0.0, 8.0, 0.0]),
]


def accepted_index(means, relative):
    """Index 0..15 of the first candidate row the search accepts, or None."""
    bar = 0.0 if relative else float(means[0])
    for k in range(ROWS - 1):
        if means[1 + k] <= bar:
            return k
    return None


def clarity(means, relative, upto=None):
    """min over the candidates decided (up to and including the accepted one,
    or `upto`, or all 16) of |mean_k - bar| / bound(mean_k): the decisions are
    the model's alone when this is at least CLEAR."""
    bar = 0.0 if relative else float(means[0])
    acc = accepted_index(means, relative)
    last = (ROWS - 2 if acc is None else acc) if upto is None else upto
    m = np.asarray(means[1:2 + last], np.float64)
    return float(np.min(np.abs(m - bar) / row_bound(m, means[0])))


# ---------------------------------------------------------------------- cases
# variable 0 object / 1 probe; model 0 gaussian / 1 poisson; masked: the
# measured-pixel mask of cm.detector_mask (False: measured = NULL); u16: 16-bit
# counts; descent: along -gradient (False: +gradient, which nothing accepts);
# log2step: first step = 2^log2step; bucket: where the model accepts (the CPU
# test holds the table to it): "0", "1-7", "8-15", "none".
Case = collections.namedtuple(
    "Case", "name det S N variable model masked u16 descent log2step bucket "
    "seed")


def _c(det, S, N, variable, model, masked, u16, descent, log2step, bucket,
       seed=1):
    name = "{}x{}n{}-{}-{}-{}{}-{}".format(
        det, S, N, "probe" if variable else "object", MODELS[model],
        "mask" if masked else "all", "-u16" if u16 else "", bucket)
    return Case(name, det, S, N, variable, model, masked, u16, descent,
                log2step, bucket, seed)


def _size(det, u16):
    return [
        _c(det, 1, 3, 0, 0, True, False, True, -1, "0"),
        _c(det, 3, 4, 0, 1, False, False, True, 4, "1-7"),
        _c(det, 3, 5, 1, 0, False, False, True, 11, "8-15"),
        _c(det, 1, 3, 1, 1, True, False, False, 6, "none"),
        _c(det, 3, 4, 0, 0, True, u16, False, 10, "none"),
        _c(det, 1, 5, 0, 1, True, u16, True, 11, "8-15"),
        _c(det, 1, 4, 1, 0, False, u16, True, 4, "1-7"),
        _c(det, 3, 3, 1, 1, False, u16, True, -1, "0"),
        _c(det, 1, 4, 1, 1, True, False, True, 11, "8-15"),
    ]


CASES = _size(128, False) + _size(256, True) + _size(512, True) + [
    _c(256, 8, 3, 0, 0, True, False, True, 4, "1-7"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the trial-by-trial entries: (case, k0, nslots, what the model does); the
# first step tried is the case's candidate k0, step0 / 2^k0
TRIALS = [
    ("128x1n3-object-gaussian-mask-0", 0, 1, "first"),
    ("128x1n3-probe-poisson-mask-none", 0, 1, "out"),
    ("128x3n4-object-poisson-all-1-7", 0, 30, "later"),
    ("256x1n4-probe-gaussian-all-u16-1-7", 0, 30, "later"),
    ("256x3n3-probe-poisson-all-u16-0", 0, 4, "first"),
    ("256x3n4-object-gaussian-mask-u16-none", 0, 4, "out"),
    ("256x1n5-object-poisson-mask-u16-8-15", 0, 4, "out"),
    ("512x3n5-probe-gaussian-all-8-15", 0, 30, "later"),
    ("512x1n3-probe-poisson-mask-none", 0, 4, "out"),
    ("512x3n4-object-poisson-all-1-7", 3, 4, "later"),
    ("128x1n4-probe-gaussian-all-1-7", 2, 4, "later"),
]


def _window(det, rin=0.6):
    """Flat-top amplitude: 1 inside rin of the half-width, a linear ramp to 0
    at the edge."""
    o = (np.arange(det) + 0.5) - det / 2
    r = np.sqrt(np.add.outer(o**2, o**2)) / (det / 2)
    return np.clip((1.0 - r) / (1.0 - rin), 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The inputs of a case, from its seed: what the GPU test sends and the CPU
    test checks.  Arrays are read-only (they are shared)."""
    c = BY_NAME[name]
    det, S, N = c.det, c.S, c.N
    rng = np.random.default_rng([c.seed, det, S, N, c.variable, c.model])
    HW = det + 24
    scan = (1.0 + 21.0 * rng.random((N, 2))).astype(np.float32)
    psi_true = ((0.75 + 0.25 * rng.random((1, HW, HW))) * np.exp(
        1j * np.pi * (rng.random((1, HW, HW)) - 0.5))).astype(np.complex64)
    # (16-bit counts: an amplitude that fills a good part of their range)
    amp = 30.0 if c.u16 else 1.0
    w = _window(det)
    probe = np.stack([amp * w * np.exp(1j * np.pi * rng.random((det, det))) /
                      (m + 1) for m in range(S)])[None, None].astype(
                          np.complex64)
    data = ops.simulate(det, probe, scan, psi_true).astype(np.float32)
    mask = cm.detector_mask(det) if c.masked else None
    if c.u16:
        data = np.rint(np.minimum(data, 60000)).astype(np.uint16)
        model_data = data.astype(np.float64)
    else:
        if mask is not None:
            data[:, ~mask] = np.nan
        model_data = data
    psi = (0.9 * psi_true).astype(np.complex64)
    grad = cm.grad_probe if c.variable else cm.grad_psi
    with np.errstate(invalid="ignore"):
        g = grad(MODELS[c.model], model_data.astype(np.float32), psi, scan,
                 probe, det, mask)
    x, other = (probe, psi) if c.variable else (psi, probe)
    # the model's descent direction, scaled so that a step of 1 moves x by
    # 20 % (as the entry test of tests/test_cgrad_models_gpu.py does)
    sign = -1.0 if c.descent else 1.0
    d = (sign * 0.2 * np.linalg.norm(x) / np.linalg.norm(g) * g).astype(
        np.complex64).reshape(x.shape)
    out = dict(case=c, scan=scan, data=data, model_data=model_data, mask=mask,
               x=x, d=d, other=other, step0=2.0**c.log2step,
               num_measured=det * det if mask is None else int(mask.sum()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The model's answer for a case: cost rows, plain rows, the row means, the
    state after the linear search and its xs."""
    P = inputs(name)
    c = P["case"]
    A, B = far_planes(c.variable, P["x"], P["d"], P["other"], P["scan"], c.det)
    rows = cost_rows(A, B, P["model_data"], P["mask"], c.model, P["step0"])
    plain = rows if c.model == 0 else plain_rows(
        A, B, P["model_data"], P["mask"], c.model, P["step0"])
    means = rows.sum(axis=1) / c.N
    state = search_linear(means, [0.0, P["step0"], 0.0, 0.0, 0.0], c.model)
    A4, B4 = far_planes_float32(c.variable, P["x"], P["d"], P["other"],
                                P["scan"], c.det)
    bound, f32 = widened(rows, cost_rows_float32(
        A4, B4, P["model_data"], P["mask"], c.model, P["step0"]))
    plain_bound, plain_f32 = widened(plain, plain_rows_float32(
        A4, B4, P["model_data"], P["mask"], c.model, P["step0"]))
    # the row sums: the project's bound on them; a widened row: the sum of its
    # entries' bounds
    sums = rows.sum(axis=1)
    sum_bound = np.where(f32.max(axis=1) > 1.0, bound.sum(axis=1),
                         row_bound(sums, sums[0]))
    out = dict(rows=rows, plain=plain, means=means, state=state, bound=bound,
               float32_ratio=f32, plain_bound=plain_bound,
               plain_float32_ratio=plain_f32, sum_bound=sum_bound,
               accepted=accepted_index(means, c.model),
               xs=apply_step(P["x"], P["d"], state))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def in_bucket(accepted, bucket):
    return {"0": accepted == 0,
            "1-7": accepted is not None and 1 <= accepted <= 7,
            "8-15": accepted is not None and 8 <= accepted <= 15,
            "none": accepted is None}[bucket]


def trial_reference(name, k0, nslots):
    """The trial-by-trial search of a case in the model, from its candidate
    k0 on: (state, the last step length tried, the mean plain costs of x and
    of the 16 candidates)."""
    P, R = inputs(name), reference(name)
    steps = step_lengths(P["step0"])
    means = R["plain"].sum(axis=1) / P["case"].N
    cost = dict(zip(steps, means[1:]))
    st, tried = search_trials(cost.__getitem__, means[0], steps[k0], nslots)
    return st, tried, means
