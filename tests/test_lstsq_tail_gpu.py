"""The lstsq_grad minibatch tail, entry by entry, against the float64 model of
tests/lstsq_tail.py (itself pinned to the oracle by test_lstsq_tail_cpu.py).

Every case calls the C entry with raw pointers, on synthetic inputs with a
fixed seed.  Output buffers start as NaN, in-place arrays from random contents,
and every buffer a kernel may write carries 64 floats of a known pattern behind
its logical end that must come back untouched.

Sizes: more than 256 positions (the one-workgroup loops over positions take a
second round at 257 and four at 1000), pixel counts that are no multiple of
256, at and above the 64-workgroup cap of the normalisation kernels (16384,
16900, 65536), element counts above the 2048-workgroup grid cap
(2048 * 256 + 300), empty shares (B = 0), every `recover_*` combination, NULL
for every optional pointer, row strides of (C, S, m) = (1, 2, 0) and (2, 3, 1).

Bars.  Sums over pixels: rtol 2e-4, atol 2e-5 max|want| (the bar of
test_step_statistics_on_pairs_vs_numpy).  Arrays: assert_close at OP_NORMWISE /
OP_MAXABS.  Scalar arithmetic (solves, step lengths, weights, `steps`): 8 x
the error of the same formulas evaluated in float32 NumPy on the case's own
inputs, and not below 1e-6.  Those float32 errors, the largest over the cases of
each entry (MEASURED collects them as the cases run):
  step_sums 1.4e-07   step_solve 2.9e-07   eigen_weights0 1.1e-07
  eigen_proj_mean 1.2e-07   eigen_dsum 8.3e-08   eigen_weights 1.3e-07
  tail_mid 2.5e-07   tail_solve1 2.5e-07   tail_finish 1.7e-07
  two ranks (steps ; weights) 2.2e-07 ; 2.6e-07   pixel_update1 sums3 1.1e-07
so every scalar bar is 8 x a figure between 1e-7 and 3e-7, or the floor."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import lstsq_tail as lt
from util import OP_MAXABS, OP_NORMWISE, assert_close

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = (np.arange(GUARD, dtype=np.float32) * 0.5 - 1234.0)
EPS = 2.5e-3  # large enough that dropping it is seen at the scalar bars
BS = [1, 63, 256, 257, 1000]
BS0 = [0] + BS
RECOVER = [(True, True), (True, False), (False, True)]
STRIDES = [(1, 2, 0), (2, 3, 1)]  # (C, S, m)
ABOVE_GRID_CAP = 2048 * 256 + 300
MEASURED = {}  # entry -> largest float32-restatement error seen (the docstring)


def _api():
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    return A, check, lib


def rc(rng, *shape):
    return (rng.random((*shape, 2), dtype=np.float32) - 0.5).view(
        np.complex64)[..., 0]


class Dev:
    """A device buffer of float32 or complex64 with GUARD floats of PATTERN
    behind its logical end; NaN unless `init` gives its contents."""

    def __init__(self, shape, cplx=False, init=None):
        A, _, _ = _api()
        self.shape, self.cplx = tuple(np.atleast_1d(shape)), cplx
        self.n = int(np.prod(self.shape)) * (2 if cplx else 1)
        host = np.full(self.n + GUARD, np.nan, np.float32)
        if init is not None:
            a = np.ascontiguousarray(
                np.broadcast_to(init, self.shape),
                dtype=np.complex64 if cplx else np.float32)
            host[:self.n] = a.view(np.float32).ravel()
        host[self.n:] = PATTERN
        self.flat = A.to_device(host)

    def ptr(self, offset=0):
        """Address of float (or complex) element `offset` of the buffer."""
        return self.flat.data_ptr() + offset * (8 if self.cplx else 4)

    def get(self):
        host = self.flat.cpu().numpy()
        np.testing.assert_array_equal(host[self.n:], PATTERN,
                                      err_msg="written past the end")
        a = host[:self.n].copy()
        return (a.view(np.complex64) if self.cplx else a).reshape(self.shape)


def dev(x):
    A, _, _ = _api()
    return None if x is None else A.to_device(np.ascontiguousarray(x))


def dptr(t):
    return None if t is None else t.data_ptr()


def bar(entry, fn, *args, **kwargs):
    """The scalar bar of this case (and the measured float32 error, kept for
    the module docstring)."""
    e = lt.float32_error(fn, *args, **kwargs)
    MEASURED[entry] = max(MEASURED.get(entry, 0.0), e)
    return lt.scalar_bar(e)


def check_scalar(got, want, tol, what, metric=lt.rel_each):
    err = metric(got, want)
    print(f"{what}: error {err:.2e} (bar {tol:.2e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}\n{got}\n{want}"


def check_sums(got, want, what):
    """Sums over pixels."""
    want = np.asarray(want, np.float64)
    np.testing.assert_allclose(got, want, rtol=2e-4,
                               atol=2e-5 * np.abs(want).max(), err_msg=what)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def solve_case(B, allrank=False):
    """stats (B, 8), costs, and the sums / count the solve runs with: the local
    sums and B, or (allrank) sums and a count of a larger minibatch this is a
    share of.  The conditions the issue sets are asserted on the float64
    solutions: A1, A4 positive over two decades, |A2|^2 <= A1 A4 / 2, between
    a quarter and three quarters of the rows with Re x1 < 0 and the same for
    x2 (B = 1: x1 < 0 < x2, one clamped and one not), stats7 away from zero."""
    for attempt in range(200):
        rng = np.random.default_rng(7919 * attempt + 31 * B + allrank)
        s = np.empty((B, 8), np.float32)
        s[:, 0] = 10**rng.uniform(-1, 1, B)
        s[:, 1] = 10**rng.uniform(-1, 1, B)
        r = np.sqrt(rng.uniform(0.05, 0.45, B) * s[:, 0] * s[:, 1])
        ph = rng.uniform(0, 2 * np.pi, B)
        s[:, 2], s[:, 3] = r * np.cos(ph), r * np.sin(ph)
        s[:, 4] = rng.standard_normal(B) * np.sqrt(s[:, 0])
        s[:, 5] = rng.standard_normal(B) * np.sqrt(s[:, 1])
        s[:, 6] = rng.standard_normal(B)
        s[:, 7] = 0.5 + rng.random(B)
        costs = (rng.random(B) + 0.1).astype(np.float32)
        sums = lt.step_sums(s, costs, EPS)
        count = float(max(B, 1))
        if allrank:
            sums = 1.7 * sums + np.array([3.0, 5.0, 2.0])
            count = float(B + 337)
        sums = sums.astype(np.float32)
        if B == 0:
            break
        x1, x2 = lt.solve(s, EPS, sums, count, True, True)
        n1, n2 = np.mean(x1.real < 0), np.mean(x2.real < 0)
        if (B == 1 and x1.real[0] < 0 < x2.real[0]) or (
                B >= 4 and 0.25 <= n1 <= 0.75 and 0.25 <= n2 <= 0.75):
            break
    else:
        raise AssertionError("no inputs meet the conditions")
    if B:
        A1 = s[:, 0] + EPS + 0.5 * sums[0] / count
        A4 = s[:, 1] + EPS + 0.5 * sums[1] / count
        assert np.all(s[:, :2] > 0) and s[:, 7].min() >= 0.5
        assert np.all(s[:, 2]**2 + s[:, 3]**2 <= 0.5 * A1 * A4)
        if B >= 4:
            assert s[:, 0].max() / s[:, 0].min() > 30
            assert s[:, 1].max() / s[:, 1].min() > 30
    return s, costs, sums, count


@functools.lru_cache(maxsize=None)
def sums5_case(B, P):
    rng = np.random.default_rng(5 * B + 1)
    s = (rng.standard_normal((B, 5)) * P * 0.2).astype(np.float32)
    s[:, 2] = P * (0.5 + rng.random(B))  # sum |O E|^2 > 0
    return s


def _stats_ptr(s):
    return dev(s) if len(s) else None


# ------------------------------------------- (a) scalar, position-sized entries
@pytest.mark.parametrize("costs_given", [False, True])
@pytest.mark.parametrize("B", BS0)
def test_step_sums(B, costs_given):
    """tike_lstsq_step_sums; costs NULL: sums[2] = 0; B = 0: zeros."""
    A, check, lib = _api()
    s, costs, _, _ = solve_case(B)
    costs = costs if costs_given else None
    out = Dev(3)
    sd, cd = _stats_ptr(s), dev(costs) if B else None
    check(lib.tike_lstsq_step_sums(dptr(sd), dptr(cd), B, EPS, out.ptr(),
                                   A.stream_ptr()))
    want = lt.step_sums(s, costs if B else None, EPS)
    check_scalar(out.get(), want,
                 bar("step_sums", lt.step_sums, s, costs if B else None, EPS,
                     metric=lt.rel_each), "sums")


@pytest.mark.parametrize("allrank", [False, True])
@pytest.mark.parametrize("recover", RECOVER)
@pytest.mark.parametrize("B", BS0)
def test_step_solve(B, recover, allrank):
    """tike_lstsq_step_solve: the real-part shortcut against the complex
    solve, the clamp at zero, the three recover_* branches; count = B with the
    local sums, and a count over all ranks with sums that are not the local
    ones.  B = 0: { 0, 0, 0, 0, sums[2] / count }."""
    A, check, lib = _api()
    s, _, sums, count = solve_case(B, allrank)
    out = Dev(5)
    sd, sumd = _stats_ptr(s), dev(sums)
    check(lib.tike_lstsq_step_solve(dptr(sd), B, EPS, dptr(sumd), count,
                                    int(recover[0]), int(recover[1]),
                                    out.ptr(), A.stream_ptr()))
    args = (s, EPS, sums, count) + recover
    check_scalar(out.get(), lt.step_solve(*args),
                 bar("step_solve", lt.step_solve, *args, metric=lt.rel_each),
                 "out")


def _weights_case(B, C, S, seed=0):
    rng = np.random.default_rng(100 * B + 10 * C + S + seed)
    return (rng.standard_normal((B, C + 1, S)) * 0.4 + 1).astype(np.float32)


def _only_column_changed(got, before, want, c, m, tol, what):
    """Column [:, c, m] of the (B, C + 1, S) array against `want`; every other
    element bit-for-bit what it was."""
    keep = np.ones(before.shape, bool)
    keep[:, c, m] = False
    np.testing.assert_array_equal(got[keep], before[keep],
                                  err_msg=f"{what}: wrote outside its column")
    if before.shape[0]:
        check_scalar(got[:, c, m], want, tol, what, metric=lt.rel_max)


@pytest.mark.parametrize("C,S,m", STRIDES)
@pytest.mark.parametrize("B", BS0)
def test_eigen_weights0(B, C, S, m):
    """tike_eigen_weights0.  B = 0 used to leave `norms` unwritten although the
    caller all-reduces it: an empty share now contributes zeros."""
    A, check, lib = _api()
    s = solve_case(B)[0]
    w = _weights_case(B, C, S)
    wd, norms, sd = Dev(w.shape, init=w), Dev(C), _stats_ptr(s)
    check(lib.tike_eigen_weights0(wd.ptr(), dptr(sd), B, C, S, m, norms.ptr(),
                                  A.stream_ptr()))
    want_w, want_n = lt.eigen_weights0(w, s, m)
    tol = bar("eigen_weights0", lt.eigen_weights0, w, s, m)
    _only_column_changed(wd.get(), w, want_w[:, 0, m], 0, m, tol, "weights")
    check_scalar(norms.get(), want_n, tol, "norms")


@pytest.mark.parametrize("first_stride", [1, 5])
@pytest.mark.parametrize("B", BS0)
def test_eigen_proj_mean(B, first_stride):
    A, check, lib = _api()
    C, S, m = STRIDES[first_stride == 5]
    c, P = C, 16900
    rng = np.random.default_rng(B + first_stride)
    first = (rng.standard_normal((B, first_stride)) * P * 0.3).astype(
        np.float32)
    w = _weights_case(B, C, S)
    norm = np.float32(3.7)
    wd, fd, nd, pm = Dev(w.shape, init=w), dev(first), dev([norm]), Dev(B)
    check(lib.tike_eigen_proj_mean(dptr(fd) if B else None, first_stride,
                                   wd.ptr(c * S + m), (C + 1) * S, dptr(nd), P,
                                   B, pm.ptr(), A.stream_ptr()))
    np.testing.assert_array_equal(wd.get(), w)  # read only
    got = pm.get()
    if B:
        args = (first[:, 0], w[:, c, m], norm, P)
        check_scalar(got, lt.eigen_proj_mean(*args),
                     bar("eigen_proj_mean", lt.eigen_proj_mean, *args), "pm",
                     metric=lt.rel_max)


@pytest.mark.parametrize("B", BS0)
def test_eigen_dsum(B):
    """tike_eigen_dsum; B = 0: 0."""
    A, check, lib = _api()
    P = 16900
    s5 = sums5_case(B, P)
    out, sd = Dev(1), _stats_ptr(s5)
    check(lib.tike_eigen_dsum(dptr(sd), B, P, out.ptr(), A.stream_ptr()))
    check_scalar(out.get()[0], lt.eigen_dsum(s5, P),
                 bar("eigen_dsum", lt.eigen_dsum, s5, P), "dsum")


@pytest.mark.parametrize("coefs_given", [False, True])
@pytest.mark.parametrize("C,S,m", STRIDES)
@pytest.mark.parametrize("B", BS0)
def test_eigen_weights(B, C, S, m, coefs_given):
    """tike_eigen_weights on the last eigen probe's column; with coefs_c: the
    all-rank case (count above B, a dsum that is not the local one)."""
    A, check, lib = _api()
    c, P = C, 16900
    s5 = sums5_case(B, P)
    w = _weights_case(B, C, S, seed=3)
    count = float(B + 337) if coefs_given else float(max(B, 1))
    dsum = np.float32(lt.eigen_dsum(s5, P) * (2.3 if coefs_given else 1) + (
        B == 0))
    esum = np.float32(P * 1.01)
    rng = np.random.default_rng(B)
    coefs = rc(rng, B, C)
    wd = Dev(w.shape, init=w)
    cd = Dev(coefs.shape, cplx=True, init=coefs) if coefs_given else None
    sd, dd, ed = _stats_ptr(s5), dev([dsum]), dev([esum])
    check(lib.tike_eigen_weights(
        dptr(sd), B, P, dptr(dd), count, wd.ptr(c * S + m), (C + 1) * S,
        cd.ptr(c - 1) if cd else None, C, dptr(ed), A.stream_ptr()))
    args = (s5, P, dsum, count, w[:, c, m], esum if coefs_given else None)
    want_w, want_c = lt.eigen_weights(*args)
    tol = bar("eigen_weights", lt.eigen_weights, *args)
    _only_column_changed(wd.get(), w, want_w, c, m, tol, "weights")
    if coefs_given:
        got = cd.get()
        keep = np.ones(coefs.shape, bool)
        keep[:, c - 1] = False
        np.testing.assert_array_equal(got[keep], coefs[keep])
        if B:
            check_scalar(got[:, c - 1], want_c, tol, "coefs",
                         metric=lt.rel_max)


# ------------------------------------------------------ (b) pixel-sized entries
@functools.lru_cache(maxsize=None)
def eigen_case(npix):
    rng = np.random.default_rng(npix)
    E = rc(rng, npix) * 2
    update = rc(rng, npix) * 37 + 0.3 * E * 37  # correlated: eu is not ~ 0
    return E, update


@pytest.mark.parametrize("with_esum", [False, True])
@pytest.mark.parametrize("npix", [16, 256, 1000, 16384, 16900, 65536])
def test_eigen_normalise(npix, with_esum):
    """tike_eigen_normalise: the expanded quadratic of the kernels against the
    direct form, below, at and above the 64-workgroup cap."""
    A, check, lib = _api()
    E, update = eigen_case(npix)
    count, beta = 37.0, 0.1
    Ed, ud = Dev(npix, cplx=True, init=E), dev(update)
    esum, work = Dev(1), Dev(4)
    check(lib.tike_eigen_normalise(Ed.ptr(), dptr(ud), count, beta, npix,
                                   esum.ptr() if with_esum else None,
                                   work.ptr(), A.stream_ptr()))
    want, want_esum = lt.eigen_normalise(E, update, count, beta)
    assert_close(Ed.get(), want, OP_NORMWISE, OP_MAXABS, "E")
    work.get()
    got = esum.get()
    if with_esum:
        check_sums(got, [want_esum], "esum")
    else:
        assert np.isnan(got).all()


@functools.lru_cache(maxsize=None)
def probe_case(n):
    rng = np.random.default_rng(n % 1000)
    return rc(rng, n), rc(rng, n), rc(rng, n)


@pytest.mark.parametrize("with_combined", [False, True])
@pytest.mark.parametrize("n", [1, 300, ABOVE_GRID_CAP])
def test_probe_update(n, with_combined):
    """tike_probe_update, the last size on the grid-stride path."""
    A, check, lib = _api()
    probe, combined, mpu = probe_case(n)
    beta, inb = np.float32(0.731), 0.25
    pd = Dev(n, cplx=True, init=probe)
    cd = Dev(n, cplx=True, init=combined) if with_combined else None
    md, bd = dev(mpu), dev([beta])
    check(lib.tike_probe_update(pd.ptr(), cd.ptr() if cd else None, dptr(md),
                                dptr(bd), inb, n, A.stream_ptr()))
    want_p, want_c = lt.probe_update(probe, combined, mpu, beta, inb)
    assert_close(pd.get(), want_p, OP_NORMWISE, OP_MAXABS, "probe")
    if cd:
        assert_close(cd.get(), want_c, OP_NORMWISE, OP_MAXABS, "combined")


@functools.lru_cache(maxsize=None)
def object_case(n):
    rng = np.random.default_rng(n % 1000 + 1)
    acc = (rng.standard_normal((2, n))).astype(np.float32)
    precond = ((rng.random(n) + 0.05) + 1j * rng.standard_normal(n)).astype(
        np.complex64)
    combined = rng.standard_normal((2, n)).astype(np.float32)
    pmax = np.float32(precond.real.max())
    return acc, precond, combined, pmax, lt.object_update_precond(
        acc, precond, pmax, 0.05)


@pytest.mark.parametrize("outputs", range(8))
@pytest.mark.parametrize("n", [1, 300, ABOVE_GRID_CAP])
def test_object_update_precond(n, outputs):
    """tike_object_update_precond with every subset of { upd_sum, upd_precond,
    combined }."""
    A, check, lib = _api()
    acc, precond, combined, pmax, (want_sum, want_pre) = object_case(n)
    us = Dev(n, cplx=True) if outputs & 1 else None
    up = Dev(n, cplx=True) if outputs & 2 else None
    cb = Dev((2, n), init=combined) if outputs & 4 else None
    ad, prd, pmd = dev(acc), dev(precond), dev([pmax])
    check(lib.tike_object_update_precond(
        dptr(ad), dptr(prd), dptr(pmd), 0.05, us.ptr() if us else None,
        up.ptr() if up else None, cb.ptr() if cb else None, n, A.stream_ptr()))
    if us:
        assert_close(us.get(), want_sum, OP_NORMWISE, OP_MAXABS, "upd_sum")
    if up:
        assert_close(up.get(), want_pre, OP_NORMWISE, OP_MAXABS, "upd_precond")
    if cb:
        assert_close(cb.get(), combined.astype(np.float64) + acc, OP_NORMWISE,
                     OP_MAXABS, "combined")


# ---------------------------------------------------- (c) the packed entries
def _mid_cases():
    out, i = [], 0
    for B in BS0:
        for npix in (None, 256, 16384, 16900):
            out.append((B, npix, RECOVER[i % 3], i % 2 == 1))
            i += 1
    return out


@pytest.mark.parametrize("B,npix,recover,allrank", _mid_cases())
def test_tail_mid(B, npix, recover, allrank):
    """tike_lstsq_tail_mid: tail3[0..1] (tail3[2], the dsum accumulator, is
    not its to write), and with eigen0: nacc and the normalised E."""
    A, check, lib = _api()
    s, _, sums3, count = solve_case(B, allrank)
    beta = 0.1
    E = update = Ed = ud = nacc = None
    if npix:
        E, update = eigen_case(npix)
        Ed, ud = Dev(npix, cplx=True, init=E), dev(update)
        nacc = Dev(3, init=0.0)
    tail3 = Dev(3, init=[np.nan, np.nan, 0.25])
    sd, s3d = _stats_ptr(s), dev(sums3)
    check(lib.tike_lstsq_tail_mid(
        Ed.ptr() if npix else None, dptr(ud), npix or 0,
        nacc.ptr() if npix else None, beta, dptr(sd), B, EPS, dptr(s3d), count,
        int(recover[0]), int(recover[1]), tail3.ptr(), A.stream_ptr()))
    args = (None, None, beta, s, EPS, sums3, count) + recover
    want = lt.tail_mid(E, update, *args[2:])
    got = tail3.get()
    assert got[2] == 0.25
    check_scalar(got[:2], want["tail"],
                 bar("tail_mid", lt.tail_mid, *args, metric=lt.rel_each),
                 "tail3")
    if npix:
        check_sums(nacc.get(), want["nacc"], "nacc")
        assert_close(Ed.get(), want["E"], OP_NORMWISE, OP_MAXABS, "E")


@pytest.mark.parametrize("B,npix,recover", [
    (B, npix, RECOVER[(i + j) % 3]) for i, B in enumerate(BS0)
    for j, npix in enumerate((256, 16384, 16900))])
def test_tail_solve1(B, npix, recover):
    """tike_lstsq_tail_solve1: E' from nacc, sums3, and all of tail3."""
    A, check, lib = _api()
    s, costs, _, count = solve_case(B)
    s5 = sums5_case(B, npix)
    E, update = eigen_case(npix)
    beta = 0.1
    nacc = lt.norm_sums(E, update).astype(np.float32)
    Ed, ud, nd = Dev(npix, cplx=True, init=E), dev(update), dev(nacc)
    sums3, tail3 = Dev(3), Dev(3)
    sd, cd, s5d = _stats_ptr(s), dev(costs) if B else None, _stats_ptr(s5)
    check(lib.tike_lstsq_tail_solve1(
        Ed.ptr(), dptr(ud), npix, dptr(nd), beta, dptr(sd), dptr(cd),
        dptr(s5d), B, EPS, count, int(recover[0]), int(recover[1]),
        sums3.ptr(), tail3.ptr(), A.stream_ptr()))
    args = (E, update, beta, s, costs, s5, EPS, count) + recover
    want = lt.tail_solve1(*args)
    tol = bar("tail_solve1", lt.tail_solve1, *args, metric=lt.rel_each,
              pick=lambda o: (o["sums3"], o["tail3"]))
    check_scalar(sums3.get(), want["sums3"], tol, "sums3")
    check_scalar(tail3.get(), want["tail3"], tol, "tail3")
    assert_close(Ed.get(), want["E"], OP_NORMWISE, OP_MAXABS, "E")


@pytest.mark.parametrize("B,nprobe,probe,combined,weights,sums5,stride", [
    (63, 300, True, True, True, True, 0),              # nprobe > B
    (1000, 300, True, True, True, True, 1),            # B > nprobe
    (257, ABOVE_GRID_CAP, True, True, True, True, 0),  # above the grid cap
    (257, 300, False, False, True, True, 1),
    (257, 300, True, False, False, False, 0),
    (257, 300, True, True, True, False, 1),
    (1000, 0, False, False, True, True, 0),
    (1000, 300, False, False, False, False, 0),        # `steps` alone
    (0, 300, True, True, True, True, 1),               # an empty share
    (0, 0, False, False, True, True, 0),
])
def test_tail_finish(B, nprobe, probe, combined, weights, sums5, stride):
    """tike_lstsq_tail_finish: all five `steps`, the probe update, both weight
    columns (read at [n][0][m] and [n][1][m] = n * row + S + m)."""
    A, check, lib = _api()
    C, S, m = STRIDES[stride]
    npix = 16900
    s, _, sums3, _ = solve_case(B, True)
    count = float(B + 337)
    tail3 = np.array([0.61 * count, 0.27 * count, 1.9 * count], np.float32)
    s5 = sums5_case(B, npix) if sums5 else None
    w = _weights_case(B, C, S, seed=9) if weights else None
    P0, C0, mpu = probe_case(max(nprobe, 1))
    P0, C0, mpu = P0[:nprobe], C0[:nprobe], mpu[:nprobe]
    steps = Dev(5)
    pd = Dev(nprobe, cplx=True, init=P0) if probe else None
    cd = Dev(nprobe, cplx=True, init=C0) if combined else None
    wd = Dev(w.shape, init=w) if weights else None
    md, t3d, s3d = dev(mpu), dev(tail3), dev(sums3)
    sd, s5d = _stats_ptr(s), None if s5 is None else _stats_ptr(s5)
    check(lib.tike_lstsq_tail_finish(
        dptr(t3d), dptr(s3d), count, steps.ptr(), pd.ptr() if pd else None,
        cd.ptr() if cd else None, dptr(md) if nprobe else None, 0.25, nprobe,
        wd.ptr() if wd else None, (C + 1) * S, S, m, dptr(sd), dptr(s5d), B,
        npix, A.stream_ptr()))
    args = (tail3, sums3, count, P0 if probe else None,
            C0 if combined else None, mpu, 0.25, w, m, s, s5, npix)
    want = lt.tail_finish(*args)
    tol = bar("tail_finish", lt.tail_finish, *args,
              pick=lambda o: (list(o["steps"]), o["weights"]))
    check_scalar(steps.get(), want["steps"], tol, "steps")
    if probe:
        assert_close(pd.get(), want["probe"], OP_NORMWISE, OP_MAXABS, "probe")
    if combined:
        assert_close(cd.get(), want["combined"], OP_NORMWISE, OP_MAXABS,
                     "combined")
    if weights:
        got = wd.get()
        keep = np.ones(w.shape, bool)
        keep[:, 0, m] = False
        keep[:, 1, m] = not sums5
        np.testing.assert_array_equal(got[keep], w[keep])
        if B:
            check_scalar(got[:, :2, m], want["weights"][:, :2, m], tol,
                         "weights", metric=lt.rel_max)


# ------------------------------------------------- (d) two ranks without RCCL
@functools.lru_cache(maxsize=None)
def share_problem():
    B, pw, S = 513, 16, 2
    rng = np.random.default_rng(513)
    O, chi0 = rc(rng, B, pw, pw) * 2, rc(rng, B, pw, pw)
    mpu, probe = rc(rng, S, pw, pw), rc(rng, S, pw, pw)
    E = rc(rng, pw, pw) * 2
    w = _weights_case(B, 1, S, seed=4)
    w[:, 1] *= 0.2
    s, costs, _, _ = solve_case(B)
    return B, pw, S, O, chi0, mpu, probe, E, w, s, costs


@pytest.mark.parametrize("shares", [(300, 213), (513, 0)])
def test_two_ranks_without_a_communicator(shares):
    """The all-rank contract of the packed tail: sums3, the eigen update,
    tail3 and count span the minibatch, stats and weights are local.  Each
    share runs tike_eigen_pixel_update1 (with sums3), tike_lstsq_tail_mid,
    tike_eigen_position_sums1 and tike_lstsq_tail_finish; the small buffers
    are added on the host where comm.Allreduce would add them.  Also with one
    share empty."""
    A, check, lib = _api()
    st = A.stream_ptr()
    B, pw, S, O, chi0, mpu, probe, E, w, s, costs = share_problem()
    P, row, count, num_batch = pw * pw, 2 * S, float(B), 4
    beta = min(0.1, 1.0 / num_batch)
    norm = np.float32(np.sum(np.square(w[:, 1, 0].astype(np.float64))))
    eproj = lt.eigen_proj(O, chi0, mpu[0], E).astype(np.float32)
    kw = dict(eps=EPS, count=count, num_batch=num_batch, recover_psi=True,
              recover_probe=True)
    args = (s, costs, O, chi0, mpu, E, w, norm, probe, np.zeros_like(probe))
    want = lt.packed_tail(*args, **kw)
    bounds = np.cumsum((0,) + shares)
    ranks = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        n = hi - lo
        r = dict(lo=lo, hi=hi, n=n, update=Dev((pw, pw), cplx=True, init=0),
                 sums3=Dev(3), E=Dev((pw, pw), cplx=True, init=E),
                 w=Dev((n, 2, S), init=w[lo:hi]),
                 keep=[dev(x[lo:hi]) if n else None
                       for x in (O, chi0, eproj, s, costs)],
                 mpu=dev(mpu), norm=dev([norm]))
        ranks.append(r)
        pO, pchi, pproj, pstats, pcosts = map(dptr, r["keep"])
        check(lib.tike_eigen_pixel_update1(
            pO, pchi, dptr(r["mpu"]), r["E"].ptr(), pproj, r["w"].ptr(S), row,
            dptr(r["norm"]), r["update"].ptr(), n, pw, 1, pstats, pcosts, EPS,
            r["sums3"].ptr(), None, None, 0, 0, st))
    # all-reduce { sums3 ; update }
    sums3 = sum(r["sums3"].get().astype(np.float64) for r in ranks)
    update = sum(r["update"].get().astype(np.complex128) for r in ranks)
    s3d, ud = dev(sums3.astype(np.float32)), dev(update.astype(np.complex64))
    for r in ranks:
        pO, pchi, _, pstats, _ = map(dptr, r["keep"])
        r["nacc"], r["tail3"] = Dev(3, init=0.0), Dev(3, init=0.0)
        r["sums5"] = Dev((r["n"], 5))
        check(lib.tike_lstsq_tail_mid(
            r["E"].ptr(), dptr(ud), P, r["nacc"].ptr(), beta, pstats, r["n"],
            EPS, dptr(s3d), count, 1, 1, r["tail3"].ptr(), st))
        check(lib.tike_eigen_position_sums1(
            pO, pchi, dptr(r["mpu"]), r["E"].ptr(), r["sums5"].ptr(),
            r["tail3"].ptr(2), r["n"], pw, 1, None, None, 0, 0, st))
    # all-reduce tail3
    tail3 = sum(r["tail3"].get().astype(np.float64) for r in ranks)
    t3d = dev(tail3.astype(np.float32))
    for r in ranks:
        _, _, _, pstats, _ = map(dptr, r["keep"])
        r["steps"] = Dev(5)
        r["probe"] = Dev(probe.shape, cplx=True, init=probe)
        r["combined"] = Dev(probe.shape, cplx=True, init=0)
        check(lib.tike_lstsq_tail_finish(
            dptr(t3d), dptr(s3d), count, r["steps"].ptr(), r["probe"].ptr(),
            r["combined"].ptr(), dptr(r["mpu"]), 1.0 / num_batch, probe.size,
            r["w"].ptr(), row, S, 0, pstats, r["sums5"].ptr(), r["n"], P, st))
    tol_steps = bar("two ranks (steps)", lt.packed_tail, *args, **kw,
                    metric=lt.rel_each, pick=lambda o: list(o["steps"]))
    tol_w = bar("two ranks (weights)", lt.packed_tail, *args, **kw,
                pick=lambda o: o["weights"])
    check_sums(sums3, want["sums3"], "sums3")
    assert_close(update, want["update"], OP_NORMWISE, OP_MAXABS, "update")
    check_sums(tail3, want["tail3"], "tail3")
    for r in ranks:
        check_scalar(r["steps"].get(), want["steps"], tol_steps, "steps")
        assert_close(r["E"].get(), want["E"], OP_NORMWISE, OP_MAXABS, "E")
        assert_close(r["probe"].get(), want["probe"], OP_NORMWISE, OP_MAXABS,
                     "probe")
        assert_close(r["combined"].get(), want["combined"], OP_NORMWISE,
                     OP_MAXABS, "combined")
    got_w = np.concatenate([r["w"].get() for r in ranks])
    check_scalar(got_w, want["weights"], tol_w, "weights", metric=lt.rel_max)


# ------------------------------------- (e) the per-position kernels, directly
SLAB = 114  # positions per slab of the reference (bounds its memory)


def _pair_problem(pw, N, S, chi_modes, border):
    """Inputs of the three per-position entries and the model's results,
    formed in slabs of positions."""
    from oracle import operators as oracle
    rng = np.random.default_rng(pw + 7 * N + chi_modes)
    HW = pw + 40
    scan = (rng.random((N, 2)) * 30 + 2.25).astype(np.float32)
    if border:  # the window leaves the image: the pair falls back
        scan[1] = (HW - pw + 2.5, 3.5)
        scan[N - 2] = (-1.75, HW - pw + 1.25)
    psi, gobj = rc(rng, HW, HW), rc(rng, HW, HW)
    probe, mpu = rc(rng, S, pw, pw), rc(rng, S, pw, pw)
    chi = rc(rng, N, chi_modes, pw, pw)
    E = rc(rng, pw, pw) * 2
    w = (rng.standard_normal((N, 2, S)) * 0.3 + 1).astype(np.float32)
    update0 = rc(rng, pw, pw)
    costs = (rng.random(N) + 0.1).astype(np.float32)
    norm = np.float32(np.sum(np.square(w[:, 1, 0].astype(np.float64))))
    count, beta = float(N), 0.1
    O = np.empty((N, pw, pw), np.complex64)
    eproj, q = np.empty(N), np.empty(N)
    update = update0.astype(np.complex128)
    slabs = [(lo, min(N, lo + SLAB)) for lo in range(0, N, SLAB)]
    for lo, hi in slabs:
        O[lo:hi] = oracle.patch_fwd(psi, scan[lo:hi], patch_width=pw)
        x = chi[lo:hi, 0]
        eproj[lo:hi] = lt.eigen_proj(O[lo:hi], x, mpu[0], E)
        q[lo:hi] = lt.q_of(O[lo:hi], x, E)
        update = lt.pixel_update1(update, O[lo:hi], x, mpu[0],
                                  eproj[lo:hi].astype(np.float32),
                                  w[lo:hi, 1, 0], norm)
    upd_in = update.astype(np.complex64)  # the all-ranks update, as stored
    E1 = lt.eigen_normalise(E, upd_in, count, beta)[0]
    stats, sums5 = np.empty((N, 8)), np.empty((N, 5))
    for lo, hi in slabs:
        G = oracle.patch_fwd(gobj, scan[lo:hi], patch_width=pw)
        x = chi[lo:hi, 0]
        Pn = (w[lo:hi, 0, 0, None, None] * probe[0].astype(np.complex128) +
              w[lo:hi, 1, 0, None, None] * E.astype(np.complex128))
        stats[lo:hi] = lt.step_stats(G, O[lo:hi], x, probe[0], Pn, mpu[0])
        sums5[lo:hi] = lt.position_sums5(O[lo:hi], x, mpu[0], E1)
    return dict(HW=HW, scan=scan, psi=psi, gobj=gobj, probe=probe, mpu=mpu,
                chi=chi, E=E, w=w, update0=update0, costs=costs, norm=norm,
                count=count, beta=beta, O=O, eproj=eproj, q=q, update=update,
                upd_in=upd_in, nacc=lt.norm_sums(E, upd_in), stats=stats,
                sums5=sums5)


def _pair_cases():
    """(window, positions, chi_modes, psi given).  The split of a position's
    pixels in tike_lstsq_step_stats_eigen1 (its `nsplit` loop: doubled while
    < 16, pairs * nsplit * 2 <= 8192 and 2048 * nsplit divides the window's
    pixels): windows 16 and 32 (256 and 1024 pixels): 1, with 16 and 8 row
    groups; 64 (4096): 4; 128 and 256: 16; 128 with 1026 positions (513
    pairs): 8, since 513 * 16 * 2 > 8192.  (Deterministic mode: always 1.)
    Positions: odd and even, one chunk of the pixel update (<= 8) and two
    (9, 10), chunks of 10 positions (300)."""
    out, k = [], 0
    for pw in (16, 32, 64, 128, 256):
        for N in (1, 2, 9, 10) + ((300,) if pw <= 32 else ()):
            out.append((pw, N, 1 if k % 2 == 0 else 2, (k // 2) % 2 == 0))
            k += 1
        k += 1  # another pairing of chi_modes and psi at the next window
    out.append((128, 1026, 1, True))
    return out


@pytest.mark.parametrize("pw,N,chi_modes,with_psi", _pair_cases())
def test_per_position_tail_kernels(pw, N, chi_modes, with_psi):
    """tike_eigen_pixel_update1 (with sums3), tike_eigen_pixel_update1q (with
    eproj_out) and tike_lstsq_step_stats_eigen1 (nacc, stats, and sums5
    against E'; eigen0 not written) against the model, with positions whose
    window leaves the image from 9 positions on."""
    A, check, lib = _api()
    st = A.stream_ptr()
    S = 2
    p = _pair_problem(pw, N, S, chi_modes, border=N >= 9)
    HW = p["HW"]
    d = {k: dev(p[k]) for k in ("scan", "psi", "gobj", "probe", "mpu", "chi",
                                "w", "costs", "O", "upd_in")}
    Ed = Dev((pw, pw), cplx=True, init=p["E"])
    normd = dev([p["norm"]])
    psi_ptr = dptr(d["psi"]) if with_psi else None
    wc = d["w"].data_ptr() + 4 * S  # weights[0][1][0], rows 2 S floats apart
    stats_in = p["stats"].astype(np.float32)
    # --- tike_eigen_pixel_update1, sums3 from one more workgroup
    upd, sums3 = Dev((pw, pw), cplx=True, init=p["update0"]), Dev(3)
    eprojd, statsd = dev(p["eproj"].astype(np.float32)), dev(stats_in)
    check(lib.tike_eigen_pixel_update1(
        dptr(d["O"]), dptr(d["chi"]), dptr(d["mpu"]), Ed.ptr(), dptr(eprojd),
        wc, 2 * S, dptr(normd), upd.ptr(), N, pw, chi_modes, dptr(statsd),
        dptr(d["costs"]), EPS, sums3.ptr(), psi_ptr, dptr(d["scan"]), HW, HW,
        st))
    assert_close(upd.get(), p["update"], OP_NORMWISE, OP_MAXABS, "update")
    check_scalar(sums3.get(), lt.step_sums(stats_in, p["costs"], EPS),
                 bar("pixel_update1 sums3", lt.step_sums, stats_in, p["costs"],
                     EPS, metric=lt.rel_each), "sums3")
    # --- tike_eigen_pixel_update1q: the projection formed from q
    upd, eout, c0 = Dev((pw, pw), cplx=True, init=p["update0"]), Dev(N), Dev(64)
    q32 = p["q"].astype(np.float32)
    qd = dev(q32)
    check(lib.tike_eigen_pixel_update1q(
        dptr(d["O"]), dptr(d["chi"]), dptr(d["mpu"]), Ed.ptr(), dptr(qd), wc,
        2 * S, dptr(normd), upd.ptr(), N, pw, chi_modes, psi_ptr,
        dptr(d["scan"]), HW, HW, c0.ptr(), eout.ptr(), st))
    c0.get()
    check_sums(eout.get(), lt.eigen_proj_from_q(q32, p["mpu"][0], p["E"]),
               "eigen_proj from q")
    assert_close(upd.get(), p["update"], OP_NORMWISE, OP_MAXABS,
                 "update (from q)")
    # --- tike_lstsq_step_stats_eigen1
    nacc, stats, sums5 = Dev(3, init=0.0), Dev((N, 8)), Dev((N, 5))
    check(lib.tike_lstsq_step_stats_eigen1(
        dptr(d["chi"]), dptr(d["scan"]), dptr(d["gobj"]), dptr(d["probe"]),
        Ed.ptr(), dptr(d["w"]), 1, dptr(d["mpu"]), dptr(d["O"]),
        dptr(d["upd_in"]), nacc.ptr(), p["count"], p["beta"], stats.ptr(),
        sums5.ptr(), N, S, chi_modes, pw, HW, HW, st))
    check_sums(nacc.get(), p["nacc"], "nacc")
    check_sums(stats.get(), p["stats"], "stats")
    check_sums(sums5.get(), p["sums5"], "sums5 against E'")
    np.testing.assert_array_equal(Ed.get().view(np.float32),
                                  p["E"].view(np.float32),
                                  err_msg="eigen0 was written")


def test_step_stats_eigen1_refuses_windows_without_a_row_walk():
    """A window of 48 neither divides 256 nor is a multiple of it:
    TIKE_ERR_UNSUPPORTED, and nothing is written."""
    A, check, lib = _api()
    from tike_amd._lib import ERR_UNSUPPORTED
    pw, N, S, HW = 48, 2, 2, 88
    rng = np.random.default_rng(48)
    d = {k: dev(v) for k, v in dict(
        chi=rc(rng, N, 1, pw, pw), gobj=rc(rng, HW, HW), O=rc(rng, N, pw, pw),
        probe=rc(rng, S, pw, pw), mpu=rc(rng, S, pw, pw), E=rc(rng, pw, pw),
        upd=rc(rng, pw, pw), w=np.ones((N, 2, S), np.float32),
        scan=np.full((N, 2), 3.5, np.float32)).items()}
    nacc, stats, sums5 = Dev(3, init=0.0), Dev((N, 8)), Dev((N, 5))
    rcode = lib.tike_lstsq_step_stats_eigen1(
        dptr(d["chi"]), dptr(d["scan"]), dptr(d["gobj"]), dptr(d["probe"]),
        dptr(d["E"]), dptr(d["w"]), 1, dptr(d["mpu"]), dptr(d["O"]),
        dptr(d["upd"]), nacc.ptr(), float(N), 0.1, stats.ptr(), sums5.ptr(),
        N, S, 1, pw, HW, HW, A.stream_ptr())
    assert rcode == ERR_UNSUPPORTED
    assert np.all(nacc.get() == 0)
    assert np.isnan(stats.get()).all() and np.isnan(sums5.get()).all()


# ------------------------------------ (f) q of tike_ifft2_pass2_gradients_eproj
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("N", [3, 8])
@pytest.mark.parametrize("det", [128, 256])
def test_pass2_gradients_eproj_q(det, N, S):
    """q[n] = sum Re(conj(O_n) chi_n,0 conj(E_0)) from pass 2, against a
    complex128 NumPy ifft2 of the same far plane."""
    import torch
    A, check, lib = _api()
    st = A.stream_ptr()
    rng = np.random.default_rng(det + N + S)
    far = rc(rng, N, S, det, det)
    O = rc(rng, N, det, det) * 2
    probe, eigen = rc(rng, S, det, det), rc(rng, 1, 1, det, det) * 2
    w = (rng.standard_normal((N, 2, S)) * 0.3 + 1).astype(np.float32)
    chi0 = np.fft.ifft2(far[:, 0].astype(np.complex128), norm="ortho")
    want = lt.q_of(O, chi0, eigen[0, 0])
    d = {k: dev(v) for k, v in dict(far=far, O=O, probe=probe, eigen=eigen,
                                    w=w).items()}
    ones = torch.ones((N, det, det), dtype=torch.float32, device="cuda")
    work = torch.empty_like(d["far"])
    check(lib.tike_ifft2_pass1_scaled(A.ptr(d["far"]), A.ptr(ones), None, None,
                                      S, A.ptr(work), N * S, det, st))
    objproj, chi0d = Dev((N, det, det), cplx=True), Dev((N, det, det),
                                                        cplx=True)
    mpu = Dev((S, det, det), cplx=True, init=0)
    qtab, q = Dev(N * det // 4), Dev(N)
    check(lib.tike_ifft2_pass2_gradients_eproj(
        A.ptr(work), dptr(d["O"]), dptr(d["probe"]), dptr(d["eigen"]),
        dptr(d["w"]), 1, 1, objproj.ptr(), chi0d.ptr(), mpu.ptr(), 1.0, N, S,
        det, 1.0 / det, qtab.ptr(), q.ptr(), st))
    qtab.get()
    check_sums(q.get(), want, "q")
    assert_close(chi0d.get(), chi0, OP_NORMWISE, OP_MAXABS, "chi0")


# ------------------------------------------------------ (g) deterministic mode
def test_this_module_under_the_deterministic_switch():
    """Every case above once more in a process with TIKE_DETERMINISTIC=1
    (fixed-order sums, one workgroup per position pair), same bars."""
    from tike_amd import _lib
    if _lib.DETERMINISTIC:
        return  # this is the child
    env = dict(os.environ, TIKE_DETERMINISTIC="1")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q",
         "-m", "gpu", "-p", "no:cacheprovider"],
        capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout

