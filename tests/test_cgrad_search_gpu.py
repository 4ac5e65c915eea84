"""The conjugate-gradient search entries (tike_cgrad_line_search{,_masked},
tike_cgrad_line_search_linear{,_masked}), called through tike_amd._lib with raw
pointers, against the float64 model of tests/cgrad_search.py on the cases of
its table (tests/test_cgrad_search_cpu.py pins the model and shows that the
model alone decides every case).

Bounds.  A cost row, per pattern: |got - want| <= 1e-5 |want| + 2e-10 |row 0
of that pattern| -- the bound test_linear_masked_entry_row_sums_vs_numpy holds
the row sums to; the same on the row sums, on fx (a mean) and on the trial
entries' per-pattern costs.  xs: 2^-23 (|x| + |a d|) per component (one
multiply-add).  step, done, trials, failures: exactly equal.  The worst ratio
of error to bound of every (detector, model, variable) is collected in WORST
as the cases run (profiles/cgrad_search_entries.md).

Five poisson (case, row) pairs, where a pattern's total crosses zero and only
the 2e-10 floor is left of the bound, miss it by float32 rounding of the
forward pass: 1.5 (128^2), 25 (256^2) and 5.5 (512^2) row bounds in the row
next to the accepted one of the masked probe cases, 11..28 and 1.8..4.5 in
row 0 of the unmasked three-mode object cases at 256^2 and 512^2.  A float32
NumPy restatement of the entry misses it there too (2.0, 30, 5.8, 64, 1.6), and
cs.widened -- which never looks at a kernel -- sets such a row's bound to 4 x
the restatement's error; test_cgrad_search_cpu.py pins that rule."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cgrad_search as cs

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cs.CASES]
GUARD = 64
PATTERN = np.arange(GUARD, dtype=np.float32) * 0.25 - 321.0
WORST = {}  # (what, det, model, variable) -> worst error / bound


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: the worst error / bound of every group it saw."""
    yield
    for key in sorted(WORST):
        print("WORST", *key, "{:.4f}".format(WORST[key]))


def _api():
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    return A, check, lib


def _scale(det):
    from tike_amd.operators.propagation import fft_scales
    return fft_scales(det, "ortho")[0]


def _note(what, c, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = float(np.max(r))
    key = (what, c.det, cs.MODELS[c.model], "probe" if c.variable else "object")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("RATIO {} {} {:.4f}".format(what, c.name, worst))
    return worst


class Guarded:
    """A float32 / complex64 device buffer with GUARD floats of PATTERN behind
    its logical end, which must come back untouched."""

    def __init__(self, host):
        A, _, _ = _api()
        host = np.ascontiguousarray(host)
        self.dtype, self.shape = host.dtype, host.shape
        flat = host.view(np.float32).ravel()
        self.n = flat.size
        self.t = A.to_device(np.concatenate([flat, PATTERN]))

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        host = self.t.cpu().numpy()
        np.testing.assert_array_equal(host[self.n:], PATTERN,
                                      err_msg="written past the end")
        return host[:self.n].copy().view(self.dtype).reshape(self.shape)


def _device_inputs(P):
    A, _, _ = _api()
    c = P["case"]
    data = P["data"].view(np.int16) if c.u16 else P["data"]
    t = dict(x=A.to_device(P["x"]), d=A.to_device(P["d"]),
             other=A.to_device(P["other"]), scan=A.to_device(P["scan"]),
             data=A.to_device(data),
             mask=None if P["mask"] is None else A.to_device(
                 P["mask"].astype(np.uint8)))
    assert t["data"].element_size() == (2 if c.u16 else 4)
    return t


class Linear:
    """One case's buffers for the all-at-once entries.  costs_k and xs start
    from garbage the entry must overwrite."""

    def __init__(self, name, chunk=None):
        A, _, _ = _api()
        self.P = P = cs.inputs(name)
        self.c = c = P["case"]
        self.chunk = c.N if chunk is None else chunk
        self.t = _device_inputs(P)
        m = min(self.chunk, c.N)
        far = np.full((m, c.S, c.det, c.det), np.nan, np.complex64)
        self.far_a, self.far_b = A.to_device(far), A.to_device(far)
        self.costs_k = Guarded(np.full(cs.ROWS * c.N + 1, 7.0, np.float32))
        self.xs = Guarded(np.full(P["x"].shape, np.nan, np.complex64))
        self.state = A.to_device(np.array([123.0, P["step0"], 0.0, 0.0, 0.0]))
        self.sums = A.to_device(np.full(cs.ROWS, 5.0))

    def call(self, stage=0, a_valid=0, plain=False, model=None, count=None,
             u16=None):
        A, check, lib = _api()
        P, c, t = self.P, self.c, self.t
        H, W = (P["other"] if c.variable else P["x"]).shape[-2:]
        args = (c.variable, A.ptr(t["x"]), A.ptr(t["d"]), self.xs.ptr(),
                A.ptr(t["other"]), A.ptr(t["scan"]), A.ptr(t["data"]),
                int(c.u16) if u16 is None else u16, A.ptr(self.far_a), a_valid,
                A.ptr(self.far_b), self.costs_k.ptr(), c.N, self.chunk, c.S,
                c.det, H, W, _scale(c.det),
                float(c.N) if count is None else count, A.ptr(self.state),
                stage, A.ptr(self.sums))
        if plain:
            assert c.model == 0 and t["mask"] is None
            return lib.tike_cgrad_line_search_linear(*args, A.stream_ptr())
        return lib.tike_cgrad_line_search_linear_masked(
            *args, None if t["mask"] is None else A.ptr(t["mask"]),
            c.model if model is None else model, P["num_measured"],
            A.stream_ptr())

    def fill_far_a(self):
        """What the gradient pass at x leaves in its scratch: the hand-off of
        tike_fwd_pass1, or at 128^2 the far plane of tike_ptycho_fwd."""
        A, check, lib = _api()
        P, c, t = self.P, self.c, self.t
        psi, probe = (t["other"], t["x"]) if c.variable else (t["x"],
                                                              t["other"])
        H, W = psi.shape[-2:]
        if c.det == 128:
            check(lib.tike_ptycho_fwd(
                A.ptr(psi), A.ptr(t["scan"]), A.ptr(probe), 0, None, None, 0,
                0, A.ptr(self.far_a), c.N, c.S, c.det, c.det, H, W,
                _scale(c.det), 0, A.stream_ptr()), "forward")
        else:
            check(lib.tike_fwd_pass1(
                A.ptr(psi), A.ptr(t["scan"]), A.ptr(probe), 0, None, None,
                None, 0, 0, A.ptr(self.far_a), None, c.N, c.S, c.det, c.det, H,
                W, A.stream_ptr()), "forward pass 1")

    def rows(self):
        k = self.costs_k.get()
        return k[:-1].reshape(cs.ROWS, self.c.N).astype(np.float64), k[-1:]

    def result(self):
        rows, word = self.rows()
        return dict(rows=rows, accepted_word=word.view(np.int32)[0],
                    state=self.state.cpu().numpy().copy(), xs=self.xs.get(),
                    sums=self.sums.cpu().numpy().copy())


def _check_rows(c, got, R, passes=(0, 1), what="rows"):
    """Every entry of the cost rows of `passes` against the model, pattern by
    pattern; rows 9..16 are exactly zero when the first pass accepted."""
    want = np.array(R["rows"])
    first_accepts = R["accepted"] is not None and R["accepted"] < cs.STEPS
    if first_accepts:
        want[1 + cs.STEPS:] = 0.0
    sel = np.zeros(cs.ROWS, bool)
    if 0 in passes:
        sel[:1 + cs.STEPS] = True
    if 1 in passes:
        sel[1 + cs.STEPS:] = True
    bound = R["bound"]
    err = np.abs(got - want)
    worst = _note(what, c, err[sel], bound[sel])
    wide = sel & (R["float32_ratio"].max(axis=1) > 1.0)
    for row in np.flatnonzero(wide):  # (both numbers, against the row bound)
        print("WIDENED {} {} row {}: kernel {:.3f} float32 NumPy {:.3f}".format(
            what, c.name, row, (err[row] / cs.row_bound(want, want[0])[row]
                                ).max(), R["float32_ratio"][row].max()))
    if first_accepts and 1 in passes:
        np.testing.assert_array_equal(got[1 + cs.STEPS:], 0.0)
    assert worst <= 1.0, (worst, np.argwhere(err > bound))


def _check_state(c, state, R, what="fx"):
    want = R["state"]
    np.testing.assert_array_equal(state[1:], want[1:])
    err = abs(state[0] - want[0])
    assert _note(what, c, np.array([err]), np.array(
        [cs.row_bound(want[0], R["means"][0])])) <= 1.0, (state, want)


def _check_xs(P, xs, a):
    """xs against x + a d (a = 0: bit-equal to x)."""
    if a == 0.0:
        np.testing.assert_array_equal(xs, P["x"])
        return
    want = P["x"].astype(np.complex128) + a * P["d"].astype(np.complex128)
    b = cs.xs_bound(P["x"], P["d"], a)
    e = xs.astype(np.complex128) - want
    assert np.all(np.abs(e.real) <= b.real) and np.all(
        np.abs(e.imag) <= b.imag), (np.abs(e).max(), a)


def _check_linear(L, R, what=""):
    c = L.c
    got = L.result()
    _check_rows(c, got["rows"], R, what="rows" + what)
    _check_state(c, got["state"], R, what="fx" + what)
    assert got["accepted_word"] == (R["accepted"] is not None)
    _check_xs(L.P, got["xs"], R["state"][1] if R["state"][2] else 0.0)
    return got


# ------------------------------------------------ the all-at-once entry, stage 0
@pytest.mark.parametrize("name", NAMES)
def test_linear_search_vs_model(name):
    """tike_cgrad_line_search_linear_masked, stage 0: all 17 x N cost entries,
    the five state words and xs (unmasked gaussian cases: the entry without
    mask arguments too)."""
    from tike_amd import _lib
    _, check, _ = _api()
    L = Linear(name)
    R = cs.reference(name)
    check(L.call(), name)
    got = _check_linear(L, R)
    if _lib.DETERMINISTIC:  # fixed-order sums: a second call, bit for bit
        L2 = Linear(name)
        check(L2.call(), name)
        again = L2.result()
        np.testing.assert_array_equal(again["rows"], got["rows"])
        np.testing.assert_array_equal(again["state"], got["state"])
    c = L.c
    if c.model == 0 and not c.masked:
        M = Linear(name)
        check(M.call(plain=True), name)
        _check_linear(M, R, what=" (plain entry)")


def test_linear_search_16_bit_counts_at_128_are_unsupported():
    from tike_amd._lib import ERR_UNSUPPORTED
    L = Linear("128x1n3-object-gaussian-mask-0")
    assert L.call(u16=1) == ERR_UNSUPPORTED
    T = Trials("128x1n3-object-gaussian-mask-0", 0, 1)
    assert T.call(u16=1) == ERR_UNSUPPORTED


# ----------------------------------------------------------------- chunks
def _ragged(N):
    """A chunk length below N that leaves a shorter last chunk."""
    chunk = 2 if N % 2 else 3
    assert chunk < N and N % chunk
    return chunk


@pytest.mark.parametrize("name", [c.name for c in cs.CASES
                                  if c.bucket in ("0", "8-15", "none")])
def test_linear_search_in_ragged_chunks(name):
    """chunk < N, a shorter last chunk: the hand-offs are formed chunk by chunk, and re-formed
    in the second pass behind the `accepted` word."""
    _, check, _ = _api()
    L = Linear(name, chunk=_ragged(cs.BY_NAME[name].N))
    check(L.call(), name)
    _check_linear(L, cs.reference(name), what=" (chunks)")


# -------------------------------------------------------------- a_valid = 1
@pytest.mark.parametrize("name", [c.name for c in cs.CASES
                                  if c.bucket in ("0", "8-15")])
def test_linear_search_reads_the_gradient_pass_hand_off(name):
    _, check, _ = _api()
    L = Linear(name)
    L.fill_far_a()
    check(L.call(a_valid=1), name)
    _check_linear(L, cs.reference(name), what=" (a_valid)")


# ------------------------------------------------------- stages 1, 2, 3, 4
def _check_sums(c, got, R, sel, what):
    want = R["rows"].sum(axis=1)
    bound = R["sum_bound"]
    err = np.abs(got - want)
    assert _note(what, c, err[sel], bound[sel]) <= 1.0, (got, want)


@pytest.mark.parametrize("name", NAMES)
def test_linear_search_staged(name):
    """Stage 1 leaves the row sums 0..8 (9..16 untouched), stage 3 the row
    sums 9..16 (zeros after an accept); stages 2 and 4 decide from them: the
    same state and xs as stage 0."""
    _, check, _ = _api()
    L, R = Linear(name), cs.reference(name)
    c = L.c
    first_accepts = R["accepted"] is not None and R["accepted"] < cs.STEPS
    lo = np.arange(cs.ROWS) <= cs.STEPS
    check(L.call(stage=1), name)
    got = L.result()
    _check_sums(c, got["sums"], R, lo, "sums 1")
    np.testing.assert_array_equal(got["sums"][~lo], 5.0)
    _check_rows(c, got["rows"], R, passes=(0,), what="rows (stage 1)")
    np.testing.assert_array_equal(got["rows"][~lo], 0.0)
    np.testing.assert_array_equal(got["state"],
                                  [123.0, L.P["step0"], 0.0, 0.0, 0.0])
    check(L.call(stage=2), name)
    st = L.result()["state"]
    assert st[2] == float(first_accepts) and st[3] == (
        R["accepted"] + 1 if first_accepts else 8) and st[4] == 0
    check(L.call(stage=3), name)
    got = L.result()
    if first_accepts:
        np.testing.assert_array_equal(got["sums"][~lo], 0.0)
    else:
        _check_sums(c, got["sums"], R, ~lo, "sums 3")
    _check_sums(c, got["sums"], R, lo, "sums 1")  # still there
    np.testing.assert_array_equal(got["state"], st)
    check(L.call(stage=4), name)
    _check_linear(L, R, what=" (staged)")


# ------------------------------ stages 2 and 4 on sums written out by hand
@pytest.mark.parametrize("k", range(len(cs.DECIDE_TABLE)))
def test_decisions_from_given_sums(k):
    """The rule of ls_pick_sums_kernel on the table of tests/cgrad_search.py:
    count = 4, so the means are exact and `<=` is pinned on the device."""
    A, check, _ = _api()
    rows, fx, step0, first, rel, trials, fails, want = cs.DECIDE_TABLE[k]
    count = 4.0
    L = Linear("128x1n3-object-gaussian-mask-0")
    means = cs.table_means(fx if first else 123.0, rows if first else None,
                           None if first else rows)
    L.sums.copy_(A.to_device(means * count))
    L.state.copy_(A.to_device(np.array([77.0 if first else fx, step0, 0.0,
                                        trials, fails])))
    check(L.call(stage=2 if first else 4, model=rel, count=count), str(k))
    got = L.result()
    np.testing.assert_array_equal(got["state"], np.array(want))
    np.testing.assert_array_equal(got["rows"], 7.0)  # no cost pass was made
    if first:
        assert np.all(np.isnan(got["xs"]))  # xs is formed by stage 4 only
    else:
        _check_xs(L.P, got["xs"], want[1] if want[2] else 0.0)


def test_second_decision_after_an_accept_changes_nothing_but_xs():
    A, check, _ = _api()
    L = Linear("128x1n3-object-gaussian-mask-0")
    L.sums.copy_(A.to_device(np.zeros(cs.ROWS)))  # would accept at once
    state = np.array([3.0, 0.25, 1.0, 2.0, 1.0])
    L.state.copy_(A.to_device(state))
    check(L.call(stage=4), "stage 4")
    got = L.result()
    np.testing.assert_array_equal(got["state"], state)
    _check_xs(L.P, got["xs"], 0.25)


# --------------------------------------------------- the trial-by-trial entry
class Trials:

    def __init__(self, name, k0, nslots, chunk=None):
        A, _, _ = _api()
        self.P = P = cs.inputs(name)
        self.c = c = P["case"]
        self.nslots = nslots
        self.chunk = c.N if chunk is None else chunk
        self.t = _device_inputs(P)
        self.scratch = A.to_device(np.full(
            (min(self.chunk, c.N), c.S, c.det, c.det), np.nan, np.complex64))
        self.costs = Guarded(np.full(c.N, np.nan, np.float32))
        self.xs = Guarded(np.full(P["x"].shape, np.nan, np.complex64))
        self.skip = A.to_device(np.array([5], np.int32))
        self.st0, self.tried, self.means = cs.trial_reference(name, k0, nslots)
        # (done = 1 and the counters of earlier searches on entry)
        self.state = A.to_device(np.array(
            [self.means[0], cs.step_lengths(P["step0"])[k0], 1.0, 2.0, 1.0]))
        self.row = 1 + k0 + int(self.st0[3]) - 1  # the last trial made

    def call(self, plain=False, u16=None):
        A, _, lib = _api()
        P, c, t = self.P, self.c, self.t
        H, W = (P["other"] if c.variable else P["x"]).shape[-2:]
        args = (c.variable, A.ptr(t["x"]), A.ptr(t["d"]), self.xs.ptr(),
                A.ptr(t["other"]), A.ptr(t["scan"]), A.ptr(t["data"]),
                int(c.u16) if u16 is None else u16, A.ptr(self.scratch),
                self.costs.ptr(), c.N, self.chunk, c.S, c.det, H, W,
                _scale(c.det), float(c.N), A.ptr(self.state),
                A.ptr(self.skip), self.nslots)
        if plain:
            assert c.model == 0 and t["mask"] is None
            return lib.tike_cgrad_line_search(*args, A.stream_ptr())
        return lib.tike_cgrad_line_search_masked(
            *args, None if t["mask"] is None else A.ptr(t["mask"]), c.model,
            P["num_measured"], A.stream_ptr())

    def verify(self, what=""):
        c, R = self.c, cs.reference(self.c.name)
        state = self.state.cpu().numpy()
        want = self.st0 + np.array([0.0, 0.0, 0.0, 2.0, 1.0])
        np.testing.assert_array_equal(state[1:], want[1:])
        if want[2]:
            err = np.array([abs(state[0] - want[0])])
            assert _note("trial fx" + what, c, err, np.array(
                [cs.row_bound(want[0], self.means[0])])) <= 1.0, (state, want)
        else:
            assert state[0] == want[0]  # fx of the caller, untouched
        plain = R["plain"]
        err = np.abs(self.costs.get() - plain[self.row])
        assert _note("trial costs" + what, c, err,
                     R["plain_bound"][self.row]) <= 1.0, (self.costs.get(),
                                                          plain[self.row])
        if R["plain_float32_ratio"][self.row].max() > 1.0:
            print("WIDENED trial costs {} row {}: kernel {:.3f} float32 NumPy "
                  "{:.3f}".format(c.name, self.row, (err / cs.row_bound(
                      plain[self.row], plain[0])).max(),
                      R["plain_float32_ratio"][self.row].max()))
        _check_xs(self.P, self.xs.get(), float(np.float32(self.tried)))


@pytest.mark.parametrize("name,k0,nslots,what", cs.TRIALS)
def test_trial_search_vs_model(name, k0, nslots, what):
    """tike_cgrad_line_search_masked: state, the costs of the last trial made,
    and xs (several ragged chunks when nslots = 4; unmasked gaussian cases:
    the entry without mask arguments too)."""
    _, check, _ = _api()
    chunk = _ragged(cs.BY_NAME[name].N) if nslots == 4 else None
    T = Trials(name, k0, nslots, chunk)
    check(T.call(), name)
    T.verify()
    if T.c.model == 0 and not T.c.masked:
        T = Trials(name, k0, nslots, chunk)
        check(T.call(plain=True), name)
        T.verify(" (plain entry)")


# ------------------------------------------------------- deterministic mode
def test_linear_search_under_the_deterministic_switch():
    """One shape per detector size once more in a process with
    TIKE_DETERMINISTIC=1: same bounds, and two calls give bit-identical
    costs_k (test_linear_search_vs_model makes the second call there)."""
    here = os.path.abspath(__file__)
    env = dict(os.environ, TIKE_DETERMINISTIC="1")
    ids = ["{}::test_linear_search_vs_model[{}]".format(here, n)
           for n in ("128x3n4-object-poisson-all-1-7",
                     "256x1n5-object-poisson-mask-u16-8-15",
                     "512x3n5-probe-gaussian-all-8-15")]
    out = subprocess.run(
        [sys.executable, "-m", "pytest", *ids, "-x", "-q", "-m", "gpu", "-p",
         "no:cacheprovider"], capture_output=True, text=True, env=env,
        timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "3 passed" in out.stdout
