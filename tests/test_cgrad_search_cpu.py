"""tests/cgrad_search.py -- the float64 model the conjugate-gradient search
entries are held to on the GPU -- against independent arithmetic, and the
preconditions of every case of its table: the model alone decides each search
(every decision is at least 100 bounds away from the bar), and the table
reaches every branch of the two passes under each noise model."""
import numpy as np
import pytest

import cgrad_models as cm
import cgrad_search as cs

NAMES = [c.name for c in cs.CASES]


# ------------------------------------------- the model, independent arithmetic
@pytest.mark.parametrize("name", ["128x3n4-object-poisson-all-1-7",
                                  "128x3n5-probe-gaussian-all-8-15"])
def test_far_plane_is_linear_in_the_variable(name):
    """|A + s B|^2 is the intensity of a float64 forward pass of x + s d."""
    P = cs.inputs(name)
    c = P["case"]
    A, B = cs.far_planes(c.variable, P["x"], P["d"], P["other"], P["scan"],
                         c.det)
    assert A.dtype == np.complex128 and A.shape == (c.N, c.S, c.det, c.det)
    for s in (0.37, 2.0**c.log2step):
        moved = P["x"].astype(np.complex128) + s * P["d"].astype(np.complex128)
        psi, probe = (P["other"], moved) if c.variable else (moved, P["other"])
        want = np.sum(np.abs(cs.forward(psi, P["scan"], probe, c.det))**2,
                      axis=1)
        got = cs.intensity(A, B, s)
        assert np.abs(got - want).max() <= 1e-12 * want.max()
    # ... and of the float32 oracle's forward pass, to its own rounding
    f32 = cm.ops.ptycho_fwd(*((P["x"], P["scan"], P["other"]) if c.variable
                              else (P["other"], P["scan"], P["x"])), c.det)
    assert np.abs(f32[:, 0] - A).max() <= 2e-6 * np.abs(A).max()


@pytest.mark.parametrize("name", ["128x1n3-probe-poisson-mask-none",
                                  "128x3n4-object-poisson-all-1-7",
                                  "256x1n5-object-poisson-mask-u16-8-15"])
def test_poisson_rows_are_differences_of_plain_costs(name):
    R = cs.reference(name)
    rows, plain = R["rows"], R["plain"]
    np.testing.assert_array_equal(rows[0], plain[0])
    # (the plain float64 costs round at 2^-52 of themselves, the terms summed
    # at 2^-52 of the largest: 1e-12 of row 0 covers both)
    tol = 1e-12 * np.abs(plain).max()
    assert np.abs(rows[1:] - (plain[1:] - plain[0])).max() <= tol
    # unmeasured counts never enter
    assert np.all(np.isfinite(rows))


def test_gaussian_rows_are_the_plain_costs_of_cgrad_models():
    name = "128x1n3-object-gaussian-mask-0"
    P, R = cs.inputs(name), cs.reference(name)
    c = P["case"]
    s = cs.step_lengths(P["step0"])
    assert s[0] == 0.5 and s[15] == 0.5 / 2**15
    for k in (0, 5, 16):
        x = P["x"].astype(np.complex128) + (s[k - 1] if k else 0.0) * P["d"]
        far = cs.forward(x, P["scan"], P["other"], c.det)
        want = cm.cost_each("gaussian", P["model_data"],
                            np.sum(np.abs(far)**2, axis=1), P["mask"])
        np.testing.assert_allclose(R["rows"][k], want, rtol=1e-12)


_means = cs.table_means


@pytest.mark.parametrize("k", range(len(cs.DECIDE_TABLE)))
def test_decide_against_the_table(k):
    rows, fx, step0, first, rel, trials, fails, want = cs.DECIDE_TABLE[k]
    means = _means(fx if first else 123.0, rows if first else None,
                   None if first else rows)
    got = cs.decide(means, 77.0 if first else fx, step0, first, not first, rel,
                    trials, fails)
    np.testing.assert_array_equal(got, np.array(want))


def test_decide_counts_a_failure_on_the_last_pass_only():
    five = _means(4.0, [5.0] * 8, [5.0] * 8)
    for first in (True, False):
        for last in (True, False):
            st = cs.decide(five, 4.0, 1.0, first, last, 0, 3.0, 2.0)
            np.testing.assert_array_equal(
                st, [4.0, 2.0**-8, 0.0, 11.0, 3.0 if last else 2.0])


def test_search_linear_composes_two_passes():
    five = [5.0] * 8
    # first pass accepts: the second is not run (its rows would accept at once)
    m = _means(4.0, [5, 5, 4.0, 0, 0, 0, 0, 0], [0.0] * 8)
    np.testing.assert_array_equal(
        cs.search_linear(m, [99.0, 1.0, 0.0, 2.0, 1.0], 0),
        [4.0, 0.25, 1.0, 5.0, 1.0])
    # second pass accepts at its k = 2: step = 2^-10, trials 8 + 3
    m = _means(4.0, five, [5, 5, 3.0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(
        cs.search_linear(m, [99.0, 1.0, 0.0, 0.0, 0.0], 0),
        [3.0, 2.0**-10, 1.0, 11.0, 0.0])
    # neither: ONE failure, 16 trials, step / 2^16
    m = _means(4.0, five, five)
    st = cs.search_linear(m, [99.0, 1.0, 0.0, 0.0, 0.0], 0)
    np.testing.assert_array_equal(st, [4.0, 2.0**-16, 0.0, 16.0, 1.0])
    x, d = np.array([1 + 2j]), np.array([0.5 - 1j])
    np.testing.assert_array_equal(cs.apply_step(x, d, st), x)
    st[1:3] = 0.5, 1.0
    np.testing.assert_array_equal(cs.apply_step(x, d, st), [1.25 + 1.5j])


def test_search_trials_against_the_table():
    costs = {1.0: 9.0, 0.5: 4.0, 0.25: 3.0, 0.125: float("nan")}
    f = costs.__getitem__
    # accept at slot 1 (a tie)
    st, tried = cs.search_trials(f, 9.0, 1.0, 1)
    np.testing.assert_array_equal(st, [9.0, 1.0, 1.0, 1.0, 0.0])
    assert tried == 1.0
    # accept at slot 2, counters carried
    st, tried = cs.search_trials(f, 4.5, 1.0, 30, 3.0, 1.0)
    np.testing.assert_array_equal(st, [4.0, 0.5, 1.0, 5.0, 1.0])
    assert tried == 0.5
    # out of slots: done = 0, step / 2^nslots, one failure, xs = the last trial
    st, tried = cs.search_trials(f, 2.0, 1.0, 3)
    np.testing.assert_array_equal(st, [2.0, 0.125, 0.0, 3.0, 1.0])
    assert tried == 0.25
    # a NaN cost is never accepted
    st, tried = cs.search_trials(f, 2.0, 0.125, 1)
    np.testing.assert_array_equal(st, [2.0, 0.0625, 0.0, 1.0, 1.0])
    assert tried == 0.125


# ------------------------------------------------------- the table of cases
def test_table_covers_every_factor_at_every_size():
    for det in (128, 256, 512):
        cases = [c for c in cs.CASES if c.det == det]
        assert {c.S for c in cases} >= {1, 3}
        assert {c.N for c in cases} == {3, 4, 5}
        assert {(c.variable, c.model) for c in cases} == {
            (0, 0), (0, 1), (1, 0), (1, 1)}
        assert {(c.model, c.masked) for c in cases} == {
            (0, False), (0, True), (1, False), (1, True)}
        assert {c.u16 for c in cases} == ({False} if det == 128 else
                                          {False, True})
        # the chunked runs need a second-pass accept and a search that fails
        assert {c.bucket for c in cases} == {"0", "1-7", "8-15", "none"}
    assert any(c.det == 256 and c.S == 8 for c in cs.CASES)
    assert 25 <= len(cs.CASES) <= 35


def test_every_branch_is_hit_under_each_noise_model():
    for model in (0, 1):
        hit = {c.bucket for c in cs.CASES if c.model == model}
        assert hit == {"0", "1-7", "8-15", "none"}, (model, hit)


@pytest.mark.parametrize("name", NAMES)
def test_case_inputs_are_what_the_entries_require(name):
    P = cs.inputs(name)
    c = P["case"]
    HW = c.det + 24
    assert P["x"].dtype == P["d"].dtype == P["other"].dtype == np.complex64
    assert P["scan"].dtype == np.float32 and P["scan"].shape == (c.N, 2)
    obj, probe = (P["other"], P["x"]) if c.variable else (P["x"], P["other"])
    assert obj.shape == (1, HW, HW) and probe.shape == (1, 1, c.S, c.det,
                                                        c.det)
    assert P["d"].shape == P["x"].shape
    # the patch and its +1 taps stay inside the object; positions fractional
    assert P["scan"].min() >= 1 and np.floor(P["scan"]).max() + c.det + 1 < HW
    assert np.all(P["scan"] != np.floor(P["scan"]))
    assert P["data"].shape == (c.N, c.det, c.det)
    if c.u16:
        assert P["data"].dtype == np.uint16 and P["data"].max() > 1000
        np.testing.assert_array_equal(P["model_data"], P["data"])
    else:
        assert P["data"].dtype == np.float32
        if c.masked:
            assert np.all(np.isnan(P["data"][:, ~P["mask"]]))
            assert np.all(np.isfinite(P["data"][:, P["mask"]]))
        else:
            assert np.all(np.isfinite(P["data"]))
    assert (P["mask"] is not None) == c.masked
    assert 0 < P["num_measured"] <= c.det**2
    assert np.all(np.isfinite(P["d"])) and np.abs(P["d"]).max() > 0
    # the first step is a power of two: every halving is exact
    assert P["step0"] == 2.0**c.log2step and -4 < c.log2step < 14


@pytest.mark.parametrize("name", NAMES)
def test_case_is_decided_by_the_model_alone(name):
    """Every candidate up to the accepted one (all 16 when none is) is at
    least 100 row bounds away from the bar, and the accept falls where the
    table says."""
    R = cs.reference(name)
    c = cs.BY_NAME[name]
    assert np.all(np.isfinite(R["rows"]))
    assert cs.in_bucket(R["accepted"], c.bucket), R["accepted"]
    assert cs.clarity(R["means"], c.model) >= cs.CLEAR
    # ... and so it is at the bounds in force where a row's bound is widened
    bar = 0.0 if c.model else R["means"][0]
    last = 15 if R["accepted"] is None else R["accepted"]
    decided = slice(1, 2 + last)
    assert np.all(np.abs(R["means"][decided] - bar) >=
                  cs.CLEAR * R["bound"][decided].mean(axis=1))
    st = R["state"]
    if R["accepted"] is None:
        np.testing.assert_array_equal(
            st[1:], [2.0**(c.log2step - 16), 0.0, 16.0, 1.0])
    else:
        np.testing.assert_array_equal(
            st[1:], [2.0**(c.log2step - R["accepted"]), 1.0,
                     R["accepted"] + 1.0, 0.0])


@pytest.mark.parametrize("name,k0,nslots,what", cs.TRIALS)
def test_trial_case_is_decided_by_the_model_alone(name, k0, nslots, what):
    st, tried, means = cs.trial_reference(name, k0, nslots)
    made = int(st[3])
    assert k0 + made <= 16  # every trial made is one of the model's rows
    assert cs.clarity(np.delete(means, slice(1, 1 + k0)), 0,
                      upto=made - 1) >= cs.CLEAR
    assert {"first": st[2] == 1 and made == 1,
            "later": st[2] == 1 and 1 < made <= nslots,
            "out": st[2] == 0 and made == nslots and st[4] == 1}[what], st


def test_trial_table_covers_slots_models_variables_and_u16():
    cases = [(cs.BY_NAME[n], s, w) for n, _, s, w in cs.TRIALS]
    assert {s for _, s, _ in cases} == {1, 4, 30}
    assert {w for _, _, w in cases} == {"first", "later", "out"}
    assert {c.det for c, _, _ in cases} == {128, 256, 512}
    assert {(c.variable, c.model) for c, _, _ in cases} == {
        (0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c.u16 and c.det == 256 for c, _, _ in cases)


@pytest.mark.parametrize("name", NAMES)
def test_bounds_are_widened_by_the_float32_restatement_only(name):
    """A row keeps the row bound unless the float32 NumPy restatement of the
    entries' formulas itself misses it there; then the row's bound is 4 x that
    restatement's error.  Gaussian rows never need it; poisson rows do where a
    pattern's total crosses zero (row 0 of the unmasked three-mode cases, the
    row next to the accepted one of the probe cases), and never beyond the
    row bound of the largest pattern's plain cost."""
    R = cs.reference(name)
    c = cs.BY_NAME[name]
    base = cs.row_bound(R["rows"], R["rows"][0])
    wide = R["float32_ratio"].max(axis=1) > 1.0
    np.testing.assert_array_equal(R["bound"][~wide], base[~wide])
    assert np.all(R["bound"] >= base)
    assert wide.sum() <= 1 and not (wide.any() and c.model == 0)
    top = np.abs(R["rows"][0]).max()
    assert np.all(R["bound"][wide] <= cs.row_bound(top, top))
    np.testing.assert_allclose(
        R["bound"][wide], np.maximum(base, 4.0 * np.abs(
            R["float32_ratio"] * base).max(axis=1, keepdims=True))[wide],
        rtol=1e-12)
    # the trial entries' plain costs: the same rule
    pbase = cs.row_bound(R["plain"], R["plain"][0])
    pwide = R["plain_float32_ratio"].max(axis=1) > 1.0
    np.testing.assert_array_equal(R["plain_bound"][~pwide], pbase[~pwide])
    assert not (pwide.any() and c.model == 0)
    top = np.abs(R["plain"]).max()
    assert np.all(R["plain_bound"][pwide] <= cs.row_bound(top, top))


def test_float32_restatement_on_float64_far_planes_is_the_model():
    """The float32 formulas on the float64 far planes stay within the row
    bound of the model wherever the totals do not cancel: the restatement
    states the same rows."""
    name = "128x3n5-probe-gaussian-all-8-15"
    P, R = cs.inputs(name), cs.reference(name)
    c = P["case"]
    A, B = cs.far_planes(c.variable, P["x"], P["d"], P["other"], P["scan"],
                         c.det)
    for name2, fn, want in (("rows", cs.cost_rows_float32, R["rows"]),
                            ("plain", cs.plain_rows_float32, R["plain"])):
        got = fn(A, B, P["model_data"], P["mask"], c.model, P["step0"])
        assert np.all(np.abs(got - want) <= cs.row_bound(want, want[0])), name2
    name = "128x1n5-object-poisson-mask-8-15"
    P, R = cs.inputs(name), cs.reference(name)
    c = P["case"]
    A, B = cs.far_planes(c.variable, P["x"], P["d"], P["other"], P["scan"],
                         c.det)
    got = cs.cost_rows_float32(A, B, P["model_data"], P["mask"], c.model,
                               P["step0"])
    assert np.all(np.abs(got - R["rows"]) <= cs.row_bound(R["rows"],
                                                           R["rows"][0]))
