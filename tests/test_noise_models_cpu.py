"""tests/noise_models.py -- the float64 model the noise-model entries are held
to on the GPU -- against the oracle on a benign case, the preconditions of
every case of its table, the share of entries the bounds leave untested, and
three perturbations every bound must catch."""
import numpy as np
import pytest

import noise_models as nm
from oracle import operators as ops
from oracle import solvers as osol

NAMES = [c.name for c in nm.CASES]
# one case of every shape (the variants of a shape share far plane and counts)
SHAPES = [c.name for c in nm.CASES if c.masked and
          (c.u16 or c.kind == "stored")]


# ------------------------------------------------ the model against the oracle
def _benign(S, det, masked, seed=3):
    """A uniform random far plane and counts I u, u in (0.5, 1.5): no dark
    pixel, no dynamic range -- what the float32 oracle is good for."""
    rng = np.random.default_rng(seed)
    N = 4
    F = (rng.random((N, S, det, det)) - 0.5 + 1j *
         (rng.random((N, S, det, det)) - 0.5)).astype(np.complex64)
    I = ops.intensity_from_farplane(F[:, None])
    d = (I * rng.uniform(0.5, 1.5, I.shape)).astype(np.float32)
    mask = rng.random((det, det)) > 0.2 if masked else np.ones((det, det),
                                                               bool)
    return F, I, d, mask


@pytest.mark.parametrize("model", [0, 1])
def test_factor_gradient_and_costs_are_the_oracles(model):
    F, I, d, mask = _benign(3, 20, True)
    name = nm.MODELS[model]
    I64, d64 = I.astype(np.float64), d.astype(np.float64)
    fac = nm.factor(model, I64, d64, mask, 0.7)
    want = getattr(ops, name + "_grad")(d, F[:, None], I)[:, 0]
    got = nm.gradient(F, fac)
    # float32 tolerance: the oracle's product and quotient round at 2^-24
    assert np.abs(got[..., mask] + want[..., mask]).max() <= 1e-6 * np.abs(
        want).max()
    np.testing.assert_array_equal(fac[:, ~mask], np.float32(0.7) -
                                  np.float32(1))
    np.testing.assert_array_equal(got[..., ~mask],
                                  F[..., ~mask].astype(np.complex128) *
                                  float(np.float32(0.7) - np.float32(1)))
    each = getattr(ops, name + "_each_pattern")(d[:, mask][:, None, :],
                                                I[:, mask][:, None, :])
    np.testing.assert_allclose(nm.costs(model, I64, d64, mask)[0], each,
                               rtol=2e-6)
    np.testing.assert_allclose(nm.costs_float32(model, I, d, mask), each,
                               rtol=2e-6)
    np.testing.assert_allclose(
        nm.factor_float32(model, I, d)[:, mask], fac[:, mask], rtol=1e-6,
        atol=1e-6)


@pytest.mark.parametrize("S,masked", [(1, False), (3, True), (8, True)])
def test_step_lengths_are_the_oracles(S, masked):
    F, I, d, mask = _benign(S, 16, masked, seed=S)
    N = len(F)
    xi = (1 - d / (I + 1e-9))[:, None, None]
    start = np.full((N, 1, S, 1, 1), nm.STEP_START, np.float32)
    want = osol.poisson_steplength_all_modes(
        xi, np.abs(F[:, None])**2, I, d, mask, start, nm.WEIGHT)
    m = mask if masked else None
    I64, d64 = I.astype(np.float64), d.astype(np.float64)
    got = nm.steps_all_modes(F, I64, d64, m)
    np.testing.assert_allclose(got, want[:, 0, :, 0, 0], rtol=2e-5)
    np.testing.assert_allclose(
        nm.steps_float32(F, I, d, m, nm.STEP_START, nm.WEIGHT, False), got,
        rtol=2e-5)
    want = osol.poisson_steplength_dominant_mode(
        xi, I, d, mask, np.full((N, 1, 1, 1, 1), nm.STEP_START, np.float32),
        nm.WEIGHT)
    got = nm.steps_dominant_mode(F, I64, d64, m)
    assert got.shape == (N, S)
    np.testing.assert_allclose(got, np.broadcast_to(want[:, 0, :, 0, 0],
                                                    (N, S)), rtol=2e-5)
    np.testing.assert_allclose(
        nm.steps_float32(F, I, d, m, nm.STEP_START, nm.WEIGHT, True), got,
        rtol=2e-5)


def test_chi_is_the_oracles_adjoint_transform():
    F, I, d, mask = _benign(2, 16, True)
    fac = nm.factor(1, I.astype(np.float64), d.astype(np.float64), mask, 0.7)
    steps = np.array([[0.5, 0.75]] * len(F))
    G = nm.scaled_gradient(F, fac, steps, mask)
    np.testing.assert_array_equal(G[..., ~mask],
                                  nm.gradient(F, fac)[..., ~mask])
    np.testing.assert_allclose(G[:, 1][..., mask],
                               0.75 * nm.gradient(F, fac)[:, 1][..., mask],
                               rtol=1e-15)
    want = ops.propagation_adj(G.astype(np.complex64))
    got = nm.chi(G, nm.scale_of(16))
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


# ------------------------------------------------------- the table of cases
def test_table_covers_what_the_entries_branch_on():
    stored = [c for c in nm.CASES if c.kind == "stored"]
    assert {(c.det, c.S, c.masked) for c in stored} == {
        (d, s, m) for d in (24, 48, 15) for s in (1, 3, 8, 9)
        for m in (False, True)}
    assert all(c.N == 3 and not c.u16 for c in stored)
    hand = [c for c in nm.CASES if c.kind == "handoff"]
    assert {(c.det, c.S, c.N) for c in hand} == {
        (256, 1, 3), (256, 3, 3), (256, 6, 3), (256, 7, 3), (256, 8, 3),
        (512, 1, 2), (512, 4, 2)}
    for shape in {(c.det, c.S) for c in hand}:
        assert {(c.masked, c.u16) for c in hand if (c.det, c.S) == shape} == {
            (False, False), (False, True), (True, False), (True, True)}
    assert 24 <= len(nm.CASES) <= 60
    # 24^2 ends inside the first 1024-pixel trip of the all-modes step kernel,
    # 48^2 takes several and a tail, 15^2 is odd
    assert 24 * 24 < 1024 < 48 * 48 and (48 * 48) % 1024 and (15 * 15) % 2


@pytest.mark.parametrize("name", NAMES)
def test_case_inputs_are_detector_like(name):
    P = nm.inputs(name)
    c = P["case"]
    assert P["kinds"] == nm.PATTERNS[c.N] and "dim" in P["kinds"]
    assert any(k.endswith("+hot") for k in P["kinds"])
    I, d, mask = P["I"], P["model_data"], P["mask"]
    on = np.ones((c.det, c.det), bool) if mask is None else mask
    assert P["F"].shape == (c.N, c.S, c.det, c.det)
    assert np.all(I > 0) and np.all(np.isfinite(I))  # no 0 / 0 anywhere
    np.testing.assert_allclose(I.max(axis=(-2, -1)), nm.PEAK, rtol=1e-5)
    assert P["num_measured"] == on.sum()
    if c.masked:
        share = 1.0 - on.mean()
        assert 0.08 < share < 0.25
        assert (~on).all(axis=1).any() and (~on).all(axis=0).any()
    if c.u16:
        assert P["data"].dtype == np.uint16
        assert np.all(P["data"][:, ~on] == 65535)
    else:
        assert P["data"].dtype == np.float32
        assert np.all(np.isnan(P["data"][:, ~on]))
    dm = d[:, on]
    assert np.all(dm == np.rint(dm)) and dm.min() >= 0 and dm.max() <= 65535
    for n, kind in enumerate(P["kinds"]):
        zeros = (dm[n] == 0).mean()
        if kind == "dim":
            bright = I[n][on] > 1e3
            assert bright.any() and np.all(dm[n][bright] < 0.01 * I[n][on][
                bright])
            continue
        assert dm[n].max() >= 5e4, dm[n].max()
        assert zeros > (0.5 if kind.startswith("nine") else 0.15), zeros
        assert (dm[n] == 1).any()
        # counts where the model expects less than one; at the kernels' own
        # sizes, where it expects next to nothing
        assert I[n][on][dm[n] >= 1].min() < (1.0 if c.det < 256 else 1e-2)
        decades = np.log10(I[n].max() / I[n].min())
        assert decades > (9 if kind.startswith("nine") else 6)
    for n, (y, x) in P["hot"].items():
        assert on[y, x] and d[n, y, x] == 65535 and 0.3 < I[n, y, x] < 3.0
    if c.kind == "handoff":
        assert P["probe"].dtype == np.complex64
        assert P["probe"].shape == (c.N, c.S, c.det, c.det)
        # the forward error scale: float32 rounding of a transform of
        # log2(det^2) stages, a few 2^-24 of the largest wave
        top = np.abs(P["F"]).max(axis=(-2, -1))
        assert np.all(P["e"] > 0) and np.all(P["e"] < 64 * 2.0**-24 * top)
    else:
        assert np.all(P["e"] == 0)
        np.testing.assert_array_equal(P["F"], P["F32"])


@pytest.mark.parametrize("name", NAMES)
def test_sums_and_step_lengths_are_finite_and_bounded(name):
    c = nm.BY_NAME[name]
    for model in (0, 1):
        for ums, stored in ((nm.UNMEASURED, False), (1.0, c.kind == "stored")):
            R = nm.reference(name, model, ums, stored)
            assert np.all(np.isfinite(R["costs"]))
            assert np.all(R["costs_bound"] > 0)
            # 1e-5 of the absolute terms, unless float32 itself does worse
            assert np.all(R["costs_bound"] < 1e-3 * (1 + np.abs(R["costs"])))
            if model == 0:
                continue
            for key in ("steps_all", "steps_dominant"):
                assert np.all(np.isfinite(R[key]))
                assert np.all(R[key + "_denominator"] > 0)
                assert np.all(np.isfinite(R[key + "_bound"]))
                assert np.all(R[key + "_bound"] < 1e-3), R[key + "_bound"]
                # the restatement states the same step lengths
                assert np.all(np.abs(R[key + "_float32"] - R[key]) <
                              1e-4 * np.abs(R[key]))


@pytest.mark.parametrize("name", SHAPES)
def test_bounds_leave_at_most_a_thousandth_untested(name):
    """Per case, the share of measured entries whose bound exceeds 1e-2 (1 +
    |want|) is at most 0.1 %: a condition on the inputs."""
    P = nm.inputs(name)
    on = P["mask"]
    for model in (0, 1):
        R = nm.reference(name, model)
        for key in ("factor", "gradient"):
            want, bound = R[key], R[key + "_bound"]
            sel = np.broadcast_to(on, want.shape)
            wide = bound[sel] > 1e-2 * (1.0 + np.abs(want[sel]))
            print("UNTESTED {} {} {} {:.2e}".format(name, nm.MODELS[model],
                                                    key, wide.mean()))
            assert wide.mean() <= 1e-3
        assert np.all(R["factor_bound"][:, ~on] == 0)
        assert np.all(R["dI"] < 1e-2 * (1.0 + R["I"]))


# ------------------------------------------------------- the bounds have teeth
TEETH = ("stored-48x1n3-mask", "handoff-256x3n3-mask-u16")


def _bounds(name, model, ums):
    R = nm.reference(name, model, ums)
    chi, chi_bound = nm.chi_reference(name, model, ums, model == 1)
    want = {k: R[k] for k in ("factor", "gradient", "costs")}
    bound = {k: R[k + "_bound"] for k in want}
    if model == 1:
        for k in ("steps_all", "steps_dominant"):
            want[k], bound[k] = R[k], R[k + "_bound"]
    want["chi"], bound["chi"] = chi, chi_bound
    return want, bound


def _exceeds(got, want, bound, key):
    """Whether `got` misses the bound somewhere (a NaN misses it)."""
    err = np.abs(got - want)
    if key == "chi":
        err = np.linalg.norm(got - want, axis=(-2, -1))
    return not np.all(err <= bound)


def _perturbed(name, model, ums, what):
    P = nm.inputs(name)
    c = P["case"]
    d, mask, eps = np.array(P["model_data"]), P["mask"], nm.EPS
    if what == "eps":
        eps = 1e-6
    elif what == "int16":
        # the brightest measured count of the nine-decade pattern, >= 32768,
        # read as a signed 16-bit integer
        n = [k.startswith("nine") for k in P["kinds"]].index(True)
        y, x = np.unravel_index(np.argmax(np.where(mask, d[n], -1)),
                                mask.shape)
        assert d[n, y, x] >= 32768
        d[n, y, x] -= 65536
    else:
        # one unmeasured pixel taken as measured, holding what 16-bit data
        # hold there
        y, x = np.argwhere(~mask)[7]
        mask = mask.copy()
        mask[y, x] = True
        d[:, y, x] = 65535
    return nm.model_outputs(model, P["F"], P["I"], d, mask, ums, P["scale"],
                            eps)


@pytest.mark.parametrize("what", ["eps", "int16", "masked pixel"])
@pytest.mark.parametrize("model", [0, 1])
def test_every_bound_catches_the_perturbation(model, what):
    """1e-9 swapped for 1e-6, one count read as int16, one masked pixel
    included: every output that the perturbation reaches misses its bound in
    one of the two cases.  Three outputs are beyond reach of a change of the
    constant, at any input: the gaussian cost does not contain it; in the
    poisson cost it moves d log(I + 1e-9) by at most 1e-6 d / I at the few
    pixels with a count and I < 1e-3, against a bound of 1e-5 of the absolute
    terms of the bright pixels (worst error / bound over the stored cases:
    0.0065); and the gaussian chi, judged in the 2-norm of a tile, sees
    sqrt d / (sqrt I + 1e-9) move only where sqrt I is small, so F factor is
    too (worst: 0.56)."""
    caught = {}
    for name in TEETH:
        ums = nm.UNMEASURED
        want, bound = _bounds(name, model, ums)
        got = _perturbed(name, model, ums, what)
        assert set(got) == set(want)
        for key in want:
            hit = _exceeds(got[key], want[key], bound[key], key)
            print("TEETH {} {} {} {}: {}".format(name, nm.MODELS[model], what,
                                                 key, hit))
            caught[key] = caught.get(key, False) or hit
    beyond = set()
    if what == "eps":
        beyond = {"costs"} if model else {"costs", "chi"}
    assert {k for k, v in caught.items() if not v} <= beyond, caught
    # (and an unperturbed model misses nothing)
    for name in TEETH:
        want, bound = _bounds(name, model, nm.UNMEASURED)
        P = nm.inputs(name)
        got = nm.model_outputs(model, P["F"], P["I"], P["model_data"],
                               P["mask"], nm.UNMEASURED, P["scale"])
        for key in want:
            assert not _exceeds(got[key], want[key], bound[key], key)
