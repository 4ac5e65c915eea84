"""Pins tests/overlap_sums.py -- the float64 model of the gather sums and the
footprint scatter, its table of cases and its bounds -- without a GPU:

  - the model against oracle.patch_fwd / patch_adj and the oracle's lstsq
    gradient lines (solvers.get_nearplane_gradients: conj(unique_probe) chi
    summed over the modes, conj(patches) chi summed over the positions) at the
    float32 tolerance of tests/util.py;
  - adjointness in float64, <patches_of(psi), v> == <psi, scatter(v)>;
  - the preconditions of the cases: the position lists, the route of every
    group of the scatter cases, the chunk counts, the float32 restatement
    inside its own bound, at most 1 % of a case's elements widened by the
    restatement term (the worst single output: the one-product objproj of the
    S = 1 case, 1.8 % of its 225 elements);
  - reach: every mutant of overlap_sums.MUTANTS leaves the bound somewhere."""
import numpy as np
import pytest

import overlap_sums as om
from oracle import operators as ops
from oracle import solvers as osol
from util import assert_close

GATHER = [g.name for g in om.GATHER]
SCATTER = [s.name for s in om.SCATTER]
KEYS = ("patches", "objproj", "m_probe_update", "probe_preconditioner")


def _prev(I, key):
    return {"m_probe_update": I["mpu0"]}.get(key)


# ------------------------------------------------------------ model vs oracle
@pytest.mark.parametrize("name", GATHER)
def test_gather_model_vs_oracle(name):
    I = om.gather_inputs(name)
    c, R = I["case"], om.gather_reference(name)
    patches = ops.patch_fwd(I["psi"], I["scan"], patch_width=c.pw)
    assert_close(R["patches"].value, patches, what="patches")
    # pfa_model states the same gather (with the reference's linear taps)
    import pfa_model as pm
    np.testing.assert_allclose(R["patches"].value,
                               pm.patches_of(I["psi"], I["scan"], c.pw),
                               rtol=0, atol=1e-13)
    call = I["call"]
    unique = osol.get_varying_probe(
        I["probe"][None, None],
        None if call["eigen"] is None else call["eigen"][None],
        None if call["form"] == "shared" else I["weights"])
    unique = np.broadcast_to(unique, (c.nscan, 1, c.S, c.pw, c.pw)).copy()
    if call["form"] == "unique":
        unique[:, 0, :c.Sm] = I["unique"]
    chi = I["chi"][:, None]
    proj = np.sum(np.conj(unique) * chi, axis=(1, 2))
    assert_close(R["objproj"].value, proj, what="objproj")
    mpu = np.sum(np.conj(patches[:, None, None]) * chi, axis=0)[0]
    assert_close(R["m_probe_update"].value, mpu, what="m_probe_update")
    pre = np.sum(np.abs(patches)**2, axis=0)
    assert_close(R["probe_preconditioner"].value, pre, what="preconditioner")


@pytest.mark.parametrize("name", [s.name for s in om.SCATTER
                                  if s.layout != "over"])
def test_scatter_model_vs_oracle(name):
    I = om.scatter_inputs(name)
    c = I["case"]
    for entry in om.SCATTER_ENTRIES:
        v = om.scatter_values(I, entry)[0]
        vs = np.broadcast_to(v, (c.nscan, c.pw, c.pw)).astype(np.complex64)
        want = ops.patch_adj(I["scan"], vs, height=c.H, width=c.W)
        assert_close(om.scatter_reference(name, entry).value, want, what=entry)


def test_overhanging_pixels_are_dropped():
    """The footprint of a position over a border, cut at the border, is what
    the same footprint leaves inside a larger object."""
    I = om.scatter_inputs("pw65-over-n13")
    c, m = I["case"], 8
    R = om.scatter_reference(c.name, "tike_scatter_patches")
    big = om.scatter(I["proj"], I["scan"] + np.float32(m), c.H + 2 * m,
                     c.W + 2 * m)
    inner = (slice(m, m + c.H), slice(m, m + c.W))
    # (the fractions of the moved positions round differently in float32)
    np.testing.assert_allclose(R.value, big.value[inner], rtol=0, atol=1e-5)
    outside = big.abs_terms.copy()
    outside[inner] = 0
    assert outside.max() > 0  # (something does hang over)
    rows, cols = np.nonzero(outside)
    assert rows.min() < m and rows.max() >= m + c.H
    assert cols.min() < m and cols.max() >= m + c.W


@pytest.mark.parametrize("name", GATHER[:6])
def test_adjointness(name):
    I = om.gather_inputs(name)
    c = I["case"]
    v = I["chi"][:, 0].astype(np.complex128)
    psi = I["psi"].astype(np.complex128)
    lhs = np.vdot(v, om.patches_of(psi, I["scan"], c.pw).value)
    rhs = np.vdot(om.scatter(v, I["scan"], I["H"], I["W"]).value, psi)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


# -------------------------------------------------------------- preconditions
def _has_specials(scan, H, W, pw, nscan):
    corner, frac = om.corners(scan)
    rows = {tuple(r) for r in np.asarray(scan).tolist()}
    assert len(rows) == len(scan) - 1, "one position listed twice"
    assert (1.0, 1.0) in rows and (float(H - pw - 1), float(W - pw - 1)) in rows
    assert np.any(np.all(frac == 0, axis=1) & np.all(corner > 1, axis=1))
    assert np.any((frac[:, 0] > 0) & (frac[:, 0] < 1e-5)
                  & (frac[:, 1] < 1) & (frac[:, 1] > 1 - 1e-5))


def test_position_lists():
    for g in om.GATHER:
        I = om.gather_inputs(g.name)
        corner, _ = om.corners(I["scan"])
        assert corner.min() >= 1
        assert np.all(corner <= (I["H"] - g.pw - 1, I["W"] - g.pw - 1))
        assert (I["H"], I["W"]) == (g.pw + 21, g.pw + 34)
        if g.nscan >= 8:
            _has_specials(I["scan"], I["H"], I["W"], g.pw, g.nscan)
    for s in om.SCATTER:
        I = om.scatter_inputs(s.name)
        assert s.H != s.W
        if s.layout == "whole":
            assert np.all(I["scan"] == np.floor(I["scan"]))
            rows = {tuple(r) for r in I["scan"].tolist()}
            assert (1.0, 1.0) in rows and (s.H - s.pw - 1.0, s.W - s.pw - 1.0) in rows
        elif s.nscan >= 8:
            _has_specials(I["scan"], s.H, s.W, s.pw, s.nscan)
        corner, _ = om.corners(I["scan"])
        inside = (corner.min() >= 1
                  and np.all(corner <= (s.H - s.pw - 1, s.W - s.pw - 1)))
        assert inside == (s.layout != "over")
        if s.layout == "over":
            assert corner[:, 0].min() < 0 and corner[:, 1].min() < 0
            assert (corner[:, 0].max() + s.pw >= s.H
                    and corner[:, 1].max() + s.pw >= s.W)


def test_scatter_groups_take_the_claimed_route():
    seen = set()
    for s in om.SCATTER:
        scan = om.scatter_inputs(s.name)["scan"]
        assert om.boxed_groups(scan) == s.boxed, s.name
        assert len(s.boxed) == (s.nscan + om.GROUP - 1) // om.GROUP
        corner, _ = om.corners(scan[:om.GROUP])
        spread = corner.max(axis=0) - corner.min(axis=0)
        want = {"wide_in": (None, om.GSPREAD), "wide_out": (None, om.GSPREAD + 1),
                "tall_in": (om.GSPREAD, None), "tall_out": (om.GSPREAD + 1, None)}
        for got, exact in zip(spread, want.get(s.layout, (None, None))):
            assert exact is None or got == exact, s.name
        seen.add((s.pw, s.layout))
    assert {pw for pw, _ in seen} == {7, 31, 32, 63, 64, 65, 130}
    assert {l for _, l in seen} == set(om._LAYOUT)
    # the fallback at every wave count of a strip's columns, the box's too
    assert {pw for pw, l in seen if l.endswith("_out")} >= {7, 31, 32, 63, 65, 130}


def test_chunk_counts():
    assert [om.num_chunks(n) for n in (1, 8, 9, 70)] == [1, 1, 2, 9]
    assert {g.nscan for g in om.GATHER} == {1, 8, 9, 70}
    assert {g.pw for g in om.GATHER} >= {15, 17, 40}
    assert {g.S for g in om.GATHER} >= {1, 2, 3, 5, 6, 8, 7, 9, 16}
    assert {g.form for g in om.GATHER} >= {"shared", "weights", "eigen", "unique"}
    assert ("eigen", 1, 1, 3) in {(g.form, g.C, g.Sm, g.S) for g in om.GATHER}
    assert any(g.form == "eigen" and g.C == 2 and g.Sm == g.S for g in om.GATHER)
    assert {g.outputs for g in om.GATHER} == set(om.OUTPUTS)


def _widened(pairs):
    """(the restatement's worst error / bound, widened elements / elements)."""
    worst, wide, total = 0.0, 0, 0
    for want, f32, prev in pairs:
        worst = max(worst, float(om.restatement_ratio(want, f32).max()))
        w = om.bound(want, f32, prev)[1]
        wide, total = wide + int(w.sum()), total + w.size
    return worst, wide / total


@pytest.mark.parametrize("name", GATHER)
def test_gather_restatement_within_its_bound(name):
    I = om.gather_inputs(name)
    R, R4 = om.gather_reference(name), om.gather_reference(name, None, om.F4)
    worst, frac = _widened([(R[k], R4[k], _prev(I, k)) for k in KEYS])
    print("RESTATEMENT {} worst {:.3f} widened {:.4f}".format(name, worst, frac))
    assert worst <= 1.0 and frac <= 0.01


@pytest.mark.parametrize("name", SCATTER)
def test_scatter_restatement_within_its_bound(name):
    I = om.scatter_inputs(name)
    worst, frac = _widened([
        (om.scatter_reference(name, e), om.scatter_reference(name, e, None, om.F4),
         om.scatter_values(I, e)[1]) for e in om.SCATTER_ENTRIES])
    print("RESTATEMENT {} worst {:.3f} widened {:.4f}".format(name, worst, frac))
    assert worst <= 1.0 and frac <= 0.01
    for e in om.SCATTER_ENTRIES:  # some pixel no footprint reaches, or weighs 0
        assert np.any(om.scatter_reference(name, e).abs_terms == 0) or \
            I["case"].layout == "over" or I["case"].W == 20


def test_whole_pixel_footprint_has_an_empty_last_column():
    I = om.scatter_inputs("pw31-neighbours-n1")
    scan = np.floor(I["scan"])
    R = om.scatter(I["proj"], scan, I["case"].H, I["case"].W)
    sy, sx = scan[0].astype(int)
    assert np.all(R.abs_terms[sy:sy + 31, sx:sx + 31] > 0)
    assert np.all(R.abs_terms[:, sx + 31] == 0) and np.all(R.abs_terms[sy + 31] == 0)


# ---------------------------------------------------------------------- reach
def _escapes(mut, side):
    """The first (case, output) of a side on which the mutant leaves the bound."""
    for g in om.GATHER if side == "gather" else ():
        I = om.gather_inputs(g.name)
        R, M = om.gather_reference(g.name), om.gather_reference(g.name, mut)
        for k in KEYS:
            prev = _prev(I, k)
            got = M[k].value + (0 if prev is None else prev)
            if om.ratio(got, R[k], om.gather_bound(g.name, k, prev)[0], prev) > 1:
                return g.name, k
    for s in om.SCATTER if side == "scatter" else ():
        I = om.scatter_inputs(s.name)
        for e in om.SCATTER_ENTRIES:
            prev = om.scatter_values(I, e)[1]
            R, M = om.scatter_reference(s.name, e), om.scatter_reference(s.name, e, mut)
            if om.ratio(M.value + prev, R, om.scatter_bound(s.name, e)[0], prev) > 1:
                return s.name, e
    return None


# the side(s) of the family a mutant changes
REACH = [(m, "gather") for m in om.MUTANTS
         if m not in ("no_last_column", "no_last_row")] + [
    (m, "scatter") for m in ("w01_w10", "no_last_column", "no_last_row", "H_W",
                             "no_duplicate")]


@pytest.mark.parametrize("mut,side", REACH)
def test_mutant_leaves_the_bound(mut, side):
    where = _escapes(mut, side)
    print("MUTANT", mut, side, where)
    assert where is not None


def test_dropped_position_of_a_later_chunk_is_seen():
    """... also where the list has several chunks and the sum 70 terms."""
    name = "pw17-n70-S5-eigen25"
    I, R = om.gather_inputs(name), om.gather_reference(name)
    M = om.gather_reference(name, "chunk_last")
    for k, prev in (("m_probe_update", I["mpu0"]), ("probe_preconditioner", None)):
        got = M[k].value + (0 if prev is None else prev)
        assert om.ratio(got, R[k], om.gather_bound(name, k, prev)[0], prev) > 1


def test_model_itself_is_inside():
    for g in om.GATHER[:3]:
        R = om.gather_reference(g.name)
        for k in KEYS:
            assert om.ratio(R[k].value, R[k], om.gather_bound(g.name, k)[0]) == 0
