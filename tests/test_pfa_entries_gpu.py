"""The prime-factor chunk entries (csrc/pfa.hip), each called on its own by raw
pointers, against the float64 model of tests/pfa_model.py (itself pinned to
np.fft and the oracle by test_pfa_entries_cpu.py).

Output buffers start as NaN, in-place and accumulated ones from random
contents, and every writable buffer carries a guard pattern behind its end
(tests/devbuf.py).  Shapes: 96 = 3 x 32, 160 = 5 x 32, 224 = 7 x 32, 192 = 3 x
64, 384 / 640 / 896 (M = 128, the one-launch forward), 1024 and 2048 (the
Cooley-Tukey step); windows pw = det, smaller by an even and by an odd
difference, pw = 5, and 600 in 640 (the loops for windows wider than 512);
S in {1, 3, 4, 5, 6, 7, 14, 16, 50}; 0, 1, 8, 9 and 17 positions, inside the
object, on its last legal corner, one row past it and over every side.

Bars.  Arrays: assert_close at OP_NORMWISE / OP_MAXABS against the model;
patches at whole-pixel positions exact.  Costs: 8 x the error of the same
formula in float32 NumPy on the model's far plane rounded to float32, not
below 1e-6 x the mean |term|, pattern by pattern.  The largest float32 error
of a pattern of the cases below, relative to its mean |term|, per (p, model)
-- gaussian ; poisson:
  p = 3: 7.9e-08 ; 8.2e-08   p = 5: 4.3e-08 ; 1.9e-08
  p = 7: 1.3e-07 ; 6.4e-08   p = 4: 8.2e-07 ; 6.0e-08
(MEASURED collects them as the cases run and every case prints the figure so
far), so the bars are the floor or little above it, up to 6.6e-6 x the mean
|term| for the 4 M pixels of 2048^2.
tike_pfa_fwd_subtiles against tike_pfa_fwd_gather + tike_pfa_fft2: their
difference must stay within the sum of their two errors against the model
(normwise, measured on an MI355X over the cases below: one launch 1.09e-07 ..
1.42e-07, two launches 1.10e-07 .. 1.43e-07, difference 0 .. 1.51e-07; 0 where
no position takes the interior path of the one-launch kernel).

LDS above 48 KiB.  Products: det = pw = 224, S = 14 (224 x 28 x 8 = 50 176
bytes).  Gather with eigen probes: the smallest detector (96, pw = det) and
there the fewest modes whose 8 pw (1 + S + C Sm) exceeds 49 152 with Sm <= S, C
<= 3: S = 16, C = 3, Sm = 16 (49 920 bytes)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pfa_cases as pc
import pfa_model as pm
from devbuf import Dev, dev, dptr
from util import assert_close, relerr

pytestmark = pytest.mark.gpu

ERR_ARG = 1000001
MEASURED = {}


def _api():
    import tike_amd._arrays as A
    from tike_amd._lib import lib
    return A, lib


def probe_args(pr):
    """The device arrays of a probe case (kept alive by the caller) and the
    arguments probe, probe_per_scan, unique, eigen_probe, eigen_weights,
    num_eigen, eigen_modes."""
    keep = [dev(pr[k]) for k in ("probe", "unique", "eigen", "weights")]
    p, u, e, w = keep
    return keep, (dptr(p), int(pr["form"] == "per_scan"), dptr(u), dptr(e),
                  dptr(w), pr["C"], pr["Sm"])


def whole_pixel(scan):
    return np.all(scan == np.floor(scan), axis=1)


# (det, pw, S, nscan, form, C, Sm, first position of the ring)
CASES = [
    (96, 96, 1, 1, "shared", 0, 0, 3),
    (96, 96, 6, 17, "unique", 0, 2, 0),
    (96, 64, 3, 8, "eigen", 1, 1, 0),
    (96, 64, 7, 9, "weights", 0, 0, 4),
    (96, 95, 4, 9, "shared", 0, 0, 0),
    (96, 95, 4, 9, "per_scan", 0, 0, 3),
    (96, 95, 4, 9, "weights", 0, 0, 5),
    (96, 95, 4, 9, "eigen", 2, 2, 7),
    (96, 95, 4, 9, "unique", 0, 4, 9),
    (96, 5, 5, 17, "per_scan", 0, 0, 0),
    (96, 95, 3, 0, "shared", 0, 0, 0),
    (96, 64, 4, 0, "eigen", 2, 2, 0),
    (160, 160, 3, 9, "unique", 0, 1, 0),
    (160, 127, 5, 17, "eigen", 1, 5, 0),
    (160, 5, 4, 8, "per_scan", 0, 0, 8),
    (160, 100, 1, 1, "weights", 0, 0, 4),
    (224, 224, 4, 8, "eigen", 2, 2, 3),
    (224, 100, 6, 17, "shared", 0, 0, 0),
    (224, 223, 3, 9, "per_scan", 0, 0, 9),
    (192, 192, 7, 9, "eigen", 1, 7, 0),
    (192, 128, 1, 17, "weights", 0, 0, 0),
    (192, 191, 5, 8, "unique", 0, 3, 5),
    (640, 600, 2, 2, "shared", 0, 0, 3),
    (640, 600, 3, 2, "eigen", 1, 1, 5),
    (1024, 1024, 1, 2, "shared", 0, 0, 3),
    (1024, 1001, 1, 2, "eigen", 1, 1, 5),
    (2048, 2048, 1, 1, "shared", 0, 0, 4),
    (2048, 2000, 1, 1, "weights", 0, 0, 10),
]
# LDS above 48 KiB (the hipFuncSetAttribute branch of the launchers)
LDS_PRODUCTS = (224, 224, 14, 2, "shared", 0, 0, 3)
LDS_GATHER = (96, 96, 16, 2, "eigen", 3, 16, 3)
# tike_pfa_supported = 1 with more eigen rows than its 2 S: C Sm = 3 S
SUPPORT = [
    (96, 96, 50, 2, "eigen", 3, 50, 3),
    (160, 160, 30, 1, "eigen", 3, 30, 4),
    (224, 224, 21, 1, "eigen", 3, 21, 2),
    (96, 96, 10, 2, "eigen", 2, 10, 3),
]


def _id(c):
    return "-".join(str(v) for v in c)


def run_gather(case):
    A, lib = _api()
    det, pw, S, nscan, form, C, Sm, first = case
    assert lib.tike_pfa_supported(S, pw, det) == 1
    g = pm.Geom(det)
    H, W = pc.object_shape(pw)
    psi = pc.random_object(pw, det + pw)
    scan = pc.positions(pw, nscan, first)
    pr = pc.probe_case(form, nscan, S, pw, 7 * det + S, C=C, Sm=Sm)
    keep, pargs = probe_args(pr)
    nb = max(nscan, 1)  # (no position: buffers that must stay as they are)
    sub = Dev((nb, S, g.p, g.p, g.M, g.M), cplx=True)
    patches = Dev((nb, pw, pw), cplx=True)
    psi_d, scan_d = dev(psi), dev(scan)
    rc = lib.tike_pfa_fwd_gather(dptr(psi_d), dptr(scan_d), *pargs, sub.ptr(),
                                 patches.ptr(), nscan, S, pw, det, H, W,
                                 A.stream_ptr())
    assert rc == 0, rc
    if nscan == 0:
        assert sub.untouched() and patches.untouched()
        return
    want_sub, want_patches = pm.fwd_gather(psi, scan, pr["probes"], det)
    got_sub, got_patches = sub.get(), patches.get()
    assert not np.isnan(got_sub.view(np.float32)).any()
    assert not np.isnan(got_patches.view(np.float32)).any()
    assert_close(got_sub, want_sub, what="subtiles")
    assert_close(got_patches, want_patches, what="patches")
    whole = whole_pixel(scan)
    np.testing.assert_array_equal(got_patches[whole],
                                  want_patches[whole].astype(np.complex64))
    # ... and with patches NULL the sub-tiles are the same
    sub2 = Dev((nb, S, g.p, g.p, g.M, g.M), cplx=True)
    rc = lib.tike_pfa_fwd_gather(dptr(psi_d), dptr(scan_d), *pargs, sub2.ptr(),
                                 None, nscan, S, pw, det, H, W, A.stream_ptr())
    assert rc == 0, rc
    np.testing.assert_array_equal(sub2.get(), got_sub)
    del keep


def run_products(case, skip=()):
    A, lib = _api()
    det, pw, S, nscan, form, C, Sm, first = case
    assert lib.tike_pfa_supported(S, pw, det) == 1
    g = pm.Geom(det)
    rng = np.random.default_rng(det * 31 + pw + S)
    nb = max(nscan, 1)
    sub = pc.rc(rng, nb, S, g.p, g.p, g.M, g.M)
    patches = pc.rc(rng, nb, pw, pw)
    mpu0 = pc.rc(rng, S, pw, pw)
    pr = pc.probe_case(form, nscan, S, pw, 5 * det + S, C=C, Sm=Sm)
    keep, pargs = probe_args(pr)
    inv_scale, scale = 0.7, 0.25
    objproj = Dev((nb, pw, pw), cplx=True)
    chi0 = Dev((nb, pw, pw), cplx=True)
    mpu = Dev((S, pw, pw), cplx=True, init=mpu0)
    sub_d, patches_d = dev(sub), dev(patches)
    rc = lib.tike_pfa_inv_products(
        dptr(sub_d), dptr(patches_d), *pargs,
        None if "objproj" in skip else objproj.ptr(),
        None if "chi0" in skip else chi0.ptr(),
        None if "mpu" in skip else mpu.ptr(), scale, nscan, S, pw, det,
        inv_scale, A.stream_ptr())
    assert rc == 0, rc
    if nscan == 0:
        assert objproj.untouched() and chi0.untouched() and mpu.untouched()
        return
    w_objproj, w_chi0, w_mpu, _ = pm.inv_products(
        sub[:nscan], patches[:nscan], pr["probes"], det, inv_scale, scale, mpu0)
    for name, buf, want in (("objproj", objproj, w_objproj),
                            ("chi0", chi0, w_chi0), ("mpu", mpu, w_mpu)):
        if name in skip:
            assert buf.untouched(), name
        else:
            got = buf.get()
            assert not np.isnan(got.view(np.float32)).any(), name
            assert_close(got, want, what=name)
    del keep


# ------------------------------------------------------- gather and products
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fwd_gather(case):
    """tike_pfa_fwd_gather: pad(patch x probe) in the sub-tile layout, and
    patches; no position: returns 0 and touches nothing."""
    run_gather(case)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_inv_products(case):
    """tike_pfa_inv_products on random sub-tiles: objproj, chi0 and the
    accumulated m_probe_update (from random contents)."""
    run_products(case)


@pytest.mark.parametrize("skip", [("objproj",), ("chi0",), ("mpu",),
                                  ("objproj", "chi0")])
@pytest.mark.parametrize("case", [CASES[7], CASES[13]], ids=_id)
def test_inv_products_null_outputs(case, skip):
    """Each output NULL to skip: the others as before, the skipped untouched."""
    run_products(case, skip)


def test_lds_above_48k_products():
    """224 x 28 x 8 = 50 176 bytes of dynamic LDS."""
    det, pw, S = LDS_PRODUCTS[:3]
    assert 8 * pw * 2 * S == 50176 > 48 * 1024
    run_products(LDS_PRODUCTS)


def test_lds_above_48k_gather():
    """The smallest supported shape with eigen probes above 48 KiB: at det = pw
    = 96 the fewest modes with 8 pw (1 + S + C Sm) > 49 152."""
    _, lib = _api()
    det, pw, S, _, _, C, Sm, _ = LDS_GATHER
    need = lambda s, c, sm: 8 * pw * (1 + s + c * sm)
    assert 48 * 1024 < need(S, C, Sm) == 49920 <= 150 * 1024
    assert all(need(s, c, sm) <= 48 * 1024 for s in range(1, S)
               for c in range(4) for sm in range(s + 1))
    assert lib.tike_pfa_supported(S, pw, det) == 1
    run_gather(LDS_GATHER)
    run_products(LDS_GATHER)


@pytest.mark.parametrize("case", SUPPORT, ids=_id)
def test_supported_shapes_run(case):
    """Where tike_pfa_supported says 1, the gather and the products return 0
    and match the model for every valid eigen shape (Sm <= S, C <= 3) -- also
    where the hoisted probe and eigen rows exceed the LDS of a CU."""
    run_gather(case)
    run_products(case)


# ------------------------------------------------------ sub-tile transforms
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("det", [96, 160, 224, 192, 384, 1024, 2048])
def test_fft2(det, inverse):
    """tike_pfa_fft2: the unscaled M x M transform of every sub-tile."""
    A, lib = _api()
    g = pm.Geom(det)
    ntile = 1 if det >= 1024 else 3
    x = pc.rc(np.random.default_rng(det + inverse), ntile, g.p, g.p, g.M, g.M)
    out = Dev(x.shape, cplx=True)
    x_d = dev(x)
    rc = lib.tike_pfa_fft2(dptr(x_d), out.ptr(), ntile, det, inverse,
                           A.stream_ptr())
    assert rc == 0, rc
    assert_close(out.get(), pm.subtile_fft(x.astype(np.complex128), inverse),
                 what="sub-tile transforms")
    np.testing.assert_array_equal(x_d.cpu().numpy(), x)
    assert lib.tike_pfa_fft2(dptr(x_d), out.ptr(), 0, det, inverse,
                             A.stream_ptr()) == 0


# ------------------------------------------- gather + transform in one launch
SUBTILES = (
    [(384, 384, 2, 2, "shared", 0, 0, f) for f in range(0, 18, 2)] +
    [(384, 301, 2, 2, "eigen", 1, 1, 3), (384, 300, 1, 2, "weights", 0, 0, 5),
     (384, 5, 2, 2, "eigen", 2, 2, 7), (384, 384, 2, 0, "shared", 0, 0, 0),
     (640, 640, 2, 2, "eigen", 1, 2, 3), (640, 600, 2, 2, "shared", 0, 0, 5),
     (896, 896, 2, 2, "shared", 0, 0, 3), (896, 895, 1, 2, "weights", 0, 0, 9)])


@pytest.mark.parametrize("case", SUBTILES, ids=_id)
def test_fwd_subtiles(case):
    """tike_pfa_fwd_subtiles against the model, and against what
    tike_pfa_fwd_gather + tike_pfa_fft2 leave (both sides of `interior`: the
    last legal corner, one row and one column past it are positions 3, 4 and
    17 of the ring)."""
    A, lib = _api()
    det, pw, S, nscan, form, C, Sm, first = case
    assert lib.tike_pfa_fwd_subtiles_supported(S, pw, det) == 1
    g = pm.Geom(det)
    H, W = pc.object_shape(pw)
    psi = pc.random_object(pw, det + pw)
    scan = pc.positions(pw, nscan, first)
    pr = pc.probe_case(form, nscan, S, pw, 3 * det + S, C=C, Sm=Sm)
    keep, pargs = probe_args(pr)
    probe_p, _, _, eigen_p, w_p, nC, nSm = pargs
    nb = max(nscan, 1)
    shape = (nb, S, g.p, g.p, g.M, g.M)
    one, patches = Dev(shape, cplx=True), Dev((nb, pw, pw), cplx=True)
    scratch = Dev((S + nC * nSm, det, det), cplx=True)
    psi_d, scan_d = dev(psi), dev(scan)
    rc = lib.tike_pfa_fwd_subtiles(dptr(psi_d), dptr(scan_d), probe_p, eigen_p,
                                   w_p, nC, nSm, scratch.ptr(), one.ptr(),
                                   patches.ptr(), nscan, S, pw, det, H, W,
                                   A.stream_ptr())
    assert rc == 0, rc
    if nscan == 0:
        assert one.untouched() and patches.untouched() and scratch.untouched()
        return
    scratch.get()  # (guard)
    mid, two = Dev(shape, cplx=True), Dev(shape, cplx=True)
    patches2 = Dev((nb, pw, pw), cplx=True)
    assert lib.tike_pfa_fwd_gather(dptr(psi_d), dptr(scan_d), *pargs, mid.ptr(),
                                   patches2.ptr(), nscan, S, pw, det, H, W,
                                   A.stream_ptr()) == 0
    assert lib.tike_pfa_fft2(mid.ptr(), two.ptr(), nscan * S, det, 0,
                             A.stream_ptr()) == 0
    sub, want_patches = pm.fwd_gather(psi, scan, pr["probes"], det)
    want = pm.subtile_fft(sub)
    got1, got2, got_patches = one.get(), two.get(), patches.get()
    assert_close(got1, want, what="one launch")
    assert_close(got2, want, what="two launches")
    assert_close(got_patches, want_patches, what="patches")
    assert_close(patches2.get(), want_patches, what="patches, two launches")
    whole = whole_pixel(scan)
    np.testing.assert_array_equal(got_patches[whole],
                                  want_patches[whole].astype(np.complex64))
    e1, e2 = relerr(got1, want), relerr(got2, want)
    diff = float(np.linalg.norm((got1.astype(np.complex128) - got2).ravel()) /
                 np.linalg.norm(want.ravel()))
    print(f"fwd_subtiles {_id(case)}: one launch {e1:.2e}, two launches "
          f"{e2:.2e}, difference {diff:.2e}")
    assert diff <= e1 + e2
    del keep


# ------------------------------------------------------------------ combine
COMBINE = [(det, S) for det, S, _ in pc.COMBINE]


@functools.lru_cache(maxsize=2)
def combine_inputs(det, S):
    c = pc.combine_case(det, S, dict((d, n) for d, _, n in pc.COMBINE)[det])
    c["F32"] = pm.far_plane(c["sub"], det, c["fwd_scale"]).astype(np.complex64)
    return c


@functools.lru_cache(maxsize=8)
def combine_model(det, S, model, masked, us):
    """(in-place result, costs, the cost bar per pattern) of one setting."""
    c = combine_inputs(det, S)
    mask = c["mask"] if masked else None
    data = c["data_nan"] if masked else c["data"]
    nm = int(c["mask"].sum()) if masked else det * det
    out, costs, _, _ = pm.combine_gradient(c["sub"], data, mask, det,
                                           c["fwd_scale"], model, us, nm)
    c64, _, _, mean_abs = pm.costs_and_factor(c["F32"], data, mask, model, us, nm)
    c32 = pm.costs_and_factor(c["F32"], data, mask, model, us, nm,
                              dtype=np.float32)[0]
    e32 = np.abs(c32.astype(np.float64) - c64)  # of every pattern
    key = (pm.Geom(det).p, model)
    MEASURED[key] = max(MEASURED.get(key, 0.0), float((e32 / mean_abs).max()))
    return out, costs, np.maximum(8.0 * e32, 1e-6 * mean_abs), nm


# per shape: every (model, mask, unmeasured_scaling) with the gradient, cost
# only, and once more with costs NULL (ordered so that the model of a setting
# is computed once)
COMBINE_SETTINGS = [
    (det, S, model, masked, us, apply_gradient, with_costs)
    for det, S in COMBINE for model in (0, 1) for masked in (False, True)
    for us in (1.0, 0.9)
    for apply_gradient, with_costs in ((1, True), (0, True), (1, False))
    if with_costs or us == 0.9]


@pytest.mark.parametrize(
    "det,S,model,masked,us,apply_gradient,with_costs", COMBINE_SETTINGS)
def test_combine_gradient(det, S, model, masked, us, apply_gradient, with_costs):
    """tike_pfa_combine_gradient on a chosen far plane (never dark): costs, and
    in place the input of the inverse sub-tile transforms; apply_gradient = 0
    leaves the sub-tiles bit for bit; NaN counts under the mask."""
    A, lib = _api()
    c = combine_inputs(det, S)
    want, want_costs, bars, nm = combine_model(det, S, model, masked, us)
    sub = Dev(c["sub"].shape, cplx=True, init=c["sub"])
    costs = Dev(c["nscan"]) if with_costs else None
    data_d = dev(c["data_nan"] if masked else c["data"])
    mask_d = dev(c["mask"]) if masked else None
    rc = lib.tike_pfa_combine_gradient(
        sub.ptr(), dptr(data_d), dptr(mask_d), costs.ptr() if costs else None,
        c["nscan"], S, det, c["fwd_scale"], model, us, nm, apply_gradient,
        A.stream_ptr())
    assert rc == 0, rc
    if costs is not None:
        got = costs.get().astype(np.float64)
        err = np.abs(got - want_costs)
        print(f"costs det {det} model {model}: error {err.max():.2e}, bars "
              f"{bars.min():.2e}, cost {want_costs[0]:.4f}; largest float32 "
              f"error / mean |term| at p = {pm.Geom(det).p} so far "
              f"{MEASURED[(pm.Geom(det).p, model)]:.1e}")
        assert np.all(err <= bars), (got, want_costs, bars)
    if apply_gradient:
        assert_close(sub.get(), want, what="F x factor through the inverse DFT")
    else:
        assert sub.untouched()


def test_combine_gradient_no_position():
    A, lib = _api()
    sub, costs = Dev((1, 1, 3, 3, 32, 32), cplx=True), Dev(1)
    data_d = dev(np.ones((1, 96, 96), np.float32))
    assert lib.tike_pfa_combine_gradient(sub.ptr(), dptr(data_d), None,
                                         costs.ptr(), 0, 1, 96, 1.0 / 96, 0, 1.0,
                                         96 * 96, 1, A.stream_ptr()) == 0
    assert sub.untouched() and costs.untouched()


# ------------------------------------------------------- deterministic mode
def test_products_deterministic_mode():
    """tike_set_deterministic is process-wide: a fresh child runs the products
    at 96^2, 17 positions with ample scratch twice (bit-identical, within the
    bars), with scratch for one set of partial sums only (the one-chunk
    fallback) and with less than that (TIKE_ERR_ARG, nothing written)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "TIKE_DETERMINISTIC"}
    p = subprocess.run([sys.executable, os.path.join(here, "_pfa_entries_child.py")],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    r = json.loads(line[len("RESULT "):])
    assert r["nchunk"] > 1
    assert r["ample_digests"][0] == r["ample_digests"][1]
    assert r["ample_ok"] and r["one_set_ok"], r
    assert r["too_small_rc"] == ERR_ARG and r["too_small_untouched"], r
