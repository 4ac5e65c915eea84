"""Far-field blur on the GPU: the two entries of blur.hip entry by entry
against the float64 model (tests/blur.py), then the routes built on them.

Every figure a bar is set on is printed before it is asserted.  u = 2^-24 is
the unit roundoff of float32."""
import functools

import numpy as np
import pytest

import autograd_cost as ac
import blur as bl
import fly_scan as fs
import noise_models as nm_
from util import OP_NORMWISE, assert_close, relerr

pytestmark = pytest.mark.gpu

U = 2.0**-24
MODEL_ID = {"gaussian": 0, "poisson": 1}
VARIANTS = [(model, masked, u16) for model in ("gaussian", "poisson")
            for masked in (False, True) for u16 in (False, True)]


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(
        np.ascontiguousarray(a)).to("cuda")


def _u16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(
        "cuda").view(torch.uint16)


def _bits(x):
    import torch
    return x.view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def _kernel(k, rng):
    """A non-negative float32 kernel of sum 1 (to float32 rounding): a Gaussian
    of sigma 0.8 with uneven taps, one of them exactly 0."""
    K = bl.gaussian_kernel(k, 0.8).astype(np.float64) * rng.uniform(
        0.5, 1.5, (k, k))
    K[0, k - 1] = 0.0
    return bl.normalised(K)


@functools.lru_cache(maxsize=None)
def _inputs(nframe, det, k):
    """Detector-like stored intensities, a kernel, Poisson counts of the
    blurred model (uint16 saturates at 65535, as a detector's counter does), a
    signed upstream; and, per noise model and mask, everything the float64
    model says about them.  Computed once and left unchanged."""
    rng = np.random.default_rng(1000 * det + 10 * k + nframe)
    I32 = bl.detector_intensity(nframe, det, rng)
    K = _kernel(k, rng)
    Im = bl.blur(K, I32)
    counts = rng.poisson(Im).astype(np.float64)
    up = ac.frame_weights(nframe, seed=det)
    mask = fs.block_mask(det)
    # the float32 I_model: the entry's own order, taps ascending u then v
    Im32 = np.zeros_like(I32)
    r = k // 2
    for u in range(k):
        for v in range(k):
            Im32 = Im32 + K[u, v] * np.roll(I32, (u - r, v - r), axis=(-2, -1))
    assert Im32.dtype == np.float32
    out = dict(I32=I32, K=K, Im=Im, Im32=Im32, counts=counts, up=up, mask=mask)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(nframe, det, k, model, masked, u16):
    P = _inputs(nframe, det, k)
    mask = P["mask"] if masked else None
    n = bl.num_measured(mask, det)
    d = np.minimum(P["counts"], 65535) if u16 else P["counts"].astype(
        np.float32).astype(np.float64)
    sel = np.ones((det, det), bool) if mask is None else mask
    Im, K = P["Im"], P["K"]
    up = P["up"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (np.sqrt(d) / (np.sqrt(Im) + 1e-9) if model == "gaussian" else
             d / (Im + 1e-9))
    lp = np.where(sel, 1 - q, 0.0)
    scale = np.where(sel, np.abs(1 - q) + q, 0.0) * np.abs(up)[:, None, None] / n
    g = lp * up[:, None, None] / n
    cost, cabs = nm_.costs(MODEL_ID[model], Im, d, mask)
    c4 = nm_.costs_float32(MODEL_ID[model], P["Im32"], d, mask)
    return dict(d=d, mask=mask, n=n, sel=sel, lp=lp, scale=scale, g=g,
                table=bl.correlate(K, g), table_scale=bl.correlate(K, scale),
                costs=cost, costs_abs=cabs, costs_float32=c4,
                reach=bl.correlate(np.ones((k, k)), sel.astype(np.float64)))


def _data_d(R, masked, u16):
    if u16:
        junk = R["d"].astype(np.uint16)
        if masked:
            junk[:, ~R["mask"]] = 65535  # no NaN in uint16: must not count
        return _u16(junk)
    d = R["d"].astype(np.float32)
    return _dev(fs.masked(d, R["mask"]) if masked else d)


def _cost_factor(I_d, K_d, data_d, u16, mask_d, up_d, costs, table, blurred,
                 nframe, det, model, n):
    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    check(lib.tike_blur_cost_factor(
        A.ptr(I_d), A.ptr(K_d), int(K_d.shape[-1]), A.ptr(data_d), int(u16),
        A.ptr(mask_d), A.ptr(up_d), A.ptr(costs), A.ptr(table),
        A.ptr(blurred), nframe, det, MODEL_ID[model], n, A.stream_ptr()),
        "tike_blur_cost_factor")


# (nframe, det, k): the halo covers the plane almost twice; det not a multiple
# of 4; one tile exactly; a tile and a sliver (33 = 32 + 1); several tiles
FACTOR_CASES = [(3, 5, 5), (2, 8, 7), (1, 16, 3), (2, 33, 5), (1, 64, 7),
                (2, 128, 5)]


@pytest.mark.parametrize("model,masked,u16", VARIANTS)
@pytest.mark.parametrize("nframe,det,k", FACTOR_CASES)
def test_blur_cost_factor(nframe, det, k, model, masked, u16):
    """Entry by entry against the float64 model on detector-like frames:
      table    |err| <= (2 k^2 + 6) u  K (star) [mask (|l'| + q) |up| / n],
               q = sqrt(d) / (sqrt(I_model) + 1e-9) or d / (I_model + 1e-9):
               the first-order float32 error of a k^2-term sum of
               non-negatives, the factor, and a k^2-term signed sum
      blurred  (k^2 + 1) u relative
      costs    the bound of noise_models.reference: 1e-5 of the mean |term|
               plus 4 x the distance of the float32 restatement -- here at the
               float32 I_model formed in the entry's tap order --, widened by
               (k^2 + 1) u of the mean |term|
    The table is exactly 0 where no measured pixel lies within r; two calls
    give the same bits; each output alone equals what all three give; nothing
    in front of or behind an output is written."""
    import torch
    P = _inputs(nframe, det, k)
    R = _reference(nframe, det, k, model, masked, u16)
    I_d, K_d, up_d = _dev(P["I32"]), _dev(P["K"]), _dev(P["up"])
    mask_d = _dev(R["mask"].astype(np.uint8)) if masked else None
    data_d = _data_d(R, masked, u16)

    def run(which):
        costs = torch.full((nframe + 2,), 7.0, device="cuda")
        table = torch.full((nframe + 2, det, det), 7.0, device="cuda")
        blurred = torch.full((nframe + 2, det, det), 7.0, device="cuda")
        _cost_factor(I_d, K_d, data_d, u16, mask_d, up_d,
                     costs[1:] if "c" in which else None,
                     table[1:] if "t" in which else None,
                     blurred[1:] if "b" in which else None, nframe, det, model,
                     R["n"])
        for o in (costs, table, blurred):
            assert bool((o[0] == 7.0).all()) and bool((o[-1] == 7.0).all())
        return costs[1:-1], table[1:-1], blurred[1:-1]

    first, again = run("ctb"), run("ctb")
    for a, b in zip(first, again):
        assert torch.equal(_bits(a), _bits(b))
    for i, which in enumerate("ctb"):
        alone = run(which)
        assert torch.equal(_bits(alone[i]), _bits(first[i])), which
        for j in range(3):
            assert j == i or bool((alone[j] == 7.0).all())
    assert np.array_equal(I_d.cpu().numpy(), P["I32"])
    costs, table, blurred = (x.cpu().numpy().astype(np.float64) for x in first)
    assert all(np.all(np.isfinite(x)) for x in (costs, table, blurred))
    berr = np.max(np.abs(blurred - P["Im"]) / P["Im"]) / U
    tratio = np.abs(table - R["table"]) / np.where(
        R["table_scale"] > 0, (2 * k * k + 6) * U * R["table_scale"], 1.0)
    cbound = ((1e-5 + (k * k + 1) * U) * R["costs_abs"]
              + 4 * np.abs(R["costs_float32"] - R["costs"]))
    cratio = np.abs(costs - R["costs"]) / cbound
    dark = R["reach"] == 0
    print(f"blur cost factor {(nframe, det, k)} {model} masked={masked} "
          f"u16={u16}: table max |err| / bound {tratio.max():.3f}, blurred "
          f"{berr:.2f} u, costs |err| / bound {cratio.max():.3f}, "
          f"{int(dark.sum())} pixels out of reach")
    assert np.all(table[:, dark] == 0.0)
    assert np.all(table[:, R["table_scale"][0] == 0] == 0.0)
    assert berr <= k * k + 1
    assert np.all(tratio <= 1.0), tratio.max()
    assert np.all(cratio <= 1.0), cratio.max()
    # blurred alone needs no counts
    only = torch.full((nframe, det, det), 7.0, device="cuda")
    _cost_factor(I_d, K_d, None, 0, None, None, None, None, only, nframe, det,
                 model, R["n"])
    assert torch.equal(_bits(only), _bits(first[2]))


@pytest.mark.parametrize("model,masked,u16", VARIANTS)
def test_delta_kernel_is_tike_cost_factor(model, masked, u16):
    """k = 3 with K the delta on the intensities of a far plane: I_model is I
    exactly, so table and costs are tike_cost_factor's on that far plane to
    that entry's own bounds (test_autograd_cost_gpu.py: 1e-6 of |upstream_f|
    (1 + q) / n per table entry, 1e-6 of the terms' absolute parts per cost)
    -- and the table, which sums one product and zeros, has its bits."""
    import torch

    import test_autograd_cost_gpu as tc
    nframe, P_, npix = 2, 3, 33 * 33
    det = 33
    far, _, data, mask, upstream = tc._entry_inputs(nframe, P_, npix, masked,
                                                    u16)
    n = npix if mask is None else int(mask.sum())
    far_d, up_d = _dev(far), _dev(upstream)
    data_d = _u16(data) if u16 else _dev(data)
    mask_d = None if mask is None else _dev(mask.astype(np.uint8))
    want_c = torch.empty(nframe, device="cuda")
    want_t = torch.empty((nframe, npix), device="cuda")
    tc._launch_factor(far_d, data_d, u16, mask_d, up_d, want_c, want_t, nframe,
                      P_, npix, model, n)
    I_d = _dev(tc._intensity32(far_d, nframe, P_, npix))
    costs = torch.empty(nframe, device="cuda")
    table = torch.empty((nframe, det, det), device="cuda")
    _cost_factor(I_d, _dev(bl.delta_kernel(3)), data_d, u16, mask_d, up_d,
                 costs, table, None, nframe, det, model, n)
    assert torch.equal(_bits(table.view(nframe, npix)), _bits(want_t))
    I32 = I_d.cpu().numpy()
    sel = np.ones(npix, bool) if mask is None else mask
    clean = np.where(sel, data, 0).astype(np.float64)
    parts = I32 + clean * (1 if model == "gaussian" else
                           np.abs(np.log(I32.astype(np.float64) + 1e-9)))
    err = np.abs(costs.cpu().numpy().astype(np.float64)
                 - want_c.cpu().numpy()) / (parts[:, sel].sum(axis=1) / n)
    print(f"delta kernel {model} masked={masked} u16={u16}: table bits equal, "
          f"costs |diff| / sum parts {err.max():.2e}")
    assert np.all(err <= 1e-6), err


def test_blur_entries_refuse_bad_arguments():
    """TIKE_ERR_ARG by case, and 0 without a launch for no frames."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import ERR_ARG, lib
    det, k, nframe = 8, 3, 2
    I = torch.ones((nframe, det, det), device="cuda")
    K = _dev(bl.delta_kernel(7))
    d = torch.ones((nframe, det, det), device="cuda")
    out = torch.full((nframe, det, det), 7.0, device="cuda")
    st = A.stream_ptr()

    def cf(intensity=I, kernel=K, k=k, data=d, table=out, det=det, model=0,
           n=64, nframe=nframe):
        return lib.tike_blur_cost_factor(
            A.ptr(intensity), A.ptr(kernel), k, A.ptr(data), 0, None, None,
            None, A.ptr(table), None, nframe, det, model, n, st)

    assert cf() == 0
    for bad in (dict(intensity=None), dict(kernel=None), dict(k=4), dict(k=9),
                dict(k=1), dict(det=2), dict(k=7, det=6), dict(n=0),
                dict(model=2), dict(data=None), dict(nframe=-1)):
        assert cf(**bad) == ERR_ARG, bad
    out.fill_(7.0)
    assert cf(nframe=0) == 0 and bool((out == 7.0).all())
    npart = lib.tike_blur_kernel_sums_partials(det, k)
    assert npart > 0 and npart % (1 + k * k) == 0
    for args in ((det, 4), (2, 3), (6, 7), (0, 3)):
        assert lib.tike_blur_kernel_sums_partials(*args) == 0, args
    parts = torch.full((npart,), 7.0, dtype=torch.float64, device="cuda")
    kg = torch.full((k, k), 7.0, dtype=torch.float64, device="cuda")

    def ks(intensity=I, kernel=K, k=k, data=d, partials=parts, det=det,
           model=0, n=64, nframe=nframe):
        return lib.tike_blur_kernel_sums(
            A.ptr(intensity), A.ptr(kernel), k, A.ptr(data), 0, None, None,
            A.ptr(partials), A.ptr(kg), nframe, det, model, n, st)

    assert ks() == 0
    for bad in (dict(intensity=None), dict(kernel=None), dict(k=4),
                dict(det=2), dict(n=0), dict(model=-1), dict(data=None),
                dict(partials=None), dict(nframe=-1)):
        assert ks(**bad) == ERR_ARG, bad
    parts.fill_(7.0), kg.fill_(7.0)
    assert ks(nframe=0) == 0
    assert bool((parts == 7.0).all()) and bool((kg == 7.0).all())


# --------------------------------------------------------- the kernel's sums
def _kernel_sums(I_d, K_d, data_d, u16, mask_d, up_d, want_kgrad, nframe, det,
                 model, n):
    """(cost = the cost partials added in order on the host, kgrad (k, k)
    float64 or None, the raw buffers)."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    k = int(K_d.shape[-1])
    npart = lib.tike_blur_kernel_sums_partials(det, k)
    assert npart > 0
    partials = torch.full((npart + 2,), 7.0, dtype=torch.float64,
                          device="cuda")
    kgrad = torch.full((k * k + 2,), 7.0, dtype=torch.float64, device="cuda")
    check(lib.tike_blur_kernel_sums(
        A.ptr(I_d), A.ptr(K_d), k, A.ptr(data_d), int(u16), A.ptr(mask_d),
        A.ptr(up_d), A.ptr(partials[1:]),
        A.ptr(kgrad[1:]) if want_kgrad else None, nframe, det,
        MODEL_ID[model], n, A.stream_ptr()), "tike_blur_kernel_sums")
    assert float(partials[0]) == 7.0 == float(partials[-1])
    assert float(kgrad[0]) == 7.0 == float(kgrad[-1])
    ncost = npart // (1 + k * k)
    cost = 0.0
    for p in partials[1:1 + ncost].cpu().numpy():
        cost += float(p)
    return cost, kgrad[1:-1].view(k, k), partials


# (nframe, det, k): one frame (three empty frame ranges), one tile; 16 = one
# tile exactly; a tile and a sliver in both directions, k = 7; many frames
SUMS_CASES = [(1, 13, 3), (5, 16, 5), (37, 33, 7), (300, 20, 5)]


def _cost_bound(P, R, model, k, up):
    """1e-6 of the terms' absolute parts (the bar of tike_background_sums'
    partials) + the float32 I_model's (k^2 + 1) u carried through the term to
    first order, |l'| I_model."""
    Im, d, sel, n = P["Im"], R["d"], R["sel"], R["n"]
    clean = np.where(sel, d, 0.0)
    parts = Im + clean * (1 if model == "gaussian" else
                          np.abs(np.log(Im + 1e-9)))
    w = np.abs(up)[:, None, None]
    return (1e-6 * (w * parts)[:, sel].sum() / n
            + (k * k + 1) * U * (w * np.abs(R["lp"]) * Im)[:, sel].sum() / n)


@pytest.mark.parametrize("model,masked,u16", VARIANTS)
@pytest.mark.parametrize("nframe,det,k", SUMS_CASES)
def test_blur_kernel_sums(nframe, det, k, model, masked, u16):
    """kgrad against the model: |err[u, v]| <= (k^2 + 7) u sum_f sum_p mask
    (|l'| + q) |up_f| / n  I[p - (u - r, v - r)] -- the float32 factor (its
    k^2-term I_model, six roundings of its own) times the intensity, one more
    rounding, summed in float64.  The cost partials added in order against the
    model's sum_f up_f cost_f (`_cost_bound`).  Without kgrad the partials
    have the same bits; NULL upstream equals ones; two calls give the same
    bits."""
    import torch
    P = _inputs(nframe, det, k)
    R = _reference(nframe, det, k, model, masked, u16)
    I_d, K_d, up_d = _dev(P["I32"]), _dev(P["K"]), _dev(P["up"])
    mask_d = _dev(R["mask"].astype(np.uint8)) if masked else None
    data_d = _data_d(R, masked, u16)
    args = (nframe, det, model, R["n"])
    cost, kgrad, raw = _kernel_sums(I_d, K_d, data_d, u16, mask_d, up_d, True,
                                    *args)
    cost2, kgrad2, raw2 = _kernel_sums(I_d, K_d, data_d, u16, mask_d, up_d,
                                       True, *args)
    assert torch.equal(_bits(raw), _bits(raw2))
    assert torch.equal(_bits(kgrad), _bits(kgrad2))
    cost3, _, raw3 = _kernel_sums(I_d, K_d, data_d, u16, mask_d, up_d, False,
                                  *args)
    ncost = (raw.numel() - 2) // (1 + k * k)
    assert torch.equal(_bits(raw3[1:1 + ncost]), _bits(raw[1:1 + ncost]))
    ones = _kernel_sums(I_d, K_d, data_d, u16, mask_d,
                        torch.ones(nframe, device="cuda"), True, *args)
    null = _kernel_sums(I_d, K_d, data_d, u16, mask_d, None, True, *args)
    assert torch.equal(_bits(ones[1]), _bits(null[1])) and ones[0] == null[0]
    up = P["up"].astype(np.float64)
    want = bl.kgrad(model, R["d"], P["I32"], P["K"], R["mask"], up)
    want_cost = float(np.sum(up * R["costs"]))
    bound = np.zeros((k, k))
    r = k // 2
    I64 = P["I32"].astype(np.float64)
    for u in range(k):
        for v in range(k):
            bound[u, v] = (k * k + 7) * U * np.sum(
                R["scale"] * np.roll(I64, (u - r, v - r), axis=(-2, -1)))
    kratio = np.abs(kgrad.cpu().numpy() - want) / bound
    cratio = abs(cost - want_cost) / _cost_bound(P, R, model, k, up)
    print(f"blur kernel sums {(nframe, det, k)} {model} masked={masked} "
          f"u16={u16}: kgrad max |err| / bound {kratio.max():.3f}, cost "
          f"|err| / bound {cratio:.3f}")
    assert np.all(np.isfinite(kgrad.cpu().numpy())) and np.isfinite(cost)
    assert np.all(kratio <= 1.0), kratio
    assert cratio <= 1.0, cratio


@pytest.mark.parametrize("model", ["gaussian", "poisson"])
@pytest.mark.parametrize("nframe,det,k", SUMS_CASES[1:3])
def test_blur_kernel_sums_predict_the_line(nframe, det, k, model):
    """From a kernel that is not the data's (its root times uniform(0.7, 1.3))
    along a + t dir, dir the descent direction of the chain through K = a^2 /
    sum a^2, the entry's cost falls by what its kgrad predicts:
    |c(t) - c(0) - t <grad_a, dir>| stays within twice the float64 model's own
    second-order remainder plus the two costs' rounding bounds.  t is halved
    from 1e-2, in the model alone, until that remainder is a tenth of the
    first-order fall."""
    P = _inputs(nframe, det, k)
    R = _reference(nframe, det, k, model, True, False)
    I_d = _dev(P["I32"])
    mask_d = _dev(R["mask"].astype(np.uint8))
    data_d = _data_d(R, True, False)
    n = R["n"]
    a0 = np.sqrt(P["K"].astype(np.float64)) * np.random.default_rng(
        k).uniform(0.7, 1.3, (k, k))

    def device(a, want_kgrad):
        K = bl.kernel_of(a).astype(np.float32)
        c, g, _ = _kernel_sums(I_d, _dev(K), data_d, False, mask_d, None,
                               want_kgrad, nframe, det, model, n)
        return c, (g.cpu().numpy() if want_kgrad else None), K

    def model64(K):
        return nframe * bl.cost_from_intensity(model, R["d"], P["I32"], K,
                                               R["mask"])

    K0 = bl.kernel_of(a0).astype(np.float32)
    ga64 = bl.grad_a(a0, bl.kgrad(model, R["d"], P["I32"], K0, R["mask"]))
    dir_ = -ga64 / np.linalg.norm(ga64)
    slope64 = float(np.sum(ga64 * dir_))
    m0, t = model64(K0), 2e-2
    while True:
        t *= 0.5
        K1 = bl.kernel_of(a0 + t * dir_).astype(np.float32)
        remainder = abs(model64(K1) - m0 - t * slope64)
        if remainder <= 0.1 * abs(t * slope64):
            break
    c0, g0, _ = device(a0, True)
    c1, _, _ = device(a0 + t * dir_, False)
    slope = float(np.sum(bl.grad_a(a0, g0) * dir_))
    # what the two costs may be off by: their own bounds, and the kernels
    # reach the device rounded to float32, u |g K| at either end
    at = dict(R, lp=np.where(R["sel"], bl.factor(
        model, R["d"], P["I32"], K0, R["mask"]) * n, 0.0))
    rounding = (2 * _cost_bound(dict(P, Im=bl.blur(K0, P["I32"])), at, model,
                                k, np.ones(nframe))
                + 2 * U * float(np.sum(np.abs(g0 * K0))))
    miss = abs(c1 - c0 - t * slope)
    print(f"line {(nframe, det, k)} {model}: t {t:.2e} c(0) {c0:.6e} c(t) "
          f"{c1:.6e} t slope {t * slope:.3e} (model {t * slope64:.3e}); miss "
          f"{miss:.3e}, model remainder {remainder:.3e}, rounding "
          f"{rounding:.3e}")
    assert slope < 0 and c1 < c0
    assert miss <= 2 * remainder + rounding


# ------------------------------------------------------------------ the solver
RECON_NORMWISE = 1e-3  # the project's reconstruction bar


@pytest.fixture(scope="module")
def tp():
    import tike_amd.ptycho as m
    return m


def _parameters(tp, P, model, mask, **kw):
    from test_background_gpu import _parameters as parameters
    return parameters(tp, P, model, mask,
                      **dict(dict(step_length=bl.STEP_LENGTH), **kw))


def _reconstruct(tp, P, data, params, fly, bo):
    N = len(P["scan"])
    return tp.reconstruct(data, params, fly=fly, order=np.arange(N),
                          batches=[np.arange(N)], blur_options=bo)


@pytest.mark.parametrize("model,use_mask,update", bl.SOLVER_VARIANTS)
@pytest.mark.parametrize("case", sorted(bl.SOLVER_CASES))
def test_cgrad_vs_float64_model(tp, case, model, use_mask, update):
    """Two epochs of cgrad with blur_options, cg_iter 2, det 32, fly 1 and 2,
    from the first guess 0.52 / 0.02 of a Gaussian kernel of sigma 0.8: psi,
    probe, the kernel left in the options and the cost history against the
    model's three-block cgrad at RECON_NORMWISE; every line-search decision of
    the model is clear (test_blur_cpu.py)."""
    state, P, mask = bl.run_model(case, model, use_mask, update)
    fly = bl.SOLVER_CASES[case]["fly"]
    bo = tp.BlurOptions(P["k0"].copy(), update=update)
    got = _reconstruct(tp, P, P["data"], _parameters(tp, P, model, mask), fly,
                       bo)
    costs = np.array(got.algorithm_options.costs)
    want_k = bl.kernel_of(state["a"])
    print(case, model, use_mask, update,
          f"psi {relerr(got.psi, state['psi']):.2e} probe "
          f"{relerr(got.probe, state['probe']):.2e} kernel "
          f"{relerr(bo.kernel, want_k):.2e} costs", np.ravel(costs), "vs",
          np.ravel(state["costs"]))
    np.testing.assert_allclose(costs, np.array(state["costs"]),
                               rtol=RECON_NORMWISE)
    assert relerr(got.psi, state["psi"]) <= RECON_NORMWISE
    assert relerr(got.probe, state["probe"]) <= RECON_NORMWISE
    assert isinstance(bo.kernel, np.ndarray) and bo.kernel.shape == (5, 5)
    assert bo.kernel.dtype == np.float32 and np.all(bo.kernel >= 0)
    assert abs(float(bo.kernel.sum(dtype=np.float64)) - 1) <= 1e-6
    assert relerr(bo.kernel, want_k) <= RECON_NORMWISE
    if not update:
        np.testing.assert_allclose(bo.kernel, bl.normalised(P["k0"]),
                                   rtol=1e-6)


@pytest.mark.parametrize("fly", [1, 2])
def test_cgrad_delta_kernel_is_the_whole_frames_route(tp, fly, monkeypatch):
    """blur_options with the delta kernel and update=False gives the iterates
    of the same call without it on the whole-frames route
    (`_fly_cost_and_grad`; at fly 1 the call without blur_options takes the
    plain route, whose line searches the device decides: it is sent the
    whole-frames way here), to 1e-5 normwise."""
    import importlib
    cg = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    P = bl.solver_problem(f"fly{fly}")
    mask = fs.block_mask(32)
    data = fs.masked(P["data"], mask)
    bo = tp.BlurOptions(bl.delta_kernel(3), update=False)
    with_bo = _reconstruct(tp, P, data, _parameters(tp, P, "gaussian", mask),
                           fly, bo)
    assert np.array_equal(bo.kernel, bl.delta_kernel(3))
    if fly == 1:
        # the route a plain minibatch would not take
        monkeypatch.setattr(cg, "PLAIN_ROUTE", False)
    without = _reconstruct(tp, P, data, _parameters(tp, P, "gaussian", mask),
                           fly, None)
    print(f"fly {fly}: psi {relerr(with_bo.psi, without.psi):.2e} probe "
          f"{relerr(with_bo.probe, without.probe):.2e}")
    assert relerr(with_bo.psi, without.psi) <= 1e-5
    assert relerr(with_bo.probe, without.probe) <= 1e-5
    np.testing.assert_allclose(with_bo.algorithm_options.costs,
                               without.algorithm_options.costs, rtol=1e-5)


def test_operator_and_simulate(tp):
    """simulate(blur=) blurs every frame (and normalises the kernel);
    Ptycho.cost and _compute_intensity with a blur against the model."""
    import tike_amd.operators as tops
    kw = bl.SOLVER_CASES["fly2"]
    P = bl.solver_problem("fly2")
    det, fly = kw["det"], kw["fly"]
    K = P["kernel"]
    sim = tp.simulate(det, P["probe"], P["scan"], P["psi"], fly=fly,
                      blur=3 * K)
    assert_close(sim, P["data"], what="simulate(blur=)")
    plain = tp.simulate(det, P["probe"], P["scan"], P["psi"], fly=fly)
    assert_close(sim, bl.blur(K, plain), what="blur of simulate")
    with tops.Ptycho(det, kw["pw"], nz=kw["obj"], n=kw["obj"]) as op:
        inten, _ = op._compute_intensity(None, P["psi0"], P["scan"],
                                         P["probe0"], fly=fly, blur=K)
        assert_close(inten, bl.intensity(P["probe0"], P["scan"], P["psi0"],
                                         det, fly, K), what="K (*) intensity")
        for model in ("gaussian", "poisson"):
            c = float(op.cost(P["data"], P["psi0"], P["scan"], P["probe0"],
                              model=model, fly=fly, blur=K))
            want = bl.cost(model, P["data"], P["psi0"], P["scan"],
                           P["probe0"], det, fly, None, K)
            print(f"Ptycho.cost(blur=) {model}: {c:.7e} vs {want:.7e}")
            assert abs(c - want) <= OP_NORMWISE * abs(want), (model, c, want)


# --------------------------------------------------------- autograd.cost(blur=)
AUTOGRAD_CASES = ([(kind, shape, model, masked)
                   for kind, shape in ac.CASES[:2]
                   for model in ac.MODELS for masked in (False, True)]
                  + [("eigen", ac.EIGEN_CASES[1], "poisson", True),
                     ("multislice", ac.MULTISLICE_CASES[0], "gaussian", True)])


@pytest.mark.parametrize("kind,shape,model,masked", AUTOGRAD_CASES)
def test_autograd_cost_blur(kind, shape, model, masked):
    """costs and the gradients with respect to every input of the form and to
    K against the float64 model -- the form's intensity, tests/blur.py's table
    through the form's hand-written backward, its kgrad -- at the bars of
    test_autograd_cost_gpu.py; K.grad entry by entry within 2e-5 of
    sum_f sum_p mask (|l'| + q) |up_f| / n I[p - shift], the sum of the
    absolute values of what it adds up (the float32 forward's intensity is
    off by OP_NORMWISE, in the factor and in the intensity it multiplies).
    Two plain shapes (fly 2 at det 16; det 64), both models, masked and not;
    eigen probes and several slices at one shape each.  K alone gives the same
    K.grad."""
    import torch

    import test_autograd_cost_gpu as tc
    from tike_amd import autograd
    c = ac.case(kind, shape)
    data, mask, up, kw, _ = tc._inputs(c, masked)
    form, det = c["form"], c["det"]
    K = bl.gaussian_kernel(5, 0.8) * np.random.default_rng(3).uniform(
        0.6, 1.4, (5, 5)).astype(np.float32)
    K = bl.normalised(K)
    up64 = up.astype(np.float64)
    with torch.no_grad():
        I = form.intensity(c["m"]).numpy()
        want_costs = bl.cost_each(model, data, I, K, mask)
        want = form.grads(c["m"], torch.from_numpy(
            bl.table(model, data, I, K, mask, up64)))
    want_k = bl.kgrad(model, data, I, K, mask, up64)
    Im = bl.blur(K, I)
    sel = np.ones((det, det), bool) if mask is None else mask
    d = np.where(sel, np.nan_to_num(data), 0.0).astype(np.float64)
    q = (np.sqrt(d) / (np.sqrt(Im) + 1e-9) if model == "gaussian" else
         d / (Im + 1e-9))
    scale = np.where(sel, np.abs(1 - q) + q, 0.0) * np.abs(
        up64)[:, None, None] / bl.num_measured(mask, det)
    k_scale = np.array([[np.sum(scale * np.roll(I, (u - 2, v - 2),
                                                axis=(-2, -1)))
                         for v in range(5)] for u in range(5)])
    names = [k for k in form.names if kw.get(k) is not None]
    K_d = _dev(K).requires_grad_(True)
    data_d, up_d = _dev(data), _dev(up)
    rest = {k: v for k, v in kw.items() if k not in ("psi", "probe", "scan")}
    with tc._operator(c) as op:
        args = (op, data_d, kw["psi"], kw["probe"], kw["scan"])
        costs = autograd.cost(*args, model=model, blur=K_d, **rest)
        grads = torch.autograd.grad((costs * up_d).sum(),
                                    [kw[k] for k in names] + [K_d])
        detached = {k: (v.detach() if isinstance(v, torch.Tensor) else v)
                    for k, v in kw.items()}
        alone = torch.autograd.grad((autograd.cost(
            op, data_d, detached["psi"], detached["probe"], detached["scan"],
            model=model, blur=K_d,
            **{k: v for k, v in detached.items()
               if k not in ("psi", "probe", "scan")}) * up_d).sum(), [K_d])[0]
    costs = tc._host(costs)
    got = {k: tc._host(g) for k, g in zip(names, grads)}
    got_k = tc._host(grads[-1])
    cerr = np.abs(costs - want_costs) / np.abs(want_costs)
    kerr = np.abs(got_k - want_k) / k_scale
    what = f"cost(blur=) {kind} {shape} {model} masked={masked}"
    print(f"{what}: costs max rel {cerr.max():.2e}; K.grad max |err| / sum "
          f"|terms| {kerr.max():.2e} (normwise {relerr(got_k, want_k):.2e})")
    assert np.all(np.isfinite(costs)) and np.all(cerr <= 1e-5), cerr
    tc._assert_grads(tc._grad_errors(got, want, form.names),
                     what + " gradients")
    assert got_k.dtype == np.float32 and np.all(np.isfinite(got_k))
    assert np.all(kerr <= 2e-5), kerr
    assert torch.equal(alone, grads[-1])


# ------------------------------------------------------------- demonstration
def test_demonstration(tp):
    """The background demonstration's geometry, its counts blurred by a
    Gaussian of sigma 0.8 on 5 x 5 taps; six epochs, one mode, the probe
    known.  With the true kernel fixed the object error falls below the error
    without a blur by the ratio the float64 model reaches (0.4442 / 0.7047,
    test_blur_cpu.py), that ratio given 20 % slack; the fit from 0.52 / 0.02
    (L1 distance 1.010 to the true kernel) ends within 1.5 x the model's
    distance (0.0303)."""
    D = bl.DEMO
    P = bl.demo_problem()
    pw = D["problem"]["pw"]
    err, l1 = {}, None
    for how in ("none", "true", "fit"):
        bo = None
        if how != "none":
            bo = tp.BlurOptions((P["kernel"] if how == "true" else
                                 P["k0"]).copy(), update=how == "fit")
        params = _parameters(tp, P, "gaussian", None, epochs=D["epochs"],
                             cg_iter=D["cg_iter"], recover_probe=False,
                             step_length=1.0, probe=P["probe"])
        got = _reconstruct(tp, P, P["data"], params, 1, bo)
        err[how] = bl.bg.object_error(got.psi, P["psi"], P["scan"], pw)
        if how == "fit":
            l1 = float(np.abs(bo.kernel - P["kernel"]).sum())
    model = {how: bl.run_demo(how) for how in ("none", "true", "fit")}
    l1_model = float(np.abs(bl.kernel_of(model["fit"][1]["a"])
                            - P["kernel"]).sum())
    print("demonstration: object error without a blur "
          f"{err['none']:.4f} (model {model['none'][0]:.4f}), true kernel "
          f"{err['true']:.4f} ({model['true'][0]:.4f}), fitted "
          f"{err['fit']:.4f} ({model['fit'][0]:.4f}); L1 distance of the "
          f"fitted kernel {l1:.4f} (model {l1_model:.4f})")
    assert err["true"] / err["none"] <= 1.2 * (model["true"][0]
                                               / model["none"][0])
    assert l1 <= 1.5 * l1_model
