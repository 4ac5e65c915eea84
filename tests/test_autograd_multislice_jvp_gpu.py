"""The forward-mode derivative of `tike_amd.autograd.multislice_intensity` on
the GPU against the float64 model (tests/autograd_multislice_jvp.py): the new
entry on its own, `multislice_intensity_jvp` end to end on both routes, one
slice, the routes' switches, chunks and strided inputs, the adjoint identity
between the forward and the reverse mode, `multislice_gauss_newton_product`,
and Levenberg-Marquardt position recovery on a two-slice object.

Every figure a bar is set on is printed before it is asserted."""
import functools
import importlib

import numpy as np
import pytest

import autograd_jvp as aj
import autograd_model as am
import autograd_multislice as mm
import autograd_multislice_jvp as mj
from util import OP_MAXABS, OP_NORMWISE, assert_close, maxerr, relerr

pytestmark = pytest.mark.gpu

GENERAL = (6, 2, 32, 72, 2, 1)
FUSED = (6, 2, 128, 170, 2, 2)
assert GENERAL in mm.END_TO_END_CASES and FUSED in mm.END_TO_END_CASES


# ------------------------------------------- entry: tike_slice_wave_tangent
# (nscan, S, pw, H, W): narrower than one item of 8 rows x 64 columns; exactly
# one column segment; two segments with a ragged second one and rows that are
# no multiple of the strip; S at its limit; three segments, the last of two
# columns
ENTRY_CASES = [(5, 1, 15, 40, 40), (6, 3, 64, 100, 104), (4, 2, 70, 110, 120),
               (3, 16, 16, 48, 50), (2, 1, 130, 200, 210)]
# (beam per position, dbeam: None / "shared" / "each", dpsi, dscan)
ENTRY_FORMS = [(True, "each", True, True), (False, "shared", True, True),
               (True, None, True, True), (False, "each", False, True),
               (True, "shared", True, False), (True, "each", False, False),
               (False, None, False, False)]
MARGIN = 8
GUARD = 256


def _entry_positions(rng, nscan, pw, H, W):
    """Position 0 hangs over the top and the left edge of the object
    (negative coordinates), position 1 over the bottom and the right edge;
    position 2, if any, has an exactly integer first coordinate; the others
    anywhere allowed.  Every other fraction lies in [0.05, 0.95]."""
    frac = lambda *s: 0.05 + 0.9 * rng.random(s)
    scan = np.stack([rng.integers(1, H - pw, nscan) + frac(nscan),
                     rng.integers(1, W - pw, nscan) + frac(nscan)], 1)
    scan[0] = (-3 + frac(), -2 + frac())
    scan[1] = (H - pw + 2 + frac(), W - pw + 1 + frac())
    if nscan > 2:
        scan[2] = (1.0, 1 + frac())
    scan = scan.astype(np.float32)
    corner = np.floor(scan)
    assert corner[0].max() < 0 and corner[0].min() >= -MARGIN
    assert corner[1, 0] + pw > H and corner[1, 1] + pw > W
    assert corner[1, 0] + pw + 1 <= H + MARGIN
    assert corner[1, 1] + pw + 1 <= W + MARGIN
    return scan


def _framed(layer):
    """(1, H + 2 MARGIN, W + 2 MARGIN) complex128: a tap outside the object
    counts as zero (the positions move along)."""
    import torch
    H, W = layer.shape
    out = np.zeros((1, H + 2 * MARGIN, W + 2 * MARGIN), np.complex128)
    out[0, MARGIN:-MARGIN, MARGIN:-MARGIN] = layer
    return torch.from_numpy(out)


@pytest.mark.parametrize("nscan,S,pw,H,W", ENTRY_CASES)
def test_slice_wave_tangent_vs_float64_model(nscan, S, pw, H, W):
    """de = dpatch beam + patch dbeam of one slice within the operator bars
    (normwise 1e-5, max-abs 1e-4 of the largest entry) of the float64 model
    for shared and per-position beams, dbeam NULL / shared / per position,
    dpsi NULL, dscan NULL; all three NULL: exactly zero; in place (dwave is
    dbeam) and a second call: the bits of the first; footprints that hang
    over every edge of the object; the sentinels in front of and behind the
    output untouched.  With shared operands: `tike_conv_fwd_tangent` at
    det == pw to 1e-6 normwise."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    rng = np.random.default_rng(nscan + S + pw)
    host = dict(psi=mm.rc(rng, H, W), dpsi=mm.rc(rng, H, W),
                scan=_entry_positions(rng, nscan, pw, H, W),
                dscan=rng.standard_normal((nscan, 2)).astype(np.float32),
                beam=mm.rc(rng, nscan, S, pw, pw),
                dbeam=mm.rc(rng, nscan, S, pw, pw))
    dev = torch.device("cuda")
    on = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    layer, dlayer = _framed(host["psi"]), _framed(host["dpsi"])
    moved = torch.from_numpy(host["scan"]).to(am.F64) + MARGIN
    count = nscan * S * pw * pw
    sentinel = complex(7e30, -7e30)
    big = torch.empty(count + 2 * GUARD, dtype=torch.complex64, device=dev)
    out = big[GUARD:GUARD + count]
    st = A.stream_ptr()

    def call(per, kind, dpsi, dscan, inplace=False):
        big.fill_(sentinel)
        beam = on["beam"] if per else on["beam"][:1].contiguous()
        dbeam = {None: None, "shared": on["dbeam"][:1].contiguous(),
                 "each": on["dbeam"]}[kind]
        if inplace:
            out.copy_(dbeam.reshape(-1))
            dbeam = out
        check(lib.tike_slice_wave_tangent(
            A.ptr(on["psi"]), A.ptr(on["dpsi"]) if dpsi else None,
            A.ptr(on["scan"]), A.ptr(on["dscan"]) if dscan else None,
            A.ptr(beam), int(per), A.ptr(dbeam), int(kind == "each"),
            A.ptr(out), nscan, S, pw, H, W, st), "tike_slice_wave_tangent")
        got = big.cpu().numpy()
        assert np.all(got[:GUARD] == np.complex64(sentinel))
        assert np.all(got[GUARD + count:] == np.complex64(sentinel))
        return got[GUARD:GUARD + count].reshape(nscan, S, pw, pw)

    for per, kind, dpsi, dscan in ENTRY_FORMS:
        form = (per, kind, dpsi, dscan)
        got = call(*form)
        assert np.array_equal(call(*form), got), form  # two calls
        if kind == "each":
            assert np.array_equal(call(*form, inplace=True), got), form
        if kind is None and not dpsi and not dscan:
            assert not got.any() and not np.signbit(got.real).any()
            continue
        f64 = lambda a, n: torch.from_numpy(a[:n]).to(am.C128)
        want = mj.slice_tangent(
            layer, moved, f64(host["beam"], nscan if per else 1),
            dlayer if dpsi else None,
            torch.from_numpy(host["dscan"]).to(am.F64) if dscan else None,
            None if kind is None else f64(host["dbeam"],
                                          nscan if kind == "each" else 1))[1]
        want = want.numpy()
        print(f"slice wave tangent ({nscan}, {S}, {pw}, {H}, {W}) {form}: "
              f"normwise {relerr(got, want):.2e} max-abs "
              f"{maxerr(got, want):.2e}")
        assert np.abs(want).max() > 0
        assert_close(got, want, OP_NORMWISE, OP_MAXABS, str(form))
        if not per and kind == "shared":
            old = torch.empty((nscan, S, pw, pw), dtype=torch.complex64,
                              device=dev)
            check(lib.tike_conv_fwd_tangent(
                A.ptr(on["psi"]), A.ptr(on["dpsi"]), A.ptr(on["scan"]),
                A.ptr(on["dscan"]), A.ptr(on["beam"][:1].contiguous()),
                A.ptr(on["dbeam"][:1].contiguous()), A.ptr(old), nscan, S, pw,
                pw, H, W, st), "tike_conv_fwd_tangent")
            e = relerr(got, old.cpu().numpy())
            print(f"    against tike_conv_fwd_tangent: {e:.2e}")
            assert e <= 1e-6


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _case(shape, norm="ortho"):
    """Host inputs, tangents and the float64 model's I and dI (all three
    tangents) -- computed once, shared, left unchanged."""
    c = mj.case(*shape, norm=norm)
    inten, tangent = mj.case_jvp(c)
    return dict(c, intensity=inten, tangent=tangent)


def _operator(c):
    import tike_amd.operators as ops
    pw, (H, W) = c["probe"].shape[-1], c["psi"].shape[-2:]
    return ops.Ptycho(probe_shape=pw, detector_shape=pw, nz=H, n=W,
                      norm=c["norm"], **mm.optics(pw))


def _device(c, *names):
    import torch
    return [torch.from_numpy(c[k]).to("cuda") for k in names]


def _run_jvp(c, names=mj.TANGENT_NAMES, view=lambda x: x):
    """(I, dI, I of `multislice_intensity`) as host arrays; view: what is
    made of every input before the call."""
    import torch

    from tike_amd.autograd import (multislice_intensity,
                                   multislice_intensity_jvp)
    psi, probe, scan = map(view, _device(c, "psi", "probe", "scan"))
    t = dict(zip(names, map(view, _device(c, *names))))
    fly = c["fly"]
    with _operator(c) as op:
        inten, tangent = multislice_intensity_jvp(op, psi, probe, scan,
                                                  fly=fly, **t)
        with torch.no_grad():
            plain = multislice_intensity(op, psi, probe, scan, fly=fly)
    N, pw = c["scan"].shape[0], c["probe"].shape[-1]
    for x in (inten, tangent):
        assert x.dtype == torch.float32 and not x.requires_grad
        assert tuple(x.shape) == (N // fly, pw, pw)
    return tuple(x.cpu().numpy() for x in (inten, tangent, plain))


def _assert_jvp(got, want, what):
    """want: (I, dI) of the model."""
    inten, tangent, plain = got
    print(f"{what}: dI normwise {relerr(tangent, want[1]):.2e} max-abs "
          f"{maxerr(tangent, want[1]):.2e}; I normwise "
          f"{relerr(inten, want[0]):.2e}")
    assert np.array_equal(inten, plain), what  # the bits of the forward
    assert_close(inten, want[0], OP_NORMWISE, OP_MAXABS, what + " I")
    assert np.abs(want[1]).max() > 0
    assert_close(tangent, want[1], OP_NORMWISE, OP_MAXABS, what + " dI")


@pytest.mark.parametrize(
    "shape,norm", [(s, "ortho") for s in mm.END_TO_END_CASES]
    + [(GENERAL, "backward"), (FUSED, "backward")])
def test_multislice_intensity_jvp_vs_model(shape, norm):
    """dI within the operator bars (normwise 1e-5, max-abs 1e-4) of the
    float64 `hand_jvp` with all three tangents (the float32 restatement on
    the CPU: 3.7e-7 - 6.8e-7); I bit-identical to
    `multislice_intensity(...)`."""
    c = _case(shape, norm)
    _assert_jvp(_run_jvp(c), (c["intensity"], c["tangent"]),
                f"{shape} {norm}")


@pytest.mark.parametrize("shape", [GENERAL, FUSED])
@pytest.mark.parametrize("name", mj.TANGENT_NAMES)
def test_each_tangent_alone(name, shape):
    c = _case(shape)
    _assert_jvp(_run_jvp(c, (name,)), mj.case_jvp(c, (name,)),
                f"{shape} {name} alone")


@pytest.mark.parametrize("shape", [GENERAL, FUSED])
def test_no_tangent_gives_zeros(shape):
    got = _run_jvp(_case(shape), names=())
    assert np.array_equal(got[0], got[2]) and not got[1].any()


def test_one_slice_gives_the_bits_of_intensity_jvp():
    import tike_amd.operators as ops
    from tike_amd.autograd import intensity_jvp
    c = mj.case(6, 2, 32, 72, 1, 2)
    got = _run_jvp(c)
    psi, probe, scan = _device(c, "psi", "probe", "scan")
    t = dict(zip(mj.TANGENT_NAMES, _device(c, *mj.TANGENT_NAMES)))
    with ops.Ptycho(probe_shape=32, detector_shape=32, nz=72, n=72) as op:
        want = intensity_jvp(op, psi, probe, scan, fly=2, **t)
    assert np.array_equal(got[0], want[0].cpu().numpy())
    assert np.array_equal(got[1], want[1].cpu().numpy())
    assert np.abs(got[1]).max() > 0


# ------------------------------------------------------------ routes and chunks
def test_routes_agree_at_128(monkeypatch):
    """The fused route against the general route (cgrad's MULTISLICE_FUSED
    off), the tangent's Fresnel step on the two-pass kernels, and slice 0 by
    `tike_conv_fwd_tangent`: each within the bars of the model and within
    1e-5 normwise of the default route; I keeps the bits of the forward on
    its route."""
    from tike_amd import autograd
    cgrad = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    c = _case(FUSED)
    want = (c["intensity"], c["tangent"])
    assert cgrad.MULTISLICE_FUSED
    fused = _run_jvp(c)
    _assert_jvp(fused, want, "fused")
    for name, (module, lever, value) in dict(
            general=(cgrad, "MULTISLICE_FUSED", False),
            two_pass_fresnel=(autograd, "TANGENT_FRESNEL_TWO_PASS",
                              not autograd.TANGENT_FRESNEL_TWO_PASS),
            first_slice=(autograd, "FIRST_SLICE_BY_CONV_TANGENT",
                         not autograd.FIRST_SLICE_BY_CONV_TANGENT)).items():
        with monkeypatch.context() as m:
            m.setattr(module, lever, value)
            other = _run_jvp(c)
        _assert_jvp(other, want, name)
        errs = [relerr(b, a) for a, b in zip(fused[:2], other[:2])]
        print(f"{name} against the default: "
              + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) <= 1e-5, (name, errs)


@pytest.mark.parametrize("shape", [(12, 2, 32, 72, 2, 2),
                                   (12, 2, 128, 170, 3, 2)])
def test_three_chunks(shape, monkeypatch):
    """The positions cut into three chunks of whole frames (5 positions:
    frames of two are kept whole, 4 + 4 + 4) give what one chunk gives, to
    1e-6."""
    from tike_amd.ptycho.solvers import lstsq
    c = _case(shape)
    whole = _run_jvp(c)
    monkeypatch.setattr(lstsq, "CHUNK_POSITIONS_OVERRIDE", 5)
    cut = _run_jvp(c)
    _assert_jvp(cut, (c["intensity"], c["tangent"]),
                f"{shape} in three chunks")
    errs = [relerr(b, a) for a, b in zip(whole[:2], cut[:2])]
    print("three chunks against one: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-6, errs


@pytest.mark.parametrize("shape", [GENERAL, FUSED])
def test_strided_inputs_give_the_bits_of_contiguous_ones(shape):
    import torch

    def strided(x):
        wide = torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=x.dtype,
                           device=x.device)
        view = wide[..., ::2]
        view.copy_(x)
        assert not view.is_contiguous()
        return view
    c = _case(shape)
    plain, other = _run_jvp(c), _run_jvp(c, view=strided)
    assert np.array_equal(plain[0], other[0])
    assert np.array_equal(plain[1], other[1])


# ------------------------------------------------------------ adjoint identity
@pytest.mark.parametrize("shape", [GENERAL, FUSED])
def test_adjoint_identity_on_the_device(shape):
    """<u, dI> against <psi.grad, d_psi> + <probe.grad, d_probe> +
    <scan.grad, d_scan> of `multislice_intensity`'s backward (real inner
    products in the `.grad` convention, summed in float64 on the host).  The
    bound is the sum of the bars the two sides carry, as
    test_autograd_jvp_gpu.py derives it: dI, psi.grad and probe.grad are each
    1e-5 normwise -- by Cauchy-Schwarz 1e-5 (|u| |dI| + |g_psi| |d_psi| +
    |g_probe| |d_probe|) -- and scan.grad SCAN_BAR A_n per position and
    coordinate, A_n from `autograd_multislice.hand_gradients`."""
    from tike_amd.autograd import (multislice_intensity,
                                   multislice_intensity_jvp)
    c = _case(shape)
    fly = c["fly"]
    leaves = [x.requires_grad_(True) for x in _device(c, "psi", "probe", "scan")]
    d_psi, d_probe, d_scan, u = _device(c, "d_psi", "d_probe", "d_scan", "u")
    with _operator(c) as op:
        _, tangent = multislice_intensity_jvp(
            op, *leaves, d_psi=d_psi, d_probe=d_probe, d_scan=d_scan, fly=fly)
        (multislice_intensity(op, *leaves, fly=fly) * u).sum().backward()
    gpsi, gprobe, gscan = (x.grad for x in leaves)
    left = aj.inner(u, tangent)
    right = (aj.inner(gpsi, d_psi) + aj.inner(gprobe, d_probe)
             + aj.inner(gscan, d_scan))
    m, _ = mj.as_model(c)
    hand = mm.hand_gradients(*m, mj.f64(c["u"]), fly, c["norm"])
    norm = lambda a: float(np.linalg.norm(np.asarray(a, np.complex128).ravel()))
    bound = 1e-5 * (norm(c["u"]) * norm(c["tangent"])
                    + norm(hand["psi"].numpy()) * norm(c["d_psi"])
                    + norm(hand["probe"].numpy()) * norm(c["d_probe"]))
    bound += mm.SCAN_BAR * float(
        (hand["A"].numpy() * np.abs(c["d_scan"].astype(np.float64))).sum())
    print(f"adjoint identity {shape}: <u, Jv> = {left:.9e}, <J^T u, v> = "
          f"{right:.9e}, difference {abs(left - right):.2e}, bound {bound:.2e}")
    assert abs(left - right) <= bound


# --------------------------------------------- multislice_gauss_newton_product
@pytest.mark.parametrize("shape,weighted", [(GENERAL, False), (FUSED, True)])
def test_gauss_newton_product_vs_model(shape, weighted):
    """J^T W J v against the float64 model (`hand_jvp`, then
    `autograd_multislice.hand_gradients` with g = W dI): the object part -- all
    D slices -- and the probe part normwise 1e-5, the scan part 1e-6 A_n per
    position and coordinate, A_n for that g; weight None and 1 / (I + 1).
    wrt=("scan", "psi") returns those two parts in that order."""
    import torch

    from tike_amd.autograd import multislice_gauss_newton_product
    c = _case(shape)
    fly = c["fly"]
    weight = (1.0 / (c["intensity"] + 1.0)).astype(np.float32) if weighted \
        else None
    g = c["tangent"] if weight is None else weight.astype(np.float64) * c[
        "tangent"]
    m, _ = mj.as_model(c)
    hand = mm.hand_gradients(*m, torch.from_numpy(g), fly, c["norm"])
    psi, probe, scan = _device(c, "psi", "probe", "scan")
    t = dict(zip(mj.TANGENT_NAMES, _device(c, *mj.TANGENT_NAMES)))
    w = None if weight is None else torch.from_numpy(weight).to("cuda")
    with _operator(c) as op:
        gpsi, gprobe, gscan = multislice_gauss_newton_product(
            op, psi, probe, scan, weight=w, fly=fly, **t)
        part = multislice_gauss_newton_product(
            op, psi, probe, scan, weight=w, fly=fly, wrt=("scan", "psi"), **t)
    host = lambda x: x.cpu().numpy()
    ratio = np.abs(host(gscan) - hand["scan"].numpy()) / hand["A"].numpy()
    per_slice = [relerr(host(gpsi)[d], hand["psi"].numpy()[d])
                 for d in range(psi.shape[0])]
    print(f"multislice_gauss_newton_product {shape} weighted={weighted}: psi "
          f"normwise {relerr(host(gpsi), hand['psi'].numpy()):.2e} (slices "
          + " ".join(f"{e:.2e}" for e in per_slice) + "), probe normwise "
          f"{relerr(host(gprobe), hand['probe'].numpy()):.2e}, scan max |err| "
          f"/ A_n {ratio.max():.2e}")
    assert gpsi.shape == psi.shape and gpsi.dtype == torch.complex64
    assert gprobe.shape == probe.shape
    assert gscan.shape == scan.shape and gscan.dtype == torch.float32
    assert relerr(host(gpsi), hand["psi"].numpy()) <= OP_NORMWISE
    assert max(per_slice) <= OP_NORMWISE
    assert relerr(host(gprobe), hand["probe"].numpy()) <= OP_NORMWISE
    assert np.all(ratio <= 1e-6), ratio.max()
    assert len(part) == 2
    assert part[0].shape == scan.shape and part[1].shape == psi.shape
    assert np.array_equal(host(part[0]), host(gscan))  # no atomics
    assert relerr(host(part[1]), host(gpsi)) <= 1e-6  # float atomics


# ----------------------------------------------------------- position recovery
def test_levenberg_marquardt_recovers_positions_of_a_two_slice_object():
    """`mm.problem(seed=49)`: 14 x 14 raster, pw = 32, fly = 2, true positions
    +- 0.3 px, two slices -- the problem on which 80 steps of Adam end at 0.43
    of the starting error.  Four Levenberg-Marquardt steps on scan alone
    (`autograd_jvp.gauss_newton`: at most 20 CG iterations, damping 1e-3),
    every product on the GPU -- `multislice_intensity` forward, J v by
    `multislice_intensity_jvp`, J^T u by the backward of
    `multislice_intensity`: a final RMS position error of at most 0.25 of its
    start and a final cost of at most 0.01 of its start (the float64 model:
    0.139 and 0.00145; 1.8 x and 7 x that, because the device works in float32
    and CG amplifies it)."""
    import torch

    from tike_amd.autograd import (multislice_intensity,
                                   multislice_intensity_jvp)
    p = mm.problem(seed=mm.RECOVERY["seed"])
    assert mm.RECOVERY["seed"] == 49
    fly = p["fly"]
    psi, probe, data, start = _device(p, "psi", "probe", "data", "scan_start")
    with _operator(dict(p, norm="ortho")) as op:

        def forward(scan):
            with torch.no_grad():
                return multislice_intensity(op, psi, probe, scan, fly=fly)

        def jtu(scan, u):
            s = scan.detach().requires_grad_(True)
            return torch.autograd.grad(
                multislice_intensity(op, psi, probe, s, fly=fly), s,
                grad_outputs=u)[0]

        jv = lambda scan, v: multislice_intensity_jvp(
            op, psi, probe, scan, d_scan=v, fly=fly)[1]
        after, costs = aj.gauss_newton(forward, jv, jtu, data, start, **mj.LM)
    r0 = am.rms(p["scan_start"], p["scan_true"])
    r = [am.rms(s, p["scan_true"]) for s in after]
    print(f"Levenberg-Marquardt on two slices: rms {r0:.4f} -> "
          + ", ".join(f"{x:.4f}" for x in r) + f" ({r[-1] / r0:.4f}); cost "
          f"{costs[0]:.3e} -> {costs[-1]:.3e} ({costs[-1] / costs[0]:.5f})")
    assert np.isfinite(costs).all()
    assert r[-1] <= 0.25 * r0, (r0, r)
    assert costs[-1] <= 0.01 * costs[0], costs
