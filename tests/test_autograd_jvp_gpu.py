"""The forward-mode derivative of `tike_amd.autograd.intensity` on the GPU
against the float64 model (tests/autograd_jvp.py): the two new entries on
their own, `intensity_jvp` end to end and cut into chunks, `intensity` on
forward_ad dual tensors, the adjoint identity between the forward and the
reverse mode, `gauss_newton_product`, and Gauss-Newton position recovery on
fly-scan data.

Every figure a bar is set on is printed before it is asserted."""
import functools

import numpy as np
import pytest

import autograd_jvp as aj
import autograd_model as am
from test_autograd_gpu import CONFIG, END_TO_END_CASES, _case, _edge_positions
from util import OP_MAXABS, OP_NORMWISE, assert_close, maxerr, relerr

pytestmark = pytest.mark.gpu

TANGENTS = [("d_psi",), ("d_probe",), ("d_scan",),
            ("d_psi", "d_probe", "d_scan")]


def _rc(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(
        np.complex64)


def _f64(a):
    import torch
    return None if a is None else torch.from_numpy(a).to(
        am.C128 if np.iscomplexobj(a) else am.F64)


# ---------------------------------------------- entry A: tike_conv_fwd_tangent
# pw, det, S, N: tiny; padding and no multiple of a wave; odd; a full wave (a
# second column segment of one column); a second column segment and uneven
# padding; a large window with many modes
CONV_TANGENT_CASES = [(5, 5, 1, 3), (20, 32, 3, 7), (33, 33, 2, 5),
                      (64, 64, 1, 4), (65, 128, 2, 3), (128, 128, 8, 2)]


@pytest.mark.parametrize("pw,det,S,N", CONV_TANGENT_CASES)
def test_conv_fwd_tangent_vs_float64_model(pw, det, S, N):
    """Entry by entry within the operator bars (normwise 1e-5, max-abs 1e-4 of
    the largest entry) for each tangent alone -- the others NULL -- and all
    three, at positions on the object's edges; the padding exactly 0.0; every
    element written (the buffer starts as a sentinel) and nothing behind the
    plane (a guard row keeps its sentinel)."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    rng = np.random.default_rng(pw + det + S)
    H, W = pw + 9, pw + 12
    host = dict(psi=_rc(rng, 1, H, W), probe=_rc(rng, 1, 1, S, pw, pw),
                scan=_edge_positions(rng, N, pw, H, W),
                d_psi=_rc(rng, 1, H, W), d_probe=_rc(rng, 1, 1, S, pw, pw),
                d_scan=rng.standard_normal((N, 2)).astype(np.float32))
    dev = torch.device("cuda")
    on = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    model = am.as_model(host["psi"], host["probe"], host["scan"])
    pad = (det - pw) // 2
    window = np.zeros((det, det), bool)
    window[pad:pad + pw, pad:pad + pw] = True
    count = N * S * det * det
    buf = torch.empty(count + det, dtype=torch.complex64, device=dev)
    sentinel = complex(7e30, -7e30)
    for names in TANGENTS + [()]:
        t = {k: host[k] if k in names else None
             for k in ("d_psi", "d_probe", "d_scan")}
        want = aj.tangent_nearplane(*model, det, **{
            k: _f64(v) for k, v in t.items()}).numpy()
        buf.fill_(sentinel)
        ptr = lambda k: A.ptr(on[k]) if k in names else None
        check(lib.tike_conv_fwd_tangent(
            A.ptr(on["psi"]), ptr("d_psi"), A.ptr(on["scan"]), ptr("d_scan"),
            A.ptr(on["probe"]), ptr("d_probe"), A.ptr(buf), N, S, pw, det, H,
            W, A.stream_ptr()), "tike_conv_fwd_tangent")
        got = buf.cpu().numpy()
        assert np.all(got[count:] == np.complex64(sentinel)), names
        got = got[:count].reshape(N, S, det, det)
        assert np.all(got.view(np.float32).reshape(N, S, det, det, 2)[
            :, :, ~window] == 0.0), names
        print(f"conv tangent ({pw}, {det}, {S}, {N}) {names}: normwise "
              f"{relerr(got, want):.2e} max-abs {maxerr(got, want):.2e}")
        if names:
            assert np.abs(want).max() > 0
            assert_close(got, want, OP_NORMWISE, OP_MAXABS, str(names))
        else:  # no tangent: zeros, written by the kernel
            assert not got.any()


# --------------------------------------------- entry B: tike_intensity_tangent
# nframe, P, npix: P of 1, 3 and 8; npix % 4 of 1, 0 and 3; one and several
# workgroups per frame
INTENSITY_TANGENT_CASES = [(3, 1, 169), (2, 3, 256), (2, 8, 403),
                           (2, 3, 1027), (1, 8, 16384), (2, 1, 3)]


@pytest.mark.parametrize("nframe,P,npix", INTENSITY_TANGENT_CASES)
def test_intensity_tangent(nframe, P, npix):
    """I has the bits of tike_intensity; dI is within one float32
    multiply-add chain of the float64 sum, 1e-6 sum_j |far_j| |dfar_j| per
    pixel (the issue's bar; dI is twice a float32 sum of P terms of two
    rounded products each, and 2e-7 of that scale is the most measured); two
    calls give the same bits, with and without the intensity; the frames in
    front of and behind the results are not written."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    rng = np.random.default_rng(P + npix)
    far, dfar = _rc(rng, nframe, P, npix), _rc(rng, nframe, P, npix)
    dev = torch.device("cuda")
    far_d, dfar_d = torch.from_numpy(far).to(dev), torch.from_numpy(dfar).to(dev)
    ref = torch.empty((nframe, npix), dtype=torch.float32, device=dev)
    check(lib.tike_intensity(A.ptr(far_d), A.ptr(ref), nframe, P, npix,
                             A.stream_ptr()), "tike_intensity")
    out = []
    for with_intensity in (True, True, False):
        inten = torch.full((nframe + 2, npix), 7.0, dtype=torch.float32,
                           device=dev)
        tangent = torch.full((nframe + 2, npix), 7.0, dtype=torch.float32,
                             device=dev)
        check(lib.tike_intensity_tangent(
            A.ptr(far_d), A.ptr(dfar_d),
            A.ptr(inten[1:]) if with_intensity else None, A.ptr(tangent[1:]),
            nframe, P, npix, A.stream_ptr()), "tike_intensity_tangent")
        out.append((inten.cpu().numpy(), tangent.cpu().numpy()))
        for x in out[-1]:
            assert np.all(x[[0, -1]] == 7.0)
    assert np.array_equal(out[0][0][1:-1], ref.cpu().numpy())
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][1], out[2][1])
    assert np.all(out[2][0] == 7.0)  # NULL: no intensity is written
    f, d = far.astype(np.complex128), dfar.astype(np.complex128)
    want = 2 * (f.conj() * d).real.sum(axis=1)
    scale = (np.abs(f) * np.abs(d)).sum(axis=1)
    ratio = np.abs(out[0][1][1:-1] - want) / scale
    print(f"intensity tangent ({nframe}, {P}, {npix}): max |err| / "
          f"sum |far| |dfar| = {ratio.max():.2e}")
    assert np.all(ratio <= 1e-6), ratio.max()


# ------------------------------------------------------------------ end to end
NORM_CASES = [(CONFIG, norm) for norm in ("ortho", "forward", "backward")] + [
    ((4, 2, 100, 128, 240, 250, 2), norm)
    for norm in ("ortho", "forward", "backward")]


@functools.lru_cache(maxsize=None)
def _jvp_case(shape, norm="ortho"):
    """The inputs of `test_autograd_gpu._case` with seeded tangents, a random
    signed u, and the model's I, dI -- computed once, shared, left unchanged."""
    N, S, pw, det, H, W, fly = shape
    base = _case(*shape, norm)
    rng = np.random.default_rng(11 + N + det)
    c = dict(psi=base["psi"], probe=base["probe"], scan=base["scan"],
             d_psi=_rc(rng, 1, H, W), d_probe=_rc(rng, 1, 1, S, pw, pw),
             d_scan=rng.standard_normal((N, 2)).astype(np.float32),
             u=rng.standard_normal((N // fly, det, det)).astype(np.float32))
    model = am.as_model(c["psi"], c["probe"], c["scan"])
    inten, tangent = aj.hand_jvp(
        *model, det, *(_f64(c[k]) for k in ("d_psi", "d_probe", "d_scan")),
        fly, norm)
    return dict(c, intensity=inten.numpy(), tangent=tangent.numpy())


def _operator(shape, norm="ortho"):
    import tike_amd.operators as ops
    N, S, pw, det, H, W, fly = shape
    return ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W, norm=norm)


def _device(c, *names):
    import torch
    return [torch.from_numpy(c[k]).to("cuda") for k in names]


def _run_jvp(shape, norm="ortho", names=("d_psi", "d_probe", "d_scan")):
    """(I, dI, I of `intensity`) as host arrays."""
    import torch

    from tike_amd.autograd import intensity, intensity_jvp
    c = _jvp_case(shape, norm)
    psi, probe, scan = _device(c, "psi", "probe", "scan")
    t = dict(zip(names, _device(c, *names)))
    with _operator(shape, norm) as op:
        inten, tangent = intensity_jvp(op, psi, probe, scan, fly=shape[-1], **t)
        with torch.no_grad():
            plain = intensity(op, psi, probe, scan, fly=shape[-1])
    for x in (inten, tangent):
        assert x.dtype == torch.float32 and not x.requires_grad
        assert tuple(x.shape) == (shape[0] // shape[-1], shape[3], shape[3])
    return tuple(x.cpu().numpy() for x in (inten, tangent, plain))


def _assert_jvp(shape, norm, got, what):
    c = _jvp_case(shape, norm)
    inten, tangent, plain = got
    print(f"{what}: dI normwise {relerr(tangent, c['tangent']):.2e} max-abs "
          f"{maxerr(tangent, c['tangent']):.2e}; I normwise "
          f"{relerr(inten, c['intensity']):.2e}")
    assert np.array_equal(inten, plain), what  # the bits of intensity(...)
    assert_close(inten, c["intensity"], OP_NORMWISE, OP_MAXABS, what + " I")
    assert_close(tangent, c["tangent"], OP_NORMWISE, OP_MAXABS, what + " dI")


@pytest.mark.parametrize("N,S,pw,det,H,fly", END_TO_END_CASES)
def test_intensity_jvp_vs_model(N, S, pw, det, H, fly):
    """dI within the operator bars (normwise 1e-5, max-abs 1e-4) of the
    float64 `hand_jvp` with all three tangents (the float32 restatement on the
    CPU: 1.4 - 1.5e-7 normwise); I bit-identical to `intensity(...)`."""
    shape = (N, S, pw, det, H, H, fly)
    _assert_jvp(shape, "ortho", _run_jvp(shape), str(shape))


@pytest.mark.parametrize("shape,norm", NORM_CASES)
def test_intensity_jvp_other_norms(shape, norm):
    """The operator's norm is honoured (the forward scale rides on the
    transform of the tangent): det 20 and 128."""
    _assert_jvp(shape, norm, _run_jvp(shape, norm), f"{shape} norm={norm}")


def test_no_tangent_gives_zeros():
    got = _run_jvp(CONFIG, names=())
    assert np.array_equal(got[0], got[2]) and not got[1].any()


def test_three_chunks(monkeypatch):
    """Cut into three chunks of whole frames: the bits of I and dI of the
    whole run (a chunk holds half of `chunk_positions`: two far planes)."""
    from tike_amd.ptycho.solvers import lstsq
    N, S, pw, det, H, W, fly = CONFIG
    whole = _run_jvp(CONFIG)
    monkeypatch.setattr(lstsq, "CHUNK_POSITIONS_OVERRIDE", 8)
    assert max(1, lstsq.chunk_positions(S, det) // 2 // fly) * fly * 3 == N
    cut = _run_jvp(CONFIG)
    _assert_jvp(CONFIG, "ortho", cut, "three chunks")
    assert np.array_equal(whole[0], cut[0])
    assert np.array_equal(whole[1], cut[1])


# ---------------------------------------------------------------- forward mode
@pytest.mark.parametrize("names", [("d_scan",), ("d_psi", "d_probe", "d_scan")])
def test_intensity_on_dual_tensors(names):
    """`intensity` on forward_ad dual tensors returns a dual whose tangent has
    the bits of `intensity_jvp`'s dI.  Fails on the parent commit: torch asks
    for the jvp function."""
    import torch
    import torch.autograd.forward_ad as fwad

    from tike_amd.autograd import intensity
    c = _jvp_case(CONFIG)
    fly = CONFIG[-1]
    primal = dict(zip(("psi", "probe", "scan"),
                      _device(c, "psi", "probe", "scan")))
    want = _run_jvp(CONFIG, names=names)
    with _operator(CONFIG) as op, fwad.dual_level():
        for k in names:
            (tangent,) = _device(c, k)
            primal[k[2:]] = fwad.make_dual(primal[k[2:]], tangent)
        out = fwad.unpack_dual(intensity(op, primal["psi"], primal["probe"],
                                         primal["scan"], fly=fly))
        assert out.tangent is not None
        got = out.primal.cpu().numpy(), out.tangent.cpu().numpy()
    assert got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    if len(names) == 3:  # (the model's tangent is that of all three)
        _assert_jvp(CONFIG, "ortho", (got[0], got[1], want[2]), "dual tensors")


def test_other_models_keep_torchs_refusal_under_forward_ad():
    """`multislice_intensity` and the eigen-probe form of `intensity` have no
    forward-mode rule: torch's own refusal, not a wrong tangent."""
    import torch
    import torch.autograd.forward_ad as fwad

    import autograd_multislice as mm
    import tike_amd.operators as ops
    from tike_amd.autograd import intensity, multislice_intensity
    c = _jvp_case(CONFIG)
    N, S, pw, det, H, W, fly = CONFIG
    psi, probe, scan, d_scan = _device(c, "psi", "probe", "scan", "d_scan")
    refusal = pytest.raises((NotImplementedError, RuntimeError),
                            match="(?i)implement the jvp")
    with _operator(CONFIG) as op, fwad.dual_level():
        weights = torch.ones((N, 1, S), dtype=torch.float32, device="cuda")
        with refusal:
            intensity(op, psi, probe, fwad.make_dual(scan, d_scan),
                      eigen_weights=weights, fly=fly)
    wide = torch.ones((1, 1, S, 16, 16), dtype=torch.complex64, device="cuda")
    two = psi.expand(2, H, W).contiguous()
    with ops.Ptycho(probe_shape=16, detector_shape=16, nz=H, n=W,
                    **mm.optics(16)) as op, fwad.dual_level():
        with refusal:
            multislice_intensity(op, two, wide, fwad.make_dual(scan, d_scan),
                                 fly=fly)


# ------------------------------------------------------------ adjoint identity
# fly = 2 with probe window < detector; fly = 2 with window = detector; fly = 1
# with probe window < detector
ADJOINT_CASES = [CONFIG, (8, 3, 16, 16, 40, 40, 2), (6, 2, 48, 64, 120, 120, 1)]


@pytest.mark.parametrize("shape", ADJOINT_CASES)
def test_adjoint_identity_on_the_device(shape):
    """<u, dI> against <psi.grad, d_psi> + <probe.grad, d_probe> +
    <scan.grad, d_scan> of the existing backward (real inner products in the
    `.grad` convention, summed in float64 on the host).  The bound is the sum
    of the bars the two sides already carry: dI, psi.grad and probe.grad are
    each 1e-5 normwise -- by Cauchy-Schwarz 1e-5 (|u| |dI| + |g_psi| |d_psi| +
    |g_probe| |d_probe|) -- and scan.grad 1e-6 A_n per position and coordinate
    -- 1e-6 sum_n (A_n,y |ds_n,y| + A_n,x |ds_n,x|), A_n from
    `autograd_model.hand_gradients`."""
    import torch

    from tike_amd.autograd import intensity, intensity_jvp
    N, S, pw, det, H, W, fly = shape
    c = _jvp_case(shape)
    leaves = [x.requires_grad_(True) for x in _device(c, "psi", "probe", "scan")]
    d_psi, d_probe, d_scan, u = _device(c, "d_psi", "d_probe", "d_scan", "u")
    with _operator(shape) as op:
        _, tangent = intensity_jvp(op, *leaves, d_psi=d_psi, d_probe=d_probe,
                                   d_scan=d_scan, fly=fly)
        (intensity(op, *leaves, fly=fly) * u).sum().backward()
    gpsi, gprobe, gscan = (x.grad for x in leaves)
    left = aj.inner(u, tangent)
    right = (aj.inner(gpsi, d_psi) + aj.inner(gprobe, d_probe)
             + aj.inner(gscan, d_scan))
    hand = am.hand_gradients(*am.as_model(c["psi"], c["probe"], c["scan"]),
                             det, _f64(c["u"]), fly)
    norm = lambda a: float(np.linalg.norm(np.asarray(a, np.complex128).ravel()))
    bound = 1e-5 * (norm(c["u"]) * norm(c["tangent"])
                    + norm(hand["psi"].numpy()) * norm(c["d_psi"])
                    + norm(hand["probe"].numpy()) * norm(c["d_probe"]))
    bound += 1e-6 * float(
        (hand["A"].numpy() * np.abs(c["d_scan"].astype(np.float64))).sum())
    print(f"adjoint identity {shape}: <u, Jv> = {left:.9e}, <J^T u, v> = "
          f"{right:.9e}, difference {abs(left - right):.2e}, bound {bound:.2e}")
    assert abs(left - right) <= bound


# -------------------------------------------------------- gauss_newton_product
@pytest.mark.parametrize("shape,weighted", [(CONFIG, False),
                                            ((6, 2, 48, 64, 120, 120, 1), True)])
def test_gauss_newton_product_vs_model(shape, weighted, monkeypatch):
    """J^T W J v against the float64 model (`hand_jvp`, then `hand_gradients`
    with g = W dI): the object and the probe part normwise 1e-5, the scan part
    1e-6 A_n per position and coordinate, A_n for that g; weight None and
    1 / (I + 1).  wrt=("scan",) launches no object scatter and gives the bits
    of the scan part of the full product."""
    import torch

    from tike_amd import autograd
    N, S, pw, det, H, W, fly = shape
    c = _jvp_case(shape)
    weight = (1.0 / (c["intensity"] + 1.0)).astype(np.float32) if weighted \
        else None
    g = c["tangent"] if weight is None else weight.astype(np.float64) * c[
        "tangent"]
    hand = am.hand_gradients(*am.as_model(c["psi"], c["probe"], c["scan"]),
                             det, torch.from_numpy(g), fly)
    psi, probe, scan = _device(c, "psi", "probe", "scan")
    t = dict(zip(("d_psi", "d_probe", "d_scan"),
                 _device(c, "d_psi", "d_probe", "d_scan")))
    w = None if weight is None else torch.from_numpy(weight).to("cuda")
    scatters = []
    scatter = autograd.lib.tike_scatter_patches
    monkeypatch.setattr(autograd.lib, "tike_scatter_patches",
                        lambda *a: scatters.append(1) or scatter(*a))
    with _operator(shape) as op:
        gpsi, gprobe, gscan = autograd.gauss_newton_product(
            op, psi, probe, scan, weight=w, fly=fly, **t)
        assert scatters
        del scatters[:]
        (only,) = autograd.gauss_newton_product(
            op, psi, probe, scan, weight=w, fly=fly, wrt=("scan",), **t)
        assert not scatters
    host = lambda x: x.cpu().numpy()
    ratio = np.abs(host(gscan) - hand["scan"].numpy()) / hand["A"].numpy()
    print(f"gauss_newton_product {shape} weighted={weighted}: psi normwise "
          f"{relerr(host(gpsi), hand['psi'].numpy()):.2e}, probe normwise "
          f"{relerr(host(gprobe), hand['probe'].numpy()):.2e}, scan max |err| "
          f"/ A_n {ratio.max():.2e}")
    assert gpsi.shape == psi.shape and gprobe.shape == probe.shape
    assert gscan.shape == scan.shape and gscan.dtype == torch.float32
    assert relerr(host(gpsi), hand["psi"].numpy()) <= OP_NORMWISE
    assert relerr(host(gprobe), hand["probe"].numpy()) <= OP_NORMWISE
    assert np.all(ratio <= 1e-6), ratio.max()
    assert np.array_equal(host(only), host(gscan))


# ----------------------------------------------------------- position recovery
def test_gauss_newton_recovers_fly_scan_positions():
    """`problem()`: 14 x 14 raster, fly = 2, true positions +- 0.3 px.  Four
    damped Gauss-Newton steps on scan alone (`autograd_jvp.gauss_newton`: at
    most 20 CG iterations each), every product on the GPU -- J v by
    `intensity_jvp`, J^T u by the backward of `intensity`: finite costs and an
    RMS position error of at most 0.1 of its start (the float64 model reaches
    0.02; the factor 5 is room for float32 CG).  40 steps of Adam on the same
    GPU model are printed next to it."""
    import torch

    from tike_amd.autograd import intensity, intensity_jvp
    p = am.problem()
    fly = p["fly"]
    psi, probe, data, start = _device(p, "psi", "probe", "data", "scan_start")
    shape = (0, 1, p["det"], p["det"], psi.shape[-2], psi.shape[-1], fly)
    with _operator(shape) as op:

        def forward(scan):
            with torch.no_grad():
                return intensity(op, psi, probe, scan, fly=fly)

        def jtu(scan, u):
            s = scan.detach().requires_grad_(True)
            return torch.autograd.grad(intensity(op, psi, probe, s, fly=fly),
                                       s, grad_outputs=u)[0]

        jv = lambda scan, v: intensity_jvp(op, psi, probe, scan, d_scan=v,
                                           fly=fly)[1]
        after, costs = aj.gauss_newton(forward, jv, jtu, data, start)
        adam, _ = am.recover(
            lambda s: am.amplitude_loss(
                intensity(op, psi, probe, s, fly=fly), data), start)
    r0 = am.rms(p["scan_start"], p["scan_true"])
    r = [am.rms(s, p["scan_true"]) for s in after]
    ra = am.rms(adam, p["scan_true"])
    print(f"Gauss-Newton position recovery: rms {r0:.4f} -> "
          + ", ".join(f"{x:.4f}" for x in r) + f" ({r[-1] / r0:.4f}); cost "
          f"{costs[0]:.3e} -> {costs[-1]:.3e}; 40 steps of Adam: {ra:.4f} "
          f"({ra / r0:.4f})")
    assert np.isfinite(costs).all()
    assert r[-1] <= 0.1 * r0, (r0, r)
