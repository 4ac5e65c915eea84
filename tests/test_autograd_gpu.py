"""`tike_amd.autograd.intensity` on the GPU against the float64 model
(tests/autograd_model.py): the two new entries on their own, the forward and
the three gradients end to end, the same in other configurations, and
position recovery on fly-scan data by `torch.optim.Adam`.

Every figure a bar is set on is printed before it is asserted."""
import functools

import numpy as np
import pytest

import autograd_model as am
from util import OP_MAXABS, OP_NORMWISE, assert_close, maxerr, relerr

pytestmark = pytest.mark.gpu


def _rc(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(
        np.complex64)


# ------------------------------------------------- entry B: tike_scan_gradient
SCAN_GRADIENT_CASES = [(5, 8, 24, 31), (7, 13, 40, 37), (4, 33, 70, 64),
                       (3, 64, 130, 150), (2, 128, 260, 260)]


def _edge_positions(rng, nscan, pw, H, W):
    """Position 0 has floor (1, 1) and an exactly integer first coordinate,
    position 1 floor (H - pw - 1, W - pw - 1), the others anywhere allowed;
    every other fraction lies in [0.05, 0.95]."""
    frac = lambda *s: 0.05 + 0.9 * rng.random(s)
    scan = np.stack([rng.integers(1, H - pw, nscan) + frac(nscan),
                     rng.integers(1, W - pw, nscan) + frac(nscan)], 1)
    scan[0] = (1.0, 1 + frac())
    scan[1] = (H - pw - 1 + frac(), W - pw - 1 + frac())
    scan = scan.astype(np.float32)
    corner = np.floor(scan)
    assert tuple(corner[0]) == (1, 1) and scan[0, 0] == 1.0
    assert tuple(corner[1]) == (H - pw - 1, W - pw - 1)
    return scan


@pytest.mark.parametrize("nscan,pw,H,W", SCAN_GRADIENT_CASES)
def test_scan_gradient_vs_float64_model(nscan, pw, H, W):
    """|err| <= 1e-7 A_n per position and coordinate, A_n the sum of the
    absolute terms, on the same float32 objproj: a term carries a handful of
    float32 roundings (2^-24 each), the sum is float64 (float32 products with
    float64 sums stay at or below 6.1e-9 A_n on the CPU; a float32 running sum
    would not meet the bar).  Two calls give the same bits; the entries next
    to the result are not written."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    rng = np.random.default_rng(nscan + pw)
    psi, q = _rc(rng, 1, H, W), _rc(rng, nscan, pw, pw)
    scan = _edge_positions(rng, nscan, pw, H, W)
    want, absum = am.scan_gradient(torch.from_numpy(q),
                                   torch.from_numpy(psi).to(am.C128),
                                   torch.from_numpy(scan).to(am.F64))
    dev = torch.device("cuda")
    d = lambda a: torch.from_numpy(a).to(dev)
    guard = torch.full((nscan + 2, 2), 7.0, dtype=torch.float32, device=dev)
    q_d, scan_d, psi_d = d(q), d(scan), d(psi)  # (alive over the launches)
    args = (A.ptr(q_d), A.ptr(scan_d), A.ptr(psi_d))
    out = []
    for _ in range(2):
        guard.fill_(7.0)
        check(lib.tike_scan_gradient(*args, A.ptr(guard[1:]), nscan, pw, H, W,
                                     A.stream_ptr()), "tike_scan_gradient")
        out.append(guard.cpu().numpy().copy())
    assert np.array_equal(out[0], out[1])
    assert np.all(out[0][[0, -1]] == 7.0)
    got = out[0][1:-1].astype(np.float64)
    ratio = np.abs(got - want.numpy()) / absum.numpy()
    cancel = np.abs(want.numpy()) / absum.numpy()
    print(f"scan gradient ({nscan}, {pw}, {H}, {W}): max |err| / A_n = "
          f"{ratio.max():.2e}; |sum| / A_n from {cancel.min():.1e}")
    assert np.all(ratio <= 1e-7), ratio


# ------------------------------------------------ entry A: tike_farplane_scale
FARPLANE_SCALE_CASES = [(3, 1, 13), (2, 6, 16), (2, 17, 20), (1, 32, 32),
                        (1, 3, 128)]


@pytest.mark.parametrize("nframe,P,det", FARPLANE_SCALE_CASES)
def test_farplane_scale_vs_numpy(nframe, P, det):
    """farplane[f][j][p] *= scale * table[f][p] with a signed table: the
    factor is one float32 product, each part of a plane one more -- NumPy's
    float32 products in the same order give the same bits.  A frame in front
    of and one behind the planes handed in stay as they were."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    rng = np.random.default_rng(P + det)
    npix = det * det
    far = _rc(rng, nframe + 2, P, npix)
    table = rng.standard_normal((nframe, npix)).astype(np.float32)
    scale = np.float32(0.3)
    t = scale * table  # float32
    want = far.copy()
    want[1:-1].real = far[1:-1].real * t[:, None]
    want[1:-1].imag = far[1:-1].imag * t[:, None]
    dev = torch.device("cuda")
    far_d = torch.from_numpy(far).to(dev)
    table_d = torch.from_numpy(table).to(dev)
    check(lib.tike_farplane_scale(A.ptr(far_d[1:-1]), A.ptr(table_d), nframe,
                                  P, npix, float(scale), A.stream_ptr()),
          "tike_farplane_scale")
    got = far_d.cpu().numpy()
    exact = far[1:-1].astype(np.complex128) * (
        np.float64(scale) * table.astype(np.float64))[:, None]
    print(f"farplane scale ({nframe}, {P}, {det}): normwise error against "
          f"float64 {relerr(got[1:-1], exact):.2e}")
    assert np.array_equal(got.view(np.float32), want.view(np.float32))


# ------------------------------------------------------------------ end to end
END_TO_END_CASES = [(6, 2, 8, 12, 24, 1), (8, 3, 16, 16, 40, 2),
                    (12, 1, 13, 20, 37, 3), (16, 4, 32, 32, 80, 4),
                    (8, 8, 64, 64, 150, 2), (6, 2, 48, 64, 120, 1),
                    (4, 2, 128, 128, 300, 2), (3, 1, 100, 128, 260, 1)]


@functools.lru_cache(maxsize=None)
def _case(N, S, pw, det, H, W, fly, norm="ortho"):
    """Host inputs with a random signed upstream gradient, and the model's
    intensity and gradients -- computed once, shared, left unchanged."""
    import torch
    rng = np.random.default_rng(N + 3 * S + 5 * det)
    psi, probe = _rc(rng, 1, H, W), _rc(rng, 1, 1, S, pw, pw)
    scan = np.stack([1 + rng.random(N) * (H - pw - 1),
                     1 + rng.random(N) * (W - pw - 1)], 1).astype(np.float32)
    g = rng.standard_normal((N // fly, det, det)).astype(np.float32)
    m = am.as_model(psi, probe, scan)
    gt = torch.from_numpy(g).to(am.F64)
    with torch.no_grad():
        inten = am.intensity(*m, det, fly, norm).numpy()
    hand = {k: v.numpy() for k, v in am.hand_gradients(
        *m, det, gt, fly, norm).items()}
    return dict(psi=psi, probe=probe, scan=scan, g=g, intensity=inten, **{
        "grad_" + k: v for k, v in hand.items()})


def _run(case, det, fly, norm="ortho", needs=(True, True, True)):
    """(intensity, psi.grad, probe.grad, scan.grad) of sum(g * intensity) on
    the GPU, as host arrays (None where no gradient was asked for)."""
    import torch

    import tike_amd.operators as ops
    from tike_amd.autograd import intensity
    dev = torch.device("cuda")
    leaves = [torch.from_numpy(case[k]).to(dev).requires_grad_(r)
              for k, r in zip(("psi", "probe", "scan"), needs)]
    psi, probe, scan = leaves
    with ops.Ptycho(probe_shape=probe.shape[-1], detector_shape=det,
                    nz=psi.shape[-2], n=psi.shape[-1], norm=norm) as op:
        inten = intensity(op, psi, probe, scan, fly=fly)
        assert inten.dtype == torch.float32
        (inten * torch.from_numpy(case["g"]).to(dev)).sum().backward()
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    return (host(inten),) + tuple(host(x.grad) for x in leaves)


def _assert_matches(case, got, what, needs=(True, True, True)):
    inten, gpsi, gprobe, gscan = got
    lines = [f"{what}: intensity normwise {relerr(inten, case['intensity']):.2e}"
             f" max-abs {maxerr(inten, case['intensity']):.2e}"]
    for name, x in (("psi", gpsi), ("probe", gprobe)):
        if x is not None:
            lines.append(f"{name}.grad normwise "
                         f"{relerr(x, case['grad_' + name]):.2e} max-abs "
                         f"{maxerr(x, case['grad_' + name]):.2e}")
    if gscan is not None:
        ratio = np.abs(gscan - case["grad_scan"]) / case["grad_A"]
        lines.append(f"scan.grad max |err| / A_n {ratio.max():.2e}")
    print("; ".join(lines))
    assert_close(inten, case["intensity"], OP_NORMWISE, OP_MAXABS,
                 what + " intensity")
    for name, x, need in (("psi", gpsi, needs[0]), ("probe", gprobe, needs[1])):
        assert (x is not None) == need, (what, name)
        if need:
            assert x.shape == case[name].shape
            assert_close(x, case["grad_" + name], OP_NORMWISE, OP_MAXABS,
                         f"{what} {name}.grad")
    assert (gscan is not None) == needs[2], what
    if needs[2]:
        assert gscan.shape == case["scan"].shape and gscan.dtype == np.float32
        assert np.all(ratio <= 1e-6), (what, ratio)


@pytest.mark.parametrize("N,S,pw,det,H,fly", END_TO_END_CASES)
def test_intensity_and_gradients_vs_model(N, S, pw, det, H, fly):
    """Intensity, psi.grad and probe.grad within the operator bars (normwise
    1e-5, max-abs 1e-4; a float32 restatement of the formulas on the CPU is
    0.9 - 2.1e-7 normwise from the float64 one); scan.grad within 1e-6 A_n
    per position and coordinate (the float32 restatement: 3.3e-8 A_n)."""
    case = _case(N, S, pw, det, H, H, fly)
    _assert_matches(case, _run(case, det, fly),
                    f"({N}, {S}, {pw}, {det}, {H}, {fly})")


# --------------------------------------------------------- other configurations
CONFIG = (12, 2, 16, 20, 40, 45, 2)  # N, S, pw, det, H, W, fly


def test_three_chunks(monkeypatch):
    """The minibatch cut into three chunks of whole frames gives what one
    chunk gives: forward and backward."""
    from tike_amd.ptycho.solvers import lstsq
    N, S, pw, det, H, W, fly = CONFIG
    case = _case(*CONFIG)
    whole = _run(case, det, fly)
    monkeypatch.setattr(lstsq, "CHUNK_POSITIONS_OVERRIDE", 4)
    assert max(1, lstsq.chunk_positions(S, det) // fly) * fly * 3 == N
    cut = _run(case, det, fly)
    _assert_matches(case, cut, "three chunks")
    # the chunks only regroup sums over the positions
    assert np.array_equal(whole[0], cut[0])
    assert np.array_equal(whole[3], cut[3])


@pytest.mark.parametrize("det", [20, 128])
@pytest.mark.parametrize("norm", ["backward", "forward"])
def test_other_norms(norm, det):
    """The operator's norm is honoured, on both routes of the backward (the
    table applied by the inverse at 128; by tike_farplane_scale at 20)."""
    shape = CONFIG if det == 20 else (4, 2, 100, 128, 240, 250, 2)
    case = _case(*shape, norm)
    _assert_matches(case, _run(case, det, shape[-1], norm), f"norm={norm}")


@pytest.mark.parametrize("needs", [(False, False, True), (True, False, False),
                                   (False, True, False)])
def test_only_one_input_requires_a_gradient(needs):
    """The other .grads are None and the computed one is what it is when all
    three are asked for."""
    N, S, pw, det, H, W, fly = CONFIG
    case = _case(*CONFIG)
    full = _run(case, det, fly)
    part = _run(case, det, fly, needs=needs)
    _assert_matches(case, part, f"needs={needs}", needs)
    for a, b, need in zip(full[1:], part[1:], needs):
        if need and a.dtype == np.float32:  # scan.grad: no atomics
            assert np.array_equal(a, b)
        elif need:
            assert relerr(b, a) <= 1e-6


# ----------------------------------------------------------- position recovery
def test_adam_recovers_fly_scan_positions():
    """`problem()`: 14 x 14 raster, fly = 2, true positions +- 0.3 px; 40 steps
    of Adam(lr=0.05) on scan alone with the gaussian amplitude loss.  Final RMS
    position error <= 0.25 of its start and cost below 1 % of its start (the
    float64 model reaches 0.08 - 0.10 and 0.5 %)."""
    import torch

    import tike_amd.operators as ops
    from tike_amd.autograd import intensity
    p = am.problem()
    dev = torch.device("cuda")
    psi, probe, data, start = (torch.from_numpy(p[k]).to(dev) for k in (
        "psi", "probe", "data", "scan_start"))
    with ops.Ptycho(probe_shape=p["det"], detector_shape=p["det"],
                    nz=psi.shape[-2], n=psi.shape[-1]) as op:
        final, costs = am.recover(
            lambda s: am.amplitude_loss(
                intensity(op, psi, probe, s, fly=p["fly"]), data), start)
    r0 = am.rms(p["scan_start"], p["scan_true"])
    r1 = am.rms(final, p["scan_true"])
    print(f"position recovery: rms {r0:.3f} -> {r1:.3f} ({r1 / r0:.3f}), "
          f"cost {costs[0]:.2e} -> {costs[-1]:.2e} ({costs[-1] / costs[0]:.4f})")
    assert np.isfinite(costs).all()
    assert r1 <= 0.25 * r0, (r0, r1)
    assert costs[-1] < 0.01 * costs[0], (costs[0], costs[-1])
