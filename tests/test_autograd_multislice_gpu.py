"""`tike_amd.autograd.multislice_intensity` on the GPU against the float64
model (tests/autograd_multislice.py): the new entry on its own, the hand-off of
the inverse pass 1 that takes the upstream gradient, the forward and the three
gradients end to end on both routes, the same under the routes' switches, in
chunks, with other norms and with single gradients, and position recovery on a
two-slice object by `torch.optim.Adam`.

Every figure a bar is set on is printed before it is asserted."""
import functools

import numpy as np
import pytest

import autograd_model as am
import autograd_multislice as mm
from util import OP_MAXABS, OP_NORMWISE, assert_close, maxerr, relerr

pytestmark = pytest.mark.gpu


# ------------------------------------------ entry: tike_scan_gradient_slices
SLICES_CASES = [(5, 2, 8, 24, 31), (4, 3, 13, 40, 37), (3, 2, 64, 150, 141),
                (2, 4, 128, 300, 300)]


def _edge_positions(rng, nscan, pw, H, W):
    """Position 0 has floor (1, 1) and an exactly integer first coordinate;
    position 1 hangs over the bottom right corner of the object (its last
    rows and columns of taps are outside); position 2 has floor
    (H - pw - 1, W - pw - 1), the last allowed corner; position 3 hangs over
    the top left corner (negative coordinates); the others anywhere allowed.
    Every other fraction lies in [0.05, 0.95]."""
    frac = lambda *s: 0.05 + 0.9 * rng.random(s)
    scan = np.stack([rng.integers(1, H - pw, nscan) + frac(nscan),
                     rng.integers(1, W - pw, nscan) + frac(nscan)], 1)
    scan[0] = (1.0, 1 + frac())
    scan[1] = (H - pw + 2 + frac(), W - pw + 1 + frac())
    if nscan > 2:
        scan[2] = (H - pw - 1 + frac(), W - pw - 1 + frac())
    if nscan > 3:
        scan[3] = (-3 + frac(), -2 + frac())
    scan = scan.astype(np.float32)
    corner = np.floor(scan)
    assert tuple(corner[0]) == (1, 1) and scan[0, 0] == 1.0
    assert corner[1, 0] + pw > H and corner[1, 1] + pw > W
    return scan


def _slices_want(q, psi, scan, margin=8):
    """(grad, A) (nscan, 2) float64: the model's scan gradient summed over
    the slices, a tap outside the object counting as zero (the object is laid
    into a frame of zeros and the positions moved along)."""
    import torch
    D, H, W = psi.shape
    framed = np.zeros((D, H + 2 * margin, W + 2 * margin), np.complex128)
    framed[:, margin:-margin, margin:-margin] = psi
    moved = torch.from_numpy(scan).to(am.F64) + margin
    grad, absum = 0, 0
    for d in range(D):
        g, a = am.scan_gradient(torch.from_numpy(q[d]),
                                torch.from_numpy(framed[d:d + 1]), moved)
        grad, absum = grad + g.numpy(), absum + a.numpy()
    return grad, absum


@pytest.mark.parametrize("nscan,D,pw,H,W", SLICES_CASES)
def test_scan_gradient_slices_vs_float64_model(nscan, D, pw, H, W):
    """|err| <= 1e-7 A_n per position and coordinate, A_n the sum of the
    absolute terms over all slices, on the same float32 objproj: the
    arithmetic of a term is `tike_scan_gradient`'s (a handful of float32
    roundings, 2^-24 each) and the one running sum over slices and pixels is
    float64, so its bar holds.  Two calls give the same bits, a strided
    workspace the bits of a packed one, one slice the bits of
    `tike_scan_gradient`; the entries next to the result are not written."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    rng = np.random.default_rng(nscan + pw + D)
    psi, q = mm.rc(rng, D, H, W), mm.rc(rng, D, nscan, pw, pw)
    scan = _edge_positions(rng, nscan, pw, H, W)
    want, absum = _slices_want(q, psi, scan)
    dev = torch.device("cuda")
    d = lambda a: torch.from_numpy(a).to(dev)
    guard = torch.full((nscan + 2, 2), 7.0, dtype=torch.float32, device=dev)
    q_d, scan_d, psi_d = d(q), d(scan), d(psi)  # (alive over the launches)
    P = pw * pw

    def call(objproj, stride, slices=D, first=0):
        guard.fill_(7.0)
        check(
            lib.tike_scan_gradient_slices(
                A.ptr(objproj), stride, A.ptr(scan_d), A.ptr(psi_d[first:]),
                A.ptr(guard[1:]), nscan, slices, pw, H, W, A.stream_ptr()),
            "tike_scan_gradient_slices")
        return guard.cpu().numpy().copy()
    out = [call(q_d, nscan * P) for _ in range(2)]
    assert np.array_equal(out[0], out[1])
    assert np.all(out[0][[0, -1]] == 7.0)
    got = out[0][1:-1].astype(np.float64)
    ratio = np.abs(got - want) / absum
    cancel = np.abs(want) / absum
    print(f"scan gradient over slices ({nscan}, {D}, {pw}, {H}, {W}): max "
          f"|err| / A_n = {ratio.max():.2e}; |sum| / A_n from "
          f"{cancel.min():.1e}")
    assert np.all(ratio <= 1e-7), ratio
    # rows of a wider workspace, marked where no plane lies
    wide = torch.full((D, nscan + 3, pw, pw), float("nan"),
                      dtype=torch.complex64, device=dev)
    wide[:, :nscan] = q_d
    assert np.array_equal(call(wide, (nscan + 3) * P), out[0])
    # one slice: the bits of tike_scan_gradient, for every slice
    for s in range(D):
        one = call(q_d[s], nscan * P, slices=1, first=s)
        guard.fill_(7.0)
        check(
            lib.tike_scan_gradient(A.ptr(q_d[s]), A.ptr(scan_d),
                                   A.ptr(psi_d[s]), A.ptr(guard[1:]), nscan,
                                   pw, H, W, A.stream_ptr()),
            "tike_scan_gradient")
        assert np.array_equal(one, guard.cpu().numpy())


def test_scan_gradient_slices_arguments():
    """TIKE_ERR_ARG before any launch; no position: 0 and nothing written."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import ERR_ARG, lib
    dev = torch.device("cuda")
    q = torch.zeros((2, 3, 8, 8), dtype=torch.complex64, device=dev)
    psi = torch.zeros((2, 24, 24), dtype=torch.complex64, device=dev)
    scan = torch.full((3, 2), 2.5, device=dev)
    grad = torch.full((3, 2), 7.0, device=dev)
    ok = [A.ptr(q), 3 * 64, A.ptr(scan), A.ptr(psi), A.ptr(grad), 3, 2, 8, 24,
          24, A.stream_ptr()]

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.tike_scan_gradient_slices(*args)
    for k in (0, 2, 3, 4):
        assert call(**{f"a{k}": None}) == ERR_ARG
    assert call(a1=3 * 64 - 1) == ERR_ARG
    assert call(a5=-1) == ERR_ARG
    assert call(a5=1 << 31, a1=1 << 40) == ERR_ARG
    for k in (6, 7, 8, 9):
        assert call(**{f"a{k}": 0}) == ERR_ARG
    assert call(a5=0) == 0
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((grad == 0.0).all())


# ------------------------------- the inverse pass 1 that takes the table
@pytest.mark.parametrize("P", [1, 6])
@pytest.mark.parametrize("det", [128, 256, 512])
def test_scaled_pass1_hands_over_what_the_step_back_reads(det, P):
    """`tike_ifft2_pass1_scaled` (the table applied while inverse pass 1
    loads; P = S * fly planes share a frame's table) leaves in `work` what
    `tike_farplane_scale` followed by `tike_fft2_pass1(inverse)` leaves --
    the input `tike_slice_step_back` and `tike_ifft2_pass2_products` read --
    to 1e-6 normwise: the same pass-1 engine behind another load."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    rng = np.random.default_rng(det + P)
    nframe = 2
    ntile = nframe * P
    dev = torch.device("cuda")
    far = torch.from_numpy(mm.rc(rng, ntile, det, det)).to(dev)
    table = torch.from_numpy(rng.standard_normal(
        (nframe, det, det)).astype(np.float32)).to(dev)
    st = A.stream_ptr()
    got = torch.zeros_like(far)
    check(
        lib.tike_ifft2_pass1_scaled(A.ptr(far), A.ptr(table), None, None, P,
                                    A.ptr(got), ntile, det, st),
        "tike_ifft2_pass1_scaled")
    scaled = far.clone()
    check(
        lib.tike_farplane_scale(A.ptr(scaled), A.ptr(table), nframe, P,
                                det * det, 1.0, st), "tike_farplane_scale")
    want = torch.zeros_like(far)
    check(lib.tike_fft2_pass1(A.ptr(scaled), A.ptr(want), ntile, det, 1, st),
          "tike_fft2_pass1")
    got, want = got.cpu().numpy(), want.cpu().numpy()
    e = relerr(got, want)
    print(f"scaled inverse pass 1 ({det}, P = {P}): normwise {e:.2e}")
    assert np.abs(want).max() > 0
    assert e <= 1e-6


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _case(shape, norm="ortho"):
    """Host inputs and the float64 model's intensity and gradients --
    computed once, shared, left unchanged."""
    c = mm.case(*shape, norm=norm)
    return dict(c, **mm.case_model(c))


def _run(case, needs=(True, True, True), function=None):
    """(intensity, psi.grad, probe.grad, scan.grad) of sum(g * intensity) on
    the GPU, as host arrays (None where no gradient was asked for)."""
    import torch

    import tike_amd.operators as ops
    from tike_amd.autograd import multislice_intensity
    function = function or multislice_intensity
    dev = torch.device("cuda")
    leaves = [torch.from_numpy(case[k]).to(dev).requires_grad_(r)
              for k, r in zip(("psi", "probe", "scan"), needs)]
    psi, probe, scan = leaves
    pw = probe.shape[-1]
    with ops.Ptycho(probe_shape=pw, detector_shape=pw, nz=psi.shape[-2],
                    n=psi.shape[-1], norm=case["norm"], **mm.optics(pw)) as op:
        inten = function(op, psi, probe, scan, fly=case["fly"])
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
    if gpsi is not None:
        lines.append("psi.grad per slice " + " ".join(
            f"{relerr(gpsi[d], case['grad_psi'][d]):.2e}"
            for d in range(gpsi.shape[0])))
    if gscan is not None:
        ratio = np.abs(gscan - case["grad_scan"]) / case["grad_A"]
        lines.append(f"scan.grad max |err| / A_n {ratio.max():.2e}")
    print("; ".join(lines))
    assert_close(inten, case["intensity"], OP_NORMWISE, OP_MAXABS,
                 what + " intensity")
    for name, x, need in (("psi", gpsi, needs[0]), ("probe", gprobe, needs[1])):
        assert (x is not None) == need, (what, name)
        if need:
            assert x.shape == case[name].shape and x.dtype == np.complex64
            assert_close(x, case["grad_" + name], OP_NORMWISE, OP_MAXABS,
                         f"{what} {name}.grad")
    if needs[0]:
        for d in range(gpsi.shape[0]):  # every slice on its own
            assert_close(gpsi[d], case["grad_psi"][d], OP_NORMWISE, OP_MAXABS,
                         f"{what} psi.grad[{d}]")
    assert (gscan is not None) == needs[2], what
    if needs[2]:
        assert gscan.shape == case["scan"].shape and gscan.dtype == np.float32
        assert np.all(ratio <= mm.SCAN_BAR), (what, ratio)


@pytest.mark.parametrize("shape", mm.END_TO_END_CASES)
def test_intensity_and_gradients_vs_model(shape):
    """Intensity, probe.grad and psi.grad -- whole and every slice on its own
    -- within the operator bars (normwise 1e-5, max-abs 1e-4), scan.grad
    within `mm.SCAN_BAR` A_n per position and coordinate; the float32
    restatement of the formulas on the CPU and what the GPU reaches are in
    profiles/autograd_multislice.md."""
    case = _case(shape)
    _assert_matches(case, _run(case), str(shape))


# ------------------------------------------------------- routes and switches
FUSED = (6, 2, 128, 170, 2, 2)
GENERAL = (6, 2, 32, 72, 2, 2)


def test_routes_agree_at_128(monkeypatch):
    """The fused route, the same with the three-launch step back, the same
    with the table applied by `tike_farplane_scale`, and the general route:
    each within the bars of the model, and within 1e-5 normwise of the fused
    route (scan.grad, whose terms cancel: within 2 SCAN_BAR A_n, each route
    being within one)."""
    import importlib

    from tike_amd import autograd
    # (the package exports the solver function under the module's name)
    cgrad = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    case = _case(FUSED)
    assert cgrad.MULTISLICE_FUSED and cgrad.MULTISLICE_STEP_BACK_FUSED
    assert autograd.PASS1_TAKES_TABLE
    fused = _run(case)
    _assert_matches(case, fused, "fused")
    for name, (module, lever) in dict(
            three_launches=(cgrad, "MULTISLICE_STEP_BACK_FUSED"),
            two_launch_table=(autograd, "PASS1_TAKES_TABLE"),
            general=(cgrad, "MULTISLICE_FUSED")).items():
        with monkeypatch.context() as m:
            m.setattr(module, lever, False)
            other = _run(case)
        _assert_matches(case, other, name)
        errs = [relerr(b, a) for a, b in zip(fused[:3], other[:3])]
        ratio = np.abs(other[3] - fused[3]) / case["grad_A"]
        print(f"{name} against fused: " + " ".join(f"{e:.2e}" for e in errs)
              + f"; scan / A_n {ratio.max():.2e}")
        assert max(errs) <= 1e-5, (name, errs)
        assert np.all(ratio <= 2 * mm.SCAN_BAR), (name, ratio)


@pytest.mark.parametrize("shape", [(12, 2, 32, 72, 2, 2),
                                   (12, 2, 128, 170, 3, 2)])
def test_three_chunks(shape, monkeypatch):
    """The positions cut into three chunks of whole frames give what one
    chunk gives, forward and backward, to 1e-6: the chunks only regroup sums
    over the positions."""
    from tike_amd.ptycho.solvers import lstsq
    case = _case(shape)
    whole = _run(case)
    monkeypatch.setattr(lstsq, "CHUNK_POSITIONS_OVERRIDE", 5)
    # (5 positions: frames of two are kept whole, 4 + 4 + 4)
    cut = _run(case)
    _assert_matches(case, cut, f"{shape} in three chunks")
    errs = [relerr(b, a) for a, b in zip(whole, cut)]
    print("three chunks against one: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-6, errs


@pytest.mark.parametrize("shape", [GENERAL, FUSED])
@pytest.mark.parametrize("norm", ["backward", "forward"])
def test_other_norms(norm, shape):
    """The operator's norm is honoured on both routes: the last transform's
    adjoint is F^H, the unscaled inverse times the FORWARD scale -- the
    operator's own inverse would be wrong by det^2 -- and the Fresnel steps
    do not depend on it."""
    case = _case(shape, norm)
    _assert_matches(case, _run(case), f"{shape} norm={norm}")


@pytest.mark.parametrize("shape", [GENERAL, FUSED])
@pytest.mark.parametrize("needs", [(False, False, True), (True, False, False),
                                   (False, True, False)])
def test_only_one_input_requires_a_gradient(needs, shape):
    """The other .grads are None and the computed one is what it is when all
    three are asked for."""
    case = _case(shape)
    full = _run(case)
    part = _run(case, needs=needs)
    _assert_matches(case, part, f"{shape} needs={needs}", needs)
    assert np.array_equal(full[0], part[0])
    for a, b, need in zip(full[1:], part[1:], needs):
        if need and a.dtype == np.float32:  # scan.grad: no atomics
            assert np.array_equal(a, b)
        elif need:
            assert relerr(b, a) <= 1e-6


@pytest.mark.parametrize("N,fly", [(1, 1), (6, 2)])
def test_one_slice_goes_through_intensity(N, fly):
    """D = 1: the bits of `intensity` -- the intensity and scan.grad for any
    number of positions, psi.grad and probe.grad where every address has one
    contributor (one position; with more the float atomics of the scatter
    and of the sum over the positions may add in another order: 1e-6)."""
    from tike_amd.autograd import intensity
    case = mm.case(N, 2, 32, 72, 1, fly)
    want = _run(case, function=intensity)
    got = _run(case)
    assert got[1].shape == (1, 72, 72)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])
    for a, b in zip(got[1:3], want[1:3]):
        if N == 1:
            assert np.array_equal(a, b)
        assert relerr(a, b) <= 1e-6


# ----------------------------------------------------------- position recovery
def test_adam_recovers_positions_of_a_two_slice_object():
    """`mm.problem()`: the 14 x 14 raster of `autograd_model.problem`, pw = 32,
    fly = 2, true positions +- 0.3 px, behind the smooth object a second slice
    of cgrad's recipe; `mm.RECOVERY` steps of Adam(lr) on scan alone with the
    gaussian amplitude loss -- the combination cgrad refuses.  The float64
    model alone at least halves the RMS position error (asserted in
    test_autograd_multislice_cpu.py); the GPU run is held to the model with
    the bars of `test_adam_recovers_fly_scan_positions`: its final positions
    lie within 0.25 of the model's own remaining RMS error of the model's
    final positions, every cost of its history within 1 % of the model's, and
    it halves the RMS error itself."""
    import torch

    import tike_amd.operators as ops
    from tike_amd.autograd import multislice_intensity
    p = mm.problem(seed=mm.RECOVERY["seed"])
    model_final, model_costs = mm.recover_on_model(p)
    dev = torch.device("cuda")
    psi, probe, data, start = (torch.from_numpy(p[k]).to(dev) for k in (
        "psi", "probe", "data", "scan_start"))
    pw = p["det"]
    with ops.Ptycho(probe_shape=pw, detector_shape=pw, nz=psi.shape[-2],
                    n=psi.shape[-1], **mm.optics(pw)) as op:
        final, costs = am.recover(
            lambda s: am.amplitude_loss(
                multislice_intensity(op, psi, probe, s, fly=p["fly"]), data),
            start, steps=mm.RECOVERY["steps"], lr=mm.RECOVERY["lr"])
    r0 = am.rms(p["scan_start"], p["scan_true"])
    r1 = am.rms(final, p["scan_true"])
    rm = am.rms(model_final, p["scan_true"])
    apart = am.rms(final, model_final)
    history = np.abs(np.array(costs) / np.array(model_costs) - 1).max()
    print(f"position recovery: rms {r0:.3f} -> {r1:.3f} ({r1 / r0:.3f}; the "
          f"model {rm:.3f}); {apart:.2e} px rms from the model's final "
          f"positions; cost {costs[0]:.2e} -> {costs[-1]:.2e} "
          f"({costs[-1] / costs[0]:.4f}), worst step {history:.2e} from the "
          "model's history")
    assert np.isfinite(costs).all()
    assert r1 <= 0.5 * r0, (r0, r1)
    assert apart <= 0.25 * rm, (apart, rm)
    assert history <= 0.01, history
