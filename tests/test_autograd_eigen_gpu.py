"""`tike_amd.autograd.intensity` with eigen probes on the GPU against the
float64 model (tests/autograd_eigen.py): `tike_eigen_probe_gradients` on its
own, the forward and the five gradients end to end, other configurations, and
recovery of the eigen weights of a drifting probe on fly-scan data by
`torch.optim.Adam`.

Every figure a bar is set on is printed before it is asserted."""
import numpy as np
import pytest

import autograd_eigen as ae
import autograd_model as am
from util import OP_MAXABS, OP_NORMWISE, assert_close, maxerr, relerr

pytestmark = pytest.mark.gpu

PLANES = ("probe", "eigen", "objproj")
OUTPUTS = ("probe", "eigen", "weights", "objproj")


# ------------------------------------------- the entry alone
def _entry(c, shape, outputs=OUTPUTS, start=None, guard=7.0):
    """One call of tike_eigen_probe_gradients on a case: dict of host arrays
    for `outputs` (the others are handed in as NULL).  start: dict of host
    arrays the plane sums start from (zeros otherwise).  weights and objproj
    come back with one guard row in front and one behind."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    nscan, S, M, C, pw, H, W = shape
    dev = A.current_device()
    d = lambda a: None if a is None else torch.from_numpy(
        np.ascontiguousarray(a)).to(dev)
    chi, scan, psi, probe, eigen, w = (d(c[k]) for k in (
        "chi", "scan", "psi", "probe", "eigen", "weights"))
    out = dict.fromkeys(OUTPUTS)
    start = start or {}
    if "probe" in outputs:
        out["probe"] = d(start.get("probe", np.zeros_like(c["probe"])))
    if "eigen" in outputs and C:
        out["eigen"] = d(start.get("eigen", np.zeros_like(c["eigen"])))
    if "weights" in outputs:
        out["weights"] = torch.full((nscan + 2, C + 1, S), guard,
                                    dtype=torch.float32, device=dev)
    if "objproj" in outputs:
        out["objproj"] = torch.full((nscan + 2, pw, pw), guard,
                                    dtype=torch.complex64, device=dev)
    ntile = -(-pw * pw // 256)
    # the size include/tike_amd.h states, in float64 elements
    work = torch.empty(ntile * nscan * (S + C * M), dtype=torch.float64,
                       device=dev) if "weights" in outputs else None
    inner = lambda t: None if t is None else t[1:]
    check(
        lib.tike_eigen_probe_gradients(
            A.ptr(chi), A.ptr(scan), A.ptr(psi), A.ptr(probe), A.ptr(eigen),
            A.ptr(w), C, M, A.ptr(out["probe"]), A.ptr(out["eigen"]),
            A.ptr(inner(out["weights"])), A.ptr(inner(out["objproj"])),
            A.ptr(work), nscan, S, pw, H, W, A.stream_ptr()),
        "tike_eigen_probe_gradients")
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _strip(got):
    """The outputs without their guard rows, which must be untouched."""
    for k in ("weights", "objproj"):
        if got[k] is not None:
            assert np.all(got[k][[0, -1]] == 7.0), k
            got[k] = got[k][1:-1]
    return got


@pytest.mark.parametrize("shape", ae.ENTRY_CASES
                         + ae.ENTRY_CASES_EVERY_KERNEL)
def test_entry_vs_float64_model(shape):
    """On the same float32 chi.  objproj, probe_grad and eigen_grad within the
    operator bars (normwise 1e-5, max-abs 1e-4); weights_grad within 1e-7 A
    per entry, A the sum of the absolute terms -- the bar `tike_scan_gradient`
    alone is held to: float32 products with float64 sums stay at 2.2e-9 to
    1.7e-8 A on the CPU at these shapes, below a third of the bar
    (test_autograd_eigen_cpu.py asserts it), and the block of modes without
    an eigen probe is exactly 0.  Two calls give the same weights_grad and
    objproj bit for bit; the plane sums are `+=` on a start that is not zero;
    the rows next to weights_grad and objproj are not written."""
    nscan, S, M, C, pw, H, W = shape
    c = ae.entry_case(*shape)
    want = c["want"]
    got = _strip(_entry(c, shape))
    again = _strip(_entry(c, shape))
    live = want["A"] > 0
    ratio = (np.abs(got["weights"].astype(np.float64) - want["weights"])[live]
             / want["A"][live])
    line = [f"entry {shape}: weights / A {ratio.max():.2e}"]
    for k in PLANES:
        if want[k] is not None:
            line.append(f"{k} normwise {relerr(got[k], want[k]):.2e} max-abs "
                        f"{maxerr(got[k], want[k]):.2e}")
    print("; ".join(line))
    assert got["weights"].dtype == np.float32
    assert got["weights"].shape == (nscan, C + 1, S)
    assert np.all(ratio <= ae.WEIGHTS_ENTRY_BAR), ratio.max()
    assert np.all(got["weights"][~live] == 0)
    assert np.all(live[:, 0]) and np.all(live[:, 1:, :M])
    assert not np.any(live[:, 1:, M:])
    for k in PLANES:
        if want[k] is None:
            assert got[k] is None and C == 0
            continue
        assert_close(got[k], want[k], OP_NORMWISE, OP_MAXABS, f"{shape} {k}")
    # no atomics in the weight sums, one writer per objproj pixel
    assert np.array_equal(got["weights"], again["weights"])
    assert np.array_equal(got["objproj"].view(np.float32),
                          again["objproj"].view(np.float32))
    # += on a start of the result's own size
    rng = np.random.default_rng(5)
    start = {k: (ae.rc(rng, *want[k].shape) * np.abs(want[k]).mean()).astype(
        np.complex64) for k in ("probe", "eigen") if want[k] is not None}
    added = _entry(c, shape, outputs=("probe", "eigen"), start=start)
    for k, s in start.items():
        assert_close(added[k], s.astype(np.complex128) + want[k], OP_NORMWISE,
                     OP_MAXABS, f"{shape} {k} +=")
        assert relerr(added[k], got[k]) > 0.1  # (the start was not lost)


@pytest.mark.parametrize("shape", [ae.ENTRY_CASES[1], ae.ENTRY_CASES[3],
                                   ae.ENTRY_CASES_EVERY_KERNEL[11]])
@pytest.mark.parametrize("without", OUTPUTS)
def test_entry_with_one_output_missing(shape, without):
    """Every single NULL output leaves weights_grad and objproj as they are
    bit for bit and the atomic plane sums within 1e-6 normwise."""
    c = ae.entry_case(*shape)
    full = _strip(_entry(c, shape))
    part = _strip(_entry(c, shape, tuple(k for k in OUTPUTS if k != without)))
    assert part[without] is None
    for k in ("weights", "objproj"):
        if k != without:
            assert np.array_equal(part[k].view(np.float32),
                                  full[k].view(np.float32)), k
    for k in ("probe", "eigen"):
        if k != without:
            err = relerr(part[k], full[k])
            print(f"{shape} without {without}: {k} {err:.2e}")
            assert err <= 1e-6, k


def test_entry_refuses_more_than_sixteen_planes():
    """TIKE_ERR_UNSUPPORTED for C * M = 17, before anything is launched."""
    from tike_amd._lib import ERR_UNSUPPORTED
    shape = ae.ENTRY_CASES[0]
    c = dict(ae.entry_case(*shape))
    with pytest.raises(ValueError, match="unsupported size"):
        _entry(c, shape[:2] + (1, 17) + shape[4:])
    assert ERR_UNSUPPORTED == 1000002


# ------------------------------------------------------------------ end to end
LEAVES = ("psi", "probe", "scan", "eigen", "weights")


def _run(c, det, fly, norm="ortho", needs=(True,) * 5, eigen=True):
    """(intensity, {leaf: .grad}) of sum(g * intensity) on the GPU, as host
    arrays (None where no gradient was asked for).  eigen=False: the call
    without the keywords."""
    import torch

    import tike_amd.operators as ops
    from tike_amd.autograd import intensity
    dev = torch.device("cuda")
    leaves = {k: None if c[k] is None else torch.from_numpy(c[k]).to(
        dev).requires_grad_(r) for k, r in zip(LEAVES, needs)}
    psi, probe, scan = leaves["psi"], leaves["probe"], leaves["scan"]
    kw = dict(eigen_probe=leaves["eigen"],
              eigen_weights=leaves["weights"]) if eigen else {}
    with ops.Ptycho(probe_shape=probe.shape[-1], detector_shape=det,
                    nz=psi.shape[-2], n=psi.shape[-1], norm=norm) as op:
        inten = intensity(op, psi, probe, scan, fly=fly, **kw)
        assert inten.dtype == torch.float32
        (inten * torch.from_numpy(c["g"]).to(dev)).sum().backward()
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    return host(inten), {k: None if v is None else host(v.grad)
                         for k, v in leaves.items()}


def _assert_matches(c, got, what, needs=(True,) * 5):
    inten, grads = got
    want = c["want"]
    lines = [f"{what}: intensity normwise {relerr(inten, c['intensity']):.2e}"
             f" max-abs {maxerr(inten, c['intensity']):.2e}"]
    ratio = sratio = None
    for k in ("psi", "probe", "eigen"):
        if grads[k] is not None:
            lines.append(f"{k}.grad normwise {relerr(grads[k], want[k]):.2e} "
                         f"max-abs {maxerr(grads[k], want[k]):.2e}")
    if grads["weights"] is not None:
        live = want["A"] > 0
        ratio = (np.abs(grads["weights"] - want["weights"])[live]
                 / want["A"][live])
        lines.append(f"eigen_weights.grad max |err| / A {ratio.max():.2e}")
    if grads["scan"] is not None:
        sratio = np.abs(grads["scan"] - want["scan"]) / want["A_scan"]
        lines.append(f"scan.grad max |err| / A_n {sratio.max():.2e}")
    print("; ".join(lines))
    assert_close(inten, c["intensity"], OP_NORMWISE, OP_MAXABS,
                 what + " intensity")
    for k, need in zip(LEAVES, needs):
        assert (grads[k] is not None) == (need and c[k] is not None), (what, k)
        if grads[k] is not None:
            assert grads[k].shape == c[k].shape and grads[k].dtype == c[k].dtype
    for k in ("psi", "probe", "eigen"):
        if grads[k] is not None:
            assert_close(grads[k], want[k], OP_NORMWISE, OP_MAXABS,
                         f"{what} {k}.grad")
    if ratio is not None:
        assert np.all(ratio <= ae.WEIGHTS_BAR), (what, ratio.max())
        assert np.all(grads["weights"][want["A"] == 0] == 0)
    if sratio is not None:
        assert np.all(sratio <= ae.SCAN_BAR), (what, sratio.max())


@pytest.mark.parametrize("shape", ae.END_TO_END_CASES
                         + ae.END_TO_END_CASES_MORE)
def test_intensity_and_gradients_vs_model(shape):
    """Intensity, psi.grad, probe.grad and eigen_probe.grad within the
    operator bars (normwise 1e-5, max-abs 1e-4); eigen_weights.grad within
    1e-6 A per entry and scan.grad within 1e-6 A_n, the project's end-to-end
    bars (a complex64 restatement of the whole model on the CPU stays at
    2.1 - 2.5e-7 normwise for the planes, 5.4e-8 A for the weights and
    2.3e-8 A_n for the positions at exactly these shapes and inputs; the
    issue quotes 1.8 - 2.1e-7 and 4.4e-8 A for its own inputs)."""
    N, S, M, C, pw, det, H, fly = shape
    c = ae.case(*shape)
    _assert_matches(c, _run(c, det, fly), str(shape))


# --------------------------------------------------------- other configurations
CONFIG = (12, 2, 1, 2, 16, 20, 40, 2)  # N, S, M, C, pw, det, H, fly


def test_three_chunks(monkeypatch):
    """Three chunks of whole frames: the same intensity, scan.grad and
    eigen_weights.grad bit for bit (the chunks only regroup sums over the
    positions), the plane sums within the bars."""
    from tike_amd.ptycho.solvers import lstsq
    N, S, M, C, pw, det, H, fly = CONFIG
    c = ae.case(*CONFIG)
    whole = _run(c, det, fly)
    monkeypatch.setattr(lstsq, "CHUNK_POSITIONS_OVERRIDE", 4)
    assert max(1, lstsq.chunk_positions(S, det) // fly) * fly * 3 == N
    cut = _run(c, det, fly)
    _assert_matches(c, cut, "three chunks")
    assert np.array_equal(whole[0], cut[0])
    assert np.array_equal(whole[1]["scan"], cut[1]["scan"])
    assert np.array_equal(whole[1]["weights"], cut[1]["weights"])


@pytest.mark.parametrize("det", [20, 128])
@pytest.mark.parametrize("norm", ["backward", "forward"])
def test_other_norms(norm, det):
    """The operator's norm is honoured on both routes of the inverse."""
    shape = CONFIG if det == 20 else (4, 2, 1, 1, 100, 128, 240, 2)
    c = ae.case(*shape, norm)
    _assert_matches(c, _run(c, det, shape[-1], norm), f"norm={norm} det={det}")


@pytest.mark.parametrize("only", range(5))
def test_only_one_input_requires_a_gradient(only):
    """The other .grads are None and the computed one is what it is when all
    five are asked for."""
    N, S, M, C, pw, det, H, fly = CONFIG
    c = ae.case(*CONFIG)
    needs = tuple(i == only for i in range(5))
    full = _run(c, det, fly)
    part = _run(c, det, fly, needs=needs)
    _assert_matches(c, part, f"only {LEAVES[only]}", needs)
    a, b = full[1][LEAVES[only]], part[1][LEAVES[only]]
    if a.dtype == np.float32:  # scan.grad, eigen_weights.grad: no atomics
        assert np.array_equal(a, b)
    else:
        assert relerr(b, a) <= 1e-6


def test_without_the_keywords_nothing_changes():
    """eigen_weights=None is the call without the keywords: the same
    intensity and scan.grad bit for bit, the plane gradients within 1e-6
    normwise (their atomics)."""
    N, S, M, C, pw, det, H, fly = CONFIG
    c = dict(ae.case(*CONFIG))
    plain = _run(c, det, fly, eigen=False)
    c["eigen"] = c["weights"] = None
    none = _run(c, det, fly)
    assert none[1]["eigen"] is None and none[1]["weights"] is None
    assert np.array_equal(plain[0], none[0])
    assert np.array_equal(plain[1]["scan"], none[1]["scan"])
    for k in ("psi", "probe"):
        assert relerr(none[1][k], plain[1][k]) <= 1e-6, k


def test_unit_weights_and_zero_eigen_probes_give_the_shared_probe():
    """Weights all ones and eigen probes zero: the intensities of the
    shared-probe call within the operator bars."""
    N, S, M, C, pw, det, H, fly = CONFIG
    c = dict(ae.case(*CONFIG))
    plain = _run(c, det, fly, eigen=False)[0]
    c["eigen"] = np.zeros_like(c["eigen"])
    c["weights"] = np.ones_like(c["weights"])
    got = _run(c, det, fly)[0]
    print(f"unit weights: normwise {relerr(got, plain):.2e} max-abs "
          f"{maxerr(got, plain):.2e}")
    assert_close(got, plain, OP_NORMWISE, OP_MAXABS, "unit weights")


def test_deterministic_mode_gives_the_same_bits():
    """With TIKE_DETERMINISTIC=1 two backward calls give bit-identical
    gradients for all five inputs, over several chunks of the plane sums;
    without it the weight and scan gradients still do."""
    from tike_amd import _lib
    # (200 positions: three chunks of the plane sums, 96 + 96 + 8)
    shape = (200, 2, 1, 1, 16, 20, 40, 2)
    c = ae.case(*shape)
    a, b = _run(c, 20, 2), _run(c, 20, 2)
    _assert_matches(c, a, f"deterministic={_lib.DETERMINISTIC}")
    assert np.array_equal(a[0], b[0])
    for k in LEAVES if _lib.DETERMINISTIC else ("scan", "weights"):
        assert np.array_equal(a[1][k].view(np.float32),
                              b[1][k].view(np.float32)), k


# ------------------------------------------------------------ weight recovery
def test_adam_recovers_the_eigen_weights_of_fly_scan_data():
    """`ae.problem(seed=0)`: 14 x 14 raster, pw = det = 32, fly = 2, one eigen
    probe (the probe drifting sideways), true weights +-0.3; 60 steps of
    Adam(lr=0.05) on eigen_weights alone with the gaussian amplitude loss.
    Final RMS error over all weight entries <= 0.35 of its start and cost
    below 1 % of its start (the float64 model reaches 0.19 and 0.17 %)."""
    import torch

    import tike_amd.operators as ops
    from tike_amd.autograd import intensity
    p = ae.problem(seed=0)
    dev = torch.device("cuda")
    psi, probe, scan, eigen, data, start = (
        torch.from_numpy(p[k]).to(dev) for k in (
            "psi", "probe", "scan_true", "eigen", "data", "weights_start"))
    with ops.Ptycho(probe_shape=p["det"], detector_shape=p["det"],
                    nz=psi.shape[-2], n=psi.shape[-1]) as op:
        final, costs = ae.recover(
            lambda w: am.amplitude_loss(
                intensity(op, psi, probe, scan, eigen_probe=eigen,
                          eigen_weights=w, fly=p["fly"]), data), start)
    r0 = ae.weights_rms(p["weights_start"], p["weights_true"])
    r1 = ae.weights_rms(final, p["weights_true"])
    print(f"weight recovery: rms {r0:.4f} -> {r1:.4f} ({r1 / r0:.3f}), cost "
          f"{costs[0]:.2e} -> {costs[-1]:.2e} ({costs[-1] / costs[0]:.5f})")
    assert np.isfinite(costs).all() and len(costs) == ae.RECOVERY["steps"]
    assert r1 <= ae.RECOVERY["rms"] * r0, (r0, r1)
    assert costs[-1] < ae.RECOVERY["cost"] * costs[0], (costs[0], costs[-1])
