"""Gradient-of-intensity position refinement on the GPU: the sums kernel
through the C ABI against float64 NumPy, `position_pd_shifts` /
`update_positions_pd` / `Reconstruction.update_positions_pd` against the
float64 evaluation of tests/position_pd.py (pinned to the reference's own run
by test_position_pd_cpu.py) and against the fixture of that run.

Bars: 1e-5 normwise for the kernel's sums (the operator bar, tests/util.py);
2e-5 normwise for `grad` (30 x the reference's own float32 distance from
float64, left for another summation order and the hand-written transforms);
3.8e-6 px = 4 ulp at 16 for positions against the fixture."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import position_pd as pp
from util import OP_NORMWISE

pytestmark = pytest.mark.gpu

GRAD_NORMWISE = 2e-5
POSITION_ATOL = 3.8e-6


@pytest.fixture(scope="module")
def tp():
    import tike_amd.ptycho as m
    return m


def _operator(P, slices=1):
    from tike_amd.operators import Ptycho
    pw = P["probe"].shape[-1]
    optics = {} if slices == 1 else dict(
        probe_wavelength=pp.PHYS["wavelength"],
        probe_FOV_lengths=pp.PHYS["fov"],
        multislice_propagation_distance=pp.PHYS["distance"])
    return Ptycho(P["det"], pw, nz=P["psi"].shape[-2], n=P["psi"].shape[-1],
                  **optics)


# ------------------------------------------------------------------ the entry
def _planes(rng, nscan, S, npix, u16):
    """Random far planes whose displaced copies differ by a third, data near
    the intensity (counts in the hundreds when they are rounded)."""
    def c(*shape):
        return (rng.standard_normal(shape, dtype=np.float32) +
                1j * rng.standard_normal(shape, dtype=np.float32))
    amp = np.float32(10.0 if u16 else 1.0)
    far0 = amp * c(nscan, S, npix)
    far_dx = far0 + amp * np.float32(0.3) * c(nscan, S, npix)
    far_dy = far0 + amp * np.float32(0.3) * c(nscan, S, npix)
    inten = np.sum(np.abs(far0)**2, axis=1)
    data = np.maximum(inten * (1 + 0.2 * rng.standard_normal(
        inten.shape, dtype=np.float32)), 0)
    data = np.rint(data).astype(np.uint16) if u16 else data.astype(np.float32)
    return far0, far_dx, far_dy, data


def _run_entry(far0, far_dx, far_dy, data, inv_dx, with_costs=True):
    import torch
    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    nscan, S, npix = far0.shape
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda()
           for f in (far0, far_dx, far_dy)]
    if data.dtype == np.uint16:
        d = torch.from_numpy(data.view(np.int16)).cuda().view(torch.uint16)
    else:
        d = torch.from_numpy(data).cuda()
    sums = torch.full((max(nscan, 1), 5), np.nan, dtype=torch.float32,
                      device="cuda")
    costs = torch.full((max(nscan, 1),), np.nan, dtype=torch.float32,
                       device="cuda")
    check(lib.tike_position_pd_sums(
        A.ptr(dev[0]), A.ptr(dev[1]), A.ptr(dev[2]), A.ptr(d),
        int(data.dtype == np.uint16), inv_dx, A.ptr(sums),
        A.ptr(costs) if with_costs else None, nscan, S, npix,
        A.stream_ptr()), "tike_position_pd_sums")
    torch.cuda.synchronize()
    return sums[:nscan].cpu().numpy(), costs[:nscan].cpu().numpy()


def _assert_sums(got, want, what):
    sums, costs = got
    ref_sums, ref_costs = want
    for k, name in enumerate(("aa", "ab", "bb", "ar", "br")):
        miss = pp.relerr(sums[:, k], ref_sums[:, k])
        print(f"{what}: sum {name} normwise {miss:.2e}")
        assert miss <= OP_NORMWISE, (what, name, miss)
    miss = pp.relerr(costs, ref_costs)
    print(f"{what}: costs normwise {miss:.2e}")
    assert miss <= OP_NORMWISE, (what, miss)


# (24^2 is below one vector sweep of a workgroup, 100^2 no multiple of the
# vector width x 64, S = 3 odd; 70 x 8 x 256^2 alone is left out: 880 MB of
# far planes for nothing the other 26 do not reach)
ENTRY_SHAPES = [s for s in itertools.product((1, 5, 70), (1, 3, 8),
                                             (576, 10000, 65536))
                if s[0] * s[1] * s[2] <= 1 << 24]
# 25^2: rows that start off a 16-byte boundary, and a scalar tail
ENTRY_SHAPES += [(3, 2, 625), (2, 1, 7)]


@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("nscan,S,npix", ENTRY_SHAPES)
def test_sums_entry_vs_float64(nscan, S, npix, u16):
    rng = np.random.default_rng(nscan + 10 * S + npix)
    planes = _planes(rng, nscan, S, npix, u16)
    got = _run_entry(*planes, -1.0)
    _assert_sums(got, pp.sums_f64(*planes, -1.0),
                 f"{nscan} x {S} x {npix} u16 {u16}")
    again = _run_entry(*planes, -1.0)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1],
                                                               again[1])
    # costs = NULL: the sums alone, the same bits
    bare = _run_entry(*planes, -1.0, with_costs=False)
    assert np.array_equal(got[0], bare[0]) and np.all(np.isnan(bare[1]))


@pytest.mark.parametrize("npix", [625, 10000])
def test_sums_entry_keeps_the_last_pixel(npix):
    """The last pixel of the last mode carries half of sum a^2: a dropped
    tail (scalar at 625, a partly filled vector sweep at 10 000) shows."""
    nscan, S = 3, 3
    rng = np.random.default_rng(npix)
    far0, far_dx, far_dy, data = _planes(rng, nscan, S, npix, False)
    for f in (far0, far_dx, far_dy):
        f[:, :, -1] = 0
    rest = pp.sums_f64(far0, far_dx, far_dy, data, 0.5)[0][:, 0]
    # a of the last pixel = inv_dx * 2 * t^2 with far_dy = 0 there
    far0[:, -1, -1] = np.sqrt(np.sqrt(rest)).astype(np.float32)
    far_dx[:, -1, -1] = far0[:, -1, -1]
    want = pp.sums_f64(far0, far_dx, far_dy, data, 0.5)
    share = 1 - rest / want[0][:, 0]
    assert np.all((share > 0.45) & (share < 0.55)), share
    _assert_sums(_run_entry(far0, far_dx, far_dy, data, 0.5), want,
                 f"last pixel, npix {npix}")


def test_sums_entry_arguments():
    import torch
    from tike_amd._lib import ERR_ARG, lib
    z = torch.zeros(64, device="cuda").data_ptr()
    call = lambda *, f=z, d=z, s=z, n=0, S=1, npix=4: (  # noqa: E731
        lib.tike_position_pd_sums(f, z, z, d, 0, -1.0, s, None, n, S, npix,
                                  None))
    assert call() == 0  # no positions: nothing is launched
    assert call(f=None, n=1) == ERR_ARG
    assert call(d=None, n=1) == ERR_ARG
    assert call(s=None, n=1) == ERR_ARG
    assert call(S=0, n=1) == ERR_ARG
    assert call(npix=0, n=1) == ERR_ARG


# ---------------------------------------------------------- position_pd_shifts
_EVALUATED = {}


def _case(det, pw, S, N, **kw):
    """(problem, float64 evaluation at step 0.5), computed once per shape."""
    key = (det, pw, S, N, tuple(sorted(kw.items())))
    if key not in _EVALUATED:
        P = pp.problem(det, pw, S, N, **kw)
        _EVALUATED[key] = P, pp.evaluate(
            P["data"], P["psi"], P.get("varying", P["probe"]), P["scan"],
            det, step=0.5, prop=P["prop"])
    return _EVALUATED[key]


SHIFT_SHAPES = pp.FIXTURE_CASES + [(256, 256, 2, 3),  # the two-pass forward
                                   (96, 96, 2, 3)]    # the prime-factor one


@pytest.mark.parametrize("det,pw,S,N", SHIFT_SHAPES)
def test_shifts_vs_float64(tp, det, pw, S, N):
    import torch
    P, e = _case(det, pw, S, N)
    with _operator(P) as op:
        grad, costs = tp.position_pd_shifts(op, P["data"], P["psi"],
                                            P["probe"], P["scan"],
                                            costs=True)
        assert isinstance(grad, np.ndarray) and grad.dtype == np.float32
        assert isinstance(costs, np.ndarray) and grad.shape == (N, 2)
        on = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        dev = tp.position_pd_shifts(op, on(P["data"]), on(P["psi"]),
                                    on(P["probe"]), on(P["scan"]), dx=-1.0)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    assert np.array_equal(dev.cpu().numpy(), grad)
    miss = pp.relerr(grad, e["grad"])
    print(f"{(det, pw, S, N)}: grad normwise {miss:.2e}; costs normwise "
          f"{pp.relerr(costs, e['costs']):.2e}")
    assert miss <= GRAD_NORMWISE
    assert pp.relerr(costs, e["costs"]) <= 1e-4  # (tests/util.py COST_RTOL)


@pytest.mark.parametrize("chunk", [2, 3])
def test_shifts_in_chunks(tp, monkeypatch, chunk):
    from tike_amd.ptycho import position
    P, e = _case(32, 16, 2, 7)
    with _operator(P) as op:
        whole = tp.position_pd_shifts(op, P["data"], P["psi"], P["probe"],
                                      P["scan"])
        monkeypatch.setattr(position, "PD_CHUNK_OVERRIDE", chunk)
        parts = tp.position_pd_shifts(op, P["data"], P["psi"], P["probe"],
                                      P["scan"])
    assert pp.relerr(parts, whole) <= 1e-6
    assert pp.relerr(whole, e["grad"]) <= GRAD_NORMWISE


@pytest.mark.parametrize("how", ["per_position", "eigen"])
def test_shifts_with_a_varying_probe(tp, monkeypatch, how):
    from tike_amd.ptycho import position
    P, e = _case(64, 64, 2, 5, eigen=True)
    monkeypatch.setattr(position, "PD_CHUNK_OVERRIDE", 3)  # probes per chunk
    with _operator(P) as op:
        if how == "eigen":
            grad = tp.position_pd_shifts(
                op, P["data"], P["psi"], P["probe"], P["scan"],
                eigen_probe=P["eigen_probe"],
                eigen_weights=P["eigen_weights"])
        else:
            grad = tp.position_pd_shifts(op, P["data"], P["psi"],
                                         P["varying"], P["scan"])
    miss = pp.relerr(grad, e["grad"])
    print(f"{how}: grad normwise {miss:.2e}")
    assert miss <= GRAD_NORMWISE


def test_shifts_of_a_two_slice_object(tp):
    P, e = _case(32, 32, 1, 4, slices=2)
    with _operator(P, slices=2) as op:
        grad = tp.position_pd_shifts(op, P["data"], P["psi"], P["probe"],
                                     P["scan"])
    miss = pp.relerr(grad, e["grad"])
    print(f"two slices: grad normwise {miss:.2e}")
    assert miss <= GRAD_NORMWISE


# --------------------------------------------------------- update_positions_pd
@pytest.mark.parametrize("case", range(len(pp.FIXTURE_CASES)))
def test_update_vs_reference(tp, golden, case):
    ref = golden("position_pd.npz")
    det, pw, S, N = pp.FIXTURE_CASES[case]
    P = dict(psi=ref[f"psi_{case}"], probe=pp.make_probe(pw, S), det=det)
    scan0, data = ref[f"scan_{case}"], ref[f"data_{case}"]
    with _operator(P) as op:
        for j, step in enumerate(ref["steps"]):
            scan, cost = tp.update_positions_pd(op, data, P["psi"],
                                                P["probe"], scan0, dx=-1,
                                                step=float(step))
            assert isinstance(cost, float) and scan.dtype == np.float32
            there = float(op.cost(data, P["psi"], scan, P["probe"],
                                  model="gaussian"))
            miss = np.abs(scan - ref[f"scan_{case}_step{j}"]).max()
            drift = np.abs(scan.astype(np.float64).mean(0) -
                           scan0.astype(np.float64).mean(0)).max()
            print(f"{(det, pw, S, N)} step {step}: positions max |diff| "
                  f"{miss:.2e}, mean moved {drift:.2e}, cost {cost:.6e} "
                  f"(operator.cost {there:.6e}, reference "
                  f"{float(ref[f'cost_{case}_step{j}']):.6e})")
            assert miss <= POSITION_ATOL
            assert drift <= POSITION_ATOL
            assert abs(cost - there) <= 1e-5 * there
        with pytest.raises(ValueError, match="Scan positions must be >= 1"):
            tp.update_positions_pd(op, data, P["psi"], P["probe"], scan0,
                                   step=200.0)


@pytest.mark.parametrize("det,pw,S,N", [(24, 24, 1, 5), (32, 16, 2, 6)])
def test_three_steps_follow_the_float64_trajectory(tp, det, pw, S, N):
    P = pp.problem(det, pw, S, N)
    mine = theirs = P["scan"]
    start = pp.position_error(P["scan"], P["true"])
    with _operator(P) as op:
        for _ in range(3):
            theirs = pp.evaluate(P["data"], P["psi"], P["probe"], theirs,
                                 det, step=0.5)["scan"].astype(np.float32)
            mine, _ = tp.update_positions_pd(op, P["data"], P["psi"],
                                             P["probe"], mine, step=0.5)
            print(f"{(det, pw, S, N)}: error "
                  f"{pp.position_error(theirs, P['true']) / start:.3f} of its "
                  f"start, max |gpu - float64| "
                  f"{np.abs(mine - theirs).max():.2e}")
            assert np.abs(mine - theirs).max() <= 2e-5
    # (on the helper: the method has to do something on these inputs)
    assert pp.position_error(theirs, P["true"]) <= 0.8 * start


# ------------------------------------------------- Reconstruction, one process
def _parameters(tp, P, eigen=False):
    pw = P["probe"].shape[-1]
    return tp.PtychoParameters(
        probe=P["probe"].copy(), psi=P["psi"].copy(), scan=P["scan"].copy(),
        eigen_probe=P["eigen_probe"].copy() if eigen else None,
        eigen_weights=P["eigen_weights"].copy() if eigen else None,
        algorithm_options=tp.RpieOptions(num_batch=2, num_iter=1,
                                         batch_method="contiguous"),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((pw, pw), bool)))


@pytest.mark.parametrize("how", ["u16", "eigen", "on_host"])
def test_context_matches_the_function(tp, how):
    det, pw, S, N = 128, 128, 2, 10
    P = pp.problem(det, pw, S, N, scale=30.0 if how == "u16" else 1.0,
                   eigen=how == "eigen")
    data = (np.rint(P["data"]).astype(np.uint16) if how == "u16"
            else P["data"])
    pp.evaluate(data, P["psi"], P.get("varying", P["probe"]), P["scan"], det)
    with tp.Reconstruction(data, _parameters(tp, P, how == "eigen"),
                           data_on_host=how == "on_host") as ctx:
        before = ctx.get_result()
        cost = ctx.update_positions_pd(step=0.5)
        after = ctx.get_scan()
        probe = (before.probe if how != "eigen" else tp.get_varying_probe(
            before.probe, before.eigen_probe, before.eigen_weights))
        want, want_cost = tp.update_positions_pd(
            ctx.operator, data, before.psi, probe, before.scan, step=0.5)
        with pytest.raises(ValueError, match="Scan positions must be >= 1"):
            ctx.update_positions_pd(step=200.0)
        assert np.array_equal(ctx.get_scan(), after)
    print(f"{how}: max |context - function| {np.abs(after - want).max():.2e}"
          f", moved by {np.abs(after - P['scan']).max():.3f}; cost {cost:.6e}"
          f" vs {want_cost:.6e}")
    assert np.abs(after - P["scan"]).max() > 0.05
    assert np.abs(after - want).max() <= POSITION_ATOL
    assert abs(cost - want_cost) <= 1e-5 * want_cost


# -------------------------------------------------------------------- two ranks
def _ranks(tmp_path, world, step):
    """Fresh child processes, one per rank (gloo, one GPU): each prints the
    scan of the whole job and the cost it was returned."""
    here = os.path.dirname(os.path.abspath(__file__))
    store = tmp_path / f"store_{world}_{step}"
    procs = [subprocess.Popen(
        [sys.executable, os.path.join(here, "_position_pd_child.py"),
         str(rank), str(world), str(store), str(step)],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for rank in range(world)]
    results = []
    for proc in procs:
        out, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, out[-2000:] + err[-4000:]
        line = [l for l in out.splitlines() if l.startswith("RESULT ")]
        results.append(json.loads(line[-1][len("RESULT "):]))
    return results


def test_two_ranks_match_one_rank(tmp_path):
    one, = _ranks(tmp_path, 1, 0.5)
    two = _ranks(tmp_path, 2, 0.5)
    assert one["raised"] is None and np.abs(
        np.array(one["scan"]) - np.array(one["scan0"])).max() > 0.05
    for rank in two:
        assert rank["raised"] is None
        miss = np.abs(np.array(rank["scan"]) - np.array(one["scan"])).max()
        print(f"two ranks: max |diff| {miss:.2e}, cost {rank['cost']:.6e} vs "
              f"{one['cost']:.6e}")
        assert miss <= POSITION_ATOL
        assert rank["cost"] == two[0]["cost"]
        assert abs(rank["cost"] - one["cost"]) <= 1e-5 * one["cost"]


def test_two_ranks_refuse_together(tmp_path):
    for rank in _ranks(tmp_path, 2, 200.0):
        assert rank["raised"] is not None
        assert "Scan positions must be >= 1" in rank["raised"]
        assert rank["scan"] == rank["scan0"]
