"""cgrad with nothing to recover (`object_options=None`, `probe_options=None`):
every minibatch of every kind -- plain, fly scan, several slices -- is one
cost-only evaluation.  The iterate comes back bit for bit and every epoch
reports the mean over its minibatches of `Ptycho.cost`.

Several slices: `Ptycho.cost` refuses an object of several slices
(NotImplementedError) and without ProbeOptions the operator has no wavelength
(the propagator between the slices is NaN), so that kind runs with a probe
whose updates never start and is held to the float64 model of
tests/cgrad_multislice.py instead, at the bar that model's chunk costs are
held to (COST_RTOL, tests/test_cgrad_multislice_gpu.py).

The two epochs evaluate the same costs at the same iterate; their sums come
out bit for bit alike only where no float atomic takes part, so the three runs
are made by one child process under TIKE_DETERMINISTIC=1
(tests/_cgrad_cost_only_child.py), as the other bit-for-bit tests do."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cgrad_multislice as ms
import cgrad_positions as cp
import fly_scan as fs
from oracle import operators as ops
from util import COST_RTOL, OP_NORMWISE

pytestmark = pytest.mark.gpu

NEVER = 1 << 30


def _plain():
    """128^2, one mode, five positions."""
    true, psi, probe, data, _, _ = cp.problem(128, 128, 1, 5, seed=2)
    return dict(data=data, psi=cp.start(psi), probe=probe, scan=true, fly=1,
                batches=[np.arange(0, 3), np.arange(3, 5)])


def _fly():
    """The problem of tests/golden/fly_scan.npz: 12 frames of 3 positions."""
    fly = fs.FIXTURE["fly"]
    P = fs.problem(**fs.FIXTURE)
    return dict(data=P["data"], psi=P["psi0"], probe=P["probe0"],
                scan=P["scan"], fly=fly,
                batches=[np.arange(0, 5 * fly), np.arange(5 * fly, 12 * fly)])


def _two_slices(tp):
    """`general32_d2` of tests/cgrad_multislice.py: 32^2, two slices.  The
    optics of the operator travel in ProbeOptions: a probe whose updates start
    at an epoch that never comes; no ObjectOptions, so the slices are the
    default distance apart."""
    P = ms.problem(**ms.SOLVER_CASES["general32_d2"])
    pw = P["probe"].shape[-1]
    fov = (pw * ms.PIXEL, pw * ms.PIXEL)
    distance = tp.ObjectOptions().multislice_propagation_distance
    H = ops.fresnel_spectrum_propagator((pw, pw), fov, distance,
                                        ms.WAVELENGTH).astype(np.complex128)
    return dict(data=P["data"], psi=P["psi0"], probe=P["probe0"],
                scan=P["scan"], fly=1,
                batches=[np.arange(0, 5), np.arange(5, 9)],
                probe_options=tp.ProbeOptions(
                    init_rescale_from_measurements=False, update_start=NEVER,
                    probe_wavelength=ms.WAVELENGTH, probe_FOV_lengths=fov),
                cost=lambda op, d, psi, scan, probe: ms.cost(
                    "gaussian", d, psi, scan, probe, H),
                rtol=COST_RTOL)


CASES = {"plain": lambda tp: _plain(), "fly": lambda tp: _fly(),
         "two_slices": _two_slices}


def run(tp, K):
    """Two epochs in the two minibatches of the case `K`, nothing recovered,
    every pixel measured, the gaussian model: (result, mean over the
    minibatches of the reference cost at the input)."""
    data, fly, batches = K["data"], K["fly"], K["batches"]
    N, det = len(K["scan"]), data.shape[-1]
    params = tp.PtychoParameters(
        probe=K["probe"].copy(), psi=K["psi"].copy(), scan=K["scan"].copy(),
        algorithm_options=tp.CgradOptions(num_batch=2, cg_iter=2, num_iter=2,
                                          step_length=1.0,
                                          batch_method="contiguous"),
        probe_options=K.get("probe_options"), object_options=None,
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((det, det), bool),
            noise_model="gaussian"))
    cost = K.get("cost", lambda op, *args: op.cost(*args, model="gaussian",
                                                   fly=fly))
    with tp.Reconstruction(data, params, fly=fly, order=np.arange(N),
                           batches=batches, spatial_sort=False) as ctx:
        ctx.iterate(2)
        got = ctx.get_result()
        want = float(np.mean([
            float(cost(ctx.operator, data[b[0] // fly:(b[-1] + 1) // fly],
                       K["psi"], K["scan"][b], K["probe"])) for b in batches]))
    return got, want


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """Every case, run once by the child."""
    out = tmp_path_factory.mktemp("cost_only") / "results.npz"
    child = os.path.join(os.path.dirname(__file__),
                         "_cgrad_cost_only_child.py")
    subprocess.run([sys.executable, child, str(out)], check=True, timeout=300,
                   env=dict(os.environ, TIKE_DETERMINISTIC="1"))
    return np.load(out)


@pytest.mark.parametrize("case", sorted(CASES))
def test_nothing_recovered_reports_the_cost_and_moves_nothing(case, results):
    import tike_amd.ptycho as tp
    K = CASES[case](tp)
    costs, want = results[f"{case}_costs"], float(results[f"{case}_want"])
    print(f"{case}: costs {costs!r}, reference {want!r}, rel. difference "
          f"{abs(costs[0] - want) / abs(want):.2e}")
    for name in ("psi", "probe", "scan"):
        got = results[f"{case}_{name}"]
        assert got.dtype == K[name].dtype and np.array_equal(got, K[name]), name
    assert len(costs) == 2 and costs[0] == costs[1]
    assert np.isfinite(want)
    assert abs(costs[0] - want) <= K.get("rtol", OP_NORMWISE) * abs(want), (
        costs, want)
