"""The difference map on the GPU: `tike_dm_reflect` and `tike_dm_update`
against the float64 model (tests/dm_model.py) at the smallest shapes that can
still go wrong, the two routes of the exit-wave step against each other and
against the model at 256^2 and 512^2, and the solver through
`reconstruct(data, parameters)` against the model's epochs.

The GPU work runs in a child process (tests/_dm_child.py), one per section,
which writes every figure; the tests print a figure before they hold it to
its bar.  Every test here fails on the parent commit: it has no `DmOptions`,
no `solvers.dm` and no `tike_dm_reflect` / `tike_dm_update`."""
import json
import os
import subprocess
import sys

import pytest

from util import OP_NORMWISE, SOLVER_NORMWISE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_RESULTS = {}


def section(name, tmp_path_factory, **env):
    """The figures of a section of the child, computed once."""
    if name not in _RESULTS:
        out = str(tmp_path_factory.mktemp("dm") / f"{name}.json")
        proc = subprocess.run(
            [sys.executable, os.path.join(HERE, "_dm_child.py"), name, out],
            capture_output=True, text=True, timeout=600,
            env={**os.environ, **env})
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
        with open(out) as f:
            _RESULTS[name] = json.load(f)
    return _RESULTS[name]


# ------------------------------------------------------------------ entries
# det 64 / pw 48 / S 3 / nscan 5: padding on both sides, an odd number of
# modes, fewer columns than an item holds; det = pw = 32, S = 1: no padding;
# det 45 / pw 35 / S 2: rows of odd length, whose last element has no partner
# and whose 16-byte accesses are aligned to 8 bytes only, and an odd padding
# of 5, so that the window starts and ends inside a lane's pair of columns.
# The positions hold the smallest allowed one (1.0), the largest and a
# whole-pixel one.
SHAPES = ["padded", "plain", "odd"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("relaxation", [1.0, 0.6])
def test_entries_vs_float64_model(tmp_path_factory, shape, relaxation):
    r = section("entries", tmp_path_factory)[shape][f"a={relaxation}"]
    print(shape, relaxation, r)
    assert r["finite"] and r["inputs_kept"] and r["reflect_repeats"]
    assert r["padding_zero"]
    assert r["reflect_err"] <= OP_NORMWISE
    assert r["reflect_worst"] <= OP_NORMWISE
    assert r["update_err"] <= OP_NORMWISE
    assert r["update_worst"] <= OP_NORMWISE
    assert r["change_err"] <= 1e-5
    # one workgroup per position (with `change`) or several: the same waves,
    # to a rounding of float32 where the compiler fuses the two differently
    assert r["change_grid_waves"] <= 1e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_null_waves_are_the_products(tmp_path_factory, shape):
    r = section("entries", tmp_path_factory)[shape]
    print(shape, {k: v for k, v in r.items() if not k.startswith("a=")})
    assert r["null_equals_explicit"]  # bit for bit
    assert r["null_padding_zero"]
    assert r["null_err"] <= OP_NORMWISE


@pytest.mark.parametrize("shape", SHAPES)
def test_bad_arguments_and_no_positions(tmp_path_factory, shape):
    r = section("entries", tmp_path_factory)[shape]
    assert r["bad_arguments"]  # TIKE_ERR_ARG, each of them
    assert r["no_positions"] and r["nothing_written"]


# ------------------------------------------------------------------- routes
@pytest.mark.parametrize("shape", ["256", "512"])
def test_routes_agree_and_meet_the_model(tmp_path_factory, shape):
    """det = pw = 256, S = 2, nscan = 3 and 512, S = 1, nscan = 2: one
    exit-wave step far-plane-free and with a stored far plane."""
    r = section("routes", tmp_path_factory)[shape]
    print(shape, r)
    assert r["step"] > 1e-2  # the step moved the waves
    assert r["routes_waves"] <= OP_NORMWISE
    assert r["routes_costs"] <= OP_NORMWISE
    for route in ("fused", "stored"):
        assert r[f"{route}_waves"] <= OP_NORMWISE
        assert r[f"{route}_costs"] <= OP_NORMWISE


# ------------------------------------------------------------------- solver
@pytest.mark.parametrize("variant", ["float32", "uint16", "masked",
                                     "three_batches"])
def test_three_epochs_vs_float64_model(tmp_path_factory, variant):
    """det = pw = 64, S = 2, 36 positions, object and probe recovered, three
    epochs through `reconstruct`; `masked`: the gaps of a module detector
    with NaN under them and unmeasured_pixels_scaling 0.95."""
    s = section("solver", tmp_path_factory)
    r = s[variant]
    print(variant, r)
    assert r["epochs"] == 3
    assert r["psi"] <= SOLVER_NORMWISE
    assert r["probe"] <= SOLVER_NORMWISE
    assert r["costs"] <= SOLVER_NORMWISE
    assert s["float32"]["moved"] > 1e-2


def test_batches_only_partition_the_work(tmp_path_factory):
    r = section("solver", tmp_path_factory)["three_vs_one"]
    print(r)
    assert r["psi"] <= 1e-5 and r["probe"] <= 1e-5 and r["costs"] <= 1e-5


def _ranks(tmp_path, world):
    """Fresh child processes, one per rank (gloo, one GPU)."""
    store = tmp_path / f"store_{world}"
    outs = [str(tmp_path / f"out_{world}_{rank}.json")
            for rank in range(world)]
    procs = [subprocess.Popen(
        [sys.executable, os.path.join(HERE, "_dm_child.py"), "ranks",
         outs[rank], str(rank), str(world), str(store)],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for rank in range(world)]
    for proc in procs:
        out, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, out[-2000:] + err[-4000:]
    results = []
    for path in outs:
        with open(path) as f:
            results.append(json.load(f))
    return results


def test_two_ranks_match_one_rank(tmp_path):
    """The overlap sums and the cost are all-reduced: two ranks, the second
    without a share of the first minibatch, give one rank's epochs (1e-4: the
    order of float32 sums) and the same bits as each other."""
    import numpy as np

    from util import relerr
    one, = _ranks(tmp_path, 1)
    two = _ranks(tmp_path, 2)
    assert one["shares"] == [1, 35]
    assert two[0]["shares"] == [1, 18] and two[1]["shares"] == [0, 17]
    for r in two:
        psi, probe = relerr(r["psi"], one["psi"]), relerr(r["probe"],
                                                          one["probe"])
        print(f"two ranks: psi {psi:.2e} probe {probe:.2e} costs",
              r["costs"], "vs", one["costs"])
        assert psi <= 1e-4 and probe <= 1e-4
        np.testing.assert_allclose(r["costs"], one["costs"], rtol=1e-4)
        assert r["psi"] == two[0]["psi"] and r["probe"] == two[0]["probe"]


def test_a_second_reconstruction_starts_from_the_products(tmp_path_factory):
    """The waves are no part of `PtychoParameters`: an epoch on the result of
    two epochs equals an epoch of a fresh run from that object and probe, bit
    for bit, and is not what the third epoch of the first context gives.
    (TIKE_DETERMINISTIC=1: the overlap sums are float atomics otherwise, and
    no two runs of an epoch have the same last bits.)"""
    r = section("resume", tmp_path_factory, TIKE_DETERMINISTIC="1")
    print(r)
    assert r["deterministic"]
    assert r["psi_equals_fresh"] and r["probe_equals_fresh"]
    assert r["cost_equals_fresh"]
    assert r["differs_from_kept_waves"] > 1e-6
    assert r["epochs_on_record"] == 3
