#!/usr/bin/env python3
"""Golden vectors of the gradient-of-intensity position refinement (build
container only):

    python tests/golden/gen/make_position_pd_fixtures.py

`position_pd.npz`: the REFERENCE's own `tike.ptycho.position.
update_positions_pd` (run under the NumPy-backed CuPy stand-in, its
`convolution.cu` through `emu.cpp`) on the seeded problems of
tests/position_pd.py.  At this snapshot the function calls `operator.cost`
without the keyword-only `model` and raises TypeError on its last statement:
it is run with an operator subclass whose `cost` defaults `model="gaussian"`,
nothing else changed.  The value its `tike.linalg.lstsq` call returns (`grad`)
is captured during the call.  Data only; tests/test_position_pd_cpu.py and
tests/test_position_pd_gpu.py read it.
"""
import os
import subprocess
import sys

sys.dont_write_bytecode = True  # never write into /root/reference
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
REF = "/root/reference"

tmp = tempfile.mkdtemp(prefix="tike_ref_emu_")
emu = os.path.join(tmp, "libemu.so")
subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", emu,
                       os.path.join(HERE, "emu.cpp")])
os.environ["TIKE_REF_EMU_LIB"] = emu
sys.path.insert(0, os.path.join(HERE, "cupy_shim"))
sys.path.insert(0, os.path.join(REF, "src"))
sys.path.insert(0, os.path.dirname(OUT))  # tests/

import cupy as cp  # noqa: E402  (the shim)
import tike.linalg  # noqa: E402
import tike.operators  # noqa: E402
import tike.ptycho.position as ref_position  # noqa: E402

import position_pd as pp  # noqa: E402


class PtychoGaussianCost(tike.operators.Ptycho):
    """The reference operator; `cost` may be called without `model`."""

    def cost(self, data, psi, scan, probe, *, model="gaussian"):
        return super().cost(data, psi, scan, probe, model=model)


# (one slice: the optics are not used)
PHYS = dict(probe_wavelength=1e-10, probe_FOV_lengths=(1e-5, 1e-5),
            multislice_propagation_distance=1e-8)
captured = []
real_lstsq = tike.linalg.lstsq


def recording_lstsq(*args, **kwargs):
    x = real_lstsq(*args, **kwargs)
    captured.append(np.array(x))
    return x


tike.linalg.lstsq = recording_lstsq

out = {"cases": np.array(pp.FIXTURE_CASES, dtype=np.int64),
       "steps": np.array([0.05, 0.5])}
for i, (det, pw, S, N) in enumerate(pp.FIXTURE_CASES):
    P = pp.problem(det, pw, S, N)
    # (the probe is `position_pd.make_probe(pw, S)`, a closed form: stored as
    # its power only, which the CPU test compares)
    for key in ("psi", "true", "scan", "data"):
        out[f"{key}_{i}"] = P[key]
    out[f"probe_power_{i}"] = np.sum(np.abs(P["probe"].astype(np.complex128))**2)
    with PtychoGaussianCost(nscan=N, probe_shape=pw, detector_shape=det,
                            nz=pw + 24, n=pw + 24, **PHYS) as op:
        for j, step in enumerate(out["steps"]):
            del captured[:]
            scan, cost = ref_position.update_positions_pd(
                op, cp.asarray(P["data"]), cp.asarray(P["psi"]),
                cp.asarray(P["probe"]), cp.asarray(P["scan"]), dx=-1,
                step=float(step))
            assert len(captured) == 1
            out[f"scan_{i}_step{j}"] = np.asarray(scan)
            out[f"cost_{i}_step{j}"] = np.float64(cost)
            if j == 0:
                out[f"grad_{i}"] = captured[0][..., 0]  # position.py:689
            else:
                assert np.array_equal(out[f"grad_{i}"], captured[0][..., 0])
    e = pp.evaluate(P["data"], P["psi"], P["probe"], P["scan"], det, step=0.5)
    print((det, pw, S, N), "grad", out[f"grad_{i}"].dtype,
          "vs float64: normwise %.2e" % pp.relerr(out[f"grad_{i}"], e["grad"]),
          "positions max |diff| %.2e" %
          np.abs(out[f"scan_{i}_step1"] - e["scan"]).max(),
          "condition %.2f misfit %.4f" % (e["condition"].max(),
                                          e["misfit"].min()))

path = os.path.join(OUT, "position_pd.npz")
np.savez_compressed(path, **out)
print(f"position_pd.npz: {os.path.getsize(path) / 1e6:.2f} MB")
