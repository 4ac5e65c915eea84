#!/usr/bin/env python3
"""Golden vectors of fly-scan data (build container only):

    python tests/golden/gen/make_fly_fixtures.py

`fly_scan.npz`: the REFERENCE's own `tike.ptycho.simulate(fly=3)`,
`tike.ptycho.ptycho._compute_intensity(fly=3)`, the gaussian and Poisson cost
of `tike.operators.cupy.objective`, the far-plane gradients of its
`gaussian_grad` / `poisson_grad` with the frame's data and intensity repeated
over the positions of the frame, and `tike.operators.Ptycho.adj` of those
gradients (run under the NumPy-backed CuPy stand-in, `convolution.cu` through
`emu.cpp`) on the seeded problem `tests/fly_scan.FIXTURE`.  The counts the
costs and gradients are taken against are the simulated ones scaled by a
smooth factor, so that no factor vanishes; one set has a block of unmeasured
pixels whose counts are NaN (the gradient there is 0, the cost the mean over
the measured pixels).  To keep the file small the far-plane gradients are
stored for the positions of frame 0 and the object gradients for two of the
four variants.  Data only; tests/test_fly_scan_cpu.py and
tests/test_fly_scan_gpu.py read it.
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
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))  # oracle/

import cupy as cp  # noqa: E402  (the shim)
import tike.operators  # noqa: E402
import importlib  # noqa: E402

ref_objective = importlib.import_module("tike.operators.cupy.objective")
import tike.ptycho  # noqa: E402
import tike.ptycho.ptycho as ref_ptycho  # noqa: E402

import fly_scan as fs  # noqa: E402

PHYS = dict(probe_wavelength=1e-10, probe_FOV_lengths=(1e-5, 1e-5),
            multislice_propagation_distance=1e-8)
K = fs.FIXTURE
fly, det, pw, obj = K["fly"], K["det"], K["pw"], K["obj"]
P = fs.problem(**K)
scan, psi, probe = P["scan"], P["psi0"], P["probe"]
N = len(scan)

out = dict(scan=scan, psi=psi, probe=probe, psi_true=P["psi"])
out["simulated"] = tike.ptycho.simulate(det, probe, scan, P["psi"], fly=fly,
                                        **PHYS)
mask = fs.block_mask(det)
out["mask"] = mask
# counts to measure psi against: the simulated ones, modulated
yy, xx = np.meshgrid(np.arange(det), np.arange(det), indexing="ij")
data = (out["simulated"] * (1.0 + 0.3 * np.cos(0.4 * yy + 0.7 * xx))).astype(
    np.float32)
out["data"] = data
with tike.operators.Ptycho(probe_shape=pw, detector_shape=det, nz=obj, n=obj,
                           **PHYS) as op:
    inten = ref_ptycho._compute_intensity(op, cp.asarray(psi),
                                          cp.asarray(scan),
                                          cp.asarray(probe), fly=fly)
    out["intensity"] = np.asarray(inten, dtype=np.float32)
    far = op.fwd(probe=cp.asarray(probe), scan=cp.asarray(scan),
                 psi=cp.asarray(psi))
    out["farplane"] = np.asarray(far)
    uprobe = cp.asarray(np.broadcast_to(probe, (N, *probe.shape[1:])).copy())
    d_rep = np.repeat(data, fly, axis=0)
    i_rep = np.repeat(out["intensity"], fly, axis=0)
    for model in ("gaussian", "poisson"):
        out[f"cost_{model}"] = np.float64(
            getattr(ref_objective, model)(cp.asarray(data), inten))
        # all pixels measured, then the mask: 0 at unmeasured pixels, whose
        # counts (NaN for the product) never reach the reference's arithmetic
        for tag, m in (("", None), ("_masked", mask)):
            g = np.asarray(getattr(ref_objective, model + "_grad")(
                cp.asarray(d_rep), far, cp.asarray(i_rep)))
            if m is not None:
                g = g * m
                each = getattr(ref_objective, "_" + model + "_fuse")(
                    cp.asarray(data), inten)
                out[f"cost_{model}_masked"] = np.float64(
                    np.mean(np.asarray(each)[:, m]))
            g = g.astype(np.complex64)
            psi_adj, probe_adj = op.adj(farplane=cp.asarray(g), probe=uprobe,
                                        scan=cp.asarray(scan),
                                        psi=cp.asarray(psi))
            out[f"grad_far_{model}{tag}"] = g
            out[f"grad_psi_{model}{tag}"] = np.asarray(psi_adj)
            out[f"grad_probe_{model}{tag}"] = np.sum(np.asarray(probe_adj),
                                                     axis=0, keepdims=True)

# size: the far-plane gradients are kept for the positions of frame 0 (the
# whole arrays are compared with the float64 model here), the object
# gradients for gaussian + mask and poisson without; the far plane is not kept
for model in ("gaussian", "poisson"):
    for tag, m in (("", None), ("_masked", mask)):
        key = f"grad_far_{model}{tag}"
        g = fs.farplane_gradient(model, data, out["farplane"], fly, m)
        print(model, tag, "far-plane gradient vs float64 model: normwise %.2e"
              % (np.linalg.norm(g - out[key]) / np.linalg.norm(g)))
        out[key] = out[key][:fly]
del out["farplane"], out["grad_psi_gaussian"], out["grad_psi_poisson_masked"]
del out["psi_true"]

path = os.path.join(OUT, "fly_scan.npz")
np.savez_compressed(path, **out)
print(f"fly_scan.npz: {os.path.getsize(path) / 1e3:.0f} kB")
