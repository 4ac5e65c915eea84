"""The overlap-sum entries -- tike_lstsq_gradients, tike_probe_grad,
tike_probe_preconditioner (csrc/lstsq_gradients.hip), tike_scatter_patches,
tike_psi_preconditioner, tike_scatter_amplitudes (csrc/scatter.hip) -- called
through tike_amd._lib with raw pointers against the float64 model of
tests/overlap_sums.py, on every case of its table that applies to them
(tests/test_overlap_sums_cpu.py pins the model, the preconditions of the
cases and the reach of the bounds).

Every written buffer is a devbuf.Dev: a guard pattern behind its end, outputs
starting as NaN, accumulated ones from given contents.  Each output is held
element by element to the model's bound; an element without a term must hold
0, or its previous contents, exactly; scan, the values, psi and the probe
arrays must come back bit for bit.  Bad arguments return TIKE_ERR_ARG and
nscan == 0 success, with nothing written either way.  The deterministic forms
(tike_set_deterministic is process-wide) run in a fresh child process,
tests/_overlap_sums_child.py, on the reduced table, twice each, with the same
bounds.

The worst error / bound of every (entry, output, case family) is printed
after the module (profiles/overlap_sum_entries.md)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import overlap_sums as om
from _overlap_sums_child import _api, _held, run_gather, run_scatter
from devbuf import Dev

pytestmark = pytest.mark.gpu

WORST = {}  # (entry, output, family) -> worst error / bound


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: the worst error / bound of every group it saw."""
    yield
    for key in sorted(WORST):
        print("WORST", "|".join(key), "{:.4f}".format(WORST[key]))


def _note(ratios, case, family):
    for (entry, output), r in ratios.items():
        print("RATIO {} {} {} {:.4f}".format(entry, output, case, r))
        key = (entry, output, family)
        WORST[key] = max(WORST.get(key, 0.0), r)
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, (case, bad)


@pytest.mark.parametrize("name", [g.name for g in om.GATHER])
def test_gather_entries_vs_model(name):
    """tike_lstsq_gradients with the output set of the case, tike_probe_grad
    and tike_probe_preconditioner."""
    c = om.gather_inputs(name)["case"]
    ratios, _, intact = run_gather(name)
    assert intact, "an input was written"
    modes = "S<=8" if c.S <= 6 or c.S == 8 else "S runtime"
    _note(ratios, name, "{}, {}".format(c.form.rstrip("+"), modes))


@pytest.mark.parametrize("name", [s.name for s in om.SCATTER])
def test_scatter_entries_vs_model(name):
    """tike_scatter_patches, tike_psi_preconditioner and
    tike_scatter_amplitudes, each into an image that holds values."""
    c = om.scatter_inputs(name)["case"]
    ratios, _, intact = run_scatter(name)
    assert intact, "an input was written"
    _note(ratios, name, c.layout)


def _gather_call(lib, st, d, o, nscan, S, pw, H, W, null=()):
    p = {k: (None if k in null or v is None else v.ptr())
         for k, v in {**d, **o}.items()}
    return lib.tike_lstsq_gradients(
        p["chi"], p["scan"], p["psi"], p["probe"], None, None, 0, 0, None,
        p["patches"], p["m_probe_update"], p["objproj"], nscan, S, pw, H, W, st)


def test_bad_arguments_and_no_positions():
    """S = 0 and S = 17, a non-positive shape and a missing required pointer
    are TIKE_ERR_ARG; nscan == 0 succeeds; nothing is written either way."""
    A, lib = _api()
    st = A.stream_ptr()
    name = "pw15-n9-S16-shared"
    I = om.gather_inputs(name)
    c, H, W = I["case"], I["H"], I["W"]
    N, S, pw = c.nscan, c.S, c.pw
    d = {k: _held(I[k]) for k in ("chi", "scan", "psi", "probe")}
    o = dict(patches=Dev((N, pw, pw), cplx=True),
             m_probe_update=Dev((S, pw, pw), cplx=True, init=I["mpu0"]),
             objproj=Dev((N, pw, pw), cplx=True))
    pre = Dev((pw, pw), cplx=True, init=I["pre0"])
    rcs = {}
    for what, (n, s, p, h, w) in {
            "S=0": (N, 0, pw, H, W), "S=17": (N, 17, pw, H, W),
            "pw=0": (N, S, 0, H, W), "H=0": (N, S, pw, 0, W),
            "W=0": (N, S, pw, H, 0), "nscan=-1": (-1, S, pw, H, W),
            "nscan=0": (0, S, pw, H, W)}.items():
        rcs["lstsq " + what] = _gather_call(lib, st, d, o, n, s, p, h, w)
        rcs["grad " + what] = lib.tike_probe_grad(
            d["chi"].ptr(), d["scan"].ptr(), d["psi"].ptr(), o["patches"].ptr(),
            o["m_probe_update"].ptr(), n, s, p, h, w, st)
        if not what.startswith("S="):
            rcs["pre " + what] = lib.tike_probe_preconditioner(
                d["scan"].ptr(), d["psi"].ptr(), pre.ptr(), n, p, h, w, st)
    for k in ("chi", "scan", "psi", "probe"):
        rcs["lstsq no " + k] = _gather_call(lib, st, d, o, N, S, pw, H, W, (k,))
    rcs["grad no m_probe_update"] = lib.tike_probe_grad(
        d["chi"].ptr(), d["scan"].ptr(), d["psi"].ptr(), o["patches"].ptr(), None,
        N, S, pw, H, W, st)
    rcs["grad no chi"] = lib.tike_probe_grad(
        None, d["scan"].ptr(), d["psi"].ptr(), o["patches"].ptr(),
        o["m_probe_update"].ptr(), N, S, pw, H, W, st)
    rcs["pre no out"] = lib.tike_probe_preconditioner(
        d["scan"].ptr(), d["psi"].ptr(), None, N, pw, H, W, st)
    rcs["pre no psi"] = lib.tike_probe_preconditioner(
        d["scan"].ptr(), None, pre.ptr(), N, pw, H, W, st)
    # the scatter entries
    J = om.scatter_inputs("pw7-neighbours-n8")
    s = J["case"]
    scan = _held(J["scan"])
    images = {}
    for entry in om.SCATTER_ENTRIES:
        values, prev = om.scatter_values(J, entry)
        v = _held(values)
        img = images[entry] = (
            Dev((2, s.H, s.W), init=np.stack([prev.real, prev.imag]))
            if entry == "tike_scatter_patches" else Dev((s.H, s.W), init=prev))
        f = getattr(lib, entry)
        for what, (n, p, h, w) in {
                "pw=0": (s.nscan, 0, s.H, s.W), "H=0": (s.nscan, s.pw, 0, s.W),
                "W=0": (s.nscan, s.pw, s.H, 0), "nscan=-1": (-1, s.pw, s.H, s.W),
                "nscan=0": (0, s.pw, s.H, s.W)}.items():
            rcs[entry + " " + what] = f(v.ptr(), scan.ptr(), img.ptr(), n, p, h,
                                        w, st)
        rcs[entry + " no values"] = f(None, scan.ptr(), img.ptr(), s.nscan, s.pw,
                                      s.H, s.W, st)
        rcs[entry + " no scan"] = f(v.ptr(), None, img.ptr(), s.nscan, s.pw, s.H,
                                    s.W, st)
        rcs[entry + " no image"] = f(v.ptr(), scan.ptr(), None, s.nscan, s.pw,
                                     s.H, s.W, st)
    want = {k: 0 if k.endswith("nscan=0") else om.ERR_ARG for k in rcs}
    assert rcs == want
    for buf in (*o.values(), pre, *images.values()):
        assert buf.untouched()


def test_deterministic_forms():
    """All six entries under tike_set_deterministic in a fresh process: the
    same bounds, two runs bit-identical, and the one-chunk fall-back of a
    scratch buffer too small for the partial sums."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "TIKE_DETERMINISTIC"}
    p = subprocess.run([sys.executable, os.path.join(here, "_overlap_sums_child.py")],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    r = json.loads(line[len("RESULT "):])
    assert set(r["cases"]) >= set(om.DET_GATHER) | set(om.DET_SCATTER)
    assert len(r["cases"]) == len(om.DET_GATHER) + len(om.DET_SCATTER) + 1
    for case, ratios in r["cases"].items():
        keyed = {tuple(k.split(" ")): v for k, v in ratios.items()}
        _note(keyed, "deterministic " + case, "deterministic")
    assert r["identical"], "two runs from the same start differ"
    assert r["intact"], "an input was written"
