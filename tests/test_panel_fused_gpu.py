"""
The fused panel column of the stream-ordered chain (csrc/potrf_panel.hip: potrf_diag of a tile column and the panel TRSM
under it in one launch, the TRSM's column blocks formed as the row blocks of the inverse are published) against the
two-launch form (GPMI_PANEL_FUSED=0).  Same sums in the same order for every element: the factor, everything computed
from the inverses of the diagonal blocks (alpha, the log-determinant, predictions) and `info` must be the SAME BITS.
The switch is read once per process, so every variant runs in a fresh child interpreter; children are shared between
the cases that run under the same settings.
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = f"sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'inference-tools_amd')!r}]\n"

# argv: out.npz n [n ...] - one fit + predict per size; the factor itself up to n = 2048, its digest beyond
FIT_CODE = (
    "import hashlib, sys\n" + PATHS +
    "import numpy as np, workloads as wl\n"
    "from inference_amd.gp import GpRegressor\n"
    "out = {}\n"
    "for n in map(int, sys.argv[2:]):\n"
    "    d = 3\n"
    "    x, y, e = wl.synthetic_dataset(7, n, d)\n"
    "    gp = GpRegressor(x, y, y_err=e, hyperpars=wl.timing_theta(wl.SE, y, d))\n"
    "    mu, sig = gp(wl.query_points(7, 40, d))\n"
    "    L = np.tril(gp.L)\n"
    "    out[f'alpha{n}'] = gp.alpha; out[f'logdet{n}'] = np.array([gp._logdet]); out[f'mu{n}'] = mu; out[f'sig{n}'] = sig\n"
    "    out[f'Lsha{n}'] = np.frombuffer(hashlib.sha256(L.tobytes()).digest(), dtype=np.uint8)\n"
    "    if n <= 2048: out[f'L{n}'] = L\n"
    "np.savez(sys.argv[1], **out)\n")

# argv: out.npz n col [col ...] - gpmi_dev_potrf of one positive definite matrix with the sign of diagonal entry `col`
# flipped, per col: info
INFO_CODE = (
    "import ctypes as C, sys\n" + PATHS +
    "import numpy as np\n"
    "from inference_amd import _lib\n"
    "n = int(sys.argv[2]); ld = n + 32\n"
    "rng = np.random.default_rng(11)\n"
    "B = rng.standard_normal((n, 48))\n"
    "Am = B @ B.T + n * np.eye(n)\n"
    "h = _lib.Handle(0)\n"
    "d = C.c_void_p(); out = {}\n"
    "buf = np.zeros((n, ld))\n"
    "h.call('gpmi_dev_alloc', buf.nbytes, C.byref(d))\n"
    "for col in map(int, sys.argv[3:]):\n"
    "    buf[:, :n] = Am; buf[col, col] = -buf[col, col]\n"
    "    info = C.c_int(-7)\n"
    "    h.call('gpmi_dev_upload', d, buf.ctypes.data_as(C.c_void_p), buf.nbytes)\n"
    "    h.call('gpmi_dev_potrf', d, n, ld, C.byref(info))\n"
    "    out[f'info{col}'] = np.array([info.value])\n"
    "h.call('gpmi_dev_free', d); h.close()\n"
    "np.savez(sys.argv[1], **out)\n")


@functools.lru_cache(maxsize=None)
def _children(code, args, settings):
    """{'0': results, '1': results} of the child script under GPMI_PANEL_FUSED=0 and =1 with `settings` (a tuple of
    (name, value) pairs) in the environment; run once per distinct call."""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for fused in ("0", "1"):
            out = os.path.join(tmp, f"fused{fused}.npz")
            env = dict(os.environ, GPMI_PANEL_FUSED=fused, **dict(settings))
            run = subprocess.run([sys.executable, "-c", code, out, *args], env=env, capture_output=True, text=True,
                                 timeout=300)
            assert run.returncode == 0, (fused, settings, run.stderr[-2000:])
            assert "timed out" not in run.stderr, (fused, settings, run.stderr[-2000:])
            res[fused] = dict(np.load(out))
    return res


STREAM = (("GPMI_FLOW", "0"),)  # the stream-ordered chain factors the whole matrix
# n -> (sizes of the child that holds it, settings)
FIT_CASES = {
    128: ((128, 256, 300, 640), STREAM),   # no panel below the diagonal block: the fused launch is not taken
    256: ((128, 256, 300, 640), STREAM),   # one worker tile
    300: ((128, 256, 300, 640), STREAM),   # np = 384: identity padding inside a worker tile
    640: ((128, 256, 300, 640), STREAM),   # crosses an outer-panel boundary
    1152: ((1152,), STREAM + (("GPMI_PANEL_WORKERS", "2"),)),  # two workers: up to four tiles each
    # (a lane of this size has no CU-masked stream pair - they come with np >= 5120 -, so the look-ahead setting leaves this
    # factorisation on the full-chip stream; the case below is the one beside a trailing update)
    1536: ((1536,), (("GPMI_LOOKAHEAD_MIN", "2"),)),
    # a lane with the CU-masked stream pair (np >= 5120): the look-ahead panels on the 32-CU panel stream beside the
    # trailing updates on the other CUs, down to 8 trailing tile rows
    5200: ((5200,), STREAM + (("GPMI_LOOKAHEAD_MIN", "8"),)),
}


@pytest.mark.parametrize("n", sorted(FIT_CASES))
def test_fused_panel_column_is_bit_identical_to_two_launches(n):
    sizes, settings = FIT_CASES[n]
    res = _children(FIT_CODE, tuple(map(str, sizes)), settings)
    a, b = res["0"], res["1"]
    for q in ("L", "Lsha", "alpha", "logdet", "mu", "sig"):
        key = f"{q}{n}"
        if key not in a:
            assert q == "L" and n > 2048
            continue
        same = a[key].tobytes() == b[key].tobytes()
        if not same and q == "L":
            diff = np.argwhere(a[key] != b[key])
            tiles = sorted({(int(i) // 128, int(j) // 128) for i, j in diff[:100000]})
            pytest.fail(f"n={n}: L differs in {len(diff)} elements, tiles {tiles[:12]}", pytrace=False)
        assert same, (n, q, settings)


def test_fused_panel_column_reports_the_same_info():
    """A diagonal block that is not positive definite: in the very first block (column 5), and in the third column block
    of the second outer panel (tile column 6: column 805) of a matrix of nine tile columns.  LAPACK's info = the order of
    the first leading minor that fails = column + 1, from both forms, and no worker may wait out its time limit for the
    inverse of such a block (no 'timed out' in either child; each child has seconds)."""
    cols = (5, 6 * 128 + 37)
    res = _children(INFO_CODE, ("1152",) + tuple(map(str, cols)), STREAM)
    for col in cols:
        i0, i1 = int(res["0"][f"info{col}"][0]), int(res["1"][f"info{col}"][0])
        print(f"column {col}: info two launches = {i0}, fused = {i1}")
        assert i0 == i1 == col + 1, (col, i0, i1)
