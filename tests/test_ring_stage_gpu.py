"""
The LDS-DMA ring tile bodies (gemm_tiles::dma128_tile, dma64_tile) after a change inside a ring stage: exact-integer
products at the smallest shapes that reach each body, the bits of full-mantissa results against the hashes recorded
before the change (tests/golden/ring_bits.json, written by tools/ring_bits.py), and the 128 x 128 body against the
64 x 64 body on the same product.
"""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import kernel_host as kh

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("ring_bits", os.path.join(ROOT, "tools", "ring_bits.py"))
ring_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ring_bits)


@pytest.fixture(scope="module")
def dev():
    d = ring_bits.Dev()
    yield d
    d.close()


@pytest.fixture(scope="module")
def float_ops():
    return ring_bits.operands()


def fail_with_tiles(msgs, what):
    if msgs:
        pytest.fail(what + ":\n  " + "\n  ".join(msgs), pytrace=False)


# (m, n, k, lower): 128 x 128 ring through a mixed launch (406 tiles: a remainder in quarters; 384 tiles), then the small
# shapes: 64 x 64 ring tiles (the (384, 256) rectangles at k > 128 take the 32 x 64 register-staged tiles beside them)
INT_CASES = ([(3584, 3584, k, 1) for k in (256, 640)] + [(2048, 3072, 256, 0)]
             + [(384, 256, k, lo) for k in (128, 192, 320) for lo in (1, 0)]
             + [(2304, 896, 128, 1)])   # a last strip of 7 tile columns


@pytest.mark.parametrize("shape", INT_CASES, ids=lambda c: f"{c[0]}x{c[1]}-k{c[2]}-{'lower' if c[3] else 'rect'}")
def test_ring_integer_exact(dev, shape):
    """C -= A B^T on small integers equals the host product bit for bit in the whole buffer, with A and B two buffers
    of different pitch and with A and B one buffer (the trailing update's shape)."""
    m, n, k, lower = shape
    case = kh.int_gemm_case(m, n, k, n + 32, k + 32, k + 128, lower, seed=25 + m + 3 * n + 7 * k + lower)
    got = dev.gemm(case["C0"], case["A"], case["B"], m, n, k, lower)
    fail_with_tiles(kh.gemm_mismatches(got, case), f"gpmi_dev_gemm_nt m={m} n={n} k={k} lower={lower}, distinct buffers")
    P = np.full((max(m, n), k + 32), kh.OPERAND_PAD)
    P[:, :k] = np.random.default_rng(1025 + m + n + k).integers(-4, 5, (max(m, n), k))
    E = kh.gemm_expected(case["C0"], P[:m], P, n, k)
    got = dev.gemm(case["C0"], P, None, m, n, k, lower)
    fail_with_tiles(kh.gemm_mismatches(got, case, E), f"gpmi_dev_gemm_nt m={m} n={n} k={k} lower={lower}, one buffer")


def test_ring_bits_unchanged(float_ops):
    """Full-mantissa products and factors hash to what they hashed to before the ring stage was rearranged."""
    with open(ring_bits.GOLDEN) as f:
        want = json.load(f)
    got = ring_bits.hashes(float_ops)
    assert set(got) == set(want)
    diff = [name for name in sorted(want) if got[name] != want[name]]
    assert not diff, f"result bits changed: {diff}"


def test_ring_cross_body_bits(dev, float_ops):
    """The (3584, 3584, lower, k = 256) product through the 128 x 128 ring body equals, bit for bit, the same product
    computed as seven 512-column rectangles (28 x 4 tiles each: the 64 x 64 ring body) on offset device pointers - in
    every 128 x 128 tile on or below the diagonal, which is what the lower-triangular launch computes.  (The two bodies
    feed the k of a stage to their MFMAs in the same groups; the equality held before the stage was rearranged too.)"""
    m, n, k, _ = ring_bits.BIG
    C0, A, B = float_ops["big"]
    ldc, lda, ldb = C0.shape[1], A.shape[1], B.shape[1]
    whole = dev.gemm(C0, A, B, m, n, k, 1)
    dC, dA, dB = dev.upload(C0), dev.upload(A), dev.upload(B)
    try:
        for c in range(0, n, 512):
            dev.gemm_nt(C.c_void_p(dC.value + 8 * c), ldc, dA, lda, C.c_void_p(dB.value + 8 * c * ldb), ldb, m, 512, k, 0)
        parts = dev.download(dC, C0.shape)
    finally:
        dev.free(dC, dA, dB)
    ti = np.arange(m)[:, None] // kh.TILE
    tj = np.arange(n)[None, :] // kh.TILE
    bad = (tj <= ti) & (whole[:, :n].view(np.int64) != parts[:, :n].view(np.int64))
    assert np.array_equal(parts[:, n:], C0[:, n:])
    assert not bad.any(), (f"{int(bad.sum())} entries differ between the 128 x 128 and the 64 x 64 ring body, first at "
                           f"{tuple(np.argwhere(bad)[0])}")
