"""Bits of the LDS-DMA ring tile bodies (gemm_tiles::dma128_tile, dma64_tile) on full-mantissa operands: SHA-256 of the
result buffers of a 128 x 128 ring product, a small rectangular product and gpmi_dev_potrf with and without the
flag-ordered tail.  A change of the ring bodies that claims to keep the MFMA order must keep every hash.
usage: python tools/ring_bits.py [out.json]   (default tests/golden/ring_bits.json; tests/test_ring_stage_gpu.py
recomputes the hashes and compares them with that file)"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "inference-tools_amd"))

SEED = 25
GOLDEN = os.path.join(ROOT, "tests", "golden", "ring_bits.json")
BIG = (3584, 3584, 256, 1)    # 406 lower tiles: 128 x 128 ring, mixed launch
SMALL = (384, 256, 192, 0)    # 6 tiles, k > 128: 32 x 64 register-staged tiles, the body beside the ring bodies
POTRF_N = 2176


class Dev:
    """Device buffers and the device-pointer entry points on one handle."""

    def __init__(self, no_flow=False):
        from inference_amd import _lib

        self.h = _lib.Handle(0)
        if no_flow:
            self.h.call("gpmi_set_option", _lib.OPT_NO_FLOW, 1)

    def close(self):
        self.h.close()

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = C.c_void_p()
        self.h.call("gpmi_dev_alloc", a.nbytes, C.byref(p))
        self.h.call("gpmi_dev_upload", p, a.ctypes.data_as(C.c_void_p), a.nbytes)
        return p

    def download(self, p, shape):
        out = np.empty(shape)
        self.h.call("gpmi_dev_download", out.ctypes.data_as(C.c_void_p), p, out.nbytes)
        return out

    def free(self, *ptrs):
        for p in ptrs:
            self.h.call("gpmi_dev_free", p)

    def gemm_nt(self, dC, ldc, dA, lda, dB, ldb, m, n, k, lower):
        self.h.call("gpmi_dev_gemm_nt", dC, ldc, dA, lda, dB, ldb, m, n, k, lower)

    def gemm(self, C0, A, B, m, n, k, lower):
        """C -= A B^T on whole buffers (pitches = the buffers' widths; B None: A serves as both operands).  Returns the
        whole C buffer."""
        dC, dA = self.upload(C0), self.upload(A)
        dB = dA if B is None else self.upload(B)
        try:
            self.gemm_nt(dC, C0.shape[1], dA, A.shape[1], dB, (A if B is None else B).shape[1], m, n, k, lower)
            return self.download(dC, C0.shape)
        finally:
            self.free(*([dC, dA] if B is None else [dC, dA, dB]))

    def potrf(self, buf, n):
        d = self.upload(buf)
        try:
            info = C.c_int(-7)
            self.h.call("gpmi_dev_potrf", d, n, buf.shape[1], C.byref(info))
            return self.download(d, buf.shape), info.value
        finally:
            self.free(d)


def float_gemm_operands(rng, m, n, k):
    """(C0 m x (n + 32), A m x (k + 32), B n x (k + 128)): full-mantissa normal values, zero padding columns."""
    C0 = np.zeros((m, n + 32))
    C0[:, :n] = rng.standard_normal((m, n))
    A = np.zeros((m, k + 32))
    A[:, :k] = rng.standard_normal((m, k))
    B = np.zeros((n, k + 128))
    B[:, :k] = rng.standard_normal((n, k))
    return C0, A, B


def operands():
    """The operands of the three cases, drawn in a fixed order from one generator."""
    rng = np.random.default_rng(SEED)
    big = float_gemm_operands(rng, *BIG[:3])
    small = float_gemm_operands(rng, *SMALL[:3])
    G = rng.standard_normal((POTRF_N, 64))
    spd = np.zeros((POTRF_N, POTRF_N + 32))
    spd[:, :POTRF_N] = G @ G.T + POTRF_N * np.eye(POTRF_N)
    return dict(big=big, small=small, spd=spd)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def results(ops=None):
    """{case: result array}: the whole C buffers of the two products and the lower triangles of the two factors (above
    the diagonal a factorisation leaves workspace whose contents gpmi.h does not define)."""
    ops = operands() if ops is None else ops
    out = {}
    dev = Dev()
    try:
        m, n, k, lower = BIG
        out[f"gemm_{m}x{n}_k{k}_lower"] = dev.gemm(*ops["big"], m, n, k, lower)
        m, n, k, lower = SMALL
        out[f"gemm_{m}x{n}_k{k}_rect"] = dev.gemm(*ops["small"], m, n, k, lower)
        L, info = dev.potrf(ops["spd"], POTRF_N)
        assert info == 0, info
        out[f"potrf_{POTRF_N}_flow"] = np.tril(L[:, :POTRF_N])
    finally:
        dev.close()
    dev = Dev(no_flow=True)
    try:
        L, info = dev.potrf(ops["spd"], POTRF_N)
        assert info == 0, info
        out[f"potrf_{POTRF_N}_no_flow"] = np.tril(L[:, :POTRF_N])
    finally:
        dev.close()
    return out


def hashes(ops=None):
    return {name: sha(a) for name, a in results(ops).items()}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    h = hashes()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(h, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, v in sorted(h.items()):
        print(name, v)
