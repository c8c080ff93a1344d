"""ctypes wrapper over the probe libraries of tests/kernels/row_probe.hip (tests/_build/librow_probe*.so,
built by `make -C fbstab_amd/csrc rowprobe`): numpy in, numpy out, the buffers allocated with torch on cuda:0.
A helper module of tests/test_gpu_row_primitives.py.  A missing library is a failure, not a skip."""
import ctypes
import functools
import os

import numpy as np
import pytest

BUILD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build")
VARIANTS = {"default": "librow_probe.so",        # the product's flags
            "guard": "librow_probe_guard.so",    # -DFB_FMAC_GUARD_NOP=1: every group keeps its s_nop
            "nodpp": "librow_probe_nodpp.so"}    # -DFB_FMAC_DPP=0: two-pass forms only
VARIANT_BITS = {"default": 1, "guard": 3, "nodpp": 0}


@functools.lru_cache(maxsize=None)
def load(variant):
    path = os.path.join(BUILD_DIR, VARIANTS[variant])
    if not os.path.exists(path):
        pytest.fail("tests/_build/%s is missing: `make -C fbstab_amd/csrc rowprobe` "
                    "(__graft_entry__.build() builds it)" % VARIANTS[variant])
    lib = ctypes.CDLL(path)
    assert lib.rp_variant() == VARIANT_BITS[variant], (variant, lib.rp_variant())
    return lib


class Probe:
    """One probe library.  Inputs are lane images [alloc, 16 R, K] (tests/row_rules.lane_image); `count`
    QPs are computed and returned."""

    def __init__(self, variant="default"):
        import torch
        self.torch = torch
        self.lib = load(variant)
        self.dev = torch.device("cuda:0")

    def _in(self, a, dtype=np.float64):
        return self.torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(self.dev)  # (a copy: inputs may be read-only)

    def _out(self, shape, dtype=None):
        # NaN-filled (ints: -1): an entry the kernel did not write cannot pass for a result
        t = self.torch
        if dtype is None:
            return t.full(shape, float("nan"), dtype=t.float64, device=self.dev)
        return t.full(shape, -1, dtype=dtype, device=self.dev)

    def _call(self, name, *args):
        fn = getattr(self.lib, name)
        conv = [ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else ctypes.c_int(int(a)) for a in args]
        fn.restype = ctypes.c_int
        rc = fn(*conv)
        assert rc == 0, "%s returned hipError_t %d" % (name, rc)

    @staticmethod
    def _geom(img, lpq):
        assert img.ndim == 3 and img.shape[1] == lpq, (img.shape, lpq)
        return img.shape[0]

    # ---- factorisation and triangular work: N, R name the instantiation --------------------------------
    def chol(self, N, R, A_img, dadd, wg=64):
        n = self._geom(A_img, 16 * R)
        L, flag = self._out((n, N, N)), self._out((n, 16 * R), self.torch.int32)
        self._call("rp_chol_%d_%d" % (N, R), self._in(A_img), self._in(dadd), L, flag, n, n, wg)
        return L.cpu().numpy(), flag.cpu().numpy()

    def tri_inv(self, N, R, L_img, wg=64):
        n = self._geom(L_img, 16 * R)
        X = self._out((n, N, N))
        self._call("rp_triinv_%d_%d" % (N, R), self._in(L_img), X, n, n, wg)
        return X.cpu().numpy()

    def tri_inv_solve(self, N, R, L_img, B_img, wg=64):
        n = self._geom(L_img, 16 * R)
        X, W = self._out((n, N, N)), self._out((n, N, N))
        self._call("rp_triinvsolve_%d_%d" % (N, R), self._in(L_img), self._in(B_img), X, W, n, n, wg)
        return X.cpu().numpy(), W.cpu().numpy()

    def tri_solve_right(self, N, R, L_img, B_img, wg=64):
        n = self._geom(L_img, 16 * R)
        W = self._out((n, N, N))
        self._call("rp_trisolve_%d_%d" % (N, R), self._in(L_img), self._in(B_img), W, n, n, wg)
        return W.cpu().numpy()

    def subst(self, N, R, L_img, b_img, transposed=False, wg=64):
        """b_img [n, 16 R, 1].  transposed: L_img holds the factor by columns and the chain is subst_cols_t."""
        n = self._geom(L_img, 16 * R)
        x = self._out((n, N))
        self._call("rp_%s_%d_%d" % ("substcolst" if transposed else "substrows", N, R),
                   self._in(L_img), self._in(b_img), x, n, n, wg)
        return x.cpu().numpy()

    def fused(self, name, N, R, A_img, dadd, B_img, wg=64):
        """name: cholinvsolve | cholinv | cholsolveright.  Returns (a, x, w, flag)."""
        n = self._geom(A_img, 16 * R)
        L, X, W = self._out((n, N, N)), self._out((n, N, N)), self._out((n, N, N))
        flag = self._out((n, 16 * R), self.torch.int32)
        self._call("rp_%s_%d_%d" % (name, N, R), self._in(A_img), self._in(dadd), self._in(B_img), L, X, W, flag,
                   n, n, wg)
        return L.cpu().numpy(), X.cpu().numpy(), W.cpu().numpy(), flag.cpu().numpy()

    # ---- dot products: one result per lane ---------------------------------------------------------------
    def bc_dot(self, B, E, R, M_img, v_img, init_img, wg=64):
        n = self._geom(M_img, 16 * R)
        out = self._out((n, 16 * R))
        self._call("rp_bcdot_%d_%d_%d" % (B, E, R), self._in(M_img), self._in(v_img), self._in(init_img), out, n, n, wg)
        return out.cpu().numpy()

    def bc_cols_dot(self, NC, R, neg, C_img, src_img, p_img, wg=64):
        n = self._geom(C_img, 16 * R)
        out = self._out((n, 16 * R, 4))
        self._call("rp_bccols_%d_%d_%d" % (NC, R, int(neg)), self._in(C_img), self._in(src_img), self._in(p_img),
                   out, n, n, wg)
        return out.cpu().numpy()

    def dot4(self, N, M_img, b_img, init_img, wg=64):
        n = self._geom(M_img, 16)
        out = self._out((n, 16))
        self._call("rp_dot4_%d" % N, self._in(M_img), self._in(b_img), self._in(init_img), out, n, n, wg)
        return out.cpu().numpy()

    # ---- lane maps and reductions: v [n, 16 R] ------------------------------------------------------------
    def bc_all(self, R, v, wg=64):
        n = v.shape[0]
        out = self._out((n, 16 * R, 16 * R))
        self._call("rp_bcall_%d" % R, self._in(v), out, n, n, wg)
        return out.cpu().numpy()

    def lane_map(self, R, v, vi, wg=64):
        """(out_d [n, lpq, 3, lpq]: bc<J & 15>, bcs<R, J>, bcr<R, J>; out_i [n, lpq, 2, lpq]: bci<J & 15>, bcri<R, J>)"""
        n, lpq = v.shape[0], 16 * R
        od, oi = self._out((n, lpq, 3, lpq)), self._out((n, lpq, 2, lpq), self.torch.int32)
        self._call("rp_lanemap_%d" % R, self._in(v), self._in(vi, np.int32), od, oi, n, n, wg)
        return od.cpu().numpy(), oi.cpu().numpy()

    def reduce(self, R, v, wg=64):
        """[n, lpq, 4]: row_reduce sum, row_reduce max, qp_reduce sum, qp_reduce max"""
        n = v.shape[0]
        out = self._out((n, 16 * R, 4))
        self._call("rp_reduce_%d" % R, self._in(v), out, n, n, wg)
        return out.cpu().numpy()

    # ---- scalar chains -------------------------------------------------------------------------------------
    def scalar(self, x, wg=64):
        """[n, 3]: rsqrt_full, fsqrt, rcp_fast"""
        out = self._out((x.size, 3))
        self._call("rp_scalar", self._in(x), out, x.size, wg)
        return out.cpu().numpy()

    def pfb(self, a, b, alpha, wg=64):
        """[n, 6]: pfb_all's phi, g0, g1; pfb's phi; pfb_gradient's g0, g1"""
        out = self._out((a.size, 6))
        self._call("rp_pfb", self._in(a), self._in(b), self._in(alpha), out, a.size, wg)
        return out.cpu().numpy()
