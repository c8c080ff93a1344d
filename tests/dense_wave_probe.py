"""ctypes wrapper over the probe library of tests/kernels/dense_wave_probe.hip (tests/_build/libdense_wave_probe.so,
built by `make -C fbstab_amd/csrc denseprobe`, which `rowprobe` and so __graft_entry__.build() depend on): numpy
in, numpy out, the buffers allocated with torch on cuda:0.  A helper module of
tests/test_gpu_dense_wave_stages.py.  A missing library is a failure, not a skip.

Matrices go in in mathematical shape, [count, rows, cols] (tests/dense_wave_rules.problem), and are laid out by
columns here, as the C-ABI takes them; images and right-hand sides are [count, 64, 64] and [count, 64]."""
import ctypes
import functools
import os

import numpy as np
import pytest

BUILD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build")
LIBRARY = "libdense_wave_probe.so"


@functools.lru_cache(maxsize=None)
def load():
    path = os.path.join(BUILD_DIR, LIBRARY)
    if not os.path.exists(path):
        pytest.fail("tests/_build/%s is missing: `make -C fbstab_amd/csrc denseprobe` "
                    "(__graft_entry__.build() builds it)" % LIBRARY)
    lib = ctypes.CDLL(path)
    lib.dwp_ws_doubles.restype = ctypes.c_long
    return lib


class DenseWaveProbe:
    """The probe library; every call computes `count` QPs, one wavefront each."""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = load()
        self.dev = torch.device("cuda:0")

    def _in(self, a, dtype=np.float64):
        a = np.array(a, dtype=dtype, order="C")  # (a copy: inputs may be read-only)
        if a.size == 0:  # (nl = 0: a valid address that is never read)
            a = np.zeros(1, dtype=dtype)
        return self.torch.from_numpy(a).to(self.dev)

    def _cols(self, M):
        return self._in(np.asarray(M).transpose(0, 2, 1))

    def _out(self, shape, dtype=None):
        # NaN-filled (ints: -1): an entry the kernel did not write cannot pass for a result
        t = self.torch
        shape = tuple(max(1, s) for s in shape) if 0 in shape else shape
        if dtype is None:
            return t.full(shape, float("nan"), dtype=t.float64, device=self.dev)
        return t.full(shape, -1, dtype=dtype, device=self.dev)

    def _ws(self, nz, nl, nv, count):
        per = self.lib.dwp_ws_doubles(nz, nl, nv)
        assert per > 0, (nz, nl, nv)
        return self.torch.zeros((count, per), dtype=self.torch.float64, device=self.dev)  # (zeroed: see the probe)

    def _call(self, name, *args):
        fn = getattr(self.lib, name)
        conv = []
        for a in args:
            if hasattr(a, "data_ptr"):
                conv.append(ctypes.c_void_p(a.data_ptr()))
            elif isinstance(a, float):
                conv.append(ctypes.c_double(a))
            else:
                conv.append(ctypes.c_int(int(a)))
        fn.restype = ctypes.c_int
        rc = fn(*conv)
        if rc != 0:  # (a device error is not a result to go on from: nothing more is launched behind it)
            pytest.exit("%s returned hipError_t %d" % (name, rc), returncode=3)

    def _blocks(self, d):
        """The nine problem blocks of a call, in the probe's order."""
        return (self._cols(d["H"]), self._in(d["f"]), self._cols(d["G"]), self._in(d["h"]), self._cols(d["A"]),
                self._in(d["b"]), self._in(d["z"]), self._in(d["l"]), self._in(d["v"]))

    def _no_blocks(self):
        z = self._in(np.zeros(1))
        return (z,) * 9

    @staticmethod
    def _shape(d):
        return d["H"].shape[0], d["H"].shape[1], d["G"].shape[1], d["A"].shape[1]

    def assemble(self, d, sigma):
        """(Kr [count, 64, 64], dg [count, 64], atr [count, 64]) of assemble() behind load_guess()."""
        count, nz, nl, nv = self._shape(d)
        Kr, dg, atr = self._out((count, 64, 64)), self._out((count, 64)), self._out((count, 64))
        self._call("dwp_assemble", *self._blocks(d), self._in(d["gam"]), self._in(d["rvm"]), float(sigma), Kr, dg, atr,
                   self._ws(nz, nl, nv, count), nz, nl, nv, count)
        return Kr.cpu().numpy(), dg.cpu().numpy(), atr.cpu().numpy()

    def factor(self, img, n, rhs):
        """factor() and substitute(): (verdict [count], ord, dpiv, permv [count, 64], Lg [count, 64, 64] with
        Lg[q, k, t], x [count, 64]).  Where the verdict is false the other outputs keep their fill."""
        count = img.shape[0]
        t = self.torch
        verdict, ord_, permv = (self._out(s, t.int32) for s in ((count,), (count, 64), (count, 64)))
        dpiv, x = self._out((count, 64)), self._out((count, 64))
        ws = self._ws(n, 0, 1, count)
        self._call("dwp_factor", *self._no_blocks(), self._in(img), self._in(rhs), verdict, ord_, dpiv, permv, x, ws,
                   n, count)
        Lg = ws[:, : 64 * 64].reshape(count, 64, 64)
        return (verdict.cpu().numpy(), ord_.cpu().numpy(), dpiv.cpu().numpy(), permv.cpu().numpy(), Lg.cpu().numpy(),
                x.cpu().numpy())

    def static(self, img, n, rhs, order=2, spread_bits=32):
        """factor_solve_static(): (verdict [count], x [count, 64]; x keeps its fill where the verdict is false)."""
        count = img.shape[0]
        verdict, x = self._out((count,), self.torch.int32), self._out((count, 64))
        self._call("dwp_static", *self._no_blocks(), self._in(img), self._in(rhs), verdict, x, self._ws(n, 0, 1, count),
                   n, order, spread_bits, count)
        return verdict.cpu().numpy(), x.cpu().numpy()

    def products(self, d):
        """(y [count, nv], rz [count, nz], rl [count, nl]) of load_guess() and residual()."""
        count, nz, nl, nv = self._shape(d)
        y, rz, rl = self._out((count, nv)), self._out((count, nz)), self._out((count, nl))
        self._call("dwp_products", *self._blocks(d), y, rz, rl, self._ws(nz, nl, nv, count), nz, nl, nv, count)
        return y.cpu().numpy(), rz.cpu().numpy(), rl.cpu().numpy()[:, :nl]

    def feasibility(self, d, dz, dl, dv, tol):
        """The class feasibility(tol) returns for the directions (dz, dl, dv) [count, .]."""
        count, nz, nl, nv = self._shape(d)
        cls = self._out((count,), self.torch.int32)
        self._call("dwp_feasibility", *self._blocks(d), self._in(dz), self._in(dl), self._in(dv), float(tol), cls,
                   self._ws(nz, nl, nv, count), nz, nl, nv, count)
        return cls.cpu().numpy()
