"""ctypes wrapper over the probe library of tests/kernels/dense_probe.hip (tests/_build/libdense_probe.so, built
by `make -C fbstab_amd/csrc denseprobe`, which `rowprobe` and so __graft_entry__.build() depend on): numpy in,
numpy out, the buffers allocated with torch on cuda:0.  A helper module of tests/test_gpu_dense_stages.py.  A
missing library is a failure, not a skip.

Matrices go in and come out in mathematical shape, [count, rows, cols] (tests/dense_wave_rules.problem), and are
laid out by columns here, as the C-ABI and K are; images are [count, n, n], right-hand sides [count, n].  `want` is
the workgroup width asked for (256 or 64); the probe falls back from 64 to 256 as the product does, and
`layout()` says what it runs."""
import ctypes
import functools
import os

import numpy as np
import pytest

BUILD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build")
LIBRARY = "libdense_probe.so"
SENTINEL = np.uint64(0x7ff80000dead0000)  # what the step's K region holds where nothing was written
LAYOUT_FIELDS = ("threads", "wave", "k_global", "v_global", "a_lds", "lds_doubles", "nk")


@functools.lru_cache(maxsize=None)
def load():
    path = os.path.join(BUILD_DIR, LIBRARY)
    if not os.path.exists(path):
        pytest.fail("tests/_build/%s is missing: `make -C fbstab_amd/csrc denseprobe` "
                    "(__graft_entry__.build() builds it)" % LIBRARY)
    lib = ctypes.CDLL(path)
    lib.dp_layout.restype = ctypes.c_long
    return lib


class DenseProbe:
    """The probe library; every call computes `count` QPs, one workgroup each."""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = load()
        self.dev = torch.device("cuda:0")

    def layout(self, nz, nl, nv, want=256):
        """dict of LAYOUT_FIELDS and `scratch` (doubles per QP) for the instance the probe launches."""
        out = (ctypes.c_int * len(LAYOUT_FIELDS))()
        scratch = self.lib.dp_layout(nz, nl, nv, want, out)
        assert scratch >= 0, (nz, nl, nv, want)
        return dict(zip(LAYOUT_FIELDS, list(out)), scratch=scratch)

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
        shape = tuple(max(1, s) for s in shape)
        if dtype is None:
            return t.full(shape, float("nan"), dtype=t.float64, device=self.dev)
        return t.full(shape, -1, dtype=dtype, device=self.dev)

    def _scratch(self, nz, nl, nv, want, count):
        per = self.layout(nz, nl, nv, want)["scratch"]
        return self.torch.zeros((count, max(1, per)), dtype=self.torch.float64, device=self.dev)

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

    @staticmethod
    def _np(t, *cut):
        a = t.cpu().numpy()
        return a[tuple(slice(0, c) for c in cut)] if cut else a

    def _factor_out(self, count, n):
        t = self.torch
        return (self._out((count,), t.int32), self._out((count, n), t.int32), self._out((count, n * n)),
                self._out((count, 64)), self._out((count, 64), t.int32))

    def _factors(self, fo, count, n):
        verdict, perm, Kout, dpiv, ord_ = fo
        Kf = self._np(Kout, count, n * n).reshape(count, n, n).transpose(0, 2, 1)  # Kf[q, i, j] = K[i + j n]
        return dict(verdict=self._np(verdict), perm=self._np(perm, count, n), K=Kf, flat=self._np(Kout, count, n * n),
                    dpiv=self._np(dpiv), ord=self._np(ord_))

    def products(self, d, want=256):
        """dict(y, rz, rl, nrm, a_rows, a_cols): load_guess, residual, forcing_norm, and the LDS copy of A read
        back by A_row_dot / A_col_dot ([count, nv, nz]; NaN where A is not in LDS)."""
        count, nz, nl, nv = self._shape(d)
        y, rz, rl, nrm = self._out((count, nv)), self._out((count, nz)), self._out((count, nl)), self._out((count,))
        ar, ac = self._out((count, nz * nv)), self._out((count, nz * nv))
        self._call("dp_products", *self._blocks(d), y, rz, rl, nrm, ar, ac, self._scratch(nz, nl, nv, want, count),
                   nz, nl, nv, want, count)
        back = lambda a: self._np(a).reshape(count, nz, nv).transpose(0, 2, 1)
        return dict(y=self._np(y), rz=self._np(rz), rl=self._np(rl, count, nl), nrm=self._np(nrm), a_rows=back(ar),
                    a_cols=back(ac))

    def feasibility(self, d, dz, dl, dv, tol, want=256):
        """The class feasibility(tol) returns for the directions (dz, dl, dv) [count, .]."""
        count, nz, nl, nv = self._shape(d)
        cls = self._out((count,), self.torch.int32)
        self._call("dp_feasibility", *self._blocks(d), self._in(dz), self._in(dl), self._in(dv), float(tol), cls,
                   self._scratch(nz, nl, nv, want, count), nz, nl, nv, want, count)
        return self._np(cls)

    def factor(self, img, rhs, nv=4, want=256):
        """ldlt and ldlt_solve on images [count, n, n] behind the path of the shape (n, 0, nv): dict(verdict, perm,
        K [count, n, n] - what the K region holds afterwards, K[q, i, j] = entry i + j n -, flat, dpiv, ord, x).
        Where the verdict is false the other outputs keep their fill."""
        count, n = img.shape[0], img.shape[1]
        fo = self._factor_out(count, n)
        x = self._out((count, n))
        self._call("dp_factor", *self._no_blocks(), self._cols(img), self._in(rhs), *fo, x,
                   self._scratch(n, 0, nv, want, count), n, nv, want, count)
        return dict(self._factors(fo, count, n), x=self._np(x, count, n))

    def step(self, d, zb, lb, vb, sigma, alpha=0.95, want=256, adjoint=False, h_step=None):
        """newton_step<false> behind load_guess and residual with xbar = (zb, lb, vb); adjoint=True:
        dense_adjoint with the seeds (zb, lb, vb) = (gz, gl, gv).  dict of the factors (as factor()), y, rz, rl,
        gam, rvm, yb (adjoint only) and dz, dl, dv, adz, wz, wl.  The K region starts filled with SENTINEL; h_step:
        the H the step itself reads (default: the problem's)."""
        count, nz, nl, nv = self._shape(d)
        n = nz + nl
        fo = self._factor_out(count, n)
        names = (("y", nv), ("rz", nz), ("rl", nl), ("dz", nz), ("dl", nl), ("dv", nv), ("adz", nv), ("wz", nz),
                 ("wl", nl), ("gam", nv), ("rvm", nv), ("yb", nv))
        outs = [self._out((count, m)) for _, m in names]
        self._call("dp_step_adjoint" if adjoint else "dp_step", *self._blocks(d),
                   self._cols(d["H"] if h_step is None else h_step), self._in(zb), self._in(lb), self._in(vb), float(sigma), float(alpha), *fo, *outs, self._scratch(nz, nl, nv, want, count),
                   nz, nl, nv, want, count)
        r = self._factors(fo, count, n)
        for (name, m), o in zip(names, outs):
            r[name] = self._np(o, count, m)
        return r
