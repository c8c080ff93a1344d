"""TEST INFRASTRUCTURE ONLY: the single-threaded host compilations of the device logic (hostsim.cc, adjoint.cc,
dense_adjoint.cc, tangent.cc, dense_stage.cc, against the <hip/hip_runtime.h> of shim/) and their ctypes wrappers.  Beside them,
with no wrapper here: runtime_shim/ (a heap-backed <hip/hip_runtime.h>: the runtime calls, not the device environment)
and stage_driver.cc, the stand-alone program over fbstab_amd/csrc/fb_host_stage.h that tests/test_host_stage.py
builds and runs."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle.oracle_py import SolverOut, Options, default_options, _out_to_numpy, _p
from tests.linear_reference import SIGMA, is_mpc, names_of, lengths_of

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "fbstab_amd", "csrc")
NO_CONTRACTION = "-ffp-contract=off"   # host builds of the device headers round every product (no fused multiply-adds)


def build(so_name, source, headers):
    """Compiles ``source`` (of this directory) into ``so_name`` beside it unless that is newer than the source,
    the shim and the ``headers`` of fbstab_amd/csrc it includes.  Returns the library's path."""
    so = os.path.join(_HERE, so_name)
    src = os.path.join(_HERE, source)
    shim = os.path.join(_HERE, "shim")  # <hip/hip_runtime.h> for a host of one thread
    deps = [src, os.path.join(shim, "hip", "hip_runtime.h")] + [os.path.join(_CSRC, f) for f in headers]
    if not (os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", NO_CONTRACTION, "-I" + shim,
                               "-Wno-attributes", "-Wno-unknown-pragmas", "-o", so, src])
    return so


class HostSim:
    def __init__(self):
        self.lib = C.CDLL(build("libhostsim.so", "hostsim.cc", ("fb_common.h", "fb_algorithm.h", "fb_mpc.h", "fb_dense.h")))

    def solve_mpc(self, prob, x0guess=None, opts=None):
        opts = opts or default_options()
        B = prob.batch
        z = np.zeros((B, prob.nz)); l = np.zeros((B, prob.nl))
        v = np.zeros((B, prob.nv)); y = np.zeros((B, prob.nv))
        if x0guess is not None:
            z[:] = x0guess[0]; l[:] = x0guess[1]; v[:] = x0guess[2]
        out = (SolverOut * B)()
        N, nx, nu, nc = prob.sizes()
        for b in range(B):
            a = {k: np.ascontiguousarray(prob.arrays[k][b]) for k in prob.arrays}
            self.lib.hostsim_mpc_solve(
                N, nx, nu, nc, _p(a["Q"]), _p(a["R"]), _p(a["S"]), _p(a["q"]), _p(a["r"]),
                _p(a["A"]), _p(a["B"]), _p(a["c"]), _p(a["E"]), _p(a["L"]), _p(a["d"]),
                _p(a["x0"]), _p(z[b]), _p(l[b]), _p(v[b]), _p(y[b]), C.byref(opts),
                C.byref(out[b]))
        return z, l, v, y, _out_to_numpy(out)

    def solve_dense(self, prob, x0guess=None, opts=None):
        opts = opts or default_options()
        B = prob.batch
        z = np.zeros((B, prob.nz)); l = np.zeros((B, max(prob.nl, 1)))[:, :prob.nl]
        l = np.ascontiguousarray(l)
        v = np.zeros((B, prob.nv)); y = np.zeros((B, prob.nv))
        if x0guess is not None:
            z[:] = x0guess[0]; l[:] = x0guess[1]; v[:] = x0guess[2]
        out = (SolverOut * B)()
        for b in range(B):
            a = {k: np.ascontiguousarray(prob.arrays[k][b]) for k in prob.arrays}
            lb = l[b] if prob.nl else np.zeros(1)
            G = a["G"] if prob.nl else np.zeros(1)
            h = a["h"] if prob.nl else np.zeros(1)
            self.lib.hostsim_dense_solve(
                prob.nz, prob.nl, prob.nv, _p(a["H"]), _p(a["f"]), _p(G), _p(h),
                _p(a["A"]), _p(a["b"]), _p(z[b]), _p(lb), _p(v[b]), _p(y[b]),
                C.byref(opts), C.byref(out[b]))
            if prob.nl:
                l[b] = lb
        return z, l, v, y, _out_to_numpy(out)

    def newton_mpc(self, prob, b, x, xbar, sigma, alpha, refine_sweeps=0):
        """One Newton step of the flat-vector device logic for QP ``b`` at x = (z, l, v), xbar (hostsim.cc:
        hostsim_mpc_newton_refined), followed by ``refine_sweeps`` refinement sweeps.  Returns a dict."""
        N, nx, nu, nc = prob.sizes()
        a = {k: np.ascontiguousarray(prob.arrays[k][b]) for k in prob.arrays}
        nz, nl, nv = prob.nz, prob.nl, prob.nv
        out = np.zeros(3 * nz + 3 * nl + 2 * nv + 2)
        z, l, v = (np.ascontiguousarray(t, dtype=np.float64) for t in x)
        zb, lb, vb = (np.ascontiguousarray(t, dtype=np.float64) for t in xbar)
        self.lib.hostsim_mpc_newton_refined.argtypes = [C.c_int] * 4 + [C.c_void_p] * 18 + [C.c_double, C.c_double, C.c_int, C.c_void_p]
        rc = self.lib.hostsim_mpc_newton_refined(
            N, nx, nu, nc, _p(a["Q"]), _p(a["R"]), _p(a["S"]), _p(a["q"]), _p(a["r"]), _p(a["A"]), _p(a["B"]),
            _p(a["c"]), _p(a["E"]), _p(a["L"]), _p(a["d"]), _p(a["x0"]), _p(z), _p(l), _p(v), _p(zb), _p(lb), _p(vb),
            C.c_double(sigma), C.c_double(alpha), refine_sweeps, _p(out))
        o, r = 0, {"ok": rc == 0}
        for name, n in (("dz", nz), ("dl", nl), ("dv", nv), ("adz", nv), ("wz", nz), ("wl", nl), ("rz", nz), ("rl", nl)):
            r[name] = out[o:o + n].copy()
            o += n
        r["lin2_before"], r["lin2_after"] = out[o], out[o + 1]
        return r


def _pad(a):
    return a if a.size else np.zeros(1)


class HostAdjoint:
    """The adjoint of one QP on one host thread, ``kind`` "mpc": the flat-vector adjoint of fb_mpc.h (adjoint.cc);
    "dense": DenseProblem<Ctx<1>> of fb_dense.h and dense_adjoint_contract of fb_adjoint.h (dense_adjoint.cc)."""

    def __init__(self, kind="mpc"):
        if kind == "mpc":
            self.lib = C.CDLL(build("libhostsim_adjoint.so", "adjoint.cc", ("fb_common.h", "fb_mpc.h")))
            self.entry, nsize = self.lib.hostsim_mpc_adjoint, 4
        else:
            self.lib = C.CDLL(build("libhostsim_dense_adjoint.so", "dense_adjoint.cc",
                                    ("fb_common.h", "fb_adjoint.h", "fb_mpc.h", "fb_dense.h")))
            self.entry, nsize = self.lib.hostsim_dense_adjoint, 3
            self.lib.hostsim_dense_layout.argtypes = [C.c_int] * 4 + [C.c_void_p]
        self.entry.argtypes = [C.c_int] * nsize + [C.c_void_p] * 7 + [C.c_double, C.c_double, C.c_void_p, C.c_void_p]

    def layout(self, nz, nl, nv, nthreads=256):
        """Dense: DenseLayout::init(nz, nl, nv, nthreads): dict(wave, k_global, v_global, a_lds, lds_doubles)."""
        out = (C.c_int * 5)()
        self.lib.hostsim_dense_layout(nz, nl, nv, nthreads, out)
        return dict(zip(("wave", "k_global", "v_global", "a_lds", "lds_doubles"), list(out)))

    def adjoint(self, p, q, x, seeds, sigma=SIGMA, alpha=0.95, want=None):
        """Adjoint of QP ``q`` at x = (z, l, v) for seeds (gz, gl, gv) (gl / gv may be None): (status, (dz, dl,
        dv), gradients) - those of ``want`` (default: all)."""
        names, lens = names_of(p), lengths_of(p)
        sizes = p.sizes() if is_mpc(p) else (p.nz, p.nl, p.nv)
        keep = [_pad(np.ascontiguousarray(p.arrays[k][q], dtype=np.float64)) for k in names]
        data = (C.c_void_p * len(names))(*[a.ctypes.data for a in keep])
        grads = {k: np.full(lens[k], np.nan) for k in (names if want is None else want)}
        bufs = {k: _pad(g) for k, g in grads.items()}
        gptr = (C.c_void_p * len(names))(*[bufs[k].ctypes.data if k in bufs else None for k in names])
        f64 = lambda a: None if a is None else _pad(np.ascontiguousarray(a, dtype=np.float64))
        z, l, v = (f64(t) for t in x)
        gz, gl, gv = (f64(t) for t in seeds)
        adj = np.full(p.nz + p.nl + p.nv, np.nan)
        ptr = lambda a: None if a is None else a.ctypes.data
        st = self.entry(*sizes, data, ptr(z), ptr(l), ptr(v), ptr(gz), ptr(gl), ptr(gv), sigma, alpha,
                        adj.ctypes.data, gptr)
        for k in grads:
            if grads[k].size:
                grads[k] = bufs[k]
        return st, (adj[:p.nz], adj[p.nz:p.nz + p.nl], adj[p.nz + p.nl:]), grads


class HostTangent:
    """mpc_tangent_stage / dense_tangent of fb_tangent.h on one host thread (tangent.cc)."""

    def __init__(self):
        self.lib = C.CDLL(build("libhostsim_tangent.so", "tangent.cc", ("fb_common.h", "fb_tangent.h")))
        self.lib.hostsim_mpc_tangent_rhs.argtypes = [C.c_int] * 4 + [C.c_void_p] * 7
        self.lib.hostsim_dense_tangent_rhs.argtypes = [C.c_int] * 4 + [C.c_void_p] * 7

    def rhs(self, p, x, d, budget=8192):
        """(gz, gl, gv) of one QP at x = (z, l, v) for the perturbations ``d`` (name -> flat array or None).
        Dense: ``budget`` doubles of LDS decide the column block; ``self.cb`` is what came of it."""
        names = names_of(p)
        keep = [None if d.get(k) is None else _pad(np.ascontiguousarray(d[k], dtype=np.float64)) for k in names]
        ptrs = (C.c_void_p * len(names))(*[None if a is None else a.ctypes.data for a in keep])
        z, l, v = (_pad(np.ascontiguousarray(t, dtype=np.float64)) for t in x)
        gz, gl, gv = (np.full(max(n, 1), np.nan) for n in (p.nz, p.nl, p.nv))
        if is_mpc(p):
            self.lib.hostsim_mpc_tangent_rhs(p.N, p.nx, p.nu, p.nc, ptrs, z.ctypes.data, l.ctypes.data,
                                             v.ctypes.data, gz.ctypes.data, gl.ctypes.data, gv.ctypes.data)
        else:
            self.cb = self.lib.hostsim_dense_tangent_rhs(p.nz, p.nl, p.nv, budget, ptrs, z.ctypes.data,
                                                         l.ctypes.data, v.ctypes.data, gz.ctypes.data,
                                                         gl.ctypes.data, gv.ctypes.data)
            assert self.cb >= 1, "not one column fits the budget"
        return gz[:p.nz], gl[:p.nl], gv[:p.nv]


class HostDenseStage:
    """The stages of fb_dense.h on one host thread (dense_stage.cc): DenseLayout::init as compiled, and ldlt with
    ldlt_solve, newton_step and dense_adjoint of DenseProblem<Ctx<1>>, with the outputs of tests/dense_probe.py."""
    STEP_OUT = (("y", "nv"), ("rz", "nz"), ("rl", "nl"), ("dz", "nz"), ("dl", "nl"), ("dv", "nv"), ("adz", "nv"),
                ("wz", "nz"), ("wl", "nl"), ("gam", "nv"), ("rvm", "nv"), ("yb", "nv"))

    def __init__(self):
        self.lib = C.CDLL(build("libhostsim_dense_stage.so", "dense_stage.cc",
                                ("fb_common.h", "fb_adjoint.h", "fb_mpc.h", "fb_dense.h")))
        self.lib.hostsim_dense_path.restype = C.c_long
        self.lib.hostsim_dense_path.argtypes = [C.c_int] * 4 + [C.c_void_p]
        self.lib.hostsim_dense_stage_factor.argtypes = [C.c_int] * 2 + [C.c_void_p] * 5
        self.lib.hostsim_dense_stage_step.argtypes = ([C.c_int] * 3 + [C.c_void_p] * 8 + [C.c_double] * 2 + [C.c_int]
                                                      + [C.c_void_p] * 3)

    def layout(self, nz, nl, nv, nthreads):
        out = (C.c_int * 7)()
        scratch = self.lib.hostsim_dense_path(nz, nl, nv, nthreads, out)
        names = ("wave", "k_global", "v_global", "a_lds", "lds_doubles", "lda", "nk")
        return dict(zip(names, list(out)), scratch=scratch)

    def factor(self, img, rhs, nv=4):
        """As DenseProbe.factor (the K region, perm, x; no dpiv / ord: one thread takes ldlt_impl)."""
        count, n = img.shape[0], img.shape[1]
        out = dict(verdict=np.zeros(count, dtype=np.int32), perm=np.full((count, n), -1, dtype=np.int32),
                   flat=np.full((count, n * n), np.nan), x=np.full((count, n), np.nan))
        for q in range(count):
            cols = np.ascontiguousarray(np.asarray(img[q], dtype=np.float64).T)
            b = np.ascontiguousarray(rhs[q], dtype=np.float64)
            out["verdict"][q] = self.lib.hostsim_dense_stage_factor(n, nv, cols.ctypes.data, b.ctypes.data,
                                                                    out["perm"][q].ctypes.data,
                                                                    out["flat"][q].ctypes.data, out["x"][q].ctypes.data)
        out["K"] = out["flat"].reshape(count, n, n).transpose(0, 2, 1)
        return out

    def step(self, d, xb, sigma, alpha=0.95, adjoint=False, h_step=None):
        """As DenseProbe.step, for a batch of tests/dense_wave_rules.problem's kind."""
        count, nz, nl, nv = d["H"].shape[0], d["H"].shape[1], d["G"].shape[1], d["A"].shape[1]
        n = nz + nl
        size = dict(nz=nz, nl=nl, nv=nv)
        out = dict(verdict=np.zeros(count, dtype=np.int32), perm=np.full((count, n), -1, dtype=np.int32),
                   flat=np.full((count, n * n), np.nan))
        for name, m in self.STEP_OUT:
            out[name] = np.full((count, max(1, size[m])), np.nan)
        cm = lambda M: _pad(np.ascontiguousarray(np.asarray(M, dtype=np.float64).T))
        vec = lambda a: _pad(np.ascontiguousarray(a, dtype=np.float64))
        for q in range(count):
            keep = [cm(d["H"][q]), vec(d["f"][q]), cm(d["G"][q]), vec(d["h"][q]), cm(d["A"][q]), vec(d["b"][q])]
            data = (C.c_void_p * 6)(*[a.ctypes.data for a in keep])
            pt = [vec(d[k][q]) for k in ("z", "l", "v")] + [cm((d["H"] if h_step is None else h_step)[q])]
            pt += [vec(t[q]) for t in xb]
            outs = (C.c_void_p * 12)(*[out[name][q].ctypes.data for name, _ in self.STEP_OUT])
            out["verdict"][q] = self.lib.hostsim_dense_stage_step(
                nz, nl, nv, data, *[a.ctypes.data for a in pt], sigma, alpha, int(adjoint),
                out["perm"][q].ctypes.data, out["flat"][q].ctypes.data, outs)
        for name, m in self.STEP_OUT:
            out[name] = out[name][:, :size[m]]
        out["K"] = out["flat"].reshape(count, n, n).transpose(0, 2, 1)
        return out
