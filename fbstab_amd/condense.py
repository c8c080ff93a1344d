"""Condensed MPC: the states of an MPC QP eliminated on the device, the dense QP in the inputs solved by a
``FBstabDenseBatch`` and the MPC point rebuilt (include/fbstab_hip.h: fbstab_hip_mpc_condense_batch,
fbstab_hip_mpc_expand_batch).  The route for state-heavy shapes that no record kernel takes (nx above 24 with few
inputs and a short horizon): after elimination the cost of a solve no longer depends on nx.  It is the caller's
choice; ``FBstabMpcBatch`` never takes it by itself."""
import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import hip_api
from .hip_api import (DENSE_ARR, MPC_SEQ, FBstabDenseBatch, _CondensedMap, _CondensedRefGrad, _CondensedRefImages,
                      _CondensedRefs,
                      _CondensedSweepLog, _DenseBatch, _DenseOutBatch, _MpcBatch, _MpcGradBatch, _Plant,
                      _SweepScenario, _VarBatch, _check, _fill_block, _is_torch)

MATRICES, VECTORS, ALL = 1, 2, 3
_WHAT = {"matrices": MATRICES, "vectors": VECTORS, "all": ALL}
_MATRIX_SEQ = ("Q", "R", "S", "A", "B", "E", "L")
AFFINE, RECONDENSE = 0, 1
_SWEEP_MODE = {"affine": AFFINE, "recondense": RECONDENSE}
_REF_SEQ = ("q", "r", "c", "d")   # the sequences that may move along a sweep, in the order of fbstab_condensed_refs_t


def condensed_sizes(N: int, nx: int, nu: int, nc: int) -> Dict[str, int]:
    """fbstab_hip_mpc_condensed_sizes: ``nz``, ``nv`` of the condensed QP and the ``lds_bytes`` one workgroup of
    the condensing kernels needs; raises where the shape does not fit the LDS rule."""
    lib = hip_api.load_library()
    nz, nv, lds = C.c_int(), C.c_int(), C.c_longlong()
    _check(lib, lib.fbstab_hip_mpc_condensed_sizes(N, nx, nu, nc, C.byref(nz), C.byref(nv), C.byref(lds)))
    return dict(nz=nz.value, nv=nv.value, lds_bytes=lds.value)


def condensed_multi_sizes(N: int, nx: int, nu: int, nc: int, nrhs: int, rhs_per_group: int = 0) -> Dict[str, int]:
    """fbstab_hip_mpc_condensed_multi_sizes: what the many-right-hand-side calls of the condensed route use for
    ``nrhs`` right-hand sides (``nx`` of them in x0 mode) - ``rhs_per_group`` (0 asks for the library's rule), the
    ``lds_bytes`` of a workgroup and the ``work_doubles_per_qp`` of the caller's work array; raises where the LDS
    rule refuses."""
    lib = hip_api.load_library()
    used, lds, work = C.c_int(), C.c_longlong(), C.c_longlong()
    _check(lib, lib.fbstab_hip_mpc_condensed_multi_sizes(N, nx, nu, nc, nrhs, rhs_per_group, C.byref(used),
                                                         C.byref(lds), C.byref(work)))
    return dict(rhs_per_group=used.value, lds_bytes=lds.value, work_doubles_per_qp=work.value)


def condensed_sweep_sizes(N: int, nx: int, nu: int, nc: int, traj_per_group: int = 0,
                          shared_map: bool = True) -> Dict[str, int]:
    """fbstab_hip_mpc_condensed_sweep_sizes: what the closed-loop sweep of the condensed route uses -
    ``traj_per_group`` (0 asks for the library's rule), the ``lds_bytes`` of a workgroup of the step kernel (with
    ``shared_map`` the one image M of a shared model is staged into LDS) and the ``work_doubles_per_traj`` of the
    caller's work array; raises where the LDS rule refuses."""
    lib = hip_api.load_library()
    used, lds, work = C.c_int(), C.c_longlong(), C.c_longlong()
    _check(lib, lib.fbstab_hip_mpc_condensed_sweep_sizes(N, nx, nu, nc, traj_per_group, 1 if shared_map else 0,
                                                         C.byref(used), C.byref(lds), C.byref(work)))
    return dict(traj_per_group=used.value, lds_bytes=lds.value, work_doubles_per_traj=work.value)


def condensed_reference_sizes(N: int, nx: int, nu: int, nc: int, steps: int, refs_per_group: int = 0) -> Dict[str, int]:
    """fbstab_hip_mpc_condensed_reference_sizes: what the images of per-step references use for ``steps`` steps -
    ``refs_per_group`` (0 asks for the library's rule) and the ``lds_bytes`` of a workgroup; raises where the LDS
    rule refuses."""
    lib = hip_api.load_library()
    used, lds = C.c_int(), C.c_longlong()
    _check(lib, lib.fbstab_hip_mpc_condensed_reference_sizes(N, nx, nu, nc, steps, refs_per_group, C.byref(used),
                                                             C.byref(lds)))
    return dict(refs_per_group=used.value, lds_bytes=lds.value)


def condensed_sweep_adjoint_sizes(N: int, nx: int, nu: int, nc: int, traj_per_group: int = 0,
                                  shared_map: bool = True) -> Dict[str, int]:
    """fbstab_hip_mpc_condensed_sweep_adjoint_sizes: what the adjoint through the closed-loop sweep uses -
    ``traj_per_group`` and ``lds_bytes`` of its step kernel, and the doubles of the caller's work array per trajectory
    without (``work_doubles_per_traj``) and with (``work_doubles_per_traj_grad``) gradients of the data."""
    lib = hip_api.load_library()
    used, lds, work, workg = C.c_int(), C.c_longlong(), C.c_longlong(), C.c_longlong()
    _check(lib, lib.fbstab_hip_mpc_condensed_sweep_adjoint_sizes(N, nx, nu, nc, traj_per_group, 1 if shared_map else 0,
                                                                 C.byref(used), C.byref(lds), C.byref(work),
                                                                 C.byref(workg)))
    return dict(traj_per_group=used.value, lds_bytes=lds.value, work_doubles_per_traj=work.value,
                work_doubles_per_traj_grad=workg.value)


def condensed_sweep_tangent_sizes(N: int, nx: int, nu: int, nc: int, traj_per_group: int = 0,
                                  shared_map: bool = True) -> Dict[str, int]:
    """fbstab_hip_mpc_condensed_sweep_tangent_sizes: what forward mode through the closed-loop sweep uses -
    ``traj_per_group`` and ``lds_bytes`` of its step kernel (those of the forward sweep's), and the
    ``work_doubles_per_traj`` of the caller's work array."""
    lib = hip_api.load_library()
    used, lds, work = C.c_int(), C.c_longlong(), C.c_longlong()
    _check(lib, lib.fbstab_hip_mpc_condensed_sweep_tangent_sizes(N, nx, nu, nc, traj_per_group, 1 if shared_map else 0,
                                                                 C.byref(used), C.byref(lds), C.byref(work)))
    return dict(traj_per_group=used.value, lds_bytes=lds.value, work_doubles_per_traj=work.value)


class CondensedMpc:
    """``CondensedMpc(N, nx, nu, nc, max_batch)``: owns ``.dense``, a ``FBstabDenseBatch((N + 1) nu, 0, (N + 1) nc)``
    (public: ``SetFactorisation``, ``UpdateOptions`` ... apply to it), and the condensed images ``H, f, A, b`` as
    torch tensors on the device.  Inputs are torch tensors on ``device``; numpy inputs are uploaded through torch
    by this class and the results copied back."""

    def __init__(self, N: int, nx: int, nu: int, nc: int, max_batch: int = 1, device: int = 0):
        self._lib = hip_api.load_library()
        import torch
        self._torch = torch
        self.N, self.nx, self.nu, self.nc = N, nx, nu, nc
        self.device, self.max_batch = device, max_batch
        s = condensed_sizes(N, nx, nu, nc)
        self.nzc, self.nv, self.lds_bytes = s["nz"], s["nv"], s["lds_bytes"]
        self.nz, self.nl = (N + 1) * (nx + nu), (N + 1) * nx
        self.seq_len = [(N + 1) * nx * nx, (N + 1) * nu * nu, (N + 1) * nu * nx, (N + 1) * nx, (N + 1) * nu,
                        N * nx * nx, N * nx * nu, N * nx, (N + 1) * nc * nx, (N + 1) * nc * nu, (N + 1) * nc, nx]
        self.dense = FBstabDenseBatch(self.nzc, 0, self.nv, max_batch, device)
        self._dev = torch.device("cuda", device)
        self._len = dict(H=self.nzc * self.nzc, f=self.nzc, A=self.nv * self.nzc, b=self.nv)
        self._img = {}      # the condensed images of the last Condense: name -> (rows, len) tensor
        self.generation = 0  # counts the calls that wrote into them (autograd: are the forward's images still there?)

    def close(self):
        self.dense.close()

    # ---- placement -------------------------------------------------------------------------------------------
    def _to_dev(self, a):
        t = self._torch
        if _is_torch(a):
            assert a.is_cuda and a.device.index == self.device, "tensors live on the solver's device"
            return a
        return t.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self._dev)

    def _data(self, data):
        return {k: self._to_dev(data[k]) for k in MPC_SEQ}

    def _stream(self):
        return self._torch.cuda.current_stream(self._dev).cuda_stream

    def _mpc_block(self, data, B):
        blk, flags = _MpcBatch(), []
        _fill_block(blk, MPC_SEQ, self.seq_len, data, B, flags)
        assert all(flags)
        return blk

    def _images(self, names, rows_of):
        for k in names:
            rows = rows_of(k)
            t = self._img.get(k)
            if t is None or t.shape[0] != rows:
                self._img[k] = self._torch.empty((rows, self._len[k]), dtype=self._torch.float64, device=self._dev)

    # ---- the maps --------------------------------------------------------------------------------------------
    def _condense(self, data, what):
        B = data["x0"].shape[0]
        assert 1 <= B <= self.max_batch, (B, self.max_batch)
        w = _WHAT[what] if isinstance(what, str) else int(what)
        shared = B > 1 and all(data[k].shape[0] == 1 for k in _MATRIX_SEQ)
        names = [k for k, bit in (("H", MATRICES), ("f", VECTORS), ("A", MATRICES), ("b", VECTORS)) if w & bit]
        self._images(names, lambda k: 1 if (shared and k in ("H", "A")) else B)
        out = _DenseOutBatch()
        for k in names:
            t = self._img[k]
            i = DENSE_ARR.index(k)
            out.base[i], out.stride[i] = t.data_ptr(), (0 if (t.shape[0] == 1 and B > 1) else self._len[k])
        blk = self._mpc_block(data, B)
        s = self._stream()
        self.generation += 1
        _check(self._lib, self._lib.fbstab_hip_mpc_condense_batch(
            self.N, self.nx, self.nu, self.nc, B, C.byref(blk), w, C.byref(out), self.device,
            C.c_void_p(s) if s else None))
        return B

    def Condense(self, data: Dict[str, object], what="all") -> Dict[str, object]:
        """Condenses ``data`` (the 12 sequences, ``(batch, len)`` or ``(1, len)`` for a shared one) and returns the
        dict ``H, f, A, b`` of this object's image tensors (column-major images, ``(batch, len)``).  ``what``:
        "all", "matrices" (H and A only) or "vectors" (f and b only: x0, q, r, c, d moved; the other two keep what
        an earlier call wrote).  H and A are ONE ``(1, len)`` image where every matrix sequence of ``data`` is
        shared.  Queued on torch's current stream."""
        self._condense(self._data(data), what)
        return {k: self._img[k] for k in ("H", "f", "A", "b") if k in self._img}

    def _expand(self, data, U, v, y, z, l, vo, yo):
        B = U.shape[0]
        xc, x = _VarBatch(), _VarBatch()
        for i, (a, n) in enumerate(((U, self.nzc), (None, 0), (v, self.nv), (y, self.nv))):
            if a is not None:
                assert a.shape == (B, n) and a.stride(1) == 1 and a.is_cuda
                xc.base[i], xc.stride[i] = a.data_ptr(), (a.stride(0) if B > 1 else n)
        for i, (a, n) in enumerate(((z, self.nz), (l, self.nl), (vo, self.nv), (yo, self.nv))):
            if a is not None:
                assert a.shape == (B, n) and (a.stride(1) == 1 or n <= 1) and a.is_cuda
                x.base[i], x.stride[i] = a.data_ptr(), (a.stride(0) if B > 1 else n)
        blk = self._mpc_block(data, B)
        s = self._stream()
        _check(self._lib, self._lib.fbstab_hip_mpc_expand_batch(
            self.N, self.nx, self.nu, self.nc, B, C.byref(blk), C.byref(xc), C.byref(x), self.device,
            C.c_void_p(s) if s else None))

    def Expand(self, data: Dict[str, object], U, v, y):
        """``(z, l, v, y)`` of the MPC QP from the condensed point ``(U, v, y)``: the states by the dynamics, the
        costates from the stationarity condition, ``v`` and ``y`` copied.  Certificates of an infeasibility exit are
        NOT translated.  Returns numpy arrays where ``U`` is one."""
        host = not _is_torch(U)
        t = self._torch
        d = self._data(data)
        U, v, y = (self._to_dev(a) for a in (U, v, y))
        B = U.shape[0]
        out = [t.empty((B, n), dtype=t.float64, device=self._dev) for n in (self.nz, self.nl, self.nv, self.nv)]
        self._expand(d, U, v, y, *out)
        return tuple(a.cpu().numpy() for a in out) if host else tuple(out)

    def Adjoint(self, data: Dict[str, object], z, l, v, gz, gl=None, gv=None, sigma: float = 0.0,
                want: Optional[Sequence[str]] = None, adj: bool = False) -> Dict[str, object]:
        """Reverse-mode derivative of the solution map on this route (fbstab_hip_mpc_condensed_adjoint_batch): what
        ``FBstabMpcBatch.Adjoint`` returns - dL/d(sequence) for every name of ``want`` (default: all 12 of MPC_SEQ,
        ``(batch, len)``), ``"status"`` (``(batch,)`` int32: 1 where the dense factorisation failed and the gradients
        are zero) and, with ``adj=True``, ``"dz", "dl", "dv"`` - for the seeds ``gz, gl, gv`` = dL/d(z, l, v) at the
        point ``(z, l, v)`` (``gl``/``gv`` None: zero).  It runs on the condensed images of the last ``Condense`` or
        ``Solve``, which must be those of ``data``: the seeds are condensed, the dense handle's adjoint solves and
        is refined once on its own residual, the step is expanded and contracted - six launches on torch's current
        stream.  The step carries the O(sigma)
        bias of a regularisation in the condensed variables (include/fbstab_hip.h); ``sigma <= 0``: 1e-8.  A shared
        ``(1, len)`` sequence gets per-QP gradients like every other.  Returns numpy arrays where ``z`` is one."""
        t = self._torch
        host = not _is_torch(z)
        want = tuple(MPC_SEQ if want is None else want)
        assert not set(want) - set(MPC_SEQ), set(want) - set(MPC_SEQ)
        d = self._data(data)
        zd, ld, vd, gzd = (self._to_dev(a) for a in (z, l, v, gz))
        gld, gvd = (None if a is None else self._to_dev(a) for a in (gl, gv))
        B = zd.shape[0]
        assert 1 <= B <= self.max_batch, (B, self.max_batch)
        img = self._img
        assert all(k in img for k in ("H", "f", "A", "b")), "Adjoint before anything was condensed"
        assert img["f"].shape[0] == B and img["H"].shape[0] in (1, B), "the images are those of another batch"
        var_lens = (self.nz, self.nl, self.nv)
        xb = hip_api._fill_vars((zd, ld, vd), var_lens, B, [])
        sb = hip_api._fill_vars((gzd, gld, gvd), var_lens, B, [], optional=True)
        dense = _DenseBatch()
        for k in ("H", "f", "A", "b"):
            a, i = img[k], DENSE_ARR.index(k)
            dense.base[i], dense.stride[i] = a.data_ptr(), (0 if (a.shape[0] == 1 and B > 1) else self._len[k])
        mk = lambda shape, dtype=t.float64: t.zeros(shape, dtype=dtype, device=self._dev)
        res = {k: mk((B, n)) for k, n in zip(MPC_SEQ, self.seq_len) if k in want}
        grad = _MpcGradBatch()
        _fill_block(grad, MPC_SEQ, self.seq_len, res, B, [], optional=True, shared=False)
        ab = None
        if adj:
            for k, n in zip(("dz", "dl", "dv"), var_lens):
                res[k] = mk((B, n))
            ab = hip_api._fill_vars((res["dz"], res["dl"], res["dv"]), var_lens, B, [])
        work = t.empty((B, 5 * self.nzc + 3 * self.nv), dtype=t.float64, device=self._dev)
        status = mk((B,), t.int32)
        blk = self._mpc_block(d, B)
        s = self._stream()
        _check(self._lib, self._lib.fbstab_hip_mpc_condensed_adjoint_batch(
            self.dense._h, self.N, self.nx, self.nu, self.nc, B, C.byref(blk), C.byref(dense), C.byref(xb),
            C.byref(sb), C.c_double(sigma), C.byref(grad), C.byref(ab) if ab is not None else None,
            C.c_void_p(work.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(s) if s else None))
        res["status"] = status
        if host:
            res = {k: a.cpu().numpy() for k, a in res.items()}
        return res

    def Tangent(self, data: Dict[str, object], z, l, v, ddata: Dict[str, object], sigma: float = 0.0,
                rhs: bool = False) -> Dict[str, object]:
        """Forward-mode derivative of the solution map on this route (fbstab_hip_mpc_condensed_tangent_batch): what
        ``FBstabMpcBatch.Tangent`` returns - the first-order change ``dz, dl, dv`` (``(batch, n)``) of the solutions
        at the point ``(z, l, v)`` for the perturbation ``ddata`` of the problem data (name -> ``(batch, len)``
        direction, or ``(1, len)`` for one direction shared by the batch; absent names and None are zero
        perturbations; dQ and dR enter through their symmetric part), ``"status"`` (``(batch,)`` int32: 1 where the
        dense factorisation failed and the tangent is zero) and, with ``rhs=True``, the seeds ``"gz", "gl", "gv"`` of
        the tangent system.  It runs on the condensed images of the last ``Condense`` or ``Solve``, which must be
        those of ``data``: the direction kernel forms the seeds, then the six launches of ``Adjoint`` solve for them
        - seven launches on torch's current stream, and the step is ``Adjoint(..., adj=True)``'s for those seeds,
        bit for bit.  ``sigma <= 0``: 1e-8.  Returns numpy arrays where ``z`` is one."""
        t = self._torch
        host = not _is_torch(z)
        unknown = set(ddata) - set(MPC_SEQ)
        assert not unknown, unknown
        d = self._data(data)
        dd = {k: self._to_dev(a) for k, a in ddata.items() if a is not None}
        zd, ld, vd = (self._to_dev(a) for a in (z, l, v))
        B = zd.shape[0]
        assert 1 <= B <= self.max_batch, (B, self.max_batch)
        img = self._img
        assert all(k in img for k in ("H", "f", "A", "b")), "Tangent before anything was condensed"
        assert img["f"].shape[0] == B and img["H"].shape[0] in (1, B), "the images are those of another batch"
        var_lens = (self.nz, self.nl, self.nv)
        xb = hip_api._fill_vars((zd, ld, vd), var_lens, B, [])
        dense = _DenseBatch()
        for k in ("H", "f", "A", "b"):
            a, i = img[k], DENSE_ARR.index(k)
            dense.base[i], dense.stride[i] = a.data_ptr(), (0 if (a.shape[0] == 1 and B > 1) else self._len[k])
        dirb = _MpcBatch()
        _fill_block(dirb, MPC_SEQ, self.seq_len, dd, B, [], optional=True)
        mk = lambda shape, dtype=t.float64: t.zeros(shape, dtype=dtype, device=self._dev)
        res = {k: mk((B, n)) for k, n in zip(("dz", "dl", "dv"), var_lens)}
        ob = hip_api._fill_vars((res["dz"], res["dl"], res["dv"]), var_lens, B, [])
        rb = None
        if rhs:
            for k, n in zip(("gz", "gl", "gv"), var_lens):
                res[k] = mk((B, n))
            rb = hip_api._fill_vars((res["gz"], res["gl"], res["gv"]), var_lens, B, [])
        work = t.empty((B, 5 * self.nzc + 3 * self.nv + sum(var_lens)), dtype=t.float64, device=self._dev)
        status = mk((B,), t.int32)
        blk = self._mpc_block(d, B)
        s = self._stream()
        _check(self._lib, self._lib.fbstab_hip_mpc_condensed_tangent_batch(
            self.dense._h, self.N, self.nx, self.nu, self.nc, B, C.byref(blk), C.byref(dense), C.byref(xb),
            C.byref(dirb), C.c_double(sigma), C.byref(ob), C.byref(rb) if rb is not None else None,
            C.c_void_p(work.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(s) if s else None))
        res["status"] = status
        if host:
            res = {k: a.cpu().numpy() for k, a in res.items()}
        return res

    def _multi_call(self, data, z, l, v, K, seeds, sigma, want, rhs_per_group):
        """fbstab_hip_mpc_condensed_kkt_solve_batch (``seeds``: (gz, gl, gv)) or
        fbstab_hip_mpc_condensed_x0_sensitivity_batch (None), on the images of the last ``Condense`` / ``Solve``."""
        t = self._torch
        host = not _is_torch(z)
        d = self._data(data)
        zd, ld, vd = (self._to_dev(a) for a in (z, l, v))
        B = zd.shape[0]
        assert 1 <= B <= self.max_batch, (B, self.max_batch)
        img = self._img
        assert all(k in img for k in ("H", "f", "A", "b")), "derivatives before anything was condensed"
        assert img["f"].shape[0] == B and img["H"].shape[0] in (1, B), "the images are those of another batch"
        var_lens = (self.nz, self.nl, self.nv)
        xb = hip_api._fill_vars((zd, ld, vd), var_lens, B, [])
        dense = _DenseBatch()
        for k in ("H", "f", "A", "b"):
            a, i = img[k], DENSE_ARR.index(k)
            dense.base[i], dense.stride[i] = a.data_ptr(), (0 if (a.shape[0] == 1 and B > 1) else self._len[k])
        sizes = condensed_multi_sizes(self.N, self.nx, self.nu, self.nc, K, rhs_per_group)
        mk = lambda shape, dtype=t.float64: t.zeros(shape, dtype=dtype, device=self._dev)
        res = {k: mk((B, K, n)) for k, n in zip(("dz", "dl", "dv"), var_lens) if k in want}
        ob = hip_api._fill_multi(tuple(res.get(k) for k in ("dz", "dl", "dv")), var_lens, B, K, [], optional=True,
                                 first_required=False) if res else None
        work = t.empty((B, sizes["work_doubles_per_qp"]), dtype=t.float64, device=self._dev)
        status = mk((B,), t.int32)
        blk = self._mpc_block(d, B)
        s = self._stream()
        head = (self.dense._h, self.N, self.nx, self.nu, self.nc, B, C.byref(blk), C.byref(dense), C.byref(xb))
        tail = (rhs_per_group, C.c_void_p(work.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(s) if s else None)
        if seeds is not None:
            sdev = tuple(None if a is None else self._to_dev(a) for a in seeds)
            sb = hip_api._fill_multi(sdev, var_lens, B, K, [], optional=True)
            rc = self._lib.fbstab_hip_mpc_condensed_kkt_solve_batch(*head, K, C.byref(sb), C.c_double(sigma),
                                                                    C.byref(ob), *tail)
        else:
            gain = mk((B, self.nx, self.nu)) if "gain" in want else None   # (nu x nx column-major per QP)
            rc = self._lib.fbstab_hip_mpc_condensed_x0_sensitivity_batch(
                *head, C.c_double(sigma), C.byref(ob) if ob is not None else None,
                C.c_void_p(gain.data_ptr()) if gain is not None else None, self.nu * self.nx, *tail)
            if gain is not None:
                res["gain"] = gain.transpose(1, 2)
        _check(self._lib, rc)
        res["status"] = status
        if host:
            res = {k: a.cpu().numpy() for k, a in res.items()}
        return res

    def KktSolve(self, data: Dict[str, object], z, l, v, gz, gl=None, gv=None, sigma: float = 0.0,
                 rhs_per_group: int = 0) -> Dict[str, object]:
        """Several right-hand sides on ONE factorisation of the condensed K per QP
        (fbstab_hip_mpc_condensed_kkt_solve_batch): the shapes and the returned dict of ``FBstabMpcBatch.KktSolve`` -
        ``gz`` of shape ``(batch, K, nz)``, or ``(K, nz)`` for one block of K seeds shared by the batch, ``gl``, ``gv``
        the same (None: zero); ``dz (batch, K, nz)``, ``dl``, ``dv`` and ``status`` - slot k what
        ``Adjoint(..., adj=True)`` of THIS class solves for seed k (the condensed chain with its O(sigma) bias).  It
        runs on the images of the last ``Condense`` / ``Solve``, as ``Adjoint`` does.  ``rhs_per_group``: right-hand
        sides per workgroup of the kernels around the dense step, 0 for the library's rule; it changes speed, never
        results.  Returns numpy arrays where ``z`` is one."""
        assert len(gz.shape) in (2, 3), gz.shape
        return self._multi_call(data, z, l, v, gz.shape[-2], (gz, gl, gv), sigma, ("dz", "dl", "dv"), rhs_per_group)

    def X0Sensitivity(self, data: Dict[str, object], z, l, v, sigma: float = 0.0,
                      want: Sequence[str] = ("dz", "gain"), rhs_per_group: int = 0) -> Dict[str, object]:
        """The solutions' sensitivity to the initial state on ONE factorisation of the condensed K per QP
        (fbstab_hip_mpc_condensed_x0_sensitivity_batch): those of ``want`` among ``dz (batch, nx, nz)``, ``dl``,
        ``dv`` - row j the tangent for dx0 = e_j - and ``gain (batch, nu, nx)`` = du0/dx0, the local feedback law,
        plus ``status``, as ``FBstabMpcBatch.X0Sensitivity`` returns them.  Slots not in ``want`` are neither
        allocated nor written; with ``gain`` alone the finish kernel is not launched.  It runs on the images of the
        last ``Condense`` / ``Solve``."""
        unknown = set(want) - {"dz", "dl", "dv", "gain"}
        assert not unknown, unknown
        assert want, "nothing is wanted"
        return self._multi_call(data, z, l, v, self.nx, None, sigma, tuple(want), rhs_per_group)

    def X0Map(self, data: Dict[str, object]) -> Dict[str, object]:
        """The affine dependence of the condensed vectors on x0 (fbstab_hip_mpc_condensed_x0_map_batch): ``M``, the
        images [F; G] as ``(batch, ne * nx)`` - ne = nz_c + nv rows, nx columns, column-major; ONE ``(1, ne * nx)``
        image where every matrix sequence of ``data`` is shared - and ``f0 = f_c(0)``, ``b0 = b_c(0)``, ``(batch, n)``:
        f_c(x) = f0 + F x, b_c(x) = b0 + G x for this ``data`` with any initial state x.  Torch tensors on the
        device; queued on torch's current stream.  The images of the last ``Condense`` are not touched."""
        return self._x0_map(self._data(data))

    def _x0_map(self, d):
        t = self._torch
        B = d["x0"].shape[0]
        assert 1 <= B <= self.max_batch, (B, self.max_batch)
        ne = self.nzc + self.nv
        shared = B > 1 and all(d[k].shape[0] == 1 for k in _MATRIX_SEQ)
        M = t.empty((1 if shared else B, ne * self.nx), dtype=t.float64, device=self._dev)
        f0 = t.empty((B, self.nzc), dtype=t.float64, device=self._dev)
        b0 = t.empty((B, self.nv), dtype=t.float64, device=self._dev)
        s = self._stream()
        sp = C.c_void_p(s) if s else None
        blk = self._mpc_block(d, B)
        _check(self._lib, self._lib.fbstab_hip_mpc_condensed_x0_map_batch(
            self.N, self.nx, self.nu, self.nc, B, C.byref(blk), C.c_void_p(M.data_ptr()),
            0 if shared else ne * self.nx, self.device, sp))
        # f_c(0), b_c(0): the vectors kernel with every QP's x0 slot on one block of zeros
        d0 = dict(d)
        d0["x0"] = t.zeros((1, self.nx), dtype=t.float64, device=self._dev)
        blk0 = self._mpc_block(d0, B)
        out = _DenseOutBatch()
        for k, a in (("f", f0), ("b", b0)):
            i = DENSE_ARR.index(k)
            out.base[i], out.stride[i] = a.data_ptr(), self._len[k]
        _check(self._lib, self._lib.fbstab_hip_mpc_condense_batch(
            self.N, self.nx, self.nu, self.nc, B, C.byref(blk0), VECTORS, C.byref(out), self.device, sp))
        return dict(M=M, f0=f0, b0=b0)

    # ---- per-step references ---------------------------------------------------------------------------------
    def _refs(self, ref, steps, B):
        """``ref``: name -> ``(steps, batch, len)`` or ``(steps, 1, len)`` (one row for the batch) for any of q, r, c,
        d; any view whose last dimension is contiguous is passed on by its own strides (a sliding window made by
        ``torch.as_strided`` costs no copy).  -> (the block, the device tensors by name)."""
        unknown = set(ref) - set(_REF_SEQ)
        assert not unknown, unknown
        blk, dev = _CondensedRefs(), {}
        for i, k in enumerate(_REF_SEQ):
            if ref.get(k) is None:
                continue
            a = self._to_dev(ref[k])
            n = self.seq_len[MPC_SEQ.index(k)]
            assert a.dtype == self._torch.float64, a.dtype
            assert a.dim() == 3 and a.shape[0] == steps and a.shape[1] in (1, B) and a.shape[2] == n, (
                k, tuple(a.shape), (steps, B, n))
            assert a.stride(2) == 1 or n <= 1, "the last dimension of a reference is contiguous"
            blk.base[i], blk.step[i] = a.data_ptr(), a.stride(0)
            blk.stride[i] = 0 if (a.shape[1] == 1 and B > 1) else a.stride(1)
            dev[k] = a
        return blk, dev

    @staticmethod
    def _data_at_step(d, rdev, k):
        """``d`` with step ``k`` of the references in the place of q, r, c, d (views: nothing is copied)."""
        dk = dict(d)
        for name, a in rdev.items():
            dk[name] = a[k]
        return dk

    def _reference_images(self, d, refs_blk, steps, B, refs_per_group=0):
        t = self._torch
        f0 = t.empty((steps, B, self.nzc), dtype=t.float64, device=self._dev)
        b0 = t.empty((steps, B, self.nv), dtype=t.float64, device=self._dev)
        im = _CondensedRefImages(f0.data_ptr(), b0.data_ptr(), B * self.nzc, B * self.nv, self.nzc, self.nv)
        blk = self._mpc_block(d, B)
        s = self._stream()
        _check(self._lib, self._lib.fbstab_hip_mpc_condensed_reference_images_batch(
            self.N, self.nx, self.nu, self.nc, B, steps, C.byref(blk), C.byref(refs_blk), C.byref(im), refs_per_group,
            self.device, C.c_void_p(s) if s else None))
        return f0, b0, im

    def ReferenceImages(self, data: Dict[str, object], ref: Dict[str, object], refs_per_group: int = 0):
        """The images of per-step references (fbstab_hip_mpc_condensed_reference_images_batch): with the matrix
        sequences of ``data`` and, at step k, the q, r, c, d of ``ref`` (name -> ``(steps, batch, len)`` or
        ``(steps, 1, len)``; names that are absent take ``data``'s sequence at every step), ``f0 (steps, batch, nzc)``
        and ``b0 (steps, batch, nv)`` such that step k's condensed vectors are f_c = f0[k] + F x, b_c = b0[k] + G x
        with the [F; G] of ``X0Map`` - bit for bit what ``Condense(data_k with x0 = 0, "vectors")`` gives, in ONE
        launch for all steps.  ``data["x0"]`` gives the batch size and is not read.  ``refs_per_group``: steps per
        workgroup, 0 for the library's rule; it changes speed, never results.  Torch tensors on the device, queued on
        torch's current stream; numpy arrays where every array of ``ref`` is one."""
        assert ref, "no reference"
        host = not any(_is_torch(a) for a in ref.values())
        d = self._data(data)
        B = d["x0"].shape[0]
        assert 1 <= B <= self.max_batch, (B, self.max_batch)
        steps = next(a for a in ref.values() if a is not None).shape[0]
        blk, _ = self._refs(ref, steps, B)
        f0, b0, _ = self._reference_images(d, blk, steps, B, refs_per_group)
        return dict(f0=f0.cpu().numpy(), b0=b0.cpu().numpy()) if host else dict(f0=f0, b0=b0)

    def RecedingSweep(self, data: Dict[str, object], z, l, v, y, A, B, steps: int, retire: bool = True, w=None,
                      shift: bool = False, mode: str = "affine", log: Sequence[str] = (), traj_per_group: int = 0,
                      ref: Optional[Dict[str, object]] = None):
        """``steps`` warm-started closed-loop steps on this route without a host round trip
        (fbstab_hip_mpc_condensed_receding_sweep): ``data`` is condensed ("all"), in ``mode="affine"`` the map of
        ``X0Map`` is built, and every step is the dense solve plus one small kernel that logs, advances the plant
        x+ = A x + B u0 (+ w_k), retires and shifts as ``FBstabMpcBatch.RecedingSweep`` does, and forms the next
        f_c = f0 + F x+, b_c = b0 + G x+ (``mode="recondense"``: the vectors kernel runs behind it instead, and the
        sweep is bitwise a loop over ``Solve(recondense="vectors")``).  ``A``/``B``: the simulation model, row-major
        ``(nx, nx)``/``(nx, nu)`` shared by all trajectories or ``(batch, nx, nx)``/``(batch, nx, nu)``.  ``w``:
        ``(steps, batch, nx)`` or None.  ``data["x0"]`` ``(batch, nx)`` is advanced in place to the state behind the
        last step, and ``(z, l, v, y)`` hold the expanded point of the LAST step.  Returns ``dict(out, u, eflag,
        newton)`` - the dense records of the last step, ``u (steps, batch, nu)``, and the int32 ``(steps, batch)`` exit
        flags (-1 once a trajectory is retired) and Newton counts - plus those of ``log`` among ``"x"`` (the states
        the steps were solved for), ``"U"``, ``"v"`` (the returned condensed points).  Everything is queued on
        torch's current stream and nothing waits for the device: torch tensors come back as they are queued; numpy
        arguments are uploaded, and numpy arrays come back.  ``traj_per_group``: trajectories per workgroup of the
        step kernel, 0 for the library's rule; it changes speed, never results.
        The images of the LAST step's QP stay in this object: ``Adjoint`` / ``X0Sensitivity`` at the returned point
        work when ``data["x0"]`` is set to the last row of the ``"x"`` log, the state that step was solved for.
        ``ref``: per-step references (fbstab_hip_mpc_condensed_tracking_sweep) - a dict with any of ``q, r, c, d``,
        each ``(steps, batch, len)`` or ``(steps, 1, len)``, passed on by its own strides where the last dimension is
        contiguous: step k solves the QP with those sequences, ``data`` is condensed with step 0's in place, in
        ``mode="affine"`` the images of ``ReferenceImages`` are built, and the returned point is expanded with the
        LAST step's sequences (with ``ref`` and that ``data["x0"]``, use those for ``Adjoint``)."""
        assert mode in _SWEEP_MODE, mode
        unknown = set(log) - {"x", "U", "v"}
        assert not unknown, unknown
        t = self._torch
        host = not _is_torch(z)
        d = self._data(data)
        zd, ld, vd, yd = (self._to_dev(a) for a in (z, l, v, y))
        Bn = zd.shape[0]
        assert d["x0"].shape == (Bn, self.nx) and d["x0"].is_contiguous(), "every trajectory has its own x0"
        for a, n in ((zd, self.nz), (ld, self.nl), (vd, self.nv), (yd, self.nv)):
            assert a.shape == (Bn, n) and a.stride(1) == 1, (a.shape, n)
        rblk, rimg = None, None
        if ref is not None and steps > 0:
            rblk, rdev = self._refs(ref, steps, Bn)
            self._condense(self._data_at_step(d, rdev, 0), "all")
        else:
            self._condense(d, "all")
        img = self._img
        cm = None
        if mode == "affine":
            m = self._x0_map(d)
            st = lambda a, n: 0 if (a.shape[0] == 1 and Bn > 1) else n
            cm = _CondensedMap(m["M"].data_ptr(), m["f0"].data_ptr(), m["b0"].data_ptr(),
                               st(m["M"], m["M"].shape[1]), self.nzc, self.nv)
            if rblk is not None:
                keep_f0, keep_b0, rimg = self._reference_images(d, rblk, steps, Bn)
        dense = _DenseBatch()
        for k in ("H", "f", "A", "b"):
            a, i = img[k], DENSE_ARR.index(k)
            dense.base[i], dense.stride[i] = a.data_ptr(), (0 if (a.shape[0] == 1 and Bn > 1) else self._len[k])
        cimg = lambda a: a.detach().to(self._dev, t.float64).transpose(-1, -2).contiguous()
        Ad, Bd = (cimg(a if _is_torch(a) else t.from_numpy(np.ascontiguousarray(a, dtype=np.float64))) for a in (A, B))
        for a, shape in ((Ad, (self.nx, self.nx)), (Bd, (self.nu, self.nx))):
            assert tuple(a.shape) in (shape, (Bn,) + shape), (tuple(a.shape), shape)
        plant = _Plant(Ad.data_ptr(), Bd.data_ptr(), self.nx * self.nx if Ad.dim() == 3 else 0,
                       self.nx * self.nu if Bd.dim() == 3 else 0)
        wd = None
        if w is not None:
            wd = (w.detach() if _is_torch(w) else t.from_numpy(np.ascontiguousarray(w, dtype=np.float64))).to(
                self._dev, t.float64).contiguous()
            assert tuple(wd.shape) == (steps, Bn, self.nx), "w: (steps, batch, nx)"
        sc = _SweepScenario(wd.data_ptr() if wd is not None else None, 1 if shift else 0)
        mk = lambda shape, dtype=t.float64: t.zeros(shape, dtype=dtype, device=self._dev)
        res = dict(u=mk((steps, Bn, self.nu)), eflag=mk((steps, Bn), t.int32), newton=mk((steps, Bn), t.int32))
        for k, n in (("x", self.nx), ("U", self.nzc), ("v", self.nv)):
            if k in log:
                res[k] = mk((steps, Bn, n))
        ptr = lambda k: res[k].data_ptr() if (k in res and steps > 0) else None
        lg = _CondensedSweepLog(ptr("u"), ptr("x"), ptr("U"), ptr("v"), ptr("eflag"), ptr("newton"))
        sizes = condensed_sweep_sizes(self.N, self.nx, self.nu, self.nc, traj_per_group,
                                      cm is not None and (Bn == 1 or cm.stride_M == 0))
        work = t.empty((Bn, sizes["work_doubles_per_traj"]), dtype=t.float64, device=self._dev)
        out = t.zeros((Bn, 40), dtype=t.uint8, device=self._dev)
        xb = hip_api._fill_vars((zd, ld, vd, yd), (self.nz, self.nl, self.nv, self.nv), Bn, [])
        blk = self._mpc_block(d, Bn)
        s = self._stream()
        self.generation += 1
        head = (self.dense._h, self.N, self.nx, self.nu, self.nc, Bn, C.byref(blk), C.byref(dense),
                C.byref(cm) if cm is not None else None, C.byref(xb), C.c_void_p(out.data_ptr()), C.byref(plant), steps,
                1 if retire else 0, C.byref(sc), _SWEEP_MODE[mode], C.byref(lg))
        tail = (traj_per_group, C.c_void_p(work.data_ptr()), C.c_void_p(s) if s else None)
        if rblk is None:
            rc = self._lib.fbstab_hip_mpc_condensed_receding_sweep(*head, *tail)
        else:
            rc = self._lib.fbstab_hip_mpc_condensed_tracking_sweep(
                *head, C.byref(rblk), C.byref(rimg) if rimg is not None else None, *tail)
        _check(self._lib, rc)
        res["out"] = out
        if not host:
            return res
        for dst, src in ((z, zd), (l, ld), (v, vd), (y, yd)):
            dst[...] = src.cpu().numpy()
        if not _is_torch(data["x0"]):
            data["x0"][...] = d["x0"].cpu().numpy()
        res = {k: a.cpu().numpy() for k, a in res.items() if k != "out"}
        res["out"] = hip_api.out_to_numpy(out)
        return res

    def RecedingSweepAdjoint(self, data: Dict[str, object], A, B, steps: int, log: Dict[str, object], gu=None,
                             gx=None, retire: bool = True, sigma: float = 0.0, want: Sequence[str] = (),
                             mu: bool = False, mode: str = "affine", traj_per_group: int = 0,
                             gf0: bool = False, gb0: bool = False,
                             ref: Optional[Dict[str, object]] = None) -> Dict[str, object]:
        """Reverse mode through ``RecedingSweep`` in one call (fbstab_hip_mpc_condensed_receding_sweep_adjoint): the
        seeds ``gu (steps, batch, nu)`` = dL/du_k and ``gx (steps, batch, nx)`` = dL/dx_(k+1) (None: zero) are taken
        backwards along every trajectory of the sweep that ``log`` records - what ``RecedingSweep(..., log=("x", "U",
        "v"))`` returned: its ``x``, ``U``, ``v`` and ``eflag`` are read.  ``data``: the sweep's data (its ``x0`` is
        not read, only its batch size); ``A``/``B``: the plant as there.  This call condenses ``data`` ("all") and, in
        ``mode="affine"``, builds the map of ``X0Map`` itself: the images this object held before are replaced, and
        the vectors ``f``, ``b`` are scratch of the call.  Returns a dict: ``x0 (batch, nx)`` = dL/dx_0, dL/d(sequence)
        summed over the contributing steps for every name of ``want`` (``(batch, len)``; a shared ``(1, len)`` sequence
        gets per-trajectory gradients like every other), ``status`` (``(batch,)`` int32: the steps whose
        factorisation failed) and, on request, ``mu (steps, batch, nx)`` (the costates: dL/dw_k where the step is not
        retired), ``gf0 (batch, nzc)`` and ``gb0 (batch, nv)`` (the gradients of the map's f0 and b0).
        ``mode="recondense"``: every step's f_c, b_c come from the vectors kernel, as in the forward sweep of that
        mode.  ``retire``: the forward's.  ``traj_per_group``: as in ``RecedingSweep``; it changes speed, never
        results.  Everything is queued on torch's current stream; numpy inputs are uploaded and numpy arrays come
        back (decided by ``log["U"]``).
        ``ref``: the forward's per-step references (fbstab_hip_mpc_condensed_tracking_sweep_adjoint).  A name of
        ``want`` that is in ``ref`` comes back as the per-step array ``(steps, batch, len)`` - dL/d(sequence of step
        k), zeros for a step that does not contribute; a ``(steps, 1, len)`` reference gets per-trajectory rows like
        every shared sequence - and ``gf0`` / ``gb0`` are not available."""
        assert mode in _SWEEP_MODE, mode
        want = tuple(want)
        assert not set(want) - set(MPC_SEQ), set(want) - set(MPC_SEQ)
        t = self._torch
        host = not _is_torch(log["U"])
        d = self._data(data)
        Bn = d["x0"].shape[0]
        assert 1 <= Bn <= self.max_batch, (Bn, self.max_batch)
        f64 = lambda a: (a.detach() if _is_torch(a) else t.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(
            self._dev, t.float64).contiguous()
        xl, Ul, vl = (f64(log[k]) for k in ("x", "U", "v"))
        el = log["eflag"]
        el = (el.detach() if _is_torch(el) else t.from_numpy(np.ascontiguousarray(el))).to(self._dev, t.int32).contiguous()
        for a, n in ((xl, self.nx), (Ul, self.nzc), (vl, self.nv)):
            assert tuple(a.shape) == (steps, Bn, n), (tuple(a.shape), (steps, Bn, n))
        assert tuple(el.shape) == (steps, Bn), tuple(el.shape)
        gud = None if gu is None else f64(gu)
        gxd = None if gx is None else f64(gx)
        assert gud is None or tuple(gud.shape) == (steps, Bn, self.nu), "gu: (steps, batch, nu)"
        assert gxd is None or tuple(gxd.shape) == (steps, Bn, self.nx), "gx: (steps, batch, nx)"
        rblk, rimg, rdev = None, None, {}
        if ref is not None and steps > 0:
            assert not gf0 and not gb0, "gf0 / gb0 are not available with per-step references"
            rblk, rdev = self._refs(ref, steps, Bn)
        self._condense(d, "all")   # (H_c and A_c do not depend on q, r, c, d; f and b are scratch of the call)
        img = self._img
        cm = None
        if mode == "affine":
            m = self._x0_map(d)
            st = lambda a, n: 0 if (a.shape[0] == 1 and Bn > 1) else n
            cm = _CondensedMap(m["M"].data_ptr(), m["f0"].data_ptr(), m["b0"].data_ptr(),
                               st(m["M"], m["M"].shape[1]), self.nzc, self.nv)
            if rblk is not None:
                keep_f0, keep_b0, rimg = self._reference_images(d, rblk, steps, Bn)
        dense = _DenseBatch()
        for k in ("H", "f", "A", "b"):
            a, i = img[k], DENSE_ARR.index(k)
            dense.base[i], dense.stride[i] = a.data_ptr(), (0 if (a.shape[0] == 1 and Bn > 1) else self._len[k])
        cimg = lambda a: f64(a).transpose(-1, -2).contiguous()
        Ad, Bd = cimg(A), cimg(B)
        for a, shape in ((Ad, (self.nx, self.nx)), (Bd, (self.nu, self.nx))):
            assert tuple(a.shape) in (shape, (Bn,) + shape), (tuple(a.shape), shape)
        plant = _Plant(Ad.data_ptr(), Bd.data_ptr(), self.nx * self.nx if Ad.dim() == 3 else 0,
                       self.nx * self.nu if Bd.dim() == 3 else 0)
        mk = lambda shape, dtype=t.float64: t.zeros(shape, dtype=dtype, device=self._dev)
        names = tuple(k for k in MPC_SEQ if k in want or k == "x0")
        res = {k: mk((Bn, n)) for k, n in zip(MPC_SEQ, self.seq_len) if k in names and k not in rdev}
        grad = _MpcGradBatch()
        _fill_block(grad, MPC_SEQ, self.seq_len, res, Bn, [], optional=True, shared=False)
        rgrad = _CondensedRefGrad()
        for i, k in enumerate(_REF_SEQ):   # (the call writes every entry of a per-step gradient)
            if k in names and k in rdev:
                n = self.seq_len[MPC_SEQ.index(k)]
                res[k] = t.empty((steps, Bn, n), dtype=t.float64, device=self._dev)
                rgrad.base[i], rgrad.step[i], rgrad.stride[i] = res[k].data_ptr(), Bn * n, n
        if mu:
            res["mu"] = mk((steps, Bn, self.nx))
        if gf0:
            res["gf0"] = mk((Bn, self.nzc))
        if gb0:
            res["gb0"] = mk((Bn, self.nv))
        status = mk((Bn,), t.int32)
        sizes = condensed_sweep_adjoint_sizes(self.N, self.nx, self.nu, self.nc, traj_per_group,
                                              cm is not None and (Bn == 1 or cm.stride_M == 0))
        finish = mode != "affine" or any(k != "x0" for k in names)
        work = t.empty((Bn, sizes["work_doubles_per_traj_grad" if finish else "work_doubles_per_traj"]),
                       dtype=t.float64, device=self._dev)
        ptr = lambda a: C.c_void_p(a.data_ptr()) if (a is not None and a.numel() > 0) else None
        lg = _CondensedSweepLog(None, xl.data_ptr() or None, Ul.data_ptr() or None, vl.data_ptr() or None,
                                el.data_ptr() or None, None)
        if steps == 0:  # (empty logs have no address; the call reads none of them)
            lg = _CondensedSweepLog(None, work.data_ptr(), work.data_ptr(), work.data_ptr(), work.data_ptr(), None)
        blk = self._mpc_block(d, Bn)
        s = self._stream()
        self.generation += 1
        head = (self.dense._h, self.N, self.nx, self.nu, self.nc, Bn, C.byref(blk), C.byref(dense),
                C.byref(cm) if cm is not None else None, C.byref(plant), steps, 1 if retire else 0, C.byref(lg),
                ptr(gud), ptr(gxd), C.c_double(sigma), C.byref(grad))
        tail = (traj_per_group, C.c_void_p(work.data_ptr()), C.c_void_p(s) if s else None)
        if rblk is None:
            rc = self._lib.fbstab_hip_mpc_condensed_receding_sweep_adjoint(
                *head, ptr(res.get("gf0")), ptr(res.get("gb0")), ptr(res.get("mu")), C.c_void_p(status.data_ptr()),
                _SWEEP_MODE[mode], *tail)
        else:
            rc = self._lib.fbstab_hip_mpc_condensed_tracking_sweep_adjoint(
                *head, ptr(res.get("mu")), C.c_void_p(status.data_ptr()), _SWEEP_MODE[mode], C.byref(rblk),
                C.byref(rimg) if rimg is not None else None, C.byref(rgrad), *tail)
        _check(self._lib, rc)
        res["status"] = status
        if host:
            res = {k: a.cpu().numpy() for k, a in res.items()}
        return res

    def _direction_images(self, d, ddata, dref, rdev, steps, Bn):
        """The directions of f0_k, b0_k from those of q, r, c, d: the images are linear in the four sequences, so
        ``ReferenceImages``' kernel on the direction sequences gives them - every slot given, zeros where nothing
        moves.  -> (df0, db0, step count of the images: 1 where no per-step reference moves), or None."""
        t = self._torch
        ddata, dref = dict(ddata or {}), dict(dref or {})
        for name, src in (("ddata", ddata), ("dref", dref)):
            for k in src:
                if k in _MATRIX_SEQ:
                    raise NotImplementedError(
                        "RecedingSweepTangent: a direction on the matrix sequence %r (%s) - forward mode through the "
                        "sweep serves x0, w, q, r, c, d and the per-step references; H_c, A_c and the map M are held "
                        "fixed" % (k, name))
            unknown = set(src) - set(_REF_SEQ)
            assert not unknown, (name, unknown, "the direction of x0 is dx0")
        ddata = {k: a for k, a in ddata.items() if a is not None}
        dref = {k: a for k, a in dref.items() if a is not None}
        if not ddata and not dref:
            return None
        nsteps = steps if dref else 1
        blk, keep = _CondensedRefs(), []
        for i, k in enumerate(_REF_SEQ):
            n = self.seq_len[MPC_SEQ.index(k)]
            if k in dref:
                assert k in rdev, "dref[%r]: %r is not a per-step reference of this sweep (ref)" % (k, k)
                assert k not in ddata, "ddata[%r]: the sweep reads ref[%r], not data's sequence" % (k, k)
                a = self._to_dev(dref[k].detach() if _is_torch(dref[k]) else dref[k]).to(t.float64).contiguous()
                assert a.dim() == 3 and a.shape[0] == steps and a.shape[1] in (1, Bn) and a.shape[2] == n, (
                    k, tuple(a.shape), (steps, Bn, n))
                blk.base[i], blk.step[i] = a.data_ptr(), a.stride(0)
                blk.stride[i] = 0 if (a.shape[1] == 1 and Bn > 1) else n
            elif k in ddata:
                assert k not in rdev, "ddata[%r]: the sweep reads ref[%r], not data's sequence" % (k, k)
                a = self._to_dev(ddata[k].detach() if _is_torch(ddata[k]) else ddata[k]).to(t.float64).contiguous()
                a = a.reshape(1, n) if a.dim() == 1 else a
                assert a.dim() == 2 and a.shape[0] in (1, Bn) and a.shape[1] == n, (k, tuple(a.shape), (Bn, n))
                blk.base[i], blk.step[i] = a.data_ptr(), 0
                blk.stride[i] = 0 if (a.shape[0] == 1 and Bn > 1) else n
            else:
                a = t.zeros((1, n), dtype=t.float64, device=self._dev)
                blk.base[i], blk.step[i], blk.stride[i] = a.data_ptr(), 0, 0
            keep.append(a)
        df0, db0, _ = self._reference_images(d, blk, nsteps, Bn)
        return df0, db0, nsteps

    def RecedingSweepTangent(self, data: Dict[str, object], A, B, steps: int, log: Dict[str, object], dx0=None,
                             dw=None, ddata: Optional[Dict[str, object]] = None,
                             dref: Optional[Dict[str, object]] = None, ref: Optional[Dict[str, object]] = None,
                             sigma: float = 0.0, traj_per_group: int = 0) -> Dict[str, object]:
        """Forward mode through ``RecedingSweep`` in one call (fbstab_hip_mpc_condensed_receding_sweep_tangent): how
        the closed-loop u_k and x_(k+1) of the sweep that ``log`` records - what ``RecedingSweep(..., log=("x", "U",
        "v"))`` returned: its ``x``, ``U``, ``v`` and ``eflag`` are read - move along ONE direction:
        ``dx0`` ``(batch, nx)`` (``(nx,)`` or ``(1, nx)``: shared), ``dw`` ``(steps, batch, nx)``, ``ddata`` - directions
        of ``data``'s ``q, r, c, d``, ``(batch, len)``, or ``(len,)`` / ``(1, len)`` for one shared by the batch - and
        ``dref`` - directions of the per-step references ``ref`` (the forward's), ``(steps, batch, len)`` or
        ``(steps, 1, len)``.  None is zero everywhere.  ``ddata`` and ``dref`` are mapped to the directions of the
        images f0_k, b0_k by ``ReferenceImages``' kernel on the direction sequences.  A direction on a matrix sequence
        raises ``NotImplementedError``.  Directions of the plant are the caller's: add dA x_k + dB u_k to ``dw[k]``
        where step k is not retired.  ``data``: the sweep's data (its ``x0`` is not read, only its batch size);
        ``A``/``B``: the plant as there.  This call condenses ``data`` ("all") and builds the map of ``X0Map`` itself
        (a sweep that ran in ``mode="recondense"`` is differentiated through it): the images this object held before
        are replaced, and the vectors ``f``, ``b`` are scratch of the call.  Returns ``dict(du (steps, batch, nu),
        dx (steps, batch, nx), status)`` - du_k, dx_(k+1), and per trajectory the steps whose factorisation failed;
        du and dx are zero at and behind a retirement, and du is zero at a step that did not end in SUCCESS.
        ``traj_per_group``: as in ``RecedingSweep``; it changes speed, never results.  Everything is queued on torch's
        current stream; numpy inputs are uploaded and numpy arrays come back (decided by ``log["U"]``)."""
        t = self._torch
        host = not _is_torch(log["U"])
        d = self._data(data)
        Bn = d["x0"].shape[0]
        assert 1 <= Bn <= self.max_batch, (Bn, self.max_batch)
        f64 = lambda a: (a.detach() if _is_torch(a) else t.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(
            self._dev, t.float64).contiguous()
        xl, Ul, vl = (f64(log[k]) for k in ("x", "U", "v"))
        el = log["eflag"]
        el = (el.detach() if _is_torch(el) else t.from_numpy(np.ascontiguousarray(el))).to(self._dev, t.int32).contiguous()
        for a, n in ((xl, self.nx), (Ul, self.nzc), (vl, self.nv)):
            assert tuple(a.shape) == (steps, Bn, n), (tuple(a.shape), (steps, Bn, n))
        assert tuple(el.shape) == (steps, Bn), tuple(el.shape)
        rblk, rimg, rdev = None, None, {}
        if ref is not None and steps > 0:
            rblk, rdev = self._refs(ref, steps, Bn)
        dimg = self._direction_images(d, ddata, dref, rdev, steps, Bn) if steps > 0 else None
        self._condense(d, "all")   # (H_c and A_c do not depend on q, r, c, d; f and b are scratch of the call)
        img = self._img
        m = self._x0_map(d)
        st = lambda a, n: 0 if (a.shape[0] == 1 and Bn > 1) else n
        cm = _CondensedMap(m["M"].data_ptr(), m["f0"].data_ptr(), m["b0"].data_ptr(), st(m["M"], m["M"].shape[1]),
                           self.nzc, self.nv)
        if rblk is not None:
            keep_f0, keep_b0, rimg = self._reference_images(d, rblk, steps, Bn)
        dense = _DenseBatch()
        for k in ("H", "f", "A", "b"):
            a, i = img[k], DENSE_ARR.index(k)
            dense.base[i], dense.stride[i] = a.data_ptr(), (0 if (a.shape[0] == 1 and Bn > 1) else self._len[k])
        cimg = lambda a: f64(a).transpose(-1, -2).contiguous()
        Ad, Bd = cimg(A), cimg(B)
        for a, shape in ((Ad, (self.nx, self.nx)), (Bd, (self.nu, self.nx))):
            assert tuple(a.shape) in (shape, (Bn,) + shape), (tuple(a.shape), shape)
        plant = _Plant(Ad.data_ptr(), Bd.data_ptr(), self.nx * self.nx if Ad.dim() == 3 else 0,
                       self.nx * self.nu if Bd.dim() == 3 else 0)
        dr = hip_api._CondensedSweepDir()
        if dx0 is not None:
            x0d = f64(dx0)
            x0d = x0d.reshape(1, self.nx) if x0d.dim() == 1 else x0d
            assert tuple(x0d.shape) in ((1, self.nx), (Bn, self.nx)), "dx0: (batch, nx), (1, nx) or (nx,)"
            dr.dx0, dr.stride_dx0 = x0d.data_ptr(), (0 if (x0d.shape[0] == 1 and Bn > 1) else self.nx)
        if dw is not None and steps > 0:
            dwd = f64(dw)
            assert tuple(dwd.shape) == (steps, Bn, self.nx), "dw: (steps, batch, nx)"
            dr.dw = dwd.data_ptr()
        if dimg is not None:
            df0, db0, nsteps = dimg
            dr.df0, dr.db0 = df0.data_ptr(), db0.data_ptr()
            dr.step_df0, dr.step_db0 = (Bn * self.nzc, Bn * self.nv) if nsteps > 1 else (0, 0)
            dr.stride_df0, dr.stride_db0 = self.nzc, self.nv
        mk = lambda shape, dtype=t.float64: t.zeros(shape, dtype=dtype, device=self._dev)
        res = dict(du=mk((steps, Bn, self.nu)), dx=mk((steps, Bn, self.nx)))
        status = mk((Bn,), t.int32)
        sizes = condensed_sweep_tangent_sizes(self.N, self.nx, self.nu, self.nc, traj_per_group,
                                              Bn == 1 or cm.stride_M == 0)
        work = t.empty((Bn, sizes["work_doubles_per_traj"]), dtype=t.float64, device=self._dev)
        lg = _CondensedSweepLog(None, xl.data_ptr() or None, Ul.data_ptr() or None, vl.data_ptr() or None,
                                el.data_ptr() or None, None)
        outs = (C.c_void_p(res["du"].data_ptr()), C.c_void_p(res["dx"].data_ptr()))
        if steps == 0:  # (empty arrays have no address; the call reads and writes none of them)
            lg = _CondensedSweepLog(None, work.data_ptr(), work.data_ptr(), work.data_ptr(), work.data_ptr(), None)
            outs = (C.c_void_p(work.data_ptr()), C.c_void_p(work.data_ptr()))
        s = self._stream()
        self.generation += 1
        _check(self._lib, self._lib.fbstab_hip_mpc_condensed_receding_sweep_tangent(
            self.dense._h, self.N, self.nx, self.nu, self.nc, Bn, C.byref(dense), C.byref(cm),
            C.byref(rimg) if rimg is not None else None, C.byref(plant), steps, C.byref(lg), C.byref(dr),
            C.c_double(sigma), outs[0], outs[1], C.c_void_p(status.data_ptr()), traj_per_group,
            C.c_void_p(work.data_ptr()), C.c_void_p(s) if s else None))
        res["status"] = status
        if host:
            res = {k: a.cpu().numpy() for k, a in res.items()}
        return res

    def Solve(self, data: Dict[str, object], z, l, v, y, out=None, recondense="all"):
        """The signature and in-place semantics of ``FBstabMpcBatch.Solve``: the guess is read from ``(z, l, v)`` -
        U is the u blocks of z, v is v; l does not enter - and ``(z, l, v, y)`` are overwritten with the point of
        the MPC QP.  ``recondense``: "all" condenses ``data`` first, "vectors" only f and b (only x0, q, r, c, d
        moved since the last call), "none" solves on the images as they stand.  Returns ``out``, the DENSE solver's
        records (a torch uint8 tensor ``(batch, 40)``; ``hip_api.out_to_numpy``; a numpy record array for numpy
        arguments): exit flags and residuals are those of the condensed QP, and the Newton and proximal counts are
        those of the condensed solve - not comparable with the counts of the MPC kernels."""
        assert recondense in ("all", "vectors", "none"), recondense
        t = self._torch
        host = not _is_torch(z)
        d = self._data(data)
        zd, ld, vd, yd = (self._to_dev(a) for a in (z, l, v, y))
        B = zd.shape[0]
        if recondense != "none":
            self._condense(d, recondense)
        img = self._img
        assert all(k in img for k in ("H", "f", "A", "b")), "Solve(recondense=...) before anything was condensed"
        assert img["f"].shape[0] == B and img["H"].shape[0] in (1, B), "the images are those of another batch"
        U = zd.view(B, self.N + 1, self.nx + self.nu)[:, :, self.nx:].reshape(B, self.nzc).contiguous()
        l0 = t.empty((B, 0), dtype=t.float64, device=self._dev)
        vc = vd.clone() if host or vd.stride(1) != 1 else vd
        yc = t.empty((B, self.nv), dtype=t.float64, device=self._dev)
        dout = None if (out is None or host) else out
        dout = self.dense.Solve(dict(H=img["H"], f=img["f"], A=img["A"], b=img["b"]), U, l0, vc, yc, out=dout,
                                async_=True)
        self._expand(d, U, vc, yc, zd, ld, vd, yd)
        if not host:
            return dout
        for dst, src in ((z, zd), (l, ld), (v, vd), (y, yd)):
            dst[...] = src.cpu().numpy()
        rec = hip_api.out_to_numpy(dout)
        if out is not None:
            out[...] = rec
            return out
        return rec
