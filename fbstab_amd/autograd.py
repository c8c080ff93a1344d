"""torch.autograd for batched solves: the solution maps (data -> z, l, v) of FBstabMpcBatch and
FBstabDenseBatch as differentiable functions.

    solver = FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    z, l, v, out = solve_mpc(solver, data)        # data: dict of the 12 sequences, (B, len) float64 on cuda
    loss(z, l, v).backward()                      # data[k].grad for every k with requires_grad

Forward: ``solver.Solve`` on torch's current stream from a zero initial guess.  Backward: ONE launch of
fbstab_hip_mpc_adjoint_batch at the returned points, which computes only the gradients torch asks for
(``needs_input_grad``).  The gradient is that of the solution map with the Newton matrix regularised by
``sigma`` (<= 0: 1e-8; include/fbstab_hip.h).  A QP whose solve did not end in SUCCESS (``out``'s eflag != 0),
or whose adjoint factorisation failed, gets ZERO gradients: its returned point is not a solution, and no
derivative of the solution map is defined there.  ``out`` (the SolverOut records, (B, 40) uint8) is not
differentiable.

The dense QP min 1/2 z'Hz + f'z s.t. Gz = h, Az <= b (the OptNet-style layer) works the same way:

    solver = FBstabDenseBatch(nz, nl, nv, max_batch=B)
    z, l, v, out = solve_dense(solver, data)      # data: dict of H, f, G, h, A, b, (B, len) float64 on cuda

with fbstab_hip_dense_adjoint_batch behind ``backward``.  The matrices are column-major images like the
solver's inputs, and so are their gradients; with ``nl == 0``, ``G`` and ``h`` are ``(B, 0)`` tensors.

Parameters shared by the batch (the matrices of an OptNet-style layer or of a differentiable MPC): an input of
shape ``(len,)`` or ``(1, len)`` beside inputs of batch B > 1 is ONE array for all QPs.  The forward passes it to
the solver with batch stride 0 (no B copies are made), and the backward asks fbstab_hip_*_adjoint_batch_reduced
for its gradient: the sum over the batch, computed on the device from the points and the adjoint steps without
the B per-QP images, in the input's own shape.  QPs that did not end in SUCCESS, or whose adjoint factorisation
failed, are left out of the sum.  The sum is formed in a fixed order: the same inputs give the same bits.
Per-QP inputs in the same call keep their per-QP gradients as above.

Forward mode (``torch.autograd.forward_ad``): inside a ``dual_level``, inputs made dual with ``make_dual`` give
``z, l, v`` their tangents J dtheta through ONE call of fbstab_hip_*_tangent_batch at the returned points, with
the tangents that are present (a shared input's tangent travels with batch stride 0 like the input).  As in the
backward, a QP whose solve did not end in SUCCESS, or whose factorisation failed, gets ZERO tangents.
(``torch.func.jvp`` is not served: it needs a ``setup_context`` style function.)

The closed loop (the receding-horizon sweep, x_(k+1) = A x_k + B u0(x_k; theta)) is differentiable as a whole:

    u, x, out = closed_loop_mpc(solver, data, A, B, steps)   # u (steps, B, nu); x (steps, B, nx): x_1 .. x_steps
    loss(u, x).backward()                                    # data[k].grad, A.grad, B.grad

Forward: ONE logged sweep (fbstab_hip_mpc_receding_sweep_logged) on a clone of ``data["x0"]`` from a zero guess.
Backward: ONE call of fbstab_hip_mpc_receding_sweep_adjoint, which takes the costate backwards through the logged
steps and computes only the gradients torch asks for; ``data["x0"].grad`` is dL/dx_0 of every trajectory, and the
plant's ``A.grad``, ``B.grad`` (``(nx, nx)`` / ``(nx, nu)`` torch tensors, row-major, shared by the trajectories)
are formed from the logged costates.  A step whose solve did not end in SUCCESS passes the costate through the
plant alone, and a retired trajectory (``retire=True``) is cut at its retirement step, as the sweep cuts it.  A
shared input gets the sum of the per-trajectory gradients, formed in torch.

Scenarios: ``closed_loop_mpc(..., w=w)`` runs the disturbed plant x_(k+1) = A x_k + B u0 + w_k (``w``: ``(steps, B,
nx)``, one realisation per trajectory - Monte-Carlo over disturbances in one launch), and ``shift=True`` moves every
returned point one stage towards the present before it is the next guess (fbstab_hip_mpc_receding_sweep_scenario;
fewer Newton steps on time-invariant horizons, more on random time-varying ones).  The backward is the same call:
the recursion does not change, and ``w.grad`` is the logged costate, dL/dw_k = mu_k, zero at and after a
trajectory's retirement step.  Not served: the batch-summed
(reduced) path inside the library, forward mode through the sweep (the condensed route below serves it), and losses
of anything but ``u`` and ``x`` (the rest of z_k, l_k, v_k).

Jacobians of the solution map with respect to the initial state, as matrices:

    J = mpc_x0_sensitivity(solver, data, z, l, v)   # J["gain"] (B, nu, nx) = du0/dx0, J["dz"] (B, nx, nz), ...

ONE call of fbstab_hip_mpc_x0_sensitivity_batch, one factorisation per QP for all nx columns.  The result is
DETACHED: plain tensors that carry no graph.  The dense QP's counterpart, for the arrays that enter it as vectors:

    J = dense_jacobian(solver, data, z, l, v, wrt="b")   # J["dz"] (B, nv, nz): row k = dz/db_k, J["dl"], J["dv"]

ONE call of fbstab_hip_dense_jacobian_batch (``wrt``: "f", "h" or "b"), DETACHED like the other.

The condensed route (``fbstab_amd.condense.CondensedMpc``, for state-heavy shapes) is differentiable too:

    cm = CondensedMpc(N, nx, nu, nc, max_batch=B)
    z, l, v, out = solve_condensed_mpc(cm, data)  # data as for solve_mpc; out: the DENSE solver's records

Forward: ``cm.Solve`` from a zero guess, condensing ``data`` first.  Backward: ONE call of ``cm.Adjoint``
(fbstab_hip_mpc_condensed_adjoint_batch: the seeds condensed, the dense adjoint, the step expanded and contracted)
with the gradients torch asks for; QPs whose condensed solve did not end in SUCCESS, or whose factorisation failed,
get zero gradients.  A shared ``(len,)`` or ``(1, len)`` input gets the torch sum over the batch of the per-QP
gradients: the device-side reduced form is not served on this route.  Forward mode (``torch.autograd.forward_ad``):
ONE call of ``cm.Tangent`` (fbstab_hip_mpc_condensed_tangent_batch) with the tangents that are present, zero
tangents for the same QPs.  Either pass re-condenses first where another ``Condense`` or ``Solve`` of ``cm`` has
replaced the forward's images since.
"""
import torch

from .hip_api import DENSE_ARR, MPC_SEQ

_REF_SEQ = ("q", "r", "c", "d")   # (condense.py: the sequences a closed loop may track step by step)

__all__ = ["MpcSolveFunction", "solve_mpc", "DenseSolveFunction", "solve_dense", "ClosedLoopMpcFunction",
           "closed_loop_mpc", "mpc_x0_sensitivity", "dense_jacobian", "CondensedMpcSolveFunction",
           "solve_condensed_mpc"]


def _forward(names, ctx, solver, sigma, arrs):
    B = max(a.shape[0] if a.dim() == 2 else 1 for a in arrs)
    # shared parameters: (len,) or (1, len) beside a batch of more than one QP; they travel as (1, len)
    ctx.shared = tuple(k for k, a in zip(names, arrs) if B > 1 and (a.dim() == 1 or a.shape[0] == 1))
    ctx.shapes = {k: a.shape for k, a in zip(names, arrs)}
    data = {k: (a.detach().reshape(1, a.numel()) if k in ctx.shared else a.detach()).contiguous()
            for k, a in zip(names, arrs)}
    dev = data[names[0]].device  # (Q and H are never empty)
    z = torch.zeros((B, solver.nz), dtype=torch.float64, device=dev)
    l = torch.zeros((B, solver.nl), dtype=torch.float64, device=dev)
    v = torch.zeros((B, solver.nv), dtype=torch.float64, device=dev)
    y = torch.zeros((B, solver.nv), dtype=torch.float64, device=dev)
    out = solver.Solve(data, z, l, v, y)
    ctx.solver, ctx.sigma = solver, sigma
    ctx.save_for_backward(*[data[k] for k in names], z, l, v, out)
    ctx.save_for_forward(*[data[k] for k in names], z, l, v, out)
    # absent tangents reach `_jvp` as None instead of zeros (one Tangent call with the tangents that are present);
    # `_backward` then makes its own zeros for seeds torch leaves out, which is what it was handed before
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(out)
    return z, l, v, out


def _backward(names, ctx, gz, gl, gv, gout):
    need = ctx.needs_input_grad[2:]
    want = [k for k, n in zip(names, need) if n]
    if not want:
        return (None, None) + (None,) * len(names)
    saved = ctx.saved_tensors
    data = dict(zip(names, saved[:len(names)]))
    z, l, v, out = saved[len(names):]
    gz, gl, gv = (torch.zeros_like(x) if g is None else g for g, x in zip((gz, gl, gv), (z, l, v)))
    reduce = [k for k in want if k in ctx.shared]
    if reduce:
        g = ctx.solver.Adjoint(data, z, l, v, gz.contiguous(), gl.contiguous(), gv.contiguous(), sigma=ctx.sigma,
                               want=want, reduce=reduce, out=out)
    else:
        g = ctx.solver.Adjoint(data, z, l, v, gz.contiguous(), gl.contiguous(), gv.contiguous(), sigma=ctx.sigma,
                               want=want)
    eflag = out[:, 0:4].contiguous().view(torch.int32)[:, 0]  # SolverOut::eflag, on the device
    keep = ((eflag == 0) & (g["status"] == 0))[:, None]
    grads = []
    for k in names:
        if k not in want:
            grads.append(None)
        elif k in reduce:  # (the library has left the same QPs out of the sum)
            grads.append(g[k].reshape(ctx.shapes[k]))
        else:
            grads.append(torch.where(keep, g[k], torch.zeros_like(g[k])))
    return (None, None) + tuple(grads)


def _jvp(names, ctx, tangents):
    saved = ctx.saved_tensors
    data = dict(zip(names, saved[:len(names)]))
    z, l, v, out = saved[len(names):]
    ddata = {}
    for k, t in zip(names, tangents):
        if t is None or t.numel() == 0:
            continue
        t = t.detach()
        ddata[k] = (t.reshape(1, t.numel()) if k in ctx.shared else t).contiguous()
    res = ctx.solver.Tangent(data, z, l, v, ddata, sigma=ctx.sigma)
    eflag = out[:, 0:4].contiguous().view(torch.int32)[:, 0]  # SolverOut::eflag, on the device
    keep = ((eflag == 0) & (res["status"] == 0))[:, None]
    return tuple(torch.where(keep, res[k], torch.zeros_like(res[k])) for k in ("dz", "dl", "dv")) + (None,)


class MpcSolveFunction(torch.autograd.Function):
    """apply(solver, sigma, *sequences in MPC_SEQ order) -> (z, l, v, out)."""

    @staticmethod
    def forward(ctx, solver, sigma, *seqs):
        return _forward(MPC_SEQ, ctx, solver, sigma, seqs)

    @staticmethod
    def backward(ctx, gz, gl, gv, gout):
        return _backward(MPC_SEQ, ctx, gz, gl, gv, gout)

    @staticmethod
    def jvp(ctx, solver_t, sigma_t, *tangents):
        return _jvp(MPC_SEQ, ctx, tangents)


def solve_mpc(solver, data, sigma: float = 0.0):
    """Differentiable batched solve: ``data`` maps the 12 names of MPC_SEQ to ``(B, len)`` float64 CUDA tensors
    (any of them may require grad; ``(len,)`` or ``(1, len)``: a parameter shared by the batch).  Returns
    ``(z, l, v, out)``; see the module docstring."""
    return MpcSolveFunction.apply(solver, sigma, *[data[k] for k in MPC_SEQ])


def mpc_x0_sensitivity(solver, data, z, l, v, sigma: float = 0.0):
    """The local feedback law and the plan's sensitivity to the initial state at the returned points ``(z, l, v)``
    (``FBstabMpcBatch.X0Sensitivity``: one factorisation per QP, nx right-hand sides): a dict of torch tensors on the
    inputs' device, ``gain (B, nu, nx)`` = du0/dx0, ``dz (B, nx, nz)``, ``dl (B, nx, nl)``, ``dv (B, nx, nv)`` - row
    j the tangent for dx0 = e_j - and ``status (B,)``.  The result is DETACHED: the inputs' graphs are not read and
    none is recorded (differentiate through ``solve_mpc`` for gradients of a loss)."""
    with torch.no_grad():
        det = lambda t: t.detach()
        arrs = {k: det(data[k]) for k in MPC_SEQ}
        B = z.shape[0]
        arrs = {k: (a.reshape(1, -1) if a.dim() == 1 else a) for k, a in arrs.items()}
        assert all(a.shape[0] in (1, B) for a in arrs.values())
        res = solver.X0Sensitivity(arrs, det(z).contiguous(), det(l).contiguous(), det(v).contiguous(), sigma=sigma,
                                   want=("dz", "dl", "dv", "gain"))
    return res


def condensed_mpc_x0_sensitivity(cm, data, z, l, v, sigma: float = 0.0):
    """``mpc_x0_sensitivity`` on the condensed route (``CondensedMpc.X0Sensitivity`` of ``cm``, on the images its last
    ``Condense`` / ``Solve`` / ``solve_condensed_mpc`` left, which must be those of ``data``): the same dict -
    ``gain (B, nu, nx)``, ``dz (B, nx, nz)``, ``dl``, ``dv`` and ``status (B,)`` - with the O(sigma) bias of the
    condensed chain.  The result is DETACHED: the inputs' graphs are not read and none is recorded."""
    with torch.no_grad():
        det = lambda t: t.detach()
        arrs = {k: det(data[k]) for k in MPC_SEQ}
        B = z.shape[0]
        arrs = {k: (a.reshape(1, -1) if a.dim() == 1 else a) for k, a in arrs.items()}
        assert all(a.shape[0] in (1, B) for a in arrs.values())
        res = cm.X0Sensitivity(arrs, det(z).contiguous(), det(l).contiguous(), det(v).contiguous(), sigma=sigma,
                               want=("dz", "dl", "dv", "gain"))
    return res


def dense_jacobian(solver, data, z, l, v, wrt: str = "b", sigma: float = 0.0):
    """The dense solutions' sensitivity to one of the arrays f, h, b at the returned points ``(z, l, v)``
    (``FBstabDenseBatch.Jacobian``: one factorisation per QP, one right-hand side per entry of the array): a dict of
    torch tensors on the inputs' device, ``dz (B, nrhs, nz)``, ``dl (B, nrhs, nl)``, ``dv (B, nrhs, nv)`` - row k the
    tangent for the perturbation e_k of ``wrt`` - and ``status (B,)``.  The result is DETACHED: the inputs' graphs
    are not read and none is recorded (differentiate through ``solve_dense`` for gradients of a loss)."""
    with torch.no_grad():
        det = lambda t: t.detach()
        arrs = {k: det(data[k]) for k in DENSE_ARR}
        B = z.shape[0]
        arrs = {k: (a.reshape(1, -1) if a.dim() == 1 else a) for k, a in arrs.items()}
        assert all(a.shape[0] in (1, B) for a in arrs.values())
        res = solver.Jacobian(arrs, det(z).contiguous(), det(l).contiguous(), det(v).contiguous(), wrt=wrt,
                              want=("dz", "dl", "dv"), sigma=sigma)
    return res


class DenseSolveFunction(torch.autograd.Function):
    """apply(solver, sigma, *arrays in DENSE_ARR order) -> (z, l, v, out)."""

    @staticmethod
    def forward(ctx, solver, sigma, *arrs):
        return _forward(DENSE_ARR, ctx, solver, sigma, arrs)

    @staticmethod
    def backward(ctx, gz, gl, gv, gout):
        return _backward(DENSE_ARR, ctx, gz, gl, gv, gout)

    @staticmethod
    def jvp(ctx, solver_t, sigma_t, *tangents):
        return _jvp(DENSE_ARR, ctx, tangents)


def solve_dense(solver, data, sigma: float = 0.0):
    """Differentiable batched dense solve: ``data`` maps the six names of DENSE_ARR to ``(B, len)`` float64 CUDA
    tensors (any of them may require grad; ``(len,)`` or ``(1, len)``: a parameter shared by the batch).  Returns
    ``(z, l, v, out)``; see the module docstring."""
    return DenseSolveFunction.apply(solver, sigma, *[data[k] for k in DENSE_ARR])


class ClosedLoopMpcFunction(torch.autograd.Function):
    """apply(solver, steps, retire, sigma, A, B, *sequences in MPC_SEQ order[, w, shift]) -> (u, x, out)."""

    @staticmethod
    def forward(ctx, solver, steps, retire, sigma, A, B, *rest):
        seqs, (w, shift) = rest[:len(MPC_SEQ)], (rest[len(MPC_SEQ):] or (None, False))
        Bn = max(a.shape[0] if a.dim() == 2 else 1 for a in seqs)
        ctx.shared = tuple(k for k, a in zip(MPC_SEQ, seqs) if Bn > 1 and (a.dim() == 1 or a.shape[0] == 1))
        assert "x0" not in ctx.shared, "every trajectory has its own initial state"
        ctx.shapes = {k: a.shape for k, a in zip(MPC_SEQ, seqs)}
        data = {k: (a.detach().reshape(1, a.numel()) if k in ctx.shared else a.detach()).contiguous()
                for k, a in zip(MPC_SEQ, seqs)}
        dev = data["Q"].device
        # (the sweep advances x0 in place and wants one copy of every sequence per trajectory)
        run = {k: (a.expand(Bn, a.shape[1]).contiguous() if k in ctx.shared else a) for k, a in data.items()}
        run["x0"] = data["x0"].clone()
        mk = lambda n: torch.zeros((Bn, n), dtype=torch.float64, device=dev)
        z, l, v, y = mk(solver.nz), mk(solver.nl), mk(solver.nv), mk(solver.nv)
        if w is None and not shift:
            r = solver.RecedingSweep(run, z, l, v, y, A.detach(), B.detach(), steps, retire=retire, log_inputs=True,
                                     log=True)
        else:
            r = solver.RecedingSweep(run, z, l, v, y, A.detach(), B.detach(), steps, retire=retire, log_inputs=True,
                                     log=True, w=None if w is None else w.detach(), shift=bool(shift))
        u = r["u"]
        x = torch.cat([r["x_log"][1:], run["x0"][None]], 0)
        ctx.solver, ctx.steps, ctx.retire, ctx.sigma = solver, steps, retire, sigma
        ctx.save_for_backward(A.detach(), B.detach(), u, *[r[k] for k in ("z_log", "l_log", "v_log", "x_log",
                                                                           "eflag_log")],
                              *[data[k] for k in MPC_SEQ])
        ctx.mark_non_differentiable(r["out"])
        return u, x, r["out"]

    @staticmethod
    def backward(ctx, gu, gx, gout):
        need = ctx.needs_input_grad
        want = [k for k, n in zip(MPC_SEQ, need[6:6 + len(MPC_SEQ)]) if n]
        plant = need[4] or need[5]
        noise = len(need) > 6 + len(MPC_SEQ) and need[6 + len(MPC_SEQ)]
        if not want and not plant and not noise:
            return (None,) * len(need)
        A, B, u, zl, ll, vl, xl, el = ctx.saved_tensors[:8]
        data = dict(zip(MPC_SEQ, ctx.saved_tensors[8:]))
        log = dict(z_log=zl, l_log=ll, v_log=vl, eflag_log=el)
        g = ctx.solver.RecedingSweepAdjoint(data, A, B, ctx.steps, log, gu=gu.contiguous(), gx=gx.contiguous(),
                                            retire=ctx.retire, sigma=ctx.sigma, want=want, mu=plant or noise)
        gA = gB = None
        if plant or noise:
            # x_(k+1) of a retired trajectory is the constant 0: its costates reach neither the plant nor w_k
            mu = torch.where((el == -1)[:, :, None], torch.zeros_like(g["mu"]), g["mu"])
            gA = torch.einsum("kbi,kbj->ij", mu, xl) if need[4] else None
            gB = torch.einsum("kbi,kbj->ij", mu, u) if need[5] else None
        grads = []
        for k in MPC_SEQ:
            if k not in want:
                grads.append(None)
            elif k in ctx.shared:
                grads.append(g[k].sum(0).reshape(ctx.shapes[k]))
            else:
                grads.append(g[k])
        tail = (mu if noise else None, None)[:len(need) - 6 - len(MPC_SEQ)]
        return (None, None, None, None, gA, gB) + tuple(grads) + tail


def closed_loop_mpc(solver, data, A, B, steps: int, retire: bool = True, sigma: float = 0.0, w=None,
                    shift: bool = False):
    """Differentiable receding-horizon sweep: ``data`` as for ``solve_mpc`` (``x0``: the trajectories' initial
    states, ``(B, nx)``), ``A``/``B`` the plant x+ = A x + B u0 as ``(nx, nx)``/``(nx, nu)`` float64 CUDA tensors.
    ``w``: None, or the disturbances ``(steps, B, nx)`` of x+ = A x + B u0 + w_k (may require grad: ``w.grad`` is the
    costate of every step, zero once the trajectory is retired); ``shift``: the shifted warm start.
    Returns ``(u, x, out)``: the inputs ``(steps, B, nu)``, the states after each step ``(steps, B, nx)`` and the last
    step's SolverOut records; see the module docstring."""
    seqs = [data[k] for k in MPC_SEQ]
    if w is None and not shift:
        return ClosedLoopMpcFunction.apply(solver, steps, retire, sigma, A, B, *seqs)
    return ClosedLoopMpcFunction.apply(solver, steps, retire, sigma, A, B, *seqs, w, bool(shift))


class CondensedMpcSolveFunction(torch.autograd.Function):
    """apply(cm, sigma, *sequences in MPC_SEQ order) -> (z, l, v, out); ``cm``: a ``condense.CondensedMpc``."""

    @staticmethod
    def forward(ctx, cm, sigma, *seqs):
        B = max(a.shape[0] if a.dim() == 2 else 1 for a in seqs)
        ctx.shared = tuple(k for k, a in zip(MPC_SEQ, seqs) if B > 1 and (a.dim() == 1 or a.shape[0] == 1))
        assert "x0" not in ctx.shared, "every QP has its own initial state"
        ctx.shapes = {k: a.shape for k, a in zip(MPC_SEQ, seqs)}
        data = {k: (a.detach().reshape(1, a.numel()) if (k in ctx.shared or a.dim() == 1) else a.detach()).contiguous()
                for k, a in zip(MPC_SEQ, seqs)}
        dev = data["Q"].device
        mk = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
        z, l, v, y = mk(cm.nz), mk(cm.nl), mk(cm.nv), mk(cm.nv)
        out = cm.Solve(data, z, l, v, y, recondense="all")
        ctx.cm, ctx.sigma, ctx.generation = cm, sigma, cm.generation
        ctx.save_for_backward(*[data[k] for k in MPC_SEQ], z, l, v, out)
        ctx.save_for_forward(*[data[k] for k in MPC_SEQ], z, l, v, out)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out)
        return z, l, v, out

    @staticmethod
    def jvp(ctx, cm_t, sigma_t, *tangents):
        saved = ctx.saved_tensors
        data = dict(zip(MPC_SEQ, saved[:len(MPC_SEQ)]))
        z, l, v, out = saved[len(MPC_SEQ):]
        ddata = {}
        for k, t in zip(MPC_SEQ, tangents):
            if t is None or t.numel() == 0:
                continue
            t = t.detach()
            ddata[k] = (t.reshape(1, t.numel()) if (k in ctx.shared or t.dim() == 1) else t).contiguous()
        if ctx.cm.generation != ctx.generation:  # another Condense or Solve has replaced the forward's images
            ctx.cm.Condense(data)
        res = ctx.cm.Tangent(data, z, l, v, ddata, sigma=ctx.sigma)
        eflag = out[:, 0:4].contiguous().view(torch.int32)[:, 0]  # SolverOut::eflag, on the device
        keep = ((eflag == 0) & (res["status"] == 0))[:, None]
        return tuple(torch.where(keep, res[k], torch.zeros_like(res[k])) for k in ("dz", "dl", "dv")) + (None,)

    @staticmethod
    def backward(ctx, gz, gl, gv, gout):
        want = [k for k, n in zip(MPC_SEQ, ctx.needs_input_grad[2:]) if n]
        if not want:
            return (None, None) + (None,) * len(MPC_SEQ)
        saved = ctx.saved_tensors
        data = dict(zip(MPC_SEQ, saved[:len(MPC_SEQ)]))
        z, l, v, out = saved[len(MPC_SEQ):]
        gz = torch.zeros_like(z) if gz is None else gz.contiguous()
        gl, gv = (None if g is None else g.contiguous() for g in (gl, gv))
        if ctx.cm.generation != ctx.generation:  # another Condense or Solve has replaced the forward's images
            ctx.cm.Condense(data)
        g = ctx.cm.Adjoint(data, z, l, v, gz, gl, gv, sigma=ctx.sigma, want=want)
        eflag = out[:, 0:4].contiguous().view(torch.int32)[:, 0]  # SolverOut::eflag, on the device
        keep = ((eflag == 0) & (g["status"] == 0))[:, None]
        grads = []
        for k in MPC_SEQ:
            if k not in want:
                grads.append(None)
                continue
            gk = torch.where(keep, g[k], torch.zeros_like(g[k]))
            grads.append(gk.sum(0).reshape(ctx.shapes[k]) if k in ctx.shared else gk.reshape(ctx.shapes[k]))
        return (None, None) + tuple(grads)


def solve_condensed_mpc(cm, data, sigma: float = 0.0):
    """Differentiable batched solve on the condensed route: ``cm`` a ``condense.CondensedMpc``, ``data`` as for
    ``solve_mpc`` (``(len,)`` or ``(1, len)``: a parameter shared by the batch; its gradient is the sum over the
    batch, formed in torch).  Returns ``(z, l, v, out)`` with ``out`` the dense solver's records; see the module
    docstring."""
    return CondensedMpcSolveFunction.apply(cm, sigma, *[data[k] for k in MPC_SEQ])


class ClosedLoopCondensedMpcFunction(torch.autograd.Function):
    """apply(cm, steps, retire, sigma, A, B, *sequences in MPC_SEQ order, w, shift[, q, r, c, d references]) ->
    (u, x, out); ``cm``: a ``condense.CondensedMpc``.  A reference is None or ``(steps, batch, len)`` /
    ``(steps, 1, len)``."""

    @staticmethod
    def forward(ctx, cm, steps, retire, sigma, A, B, *rest):
        seqs, (w, shift), refs = rest[:len(MPC_SEQ)], rest[len(MPC_SEQ):len(MPC_SEQ) + 2], rest[len(MPC_SEQ) + 2:]
        ctx.nrefs = len(refs)
        ref = {k: a.detach() for k, a in zip(_REF_SEQ, refs) if a is not None}
        Bn = max(a.shape[0] if a.dim() == 2 else 1 for a in seqs)
        ctx.shared = tuple(k for k, a in zip(MPC_SEQ, seqs) if Bn > 1 and (a.dim() == 1 or a.shape[0] == 1))
        assert "x0" not in ctx.shared, "every trajectory has its own initial state"
        ctx.shapes = {k: a.shape for k, a in zip(MPC_SEQ, seqs)}
        data = {k: (a.detach().reshape(1, a.numel()) if (k in ctx.shared or a.dim() == 1) else a.detach()).contiguous()
                for k, a in zip(MPC_SEQ, seqs)}
        dev = data["Q"].device
        run = dict(data)
        run["x0"] = data["x0"].clone()  # (the sweep advances x0 in place)
        mk = lambda n: torch.zeros((Bn, n), dtype=torch.float64, device=dev)
        z, l, v, y = mk(cm.nz), mk(cm.nl), mk(cm.nv), mk(cm.nv)
        r = cm.RecedingSweep(run, z, l, v, y, A.detach(), B.detach(), steps, retire=retire,
                             w=None if w is None else w.detach(), shift=bool(shift), log=("x", "U", "v"),
                             ref=ref or None)
        u = r["u"]
        x = torch.cat([r["x"][1:], run["x0"][None]], 0)
        ctx.cm, ctx.steps, ctx.retire, ctx.sigma = cm, steps, retire, sigma
        ctx.ref_names = tuple(ref)
        saved = (A.detach(), B.detach(), u, r["x"], r["U"], r["v"], r["eflag"], *[data[k] for k in MPC_SEQ],
                 *ref.values())
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        # absent tangents reach `jvp` as None instead of zeros (a tangent on a matrix sequence must be told from none);
        # `backward` hands an absent seed on as None, which the adjoint call reads as zeros
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(r["out"])
        return u, x, r["out"]

    @staticmethod
    def jvp(ctx, cm_t, steps_t, retire_t, sigma_t, A_t, B_t, *rest):
        nseq = len(MPC_SEQ)
        seq_t, w_t, ref_t = rest[:nseq], rest[nseq], rest[nseq + 2:]
        A, B, u, xl, Ul, vl, el = ctx.saved_tensors[:7]
        data = dict(zip(MPC_SEQ, ctx.saved_tensors[7:7 + nseq]))
        ref = dict(zip(ctx.ref_names, ctx.saved_tensors[7 + nseq:]))
        dx0, ddata, dref = None, {}, {}
        for k, t in zip(MPC_SEQ, seq_t):
            if t is None or t.numel() == 0:
                continue
            if k not in _REF_SEQ and k != "x0":
                raise NotImplementedError(
                    "forward mode through closed_loop_condensed_mpc: a tangent on the matrix sequence %r - x0, q, r, c, "
                    "d, the per-step references, w, A and B are served" % k)
            t = t.detach()
            if k == "x0":
                dx0 = t.reshape(data["x0"].shape).contiguous()
            elif k not in ctx.ref_names:   # (data's sequence does not enter where a reference stands in its place)
                ddata[k] = (t.reshape(1, t.numel()) if (k in ctx.shared or t.dim() == 1) else t).contiguous()
        for k, t in zip(_REF_SEQ, ref_t):
            if t is not None and k in ctx.ref_names:
                dref[k] = t.detach().contiguous()
        dw = None if w_t is None else w_t.detach().contiguous()
        if A_t is not None or B_t is not None:
            # directions of the plant enter as dw_k += dA x_k + dB u_k; x_(k+1) of a retired step is the constant 0
            # (a plant of every trajectory's own, (batch, nx, nx) / (batch, nx, nu), has a tangent of that shape)
            fold = lambda t, v: torch.einsum("bij,kbj->kbi" if t.dim() == 3 else "ij,kbj->kbi", t.detach(), v)
            extra = torch.zeros_like(xl)
            if A_t is not None:
                extra = extra + fold(A_t, xl)
            if B_t is not None:
                extra = extra + fold(B_t, u)
            extra = torch.where((el == -1)[:, :, None], torch.zeros_like(extra), extra)
            dw = extra if dw is None else dw + extra
        res = ctx.cm.RecedingSweepTangent(data, A, B, ctx.steps, dict(x=xl, U=Ul, v=vl, eflag=el), dx0=dx0, dw=dw,
                                          ddata=ddata or None, dref=dref or None, ref=ref or None, sigma=ctx.sigma)
        return res["du"], res["dx"], None

    @staticmethod
    def backward(ctx, gu, gx, gout):
        need = ctx.needs_input_grad
        nseq = len(MPC_SEQ)
        ref_need = dict(zip(_REF_SEQ, need[8 + nseq:]))
        ref_want = [k for k in ctx.ref_names if ref_need.get(k)]
        # (the data's own q, r, c, d do not enter where a reference stands in their place: their gradient is None)
        want = [k for k, n in zip(MPC_SEQ, need[6:6 + nseq]) if n and k not in ctx.ref_names]
        plant = need[4] or need[5]
        noise = need[6 + nseq]
        if not want and not ref_want and not plant and not noise:
            return (None,) * len(need)
        A, B, u, xl, Ul, vl, el = ctx.saved_tensors[:7]
        data = dict(zip(MPC_SEQ, ctx.saved_tensors[7:7 + nseq]))
        ref = dict(zip(ctx.ref_names, ctx.saved_tensors[7 + nseq:]))
        log = dict(x=xl, U=Ul, v=vl, eflag=el)
        g = ctx.cm.RecedingSweepAdjoint(data, A, B, ctx.steps, log, gu=None if gu is None else gu.contiguous(),
                                        gx=None if gx is None else gx.contiguous(), retire=ctx.retire, sigma=ctx.sigma,
                                        want=[k for k in want if k != "x0"] + ref_want, mu=plant or noise,
                                        ref=ref or None)
        gA = gB = mu = None
        if plant or noise:
            # x_(k+1) of a retired trajectory is the constant 0: its costates reach neither the plant nor w_k
            mu = torch.where((el == -1)[:, :, None], torch.zeros_like(g["mu"]), g["mu"])
            gA = torch.einsum("kbi,kbj->ij", mu, xl) if need[4] else None
            gB = torch.einsum("kbi,kbj->ij", mu, u) if need[5] else None
        grads = []
        for k in MPC_SEQ:
            if k not in want:
                grads.append(None)
            elif k in ctx.shared:
                grads.append(g[k].sum(0).reshape(ctx.shapes[k]))
            else:
                grads.append(g[k].reshape(ctx.shapes[k]))
        rgrads = []
        for k in _REF_SEQ[:ctx.nrefs]:   # a (steps, 1, len) reference: the torch sum over the batch
            if k not in ref_want:
                rgrads.append(None)
            else:
                rgrads.append(g[k].sum(1, keepdim=True) if ref[k].shape[1] == 1 and g[k].shape[1] > 1 else g[k])
        return (None, None, None, None, gA, gB) + tuple(grads) + (mu if noise else None, None) + tuple(rgrads)


def closed_loop_condensed_mpc(cm, data, A, B, steps: int, retire: bool = True, sigma: float = 0.0, w=None,
                              shift: bool = False, ref=None):
    """``closed_loop_mpc`` on the condensed route: ``cm`` a ``condense.CondensedMpc``, the forward pass one
    ``CondensedMpc.RecedingSweep`` (affine mode, logged), the backward pass ONE ``CondensedMpc.RecedingSweepAdjoint``
    call.  ``data``, ``A``/``B``, ``w``, ``shift`` and the returned ``(u, x, out)`` as there (``out``: the dense
    solver's records of the last step).  ``A.grad`` and ``B.grad`` are formed in torch from the costates, the state
    log and ``u``, leaving out the costates of retired steps; ``w.grad`` is the costate of every step, zero once the
    trajectory is retired; a shared ``(len,)`` / ``(1, len)`` sequence gets the torch sum over the batch.
    ``ref``: per-step references as ``CondensedMpc.RecedingSweep`` takes them - a dict with any of ``q, r, c, d``,
    ``(steps, batch, len)`` or ``(steps, 1, len)``.  They are inputs of the function: a reference's ``.grad`` is the
    per-step array (the torch sum over the batch for a ``(steps, 1, len)`` one, folded back by torch where the
    reference is an ``as_strided`` sliding window over a longer tensor), and ``data``'s sequence of that name does
    not enter the loop.
    Forward mode (``torch.autograd.forward_ad``): ONE ``CondensedMpc.RecedingSweepTangent`` call gives ``u`` and ``x``
    their tangents along the tangents of ``x0, q, r, c, d``, the references, ``w`` and the plant (``A``, ``B`` are
    folded into the disturbance direction in torch, dw_k += dA x_k + dB u_k, left out at retired steps; a shared
    ``(nx, nx)`` / ``(nx, nu)`` plant or a per-trajectory ``(batch, nx, nx)`` / ``(batch, nx, nu)`` one - the backward's
    ``A.grad``, ``B.grad`` serve the shared form alone).  A tangent on a matrix sequence raises
    ``NotImplementedError``."""
    seqs = [data[k] for k in MPC_SEQ]
    if ref is None:
        return ClosedLoopCondensedMpcFunction.apply(cm, steps, retire, sigma, A, B, *seqs, w, bool(shift))
    unknown = set(ref) - set(_REF_SEQ)
    assert not unknown, unknown
    return ClosedLoopCondensedMpcFunction.apply(cm, steps, retire, sigma, A, B, *seqs, w, bool(shift),
                                                *[ref.get(k) for k in _REF_SEQ])
