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
"""
import torch

from .hip_api import DENSE_ARR, MPC_SEQ

__all__ = ["MpcSolveFunction", "solve_mpc", "DenseSolveFunction", "solve_dense"]


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
