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
"""
import torch

from .hip_api import DENSE_ARR, MPC_SEQ

__all__ = ["MpcSolveFunction", "solve_mpc", "DenseSolveFunction", "solve_dense"]


def _forward(names, ctx, solver, sigma, arrs):
    data = {k: a.detach().contiguous() for k, a in zip(names, arrs)}
    first = data[names[0]]  # (Q and H are never empty)
    B, dev = first.shape[0], first.device
    z = torch.zeros((B, solver.nz), dtype=torch.float64, device=dev)
    l = torch.zeros((B, solver.nl), dtype=torch.float64, device=dev)
    v = torch.zeros((B, solver.nv), dtype=torch.float64, device=dev)
    y = torch.zeros((B, solver.nv), dtype=torch.float64, device=dev)
    out = solver.Solve(data, z, l, v, y)
    ctx.solver, ctx.sigma = solver, sigma
    ctx.save_for_backward(*[data[k] for k in names], z, l, v, out)
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
    g = ctx.solver.Adjoint(data, z, l, v, gz.contiguous(), gl.contiguous(), gv.contiguous(), sigma=ctx.sigma,
                           want=want)
    eflag = out[:, 0:4].contiguous().view(torch.int32)[:, 0]  # SolverOut::eflag, on the device
    keep = ((eflag == 0) & (g["status"] == 0))[:, None]
    grads = [torch.where(keep, g[k], torch.zeros_like(g[k])) if k in g else None for k in names]
    return (None, None) + tuple(grads)


class MpcSolveFunction(torch.autograd.Function):
    """apply(solver, sigma, *sequences in MPC_SEQ order) -> (z, l, v, out)."""

    @staticmethod
    def forward(ctx, solver, sigma, *seqs):
        return _forward(MPC_SEQ, ctx, solver, sigma, seqs)

    @staticmethod
    def backward(ctx, gz, gl, gv, gout):
        return _backward(MPC_SEQ, ctx, gz, gl, gv, gout)


def solve_mpc(solver, data, sigma: float = 0.0):
    """Differentiable batched solve: ``data`` maps the 12 names of MPC_SEQ to ``(B, len)`` float64 CUDA tensors
    (any of them may require grad).  Returns ``(z, l, v, out)``; see the module docstring."""
    return MpcSolveFunction.apply(solver, sigma, *[data[k] for k in MPC_SEQ])


class DenseSolveFunction(torch.autograd.Function):
    """apply(solver, sigma, *arrays in DENSE_ARR order) -> (z, l, v, out)."""

    @staticmethod
    def forward(ctx, solver, sigma, *arrs):
        return _forward(DENSE_ARR, ctx, solver, sigma, arrs)

    @staticmethod
    def backward(ctx, gz, gl, gv, gout):
        return _backward(DENSE_ARR, ctx, gz, gl, gv, gout)


def solve_dense(solver, data, sigma: float = 0.0):
    """Differentiable batched dense solve: ``data`` maps the six names of DENSE_ARR to ``(B, len)`` float64 CUDA
    tensors (any of them may require grad).  Returns ``(z, l, v, out)``; see the module docstring."""
    return DenseSolveFunction.apply(solver, sigma, *[data[k] for k in DENSE_ARR])
