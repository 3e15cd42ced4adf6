"""The batched QP solve as a differentiable torch operation.

`qp_solve(qp, q, l, u, Ax=None, Px=None)` solves `qp`'s batch for the given data and returns the
unscaled x [B, n] and y [B, m]; torch.autograd carries a loss on them back to the data through one
adjoint launch (BatchQP.adjoint, mpcqp_adjoint): the one-sided derivative on the solution's active
set, as in every QP layer.  Instances the solve did not solve contribute zero gradients.
torch.autograd.forward_ad carries tangents of the data forward through the solve instead, by one
tangent launch right behind it (BatchQP.tangent, mpcqp_tangent): the mode for a closed loop, where
the handle moves on before a backward pass could come back to a step.

The backward contract: q, l, u, Ax, Px are per instance ([B, .]); a shared 1-D q or Px receives
the sum over the batch.  Without a tape, one backward per forward: the adjoint reads the state the
handle carries, so it must run before the handle's next data, state or settings call (a later call
makes backward raise MPCQPError; retain_graph does not lift that).

`qp_solve(..., tape=True)` lifts that: forward records the solve (BatchQP.tape: the active rows, the
solution and the data, about (n + 3 m + nnzA) * 8 + m bytes per instance, held by the graph) and
backward replays the adjoint from the record (BatchQP.adjoint_replay, mpcqp_adjoint_replay).  So a
loop of qp_solve calls on one warm handle -- an MPC rollout, a weight-tuning objective over a
closed loop -- takes one loss.backward() at the end: backward is legal at any later time, after any
number of further solves on the handle, and again under retain_graph (bitwise the same gradients).
Reverse mode costs one right-hand side per step whatever the number of parameters.  The cost
tensors q and Px are referenced by the record, not copied: do not write them in place before
backward.
"""
from __future__ import annotations

import torch

from ._lib import MPCQPError
from .engine import BatchQP


class _QPSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qp: BatchQP, polish: bool, tape: bool, q, l, u, Ax, Px):
        if qp._has_data:
            qp.update(q=q, l=l, u=u, Ax=Ax, Px=Px)
        else:
            qp.set_data(Px=Px, q=q, Ax=Ax, l=l, u=u)
        r = qp.solve()
        if polish:
            qp.polish()
        ctx.qp, ctx.result, ctx.solve_id = qp, r, qp._solves
        ctx.tape = qp.tape() if tape else None
        ctx.shapes = [None if t is None else t.shape for t in (q, l, u, Ax, Px)]
        ctx.set_materialize_grads(False)
        # the handle's output buffers are overwritten by its next solve: hand out copies
        return r.x.clone(), r.y.clone()

    @staticmethod
    def jvp(ctx, _qp, _polish, _tape, *tangents):
        # forward mode (torch.autograd.forward_ad): called right behind forward, while the handle
        # carries its state -- one tangent launch, one direction; a shared 1-D tangent is every
        # instance's
        qp = ctx.qp
        d = [None if t is None else t.expand(qp.B, -1) if t.dim() == 1 else t for t in tangents]
        t = qp.tangent(*d[:3], dAx=d[3], dPx=d[4], out=ctx.result)
        return t.dx[0], t.dy[0]

    @staticmethod
    def backward(ctx, gx, gy):
        qp, need = ctx.qp, ctx.needs_input_grad[3:]
        if ctx.tape is None and qp._solves != ctx.solve_id:
            raise MPCQPError("mpcqp_adjoint: the handle has solved again since this forward")
        if gx is None:
            gx = torch.zeros(qp.B, qp.n, dtype=torch.float64, device=qp.device)
        names = ("gq", "gl", "gu", "gAx", "gPx")
        want = [k for k, nd in zip(names, need) if nd]
        if ctx.tape is None:
            a = qp.adjoint(gx, gy, out=ctx.result, want=want)
        else:
            a = qp.adjoint_replay(ctx.tape, gx, gy, want=want)
        grads = []
        for k, nd, shape in zip(names, need, ctx.shapes):
            g = getattr(a, k)[0] if nd else None
            grads.append(g.sum(0) if nd and len(shape) == 1 else g)
        return (None, None, None, *grads)


def qp_solve(qp: BatchQP, q, l, u, Ax=None, Px=None, polish=True, tape=False):
    """Solve qp's batch for q [B, n], l, u [B, m] and optionally Ax [B, nnzA], Px [B, nnzP] (None:
    the values the handle holds, or those of the matrices it was created from); polish: polish
    the solved instances before the adjoint (the active set and the accuracy of x, y it gives are
    what the gradient is taken on); tape: record the solve so that backward may come at any later
    time, after further solves on qp (module docstring).  Returns (x, y), differentiable with
    respect to the tensors given."""
    return _QPSolve.apply(qp, bool(polish), bool(tape), q, l, u, Ax, Px)
