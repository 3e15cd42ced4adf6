"""Batched torch front-end of the HIP engine.

`BatchQP` owns one `mpcqp_handle`: B instances that share the sparsity of P and A -- the shape of
every MPC-QP the reference builds for one scenario family (reference
src/trajectorySimulate.py:216-236).  The values of P and q are shared by the batch too, unless they
are given per instance ((B, nnzP) / (B, n): one cost-weight set per instance).  All tensors are float64 / int32 on the GPU; the
engine never silently moves work to the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._lib import MPCQPError, check

OSQP_INFTY = 1e30
MPCQP_UNSOLVED = -10  # OSQP 0.6 status_val of an instance no solve has touched (include/mpcqp.h)


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise MPCQPError("the MPC-QP engine needs a ROCm GPU (torch.cuda.is_available() is False)")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise MPCQPError(f"device must be a GPU, got {dev}")
    return dev


def triu_csc(P) -> sp.csc_matrix:
    """Upper triangle of P in sorted CSC (what OSQP's Python wrapper hands to the C core)."""
    P = sp.csc_matrix(P)
    if sp.tril(P, -1).nnz:
        P = sp.triu(P, format="csc")
    P = sp.csc_matrix(P)
    P.sort_indices()
    return P


def sorted_csc(A) -> sp.csc_matrix:
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


@dataclass
class SolveResult:
    x: torch.Tensor         # [B, n] unscaled primal (NaN without solution)
    y: torch.Tensor         # [B, m] unscaled dual
    status: torch.Tensor    # [B] int32, OSQP status_val
    iter: torch.Tensor      # [B] int32
    rho_updates: torch.Tensor
    obj_val: torch.Tensor
    pri_res: torch.Tensor
    dua_res: torch.Tensor
    rho: torch.Tensor


@dataclass
class PolishResult:
    x: torch.Tensor              # [B, n] the solve's buffer: polished rows overwritten
    y: torch.Tensor              # [B, m]
    status_polish: torch.Tensor  # [B] int32: 1 polished, -1 unsuccessful, 0 not attempted
    obj_val: torch.Tensor        # [B] of the solution left in x / y (NaN where not attempted)
    pri_res: torch.Tensor
    dua_res: torch.Tensor
    n_low: torch.Tensor          # [B] int32 sizes of the two active sets (0 where not attempted)
    n_upp: torch.Tensor


@dataclass
class AdjointResult:
    """Outputs of BatchQP.adjoint, [nrhs, B, .]; None where not requested.  Rows of instances that
    were not attempted (status_adjoint 0) are zero."""
    gq: torch.Tensor             # dL/dq [nrhs, B, n]
    gl: torch.Tensor             # dL/dl, dL/du [nrhs, B, m]
    gu: torch.Tensor
    gPx: torch.Tensor            # dL/dPx [nrhs, B, nnzP] (a stored upper entry stands for both halves)
    gAx: torch.Tensor            # dL/dAx [nrhs, B, nnzA]
    res: torch.Tensor            # [nrhs, B] relative residual of the scaled adjoint system
    act: torch.Tensor            # [B, m] int8: -1 lower-active, +1 upper-active, 0 inactive
    status_adjoint: torch.Tensor  # [B] int32: 1 done, 0 not attempted


@dataclass
class TangentResult:
    """Outputs of BatchQP.tangent, [ndir, B, .]; None where not requested.  Rows of instances that
    were not attempted (status_tangent 0) are zero."""
    dx: torch.Tensor             # [ndir, B, n]
    dy: torch.Tensor             # [ndir, B, m], 0 off the active rows
    dz: torch.Tensor             # [ndir, B, m] d(Ax) = A dx + dA x
    dobj: torch.Tensor           # [ndir, B] d(x'Px/2 + q'x)
    res: torch.Tensor            # [ndir, B] relative residual of the scaled system
    act: torch.Tensor            # [B, m] int8: -1 lower-active, +1 upper-active, 0 inactive
    status_tangent: torch.Tensor  # [B] int32: 1 done, 0 not attempted


@dataclass
class AdjointTape:
    """What BatchQP.adjoint_replay needs of one solve, taken by BatchQP.tape right after it.  The
    caller owns it; the handle may solve, update and be re-set-up freely afterwards.  Px and q are
    references to the cost tensors in force at the solve (shared 1-D or per instance 2-D), not
    copies: do not write them in place while the tape is in use."""
    x: torch.Tensor      # [B, n] the unscaled solution (clone)
    y: torch.Tensor      # [B, m]
    act: torch.Tensor    # [B, m] int8: -1 lower-active, +1 upper-active, 0 inactive
    taped: torch.Tensor  # [B] int32: 1 where BatchQP.adjoint would attempt the instance
    Ax: torch.Tensor     # [B, nnzA] the handle's data at the solve (copies)
    l: torch.Tensor      # [B, m]
    u: torch.Tensor
    Px: torch.Tensor     # [nnzP] or [B, nnzP]
    q: torch.Tensor      # [n] or [B, n]


class BatchQP:
    """B OSQP problems with a shared pattern, solved together on one GPU."""

    def __init__(self, P, A, batch: int, device="cuda", stream=None, **settings):
        self.device = _require_gpu(device)
        self.P = triu_csc(P)
        self.A = sorted_csc(A)
        self.n, self.m = self.P.shape[0], self.A.shape[0]
        if self.A.shape[1] != self.n:
            raise ValueError("A must have n columns")
        self.B = int(batch)
        # any setting may be a length-B array: one value per instance (mpcqp_set_settings_batched,
        # sent below before any data); the handle itself is created with the scalar ones
        rows = _lib.settings_rows(self.B, **settings) if _lib.per_instance(settings) else None
        self.settings = _lib.default_settings(
            **{k: v for k, v in settings.items() if np.ndim(v) == 0})
        self._Pp = np.ascontiguousarray(self.P.indptr, dtype=np.int32)
        self._Pi = np.ascontiguousarray(self.P.indices, dtype=np.int32)
        self._Ap = np.ascontiguousarray(self.A.indptr, dtype=np.int32)
        self._Ai = np.ascontiguousarray(self.A.indices, dtype=np.int32)
        st = _lib.Structure(self.n, self.m,
                            self._Pp.ctypes.data_as(C.POINTER(C.c_int32)),
                            self._Pi.ctypes.data_as(C.POINTER(C.c_int32)),
                            self._Ap.ctypes.data_as(C.POINTER(C.c_int32)),
                            self._Ai.ctypes.data_as(C.POINTER(C.c_int32)))
        with torch.cuda.device(self.device):
            self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
            h = C.c_void_p()
            check(_lib.lib().mpcqp_create(C.byref(st), C.byref(self.settings), self.B,
                                          C.c_void_p(self.stream.cuda_stream), C.byref(h)),
                  "mpcqp_create")
        self._h = h
        if rows is not None:
            check(_lib.lib().mpcqp_set_settings_batched(self._h, rows),
                  "mpcqp_set_settings_batched")
        self.nnzP = int(self.P.nnz)
        self.nnzA = int(self.A.nnz)
        self._has_data = False
        self._out = None
        self._solves = 0  # solves enqueued so far (diff.qp_solve: one backward per forward)

    # -------------------------------------------------------------------------------- helpers
    def _t(self, a, shape, name):
        t = torch.as_tensor(a, dtype=torch.float64, device=self.device)
        if tuple(t.shape) != tuple(shape):
            t = t.reshape(shape) if t.numel() == int(np.prod(shape)) else None
        if t is None:
            raise ValueError(f"{name} must have shape {shape}")
        return t.contiguous()

    def _batch_vec(self, a, width, name):
        t = torch.as_tensor(a, dtype=torch.float64, device=self.device)
        if t.dim() == 1:
            if t.numel() != width:
                raise ValueError(f"{name} must have {width} entries per instance")
            t = t.unsqueeze(0).expand(self.B, width)
        if tuple(t.shape) != (self.B, width):
            raise ValueError(f"{name} must have shape ({self.B}, {width})")
        return t.contiguous()

    def _keep(self, **tensors):
        # keep the caller-independent copies alive until the stream has consumed them
        self._inflight = tensors

    # ------------------------------------------------------------------------------------ API
    def _cost(self, a, width, name):
        """cost data shared by the batch, (width,), or per instance, (B, width) -> (tensor,
        per instance?)"""
        t = torch.as_tensor(a, dtype=torch.float64, device=self.device)
        if tuple(t.shape) == (self.B, width):
            return t.contiguous(), True
        if t.dim() == 2 and t.numel() != width:
            raise ValueError(f"{name} must have shape ({width},) or ({self.B}, {width})")
        return self._t(t, (width,), name), False

    def set_data(self, Px=None, q=None, Ax=None, l=None, u=None):
        """Px (nnzP,) / q (n,) shared by the batch, or (B, nnzP) / (B, n): cost data per instance
        (mpcqp_set_data_batched; a shared one beside a per-instance one is broadcast)."""
        Px, bP = self._cost(self.P.data if Px is None else Px, self.nnzP, "Px")
        q, bq = self._cost(q, self.n, "q")
        Ax = self._batch_vec(self.A.data if Ax is None else Ax, self.nnzA, "Ax")
        l = self._batch_vec(l, self.m, "l")
        u = self._batch_vec(u, self.m, "u")
        if bool((l > u).any()):
            raise ValueError("lower bound must be lower than or equal to upper bound")
        if bP or bq:
            Px = Px if bP else self._batch_vec(Px, self.nnzP, "Px")
            q = q if bq else self._batch_vec(q, self.n, "q")
            check(_lib.lib().mpcqp_set_data_batched(self._h, Px.data_ptr(), q.data_ptr(),
                                                    Ax.data_ptr(), l.data_ptr(), u.data_ptr()),
                  "mpcqp_set_data_batched")
        else:
            check(_lib.lib().mpcqp_set_data(self._h, Px.data_ptr(), q.data_ptr(), Ax.data_ptr(),
                                            l.data_ptr(), u.data_ptr()), "mpcqp_set_data")
        self._keep(Px=Px, q=q, Ax=Ax, l=l, u=u)
        self._cost_now = dict(Px=Px.detach(), q=q.detach())  # the cost data in force (tape)
        self._has_data = True

    def update(self, q=None, l=None, u=None, Ax=None, Px=None):
        """OSQP's update(), applied in its order: q, the bounds, then P, then A.  q (n,) or (B, n);
        Px (nnzP,) or (B, nnzP), upper-triangular CSC order (osqp_update_P: mpcqp_update_P)."""
        keep = {}
        if q is not None:
            q, bq = self._cost(q, self.n, "q")
            if bq:
                check(_lib.lib().mpcqp_update_lin_cost_batched(self._h, q.data_ptr()),
                      "mpcqp_update_lin_cost_batched")
            else:
                check(_lib.lib().mpcqp_update_lin_cost(self._h, q.data_ptr()),
                      "mpcqp_update_lin_cost")
            keep["q"] = q
        if l is not None or u is not None:
            if l is None or u is None:
                raise ValueError("update l and u together")
            l = self._batch_vec(l, self.m, "l")
            u = self._batch_vec(u, self.m, "u")
            if bool((l > u).any()):
                raise ValueError("lower bound must be lower than or equal to upper bound")
            check(_lib.lib().mpcqp_update_bounds(self._h, l.data_ptr(), u.data_ptr()),
                  "mpcqp_update_bounds")
            keep.update(l=l, u=u)
        if Px is not None:
            Px, bP = self._cost(Px, self.nnzP, "Px")
            if bP:
                check(_lib.lib().mpcqp_update_P_batched(self._h, Px.data_ptr()),
                      "mpcqp_update_P_batched")
            else:
                check(_lib.lib().mpcqp_update_P(self._h, Px.data_ptr()), "mpcqp_update_P")
            keep["Px"] = Px
        if Ax is not None:
            Ax = self._batch_vec(Ax, self.nnzA, "Ax")
            check(_lib.lib().mpcqp_update_A(self._h, Ax.data_ptr()), "mpcqp_update_A")
            keep["Ax"] = Ax
        self._keep(**keep)
        for k in ("Px", "q"):
            if k in keep:
                self._cost_now[k] = keep[k].detach()

    # set-up settings: fixed by the scaling and the factorization set-up, not updatable (OSQP's too)
    SETUP_SETTINGS = ("sigma", "scaling", "adaptive_rho", "adaptive_rho_interval",
                      "adaptive_rho_tolerance")

    def _settings_rows(self):
        rows = (_lib.Settings * self.B)()
        check(_lib.lib().mpcqp_get_settings(self._h, rows), "mpcqp_get_settings")
        return rows

    def get_settings(self):
        """The settings in force (mpcqp_get_settings): {name: array of B values}."""
        view = _lib.rows_view(self._settings_rows())
        return {name: view[name].copy() for name, _ in _lib.Settings._fields_}

    def update_settings(self, **kw):
        """OSQP's update_settings(): max_iter, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, alpha,
        check_termination, warm_start (mpcqp_update_settings) and rho (osqp_update_rho:
        mpcqp_update_rho), each a scalar or a length-B sequence, one value per instance.  Iterates,
        carried rho (unless given) and data scaling are kept.  A set-up setting is a ValueError."""
        kw = {_lib._setting_key(k): v for k, v in kw.items() if k != "verbose"}
        for k in kw:
            if k in self.SETUP_SETTINGS:
                raise ValueError(f"'{k}' is a set-up setting: it cannot be updated after creation")
        rho = kw.pop("rho", None)
        if kw:
            rows = self._settings_rows()
            # rows that differ (however they were set) are updated row by row: the shared form
            # would write row 0's updatable fields into every row
            view = _lib.rows_view(rows)  # a numpy view: whole columns at once
            mixed = any(bool((view[n] != view[n][0]).any()) for n, _ in _lib.Settings._fields_)
            for k, v in kw.items():
                view[k] = _lib.setting_column(self.B, k, v)
            if mixed or _lib.per_instance(kw):
                check(_lib.lib().mpcqp_update_settings_batched(self._h, rows),
                      "mpcqp_update_settings_batched")
            else:
                check(_lib.lib().mpcqp_update_settings(self._h, C.byref(rows[0])),
                      "mpcqp_update_settings")
                for k in kw:
                    setattr(self.settings, k, getattr(rows[0], k))
        if rho is not None:
            if np.ndim(rho) == 0:
                check(_lib.lib().mpcqp_update_rho(self._h, float(rho)), "mpcqp_update_rho")
            else:
                r = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
                if r.size != self.B:
                    raise ValueError(f"setting 'rho' has {r.size} values for a batch of {self.B}")
                check(_lib.lib().mpcqp_update_rho_batched(
                    self._h, r.ctypes.data_as(C.POINTER(C.c_double))), "mpcqp_update_rho_batched")

    def _on_stream(self, fn, *tensors):
        """run fn (an ABI call that queues copies on the handle's stream) into freshly allocated
        tensors, then order the caller's current stream after it, so the returned tensors are
        safe to use on the current stream whatever stream the handle runs on"""
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)  # the allocations happened on the current stream
        fn()
        for t in tensors:
            t.record_stream(self.stream)
        cur.wait_stream(self.stream)
        return tensors

    def copy_data(self):
        """(Ax, l, u) currently held by the handle, as new device tensors (ordered after the
        handle's stream for the caller's current stream)."""
        f = dict(dtype=torch.float64, device=self.device)
        Ax = torch.empty(self.B, self.nnzA, **f)
        l = torch.empty(self.B, self.m, **f)
        u = torch.empty(self.B, self.m, **f)
        return self._on_stream(lambda: check(_lib.lib().mpcqp_copy_data(
            self._h, Ax.data_ptr(), l.data_ptr(), u.data_ptr()), "mpcqp_copy_data"), Ax, l, u)

    def set_skip(self, mask):
        """int32 device tensor [B] (kept alive by the handle) or None: instances with a non-zero
        entry are skipped by every following solve (outputs and warm state unchanged)"""
        if mask is not None:
            if mask.dtype != torch.int32 or tuple(mask.shape) != (self.B,) or \
                    not mask.is_cuda or not mask.is_contiguous():
                raise ValueError(f"skip mask must be a contiguous int32 tensor of shape ({self.B},)")
        check(_lib.lib().mpcqp_set_skip(self._h, None if mask is None else mask.data_ptr()),
              "mpcqp_set_skip")
        self._skip = mask

    def set_order(self, order):
        """int32 device tensor [B] (kept alive by the handle) or None: a permutation of the
        instance ids, the order in which the persistent launch takes instances (results unchanged;
        mpcqp_set_order).  The tensor is read at every solve, so it may be rewritten in place --
        on the handle's stream, and only with another permutation (a duplicate id would let two
        waves solve one instance at once; a missing id would never be solved).  It is checked to
        be a permutation here, once."""
        if order is not None:
            if order.dtype != torch.int32 or tuple(order.shape) != (self.B,) or \
                    not order.is_cuda or not order.is_contiguous():
                raise ValueError(f"order must be a contiguous int32 tensor of shape ({self.B},)")
            with torch.cuda.stream(self.stream):
                ok = torch.equal(torch.sort(order).values,
                                 torch.arange(self.B, dtype=torch.int32, device=order.device))
            if not ok:
                raise ValueError("order must be a permutation of the instance ids 0..B-1")
        check(_lib.lib().mpcqp_set_order(self._h, None if order is None else order.data_ptr()),
              "mpcqp_set_order")
        self._order = order

    def get_state(self):
        """Warm-start state carried to the next solve (scaled xs, zs, ys; rho; has_state), as new
        device tensors -- the white-box hook the oracle's `state()` mirrors."""
        f = dict(dtype=torch.float64, device=self.device)
        xs = torch.empty(self.B, self.n, **f)
        zs = torch.empty(self.B, self.m, **f)
        ys = torch.empty(self.B, self.m, **f)
        rho = torch.empty(self.B, **f)
        hs = torch.empty(self.B, dtype=torch.int32, device=self.device)
        self._on_stream(lambda: check(_lib.lib().mpcqp_get_state(
            self._h, xs.data_ptr(), zs.data_ptr(), ys.data_ptr(), rho.data_ptr(), hs.data_ptr()),
            "mpcqp_get_state"), xs, zs, ys, rho, hs)
        return dict(x=xs, z=zs, y=ys, rho=rho, has_state=hs)

    def get_scaling(self):
        """The data scaling carried between solves (mpcqp_get_scaling): E of the last solve [B, m]
        and the unscaled P values [B, nnzP] / q [B, n] the next warm solve rescales (OSQP 0.6's
        unscale_data), as new device tensors -- the white-box hook of the oracle's state()/data()"""
        f = dict(dtype=torch.float64, device=self.device)
        E = torch.empty(self.B, self.m, **f)
        Pu = torch.empty(self.B, self.nnzP, **f)
        qu = torch.empty(self.B, self.n, **f)
        self._on_stream(lambda: check(_lib.lib().mpcqp_get_scaling(
            self._h, E.data_ptr(), Pu.data_ptr(), qu.data_ptr()), "mpcqp_get_scaling"), E, Pu, qu)
        return dict(E=E, Pu=Pu, qu=qu)

    def set_state(self, x, z, y, rho, has_state):
        """Overwrite the warm-start state (the reverse of get_state; white-box tests)."""
        f = dict(dtype=torch.float64, device=self.device)
        t = [torch.as_tensor(a, **f).contiguous() for a in (x, z, y, rho)]
        hs = torch.as_tensor(has_state, dtype=torch.int32, device=self.device).contiguous()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        check(_lib.lib().mpcqp_set_state(self._h, *(a.data_ptr() for a in t), hs.data_ptr()),
              "mpcqp_set_state")
        self._keep(state=(t, hs))

    def warm_start(self, x, y):
        x = self._batch_vec(x, self.n, "x")
        y = self._batch_vec(y, self.m, "y")
        check(_lib.lib().mpcqp_warm_start(self._h, x.data_ptr(), y.data_ptr()), "mpcqp_warm_start")

    def new_result(self) -> SolveResult:
        """Output buffers for solve_async(out=...).  An instance that a skip mask keeps from
        being solved keeps its previous outputs, so a fresh buffer starts from defined values:
        status MPCQP_UNSOLVED (-10, OSQP's 'unsolved'), iter 0, x / y / obj / residuals NaN."""
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            nan = float("nan")
            f = dict(dtype=torch.float64, device=self.device)
            i = dict(dtype=torch.int32, device=self.device)
            return SolveResult(
                x=torch.full((self.B, self.n), nan, **f), y=torch.full((self.B, self.m), nan, **f),
                status=torch.full((self.B,), MPCQP_UNSOLVED, **i), iter=torch.zeros(self.B, **i),
                rho_updates=torch.zeros(self.B, **i), obj_val=torch.full((self.B,), nan, **f),
                pri_res=torch.full((self.B,), nan, **f), dua_res=torch.full((self.B,), nan, **f),
                rho=torch.full((self.B,), nan, **f))

    def _outputs(self):
        if self._out is None:
            self._out = self.new_result()
        return self._out

    def solve_async(self, out: SolveResult = None) -> SolveResult:
        """Enqueue one solve of every instance on the handle's stream (no host sync)."""
        if not self._has_data:
            raise MPCQPError("solve before set_data")
        o = out if out is not None else self._outputs()
        info = _lib.Info(o.status.data_ptr(), o.iter.data_ptr(), o.rho_updates.data_ptr(),
                         o.obj_val.data_ptr(), o.pri_res.data_ptr(), o.dua_res.data_ptr(),
                         o.rho.data_ptr())
        check(_lib.lib().mpcqp_solve(self._h, o.x.data_ptr(), o.y.data_ptr(), C.byref(info)),
              "mpcqp_solve")
        self._last = o
        self._solves += 1
        return o

    def solve(self) -> SolveResult:
        o = self.solve_async()
        self.stream.synchronize()
        return o

    def polish(self, status=None, out: SolveResult = None, sync=True) -> PolishResult:
        """Polish the instances the directly preceding solve solved (mpcqp_polish; OSQP's polish
        step with each instance's delta / polish_refine_iter).  out: that solve's result (default:
        the last one), whose x / y rows are overwritten where the polish is accepted; status: the
        int32 [B] device tensor of its statuses (default: out.status).  Enqueued on the handle's
        stream; sync=False returns without waiting for it."""
        o = out if out is not None else getattr(self, "_last", None)
        if o is None:
            raise MPCQPError("mpcqp_polish: polish before any solve")
        st = o.status if status is None else status
        if st.dtype != torch.int32 or tuple(st.shape) != (self.B,) or not st.is_cuda or \
                not st.is_contiguous():
            raise ValueError(f"status must be a contiguous int32 device tensor of shape ({self.B},)")
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            f = dict(dtype=torch.float64, device=self.device)
            i = dict(dtype=torch.int32, device=self.device)
            nan = float("nan")
            r = PolishResult(x=o.x, y=o.y, status_polish=torch.zeros(self.B, **i),
                             obj_val=torch.full((self.B,), nan, **f),
                             pri_res=torch.full((self.B,), nan, **f),
                             dua_res=torch.full((self.B,), nan, **f),
                             n_low=torch.zeros(self.B, **i), n_upp=torch.zeros(self.B, **i))
        info = _lib.PolishInfo(r.status_polish.data_ptr(), r.obj_val.data_ptr(), r.pri_res.data_ptr(),
                               r.dua_res.data_ptr(), r.n_low.data_ptr(), r.n_upp.data_ptr())
        check(_lib.lib().mpcqp_polish(self._h, st.data_ptr(), o.x.data_ptr(), o.y.data_ptr(),
                                      C.byref(info)), "mpcqp_polish")
        if sync:
            self.stream.synchronize()
        return r

    ADJOINT_OUTPUTS = ("gq", "gl", "gu", "gPx", "gAx")

    def adjoint(self, gx, gy=None, refine=3, status=None, want=("gq", "gl", "gu"),
                out: SolveResult = None, sync=True) -> AdjointResult:
        """Adjoint solves of the instances the last solve solved (mpcqp_adjoint): gx = dL/dx
        [nrhs, B, n] (2-D: nrhs = 1) and optionally gy = dL/dy [nrhs, B, m] give the gradients named
        in `want` (of gq, gl, gu, gPx, gAx), [nrhs, B, .], with one factorization per instance
        for all nrhs <= 8 right-hand sides and `refine` rounds of iterative refinement each.  out:
        the solve's (or its polish's) result, default the last one, whose x / y are read; status
        defaults to out.status.  Valid after a solve or a polish of it, until the next data, state or
        settings call; changes no state.  Enqueued on the handle's stream; sync=False returns without
        waiting for it."""
        o = out if out is not None else getattr(self, "_last", None)
        if o is None:
            raise MPCQPError("mpcqp_adjoint: adjoint before any solve")
        st = o.status if status is None else status
        if st.dtype != torch.int32 or tuple(st.shape) != (self.B,) or not st.is_cuda or \
                not st.is_contiguous():
            raise ValueError(f"status must be a contiguous int32 device tensor of shape ({self.B},)")
        gx, gy, r, ain, aout = self._adjoint_io(gx, gy, refine, want)
        check(_lib.lib().mpcqp_adjoint(self._h, st.data_ptr(), o.x.data_ptr(), o.y.data_ptr(),
                                       C.byref(ain), C.byref(aout)), "mpcqp_adjoint")
        return self._adjoint_done(gx, gy, r, sync)

    def _adjoint_io(self, gx, gy, refine, want):
        """the right-hand sides checked and made contiguous, the AdjointResult allocated on the
        handle's stream, and the two ABI structs of mpcqp_adjoint / mpcqp_adjoint_replay"""
        unknown = [w for w in want if w not in self.ADJOINT_OUTPUTS]
        if unknown:
            raise ValueError(f"unknown adjoint outputs {unknown}: choose from {self.ADJOINT_OUTPUTS}")
        gx = torch.as_tensor(gx, dtype=torch.float64, device=self.device)
        gx = gx.unsqueeze(0) if gx.dim() == 2 else gx
        if gx.dim() != 3 or tuple(gx.shape[1:]) != (self.B, self.n):
            raise ValueError(f"gx must have shape (nrhs, {self.B}, {self.n}) or ({self.B}, {self.n})")
        nrhs = int(gx.shape[0])
        gx = gx.contiguous()
        if gy is not None:
            gy = torch.as_tensor(gy, dtype=torch.float64, device=self.device)
            gy = gy.unsqueeze(0) if gy.dim() == 2 else gy
            if tuple(gy.shape) != (nrhs, self.B, self.m):
                raise ValueError(f"gy must have shape ({nrhs}, {self.B}, {self.m})")
            gy = gy.contiguous()
        width = dict(gq=self.n, gl=self.m, gu=self.m, gPx=self.nnzP, gAx=self.nnzA)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))  # gx / gy are complete
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            f = dict(dtype=torch.float64, device=self.device)
            g = {k: torch.empty(nrhs, self.B, width[k], **f) if k in want else None
                 for k in self.ADJOINT_OUTPUTS}
            r = AdjointResult(**g, res=torch.empty(nrhs, self.B, **f),
                              act=torch.empty(self.B, self.m, dtype=torch.int8, device=self.device),
                              status_adjoint=torch.empty(self.B, dtype=torch.int32, device=self.device))
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        ain = _lib.AdjointIn(nrhs, int(refine), gx.data_ptr(), ptr(gy))
        aout = _lib.AdjointOut(*(ptr(g[k]) for k in self.ADJOINT_OUTPUTS), r.res.data_ptr(),
                               r.act.data_ptr(), r.status_adjoint.data_ptr())
        return gx, gy, r, ain, aout

    def _adjoint_done(self, gx, gy, r, sync):
        for t in (gx, gy):
            if t is not None:
                t.record_stream(self.stream)
        if sync:
            self.stream.synchronize()
        else:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return r

    def tape(self, out: SolveResult = None, status=None) -> AdjointTape:
        """Record the last solve for a later adjoint (mpcqp_adjoint_tape), right after solve() or
        polish(): clones of out's x / y (default: the last result), the active rows and the
        attempted instances as BatchQP.adjoint would report them at this point (status defaults to
        out.status), copies of the handle's Ax, l, u, and references to the Px / q tensors in
        force.  Valid where adjoint is; changes no state.  The caller owns the memory: about
        (n + 3 m + nnzA) * 8 + m bytes per instance and tape."""
        o = out if out is not None else getattr(self, "_last", None)
        if o is None:
            raise MPCQPError("mpcqp_adjoint_tape: tape before any solve")
        st = o.status if status is None else status
        if st.dtype != torch.int32 or tuple(st.shape) != (self.B,) or not st.is_cuda or \
                not st.is_contiguous():
            raise ValueError(f"status must be a contiguous int32 device tensor of shape ({self.B},)")
        f = dict(dtype=torch.float64, device=self.device)
        Ax = torch.empty(self.B, self.nnzA, **f)
        l, u = torch.empty(self.B, self.m, **f), torch.empty(self.B, self.m, **f)
        act = torch.empty(self.B, self.m, dtype=torch.int8, device=self.device)
        taped = torch.empty(self.B, dtype=torch.int32, device=self.device)
        x, y = torch.empty_like(o.x), torch.empty_like(o.y)

        def record():
            check(_lib.lib().mpcqp_adjoint_tape(self._h, st.data_ptr(), act.data_ptr(),
                                                taped.data_ptr()), "mpcqp_adjoint_tape")
            check(_lib.lib().mpcqp_copy_data(self._h, Ax.data_ptr(), l.data_ptr(), u.data_ptr()),
                  "mpcqp_copy_data")
            with torch.cuda.stream(self.stream):
                x.copy_(o.x), y.copy_(o.y)
        self._on_stream(record, Ax, l, u, act, taped, x, y)
        return AdjointTape(x=x, y=y, act=act, taped=taped, Ax=Ax, l=l, u=u, **self._cost_now)

    def adjoint_replay(self, tape: AdjointTape, gx, gy=None, refine=3, want=("gq", "gl", "gu"),
                       sync=True) -> AdjointResult:
        """BatchQP.adjoint of the solve `tape` was taken at, from the tape alone
        (mpcqp_adjoint_replay): the handle lends its plan, settings and stream and may be in any
        state -- solved again, updated, given other data, or fresh before set_data (a tape of
        another handle with the same structure and batch is as good).  gx, gy, refine, want and the
        result are adjoint's; act echoes the tape's, status_adjoint its `taped`.  Equal to adjoint
        at the tape point to rounding (bitwise where that solve's scaling started from the
        set-up data); changes no state."""
        gx, gy, r, ain, aout = self._adjoint_io(gx, gy, refine, want)
        pt = self._tape_point(tape)
        check(_lib.lib().mpcqp_adjoint_replay(self._h, C.byref(pt), C.byref(ain), C.byref(aout)),
              "mpcqp_adjoint_replay")
        for t in vars(tape).values():
            t.record_stream(self.stream)
        return self._adjoint_done(gx, gy, r, sync)

    def _tape_point(self, tape: AdjointTape):
        """the ABI's mpcqp_adjoint_point of a tape whose tensors fit this handle"""
        bP, bq = tape.Px.dim() == 2, tape.q.dim() == 2
        for t, shape, name in ((tape.Px, (self.B,) * bP + (self.nnzP,), "Px"), (tape.q, (self.B,) * bq + (self.n,), "q"),
                               (tape.Ax, (self.B, self.nnzA), "Ax"), (tape.l, (self.B, self.m), "l"),
                               (tape.u, (self.B, self.m), "u"), (tape.x, (self.B, self.n), "x"),
                               (tape.y, (self.B, self.m), "y"), (tape.act, (self.B, self.m), "act"),
                               (tape.taped, (self.B,), "taped")):
            if tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"tape.{name} must be a contiguous device tensor of shape {shape}")
        return _lib.AdjointPoint(tape.Px.data_ptr(), tape.q.data_ptr(), int(bP), int(bq),
                                 tape.Ax.data_ptr(), tape.l.data_ptr(), tape.u.data_ptr(),
                                 tape.x.data_ptr(), tape.y.data_ptr(), tape.act.data_ptr(),
                                 tape.taped.data_ptr())

    TANGENT_OUTPUTS = ("dx", "dy", "dz", "dobj")

    def tangent(self, dq=None, dl=None, du=None, dAx=None, dPx=None, refine=3, status=None,
                want=("dx", "dy"), out: SolveResult = None, sync=True) -> TangentResult:
        """Forward sensitivities of the instances the last solve solved (mpcqp_tangent): the
        perturbations dq [ndir, B, n], dl, du [ndir, B, m], dAx [ndir, B, nnzA], dPx [ndir, B, nnzP]
        (2-D: ndir = 1; None: zero; at least one given, all with the same ndir <= 8) give the
        tangents named in `want` (of dx, dy, dz, dobj), [ndir, B, .], with one factorization per
        instance for all directions and `refine` rounds of iterative refinement each.  out, status,
        the validity and the streams are BatchQP.adjoint's; changes no state."""
        o = out if out is not None else getattr(self, "_last", None)
        if o is None:
            raise MPCQPError("mpcqp_tangent: tangent before any solve")
        st = o.status if status is None else status
        if st.dtype != torch.int32 or tuple(st.shape) != (self.B,) or not st.is_cuda or \
                not st.is_contiguous():
            raise ValueError(f"status must be a contiguous int32 device tensor of shape ({self.B},)")
        unknown = [w for w in want if w not in self.TANGENT_OUTPUTS]
        if unknown:
            raise ValueError(f"unknown tangent outputs {unknown}: choose from {self.TANGENT_OUTPUTS}")
        width = dict(dq=self.n, dl=self.m, du=self.m, dAx=self.nnzA, dPx=self.nnzP)
        d, ndir = {}, None
        for k, t in dict(dq=dq, dl=dl, du=du, dAx=dAx, dPx=dPx).items():
            if t is None:
                d[k] = None
                continue
            t = torch.as_tensor(t, dtype=torch.float64, device=self.device)
            t = t.unsqueeze(0) if t.dim() == 2 else t
            ndir = int(t.shape[0]) if ndir is None else ndir
            if t.dim() != 3 or tuple(t.shape) != (ndir, self.B, width[k]):
                raise ValueError(f"{k} must have shape ({ndir or 'ndir'}, {self.B}, {width[k]}) or "
                                 f"({self.B}, {width[k]})")
            d[k] = t.contiguous()
        if ndir is None:
            raise MPCQPError("mpcqp_tangent: no perturbation given")
        self.stream.wait_stream(torch.cuda.current_stream(self.device))  # the inputs are complete
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            f = dict(dtype=torch.float64, device=self.device)
            shape = dict(dx=(self.n,), dy=(self.m,), dz=(self.m,), dobj=())
            g = {k: torch.empty(ndir, self.B, *shape[k], **f) if k in want else None
                 for k in self.TANGENT_OUTPUTS}
            r = TangentResult(**g, res=torch.empty(ndir, self.B, **f),
                              act=torch.empty(self.B, self.m, dtype=torch.int8, device=self.device),
                              status_tangent=torch.empty(self.B, dtype=torch.int32, device=self.device))
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        tin = _lib.TangentIn(ndir, int(refine), *(ptr(d[k]) for k in ("dq", "dl", "du", "dAx", "dPx")))
        tout = _lib.TangentOut(*(ptr(g[k]) for k in self.TANGENT_OUTPUTS), r.res.data_ptr(),
                               r.act.data_ptr(), r.status_tangent.data_ptr())
        check(_lib.lib().mpcqp_tangent(self._h, st.data_ptr(), o.x.data_ptr(), o.y.data_ptr(),
                                       C.byref(tin), C.byref(tout)), "mpcqp_tangent")
        for t in d.values():
            if t is not None:
                t.record_stream(self.stream)
        if sync:
            self.stream.synchronize()
        else:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return r

    def schedule_info(self):
        v = [C.c_int32() for _ in range(5)]
        check(_lib.lib().mpcqp_schedule_info(self._h, *[C.byref(x) for x in v]),
              "mpcqp_schedule_info")
        k, at = C.c_int32(), C.c_int32()
        check(_lib.lib().mpcqp_engine_kind(self._h, C.byref(k)), "mpcqp_engine_kind")
        check(_lib.lib().mpcqp_schedule_kind(self._h, C.byref(at)), "mpcqp_schedule_kind")
        w = [C.c_int32() for _ in range(4)]
        check(_lib.lib().mpcqp_kernel_info(self._h, *[C.byref(x) for x in w]), "mpcqp_kernel_info")
        return dict(engine="kkt", fac_steps=v[0].value,
                    fwd_steps=v[1].value, bwd_steps=v[2].value, lds_bytes=v[3].value,
                    waves_per_cu=v[4].value, atomics_per_step=at.value,
                    waves_per_instance=w[0].value, instances_per_cu=w[1].value,
                    kernel_regs=w[2].value, kernel_scratch_bytes=w[3].value)

    def dims(self):
        v = [C.c_int32() for _ in range(5)]
        check(_lib.lib().mpcqp_dims(self._h, *[C.byref(x) for x in v]), "mpcqp_dims")
        return dict(n=v[0].value, m=v[1].value, nnzP=v[2].value, nnzA=v[3].value,
                    nnzL=v[4].value)

    def close(self):
        if getattr(self, "_h", None):
            try:
                self.stream.synchronize()
            finally:
                _lib.lib().mpcqp_destroy(self._h)
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def data_buffers(qp: BatchQP):
    """Raw device pointers (ints) of the handle's own Ax / l / u buffers (zero-copy updates)."""
    a, l, u = C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(_lib.lib().mpcqp_data_buffers(qp._h, C.byref(a), C.byref(l), C.byref(u)),
          "mpcqp_data_buffers")
    return a.value, l.value, u.value
