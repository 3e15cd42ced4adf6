"""Per-instance cost data (P, q) in one batch, and P updates (GPU).

One handle hosts a mix of cost-weight sets of one scenario family (mpcqp_set_data_batched,
mpcqp_update_lin_cost_batched, mpcqp_update_P[_batched]).  The per-instance path adds no arithmetic:
it addresses another set-up row.  So parity is carried by a BITWISE comparison with the shared-cost
path (already pinned to the oracle), at a batch in which every wave solves several instances in
turn -- where a set-up pointer hoisted out of the instance loop, or indexed by a lane value, would
read another instance's row -- plus an independent check against the oracle per weight set.

Weight sets are (q_scale, r_scale, rs_scale) multipliers of the radial scenario's Q_state, R_input,
R_slack; states are scenarios.sample_estimates(K, seed=7) at rest; horizons (Nx = 20, accel) for the
one-wave kernel and (Nx = 40, delta-v) for the two-wave kernel.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as orc
from mpc_arpo_project_amd import qp_model, scenarios
from mpc_arpo_project_amd.engine import BatchQP, triu_csc
from mpc_arpo_project_amd.osqp_compat import OSQP
from test_cost_variants_host import HORIZONS, SETS, weighted_problem

pytestmark = pytest.mark.gpu
FAST = 1000  # iterations: below this the engine and the oracle agree exactly (test_gpu_scale_parity)
THREADS = min(16, len(os.sched_getaffinity(0)))
EPS = dict(eps_abs=1e-3, eps_rel=1e-3)


def states(K):
    X = scenarios.sample_estimates(K, seed=7)
    X[:, 2:] = 0.0  # at rest, no disturbance estimate
    return X


def family(Nx, dv, sets):
    probs = [weighted_problem(Nx, dv, w) for w in sets]
    Px, q, _ = qp_model.cost_variants(probs)
    return probs, Px, q


def outputs(qp, r):
    """everything a solve leaves behind, as host arrays: results, warm state and data scaling"""
    qp.stream.synchronize()
    o = {k: getattr(r, k).cpu().numpy().copy() for k in ("x", "y", "status", "iter", "rho")}
    o.update({"state_" + k: v.cpu().numpy() for k, v in qp.get_state().items()})
    o.update({k: v.cpu().numpy() for k, v in qp.get_scaling().items()})
    return o


def assert_same(a, b, what, rows=None):
    for k in a:
        got = a[k] if rows is None else a[k][rows]
        assert np.array_equal(got, b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("Nx,dv", HORIZONS)
def test_mixed_batch_equals_the_shared_path_bitwise(Nx, dv):
    """B = 8,192 = 2,048 states x 4 weight sets (instance 4 s + v: state s, set v), several
    instances per wave: a cold solve, a solve after a bounds-only update (which re-reads the
    instance's set-up row) and three after update(l, u, Ax) give, set by set, bit for bit what a
    shared-cost handle gives on the same 2,048 states with that set's P and q"""
    K, V = 2048, 4
    probs, Px, q = family(Nx, dv, SETS[:V])
    X = states(K)
    # data of step k: every instance moves on to another sampled state
    data = [[qp_model.configure_batch(p, np.roll(X, k, axis=0)) for p in probs] for k in range(4)]

    def run(batch, step_data, **cost):
        qp = BatchQP(probs[0].P, probs[0].A, batch=batch, **EPS)
        Ax, l, u = step_data(0)
        qp.set_data(Ax=Ax, l=l, u=u, **cost)
        outs = [outputs(qp, qp.solve())]
        _, l, u = step_data(1)
        qp.update(l=l, u=u)
        outs.append(outputs(qp, qp.solve()))
        for k in (1, 2, 3):
            Ax, l, u = step_data(k)
            qp.update(l=l, u=u, Ax=Ax)
            outs.append(outputs(qp, qp.solve()))
        info = qp.schedule_info()
        qp.close()
        return outs, info

    def mixed(k):  # row 4 s + v <- set v's data of state s
        return [np.stack([data[k][v][j] for v in range(V)], axis=1).reshape(K * V, -1)
                for j in range(3)]

    variant = np.tile(np.arange(V), K)
    got, info = run(K * V, mixed, Px=Px[variant], q=q[variant])
    per_wave = K * V / (info["instances_per_cu"] * 256)
    assert per_wave >= 4, info  # several instances per wave (the grid is one wave-set per CU slot)
    for v in range(V):
        ref, _ = run(K, lambda k: data[k][v], Px=Px[v], q=q[v])
        for step, (a, b) in enumerate(zip(got, ref)):
            assert_same(a, b, (v, step), rows=slice(v, None, V))
        # the solves did something: not every instance of the set ends in one state
        assert len(np.unique(ref[-1]["iter"])) > 1 and (ref[0]["status"] == 1).any()
    # and the weight sets are told apart: sets differ on the same states
    assert any(not np.array_equal(got[0]["x"][0::V], got[0]["x"][v::V], equal_nan=True)
               for v in range(1, V))


@pytest.mark.parametrize("Nx,dv", HORIZONS)
def test_mixed_batch_against_the_oracle(Nx, dv):
    """6 weight sets x 16 states in one handle against the CPU oracle, set by set: wherever the
    oracle needs at most FAST iterations, status and iteration count are equal"""
    K, V = 16, len(SETS)
    probs, Px, q = family(Nx, dv, SETS)
    X = states(K)
    data = [qp_model.configure_batch(p, X) for p in probs]  # row v K + s: set v, state s
    Ax, l, u = (np.concatenate([d[j] for d in data]) for j in range(3))
    variant = np.repeat(np.arange(V), K)
    qp = BatchQP(probs[0].P, probs[0].A, batch=K * V, **EPS)
    qp.set_data(Px=Px[variant], q=q[variant], Ax=Ax, l=l, u=u)
    r = qp.solve()
    st, it, xg = r.status.cpu().numpy(), r.iter.cpu().numpy(), r.x.cpu().numpy()
    qp.close()
    du_max = 0.0
    for v, p in enumerate(probs):
        rows = slice(v * K, (v + 1) * K)
        xo, _, so, io = orc.batch_solve(p.P, p.q, p.A, *data[v], nthreads=THREADS, **EPS)
        fast = io <= FAST
        ok = fast & (so == 1)
        du = float(np.abs(xg[rows][ok][:, p.u0_slice] - xo[ok][:, p.u0_slice]).max()) if ok.any() else 0.0
        du_max = max(du_max, du)
        print(f"Nx {Nx} set {SETS[v]}: fast {int(fast.sum())}/16, solved {int(ok.sum())}, "
              f"max |du0| (fast, solved) {du:.3e}")
        assert fast.sum() >= 10, (SETS[v], io)
        assert np.array_equal(st[rows][fast], so[fast]), (SETS[v], st[rows], so)
        assert np.array_equal(it[rows][fast], io[fast]), (SETS[v], it[rows], io)
    print(f"Nx {Nx}: max |du0| over the fast solved instances of all sets {du_max:.3e}")


@pytest.mark.parametrize("Nx,dv", HORIZONS)
def test_update_P_with_the_unscaled_P_is_an_update_of_A(Nx, dv):
    """osqp_update_P maps onto the drift machinery of osqp_update_A: writing back the very P the
    next rescaling would start from (get_scaling's Pu) gives, bit for bit, the solve, warm state
    and scaling that follow an update of A with unchanged values.  B = 64: 16 states x 4 sets."""
    K, V = 16, 4
    probs, Px, q = family(Nx, dv, SETS[:V])
    X = states(K)
    data = [qp_model.configure_batch(p, X) for p in probs]
    Ax, l, u = (np.concatenate([d[j] for d in data]) for j in range(3))
    variant = np.repeat(np.arange(V), K)

    def handle():
        qp = BatchQP(probs[0].P, probs[0].A, batch=K * V, **EPS)
        qp.set_data(Px=Px[variant], q=q[variant], Ax=Ax, l=l, u=u)
        return qp

    a, b = handle(), handle()
    first = outputs(a, a.solve())
    assert_same(outputs(b, b.solve()), first, "first solve")
    a.update(Ax=Ax)
    b.update(Px=b.get_scaling()["Pu"])
    second = outputs(a, a.solve())
    assert_same(outputs(b, b.solve()), second, "second solve")
    assert not np.array_equal(first["iter"], second["iter"])  # a warm solve, not a repeat
    a.close(), b.close()


@pytest.mark.parametrize("Nx,dv", HORIZONS)
def test_update_P_before_the_first_solve_is_set_data(Nx, dv):
    K, V = 16, 4
    probs, Px, q = family(Nx, dv, SETS[:V])
    X = states(K)
    data = [qp_model.configure_batch(p, X) for p in probs]
    Ax, l, u = (np.concatenate([d[j] for d in data]) for j in range(3))
    variant = np.repeat(np.arange(V), K)
    other = (variant + 1) % V

    def solve(setup, update=None):
        qp = BatchQP(probs[0].P, probs[0].A, batch=K * V, **EPS)
        qp.set_data(Ax=Ax, l=l, u=u, **setup)
        if update:
            qp.update(**update)
        o = outputs(qp, qp.solve())
        qp.close()
        return o

    # per instance over per instance; per instance over shared (the handle is promoted); shared
    # over shared; shared over per instance
    want = solve(dict(Px=Px[other], q=q[other]))
    assert_same(solve(dict(Px=Px[variant], q=q[variant]), dict(Px=Px[other], q=q[other])), want, "b/b")
    assert_same(solve(dict(Px=Px[0], q=q[0]), dict(Px=Px[other], q=q[other])), want, "b/s")
    assert not np.array_equal(want["x"], solve(dict(Px=Px[variant], q=q[variant]))["x"], equal_nan=True)
    want = solve(dict(Px=Px[2], q=q[2]))
    assert_same(solve(dict(Px=Px[0], q=q[0]), dict(Px=Px[2], q=q[2])), want, "s/s")
    assert_same(solve(dict(Px=Px[variant], q=q[variant]), dict(Px=Px[2], q=q[2])), want, "s/b")


@pytest.mark.parametrize("Nx,dv", HORIZONS)
def test_update_P_to_new_values_solves_the_new_problem(Nx, dv):
    """solve with the set (1, 1, 1), update P and q per instance to the set (4, 1, 1), solve again:
    every instance that reports `solved` reports the residuals of the NEW problem at the returned
    point, and they meet OSQP's termination test at eps = 1e-3,
        |A x - z|     <= eps + eps max(|A x|, |z|),
        |P x + q + A'y| <= eps + eps max(|P x|, |A'y|, |q|)        (all norms inf, unscaled),
    with P, q of the new set (z: the handle's scaled state, unscaled by its E).  A solve that had
    kept the old P would report, and stop on, a dual residual whose state block is 4 times off."""
    K = 16
    probs, Px, q = family(Nx, dv, (SETS[0], SETS[2]))
    X = states(K)
    Ax, l, u = qp_model.configure_batch(probs[0], X)
    qp = BatchQP(probs[0].P, probs[0].A, batch=K, **EPS)
    qp.set_data(Px=Px[0], q=q[0], Ax=Ax, l=l, u=u)
    qp.solve()
    qp.update(q=np.tile(q[1], (K, 1)), Px=np.tile(Px[1], (K, 1)))
    r = qp.solve()
    st = r.status.cpu().numpy()
    x, y = r.x.cpu().numpy(), r.y.cpu().numpy()
    pri, dua = r.pri_res.cpu().numpy(), r.dua_res.cpu().numpy()
    z = (qp.get_state()["z"] / qp.get_scaling()["E"]).cpu().numpy()
    qp.close()
    solved = np.flatnonzero(st == 1)
    P1 = sp.csc_matrix(probs[1].P)
    P1 = sp.triu(P1) + sp.triu(P1, 1).T  # full symmetric
    eps, rows = 1e-3, []
    for i in solved:
        A = sp.csc_matrix((Ax[i], probs[0].A.indices, probs[0].A.indptr), shape=probs[0].A.shape)
        Axx, Px_, Aty = A @ x[i], P1 @ x[i], A.T @ y[i]
        p_host = np.abs(Axx - z[i]).max()
        d_host = np.abs(Px_ + q[1] + Aty).max()
        ep = eps + eps * max(np.abs(Axx).max(), np.abs(z[i]).max())
        ed = eps + eps * max(np.abs(Px_).max(), np.abs(Aty).max(), np.abs(q[1]).max())
        rows.append((i, p_host, d_host, ep, ed))
        print(f"Nx {Nx} instance {i}: pri {pri[i]:.6e} (host {p_host:.6e}, bound {ep:.3e}), "
              f"dua {dua[i]:.6e} (host {d_host:.6e}, bound {ed:.3e}), relative difference "
              f"{abs(p_host - pri[i]) / pri[i]:.1e} {abs(d_host - dua[i]) / dua[i]:.1e}")
    print(f"Nx {Nx}: solved {len(solved)}/16")
    assert len(solved) >= 8, st
    for i, p_host, d_host, ep, ed in rows:
        assert abs(p_host - pri[i]) <= 1e-9 * pri[i], (i, p_host, pri[i])
        assert abs(d_host - dua[i]) <= 1e-9 * dua[i], (i, d_host, dua[i])
        # the recomputed residuals agree to 1e-9 relative: the same slack on the test they passed
        assert p_host <= ep * (1 + 1e-9) and d_host <= ed * (1 + 1e-9), (i, p_host, ep, d_host, ed)


def test_osqp_drop_in_updates_P():
    """osqp.OSQP.update(Px=..., Px_idx=...) as the drop-in: before the first solve it is, bit for
    bit, a setup with the merged P; bad lengths raise ValueError as osqp's do"""
    p0, p1 = weighted_problem(20, False), weighted_problem(20, False, SETS[2])
    X = states(1)
    Ax, l, u = qp_model.configure_batch(p0, X)
    A = sp.csc_matrix((Ax[0], p0.A.indices, p0.A.indptr), shape=p0.A.shape)
    T0, T1 = triu_csc(p0.P), triu_csc(p1.P)
    # indexed update: the stage costs of the first 10 stages only (diagonal entries: the merged P
    # stays positive semidefinite)
    cols = np.repeat(np.arange(p0.n), np.diff(T0.indptr))
    idx = np.flatnonzero((T0.data != T1.data) & (cols < 40))
    assert 0 < len(idx) < np.count_nonzero(T0.data != T1.data)
    merged = T0.copy()
    merged.data[idx] = T1.data[idx]

    def run(P, **upd):
        o = OSQP()
        o.setup(P, p0.q, A, l[0], u[0], **EPS)
        if upd:
            o.update(**upd)
        r = o.solve()
        return r.x, r.y, r.info.iter, r.info.status_val, o

    full = run(p0.P, Px=T1.data)
    fresh = run(T1)
    part = run(p0.P, Px=T1.data[idx], Px_idx=idx)
    fresh_part = run(merged)
    for got, want in ((full, fresh), (part, fresh_part)):
        assert got[3] == want[3] == 1 and got[2] == want[2]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(full[0], part[0]) and not np.array_equal(full[0], run(p0.P)[0])
    # a second, indexed update merges into the object's own copy of P: the rest of set (4, 1, 1)
    o = part[4]
    rest = np.flatnonzero(merged.data != T1.data)
    o.update(Px=T1.data[rest], Px_idx=rest)
    assert np.array_equal(o._Px, T1.data)
    assert o.solve().info.status_val == 1
    for bad in (dict(Px=T1.data[:-1]), dict(Px=np.r_[T1.data, 1.0]),
                dict(Px=T1.data[idx][:-1], Px_idx=idx), dict(Px=T1.data[idx], Px_idx=idx[:-1])):
        with pytest.raises(ValueError):
            o.update(**bad)
