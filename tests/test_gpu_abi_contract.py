"""The C ABI of libmpcqp.so as such (include/mpcqp.h, through ctypes): return codes, the text of
mpcqp_last_error(), and the copy-in / copy-out entry points bit for bit -- what the Python package
and the parity tests take for granted.  Small random structure (n = 83, m = 127: the seed-1 pattern
of test_gpu_random_structures.py), three instances, no solve: every check is about the host side
of the library."""
import ctypes as C

import numpy as np
import pytest
import torch

from mpc_arpo_project_amd import _lib
from mpc_arpo_project_amd.closed_loop import scenario_struct
from mpc_arpo_project_amd.engine import sorted_csc, triu_csc
from test_gpu_random_structures import _random_qp

pytestmark = pytest.mark.gpu

B = 3
E_INVALID, E_UNSUPPORTED, E_NODATA = -1, -3, -4
I32P = C.POINTER(C.c_int32)


def _err():
    return _lib.lib().mpcqp_last_error().decode()


@pytest.fixture(scope="module")
def qp():
    """the structure (kept alive), its analysis, and device data: shared and per-instance cost rows
    and two sets of A values and bounds"""
    P, q, A, Ax, l, u = _random_qp(1, B)
    P, A = triu_csc(P), sorted_csc(A)
    n, m = P.shape[0], A.shape[0]
    assert (n, m) == (83, 127)
    idx = [np.ascontiguousarray(a, dtype=np.int32) for a in (P.indptr, P.indices, A.indptr, A.indices)]
    st = _lib.Structure(n, m, *[a.ctypes.data_as(I32P) for a in idx])
    perm, Lp, Li, stats = _lib.analyze(P, A)
    rng = np.random.default_rng(9)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    d = dict(Px=dev(P.data), q=dev(q), Ax=dev(Ax), l=dev(l), u=dev(u),
             PxB=dev(P.data[None, :] * rng.uniform(0.5, 2.0, (B, 1))),
             qB=dev(rng.standard_normal((B, n))),
             Ax2=dev(rng.standard_normal(Ax.shape)), l2=dev(l - 1.0), u2=dev(u + 1.0))
    return dict(st=st, keep=idx, n=n, m=m, nnzP=int(P.nnz), nnzA=int(A.nnz), perm=perm, Lp=Lp,
                Li=Li, stats=stats, **d)


def _create(qp, batch=B, **settings):
    h = C.c_void_p(0xBAD)  # a failing create with a valid `out` must reset it
    s = _lib.default_settings(**settings)
    rc = _lib.lib().mpcqp_create(C.byref(qp["st"]), C.byref(s), batch, None, C.byref(h))
    return rc, h


@pytest.fixture
def handle(qp):
    rc, h = _create(qp)
    assert rc == 0 and h.value, _err()
    yield h
    torch.cuda.synchronize()
    assert _lib.lib().mpcqp_destroy(h) == 0


def _set_data(h, qp, batched):
    L = _lib.lib()
    fn, Px, q = (L.mpcqp_set_data_batched, qp["PxB"], qp["qB"]) if batched else \
        (L.mpcqp_set_data, qp["Px"], qp["q"])
    rc = fn(h, Px.data_ptr(), q.data_ptr(), qp["Ax"].data_ptr(), qp["l"].data_ptr(),
            qp["u"].data_ptr())
    assert rc == 0, _err()


# ------------------------------------------------------------------------------------ 1. create
def test_create_rejects_invalid_arguments(qp):
    L = _lib.lib()
    rc, _ = _create(qp, batch=0)
    assert rc == E_INVALID and _err()
    s = _lib.default_settings()
    assert L.mpcqp_create(C.byref(qp["st"]), C.byref(s), B, None, None) == E_INVALID
    assert _err()


@pytest.mark.parametrize("case, reason", [("polish", "polish"),
                                          ("scaled_termination", "scaled_termination"),
                                          ("m0", "m == 0")])
def test_create_reports_unsupported(qp, case, reason):
    L = _lib.lib()
    if case == "m0":
        k = qp["keep"]
        st0 = _lib.Structure(qp["n"], 0, *[a.ctypes.data_as(I32P) for a in k])
        h, s = C.c_void_p(0xBAD), _lib.default_settings()
        rc = L.mpcqp_create(C.byref(st0), C.byref(s), B, None, C.byref(h))
    else:
        rc, h = _create(qp, **{case: 1})
    assert rc == E_UNSUPPORTED
    assert h.value is None  # *out == NULL
    assert reason in _err()


def test_destroy_null_and_create_destroy_cycles(qp):
    L = _lib.lib()
    assert L.mpcqp_destroy(None) == 0
    for _ in range(10):
        rc, h = _create(qp)
        assert rc == 0 and h.value, _err()
        assert L.mpcqp_destroy(h) == 0


# ------------------------------------------------------------------- 2. calls before set_data
def test_calls_before_set_data_return_nodata(qp, handle):
    L, h = _lib.lib(), handle
    x = torch.zeros(B * max(qp["nnzP"], qp["nnzA"], qp["m"]), dtype=torch.float64, device="cuda")
    p = x.data_ptr()
    calls = {
        "update_bounds": lambda: L.mpcqp_update_bounds(h, p, p),
        "update_A": lambda: L.mpcqp_update_A(h, p),
        "update_lin_cost": lambda: L.mpcqp_update_lin_cost(h, p),
        "update_lin_cost_batched": lambda: L.mpcqp_update_lin_cost_batched(h, p),
        "update_P": lambda: L.mpcqp_update_P(h, p),
        "update_P_batched": lambda: L.mpcqp_update_P_batched(h, p),
        "warm_start": lambda: L.mpcqp_warm_start(h, p, p),
        "solve": lambda: L.mpcqp_solve(h, p, p, None),
    }
    for name, call in calls.items():
        _create(qp, polish=1)  # another message first: the next one is this call's own
        assert call() == E_NODATA, name
        assert "before set_data" in _err(), (name, _err())


# ---------------------------------------------------------------------------- 3. null arguments
def test_null_arguments_are_invalid(qp, handle):
    L, h = _lib.lib(), handle
    x = torch.zeros(B * max(qp["nnzP"], qp["nnzA"], qp["m"]), dtype=torch.float64, device="cuda")
    p = x.data_ptr()
    entry = {  # entry point -> number of data pointers, all required
        "mpcqp_set_data": 5, "mpcqp_set_data_batched": 5, "mpcqp_update_bounds": 2,
        "mpcqp_update_A": 1, "mpcqp_update_lin_cost": 1, "mpcqp_update_lin_cost_batched": 1,
        "mpcqp_update_P": 1, "mpcqp_update_P_batched": 1, "mpcqp_warm_start": 2,
        "mpcqp_set_state": 5,
    }
    for name, k in entry.items():
        fn = getattr(L, name)
        for null in range(-1, k):  # -1: the handle itself
            args = [None if j == null else p for j in range(k)]
            _create(qp, polish=1)  # another message first: the next one is this call's own
            rc = fn(None if null == -1 else h, *args)
            assert rc == E_INVALID, (name, null)
            assert "null" in _err(), (name, null, _err())
    # the handle-only entry points
    i = C.c_int32()
    for k, call in enumerate((
            lambda: L.mpcqp_solve(None, p, p, None), lambda: L.mpcqp_copy_data(None, p, p, p),
            lambda: L.mpcqp_get_state(None, p, p, p, p, p),
            lambda: L.mpcqp_get_scaling(None, p, p, p),
            lambda: L.mpcqp_set_skip(None, None), lambda: L.mpcqp_set_order(None, None),
            lambda: L.mpcqp_data_buffers(None, None, None, None),
            lambda: L.mpcqp_dims(None, None, None, None, None, None),
            lambda: L.mpcqp_schedule_info(None, None, None, None, None, None),
            lambda: L.mpcqp_kernel_info(None, None, None, None, None),
            lambda: L.mpcqp_schedule_kind(None, C.byref(i)), lambda: L.mpcqp_schedule_kind(h, None),
            lambda: L.mpcqp_engine_kind(None, C.byref(i)), lambda: L.mpcqp_engine_kind(h, None),
            lambda: L.mpcqp_export_symbolic(None, None, None, None))):
        _create(qp, polish=1)
        assert call() == E_INVALID, k
        assert "null" in _err(), (k, _err())


# ------------------------------------------------------------------------------- 4. round trips
def _copy_data(h, qp):
    out = [torch.empty_like(qp[k]) for k in ("Ax", "l", "u")]
    assert _lib.lib().mpcqp_copy_data(h, *[t.data_ptr() for t in out]) == 0, _err()
    torch.cuda.synchronize()
    return out


def _scaling(h, qp):
    Pu = torch.empty(B, qp["nnzP"], dtype=torch.float64, device="cuda")
    qu = torch.empty(B, qp["n"], dtype=torch.float64, device="cuda")
    assert _lib.lib().mpcqp_get_scaling(h, None, Pu.data_ptr(), qu.data_ptr()) == 0, _err()
    torch.cuda.synchronize()
    return Pu, qu


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
def test_round_trips_are_bitwise(qp, handle, batched):
    L, h = _lib.lib(), handle
    _set_data(h, qp, batched)
    for got, key in zip(_copy_data(h, qp), ("Ax", "l", "u")):
        assert torch.equal(got, qp[key]), key
    assert L.mpcqp_update_bounds(h, qp["l2"].data_ptr(), qp["u2"].data_ptr()) == 0, _err()
    assert L.mpcqp_update_A(h, qp["Ax2"].data_ptr()) == 0, _err()
    for got, key in zip(_copy_data(h, qp), ("Ax2", "l2", "u2")):
        assert torch.equal(got, qp[key]), key

    # the set-up cost rows, before any solve: the one row for every instance / each its own
    Pu, qu = _scaling(h, qp)
    assert torch.equal(Pu, qp["PxB"] if batched else qp["Px"].expand(B, -1))
    assert torch.equal(qu, qp["qB"] if batched else qp["q"].expand(B, -1))

    # the warm-start state
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)
    sent = [rnd(B, qp["n"]), rnd(B, qp["m"]), rnd(B, qp["m"]), rnd(B).abs(),
            torch.tensor([1, 0, 2], dtype=torch.int32, device="cuda")]
    assert L.mpcqp_set_state(h, *[t.data_ptr() for t in sent]) == 0, _err()
    got = [torch.empty_like(t) for t in sent]
    assert L.mpcqp_get_state(h, *[t.data_ptr() for t in got]) == 0, _err()
    torch.cuda.synchronize()
    for a, b in zip(got, sent):
        assert torch.equal(a, b)

    # mpcqp_warm_start: x and y stored, every instance marked as holding an unscaled guess
    x, y = rnd(B, qp["n"]), rnd(B, qp["m"])
    assert L.mpcqp_warm_start(h, x.data_ptr(), y.data_ptr()) == 0, _err()
    assert L.mpcqp_get_state(h, *[t.data_ptr() for t in got]) == 0, _err()
    torch.cuda.synchronize()
    assert torch.equal(got[0], x) and torch.equal(got[2], y)
    assert torch.equal(got[1], sent[1]) and torch.equal(got[3], sent[3])  # z and rho kept
    assert got[4].tolist() == [2] * B


def test_update_P_batched_promotes_a_shared_handle(qp, handle):
    """never solved: the new rows are the set-up rows, q becomes a row per instance of the same
    values"""
    L, h = _lib.lib(), handle
    _set_data(h, qp, False)
    assert L.mpcqp_update_P_batched(h, qp["PxB"].data_ptr()) == 0, _err()
    Pu, qu = _scaling(h, qp)
    assert torch.equal(Pu, qp["PxB"])
    assert torch.equal(qu, qp["q"].expand(B, -1))
    # and the per-instance q rows of the promoted handle
    assert L.mpcqp_update_lin_cost_batched(h, qp["qB"].data_ptr()) == 0, _err()
    Pu, qu = _scaling(h, qp)
    assert torch.equal(Pu, qp["PxB"]) and torch.equal(qu, qp["qB"])


def test_data_buffers_are_stable(qp, handle):
    L, h = _lib.lib(), handle
    _set_data(h, qp, False)
    first = [C.c_void_p() for _ in range(3)]
    again = [C.c_void_p() for _ in range(3)]
    assert L.mpcqp_data_buffers(h, *[C.byref(v) for v in first]) == 0
    assert L.mpcqp_data_buffers(h, *[C.byref(v) for v in again]) == 0
    assert all(v.value for v in first) and len({v.value for v in first}) == 3
    assert [v.value for v in first] == [v.value for v in again]


def test_dims_and_schedule_agree_with_analyze(qp, handle):
    L, h = _lib.lib(), handle
    v = [C.c_int32() for _ in range(5)]
    assert L.mpcqp_dims(h, *[C.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [qp["n"], qp["m"], qp["nnzP"], qp["nnzA"], len(qp["Li"])]
    st = qp["stats"]
    assert L.mpcqp_schedule_info(h, *[C.byref(x) for x in v]) == 0
    fac, fwd, bwd, lds, wpc = [x.value for x in v]
    assert (fac, fwd, bwd) == (st["fac_steps"], st["fwd_steps"], st["bwd_steps"])
    assert lds == (st["lds_image_bytes"] + 15) // 16 * 16  # the image, 16-byte aligned
    w = [C.c_int32() for _ in range(4)]
    assert L.mpcqp_kernel_info(h, *[C.byref(x) for x in w]) == 0
    waves, per_cu, regs, scratch = [x.value for x in w]
    assert waves == 1  # the automatic choice at this size
    assert per_cu >= 1 and wpc == waves * per_cu
    assert 0 < regs <= 512 and scratch >= 0
    nk = qp["n"] + qp["m"]
    perm, Lp = np.empty(nk, dtype=np.int32), np.empty(nk + 1, dtype=np.int32)
    Li = np.empty(len(qp["Li"]), dtype=np.int32)
    assert L.mpcqp_export_symbolic(h, *[a.ctypes.data_as(I32P) for a in (perm, Lp, Li)]) == 0
    assert np.array_equal(perm, qp["perm"]) and np.array_equal(Lp, qp["Lp"])
    assert np.array_equal(Li, qp["Li"])


# ----------------------------------------------------------------------- 5. closed loop and UKF
def test_closed_loop_and_ukf_errors_name_their_entry_point(prob20):
    L = _lib.lib()
    sc, keep = scenario_struct(prob20)
    cl = C.c_void_p()
    rc_create = L.mpcqp_cl_create(C.byref(sc), 0, None, C.byref(cl))
    msg_create = _err()
    assert L.mpcqp_cl_create(C.byref(sc), B, None, C.byref(cl)) == 0 and cl.value
    x = torch.zeros(B * max(prob20.nnzA, prob20.m), dtype=torch.float64, device="cuda")
    p = x.data_ptr()
    rc_conf = L.mpcqp_cl_configure(cl, None, p, p, p)
    msg_conf = _err()
    assert L.mpcqp_cl_destroy(cl) == 0

    um = _lib.UkfModel()
    um.alpha, um.beta, um.kappa = 1.0, 2.0, 0.0
    k = C.c_void_p()
    assert L.mpcqp_ukf_create(C.byref(um), B, None, C.byref(k)) == 0 and k.value
    rc_ukf = L.mpcqp_ukf_step(k, None, p, p, p, None, None)
    msg_ukf = _err()
    assert L.mpcqp_ukf_destroy(k) == 0

    assert (rc_create, rc_conf, rc_ukf) == (-1, -1, -1)
    # the message is the failing call's own, not the previous failure's
    assert msg_create.startswith("mpcqp_cl_create"), msg_create
    assert msg_conf.startswith("mpcqp_cl_configure"), msg_conf
    assert msg_ukf.startswith("mpcqp_ukf_step"), msg_ukf
