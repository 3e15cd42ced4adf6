"""Generates tests/golden/cl_scripted.npz.  CONTAINER-ONLY: needs /root/reference (never on the
GPU box) and is never imported by a test.

The reference's OWN `src.trajectorySimulate.trajectorySimulate` runs unmodified, with the stubs of
gen_fixtures.py for the absent third-party modules, except that `osqp.OSQP` is a scripted stand-in
(tests/closed_loop_ref.py: ScriptedOSQP): its k-th solve returns a prescribed status and an x that
is zero except for a prescribed first input, and it records every (Ax, l, u) update.  With failed
solves scripted in, the loop leaves the MPC branch and runs its two fallback controllers -- the
LQR failsafe (2) and the deadbeat debris avoidance (3) -- with the integrator carried between
them, the input-norm clip on most steps, from starts in every region around the debris box, for
the radial (isReject=True) and the in-track (isReject=False) scenario, Nx = 20, 40 steps.

Stored per run (arrays only, padded with zeros from i_term on): x0, the status and input scripts,
ctrlr_seq, x_true_pcw, ctrl_hist, x_est, i_term, isSuccess, per step the three varying Ax values
(C1, C2, -slope; the generator checks that they rebuild the recorded Ax exactly) and the full
l / u; the full Ax of one run per family; and xintf, the controller integrator after each step,
replayed by the project's pinned host controller on the reference's recorded estimates (the
reference does not return it; the replay is accepted only if it reproduces the reference's
recorded inputs bit for bit).

`python gen_scripted_loops.py` writes the file; with `--check` it only compares a fresh run with
the committed file, array by array.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gen_fixtures as G  # noqa: E402
import gen_fixtures_loops as GL  # noqa: E402
import closed_loop_ref as R  # noqa: E402
from mpc_arpo_project_amd import qp_model  # noqa: E402

OUT = os.path.join(HERE, "cl_scripted.npz")

# (family, x0, what the start is there for)
RUNS = [
    (R.FAMILY_RADIAL, (41., 1., 0., 0.), "inside the box, y > 0"),
    (R.FAMILY_RADIAL, (39., -2., 0.01, -0.01), "inside the box, y < 0"),
    (R.FAMILY_RADIAL, (40., 2.6, 0., 0.), "just above the box: in_box fails on the y test only"),
    (R.FAMILY_RADIAL, (40.5, -2.55, 0., 0.), "just below the box"),
    (R.FAMILY_RADIAL, (50., 3., 0., 0.), "near band"),
    (R.FAMILY_RADIAL, (100., 10., 0., 0.), "far"),
    (R.FAMILY_RADIAL, (2.8, 0.1, -0.05, 0.), "terminates inside the 40 steps"),
    (R.FAMILY_RADIAL, (37.3, -1., 0.4, 0.), "enters the box under the failsafe: 2 -> 3"),
    (R.FAMILY_IN_TRACK, (41., 4., 0., 0.), "in-track"),
    (R.FAMILY_IN_TRACK, (1., 41., 0., 0.), "in-track, inside the box before the swap"),
    (R.FAMILY_IN_TRACK, (-10., 100., 0., 0.), "in-track, the evaluation script's start"),
]
FULL_AX_RUNS = (0, 8)


def main():
    G.install_stubs()
    import osqp  # the stub module
    import src.mpcsim as RM
    from src.trajectorySimulate import trajectorySimulate

    nsim = 40
    u0 = (R.NX_SCRIPTED + 1) * 4
    per_run = []
    for r, (fam, x0, what) in enumerate(RUNS):
        st, uin = R.scripts(seed=100 + r, nsim=nsim)
        if fam == R.FAMILY_RADIAL:
            sim, mpc, fail, deb = G.ref_objects(RM, R.NX_SCRIPTED, False, isReject=True, x0=x0)
        else:
            sim, mpc, fail, deb = GL.ref_objects_in_track(RM, Nx=R.NX_SCRIPTED)
            sim.x0 = np.array(x0)
        sim.T_final = R.T_FINAL_SCRIPTED
        factory = R.scripted_factory(st, uin, u0)
        osqp.OSQP = factory
        run = trajectorySimulate(sim, mpc, fail, deb)
        solver = factory.made[-1]
        psim, pmpc, pfail, pdeb = R.scripted_scenario(fam, x0)
        prob = qp_model.build_problem(psim, pmpc, pfail, pdeb)
        d = R.run_arrays(run, solver, prob, nsim)
        it = int(run.i_term)
        xi, raw, seq, ctrl = R.replay_controller(prob, psim, pdeb, st, uin, d["x_est"], it)
        assert np.array_equal(seq, run.ctrlr_seq), r
        assert np.array_equal(ctrl, d["ctrl_hist"][:, 1:it + 1]), r  # the replay is the reference's
        d["xintf"] = np.zeros(nsim)
        d["xintf"][:it] = xi
        d.update(x0=np.array(x0), family=np.array(fam), status_script=st, input_script=uin,
                 clipped=np.r_[raw > prob.umax[0], np.zeros(nsim - it, bool)])
        per_run.append(d)
        print(f"run {r} ({what}): i_term {it} success {bool(run.isSuccess)} controllers "
              f"{[int(np.sum(seq == c)) for c in (1, 2, 3)]} clipped {int(np.sum(raw > 0.2))}")

    out = {k: np.array([d[k] for d in per_run]) for k in per_run[0] if k != "full_Ax"}
    for r in FULL_AX_RUNS:
        out[f"full_Ax_run{r}"] = per_run[r]["full_Ax"]

    # ---- what the fixture must contain, counted on the reference's own output
    rad = [d for d in per_run if int(d["family"]) == R.FAMILY_RADIAL]
    seqs = [d["ctrlr_seq"][:int(d["i_term"])] for d in rad]
    counts = {c: int(sum(np.sum(s == c) for s in seqs)) for c in (1, 2, 3)}
    clipped = int(sum(np.sum(d["clipped"][:int(d["i_term"])]) for d in rad))
    steps = int(sum(int(d["i_term"]) for d in rad))
    t32 = t23 = 0
    for d in rad:
        s, xi = d["ctrlr_seq"], d["xintf"]
        for i in range(1, int(d["i_term"])):
            t32 += int(s[i - 1] == 3 and s[i] == 2 and xi[i - 1] != 0)
            t23 += int(s[i - 1] == 2 and s[i] == 3 and xi[i - 1] != 0)
    print(f"radial runs: steps per controller {counts}, clipped {clipped} / not clipped "
          f"{steps - clipped}, transitions with a carried integrator 3->2: {t32}, 2->3: {t23}")
    assert min(counts.values()) >= 20, counts
    assert clipped > 0 and steps - clipped > 0
    assert t32 >= 1 and t23 >= 1
    assert any(int(d["i_term"]) < nsim for d in per_run)
    for d in per_run:
        if int(d["family"]) == R.FAMILY_IN_TRACK:
            print("in-track run", d["x0"], "controllers",
                  np.unique(d["ctrlr_seq"][:int(d["i_term"])], return_counts=True))

    if os.path.exists(OUT):
        old = dict(np.load(OUT, allow_pickle=False))
        same = set(old) == set(out) and all(np.array_equal(old[k], out[k]) for k in out)
        print("committed fixture:", "identical, array by array" if same else "DIFFERS")
        if "--check" in sys.argv:
            sys.exit(0 if same else 1)
    if "--check" not in sys.argv:
        np.savez_compressed(OUT, **out)
        print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
