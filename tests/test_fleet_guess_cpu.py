"""CPU: the mission's warm-start kernel (csrc/mmpc_guess.h) built for the host (g++ -DMMPC_EMU -ffp-contract=off, tests/guess_emu)
against the tick kernel's host build and numpy, its gfx950 code object's resource usage, and what the warm start is worth in a
mission: the host builds of the mission and manipulate kernels drive 16 robots on the CPU oracle under both protocols.

Bounds.  The kernel is step 6 of the tick kernel on the same pieces, compiled by the same compiler with the same flags: bitwise.  The
shift is a copy: bitwise against numpy.  The roll-out is checked step by step against the package's f_kinematics on the build's own
previous stage: sin / cos within 2 ulp on either side, <= 4 ulp of max(1, |x_i|), the bound of tests/test_fleet_tick_cpu.py.  In the
mission a warm-started solve and a cold one of the same inputs solve the same NLP to the tolerance 1e-8: their costs agree to
1e-6 max(1, |cost|); the iterates may differ more, in the weakly determined directions of DESIGN section 2 (printed, not bounded)."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import coracle, nlp

import guess_emu_helper as G
import manipulate_emu_helper as H
import mission_emu_helper as MH
import tick_emu_helper as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.1


def _xlim(N):
    return np.asarray(nlp.WholeBodyParams(N=N).xlim, float)


def _phases(B, seed=2):
    """phase codes drawn from {-1, 0, ..., 6}, every one of them at least 8 times"""
    ph = np.random.default_rng(seed).integers(-1, 7, B).astype(np.int32)
    assert np.bincount(ph + 1, minlength=8).min() >= 8
    return ph


@pytest.mark.parametrize("N,M", [(30, 8), (20, 8), (2, 8), (1, 8)])
def test_host_build_against_the_tick_kernels_and_numpy(mm, N, M):
    d = TH.fleet_inputs(B=256, N=N, M=M)
    xlim = _xlim(N)
    t = TH.prepare(N, M, DT, xlim, **d)
    assert not (t["u_guess"] == -7).any() and not (t["x_guess"] == -7).any()
    for reverse in (False, True):
        ug, xg = G.shift(N, DT, d["U_prev"], t["x_in"], reverse=reverse)
        assert np.array_equal(ug, t["u_guess"]) and np.array_equal(xg, t["x_guess"])
        assert np.array_equal(ug, np.concatenate([d["U_prev"][:, 1:], d["U_prev"][:, -1:]], axis=1))
        assert np.array_equal(xg[:, 0], t["x_in"])
        e_roll = TH.rollout_err(mm, DT, ug, xg)
        print("N = %d: roll-out %.2f ulp" % (N, e_roll))
        assert e_roll <= 4.0, e_roll
    if N == 1:
        # the smallest horizon: the one input row is the guess, one plant step, every read clamped to row 0
        assert np.array_equal(ug[:, 0], d["U_prev"][:, 0]) and xg.shape == (256, 2, 9)


def test_phase_mask(mm):
    N, M, B = 20, 3, 256
    d = TH.fleet_inputs(B=B, N=N, M=M)
    x_in = np.clip(d["x"], *_xlim(N))
    ph = _phases(B)
    solved = np.isin(ph, G.SOLVED)
    assert np.array_equal(solved, np.isin(ph, (0, 1, 2, 4))) and np.array_equal(~solved, np.isin(ph, (-1, 3, 5, 6)))
    full_u, full_x = G.shift(N, DT, d["U_prev"], x_in)                    # phase=None: every row
    assert not (full_u == -7).any() and not (full_x == -7).any()
    for reverse in (False, True):
        ug, xg = G.shift(N, DT, d["U_prev"], x_in, ph, reverse=reverse)
        assert (ug[~solved] == -7).all() and (xg[~solved] == -7).all()
        assert np.array_equal(ug[solved], full_u[solved]) and np.array_equal(xg[solved], full_x[solved])
    # nothing of a skipped row is read: NaN rows behind a skipped robot change nothing and stay out of its outputs
    U, xi = d["U_prev"].copy(), x_in.copy()
    U[~solved] = np.nan; xi[~solved] = np.nan
    ug, xg = G.shift(N, DT, U, xi, ph)
    assert (ug[~solved] == -7).all() and (xg[~solved] == -7).all()
    assert np.array_equal(ug[solved], full_u[solved]) and np.array_equal(xg[solved], full_x[solved])


def test_nan_stays_in_its_robot(mm):
    N, M, B = 20, 3, 64
    d = TH.fleet_inputs(B=B, N=N, M=M)
    x_in = np.clip(d["x"], *_xlim(N))
    clean_u, clean_x = G.shift(N, DT, d["U_prev"], x_in)
    U, xi = d["U_prev"].copy(), x_in.copy()
    xi[5, 2] = np.nan; xi[9, 7] = np.inf; U[17, 3, 0] = np.nan; U[30, N - 1, 4] = np.nan
    ug, xg = G.shift(N, DT, U, xi)
    bad = [5, 9, 17, 30]
    rest = np.ones(B, bool); rest[bad] = False
    assert np.array_equal(ug[rest], clean_u[rest]) and np.array_equal(xg[rest], clean_x[rest])
    for b in bad:
        assert not np.isfinite(xg[b]).all(), b
    assert np.isnan(xg[5, -1, 3]) and np.isnan(ug[17, 2, 0]) and np.isnan(ug[30, N - 1, 4]) and np.isnan(ug[30, N - 2, 4])


def test_guess_kernel_uses_no_scratch_and_no_lds_on_gfx950(mm):
    """The kernel source cross-compiled for gfx950: the kernel's own resource usage, as the compiler reports it."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    src = os.path.join(ROOT, "tests", "guess_emu", "mmpc_guess_probe.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"Function Name: mmpc_guess_probe_kernel(.*?)LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    assert m, p.stderr[-2000:]
    get = lambda name: int(re.search(re.escape(name) + r": (\d+)", m.group(1)).group(1))
    usage = "VGPRs %d, SGPRs %d, occupancy %d waves/SIMD, scratch %d B/lane, LDS %s B" % (
        get("VGPRs"), get("SGPRs"), get("Occupancy [waves/SIMD]"), get("ScratchSize [bytes/lane]"), m.group(2))
    print(usage)
    assert get("ScratchSize [bytes/lane]") == 0, usage
    assert int(m.group(2)) == 0, usage


# ---- a mission on the oracle ----------------------------------------------------------------------------------------------------
N, M, T = 20, 3, 220
NAMES = {0: "move", 1: "approach", 2: "rotate", 4: "manipulate"}


def _pars():
    """the reference's one controller in the four phases a mission solves in (fleet.py:DeviceFleet._mission_handles)"""
    W5, W500 = np.diag([5., 5, 5, 0, 0, 1, 1, 1, 1]), np.diag([500., 500, 500, 0, 0, 1, 1, 1, 1])
    return {0: nlp.WholeBodyParams(N=N), 1: nlp.WholeBodyParams(N=N, terminal_xy_equality=True),
            2: nlp.WholeBodyParams(N=N, terminal_xy_equality=True, Q=W5, P=W5),
            4: nlp.WholeBodyParams(N=N, terminal_xy_equality=True, Q=W500, P=W500)}


def _mission(F, warm, resolve=False):
    """run_mission(manipulate=...) on the CPU: the host builds of the mission, manipulate and guess kernels, coracle.solve_batch per
    phase.  Returns phase, iters, status (B,T), u0 (B,T,5) and, with `resolve`, the cost of every warm-started solve beside the cost
    of a cold solve of the same inputs."""
    B = F["x0"].shape[0]
    xlim, pars, nplan = _xlim(N), _pars(), int(2 / DT) + 1
    x, tick, phase = F["x0"].copy(), np.zeros(B, np.int64), np.zeros(B, np.int32)
    plan, prev = None, None
    uref = np.zeros((B, N, 5))
    out = dict(phase=np.zeros((B, T), np.int32), iters=np.zeros((B, T), np.int32), status=np.zeros((B, T), np.int32), u0=np.zeros((B, T, 5)),
               pairs=[])
    for t in range(T):
        r = MH.prepare(N, M, DT, xlim, x, tick, phase, prev, F["glob"], F["obs0"], F["vel"])
        m = H.prepare(N, M, DT, xlim, r["x"], r["tick"], r["phase"], F["pose"], nplan, prev, plan, F["obs0"], F["vel"])
        x, tick, phase, plan = m["x"], m["tick"], m["phase"], m["plan"]
        man = phase == H.MANIPULATE
        inp = {k: np.where(man.reshape((B,) + (1,) * (r[k].ndim - 1)), m[k], r[k]) for k in ("x_in", "traj_ref", "obs")}
        ul = prev if prev is not None else np.zeros((B, N, 5))
        if warm and prev is not None:
            ug, xg = G.shift(N, DT, prev, inp["x_in"], phase)
        U = np.zeros((B, N, 5)) if prev is None else prev.copy()
        for p, par in pars.items():
            rows = np.flatnonzero(phase == p)
            if not rows.size:
                continue
            a = (par, inp["x_in"][rows], inp["traj_ref"][rows], uref[rows], ul[rows], inp["obs"][rows])
            if warm and prev is not None:
                o = coracle.solve_batch(*a, X0=xg[rows], U0=ug[rows], mu_init=0.1, max_iter=2000)
                if resolve:
                    c = coracle.solve_batch(*a, max_iter=2000)
                    out["pairs"].append((p, o["cost"], c["cost"], c["status"], np.abs(o["X"] - c["X"]).reshape(rows.size, -1).max(axis=1)))
            else:
                o = coracle.solve_batch(*a, max_iter=2000)
            U[rows] = o["U"]
            out["iters"][rows, t], out["status"][rows, t], out["u0"][rows, t] = o["iters"], o["status"], o["U"][:, 0]
        out["phase"][:, t] = phase
        prev = U
    return out


def test_mission_on_the_oracle(mm):
    F = MH.mission_fleet(mm, 16, N, DT)
    ref, warm = _mission(F, False), _mission(F, True, resolve=True)
    for r in (ref, warm):
        assert (r["phase"][:, -1] == H.MANIP_DONE).all(), r["phase"][:, -1]
        assert (r["status"] == 0).all()
    # tick 0 is the reference protocol's
    for k in ("phase", "iters", "status", "u0"):
        assert np.array_equal(ref[k][:, 0], warm[k][:, 0]), k
    mean = {}
    for name, r in (("reference", ref), ("shifted", warm)):
        solved = np.isin(r["phase"][:, 1:], G.SOLVED)
        it = r["iters"][:, 1:]
        mean[name] = float(it[solved].mean())
        per = {NAMES[p]: round(float(it[r["phase"][:, 1:] == p].mean()), 1) for p in NAMES}
        print("%s: %d solves from tick 1 on, mean iterations %.2f, slowest %d, per phase %s, robots finished at ticks %s" % (
            name, int(solved.sum()), mean[name], int(r["iters"].max()), per, (r["phase"] == H.MANIP_DONE).argmax(axis=1).tolist()))
    assert mean["shifted"] < mean["reference"], mean
    # every warm-started solve against a cold one of the same inputs
    ph = np.concatenate([np.full(c.size, p) for p, c, _, _, _ in warm["pairs"]])
    cw, cc, st, dX = (np.concatenate([q[i] for q in warm["pairs"]]) for i in (1, 2, 3, 4))
    assert cw.size == int(np.isin(warm["phase"][:, 1:], G.SOLVED).sum()) and (st == 0).all()
    rel = np.abs(cw - cc) / np.maximum(1.0, np.abs(cc))
    print("%d warm solves re-solved cold: max |dcost| %.2e (relative to max(1, |cost|): %.2e), max |dX| %.2e; per phase |dcost| %s" % (
        cw.size, np.abs(cw - cc).max(), rel.max(), dX.max(), {NAMES[p]: "%.1e" % np.abs(cw - cc)[ph == p].max() for p in NAMES}))
    assert rel.max() <= 1e-6, rel.max()
