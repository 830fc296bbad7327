"""CPU: the fleet tick kernel (csrc/mmpc_tick.h) built for the host (g++ -DMMPC_EMU -ffp-contract=off, tests/tick_emu) against
the numpy definitions it replaces, and its gfx950 code object's resource usage.

Bounds.  Gather, obstacle table, tick counter, shift and clip consist of copies and of correctly rounded IEEE operations in the
same order on both sides: bitwise.  The plant step differs in sin / cos alone (mmpc_sincos: within 2 ulp of a number <= 1, numpy's
libm likewise), which enters multiplied by dt |dV| <= 0.1 |u|, so it moves a component by at most a couple of representable
numbers: <= 4 ulp of max(1, |x_i|).  The roll-out is checked step by step against the build's own previous stage, which keeps that
bound free of the error growth over N steps."""
import os
import re
import subprocess

import numpy as np

from oracle import nlp

import tick_emu_helper as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, DT = 30, 8, 0.1


def _xlim():
    return np.asarray(nlp.WholeBodyParams(N=N).xlim, float)


def test_host_build_against_numpy_definitions(mm):
    d = H.fleet_inputs()
    xlim = _xlim()
    B = d["x"].shape[0]
    ref = H.reference(mm, xlim, DT, N, **d)
    # the reference's index is unambiguous: the two smallest plan distances of EVERY robot differ by far more than the last-bit
    # differences of the advanced state can move them
    two = np.sort(ref["dist"], axis=1)[:, :2]
    gap = float((two[:, 1] - two[:, 0]).min())
    assert gap > 1e-9, gap
    assert ref["start"].min() == 0 and ref["start"].max() == 50 and (ref["start"] > 50 - N).any()     # the padded tail is covered
    for reverse in (False, True):
        r = H.prepare(N, M, DT, xlim, reverse=reverse, **d)
        assert np.array_equal(r["start"], ref["start"])
        assert np.array_equal(r["traj_ref"], ref["traj_ref"])
        assert np.array_equal(r["obs"], ref["obs"])
        assert np.array_equal(r["tick"], d["tick"] + 1)
        assert np.array_equal(r["u_guess"], ref["u_guess"])
        assert np.array_equal(r["x_in"], np.clip(r["x"], xlim[0], xlim[1]))
        assert np.array_equal(r["x_guess"][:, 0], r["x_in"])
        e_adv = float(H.ulp_err(r["x"], ref["x"]).max())
        e_roll = H.rollout_err(mm, DT, r["u_guess"], r["x_guess"])
        print("advance %.2f ulp, roll-out %.2f ulp, gap %.3g" % (e_adv, e_roll, gap))
        assert e_adv <= 4.0, e_adv
        assert e_roll <= 4.0, e_roll


def test_states_outside_the_limits_are_stepped_from_their_clip(mm):
    """The issue's draw stays inside xlim; here velocities and joints leave it on both sides, so that the clip before the plant
    step and the one of x_in both change values."""
    d = H.fleet_inputs(B=256)
    xlim = _xlim()
    d["x"][:, 3:6] *= 2.5
    d["x"][:, 6:] += np.random.default_rng(11).uniform(-2, 2, (256, 3))
    assert (d["x"] < xlim[0]).any() and (d["x"] > xlim[1]).any()
    ref = H.reference(mm, xlim, DT, N, **d)
    r = H.prepare(N, M, DT, xlim, **d)
    assert (r["x_in"] != r["x"]).any()
    assert np.array_equal(r["x_in"], np.clip(r["x"], xlim[0], xlim[1])) and np.array_equal(r["x_guess"][:, 0], r["x_in"])
    assert float(H.ulp_err(r["x"], ref["x"]).max()) <= 4.0
    assert H.rollout_err(mm, DT, r["u_guess"], r["x_guess"]) <= 4.0


def test_null_pointer_combinations_on_the_host(mm):
    d = H.fleet_inputs(B=64)
    xlim = _xlim()
    full = H.prepare(N, M, DT, xlim, **d)
    # advance only: the plain plant step after the last tick
    a = H.prepare(N, M, DT, xlim, d["x"], d["tick"], U_prev=d["U_prev"], want=())
    assert np.array_equal(a["x"], full["x"]) and np.array_equal(a["tick"], full["tick"])
    # prepare only (before the first tick): x and tick untouched, inputs from the state as it is
    p = H.prepare(N, M, DT, xlim, d["x"], d["tick"], None, d["glob"], d["obs0"], d["vel"])
    ref = H.reference(mm, xlim, DT, N, d["x"], d["tick"], None, d["glob"], d["obs0"], d["vel"])
    assert np.array_equal(p["x"], d["x"]) and np.array_equal(p["tick"], d["tick"])
    assert np.array_equal(p["x_in"], np.clip(d["x"], xlim[0], xlim[1]))
    assert np.array_equal(p["start"], ref["start"]) and np.array_equal(p["traj_ref"], ref["traj_ref"]) and np.array_equal(p["obs"], ref["obs"])
    assert (p["u_guess"] == -7).all() and (p["x_guess"] == -7).all()           # no previous optimum: no warm start
    # no warm-start outputs
    w = H.prepare(N, M, DT, xlim, want=("x_in", "traj_ref", "start", "obs"), **d)
    for k in ("x", "tick", "x_in", "traj_ref", "start", "obs"):
        assert np.array_equal(w[k], full[k]), k


def test_ties_padding_and_single_row_plans(mm):
    """Exact ties by construction: a plan on x = 0, 0.25, 0.5, ... and robots exactly half way between two rows (all values
    representable) take the lower row; a robot beyond the last row gets N + 1 copies of it; a plan of one row."""
    xlim = _xlim()
    ng = 80                                                  # more rows than lanes: ties within a lane's rows and across lanes
    plan = np.zeros((ng, 9)); plan[:, 0] = 0.25 * np.arange(ng); plan[:, 5] = np.arange(ng)
    lower = np.array([0, 1, 30, 62, 63, 64, 70, 78])
    B = lower.size + 2
    x = np.zeros((B, 9))
    x[:lower.size, 0] = 0.25 * lower + 0.125
    x[lower.size] = [100.0, 3.0, 0, 0, 0, 0, 0, 0, 0]        # beyond the last row
    x[lower.size + 1] = [-5.0, 0.0, 0, 0, 0, 0, 0, 0, 0]      # before the first
    glob = np.ascontiguousarray(np.repeat(plan[None], B, axis=0))
    tick = np.zeros(B, np.int64)
    obs0 = np.zeros((B, M, 3)); vel = np.zeros((B, M, 2))
    for reverse in (False, True):
        r = H.prepare(N, M, DT, xlim, x, tick, None, glob, obs0, vel, reverse=reverse)
        assert np.array_equal(r["start"], np.concatenate([lower, [ng - 1, 0]]))
        assert np.array_equal(r["traj_ref"][lower.size], np.repeat(plan[-1:], N + 1, axis=0))
        idx = np.minimum(r["start"][:, None] + np.arange(N + 1)[None, :], ng - 1)
        assert np.array_equal(r["traj_ref"], plan[idx])
        one = H.prepare(N, M, DT, xlim, x, tick, None, glob[:, 17:18].copy(), obs0, vel, reverse=reverse)
        assert (one["start"] == 0).all() and np.array_equal(one["traj_ref"], np.repeat(glob[:, 17:18], N + 1, axis=1))


def test_non_finite_state_takes_row_zero_and_stays_local(mm):
    d = H.fleet_inputs(B=64)
    xlim = _xlim()
    clean = H.prepare(N, M, DT, xlim, **d)
    x = d["x"].copy(); x[5, 0] = np.nan; x[9, 4] = np.inf
    r = H.prepare(N, M, DT, xlim, **dict(d, x=x))
    assert r["start"][5] == 0 and np.isnan(r["x_in"][5, 0])
    rest = np.ones(64, bool); rest[[5, 9]] = False
    for k in clean:
        assert np.array_equal(r[k][rest], clean[k][rest]), k


def test_tick_kernel_uses_no_scratch_on_gfx950(mm):
    """The kernel source cross-compiled for gfx950: the tick kernel's own resource usage, as the compiler reports it."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    src = os.path.join(ROOT, "tests", "tick_emu", "mmpc_tick_probe.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"Function Name: mmpc_tick_probe_kernel(.*?)LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    assert m, p.stderr[-2000:]
    get = lambda name: int(re.search(re.escape(name) + r": (\d+)", m.group(1)).group(1))
    usage = "VGPRs %d, SGPRs %d, occupancy %d waves/SIMD, scratch %d B/lane, LDS %s B" % (
        get("VGPRs"), get("SGPRs"), get("Occupancy [waves/SIMD]"), get("ScratchSize [bytes/lane]"), m.group(2))
    print(usage)
    assert get("ScratchSize [bytes/lane]") == 0, usage
    assert int(m.group(2)) == 8 * H.C.CDLL(H.build()).mmpc_tick_emu_lds_doubles(), usage
