"""Inputs, references and the host-emulation driver of the objective-scaling tests (tests/emu_scaling/mmpc_emu_scaling.cpp).
TEST ONLY: builds with g++ -DMMPC_EMU; never used by the product package.

The option (mmpc_set_objective_scaling, IPOPT's nlp_scaling_method = gradient-based) solves sigma_b f instead of f, with
sigma_b = G / g_b when g_b = |grad f(w0)|_inf exceeds G.  The references here: sigma from oracle.nlp.cost_grad in numpy, and the
C oracle's solve of the instance with Q, P, R, W, S times sigma_b."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np

import emu_helper
from oracle import nlp, coracle, synth

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu_scaling", "mmpc_emu_scaling.cpp")
_CSRC = os.path.join(_HERE, "..", "mobile-manipulator-mpc_amd", "csrc")

G_IPOPT = 100.0      # nlp_scaling_max_gradient
FAST = [(0, 20, 5), (0, 20, 3), (0, 30, 8), (1, 15, 3)]
GENERIC = [("wb", 6, 2), ("base", 5, 1), ("pose", 6, 2), ("wb-guess", 6, 2)]


def build():
    out = os.path.join(_HERE, "emu_scaling", "_build", "libmmpc_emu_scaling.so")
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".inc"))]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-O2", "-o", out, _SRC])
    return out


def kind_id(par):
    return (2 if getattr(par, "pose_ref", False) else 0) if par.kind == "wholebody" else 1


# ---- references -----------------------------------------------------------------------------------------------------------------
def start_point(par, d, b):
    """w0 of instance b: X = tile(clip(x_init)) or the X guess (row 0 stays the clipped start), U = u_last or the U guess, s = 0"""
    x0 = nlp.clip_x_init(par, d["x_init"][b])
    X = np.tile(x0, (par.N + 1, 1))
    if d.get("x_guess") is not None:
        X[1:] = d["x_guess"][b, 1:]
    U = np.array(d["u_guess"][b] if d.get("u_guess") is not None else d["u_last"][b], float)
    return X, U, np.zeros(par.N + 1)


def sigma_numpy(par, d, G=G_IPOPT):
    """sigma_b = g > G ? max(G / g, 1e-8) : 1 with g = |grad f(w0)|_inf over all of (X, U, s), from oracle.nlp.cost_grad"""
    B = d["x_init"].shape[0]
    sig = np.ones(B); g = np.zeros(B)
    for b in range(B):
        prob = nlp.Problem(par, nlp.clip_x_init(par, d["x_init"][b]), d["traj_ref"][b], d["u_ref"][b], d["u_last"][b], d["obs"][b])
        gX, gU, gs = nlp.cost_grad(prob, *start_point(par, d, b))
        g[b] = max(np.abs(gX).max(), np.abs(gU).max(), np.abs(gs).max())
        if g[b] > G:
            sig[b] = max(G / g[b], 1e-8)
    return sig, g


def scaled_par(par, sigma):
    """`par` with Q, P, R, W, S times sigma (a copy)"""
    p = copy.deepcopy(par)
    p.Q, p.P, p.R, p.W, p.S = par.Q * sigma, par.P * sigma, par.R * sigma, par.W * sigma, float(np.ravel(par.S)[0]) * sigma
    return p


def instance(d, b):
    """instance b of an input dict as a batch of one"""
    return {k: (None if v is None else np.ascontiguousarray(v[b:b + 1])) for k, v in d.items()}


def oracle_scaled(par, d, sigma):
    """the C oracle, instance by instance, with the weights times sigma_b; cost is the oracle's (the scaled objective)"""
    B = d["x_init"].shape[0]
    outs = []
    for b in range(B):
        i = instance(d, b)
        x0 = nlp.clip_x_init(par, i["x_init"][0])[None]
        X0 = None
        if i.get("x_guess") is not None:
            X0 = i["x_guess"].copy(); X0[0, 0] = x0[0]
        outs.append(coracle.solve_batch(scaled_par(par, sigma[b]), x0, i["traj_ref"], i["u_ref"], i["u_last"], i["obs"], X0=X0, U0=i.get("u_guess")))
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


def check_both_branches(sig):
    """every input builder: at least half of the instances scaled, at least one not"""
    assert (sig < 1).sum() * 2 >= len(sig) and (sig == 1).any(), sig
    return sig


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def par_of(kind, N):
    if kind == 1 or kind == "base":
        p = nlp.BaseParams(N=N)
    elif kind == "pose":
        p = nlp.pose_ref_params(N=N)
    else:
        p = nlp.WholeBodyParams(N=N)
    return p


HEADING_W = 150.0     # heading weight of the (1,15,3) case, see fast_inputs


def fast_inputs(kind, N, M, B=16):
    """the specialised shapes: synth.make_batch (seed 20240114, config_id 3), default weights for the whole-body kind.
    (0,20,5): of the generator's first 16 instances 7 are scaled, short of half; the batch is the first 10 scaled and the first 6
    unscaled instances of the generator's 64 (62.5 % of which are scaled), in the generator's order.
    (0,30,8): every make_batch instance is scaled (the reference runs 2.4 m and more ahead of the start), so instance 0 gets a
    reference drawn in to 0.3 of its length - a start on its own, short, path: sigma = 1.
    (1,15,3): Q = P = diag(5, 5, w, 0, 0, 1) with a heading weight w that qualifies through the heading term alone (x, y reach
    10 x 2.4 m = 24 at most); w = 30 scales too few starts (2 w |0.3 dpsi| > 100 needs |dpsi| > 5.5 rad), hence
    HEADING_W; every fourth instance has its reference heading moved by 2 pi, which angleDiff ignores and a plain
    difference does not."""
    par = par_of(kind, N)
    d = synth.make_batch(B, N=N, M=M, kind="base" if kind == 1 else "wholebody", config_id=3)
    d["u_last"] = np.zeros((B, N, par.nu))
    if (kind, N, M) == (0, 20, 5):
        d = synth.make_batch(4 * B, N=N, M=M, config_id=3)
        d["u_last"] = np.zeros((4 * B, N, par.nu))
        scaled = sigma_numpy(par, d)[0] < 1
        rows = np.sort(np.concatenate([np.flatnonzero(scaled)[:B - 6], np.flatnonzero(~scaled)[:6]]))
        d = {k: np.ascontiguousarray(v[rows]) for k, v in d.items()}
    if (kind, N, M) == (0, 30, 8):
        d["traj_ref"][0] = d["x_init"][0] + 0.3 * (d["traj_ref"][0] - d["x_init"][0])
    if kind == 1:
        par.Q = np.diag([5., 5., HEADING_W, 0, 0, 1.]); par.P = par.Q.copy()
        d["traj_ref"][::4, :, 2] += 2 * np.pi
        xy = 10.0 * np.abs(d["traj_ref"][:, :, :2] - d["x_init"][:, None, :2]).max()
        assert xy < G_IPOPT, xy      # whoever is scaled is scaled by the heading term
    sig, g = sigma_numpy(par, d)
    check_both_branches(sig)
    return par, d, sig


def generic_inputs(name, N, M, B=8):
    """the generic kernel's cases: dense symmetric Q and P (positive semi-definite: the default plus a rank-one term with
    off-diagonal entries), scaled by one factor so that G falls between the two smallest gradients of the batch - one instance
    keeps sigma = 1, the others are scaled.  "wb-guess": X and U guesses given, so that w0 is the guess."""
    kind = name.split("-")[0]
    par = par_of(kind, N)
    rng = np.random.default_rng(7 + N + M)
    if kind == "pose":
        x, ref, obs = emu_helper.pose_batch(B, N, seed=N)
        d = dict(x_init=x, traj_ref=ref, u_ref=np.zeros((B, N, 5)), obs=obs[:, :M])
    else:
        d = synth.make_batch(B, N=N, M=M, kind="base" if kind == "base" else "wholebody", config_id=3)
    d["u_last"] = np.zeros((B, N, par.nu))
    if name == "wb-guess":
        ug = rng.uniform(-0.2, 0.2, (B, N, par.nu))
        xg = np.zeros((B, N + 1, par.nx))
        for b in range(B):
            xg[b, 0] = nlp.clip_x_init(par, d["x_init"][b])
            for k in range(N):
                xg[b, k + 1] = nlp.f_dyn(par.kind, xg[b, k], ug[b, k], par.dt)
        d["x_guess"], d["u_guess"] = xg, ug
    n = par.Q.shape[0]
    v = rng.uniform(0.3, 1.0, n) * np.sign(rng.uniform(-1, 1, n)) * (np.diag(par.Q) > 0)
    par.Q = par.Q + 2.0 * np.outer(v, v); par.P = par.P + 3.0 * np.outer(v, v)
    assert np.abs(par.Q - np.diag(np.diag(par.Q))).max() > 0.1 and np.array_equal(par.Q, par.Q.T)
    _, g = sigma_numpy(par, d)
    gs = np.sort(g)
    f = 2.0 * G_IPOPT / (gs[0] + gs[1])
    par.Q = par.Q * f; par.P = par.P * f
    sig, _ = sigma_numpy(par, d)
    check_both_branches(sig)
    return par, d, sig


# ---- the emulation --------------------------------------------------------------------------------------------------------------
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_p = lambda a: a.ctypes.data_as(_dp) if a is not None else None
_i = lambda a: a.ctypes.data_as(_ip)


def solve(par, d, max_gradient=0.0, fast=False, reverse=False, budget=0, max_iter=200, want_scale=True, **kw):
    """One solve of the host emulation of d = dict(x_init, traj_ref, u_ref, u_last, obs[, x_guess, u_guess]).  max_gradient = 0:
    the option off.  budget > 0 (specialised kernels): budgeted launch, then one continuation without a budget, as the C ABI
    runs them.  kw: further arguments of emu_helper.make_params (mu_init, hs, as_written).  Returns dict(X, U, s, status, iters, cost, err, scale, launches); scale is pre-filled with -1."""
    lib = C.CDLL(build())
    assert lib.mmpc_emus_params_size() == C.sizeof(emu_helper.MmpcParams)
    c = lambda a: np.ascontiguousarray(a, float)
    x_init, traj_ref, u_ref, u_last, obs = c(d["x_init"]), c(d["traj_ref"]), c(d["u_ref"]), c(d["u_last"]), c(d["obs"])
    x_guess = c(d["x_guess"]) if d.get("x_guess") is not None else None
    u_guess = c(d["u_guess"]) if d.get("u_guess") is not None else None
    B, N, nx, nu, M = x_init.shape[0], par.N, par.nx, par.nu, obs.shape[-2]
    prm = emu_helper.make_params(par, M, obs.ndim == 4, x_guess is not None, max_iter=max_iter, **kw)
    if u_guess is not None:
        prm.u_guess = u_guess.ctypes.data
    X = np.zeros((B, N + 1, nx)); U = np.zeros((B, N, nu)); s = np.zeros((B, N + 1))
    status = np.zeros(B, np.int32); iters = np.zeros(B, np.int32); cost = np.zeros(B); err = np.zeros(B)
    scale = np.full(B, -1.0) if want_scale else None
    kind = kind_id(par)
    launches = 1
    head = (kind, C.byref(prm), B, _p(x_init), _p(traj_ref), _p(u_ref), _p(u_last), _p(x_guess), _p(obs), _p(X), _p(U), _p(s),
            _i(status), _i(iters), _p(cost), _p(err), int(reverse))
    tail = (C.c_double(float(max_gradient)), _p(scale))
    if not fast:
        assert lib.mmpc_emus_solve(*head, *tail) == 0
    else:
        state = None
        if budget > 0:
            sd = lib.mmpc_emus_fast_state_doubles(kind, N, M)
            assert sd > 0
            state = np.full((B, sd), np.nan)
        if lib.mmpc_emus_solve_fast(*head, int(budget), _p(state), 0, *tail) != 0:
            raise RuntimeError("no specialised instantiation for this configuration")
        if budget > 0 and (status == 3).any():
            assert lib.mmpc_emus_solve_fast(*head, 0, _p(state), 1, *tail) == 0
            launches += 1
    return dict(X=X, U=U, s=s, status=status, iters=iters, cost=cost, err=err, scale=scale, launches=launches)


def fast_lds_doubles(kind, N, M, mode):
    return C.CDLL(build()).mmpc_emus_fast_lds_doubles(int(kind), int(N), int(M), int(mode))


def lds_doubles(kind, N, M, mode, nhs=0, nq=0):
    return C.CDLL(build()).mmpc_emus_lds_doubles(int(kind), int(N), int(M), int(mode), int(nhs), int(nq))


BIT_KEYS = ("X", "U", "s", "status", "iters", "err")


def assert_bitwise(a, b, keys=BIT_KEYS, what=""):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs (max |diff| %g)" % (what, k, np.abs(x.astype(float) - y.astype(float)).max())
