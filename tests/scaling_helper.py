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
    deps = [_SRC, emu_helper.POISON_H] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".inc"))]
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


def _spd(rng, n, lo, hi, off):
    """a dense symmetric positive-definite n x n matrix: diagonal in [lo, hi], off-diagonal entries up to `off` of the smallest
    diagonal entry over n (strictly diagonally dominant)"""
    dg = rng.uniform(lo, hi, n)
    A = rng.uniform(-1, 1, (n, n)) * (off * dg.min() / n)
    A = 0.5 * (A + A.T)
    A[np.diag_indices(n)] = dg
    assert np.linalg.eigvalsh(A).min() > 0 and np.abs(A - np.diag(dg)).max() > 0
    return A


ONEHOT_VARIANTS = ("plain", "uguess", "xguess")
ONEHOT_SHAPES = [(0, 20, 5), (0, 30, 8), (1, 15, 3)]            # on the specialised and on the generic kernel
ONEHOT_DENSE = [("wb", 6, 2), ("base", 5, 1)]                    # generic kernel, dense R, W (and Q, P)
BASE_HEADING_W = (80.0, 90.0)     # Q, P heading weight of the base kind's one-hot cases: 2 w |e| reaches 237 with |e| < 2 rad


def onehot_entries(par, variant):
    """the gradient entries (k, v) a variant covers, v over the nx + nu columns; the input columns of stage N do not exist"""
    N, nx, nu = par.N, par.nx, par.nu
    st = [(k, v) for k in range(N + 1) for v in range(nx)]
    inp = [(k, nx + a) for k in range(N) for a in range(nu)]
    if getattr(par, "pose_ref", False):
        st = []          # (the state gradient goes through the forward kinematics: no one-hot construction)
    if variant == "uguess":
        return inp
    if variant == "xguess":
        return [e for e in st if e[0] >= 1]
    return sorted(st + inp)


def onehot_inputs(kind, N, M, variant, dense=False):
    """One instance per gradient entry (k_b, v_b) of onehot_entries: every entry of grad f(w0) of instance b has a prescribed
    magnitude in [10, 60] and a random sign, except entry (k_b, v_b), which has 120 + 3 (b mod 40) with its sign alternating
    over b - so g_b is that entry alone, differs from instance to instance, and sigma_b = 100 / g_b.  traj_ref and u_ref are
    solved for from the prescribed gradient; all weights are non-zero and drawn independently (P != Q, no zero in R or W),
    u_last is uniform in +-0.3.  Variants: "plain" (no guess: U = u_last, so R decides the input entries), "uguess" (U = u_last +
    a perturbation of +-0.1: R and W both contribute), "xguess" (X = tile(x0) + a perturbation of +-0.2 for the rows k >= 1; row 0
    of the guess holds 1e3 and is to be ignored).  dense: symmetric positive-definite dense R and W, and Q and P too (the generic
    kernel's cases).  The pose-reference kind has its reference on the start's own endpoint pose (state gradient zero) and input
    entries only.  Returns par, d, sigma, g; asserts that the numpy reference's g is the prescribed hot value."""
    par = par_of(kind, N)
    pose = getattr(par, "pose_ref", False)
    nx, nu, nq = par.nx, par.nu, par.Q.shape[0]
    ent = onehot_entries(par, variant)
    B = len(ent)
    rng = np.random.default_rng([N, M, nx, ONEHOT_VARIANTS.index(variant), int(dense)])
    # ---- weights
    if dense:
        par.Q, par.P = _spd(rng, nq, 3.0, 30.0, 0.5), _spd(rng, nq, 3.0, 30.0, 0.5)
        par.R, par.W = _spd(rng, nu, 2.0, 20.0, 0.8), _spd(rng, nu, 2.0, 20.0, 0.8)
    else:
        par.Q, par.P = np.diag(rng.uniform(3.0, 30.0, nq)), np.diag(rng.uniform(3.0, 30.0, nq))
        par.R, par.W = np.diag(rng.uniform(2.0, 20.0, nu)), np.diag(rng.uniform(2.0, 20.0, nu))
    if par.kind == "base":
        for A, w in zip((par.Q, par.P), BASE_HEADING_W):
            A[2, :] = A[:, 2] = 0.0          # (the heading error is no plain difference: it stays uncoupled)
            A[2, 2] = w
    assert (np.diag(par.Q) != 0).all() and (np.diag(par.P) != 0).all() and (np.diag(par.R) != 0).all() and (np.diag(par.W) != 0).all()
    assert not np.array_equal(par.Q, par.P)
    # ---- start, previous input, guesses, obstacles
    lo = np.array([-1, -1, -0.8, -1, -1, -1, -0.5, -2.0, 0.5][:nx]); hi = np.array([1, 1, 0.8, 1, 1, 1, 0.5, -0.5, 2.0][:nx])
    x_init = rng.uniform(lo, hi, (B, nx))
    assert (x_init > par.xlim[0]).all() and (x_init < par.xlim[1]).all()
    u_last = rng.uniform(-0.3, 0.3, (B, N, nu))
    d = dict(x_init=x_init, u_last=u_last)
    d["obs"] = np.tile(np.array([50.0, 50.0, 0.3]), (B, M, 1)) + rng.uniform(0, 5, (B, M, 1))
    X = np.tile(x_init[:, None, :], (1, N + 1, 1))
    U = u_last.copy()
    if variant == "uguess":
        U = u_last + rng.uniform(-0.1, 0.1, (B, N, nu))
        d["u_guess"] = U.copy()
    if variant == "xguess":
        X[:, 1:] += rng.uniform(-0.2, 0.2, (B, N, nx))
        d["x_guess"] = X.copy()
        d["x_guess"][:, 0] = 1e3
    # ---- the prescribed gradient
    gX = rng.uniform(10, 60, (B, N + 1, nx)) * rng.choice([-1.0, 1.0], (B, N + 1, nx))
    gU = rng.uniform(10, 60, (B, N, nu)) * rng.choice([-1.0, 1.0], (B, N, nu))
    hot = 120.0 + 3.0 * (np.arange(B) % 40)
    for b, (k, v) in enumerate(ent):
        h = hot[b] * (1.0 if b % 2 == 0 else -1.0)
        if v < nx:
            gX[b, k, v] = h
        else:
            gU[b, k, v - nx] = h
    # ---- references from it: 2 Q e = gX, 2 R (U - u_ref) + 2 W (U - u_last) = gU
    if pose:
        d["traj_ref"] = np.array([np.tile(nlp.endpoint_pose(x_init[b]), (N + 1, 1)) for b in range(B)])
    else:
        e = np.empty_like(gX)
        e[:, :N] = np.linalg.solve(2 * par.Q, gX[:, :N].reshape(-1, nx).T).T.reshape(B, N, nx)
        e[:, N] = np.linalg.solve(2 * par.P, gX[:, N].T).T
        ref = X - e
        if par.kind == "base":
            assert np.abs(e[..., 2]).max() < 2.0          # the heading error stays inside +-2 rad
            ref[::3, :, 2] += 2 * np.pi                   # reference headings move by non-negative multiples of 2 pi only
            ref[1::5, :, 2] += 4 * np.pi
        d["traj_ref"] = ref
    d["u_ref"] = U - np.linalg.solve(2 * par.R, (gU - np.einsum("ij,bkj->bki", 2 * par.W, U - u_last)).reshape(-1, nu).T).T.reshape(B, N, nu)
    sig, g = sigma_numpy(par, d)
    assert np.allclose(g, hot, rtol=1e-9, atol=0), np.abs(g / hot - 1).max()      # the case holds by the reference alone
    assert len(set(np.round(hot[:40], 9))) == min(B, 40) and (sig < 1).all()
    return par, d, sig, g


def obs_in_mode(obs, N, mode):
    """a static obstacle record (B, M, 3) as the input of obstacle mode False (itself), True (the table per stage) or "motion"
    (the record with zero velocities)"""
    if mode is True:
        return np.ascontiguousarray(np.repeat(obs[:, None], N + 1, axis=1))
    if mode == "motion":
        return np.concatenate([obs, np.zeros(obs.shape[:2] + (2,))], axis=2)
    return obs


DECIDERS = ("R", "W", "P", "xguess")
DECIDER_SHAPES = [(0, 20, 3), (1, 15, 3), (0, 30, 8), ("wb", 6, 2)]      # the last one on the generic kernel
_BLOCK_OF = {"R": "R", "W": "W", "P": "P", "xguess": "X"}


def grad_blocks(par, d, b):
    """max-norms of the blocks of grad f(w0) of instance b: the stage state entries ("Q"), the terminal ones ("P"), and the two
    terms of the input entries, 2 R (U - u_ref) ("R") and 2 W (U - u_last) ("W")"""
    prob = nlp.Problem(par, nlp.clip_x_init(par, d["x_init"][b]), d["traj_ref"][b], d["u_ref"][b], d["u_last"][b], d["obs"][b])
    X, U, s = start_point(par, d, b)
    gX = nlp.cost_grad(prob, X, U, s)[0]
    return dict(Q=np.abs(gX[:-1]).max(), P=np.abs(gX[-1]).max(), R=np.abs(2 * par.R @ (U - d["u_ref"][b]).T).max(),
                W=np.abs(2 * par.W @ (U - d["u_last"][b]).T).max())


def decider_inputs(name, kind, N, M, B=8):
    """Full solves whose factor another term than Q (x0 - x_ref_k) decides, on synth.make_batch (config_id 3).  Every reference is
    drawn in towards its start so that the stage state entries of grad f at tile(x_init) stay at `quiet` (well below G); the first
    three quarters of the instances then get the deciding term, the last quarter stays unscaled:
      "R": R raised (diagonal), u_ref away from a non-zero u_last in three entries per instance: 2 R |u_last - u_ref| decides;
      "W": W raised, a U guess away from a non-zero u_last in three entries per instance: 2 W |u_guess - u_last| decides;
      "P": P = 4 Q: the terminal entry decides;
      "xguess": an X guess, the roll-out of a U guess of full acceleration, that leaves the reference: Q (x_guess_k - x_ref_k)
                decides, and tile(x_init) alone would give sigma = 1.
    Asserted here, in numpy, for at least half of the instances: the intended block of grad_blocks is the largest, the next one
    is at most 0.9 of it, the instance is scaled; and check_both_branches."""
    wb = kind != 1
    par = par_of(kind, N)
    rng = np.random.default_rng([N, M, DECIDERS.index(name)])
    d = synth.make_batch(B, N=N, M=M, kind="wholebody" if wb else "base", config_id=3)
    nu = par.nu
    if not wb:
        par.Q = np.diag([25., 25., 5., 0, 0, 5.]); par.P = par.Q.copy()
    quiet = 45.0
    hotrows = np.arange(B) < B - max(2, B // 4)
    umag = np.array([1.6, 1.6, 0.45, 0.45, 0.45][:nu])              # inside the input box and the rate box around u_last
    wide = np.diag([40., 40., 150., 150., 150.][:nu])              # 2 w umag = 128 ... 135
    d["u_last"] = rng.uniform(-0.1, 0.1, (B, N, nu))
    d["u_ref"] = d["u_last"].copy() if name in ("R", "W") else d["u_ref"]
    if name == "P":
        par.P = 4.0 * par.Q
        quiet = 40.0
    if name == "xguess":
        quiet = 90.0
        # the hot rows start at 1.5 m/s straight away from where their reference leads: the roll-out leaves it from the first stage on
        away = d["x_init"][:, :2] - d["traj_ref"][:, N, :2]
        d["x_init"][hotrows, 3:5] = (1.5 * away / np.linalg.norm(away, axis=1, keepdims=True))[hotrows]
    # the references drawn in: the stage state entries at tile(x_init) reach `quiet` (the unscaled rows: half of it)
    for b in range(B):
        x0 = nlp.clip_x_init(par, d["x_init"][b])
        d["traj_ref"][b, 0] = x0
        one = instance(d, b)
        blk = grad_blocks(par, one, 0)
        q1 = max(blk["Q"], blk["P"]) if name == "xguess" else blk["Q"]
        f = (quiet * rng.uniform(0.8, 1.0) if hotrows[b] else 0.5 * quiet) / q1
        d["traj_ref"][b] = x0 + f * (d["traj_ref"][b] - x0)
    if name == "R":
        par.R = wide
    if name == "W":
        par.W = wide
        d["u_guess"] = d["u_last"] + rng.uniform(-0.02, 0.02, (B, N, nu))
    if name in ("R", "W"):
        for b in np.flatnonzero(hotrows):
            for k, a in zip(rng.choice(N, 3, replace=False), rng.choice(nu, 3, replace=nu < 3)):
                delta = umag[a] * rng.uniform(0.9, 1.0) * rng.choice([-1.0, 1.0])
                if name == "R":
                    d["u_ref"][b, k, a] = d["u_last"][b, k, a] + delta
                else:
                    d["u_guess"][b, k, a] = d["u_last"][b, k, a] + delta
    if name == "xguess":
        ug = rng.uniform(-0.05, 0.05, (B, N, nu))
        xg = np.zeros((B, N + 1, par.nx))
        for b in range(B):
            best = None
            for acc in ((1.9, -1.9) if hotrows[b] else (ug[b, 0, 0],)):      # full acceleration, the sign that leaves the reference
                u = ug[b].copy(); u[:, 0] = acc
                x = np.zeros((N + 1, par.nx))
                x[0] = nlp.clip_x_init(par, d["x_init"][b])
                for k in range(N):
                    x[k + 1] = nlp.f_dyn(par.kind, x[k], u[k], par.dt)
                dev = np.abs(x[:, :2] - d["traj_ref"][b, :, :2]).max()
                if best is None or dev > best[0]:
                    best = (dev, u, x)
            ug[b], xg[b] = best[1], best[2]
        d["x_guess"], d["u_guess"] = xg, ug
        tiled = {k: v for k, v in d.items() if k not in ("x_guess", "u_guess")}
        assert (sigma_numpy(par, tiled)[0] == 1).all()       # tile(x_init), u_last: nobody is scaled
    sig, g = sigma_numpy(par, d)
    good = 0
    want = _BLOCK_OF[name]
    for b in range(B):
        blk = grad_blocks(par, d, b)
        if want == "X":          # the X guess: the state entries, whichever stage, against the input entries
            blk = dict(X=max(blk["Q"], blk["P"]), R=blk["R"], W=blk["W"])
        rest = max(v for k, v in blk.items() if k != want)
        good += int(sig[b] < 1 and blk[want] == max(blk.values()) and rest <= 0.9 * blk[want])
    assert 2 * good >= B, (name, kind, N, M, good)
    check_both_branches(sig)
    return par, d, sig


FLEET = dict(B=8, N=30, M=8, T=3)      # the receding-horizon tests: three ticks of a fleet of eight


def fleet_plan():
    """the fleet of the receding-horizon tests (synth.make_batch with config_id 5: moving obstacles; straight plans): par, clipped starts, plans, obstacles, velocities"""
    import tick_emu_helper as H
    B, N, M = FLEET["B"], FLEET["N"], FLEET["M"]
    d = synth.make_batch(B, N=N, M=M, config_id=5, moving=True)
    par = nlp.WholeBodyParams(N=N)
    return par, np.clip(d["x_init"], par.xlim[0], par.xlim[1]), H.straight_plan(d["traj_ref"], N), d["obs"], d["obs_vel"]


def tick_inputs(x_in, loc, obs, u_prev, ug=None, xg=None):
    """the solve of one fleet tick as an input dict: u_last = the previous optimum (zeros at tick 0), u_ref = 0, the guesses of a
    shifted warm start when there are some"""
    d = dict(x_init=x_in, traj_ref=loc, u_ref=np.zeros_like(u_prev), u_last=u_prev, obs=obs)
    if ug is not None:
        d["u_guess"], d["x_guess"] = ug, xg
    return d


def guess_decides(par, d):
    """per instance: the factor at the guesses differs from the factor tile(x_init), u_last would give (relative 1e-6)"""
    plain = {k: v for k, v in d.items() if k not in ("u_guess", "x_guess")}
    return np.abs(sigma_numpy(par, d)[0] / sigma_numpy(par, plain)[0] - 1) > 1e-6


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
