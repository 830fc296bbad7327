"""GPU (MI355X): every code path mmpc_create can choose, across the shapes it accepts.

mmpc_create turns a config into a specialised kernel (MMPC_FAST_LIST), a static-LDS generic instantiation (MMPC_STATIC_LIST)
or the dynamic-LDS generic kernel mmpc_solve_kernel<KIND>; a config is accepted when the generic kernel's LDS slab fits
160 KiB.  This module runs each path at the edges of that envelope through the C ABI (mmpc_amd._capi.Engine, device-pointer
calls: stateless, no warm start) against the C oracle on identical seeded inputs, with the rules of tests/test_gpu_parity.py:
  - every instance converges on both sides, iteration counts are equal in >= 90 % of the instances;
  - an instance is in the oracle's minimum when its cost is within 1e-6 relative; those agree to 1e-6 on X and U (1e-5 with
    per-stage obstacles or half-space planes) and to 1e-9 on the cost; at most 1 of 16 is in another minimum, one that costs
    no more than 1.05 x the oracle's;
plus properties that do not depend on the algorithm: the dynamics residual of the returned trajectory, the boxes, and IPOPT's
termination test (nlp.kkt_certificate_ipopt) on the two slowest instances of every case, certified in one batch at the end.
The host layout of the slab (emu_helper.lds_bytes: the kernel's own mmpc_layout compiled for the host) decides which shapes
must be accepted and which refused."""
import copy

import numpy as np
import pytest

from oracle import nlp, coracle, synth
from cert_pool import certify
from test_slsqp_golden import cert_ok
import emu_helper

pytestmark = pytest.mark.gpu

B = 16
LDS_LIMIT = 160 * 1024
KINDS = {"wb": 0, "base": 1, "pose": 2}
_CERTS = []          # (case id, instance, nlp.Problem, X, U, s) of the two slowest instances of every matrix case


def _par(kind, N):
    return {"wb": nlp.WholeBodyParams, "base": nlp.BaseParams, "pose": nlp.pose_ref_params}[kind](N=N)


def _extra_obstacles(p0, goal, n, rng):
    """n discs beside the straight line p0 -> goal (synth.make_batch's placement, 0.8 - 2.5 to the side), none within r + 0.6
    of p0."""
    out = []
    d = (goal - p0) / max(np.linalg.norm(goal - p0), 1e-9)
    nrm = np.array([-d[1], d[0]])
    while len(out) < n:
        c = p0 + rng.uniform(0.15, 0.9) * (goal - p0) + rng.uniform(0.8, 2.5) * rng.choice([-1, 1]) * nrm
        r = rng.uniform(0.1, 0.4)
        if np.linalg.norm(c - p0) >= r + 0.6:
            out.append([c[0], c[1], r])
    return np.array(out).reshape(n, 3)


def _fit_obstacles(obs, M, x0, goal, rng):
    """obs (B, m, 3) cut or completed to M discs per instance."""
    if obs.shape[1] >= M:
        return np.ascontiguousarray(obs[:, :M])
    return np.stack([np.concatenate([obs[b], _extra_obstacles(x0[b, :2], goal[b, :2], M - obs.shape[1], rng)]) for b in range(len(obs))])


def _per_stage(obs, vel, N, dt):
    """(B, M, 3) centres moving at vel (B, M, 2) -> (B, N + 1, M, 3)"""
    out = np.repeat(obs[:, None], N + 1, axis=1)
    out[..., :2] += vel[:, None] * (dt * np.arange(N + 1))[None, :, None, None]
    return out


def _planes(hs, L, rng):
    """The first L of make_c1_starts' planes; beyond those, seeded jittered copies (point and normal, normal renormalised)."""
    out = [h.copy() for h in hs[:L]]
    for i in range(len(out), L):
        h = hs[i % len(hs)] + np.r_[rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.15, 0.15, 3)]
        h[3:] /= np.linalg.norm(h[3:])
        out.append(h)
    return np.array(out)


def make_case(kind, N, M, ops=False, L=0, aw=False, n=B):
    """Seeded inputs of one case: dict(par, x (clipped for the whole-body kinds), tr, ur, ul, obs, hs, aw)."""
    seed = 1000 + 100 * N + 10 * M + (5 if ops else 0) + L
    rng = np.random.default_rng(seed)
    par = _par(kind, N)
    hs = None
    if L:
        x, tr, obs, hs0 = synth.make_c1_starts(n, N=N, nplanes=2 if L <= 2 else 3, seed=seed)
        hs = _planes(hs0, L, rng)
        ur = np.zeros((n, N, 5))
        obs = _fit_obstacles(obs, M, x, tr[:, -1], rng)
        vel = rng.uniform(-0.5, 0.5, (n, M, 2))
    elif kind == "pose":
        x, tr, obs = emu_helper.pose_batch(n, N, seed=seed)
        ur = np.zeros((n, N, 5))
        obs = _fit_obstacles(obs, M, x, tr[:, -1], rng)
        # (slower than the other kinds' obstacles: the pose cost pins the base only through the endpoint, and discs that sweep
        #  across at 0.5 m/s leave optima whose inputs a KKT test at 1e-8 determines to ~1e-4 only)
        vel = rng.uniform(-0.2, 0.2, (n, M, 2))
    else:
        d = synth.make_batch(n, N=N, M=max(M, 1), kind="wholebody" if kind == "wb" else "base", config_id=seed, moving=True)
        x, tr, ur = d["x_init"], d["traj_ref"], d["u_ref"]
        obs, vel = d["obs"][:, :M], d["obs_vel"][:, :M]
    if ops:
        obs = _per_stage(obs, vel, N, par.dt)
    if kind != "base":
        x = np.clip(x, par.xlim[0], par.xlim[1])
    return dict(par=par, x=x, tr=tr, ur=ur, ul=np.zeros((n, N, par.nu)), obs=np.ascontiguousarray(obs), hs=hs, aw=aw)


def case_id(kind, N, M, ops=False, L=0, aw=False):
    return "%s-N%d-M%d%s%s%s" % (kind, N, M, "-ops" if ops else "", "-L%d" % L if L else "", "-aw" if aw else "")


def _engine(mm, kind, c, max_batch=B):
    par = c["par"]
    return mm._capi.Engine(KINDS[kind], par.N, c["obs"].shape[-2], par.dt, par.ulim, par.xlim, par.dulim, max_batch=max_batch,
                           obs_per_stage=c["obs"].ndim == 4, halfspaces=c["hs"], as_written=c["aw"], max_iter=2000)


def _gpu(eng, c, rows=slice(None)):
    """One device-pointer launch (x_guess = tile(x_init), U_last = 0) of the rows `rows` of case c; numpy outputs."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows], dtype=np.float64)).to(dev)
    r = eng.solve_batch_device(t(c["x"]), t(c["tr"]), t(c["ur"]), t(c["ul"]), t(c["obs"]))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _oracle(c):
    return coracle.solve_batch(c["par"], c["x"], c["tr"], c["ur"], c["ul"], c["obs"], nthreads=16, max_iter=2000, hs=c["hs"],
                               as_written=c["aw"])


def check_parity(r, o, loose):
    """The rules of tests/test_gpu_parity.py (docstring of this module)."""
    tol = 1e-5 if loose else 1e-6
    assert (r["status"] == 0).all() and (o["status"] == 0).all(), (r["status"], o["status"])
    assert (r["iters"] == o["iters"]).mean() >= 0.9, (r["iters"], o["iters"])
    rel = np.abs(r["cost"] / o["cost"] - 1)
    same = rel < 1e-6
    assert (~same).sum() <= 1 and (r["cost"][~same] <= 1.05 * o["cost"][~same]).all(), (rel, r["cost"], o["cost"])
    assert rel[same].max() <= 1e-9, rel
    dX = np.abs(r["X"][same] - o["X"][same]).max()
    dU = np.abs(r["U"][same] - o["U"][same]).max()
    assert dX <= tol and dU <= tol, (dX, dU)


def check_properties(c, r):
    """Dynamics residual of the returned trajectory <= 1e-8; input, rate (about U_last) and state boxes hold to 1e-7."""
    par, X, U = c["par"], r["X"], r["U"]
    model = "base" if par.kind == "base" else "wholebody"
    Xn = np.array([[nlp.f_dyn(model, X[b, k], U[b, k], par.dt) for k in range(par.N)] for b in range(len(X))])
    assert np.abs(Xn - X[:, 1:]).max() <= 1e-8
    assert (U <= par.ulim[1] + 1e-7).all() and (U >= par.ulim[0] - 1e-7).all()
    dU = U - c["ul"]
    assert (dU <= par.dulim[1] + 1e-7).all() and (dU >= par.dulim[0] - 1e-7).all()
    assert (X[:, 1:] <= par.xlim[1] + 1e-7).all() and (X[:, 1:] >= par.xlim[0] - 1e-7).all()


def _pool_certificates(cid, c, r):
    for b in np.argsort(-r["iters"], kind="stable")[:2]:
        prob = nlp.Problem(c["par"], c["x"][b], c["tr"][b], c["ur"][b], c["ul"][b], c["obs"][b], c["hs"], as_written=c["aw"])
        _CERTS.append((cid, int(b), prob, r["X"][b], r["U"][b], r["s"][b]))


def _run_case(mm, kind, N, M, ops=False, L=0, aw=False, c=None, eng=None, certify_as=None):
    """GPU vs oracle and the properties on one case; returns (inputs, GPU outputs, oracle outputs)."""
    c = c or make_case(kind, N, M, ops, L, aw)
    eng = eng or _engine(mm, kind, c)
    r = _gpu(eng, c)
    o = _oracle(c)
    check_parity(r, o, loose=ops or L > 0)
    check_properties(c, r)
    if certify_as:
        _pool_certificates(certify_as, c, r)
    return c, r, o


# ---------------------------------------------------------------------------------------------------------------- the matrix
GENERIC = [("wb", 1, 0), ("wb", 1, 16), ("wb", 2, 1), ("wb", 31, 16), ("wb", 35, 16), ("wb", 44, 5), ("wb", 47, 2),
           ("wb", 49, 0), ("wb", 32, 16, True), ("wb", 39, 8, True),
           ("base", 1, 0), ("base", 40, 3), ("base", 59, 16), ("base", 63, 13), ("base", 63, 10, True),
           ("pose", 1, 2), ("pose", 38, 16), ("pose", 55, 0), ("pose", 35, 16, True)]
PLANES = [(20, 3, 1, False), (20, 16, 8, False), (20, 10, 5, True), (20, 3, 6, True), (30, 0, 2, True)]
FAST = [("wb", 20, 5), ("wb", 30, 8), ("wb", 20, 3), ("base", 15, 3)]      # MMPC_FAST_LIST


@pytest.mark.parametrize("spec", GENERIC, ids=[case_id(*s) for s in GENERIC])
def test_generic_kernel_envelope(mm, spec):
    """The dynamic-LDS generic kernel of each kind at the edges: N = 1, 2, the largest N whose slab fits at M = 0 / 5 / 16,
    per-stage obstacles, M = 0 and M = 16."""
    kind, N, M = spec[:3]
    ops = len(spec) > 3
    c = make_case(kind, N, M, ops)
    eng = _engine(mm, kind, c)
    assert eng.lds_bytes == emu_helper.lds_bytes(KINDS[kind], N, M, ops) <= LDS_LIMIT
    _run_case(mm, kind, N, M, ops, c=c, eng=eng, certify_as=case_id(kind, N, M, ops))


@pytest.mark.parametrize("spec", PLANES, ids=[case_id("wb", N, M, False, L, aw) for N, M, L, aw in PLANES])
def test_halfspace_planes_envelope(mm, spec):
    """L = 1 and L = 8 intended rows, the largest as-written plane counts that fit (L = 5 up to M = 10, L = 6 up to M = 3 at
    N = 20; L = 2 at N = 30 with M = 0 only)."""
    N, M, L, aw = spec
    c = make_case("wb", N, M, L=L, aw=aw)
    eng = _engine(mm, "wb", c)
    assert eng.lds_bytes == emu_helper.lds_bytes(0, N, M, False, L, aw) <= LDS_LIMIT
    _run_case(mm, "wb", N, M, L=L, aw=aw, c=c, eng=eng, certify_as=case_id("wb", N, M, False, L, aw))


def test_dense_weights_and_terminal_equality_at_the_largest_shape(mm):
    """Dense symmetric weights and the terminal-xy equality (both run on the generic kernel only) at whole-body (44, 5), the
    largest horizon that fits with five obstacles; the reference is shortened so that the equality is reachable."""
    N, M = 44, 5
    c = make_case("wb", N, M)
    par = c["par"]
    rng = np.random.default_rng(44)
    A = rng.normal(size=(9, 9)) * 0.3
    Cr = rng.normal(size=(5, 5)) * 0.1
    par.Q = par.Q + A @ A.T; par.P = par.P + A @ A.T; par.R = par.R + Cr @ Cr.T
    par.terminal_xy_equality = True
    c["tr"][:, :, :2] = c["x"][:, None, :2] + 0.4 * (c["tr"][:, :, :2] - c["x"][:, None, :2])
    eng = _engine(mm, "wb", c)
    eng.set_weights(Q=par.Q, R=par.R, P=par.P, S=par.S, W=par.W)
    eng.set_terminal_xy_equality(True)
    _, r, _ = _run_case(mm, "wb", N, M, c=c, eng=eng, certify_as="wb-N44-M5-dense-xyeq")
    assert np.abs(r["X"][:, N, :2] - c["tr"][:, N, :2]).max() < 1e-9


FAST_OPS = [s + (ops,) for s in FAST for ops in (False, True)]


@pytest.mark.parametrize("spec", FAST_OPS, ids=[case_id(*s) for s in FAST_OPS])
def test_specialised_kernels_against_oracle_and_generic(mm, monkeypatch, spec):
    """Every specialised kernel, with and without per-stage obstacles: against the oracle, and against the generic kernel
    of the same shape (MMPC_FORCE_GENERIC at creation) on the same inputs - the same algorithm, so the same iteration counts."""
    kind, N, M, ops = spec
    c = make_case(kind, N, M, ops)
    fast = _engine(mm, kind, c)
    monkeypatch.setenv("MMPC_FORCE_GENERIC", "1")
    gen = _engine(mm, kind, c)
    monkeypatch.delenv("MMPC_FORCE_GENERIC")
    assert gen.lds_bytes == emu_helper.lds_bytes(KINDS[kind], N, M, ops) != fast.lds_bytes      # two different kernels run
    _, rf, _ = _run_case(mm, kind, N, M, ops, c=c, eng=fast, certify_as="fast-" + case_id(kind, N, M, ops))
    _, rg, _ = _run_case(mm, kind, N, M, ops, c=c, eng=gen)
    assert (rf["iters"] == rg["iters"]).mean() >= 0.9, (rf["iters"], rg["iters"])


@pytest.mark.parametrize("M", [5, 3], ids=["wb-N20-M5", "wb-N20-M3"])
def test_static_and_dynamic_generic_kernels(mm, monkeypatch, M):
    """Whole-body (20, M) forced onto the generic kernel: its static-LDS instantiation (MMPC_STATIC_LIST: what dense weights
    or the terminal equality select at these shapes) and, with MMPC_NO_STATIC_GENERIC, the dynamic-LDS kernel."""
    c = make_case("wb", 20, M)
    monkeypatch.setenv("MMPC_FORCE_GENERIC", "1")
    static = _engine(mm, "wb", c)
    monkeypatch.setenv("MMPC_NO_STATIC_GENERIC", "1")
    dynamic = _engine(mm, "wb", c)
    monkeypatch.delenv("MMPC_NO_STATIC_GENERIC")
    monkeypatch.delenv("MMPC_FORCE_GENERIC")
    _, rs, _ = _run_case(mm, "wb", 20, M, c=c, eng=static)
    _, rd, _ = _run_case(mm, "wb", 20, M, c=c, eng=dynamic)
    assert (rs["iters"] == rd["iters"]).mean() >= 0.9, (rs["iters"], rd["iters"])


@pytest.mark.parametrize("spec", [("wb", 20, 5), ("base", 15, 3)], ids=["wb-N20-M5-ops", "base-N15-M3-ops"])
def test_budgeted_launches_with_per_stage_obstacles(mm, spec):
    """Iteration budget 7 on the specialised kernels with per-stage obstacles: launch, then continuations until nobody is
    suspended; every output is bitwise that of the launch without a budget."""
    import torch
    kind, N, M = spec
    c = make_case(kind, N, M, True)
    eng = _engine(mm, kind, c)
    ref = _gpu(eng, c)
    assert (ref["status"] == 0).all() and (ref["iters"] > 7).any()
    eng.set_iteration_budget(7)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    args = [t(c[k]) for k in ("x", "tr", "ur", "ul", "obs")]
    out = eng.solve_batch_device(*args)
    assert eng.suspended_count() == int((ref["iters"] > 7).sum())
    for _ in range(2000 // 7 + 1):
        torch.cuda.synchronize()
        if not bool((out["status"] == 3).any()):
            break
        eng.resume_batch_device(*args, out=out)
    torch.cuda.synchronize()
    eng.set_iteration_budget(0)
    for k in ("X", "U", "s", "status", "iters", "cost", "err"):
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), k


@pytest.mark.parametrize("spec", FAST, ids=[case_id(*s) for s in FAST])
def test_bounds_just_under_the_infinity_threshold(mm, spec):
    """Every +-inf limit set to +-9.9e18 (and the base-velocity boxes of the whole-body kind too): rows with slacks near 1e19,
    kept because |b| < 1e19, enter the specialised kernels' product form of the barrier's log sum.  Each instance equals the
    oracle under the same limits, in the same number of iterations."""
    kind, N, M = spec
    c = make_case(kind, N, M)
    par = c["par"]
    big = 9.9e18
    par.ulim, par.xlim, par.dulim = par.ulim.copy(), par.xlim.copy(), par.dulim.copy()
    for a in (par.ulim, par.xlim, par.dulim):
        a[0][~np.isfinite(a[0])] = -big
        a[1][~np.isfinite(a[1])] = big
    if kind == "wb":
        par.xlim[:, 3:6] = [[-big] * 3, [big] * 3]
    eng = _engine(mm, kind, c)
    assert eng.lds_bytes != emu_helper.lds_bytes(KINDS[kind], N, M)          # the specialised kernel runs
    _, r, o = _run_case(mm, kind, N, M, c=c, eng=eng)
    assert np.array_equal(r["iters"], o["iters"]), (r["iters"], o["iters"])
    assert np.abs(r["X"] - o["X"]).max() <= 1e-6 and np.abs(r["U"] - o["U"]).max() <= 1e-6
    # (the certificate's least squares cannot carry rows whose slacks are ~1e19: it is taken on the same NLP without them - rows
    #  that far from any iterate never restrict it, their multipliers are ~mu / 1e19)
    cpar = copy.copy(par)
    cpar.ulim, cpar.xlim, cpar.dulim = [np.where(np.abs(a) >= 1e18, np.copysign(np.inf, a), a) for a in (par.ulim, par.xlim, par.dulim)]
    _pool_certificates("big-" + case_id(kind, N, M), dict(c, par=cpar), r)


# ---------------------------------------------------------------------------------------------------- create-time boundary
def _n_max(kind, M, ops):
    return max(N for N in range(1, 64) if emu_helper.lds_bytes(kind, N, M, ops) <= LDS_LIMIT)


BOUNDARY = [(kind, ops, M) for kind in KINDS for ops in (False, True) for M in (0, 16)]


@pytest.mark.parametrize("spec", BOUNDARY, ids=["%s-M%d%s" % (k, M, "-ops" if ops else "") for k, ops, M in BOUNDARY])
def test_create_accepts_exactly_the_slabs_that_fit(mm, spec):
    """N_max = the largest horizon whose slab fits 160 KiB (host layout): created, with the slab the host computes and at least
    one resident problem per CU; N_max + 1 refused with an error that names LDS (include/mmpc.h: mmpc_config)."""
    kind, ops, M = spec
    k = KINDS[kind]
    n = _n_max(k, M, ops)
    c = make_case(kind, n, M, ops, n=1)
    eng = _engine(mm, kind, c, max_batch=1)
    assert eng.lds_bytes == emu_helper.lds_bytes(k, n, M, ops)
    assert eng.problems_per_cu >= 1 and eng.problems_per_cu * eng.lds_bytes <= LDS_LIMIT
    eng.close()
    if n < 63:
        with pytest.raises(RuntimeError, match="LDS"):
            _engine(mm, kind, make_case(kind, n + 1, M, ops, n=1), max_batch=1)


def test_create_boundary_of_as_written_planes(mm):
    """As-written planes at N = 20: L = 5 fits up to M = 10, L = 7 never (host layout and mmpc_create agree)."""
    for M, L, fits in ((10, 5, True), (11, 5, False), (0, 7, False)):
        assert (emu_helper.lds_bytes(0, 20, M, False, L, True) <= LDS_LIMIT) == fits
        c = make_case("wb", 20, M, L=L, aw=True, n=1)
        if fits:
            eng = _engine(mm, "wb", c, max_batch=1)
            assert eng.lds_bytes == emu_helper.lds_bytes(0, 20, M, False, L, True)
            assert eng.problems_per_cu >= 1 and eng.problems_per_cu * eng.lds_bytes <= LDS_LIMIT
            eng.close()
        else:
            with pytest.raises(RuntimeError, match="LDS"):
                _engine(mm, "wb", c, max_batch=1)


# ------------------------------------------------------------------------------------------------- handles and launch order
def test_interleaved_handles_of_one_kind(mm):
    """The dynamic-LDS size is an attribute of the kernel function, shared by the handles of a kind: a large handle (49, 0),
    then a small one (12, 2), created before either launches; launches A, B, A give A the same results twice, and both match
    the oracle."""
    ca, cb = make_case("wb", 49, 0), make_case("wb", 12, 2)
    a = _engine(mm, "wb", ca)
    b = _engine(mm, "wb", cb)
    assert a.lds_bytes > 150 * 1024 and b.lds_bytes < a.lds_bytes // 2
    ra = _gpu(a, ca)
    rb = _gpu(b, cb)
    ra2 = _gpu(a, ca)
    for k in ("X", "U", "s", "status", "iters", "cost", "err"):
        assert np.array_equal(ra[k], ra2[k]), k
    check_parity(ra, _oracle(ca), loose=False)
    check_parity(rb, _oracle(cb), loose=False)


@pytest.mark.parametrize("spec", [("wb", 35, 16), ("base", 63, 13)], ids=["wb-N35-M16", "base-N63-M13"])
def test_launch_order_on_the_generic_kernel(mm, spec):
    """B = 320 > 256: the a-priori difficulty key orders the first launch, the iteration counts of that launch the second one.
    Each instance gets bitwise what it gets in launches of 16 (batch order)."""
    kind, N, M = spec
    n = 320
    c = make_case(kind, N, M, n=n)
    eng = _engine(mm, kind, c, max_batch=n)
    r1 = _gpu(eng, c)
    r2 = _gpu(eng, c)
    parts = [_gpu(eng, c, slice(i, i + B)) for i in range(0, n, B)]
    for k in ("X", "U", "s", "status", "iters", "cost", "err"):
        small = np.concatenate([p[k] for p in parts])
        assert np.array_equal(r1[k], small) and np.array_equal(r2[k], small), k
    assert (r1["status"] == 0).mean() > 0.9


# ------------------------------------------------------------------------------------------------------------ certificates
def test_certificates_of_the_slowest_instances():
    """IPOPT's termination test of the reference NLP on the two slowest GPU instances of every matrix case above (one batch on
    the host cores).  Runs after the cases in this module, which fill the pool."""
    assert _CERTS, "the matrix cases of this module fill the pool: run the whole module"
    cs = certify([(p, X, U, s) for _, _, p, X, U, s in _CERTS], label="envelope certificates")
    bad = [(cid, b, c["E0"]) for (cid, b, *_), c in zip(_CERTS, cs) if not cert_ok(c)]
    assert not bad, bad
