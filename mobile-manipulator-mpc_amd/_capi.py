"""ctypes binding of the C ABI in include/mmpc.h (csrc/libmmpc.so).  No fallback of any kind:
a missing library or a failing call raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMPC_LIB") or os.path.join(_HERE, "csrc", "libmmpc.so")   # MMPC_LIB: A/B builds of the same HIP library

KIND_WHOLEBODY, KIND_BASE, KIND_WHOLEBODY_POSE = 0, 1, 2
STATUS_CONVERGED, STATUS_MAXITER, STATUS_NUMERIC, STATUS_SUSPENDED = 0, 1, 2, 3
PHASE_MOVE, PHASE_APPROACH, PHASE_ROTATE, PHASE_DONE = 0, 1, 2, 3      # MMPC_PHASE_*: mission_prepare
PHASE_MANIPULATE, PHASE_MANIP_DONE = 4, 5                              # ... and manipulate_prepare
HOLD_NEW, HOLD_READY, HOLD_LISTED, HOLD_RETIRED, HOLD_RETIRED_AT_DONE, HOLD_SUSPENDED = 0, 1, 2, 3, 4, 8   # MMPC_HOLD_*: mission_round
STATUS_Q8_REFUSED = 8      # host-side only (controllers/_q8.py): converged, but an as-written extra half-space row is violated


class MmpcConfig(C.Structure):
    _fields_ = [("kind", C.c_int), ("N", C.c_int), ("M", C.c_int), ("obs_per_stage", C.c_int),
                ("max_batch", C.c_int), ("device", C.c_int), ("max_iter", C.c_int),
                ("dt", C.c_double), ("tol", C.c_double), ("mu_init", C.c_double),
                ("ulim", (C.c_double * 5) * 2), ("xlim", (C.c_double * 9) * 2), ("dulim", (C.c_double * 5) * 2),
                ("L", C.c_int), ("halfspace", (C.c_double * 6) * 8), ("as_written", C.c_int), ("specialise", C.c_int),
                ("generic_budget", C.c_int)]


EXPORTS = ["mmpc_create", "mmpc_destroy", "mmpc_set_weights", "mmpc_set_terminal_xy_equality", "mmpc_reset",
           "mmpc_solve_batch", "mmpc_solve_batch_device", "mmpc_get_u_latest", "mmpc_set_u_latest",
           "mmpc_lds_bytes", "mmpc_problems_per_cu", "mmpc_set_warm_start", "mmpc_set_schedule_hint", "mmpc_set_iteration_budget", "mmpc_resume_batch_device", "mmpc_solve_list_device", "mmpc_suspended_count", "mmpc_last_error", "mmpc_version", "mmpc_ik_batch", "mmpc_ik_batch_device",
           "mmpc_tick_prepare_device", "mmpc_set_obstacle_clock", "mmpc_set_objective_scaling",
           "mmpc_mission_prepare_device", "mmpc_manipulate_prepare_device", "mmpc_solve_rows_device", "mmpc_shift_guess_device",
           "mmpc_mission_round_device", "mmpc_manipulate_round_device", "mmpc_mission_commit_device",
           "mmpc_set_resume_budget", "mmpc_mission_rejoin_device",
           "mmpc_shape_supported", "mmpc_load_shape_library", "mmpc_runs_specialised", "mmpc_set_persistent_grid"]
LISTED_SHAPES = ((KIND_WHOLEBODY, 20, 5), (KIND_WHOLEBODY, 30, 8), (KIND_WHOLEBODY, 20, 3), (KIND_BASE, 15, 3))   # MMPC_FAST_LIST

_lib = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def lib():
    """Loads libmmpc.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "HIP extension %s is missing - build it with __graft_entry__.build() "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        # torch ships its own libamdhip64.so.7 / libhsa-runtime64.so.1; libmmpc.so asks for the same sonames.  Whichever is
        # mapped first serves both, and torch cannot initialise on the system copy ("No HIP GPUs are available" when the first
        # torch.cuda call comes after a solve) - so the process settles on torch's runtime before the library is opened.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.mmpc_create.argtypes = [C.POINTER(MmpcConfig), C.POINTER(C.c_void_p)]
        L.mmpc_destroy.argtypes = [C.c_void_p]
        L.mmpc_set_weights.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_double, _dp]
        L.mmpc_set_terminal_xy_equality.argtypes = [C.c_void_p, C.c_int]
        L.mmpc_reset.argtypes = [C.c_void_p]
        L.mmpc_solve_batch.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp]
        L.mmpc_solve_batch_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 13 + [C.c_void_p]
        L.mmpc_get_u_latest.argtypes = [C.c_void_p, C.c_int, _dp]
        L.mmpc_set_u_latest.argtypes = [C.c_void_p, C.c_int, _dp]
        L.mmpc_lds_bytes.argtypes = [C.c_void_p]
        L.mmpc_problems_per_cu.argtypes = [C.c_void_p]
        L.mmpc_set_warm_start.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
        L.mmpc_set_schedule_hint.argtypes = [C.c_void_p, C.c_int]
        L.mmpc_set_persistent_grid.argtypes = [C.c_void_p, C.c_int]
        L.mmpc_set_iteration_budget.argtypes = [C.c_void_p, C.c_int]
        L.mmpc_resume_batch_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 13 + [C.c_void_p]
        L.mmpc_solve_list_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 13 + [C.c_void_p]
        L.mmpc_suspended_count.argtypes = [C.c_void_p, _ip]
        L.mmpc_last_error.argtypes = [C.c_void_p]
        L.mmpc_last_error.restype = C.c_char_p
        L.mmpc_version.restype = C.c_char_p
        L.mmpc_ik_batch.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip]
        L.mmpc_ik_batch_device.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_void_p]
        L.mmpc_tick_prepare_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 8 + [C.c_void_p]
        L.mmpc_mission_prepare_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 8 + [C.c_void_p]
        L.mmpc_manipulate_prepare_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 11 + [C.c_void_p]
        L.mmpc_shift_guess_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_void_p]
        L.mmpc_mission_round_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 10 + [C.c_longlong, C.c_void_p]
        L.mmpc_manipulate_round_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 13 + [C.c_longlong, C.c_void_p]
        L.mmpc_mission_commit_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_void_p, C.c_void_p]
        L.mmpc_mission_rejoin_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_void_p, C.c_void_p]
        L.mmpc_set_resume_budget.argtypes = [C.c_void_p, C.c_int]
        L.mmpc_solve_rows_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 13 + [C.c_void_p]
        L.mmpc_set_obstacle_clock.argtypes = [C.c_void_p, C.c_void_p]
        L.mmpc_set_objective_scaling.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        L.mmpc_shape_supported.argtypes = [C.c_int, C.c_int, C.c_int]
        L.mmpc_load_shape_library.argtypes = [C.c_char_p]
        L.mmpc_runs_specialised.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def ik_batch(q0, target_xz, device=0):
    """mmpc_ik_batch: q0 (B,3), target_xz (B,2) -> dict(q (B,3), status (B,), iters (B,)).  Runs on the GPU (no fallback)."""
    q0 = np.ascontiguousarray(np.atleast_2d(q0), np.float64)
    t = np.ascontiguousarray(np.atleast_2d(target_xz), np.float64)
    B = q0.shape[0]
    if q0.shape != (B, 3) or t.shape != (B, 2):
        raise ValueError("q0 must be (B,3) and target_xz (B,2)")
    q = np.empty((B, 3)); st = np.empty(B, np.int32); it = np.empty(B, np.int32)
    L = lib()
    rc = L.mmpc_ik_batch(int(device), B, _d(q0), _d(t), _d(q), _i(st), _i(it))
    if rc != 0:
        raise RuntimeError("mmpc_ik_batch failed (%d): %s" % (rc, (L.mmpc_last_error(None) or b"").decode()))
    return dict(q=q, status=st, iters=it)


def prepare_shape(kind, N, M, specialise, planes=0):
    """The `specialise` keyword of Engine, the controllers and DeviceFleet, before the handle is created.  Returns the value of
    mmpc_config.specialise (1: a library with the shape's kernels is loaded in this process, 0: the handle runs what it runs
    without the keyword).
      False     nothing is looked up;
      "cached"  the shape's library csrc/shapes/libmmpc_shape_<kind>_<N>_<M>.so is loaded when it exists and is current (no
                older than the kernel sources, built from them), else the handle runs the generic kernel;
      True      the library is built when it is missing or stale - ONE TO TWO MINUTES of hipcc, once per shape and source
                version - and loaded.  ValueError for a shape outside the specialised envelope (mmpc_shape_supported), with
                half-space planes and for the pose-reference kind.
    A listed shape (LISTED_SHAPES) ignores the argument: it always runs its built-in kernels.  Dense weights and the terminal
    equality fall back to the generic kernel per launch, as they do on a listed shape (Engine.runs_specialised).  A shape
    library is not always the faster kernel: DESIGN.md section 4 has the measured table per shape."""
    if specialise is False or specialise is None:
        return 0
    if specialise is not True and specialise != "cached":
        raise ValueError("specialise must be False, True or 'cached' (got %r)" % (specialise,))
    kind, N, M = int(kind), int(N), int(M)
    if (kind, N, M) in LISTED_SHAPES:
        return 0
    from . import build
    why = None
    if kind == KIND_WHOLEBODY_POSE:
        why = "the pose-reference kind has no specialised kernel"
    elif planes:
        why = "half-space planes run on the generic kernel only"
    elif not build.shape_supported(kind, N, M):
        why = "(kind, N, M) = (%d, %d, %d) is outside the envelope of the specialised kernels (mmpc_shape_supported)" % (kind, N, M)
    if why:
        if specialise is True:
            raise ValueError("specialise=True: " + why)
        return 0
    if specialise is True:
        path = build.build_shape_library(kind, N, M)
        try:
            build.load_shape_library(path)
        except RuntimeError:      # (as new as the sources, yet not built from them: a copied file)
            build.load_shape_library(build.build_shape_library(kind, N, M, force=True))
        return 1
    if not build.shape_library_current(kind, N, M):
        return 0
    try:
        build.load_shape_library(build.shape_library_path(kind, N, M))
    except RuntimeError:
        return 0
    return 1


class Engine:
    """Owns one mmpc_handle (one controller's NLP structure on one GPU)."""

    def __init__(self, kind, N, M, dt, ulim, xlim, dulim, max_batch=1, device=0, obs_per_stage=False,
                 tol=1e-8, mu_init=1.0, max_iter=2000, halfspaces=None, as_written=False, specialise=False, generic_budget=False):
        """specialise: False (default), "cached" or True - run the specialised kernels of a shape library for an unlisted
        (kind, N, M); see prepare_shape (True may compile for one to two minutes).
        generic_budget: mmpc_config.generic_budget - iteration budgets and continuation on the generic kernel too (set_iteration_budget
        then succeeds whichever kernel the handle runs; the list launches accept the budget).  False: the specialised kernels only."""
        self.kind, self.N, self.M = kind, int(N), int(M)
        self.nx, self.nu = (6, 2) if kind == KIND_BASE else (9, 5)
        self.nref = 4 if kind == KIND_WHOLEBODY_POSE else self.nx      # reference row: endpoint pose (x,y,z,psi) or the state
        # obs_per_stage: False (static record), True (table per stage), "motion" (record with velocities + clock); an int is
        # handed to mmpc_create as it is (which refuses anything but 0, 1, 2)
        self.max_batch, self.device, self.max_iter = int(max_batch), int(device), int(max_iter)
        self.obs_mode = 2 if obs_per_stage == "motion" else int(obs_per_stage)
        self.obs_per_stage = "motion" if self.obs_mode == 2 else bool(self.obs_mode)
        cfg = MmpcConfig()
        cfg.kind, cfg.N, cfg.M, cfg.obs_per_stage = kind, self.N, self.M, self.obs_mode
        cfg.max_batch, cfg.device, cfg.max_iter = self.max_batch, self.device, int(max_iter)
        cfg.dt, cfg.tol, cfg.mu_init = float(dt), float(tol), float(mu_init)
        ulim = np.asarray(ulim, float); xlim = np.asarray(xlim, float); dulim = np.asarray(dulim, float)
        for r in range(2):
            for j in range(5):
                cfg.ulim[r][j] = ulim[r, j] if j < self.nu else 0.0
                cfg.dulim[r][j] = dulim[r, j] if j < self.nu else 0.0
            for j in range(9):
                cfg.xlim[r][j] = xlim[r, j] if j < self.nx else 0.0
        cfg.L = 0
        cfg.as_written = int(bool(as_written))
        cfg.generic_budget = int(bool(generic_budget))
        self.generic_budget = bool(generic_budget)
        cfg.specialise = prepare_shape(kind, N, M, specialise, planes=0 if halfspaces is None else len(halfspaces))
        if halfspaces is not None and len(halfspaces):
            hs = np.asarray(halfspaces, float).reshape(-1, 6)
            if hs.shape[0] > 8:
                raise ValueError("at most 8 half-space obstacles")
            cfg.L = hs.shape[0]
            for j in range(cfg.L):
                for a in range(6):
                    cfg.halfspace[j][a] = hs[j, a]
        self._h = C.c_void_p()
        rc = lib().mmpc_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = lib().mmpc_last_error(self._h).decode() if self._h else ""
            if self._h:
                lib().mmpc_destroy(self._h)
                self._h = C.c_void_p()
            raise RuntimeError("mmpc_create failed (%d) %s" % (rc, msg))

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, lib().mmpc_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            lib().mmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def lds_bytes(self):
        return lib().mmpc_lds_bytes(self._h)

    @property
    def runs_specialised(self):
        """mmpc_runs_specialised: the next launch runs a specialised kernel (follows the weights and the terminal equality)"""
        return bool(lib().mmpc_runs_specialised(self._h))

    @property
    def problems_per_cu(self):
        return lib().mmpc_problems_per_cu(self._h)

    def set_weights(self, Q=None, R=None, P=None, S=None, W=None):
        def m(a, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, float)
            if a.shape != (n, n):
                raise ValueError("weight matrix must be %dx%d" % (n, n))
            return a
        Q, P, R, W = m(Q, self.nref), m(P, self.nref), m(R, self.nu), m(W, self.nu)
        Sv = -1.0 if S is None else float(np.ravel(S)[0])
        self._chk(lib().mmpc_set_weights(self._h, _d(Q), _d(R), _d(P), Sv, _d(W)), "mmpc_set_weights")

    def set_warm_start(self, u_guess=None, mu_init=1.0):
        """mmpc_set_warm_start: `u_guess` (B,N,nu) cuda float64 tensor (kept alive by the engine) or None, initial barrier
        parameter `mu_init`.  Applies to the following solve_batch_device calls (their x_guess is the initial X)."""
        if u_guess is not None:
            import torch
            if (not u_guess.is_cuda or u_guess.dtype != torch.float64 or not u_guess.is_contiguous()
                    or u_guess.device.index != self.device or tuple(u_guess.shape[1:]) != (self.N, self.nu)):
                raise ValueError("u_guess must be a contiguous cuda:%d float64 tensor (B, N, nu)" % self.device)
        self._u_guess = u_guess
        self._chk(lib().mmpc_set_warm_start(self._h, C.c_void_p(u_guess.data_ptr()) if u_guess is not None else None,
                                            float(mu_init)), "mmpc_set_warm_start")

    def set_obstacle_clock(self, tick=None):
        """mmpc_set_obstacle_clock (motion handles): `tick` (max_batch,) cuda int64 tensor of per-instance tick counts (kept alive
        by the engine, read by the kernels at launch time) or None (tick 0 for every instance)."""
        if tick is not None:
            import torch
            if (not tick.is_cuda or tick.dtype != torch.int64 or not tick.is_contiguous() or tick.device.index != self.device
                    or tuple(tick.shape) != (self.max_batch,)):
                raise ValueError("tick must be a contiguous cuda:%d int64 tensor (max_batch,) = (%d,)" % (self.device, self.max_batch))
        self._chk(lib().mmpc_set_obstacle_clock(self._h, C.c_void_p(tick.data_ptr()) if tick is not None else None),
                  "mmpc_set_obstacle_clock")
        self._tick = tick

    def set_objective_scaling(self, max_gradient=100.0, scale_out=None):
        """mmpc_set_objective_scaling: IPOPT's gradient-based objective scaling (nlp_scaling_max_gradient = max_gradient; 0 switches
        it off again).  `scale_out`: (max_batch,) cuda float64 tensor that receives the factor of every instance a launch solves
        (kept alive by the engine) or None."""
        if scale_out is not None:
            import torch
            if (not scale_out.is_cuda or scale_out.dtype != torch.float64 or not scale_out.is_contiguous()
                    or scale_out.device.index != self.device or tuple(scale_out.shape) != (self.max_batch,)):
                raise ValueError("scale_out must be a contiguous cuda:%d float64 tensor (max_batch,) = (%d,)" % (self.device, self.max_batch))
        self._chk(lib().mmpc_set_objective_scaling(self._h, float(max_gradient),
                                                   C.c_void_p(scale_out.data_ptr()) if scale_out is not None else None),
                  "mmpc_set_objective_scaling")
        self._scale_out = scale_out

    def set_nlp_scaling(self, nlp_scaling=None, nlp_scaling_max_gradient=100.0):
        """The IPOPT options of the same names, as the controllers take them: None / "none" (off: the engine's default) or
        "gradient-based" (IPOPT's default, which the reference runs under) with its bound on the objective gradient."""
        if nlp_scaling in (None, "none"):
            return self.set_objective_scaling(0.0)
        if nlp_scaling != "gradient-based":
            raise ValueError("nlp_scaling must be None, 'none' or 'gradient-based' (got %r)" % (nlp_scaling,))
        if not float(nlp_scaling_max_gradient) > 0:
            raise ValueError("nlp_scaling_max_gradient must be positive")
        self.set_objective_scaling(float(nlp_scaling_max_gradient))

    def set_schedule_hint(self, mode):
        """mmpc_set_schedule_hint: launch order of a batch's workgroups - 0/False batch order, 1/True (default) longest-first
        by the previous launch's iteration counts when there is one, else by the a-priori difficulty key of the batch's own
        data, 2 always the a-priori key."""
        self._chk(lib().mmpc_set_schedule_hint(self._h, int(mode)), "mmpc_set_schedule_hint")

    def set_persistent_grid(self, n):
        """mmpc_set_persistent_grid: workgroups of the plain launch of a specialised kernel - 0 (default) what the device holds
        at once, n > 0 that many (each solves several instances in turn), n < 0 one workgroup per instance."""
        self._chk(lib().mmpc_set_persistent_grid(self._h, int(n)), "mmpc_set_persistent_grid")

    def set_iteration_budget(self, budget):
        """mmpc_set_iteration_budget: iterations a launch may spend on an instance before it is suspended (0: off).  Needs a
        specialised kernel for the shape, or an engine created with generic_budget."""
        self._chk(lib().mmpc_set_iteration_budget(self._h, int(budget)), "mmpc_set_iteration_budget")

    def set_resume_budget(self, c):
        """mmpc_set_resume_budget: iterations a continuation may spend on a suspended instance before it is suspended again (0, the
        default: resume_batch_device runs to the end).  With c > 0 resume_batch_device can be called again until suspended_count()
        is 0, and a budgeted list launch carries the instances that are still suspended."""
        self._chk(lib().mmpc_set_resume_budget(self._h, int(c)), "mmpc_set_resume_budget")

    def suspended_count(self):
        """mmpc_suspended_count: instances the last budgeted launch - or, under a resume budget, the last continuation - left
        suspended (waits for the handle's launches)."""
        n = C.c_int(0)
        self._chk(lib().mmpc_suspended_count(self._h, C.byref(n)), "mmpc_suspended_count")
        return n.value

    def set_terminal_xy_equality(self, on):
        self._chk(lib().mmpc_set_terminal_xy_equality(self._h, int(bool(on))), "mmpc_set_terminal_xy_equality")

    def reset(self):
        self._chk(lib().mmpc_reset(self._h), "mmpc_reset")

    def obs_shape(self, B):
        if self.obs_mode == 2:
            return (B, self.M, 5)
        return (B, self.N + 1, self.M, 3) if self.obs_per_stage else (B, self.M, 3)

    def solve_batch(self, x_init, traj_ref, u_ref, obs):
        """Host arrays in, host arrays out (dict).  Updates the handle's warm start."""
        N, nx, nu = self.N, self.nx, self.nu
        x_init = np.ascontiguousarray(x_init, float)
        B = x_init.shape[0]
        traj_ref = np.ascontiguousarray(traj_ref, float)
        u_ref = np.ascontiguousarray(u_ref, float)
        obs = np.ascontiguousarray(obs, float)
        if x_init.shape != (B, nx) or traj_ref.shape != (B, N + 1, self.nref) or u_ref.shape != (B, N, nu):
            raise ValueError("shape mismatch: x_init %s traj_ref %s u_ref %s" % (x_init.shape, traj_ref.shape, u_ref.shape))
        if obs.shape != self.obs_shape(B):
            raise ValueError("obs shape %s, expected %s" % (obs.shape, self.obs_shape(B)))
        out = dict(u0=np.empty((B, nu)), X=np.empty((B, N + 1, nx)), U=np.empty((B, N, nu)), s=np.empty((B, N + 1)),
                   status=np.empty(B, np.int32), iters=np.empty(B, np.int32), cost=np.empty(B))
        self._chk(lib().mmpc_solve_batch(self._h, B, _d(x_init), _d(traj_ref), _d(u_ref), _d(obs), _d(out["u0"]),
                                         _d(out["X"]), _d(out["U"]), _d(out["s"]), _i(out["status"]),
                                         _i(out["iters"]), _d(out["cost"])), "mmpc_solve_batch")
        return out

    def get_u_latest(self, B):
        a = np.empty((B, self.N, self.nu))
        self._chk(lib().mmpc_get_u_latest(self._h, B, _d(a)), "mmpc_get_u_latest")
        return a

    def set_u_latest(self, u):
        u = np.ascontiguousarray(u, float)
        self._chk(lib().mmpc_set_u_latest(self._h, u.shape[0], _d(u)), "mmpc_set_u_latest")

    def solve_batch_device(self, x_init, traj_ref, u_ref, u_last, obs, x_guess=None, out=None, stream=None, resume=False, rows=None,
                           either_family=False):
        """torch CUDA float64 tensors in / out, asynchronous on torch's current stream (or `stream`).
        PyTorch is only the owner of the device memory and of the stream here.
        rows = (list, count): mmpc_solve_list_device - only the instances list[0 .. count[0]-1] (int32 cuda tensors: a list of
        row indices and a one-element count, both read on the device) are solved, in list order; the other rows are not touched.
        either_family (with rows): mmpc_solve_rows_device - the same on a handle that runs the generic kernel as well; no budget
        (an engine created with generic_budget: both list launches take either family and honour the budget)."""
        import torch
        if rows is not None and (out is None or resume):
            raise ValueError("a list launch needs the output set of the whole batch (out=...) and is not a continuation")
        N, nx, nu = self.N, self.nx, self.nu
        B = x_init.shape[0]
        for t_, shp in ((x_init, (B, nx)), (traj_ref, (B, N + 1, self.nref)), (u_ref, (B, N, nu)), (u_last, (B, N, nu))):
            if tuple(t_.shape) != shp or t_.dtype != torch.float64 or not t_.is_cuda or not t_.is_contiguous():
                raise ValueError("device tensor must be contiguous cuda float64 of shape %s" % (shp,))
        if tuple(obs.shape) != self.obs_shape(B) or obs.dtype != torch.float64 or not obs.is_cuda or not obs.is_contiguous():
            raise ValueError("obs must be contiguous cuda float64 of shape %s" % (self.obs_shape(B),))
        if x_guess is not None and (tuple(x_guess.shape) != (B, N + 1, nx) or x_guess.dtype != torch.float64
                                    or not x_guess.is_cuda or not x_guess.is_contiguous()):
            raise ValueError("x_guess must be contiguous cuda float64 of shape %s" % ((B, N + 1, nx),))
        dev = x_init.device
        for t_ in (traj_ref, u_ref, u_last, obs, x_guess):
            if t_ is not None and t_.device != dev:
                raise ValueError("all device tensors of one call must live on %s" % dev)
        if getattr(self, "_u_guess", None) is not None and self._u_guess.shape[0] < B:
            raise ValueError("the u_guess set by set_warm_start holds %d instances, this call has %d" % (self._u_guess.shape[0], B))
        if out is None:
            out = dict(X=torch.empty((B, N + 1, nx), dtype=torch.float64, device=dev),
                       U=torch.empty((B, N, nu), dtype=torch.float64, device=dev),
                       s=torch.empty((B, N + 1), dtype=torch.float64, device=dev),
                       status=torch.empty(B, dtype=torch.int32, device=dev),
                       iters=torch.empty(B, dtype=torch.int32, device=dev),
                       cost=torch.empty(B, dtype=torch.float64, device=dev),
                       err=torch.empty(B, dtype=torch.float64, device=dev))
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        p = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None
        if rows is not None:
            lst, cnt = rows
            for t_ in (lst, cnt):
                if t_.dtype != torch.int32 or not t_.is_cuda or not t_.is_contiguous() or t_.device != dev:
                    raise ValueError("rows = (list, count): contiguous int32 tensors on %s" % dev)
            if cnt.numel() != 1 or lst.numel() < 1:
                raise ValueError("rows = (list, count): a one-element count and a list of at least one entry")
            fn, name = (lib().mmpc_solve_rows_device, "mmpc_solve_rows_device") if either_family else (lib().mmpc_solve_list_device, "mmpc_solve_list_device")
            self._chk(fn(self._h, B, p(lst), p(cnt), int(min(lst.numel(), B)), p(x_init), p(traj_ref), p(u_ref), p(u_last),
                         p(x_guess), p(obs), p(out["X"]), p(out["U"]), p(out["s"]), p(out["status"]),
                         p(out["iters"]), p(out["cost"]), p(out["err"]), C.c_void_p(st)), name)
            return out
        fn = lib().mmpc_resume_batch_device if resume else lib().mmpc_solve_batch_device
        self._chk(fn(self._h, B, p(x_init), p(traj_ref), p(u_ref), p(u_last), p(x_guess),
                     p(obs), p(out["X"]), p(out["U"]), p(out["s"]), p(out["status"]),
                     p(out["iters"]), p(out["cost"]), p(out["err"]), C.c_void_p(st)),
                  "mmpc_resume_batch_device" if resume else "mmpc_solve_batch_device")
        return out

    def solve_rows_device(self, rows, x_init, traj_ref, u_ref, u_last, obs, out, x_guess=None, stream=None):
        """mmpc_solve_rows_device: rows = (list, count) as in solve_batch_device, on whichever kernel family the handle runs (the
        generic one included: dense weights, the terminal-xy equality, an unlisted shape); `out` is the output set of the whole
        batch, of which only the listed rows are written.  RuntimeError (-4) when the handle has an iteration budget set - unless the
        engine was created with generic_budget: the budget then holds on either family and resume_batch_device continues the rows."""
        return self.solve_batch_device(x_init, traj_ref, u_ref, u_last, obs, x_guess=x_guess, out=out, stream=stream, rows=rows, either_family=True)

    def resume_batch_device(self, x_init, traj_ref, u_ref, u_last, obs, out, x_guess=None, stream=None):
        """mmpc_resume_batch_device: continues the instances the preceding budgeted solve_batch_device call (same tensors,
        same `out`) left suspended; the other rows of `out` are not touched."""
        return self.solve_batch_device(x_init, traj_ref, u_ref, u_last, obs, x_guess=x_guess, out=out, stream=stream, resume=True)

    def tick_prepare(self, x, tick, U_prev=None, glob=None, obs0=None, vel=None, x_in=None, traj_ref=None, start=None, obs=None,
                     u_guess=None, x_guess=None, stream=None):
        """mmpc_tick_prepare_device: the glue of one receding-horizon tick in one launch, asynchronous on torch's current stream
        (or `stream`).  x (B,9) float64 and tick (B,) int64 are updated in place (advanced with U_prev[:, 0] when U_prev is given);
        every other tensor is optional: glob (B,nglob,9), obs0 (B,M,3), vel (B,M,2) in; x_in (B,9), traj_ref (B,N+1,9), start (B,)
        int32, obs (B,N+1,M,3), u_guess (B,N,5), x_guess (B,N+1,9) out.  Contiguous cuda tensors on one device."""
        import torch
        N, M = self.N, self.M
        B = x.shape[0]
        dev = x.device
        ng = glob.shape[1] if glob is not None and glob.dim() == 3 else 0
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        for name, t_, shp, dt_ in (("x", x, (B, 9), f64), ("tick", tick, (B,), i64), ("U_prev", U_prev, (B, N, 5), f64), ("glob", glob, (B, ng, 9), f64),
                                   ("obs0", obs0, (B, M, 3), f64), ("vel", vel, (B, M, 2), f64), ("x_in", x_in, (B, 9), f64),
                                   ("traj_ref", traj_ref, (B, N + 1, 9), f64), ("start", start, (B,), i32), ("obs", obs, (B, N + 1, M, 3), f64),
                                   ("u_guess", u_guess, (B, N, 5), f64), ("x_guess", x_guess, (B, N + 1, 9), f64)):
            if t_ is None:
                if name in ("x", "tick"):
                    raise ValueError("%s is required" % name)
                continue
            if tuple(t_.shape) != shp or t_.dtype != dt_ or not t_.is_cuda or not t_.is_contiguous() or t_.device != dev:
                raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dt_, shp, dev))
        if u_guess is not None and U_prev is not None and u_guess.data_ptr() == U_prev.data_ptr():
            raise ValueError("u_guess must not be U_prev")
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        p = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None
        self._chk(lib().mmpc_tick_prepare_device(self._h, B, p(x), p(tick), p(U_prev), p(glob), int(ng), p(obs0), p(vel), p(x_in), p(traj_ref),
                                                 p(start), p(obs), p(u_guess), p(x_guess), C.c_void_p(st)), "mmpc_tick_prepare_device")

    def mission_prepare(self, x, tick, phase, lists, counts, U_prev=None, glob=None, obs0=None, vel=None, x_in=None, traj_ref=None, start=None,
                        obs=None, stream=None):
        """mmpc_mission_prepare_device: tick_prepare with the reference's task state machine per robot, asynchronous on torch's
        current stream (or `stream`).  x (B,9) float64, tick (B,) int64 and phase (B,) int32 (PHASE_*) are updated in place; lists
        (3,B) int32 receives the rows to solve per phase, counts (4,) int32 the number of robots in each phase (row p of `lists` and
        counts[p:p+1] are the `rows` of solve_rows_device on phase p's handle).  glob (B,nglob,9) is required; obs0, vel in and x_in,
        traj_ref, start, obs out as in tick_prepare.  Contiguous cuda tensors on one device."""
        import torch
        N, M = self.N, self.M
        B = x.shape[0]
        dev = x.device
        ng = glob.shape[1] if glob is not None and glob.dim() == 3 else 0
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        for name, t_, shp, dt_ in (("x", x, (B, 9), f64), ("tick", tick, (B,), i64), ("phase", phase, (B,), i32), ("lists", lists, (3, B), i32),
                                   ("counts", counts, (4,), i32), ("U_prev", U_prev, (B, N, 5), f64), ("glob", glob, (B, ng, 9), f64),
                                   ("obs0", obs0, (B, M, 3), f64), ("vel", vel, (B, M, 2), f64), ("x_in", x_in, (B, 9), f64),
                                   ("traj_ref", traj_ref, (B, N + 1, 9), f64), ("start", start, (B,), i32), ("obs", obs, (B, N + 1, M, 3), f64)):
            if t_ is None:
                if name in ("x", "tick", "phase", "lists", "counts", "glob"):
                    raise ValueError("%s is required" % name)
                continue
            if tuple(t_.shape) != shp or t_.dtype != dt_ or not t_.is_cuda or not t_.is_contiguous() or t_.device != dev:
                raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dt_, shp, dev))
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        p = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None
        self._chk(lib().mmpc_mission_prepare_device(self._h, B, p(x), p(tick), p(phase), p(U_prev), p(glob), int(ng), p(obs0), p(vel), p(x_in),
                                                    p(traj_ref), p(start), p(obs), p(lists), p(counts), C.c_void_p(st)), "mmpc_mission_prepare_device")

    def manipulate_prepare(self, x, tick, phase, pose, plan, lst, counts, U_prev=None, qgoal=None, ik_status=None, obs0=None, vel=None,
                           x_in=None, traj_ref=None, start=None, obs=None, stream=None):
        """mmpc_manipulate_prepare_device: the manipulate phase of a mission tick, after mission_prepare on the same x (B,9), tick (B,)
        and phase (B,), which are updated in place; asynchronous on torch's current stream (or `stream`).  pose (B,4) float64 is the
        endpoint's pose target; plan (B,nplan,9) receives a robot's joint-space plan at its transition (PHASE_DONE -> PHASE_MANIPULATE)
        and is read afterwards, qgoal (B,3) and ik_status (B,) int32 (optional) the IK's answer and status; lst (B,) int32 receives the
        rows to solve, counts (2,) int32 the robots in PHASE_MANIPULATE and in PHASE_MANIP_DONE ((lst, counts[0:1]) are the `rows` of
        solve_rows_device on the manipulate handle).  obs0, vel in and x_in, traj_ref, start, obs out as in tick_prepare.  Contiguous
        cuda tensors on one device."""
        import torch
        N, M = self.N, self.M
        B = x.shape[0]
        dev = x.device
        npl = plan.shape[1] if plan is not None and plan.dim() == 3 else 0
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        for name, t_, shp, dt_ in (("x", x, (B, 9), f64), ("tick", tick, (B,), i64), ("phase", phase, (B,), i32), ("pose", pose, (B, 4), f64),
                                   ("plan", plan, (B, npl, 9), f64), ("lst", lst, (B,), i32), ("counts", counts, (2,), i32),
                                   ("U_prev", U_prev, (B, N, 5), f64), ("qgoal", qgoal, (B, 3), f64), ("ik_status", ik_status, (B,), i32),
                                   ("obs0", obs0, (B, M, 3), f64), ("vel", vel, (B, M, 2), f64), ("x_in", x_in, (B, 9), f64),
                                   ("traj_ref", traj_ref, (B, N + 1, 9), f64), ("start", start, (B,), i32), ("obs", obs, (B, N + 1, M, 3), f64)):
            if t_ is None:
                if name in ("x", "tick", "phase", "pose", "plan", "lst", "counts"):
                    raise ValueError("%s is required" % name)
                continue
            if tuple(t_.shape) != shp or t_.dtype != dt_ or not t_.is_cuda or not t_.is_contiguous() or t_.device != dev:
                raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dt_, shp, dev))
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        p = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None
        self._chk(lib().mmpc_manipulate_prepare_device(self._h, B, p(x), p(tick), p(phase), p(U_prev), p(pose), int(npl), p(plan), p(qgoal),
                                                       p(ik_status), p(obs0), p(vel), p(x_in), p(traj_ref), p(start), p(obs), p(lst), p(counts),
                                                       C.c_void_p(st)), "mmpc_manipulate_prepare_device")

    def shift_guess(self, phase, U_prev, x_in, u_guess, x_guess, stream=None):
        """mmpc_shift_guess_device: the shifted warm start of a mission tick, asynchronous on torch's current stream (or `stream`).
        U_prev (B,N,5) and x_in (B,9) in; u_guess (B,N,5) = U_prev shifted one stage (the last row twice) and x_guess (B,N+1,9) = the
        plant's roll-out under it from x_in out, as tick_prepare writes them.  phase (B,) int32 or None (every row): a robot whose
        phase is not one of 0, 1, 2, 4 is skipped, none of its rows is read or written.  Contiguous cuda tensors on one device."""
        import torch
        N = self.N
        for name, t_ in (("U_prev", U_prev), ("x_in", x_in), ("u_guess", u_guess), ("x_guess", x_guess)):
            if t_ is None:
                raise ValueError("%s is required" % name)
        B = x_in.shape[0]
        dev = x_in.device
        f64, i32 = torch.float64, torch.int32
        for name, t_, shp, dt_ in (("phase", phase, (B,), i32), ("U_prev", U_prev, (B, N, 5), f64), ("x_in", x_in, (B, 9), f64),
                                   ("u_guess", u_guess, (B, N, 5), f64), ("x_guess", x_guess, (B, N + 1, 9), f64)):
            if t_ is None:
                continue
            if tuple(t_.shape) != shp or t_.dtype != dt_ or not t_.is_cuda or not t_.is_contiguous() or t_.device != dev:
                raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dt_, shp, dev))
        if u_guess.data_ptr() == U_prev.data_ptr():
            raise ValueError("u_guess must not be U_prev")
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        p = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None
        self._chk(lib().mmpc_shift_guess_device(self._h, B, p(phase), p(U_prev), p(x_in), p(u_guess), p(x_guess), C.c_void_p(st)),
                  "mmpc_shift_guess_device")

    def _round_check(self, specs, required, dev):
        for name, t_, shp, dt_ in specs:
            if t_ is None:
                if name in required:
                    raise ValueError("%s is required" % name)
                continue
            if tuple(t_.shape) != shp or t_.dtype != dt_ or not t_.is_cuda or not t_.is_contiguous() or t_.device != dev:
                raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dt_, shp, dev))

    def mission_round(self, x, tick, phase, lists, counts, U_last, hold, solve_phase, tick_limit, glob=None, obs0=None, vel=None, x_in=None,
                      traj_ref=None, start=None, obs=None, stream=None):
        """mmpc_mission_round_device: mission_prepare per robot under the hold word (HOLD_*), asynchronous on torch's current stream (or
        `stream`).  hold (B,) and solve_phase (B,) int32 are updated in place: a robot whose hold is HOLD_NEW (no advance) or HOLD_READY
        (advance with U_last[b, 0]) gets the steps of mission_prepare and, when it enters list p, HOLD_LISTED and solve_phase = p; a
        HOLD_READY robot with tick + 1 >= tick_limit retires (plant step and state machine, no output, no list); every other robot is
        skipped.  U_last (B,N,5) is required; the other tensors as in mission_prepare."""
        import torch
        N, M = self.N, self.M
        B = x.shape[0]
        dev = x.device
        ng = glob.shape[1] if glob is not None and glob.dim() == 3 else 0
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        self._round_check((("x", x, (B, 9), f64), ("tick", tick, (B,), i64), ("phase", phase, (B,), i32), ("lists", lists, (3, B), i32),
                           ("counts", counts, (4,), i32), ("U_last", U_last, (B, N, 5), f64), ("hold", hold, (B,), i32),
                           ("solve_phase", solve_phase, (B,), i32), ("glob", glob, (B, ng, 9), f64), ("obs0", obs0, (B, M, 3), f64),
                           ("vel", vel, (B, M, 2), f64), ("x_in", x_in, (B, 9), f64), ("traj_ref", traj_ref, (B, N + 1, 9), f64),
                           ("start", start, (B,), i32), ("obs", obs, (B, N + 1, M, 3), f64)),
                          ("x", "tick", "phase", "lists", "counts", "U_last", "hold", "solve_phase", "glob"), dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        p = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None
        self._chk(lib().mmpc_mission_round_device(self._h, B, p(x), p(tick), p(phase), p(U_last), p(glob), int(ng), p(obs0), p(vel), p(x_in),
                                                  p(traj_ref), p(start), p(obs), p(lists), p(counts), p(hold), p(solve_phase), int(tick_limit),
                                                  C.c_void_p(st)), "mmpc_mission_round_device")

    def manipulate_round(self, x, tick, phase, pose, plan, lst, counts, U_last, hold, solve_phase, tick_limit, qgoal=None, ik_status=None,
                         obs0=None, vel=None, x_in=None, traj_ref=None, start=None, obs=None, stream=None):
        """mmpc_manipulate_round_device: manipulate_prepare per robot under the hold word, after mission_round on the same tensors;
        asynchronous on torch's current stream (or `stream`).  A HOLD_NEW / HOLD_READY robot gets the steps of manipulate_prepare (a
        HOLD_READY one in PHASE_MANIPULATE advances with U_last[b, 0]) and, when it enters the list, HOLD_LISTED and solve_phase = 4; a
        HOLD_READY robot in PHASE_MANIPULATE with tick + 1 >= tick_limit retires; one the mission round retired at PHASE_DONE
        (HOLD_RETIRED_AT_DONE) makes its transition without outputs and becomes HOLD_RETIRED; every other robot is skipped."""
        import torch
        N, M = self.N, self.M
        B = x.shape[0]
        dev = x.device
        npl = plan.shape[1] if plan is not None and plan.dim() == 3 else 0
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        self._round_check((("x", x, (B, 9), f64), ("tick", tick, (B,), i64), ("phase", phase, (B,), i32), ("pose", pose, (B, 4), f64),
                           ("plan", plan, (B, npl, 9), f64), ("lst", lst, (B,), i32), ("counts", counts, (2,), i32),
                           ("U_last", U_last, (B, N, 5), f64), ("hold", hold, (B,), i32), ("solve_phase", solve_phase, (B,), i32),
                           ("qgoal", qgoal, (B, 3), f64), ("ik_status", ik_status, (B,), i32), ("obs0", obs0, (B, M, 3), f64),
                           ("vel", vel, (B, M, 2), f64), ("x_in", x_in, (B, 9), f64), ("traj_ref", traj_ref, (B, N + 1, 9), f64),
                           ("start", start, (B,), i32), ("obs", obs, (B, N + 1, M, 3), f64)),
                          ("x", "tick", "phase", "pose", "plan", "lst", "counts", "U_last", "hold", "solve_phase"), dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        p = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None
        self._chk(lib().mmpc_manipulate_round_device(self._h, B, p(x), p(tick), p(phase), p(U_last), p(pose), int(npl), p(plan), p(qgoal),
                                                     p(ik_status), p(obs0), p(vel), p(x_in), p(traj_ref), p(start), p(obs), p(lst), p(counts),
                                                     p(hold), p(solve_phase), int(tick_limit), C.c_void_p(st)), "mmpc_manipulate_round_device")

    def mission_commit(self, hold, solve_phase, set, rejoin, out, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist, counters,
                       stream=None):
        """mmpc_mission_commit_device: takes a round's solves (out["U"], out["status"], out["iters"]) into U_last (B,N,5) and row
        [b, tick[b]] of the histories u0 (B,T,5), iters_hist, status_hist, phase_hist (B,T) int32, for the robots with HOLD_LISTED
        (rejoin = 0) or HOLD_SUSPENDED + set (rejoin = 1), which become HOLD_READY - or, with status 3 and rejoin = 0, HOLD_SUSPENDED +
        set.  counters (4,) int32 = committed, suspended, failed, live (over all robots).  Asynchronous on torch's current stream (or
        `stream`)."""
        self._commit_call(hold, solve_phase, set, int(rejoin), out, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist, counters, stream)

    def mission_rejoin(self, hold, solve_phase, set, out, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist, counters, stream=None):
        """mmpc_mission_rejoin_device: mission_commit(rejoin = 1) for a run under a resume budget - a robot with HOLD_SUSPENDED + set
        whose status is still 3 stays suspended, nothing of it is written and counters[1] counts it; every other one rejoins."""
        self._commit_call(hold, solve_phase, set, None, out, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist, counters, stream)

    def _commit_call(self, hold, solve_phase, set, rejoin, out, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist, counters, stream):
        # (rejoin None: mmpc_mission_rejoin_device, which has no such argument)
        import torch
        N = self.N
        B = hold.shape[0]
        dev = hold.device
        T = u0.shape[1] if u0 is not None and u0.dim() == 3 else 0
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        names = ("hold", "solve_phase", "U", "status", "iters", "tick", "phase", "U_last", "u0", "iters_hist", "status_hist", "phase_hist", "counters")
        self._round_check((("hold", hold, (B,), i32), ("solve_phase", solve_phase, (B,), i32), ("U", out["U"], (B, N, 5), f64),
                           ("status", out["status"], (B,), i32), ("iters", out["iters"], (B,), i32), ("tick", tick, (B,), i64),
                           ("phase", phase, (B,), i32), ("U_last", U_last, (B, N, 5), f64), ("u0", u0, (B, T, 5), f64),
                           ("iters_hist", iters_hist, (B, T), i32), ("status_hist", status_hist, (B, T), i32),
                           ("phase_hist", phase_hist, (B, T), i32), ("counters", counters, (4,), i32)), names, dev)
        if U_last.data_ptr() == out["U"].data_ptr():
            raise ValueError("U_last must not be out['U']")
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        p = lambda t_: C.c_void_p(t_.data_ptr())
        tail = (p(out["U"]), p(out["status"]), p(out["iters"]), p(tick), p(phase), p(U_last), p(u0), p(iters_hist), p(status_hist), p(phase_hist),
                int(T), p(counters), C.c_void_p(st))
        if rejoin is None:
            self._chk(lib().mmpc_mission_rejoin_device(self._h, B, p(hold), p(solve_phase), int(set), *tail), "mmpc_mission_rejoin_device")
        else:
            self._chk(lib().mmpc_mission_commit_device(self._h, B, p(hold), p(solve_phase), int(set), int(rejoin), *tail), "mmpc_mission_commit_device")
