/*
 * mmpc.h - C ABI of the MI355X batched MPC solve engine (libmmpc.so).
 *
 * The reference (HsinyuG/mobile-manipulator-mpc) is pure Python: its hot path has no FFI.  The
 * boundary this library replaces is the Python controller object the closed-loop driver calls
 * (interface_wholebody_qref.py:134  `self.controller.solve(current_state, local_traj_ref,
 * local_u_ref)`), i.e. the public surface of controllers/mpc_wholebody_qref.py:6-331 and
 * controllers/mpc_base.py:6-226.  Each entry point below names the reference interface it
 * stands in for.  Plain pointers and sizes only; nothing throws across the ABI; every function
 * returns 0 on success or a negative MMPC_E_* code (text via mmpc_last_error()).
 *
 * Array conventions are the reference's: float64, C order, one record per problem instance:
 *   x_init[B][nx]  traj_ref[B][N+1][nx]  u_ref[B][N][nu]  obs[B][M][3] = (x, y, radius)
 *   (or obs[B][N+1][M][3] when cfg.obs_per_stage = 1: per-stage centres for moving obstacles;
 *    or obs[B][M][5] = (x, y, radius, v_x, v_y) when cfg.obs_per_stage = 2: linear motion, see mmpc_set_obstacle_clock)
 *   X[B][N+1][nx]  U[B][N][nu]  s[B][N+1]
 * whole-body kind: nx=9 [x,y,psi,dx,dy,dpsi,q1,q2,q3], nu=5 [dV,dw,dq1,dq2,dq3]
 * (robot_models/mobile_manipulator.py:22,62-65); base kind: nx=6, nu=2 (robot_models/base.py:26).
 */
#ifndef MMPC_H
#define MMPC_H
#ifdef __cplusplus
extern "C" {
#endif

#define MMPC_KIND_WHOLEBODY 0 /* controllers/mpc_wholebody_qref.py:MPCWholeBody */
#define MMPC_KIND_BASE 1      /* controllers/mpc_base.py:MPCBase */
#define MMPC_KIND_WHOLEBODY_POSE 2 /* controllers/mpc_wholebody.py:MPCWholeBody - whole-body model, the state cost tracks the
                                      endpoint pose forward_tranformation(x)[0] = (x, y, z, psi): traj_ref[B][N+1][4], Q and P
                                      are 4x4 (:11-12,79-80,104-106); circle rows only; X is warm-started too (:134-139) */

#define MMPC_OK 0
#define MMPC_E_ARG (-1)         /* bad argument / unsupported size */
#define MMPC_E_HIP (-2)         /* HIP runtime error */
#define MMPC_E_NODEVICE (-3)    /* no gfx950 device visible */
#define MMPC_E_UNSUPPORTED (-4) /* feature not implemented */

/* per-instance solver status written to status[B] */
#define MMPC_STATUS_CONVERGED 0 /* scaled KKT error <= tol */
#define MMPC_STATUS_MAXITER 1
#define MMPC_STATUS_NUMERIC 2   /* NaN / non-PD even with the Gauss-Newton Hessian; also: NaN or inf in the instance's data (x_init,
                                   references, obstacles, u_last) - detected at the first evaluation, the other instances of the
                                   batch are not affected (opti.solve() raises for such an instance, mpc_wholebody_qref.py:315) */
#define MMPC_STATUS_SUSPENDED 3 /* iteration budget of the launch used up (mmpc_set_iteration_budget): X, U, s hold the current
                                   iterate, mmpc_resume_batch_device continues the solve */

/* per-robot task phase of a fleet mission (mmpc_mission_prepare_device): the task_flag of interface_wholebody_qref.py:146-228 */
#define MMPC_PHASE_MOVE 0     /* 'move': track the nearest window of the global plan */
#define MMPC_PHASE_APPROACH 1 /* 'approach': inside the 2 m box around the goal - hold the goal pose, terminal-xy equality on */
#define MMPC_PHASE_ROTATE 2   /* 'rotate': within 0.2 m of the goal - the same with the weights diag(5,5,5,0,0,1,1,1,1) */
#define MMPC_PHASE_DONE 3     /* 'move finish': reached at 1 cm and 0.5 degrees; the robot is frozen */
#define MMPC_PHASE_MANIPULATE 4 /* 'manipulate': the arm tracks the joint-space plan to the IK's answer (mmpc_manipulate_prepare_device) */
#define MMPC_PHASE_MANIP_DONE 5 /* 'manipulate finish': the endpoint is within 1 cm of its pose target; the robot is frozen */

/* Build-time structure of the NLP = constructor arguments of MPCWholeBody.__init__
 * (mpc_wholebody_qref.py:7-23: N, ulim, xlim, dulim, robot.dt) / MPCBase.__init__
 * (mpc_base.py:7-17).  +-INFINITY marks an absent bound (the reference uses ca.inf). */
typedef struct mmpc_config {
    int kind;          /* MMPC_KIND_* */
    int N;             /* horizon, 1 <= N <= 63, and the LDS slab of the generic kernel must fit (see below) */
    int M;             /* circle obstacles per instance, 0 <= M <= 16 (len(obstacle_list)).
                          Envelope: mmpc_create accepts a config when, besides these ranges, the generic kernel's LDS slab for it
                          (mmpc_lds_bytes of a handle that runs the generic kernel) is at most 160 KiB; otherwise it returns
                          MMPC_E_ARG with an error that names LDS.  Largest N at M = 0 / 5 / 8 / 16:
                            whole-body         49 / 44 / 41 / 35    (obs_per_stage = 1: 49 / 42 / 39 / 32)
                            base               63 / 63 / 63 / 59    (obs_per_stage = 1: 63 / 63 / 63 / 51; N = 63 up to M = 13, 10)
                            pose-reference     55 / 49 / 45 / 38    (obs_per_stage = 1: 55 / 47 / 43 / 35)
                          obs_per_stage = 2 (the motion record: 2 M + 1 doubles more than the static one) has the rows of
                          obs_per_stage = 0:  49 / 44 / 41 / 35,  63 / 63 / 63 / 59 (N = 63 up to M = 13),  55 / 49 / 45 / 38.
                          Half-space planes at N = 20: intended rows fit for L <= 8 at any M; as written, L = 5 fits up to
                          M = 10, L = 6 up to M = 3, L = 7 and 8 never; at N = 30, as-written L = 2 fits with M = 0 only. */
    int obs_per_stage; /* 0: obs[B][M][3]; 1: obs[B][N+1][M][3]; 2: the motion record obs[B][M][5] = (c_x, c_y, r, v_x, v_y) - the
                          kernels form the centre of obstacle m at stage k where they read it, (c_x + v_x t_k, c_y + v_y t_k) with
                          t_k = (double)(tick_b + k) dt, every operation rounded on its own (no fused multiply-add): the very
                          centres of step 5 of mmpc_tick_prepare_device, so a solve equals the solve of that table bit for bit.
                          tick_b comes from mmpc_set_obstacle_clock (default 0: the record is "position now").  Every solve
                          entry point takes the record where it takes the table.  Any other value is MMPC_E_ARG */
    int max_batch;     /* capacity of the device-side buffers: warm start, outputs of the host-pointer call, launch order and - for
                          horizons N >= 21 on a specialised kernel - one 8 (N nu (nx + 1) + N nu (nu - 1) / 2 + 64) byte block of
                          feedback gains per instance (14.9 KB at N = 30: 122 MB for 8192 instances) */
    int device;        /* HIP device ordinal */
    int max_iter;      /* interior-point iteration cap (reference passes ipopt.max_iter 2000, :280) */
    double dt;         /* robot.dt (demo_wholebody_qref.py:10) */
    double tol;        /* scaled KKT tolerance (ipopt tol / acceptable_tol 1e-8, :283) */
    double mu_init;    /* initial barrier parameter */
    double ulim[2][5]; /* [lo|hi][nu] */
    double xlim[2][9]; /* [lo|hi][nx]; psi entry +-INFINITY (mpc_base.py:16 stores 5 columns) */
    double dulim[2][5];
                       /* a limit of magnitude >= 1e19 (in particular +-INFINITY) is no row: IPOPT's nlp_lower/upper_bound_inf,
                          which the reference leaves at their defaults */
    int L;             /* half-space ("manipulation") obstacles, 0..8: len(obstacle_manipulation_list)
                          (mpc_wholebody_qref.py:10,39; demo_wholebody_qref.py:21-33); whole-body kind only */
    double halfspace[8][6]; /* per obstacle: point (3), outward normal (3).  One row per (stage, arm sample point):
                          -max_j n_j.((p_j - 0.03 n_j) - P_i) <= s_k, the INTENDED form of obsAvoidConvex (:57-89) */
    int as_written;    /* L >= 2: the NLP AS WRITTEN - obsAvoidConvex calls subject_to inside its plane loop and keeps one `constr`
                          matrix for all stages (:77-89,156), so besides the intended row it emits, per (stage k >= 1, point i,
                          j < L-1):  -max(c_{k,i,0..j}, c_{k-1,i,j+1..L-1}) <= s_k  (the entries j' > j still hold the PREVIOUS
                          stage's expressions; at k = 0 they hold free variables that can always satisfy the row).  These rows
                          tie x_k to x_{k-1}; the generic kernel carries them.  0: intended rows only */
    int specialise;    /* 0 (the default): the handle runs what it ran before shape libraries existed - the built-in specialised
                          kernels for the four listed shapes, the generic kernel otherwise.  1: when a shape library with the
                          handle's (kind, N, M) has been loaded (mmpc_load_shape_library) before mmpc_create, the handle takes its
                          kernels exactly as it takes a listed shape's; without one it runs the generic kernel.  Ignored for a listed
                          shape, with half-space planes (L > 0) and for the pose-reference kind */
    int generic_budget; /* 0 (the default): iteration budgets and continuation on the specialised kernels only - a handle whose
                          (kind, N, M) runs the generic kernel refuses mmpc_set_iteration_budget, a generic launch ignores a
                          budget.  1: the generic kernel honours the budget too (mmpc_set_iteration_budget: "either family").  The
                          handle then runs the run-time-sized generic kernel and its continuation twin - not the static-LDS
                          instantiation of a listed configuration -, with or without a budget: on those configurations the same
                          solve by another instantiation (equal to rounding, not bit for bit, and slower: profiles/
                          generic_continuation.txt); everywhere else a handle without a budget is bit for bit a default one.  Save area per instance, allocated at the first budget: the
                          larger of the two families' states; the generic one is
                            8 (2 (N+1) nx + N nu + (N+1) + 2 (N+1) R + 64) bytes,  R = 2 nu + 2 nx + M + 4 [whole-body] + 6 [L > 0]
                            + 6 (L-1) [as written] row slots per stage:  26 264 bytes at (whole-body, N = 30, M = 8).
                          Any other value is MMPC_E_ARG */
} mmpc_config;

typedef struct mmpc_handle_s *mmpc_handle;

/* MPCWholeBody.__init__ / MPCBase.__init__ + reset() (mpc_wholebody_qref.py:25-46,142-285):
 * allocates device state, uploads the structure.  Weights start at the reference defaults
 * (:12-16 / mpc_base.py:11-14). */
int mmpc_create(const mmpc_config *cfg, mmpc_handle *out);
int mmpc_destroy(mmpc_handle h);

/* setWeight(Q,R,P,S,W) (mpc_wholebody_qref.py:119-139; mpc_base.py:96-112 where S is `M`):
 * row-major nx*nx / nu*nu matrices (Q, P: 4*4 for MMPC_KIND_WHOLEBODY_POSE); a NULL pointer keeps the current value;
 * S<0 keeps S. */
int mmpc_set_weights(mmpc_handle h, const double *Q, const double *R, const double *P, double S, const double *W);

/* The hard terminal equality the driver injects through controller.opti
 * (interface_wholebody_qref.py:166-167: X[N,:2] == X_ref[N,:2]). */
int mmpc_set_terminal_xy_equality(mmpc_handle h, int on);

/* reset(): clears the warm start (u_latest / x_guess = None, mpc_wholebody_qref.py:164-165). */
int mmpc_reset(mmpc_handle h);

/* solve(x_init, traj_ref, u_ref) for B instances (mpc_wholebody_qref.py:287-331, mpc_base.py:191-226).
 * Host pointers.  Uses the handle's warm start (u_latest, and x_guess for the base and pose-reference kinds) for
 * instances 0..B-1 and replaces it for the instances that CONVERGED - the reference assigns u_latest / x_guess after a
 * successful solve only (:329-330 follow the exception of :315), a failed instance keeps what it had.
 * x_init of the whole-body kind is clipped to xlim (:290-291) inside.
 * Any out_* may be NULL except out_u0.  out_u0[B][nu] = U*[0] (the reference's return value).
 * B = 0 (an empty batch, e.g. the shard of a rank beyond the end of the batch) is a no-op that returns MMPC_OK, here and in
 * the device-pointer calls; B > max_batch is MMPC_E_ARG. */
int mmpc_solve_batch(mmpc_handle h, int B, const double *x_init, const double *traj_ref, const double *u_ref,
                     const double *obs, double *out_u0, double *out_X, double *out_U, double *out_s, int *out_status,
                     int *out_iters, double *out_cost);

/* Same solve on DEVICE pointers (inputs already resident in HBM), asynchronous on `stream`
 * (a hipStream_t, passed as void*; NULL = default stream).  Stateless: u_last is the explicit
 * U_last parameter / U initial guess (:303,:310), x_guess the X initial guess for the base kind
 * (mpc_base.py:200; NULL = tile(x_init), :302).  status/iters are int32 arrays, cost/err float64. */
int mmpc_solve_batch_device(mmpc_handle h, int B, const double *d_x_init, const double *d_traj_ref,
                            const double *d_u_ref, const double *d_u_last, const double *d_x_guess,
                            const double *d_obs, double *d_X, double *d_U, double *d_s, int *d_status, int *d_iters,
                            double *d_cost, double *d_err, void *stream);

/* List launch (specialised kernels, and the generic kernel of a cfg.generic_budget handle; no reference counterpart): the same solve for the instances d_list[0 .. *d_count - 1] only -
 * row indices into the B-row arrays, every index at most once; list and count live in DEVICE memory (the count is read by the
 * kernel: a caller that builds the list on the device never has to synchronise), `capacity` (<= B) bounds the count and is the
 * size of the grid.  An entry outside [0, B) is skipped (nothing can validate a device-side list on the host); a repeated entry is
 * the caller's error (two workgroups would solve the same rows).  Rows that are not listed are neither read nor written.  Instances start in list order (put the ones that
 * are expected to take longest first); the handle's schedule hint is not used and not updated.  With an iteration budget set the
 * listed instances that need more are suspended as in mmpc_solve_batch_device and mmpc_resume_batch_device (same B) continues
 * exactly them.  What it is for: a receding-horizon loop over many robots in which the robots whose solve is finished advance
 * to their next tick while the few suspended ones are still being continued on another stream (bench.py --config c5).
 * A handle that runs the generic kernel is refused (MMPC_E_UNSUPPORTED) unless it was created with cfg.generic_budget, where this
 * call and mmpc_solve_rows_device are the same launch on either family; mmpc_solve_rows_device is the list launch for either family
 * on every handle. */
int mmpc_solve_list_device(mmpc_handle h, int B, const int *d_list, const int *d_count, int capacity, const double *d_x_init,
                           const double *d_traj_ref, const double *d_u_ref, const double *d_u_last, const double *d_x_guess,
                           const double *d_obs, double *d_X, double *d_U, double *d_s, int *d_status, int *d_iters,
                           double *d_cost, double *d_err, void *stream);

/* List launch on whichever kernel the handle runs (no reference counterpart).  Semantics of mmpc_solve_list_device - listed rows
 * only, entries outside [0, B) skipped, unlisted rows neither read nor written, the grid is `capacity` - on a specialised handle (there
 * it IS that launch) and on a generic one: weights the specialised kernels refuse, the terminal-xy equality, an unlisted shape.  No
 * iteration budget: MMPC_E_UNSUPPORTED when the handle has one set (continuations stay with mmpc_solve_list_device) - except on a
 * handle created with cfg.generic_budget, where the budget holds on either family: the listed instances that need more are suspended
 * and mmpc_resume_batch_device (same B) continues exactly them.  What it is
 * for: the per-phase lists of mmpc_mission_prepare_device, whose 'approach' and 'rotate' handles carry the terminal equality. */
int mmpc_solve_rows_device(mmpc_handle h, int B, const int *d_list, const int *d_count, int capacity, const double *d_x_init,
                           const double *d_traj_ref, const double *d_u_ref, const double *d_u_last, const double *d_x_guess,
                           const double *d_obs, double *d_X, double *d_U, double *d_s, int *d_status, int *d_iters,
                           double *d_cost, double *d_err, void *stream);

/* warm start access (self.u_latest, mpc_wholebody_qref.py:165,330): host <-> device copies */
int mmpc_get_u_latest(mmpc_handle h, int B, double *u_latest);
int mmpc_set_u_latest(mmpc_handle h, int B, const double *u_latest);

/* ManipulatorPanda3DoF.inverse_transformation(q_initial_guess, x_target) for B instances
 * (robot_models/manipulator_3DoF.py:79-133; called by Interface.globalPlanManipulator, interface_wholebody_qref.py:286):
 * minimise (x_e(q)-x*)^2 + (z_e(q)-z*)^2 over the joint box of :123, started at q0.  Stateless, no handle:
 * q0[B][3], target_xz[B][2] = (x*, z*) in the arm base frame (the reference asserts y* == 0, :100), out_q[B][3];
 * out_status[B] (0: projected gradient <= 1e-8) and out_iters[B] may be NULL.  Errors: mmpc_last_error(NULL). */
int mmpc_ik_batch(int device, int B, const double *q0, const double *target_xz, double *out_q, int *out_status,
                  int *out_iters);
int mmpc_ik_batch_device(int device, int B, const double *d_q0, const double *d_target_xz, double *d_q, int *d_status,
                         int *d_iters, void *stream);

/* Opt-in warm start for the device-pointer entry point (no reference counterpart: the reference starts every solve from
 * U = U_last, X = tile(x_init), mu = IPOPT's default, mpc_wholebody_qref.py:301-303).  d_u_guess [B][N][nu] (device memory
 * that stays valid until it is replaced or cleared with NULL) becomes the initial U of the following
 * mmpc_solve_batch_device calls - separate from d_u_last, which stays the U_last PARAMETER of the cost and of the rate
 * bounds -, their d_x_guess the initial X, mu_init the initial barrier parameter.  A receding-horizon caller passes the
 * previous optimum shifted by one stage, the roll-out of the dynamics under it, and mu_init = 0.1: the same NLP, solved
 * in fewer than half the iterations.  mmpc_set_warm_start(h, NULL, 1.0) restores the default. */
int mmpc_set_warm_start(mmpc_handle h, const double *d_u_guess, double mu_init);

/* The clock of the motion record (handles created with obs_per_stage = 2; MMPC_E_UNSUPPORTED on any other).  d_tick [max_batch]
 * (device memory, int64, one tick count per instance ROW - list launches and continuations index it like every other
 * per-instance array) stays registered until it is replaced; the kernels read it at launch time, so a caller that keeps the
 * counts current on the device registers it once: it is the very array mmpc_tick_prepare_device advances.  NULL (the default)
 * means tick 0 for every instance.  Range: 0 <= tick < 2^52 (a kernel may form (double)(tick + k) as (double)tick + (double)k,
 * which is exact there).  The call waits for the handle's launches in flight.  A caller with tracker output ("where the
 * obstacle is now and how fast it moves") fills the record per solve and leaves the clock at NULL. */
int mmpc_set_obstacle_clock(mmpc_handle h, const long long *d_tick);

/* Objective scaling, opt-in: IPOPT's nlp_scaling_method = gradient-based with nlp_scaling_max_gradient = max_gradient (and
 * nlp_scaling_min_value = 1e-8) - the defaults the reference's solver runs under, since its option dict names neither
 * (controllers/mpc_wholebody_qref.py:280-285).  Per instance: g = max-norm of the objective's gradient over all of (X, U, s) at the
 * starting point the solve is given (X = tile(clip(x_init)) or the X guess, U = u_last or the opt-in U guess, s = 0; before the
 * bound push), sigma = g > max_gradient ? max(max_gradient / g, 1e-8) : 1, and the solve is the solve of the NLP with objective
 * sigma f: tolerance, termination test, barrier schedule and filter all act on the scaled problem, as in IPOPT.  out_cost stays the
 * unscaled objective f(X, U, s); out_err is the scaled problem's error.  IPOPT's scaling of constraint rows (rows whose gradient
 * exceeds the same bound) is not modelled because it cannot fire: every row of this NLP has a gradient of max-norm at most about 1
 * (circle rows: unit vectors; dynamics rows: 1 and dt; self-collision rows: arm lengths below 1 m), far from any sensible bound.
 * max_gradient = 0 (the default) is off: a solve is then bit for bit the solve without this call.  IPOPT's value is 100.  A negative
 * or non-finite max_gradient is MMPC_E_ARG.  d_scale_out [max_batch] (device memory, may be NULL) stays registered until the next
 * call and receives sigma_b of every instance a launch solves, indexed by instance ROW (list launches and continuations included; a
 * continuation goes on with the factor of the solve it continues).  Applies to every solve entry point and both kernel families; the
 * LDS per problem and the problems per CU do not change.  Keep the setting unchanged between a budgeted launch and its continuations.
 * The call waits for the handle's launches in flight. */
int mmpc_set_objective_scaling(mmpc_handle h, double max_gradient, double *d_scale_out);

/* Launch order of the workgroups (= instances) of a batch.  A batch takes as long as its last wave, so the instances
 * that need the most interior-point iterations should start first.  mode 1 (default): longest-first by the iteration counts
 * of the handle's previous launch of the same B when there is one (a receding-horizon loop solves the same robots every
 * tick), else by an a-priori difficulty key computed from this batch's own data (how deep the reference path cuts into an
 * inflated obstacle disc); mode 2: always the a-priori key (no memory of earlier launches); mode 0: batch order.
 * Results never depend on the order.  No reference counterpart (the reference solves one instance at a time). */
int mmpc_set_schedule_hint(mmpc_handle h, int mode);

/* Grid of the plain launch of a specialised kernel (whole batch, no iteration budget).  That launch is persistent: it starts as
 * many workgroups as the device holds at once (problems per CU x compute units, at most B), and a workgroup that has finished an
 * instance draws the next position of the launch order from a counter of the handle - a slot never waits for the dispatch of a
 * new workgroup.  n = 0 (default): that grid; n > 0: n workgroups (at most B; a small n makes every workgroup solve several
 * instances in turn - tests); n < 0: one workgroup per instance, the launch form of budgeted, continuation and list launches and of
 * the generic kernels, which this call does not change.  Results never depend on n.  Read by the handle's next launch. */
int mmpc_set_persistent_grid(mmpc_handle h, int n);

/* Iteration budget and continuation (specialised kernels; the generic kernel on a handle created with cfg.generic_budget - "either
 * family" below; no reference counterpart - IPOPT runs one instance to the end).  One wave solves one instance, so a launch lasts as long as its slowest instance: a handful of instances that need
 * several hundred iterations (heavy tail of the interior-point iteration count) would hold the results of thousands of
 * finished ones.  With budget > 0, mmpc_solve_batch_device gives every instance at most `budget` iterations per launch;
 * an instance that is not converged by then writes its primal-dual state to the handle (18.7 KB at N=20, M=5) and ends
 * with status MMPC_STATUS_SUSPENDED, X/U/s holding its current iterate.  mmpc_resume_batch_device - same arguments as the
 * launch it continues, any stream - runs the suspended instances to the end (no budget) with one workgroup each;
 * the other instances' outputs are not touched.  A resumed solve executes exactly the iterations the uninterrupted one
 * would have: results are bitwise identical.  mmpc_suspended_count waits for the handle's launches and returns how many
 * instances the last budgeted launch left suspended.  budget = 0 (default) switches the feature off.
 * A continuation belongs to the budgeted launch directly before it on the handle (same B): after any other launch, a first
 * continuation, mmpc_reset or a change of the budget the save areas are stale and mmpc_resume_batch_device returns
 * MMPC_E_UNSUPPORTED instead of overwriting results with the continuation of an older problem.
 * Either family (cfg.generic_budget = 1): the budget is accepted whichever kernel the handle runs, and every launch honours it -
 * also the launches of a listed shape that go to the generic kernel for dense weights or the terminal-xy equality - through
 * mmpc_solve_batch_device, mmpc_solve_list_device and mmpc_solve_rows_device alike; the host-pointer mmpc_solve_batch continues
 * suspended instances at once.  A generic solve parks at the same point of its iteration as a specialised one (after the
 * termination test, before the barrier update), saves the part of its state that outlives an iteration (size: cfg.generic_budget)
 * and its continuation is bit for bit the uninterrupted solve of the same handle.  The family must not change between a budgeted
 * launch and its continuation: mmpc_set_weights and mmpc_set_terminal_xy_equality leave the save areas stale on such a handle
 * (MMPC_E_UNSUPPORTED from mmpc_resume_batch_device), like the events above.  Without a budget the handle behaves like a default one. */
int mmpc_set_iteration_budget(mmpc_handle h, int budget);
int mmpc_resume_batch_device(mmpc_handle h, int B, const double *d_x_init, const double *d_traj_ref, const double *d_u_ref,
                             const double *d_u_last, const double *d_x_guess, const double *d_obs, double *d_X, double *d_U,
                             double *d_s, int *d_status, int *d_iters, double *d_cost, double *d_err, void *stream);
int mmpc_suspended_count(mmpc_handle h, int *count);

/* Resume budget: a continuation that can be suspended again (opt-in; c = 0, the default, is everything above unchanged).  c < 0:
 * MMPC_E_ARG; c > 0 on a handle that takes no iteration budget: MMPC_E_UNSUPPORTED, as mmpc_set_iteration_budget.  Waits for the
 * handle's launches in flight; does not invalidate a pending continuation (a solve is the same bits wherever it is cut).  With c > 0:
 *   - mmpc_resume_batch_device gives every suspended instance at most c further iterations (same striding grid).  An instance that is
 *     still unfinished keeps status 3, its iters is the total so far, X/U/s hold the current iterate and its save area is rewritten;
 *     one that reaches max_iter inside the continuation ends with status 1 (the cap comes first, as in a budgeted launch).  After the
 *     kernel, on the same stream, the handle's list is compacted to the instances whose status is still 3, and the continuation
 *     stays valid: another mmpc_resume_batch_device with the same B and the same arguments continues exactly those, and so on; with
 *     nobody left it is a no-op that returns MMPC_OK.  mmpc_suspended_count: the count after the latest budgeted launch or
 *     continuation.
 *   - A budgeted list launch (mmpc_solve_list_device, mmpc_solve_rows_device) that could have been a continuation - same B, same
 *     kernel family, none of the events above in between - keeps the handle's suspended set S and merges: S := {b in S :
 *     status[b] == 3} united with {b listed : status[b] == 3}, every row once (also where the list names a row twice).  A carried row
 *     that the list names again starts afresh: the launch overwrites its save area, and it is in S by its new status.  The caller
 *     passes the same output buffers, and unchanged inputs for the carried rows ("same arguments as the launch it continues").
 *     A whole-batch budgeted launch replaces S as before.
 *   - The continuation inside the host-pointer mmpc_solve_batch runs to the end whatever c is: that call returns finished solves.
 * The two list buffers and the duplicate guard of the merge (a stamp per row) are allocated with the save areas, at the first
 * budget; no launch gains a host synchronisation, an allocation or a copy (csrc/mmpc_suspend.h). */
int mmpc_set_resume_budget(mmpc_handle h, int c);

/* The glue of one receding-horizon tick for B robots that stay in device memory between ticks (no reference counterpart as
 * a batch; per robot it is the reference's closed loop without the simulator, interface_wholebody_qref.py:100-143).  Whole-body
 * handles created with obs_per_stage = 1 or 2 only (MMPC_E_UNSUPPORTED otherwise); N, M, dt and xlim come from the handle.  One
 * launch, one 64-lane workgroup per robot b:
 *   1. advance - skipped when d_U_prev is NULL (before the first tick): x_b <- f(clip(x_b, xlim), U_prev[b][0]) with the plant
 *      step of robot_models/mobile_manipulator.py (every operation rounded on its own, no fused multiply-add), tick_b <- tick_b + 1;
 *   2. d_x_in[b][9] = clip(x_b, xlim): the x_init of the solve;
 *   3. j = the row of the robot's global plan d_glob[b][nglob][9] nearest to the (unclipped) x_b in columns 0, 1 - the first row
 *      that attains the minimum of sqrt(dx dx + dy dy) (calcLocalRefTraj, :353-396); a robot whose state is not finite takes
 *      j = 0 and its NaN reaches the solve, which reports MMPC_STATUS_NUMERIC for it alone;
 *   4. d_traj_ref[b][k] = glob[b][min(j + k, nglob - 1)], k = 0..N; d_start[b] = j (int32);
 *   5. d_obs[b][k][m] = (c_x + v_x t_k, c_y + v_y t_k, r), t_k = (double)(tick_b + k) dt, from d_obs0[B][M][3] = (c_x, c_y, r) and
 *      d_vel[B][M][2] - on a handle with obs_per_stage = 2 there is no table: d_obs must be NULL (MMPC_E_ARG otherwise) and
 *      the solve forms the same centres from its record and d_tick, registered once with mmpc_set_obstacle_clock;
 *   6. shifted warm start - only when d_U_prev, d_u_guess and d_x_guess are all given: u_guess[k] = U_prev[k + 1] for k < N - 1,
 *      u_guess[N - 1] = U_prev[N - 1]; x_guess[0] = x_in, x_guess[k + 1] = f(x_guess[k], u_guess[k]): the initial point that
 *      mmpc_set_warm_start describes (register d_u_guess there, pass d_x_guess to the solve).  d_u_guess must not be d_U_prev.
 * d_x [B][9] and d_tick [B] (int64) are updated in place and are required (d_tick: when the call advances or writes d_obs).
 * Every output pointer may be NULL and that part is skipped: with d_x, d_tick and d_U_prev alone the call is the plain plant
 * step after the last tick.  The window and the start index need d_glob (nglob >= 1), the table d_obs0 and d_vel; a missing
 * one, or B > max_batch, is MMPC_E_ARG.  B = 0 is a no-op.  Asynchronous on `stream` and ordered against the handle's other
 * launches as they are among themselves; no allocation, copy or synchronisation inside.  A tick of the loop is: this call
 * with the previous tick's d_U as d_U_prev, mmpc_solve_batch_device on its outputs (d_u_last = the same previous d_U) into the
 * other of two output sets, swap. */
int mmpc_tick_prepare_device(mmpc_handle h, int B, double *d_x, long long *d_tick, const double *d_U_prev, const double *d_glob,
                             int nglob, const double *d_obs0, const double *d_vel, double *d_x_in, double *d_traj_ref, int *d_start,
                             double *d_obs, double *d_u_guess, double *d_x_guess, void *stream);

/* mmpc_tick_prepare_device with the reference's task state machine per robot (interface_wholebody_qref.py:146-197, up to 'move
 * finish'; the manipulate phase is not covered).  Handle requirements, argument checks, stream ordering and "no allocation, copy or
 * synchronisation" as there; in addition d_phase [B] (int32, MMPC_PHASE_*, in/out: the phase the robot was last solved in), d_glob,
 * d_lists [3][B] and d_counts [4] (int32) are required, and one hipMemsetAsync of the four counts is queued before the kernel.  Per
 * robot b, with g = glob[b][nglob - 1] (the goal) and p = d_phase[b]:
 *   1. advance as in mmpc_tick_prepare_device, only when d_U_prev is given and p != DONE.  A DONE robot is frozen: its rows of x,
 *      tick, x_in, traj_ref, start and obs are neither read for output nor written, and it appears in no list (a phase code outside
 *      0..3 counts as DONE);
 *   2. state machine on the unclipped state after the advance, in this order, several transitions per call possible:
 *      p == MOVE and |x0 - g0| <= 2 and |x1 - g1| <= 2  =>  APPROACH;   p in {MOVE, APPROACH} and d <= 0.2  =>  ROTATE;
 *      p == ROTATE and |angleDiff(x2, g2)| <= 0.5 pi / 180 and d <= 0.01  =>  DONE,  with d = sqrt(dx dx + dy dy) and angleDiff
 *      the controllers' (fmod(a + pi, 2 pi) - pi of both arguments, then the sign cases).  A comparison with a NaN is false: a
 *      non-finite robot keeps its phase and its NaN reaches the solve;
 *   3. for p != DONE: d_x_in = clip(x); the obstacle table as in mmpc_tick_prepare_device; MOVE: d_start and d_traj_ref are that
 *      call's nearest-row window; APPROACH and ROTATE (calcLocalRefPose, :398-410): traj_ref[k] = g for k = 0..N with column 2
 *      replaced by x2 + angleDiff(g2, x2), start = nglob - 1.  The input reference stays the caller's (the plan's u_ref is zero);
 *   4. d_phase[b] = p; for p < 3 the robot is appended to d_lists[p] (row p of the [3][B] array) at atomicAdd(&d_counts[p], 1), for
 *      p == 3 d_counts[3] is incremented.  Order inside a list is unspecified; entries beyond a count are not written.
 * A mission tick is this call on the 'move' handle followed by mmpc_solve_rows_device(h_p, B, d_lists + p B, d_counts + p, B, ...)
 * on the handles of the three phases, all into one output set at disjoint rows (fleet.py:DeviceFleet.run_mission). */
int mmpc_mission_prepare_device(mmpc_handle h, int B, double *d_x, long long *d_tick, int *d_phase, const double *d_U_prev,
                                const double *d_glob, int nglob, const double *d_obs0, const double *d_vel, double *d_x_in,
                                double *d_traj_ref, int *d_start, double *d_obs, int *d_lists, int *d_counts, void *stream);

/* The manipulate phase of a mission (interface_wholebody_qref.py:204-226): runs after mmpc_mission_prepare_device in every tick, on
 * the same d_x, d_tick and d_phase, and takes on the robots that call left at MMPC_PHASE_DONE (which it counts, with every code >= 3,
 * as frozen).  Handle requirements, argument checks, stream ordering and "no allocation, copy or synchronisation" as there; d_phase,
 * d_pose [B][4] (the endpoint's pose target x, y, z, psi), d_plan [B][nplan][9], d_list [B] and d_counts [2] (int32) are required,
 * nplan must be in 2..2^16 (int(t_manipulate / dt) + 1 rows), d_qgoal [B][3] and d_ik_status [B] (int32) may be NULL, and one
 * hipMemsetAsync of the two counts is queued before the kernel.  Per robot b, with p = d_phase[b] and g = d_pose[b]:
 *   0. p outside {3, 4}: nothing of the robot is read for output or written; p == 5 increments d_counts[1];
 *   1. p == 4 on entry and d_U_prev given: advance as in mmpc_tick_prepare_device (the mission kernel froze this robot).  A robot that
 *      enters with p == 3 was advanced by the mission kernel in the same tick and is not advanced again;
 *   2. p == 3, the transition, on the unclipped state: tx = sqrt(dx dx + dy dy) + 0.007 with dx = g0 - x0, dy = g1 - x1, tz = g2 -
 *      (0.606 + 0.333); q_goal = the arm's inverse kinematics from x[6..8] for the target (tx, tz) (as mmpc_ik_batch_device) into
 *      d_qgoal[b], its status into d_ik_status[b]; d_plan[b][j] = (j / T) (target - x) + x for j < T = nplan - 1 and the target itself
 *      for j = T, target = (x[0..5], q_goal): np.linspace(x, target, nplan).  A failed IK does not stop the robot: the plan goes to the
 *      point the solver returned, the status says so.  Then p = 4;
 *   3. p == 4, finish test on the unclipped state: e = (x0 + (r + b_x) cos x2, x1 + (r + b_x) sin x2, z + b_z), (r, z) the arm's
 *      endpoint in its own frame; sqrt(sum (e_i - g_i)^2) <= 0.01  =>  p = 5: d_counts[1] is incremented, no outputs, frozen from now
 *      on.  A comparison with a NaN is false: a non-finite robot keeps its phase;
 *   4. p == 4 and not finished (calcLocalRefTraj([6, 7, 8])): j = the first plan row that attains the minimum distance to x in columns
 *      6, 7, 8; d_traj_ref[b][k] = plan[b][min(j + k, nplan - 1)], d_start[b] = j, d_x_in[b] = clip(x), the obstacle table as in
 *      mmpc_tick_prepare_device (none on a motion handle); the robot is appended to d_list at atomicAdd(&d_counts[0], 1).  Order
 *      inside the list is unspecified; entries beyond the count are not written;
 *   5. d_phase[b] = p.
 * A mission tick with the manipulate phase is mmpc_mission_prepare_device, this call, and mmpc_solve_rows_device on the handles of the
 * four phases (the fourth: terminal-xy equality, weights diag(500, 500, 500, 0, 0, 1, 1, 1, 1), rows d_list / d_counts), all into one
 * output set at disjoint rows (fleet.py:DeviceFleet.run_mission(manipulate=...)). */
int mmpc_manipulate_prepare_device(mmpc_handle h, int B, double *d_x, long long *d_tick, int *d_phase, const double *d_U_prev,
                                   const double *d_pose, int nplan, double *d_plan, double *d_qgoal, int *d_ik_status,
                                   const double *d_obs0, const double *d_vel, double *d_x_in, double *d_traj_ref, int *d_start,
                                   double *d_obs, int *d_list, int *d_counts, void *stream);

/* The shifted warm start of a mission tick: step 6 of mmpc_tick_prepare_device on its own, for fleets whose x_in is written by
 * mmpc_mission_prepare_device and mmpc_manipulate_prepare_device, which write no guess.  Whole-body handles only
 * (MMPC_KIND_WHOLEBODY; MMPC_E_UNSUPPORTED on any other kind); N and dt come from the handle; obs_per_stage does not matter, the
 * call touches no obstacle.  One launch, one 64-lane workgroup per robot b:
 *   d_u_guess[b][k] = U_prev[b][min(k + 1, N - 1)], k = 0..N-1;
 *   d_x_guess[b][0] = d_x_in[b], d_x_guess[b][k + 1] = f(d_x_guess[b][k], U_prev[b][min(k + 1, N - 1)]) with the plant step of
 *   mmpc_tick_prepare_device (every operation rounded on its own): bit for bit what that call writes from the same x_in and U_prev.
 * d_phase [B] (int32, MMPC_PHASE_*) may be NULL, which means every row; otherwise a robot whose phase is not MOVE, APPROACH, ROTATE
 * or MANIPULATE - the codes that appear in a solve list - is skipped: none of its rows is read or written.  d_U_prev [B][N][5],
 * d_x_in [B][9], d_u_guess [B][N][5] and d_x_guess [B][N+1][9] are required; a missing one, d_u_guess == d_U_prev or B > max_batch
 * is MMPC_E_ARG.  B = 0 is a no-op.  Asynchronous on `stream` and ordered against the handle's other launches as
 * mmpc_tick_prepare_device is; no allocation, copy or synchronisation inside.  A mission tick with the warm start is:
 *   1. mmpc_mission_prepare_device;
 *   2. mmpc_manipulate_prepare_device, when the phase is on;
 *   3. this call with that tick's d_x_in and the previous tick's d_U as d_U_prev;
 *   4. mmpc_solve_rows_device with d_x_guess on the handles of the phases, each with d_u_guess registered through
 *      mmpc_set_warm_start(h, d_u_guess, 0.1) (d_u_last stays the previous d_U: the NLP of the tick is unchanged). */
int mmpc_shift_guess_device(mmpc_handle h, int B, const int *d_phase, const double *d_U_prev, const double *d_x_in,
                            double *d_u_guess, double *d_x_guess, void *stream);

/* ---- Missions under iteration budgets: the glue per robot (csrc/mmpc_round.h).  Under a budget a robot whose solve was suspended is
 * continued on a side stream while the others go on, so only some robots take part in a round.  d_hold [B] (int32) says which: */
#define MMPC_HOLD_NEW 0       /* not solved yet: the next round does not advance the robot */
#define MMPC_HOLD_READY 1     /* d_U_last[b] is its latest optimum: the next round advances it with U_last[b][0] */
#define MMPC_HOLD_LISTED 2    /* in a solve list of the current round (between a round call and the commit) */
#define MMPC_HOLD_RETIRED 3   /* has taken tick_limit ticks and its last plant step: never touched again */
#define MMPC_HOLD_RETIRED_AT_DONE 4 /* retired by the mission round at MMPC_PHASE_DONE: the manipulate round, where one runs, makes
                                     * the output-less transition of the lock step's last call and sets RETIRED; else it stays */
#define MMPC_HOLD_SUSPENDED 8 /* + s: its continuation is in flight on handle set s (s >= 0) */

/* mmpc_mission_prepare_device per robot.  The arguments, handle requirements, argument checks, B = 0, stream ordering, the
 * hipMemsetAsync of the four counts and "no allocation, copy or synchronisation" are that call's; d_U_last [B][N][5] (required)
 * takes the place of d_U_prev, and d_tick, d_hold [B], d_solve_phase [B] (int32) are required as well; tick_limit >= 1 (else
 * MMPC_E_ARG).  Per robot b:
 *   - d_hold[b] neither NEW nor READY: skipped.  Nothing of the robot is read for output or written; it enters no list and no count;
 *   - a robot frozen on entry (phase code outside 0..2) increments d_counts[3] and nothing else, as in the prepare call;
 *   - READY and d_tick[b] + 1 >= tick_limit: the robot retires.  It gets what the prepare call without outputs does to it (plant step
 *     with d_U_last[b][0], state machine; d_x, d_tick, d_phase written), writes no output, enters no list and no count, and
 *     d_hold[b] = RETIRED - or RETIRED_AT_DONE when the step took it to MMPC_PHASE_DONE;
 *   - otherwise exactly the steps of mmpc_mission_prepare_device, with the advance decided per robot: READY advances with
 *     d_U_last[b][0], NEW does not.  A robot that enters list p gets d_hold[b] = LISTED and d_solve_phase[b] = p; one that reaches
 *     MMPC_PHASE_DONE keeps its hold.
 * A round of a mission under budgets is: mmpc_mission_commit_device(rejoin = 1) for the handle set whose continuations have come
 * back; this call; mmpc_manipulate_round_device when the phase is on; mmpc_shift_guess_device with d_solve_phase as d_phase and
 * d_U_last as d_U_prev (shifted warm start); mmpc_solve_rows_device on the budgeted handles of the set with d_u_last = d_U_last;
 * mmpc_mission_commit_device(rejoin = 0); mmpc_resume_batch_device per handle on side streams (fleet.py:DeviceFleet.run_mission).
 * With a resume budget on the set's handles (mmpc_set_resume_budget) mmpc_mission_rejoin_device takes the place of the first call. */
int mmpc_mission_round_device(mmpc_handle h, int B, double *d_x, long long *d_tick, int *d_phase, const double *d_U_last,
                              const double *d_glob, int nglob, const double *d_obs0, const double *d_vel, double *d_x_in,
                              double *d_traj_ref, int *d_start, double *d_obs, int *d_lists, int *d_counts, int *d_hold,
                              int *d_solve_phase, long long tick_limit, void *stream);

/* mmpc_manipulate_prepare_device per robot, after mmpc_mission_round_device on the same arrays; everything not named here is that
 * call's, d_U_last, d_tick, d_hold, d_solve_phase and tick_limit as in mmpc_mission_round_device.  Per robot b:
 *   - d_hold[b] == RETIRED_AT_DONE: the transition of the prepare call without outputs (IK, d_qgoal, d_ik_status, d_plan, finish test,
 *     d_phase = 4 or 5), no output, no list, no count; d_hold[b] = RETIRED;
 *   - d_hold[b] neither NEW nor READY otherwise: skipped as above;
 *   - READY, phase 4 and d_tick[b] + 1 >= tick_limit: retires - the prepare call without outputs (plant step, finish test), no list,
 *     no count, d_hold[b] = RETIRED;
 *   - otherwise exactly the steps of mmpc_manipulate_prepare_device: a READY robot in phase 4 advances with d_U_last[b][0], one at
 *     phase 3 (advanced by the mission round) makes the transition.  A robot that enters the list gets d_hold[b] = LISTED and
 *     d_solve_phase[b] = 4. */
int mmpc_manipulate_round_device(mmpc_handle h, int B, double *d_x, long long *d_tick, int *d_phase, const double *d_U_last,
                                 const double *d_pose, int nplan, double *d_plan, double *d_qgoal, int *d_ik_status,
                                 const double *d_obs0, const double *d_vel, double *d_x_in, double *d_traj_ref, int *d_start,
                                 double *d_obs, int *d_list, int *d_counts, int *d_hold, int *d_solve_phase, long long tick_limit,
                                 void *stream);

/* Takes the solves of a round into the fleet's state: one launch, one 64-lane workgroup per robot.  Whole-body handles only (N comes
 * from the handle).  All arrays are required: d_hold, d_solve_phase [B]; of the output set d_U [B][N][5], d_status, d_iters [B];
 * d_tick [B] (int64), d_phase [B]; d_U_last [B][N][5] (not d_U); the histories d_u0 [B][T][5], d_iters_hist, d_status_hist,
 * d_phase_hist [B][T] (int32), T >= 1; d_counters [4] (int32) = committed, suspended, failed, live, zeroed by one hipMemsetAsync
 * queued before the kernel.  set must be in 0..15, rejoin 0 or 1.  A robot is handled when d_hold[b] == LISTED and rejoin == 0, or
 * d_hold[b] == SUSPENDED + set and rejoin == 1; no other robot is written:
 *   - d_status[b] == 3 (suspended: the budget is used up) and rejoin == 0: d_hold[b] = SUSPENDED + set, d_solve_phase[b] = -1,
 *     counters[1] += 1;
 *   - any other status: d_U_last[b] = d_U[b]; with t = d_tick[b] in 0..T-1, row [b][t] of the histories = d_U[b][0], d_iters[b],
 *     d_status[b], d_phase[b]; d_hold[b] = READY, d_solve_phase[b] = -1; counters[0] += 1, and counters[2] += 1 when the status is
 *     not 0 (a failed solve does not stop a robot).
 * counters[3] counts, over ALL robots after the above, those the run still has work for: hold NEW, LISTED, SUSPENDED + any set, or
 * READY with a phase in {0, 1, 2, 4}.  Missing array, d_U_last == d_U, bad set / rejoin / T or B > max_batch: MMPC_E_ARG.  B = 0 is
 * a no-op.  Asynchronous on `stream`, ordered against the handle's other launches as mmpc_mission_prepare_device is; no allocation,
 * copy or synchronisation inside. */
int mmpc_mission_commit_device(mmpc_handle h, int B, int *d_hold, int *d_solve_phase, int set, int rejoin, const double *d_U,
                               const int *d_status, const int *d_iters, const long long *d_tick, const int *d_phase, double *d_U_last,
                               double *d_u0, int *d_iters_hist, int *d_status_hist, int *d_phase_hist, int T, int *d_counters,
                               void *stream);

/* The rejoin of a run whose continuations can be suspended again (mmpc_set_resume_budget): the arguments of
 * mmpc_mission_commit_device without rejoin, the same argument checks, hipMemsetAsync of the counters and stream ordering.  Handles
 * the robots with d_hold[b] == SUSPENDED + set:
 *   - d_status[b] == 3 (the continuation used up its resume budget): the robot stays SUSPENDED + set, nothing of it is written, and
 *     counters[1] += 1;
 *   - any other status: exactly what mmpc_mission_commit_device(rejoin = 1) does - d_U_last, the histories at d_tick[b], hold READY,
 *     counters[0], and counters[2] on a failed status.
 * counters[3] counts the live robots as there.  In a round it takes the place of mmpc_mission_commit_device(rejoin = 1). */
int mmpc_mission_rejoin_device(mmpc_handle h, int B, int *d_hold, int *d_solve_phase, int set, const double *d_U, const int *d_status,
                               const int *d_iters, const long long *d_tick, const int *d_phase, double *d_U_last, double *d_u0,
                               int *d_iters_hist, int *d_status_hist, int *d_phase_hist, int T, int *d_counters, void *stream);

/* Streams and threads: a handle owns device state that its launches read and write (parameter block, schedule hint,
 * warm start).  Calls on one handle must come from one host thread at a time.  Launches may use different streams:
 * a launch on another stream than the handle's previous one is ordered after it (event wait), and the entry points
 * that change the parameter block or the warm start (mmpc_set_weights, mmpc_set_terminal_xy_equality,
 * mmpc_set_warm_start, mmpc_set_obstacle_clock, mmpc_set_objective_scaling, mmpc_reset, mmpc_get/set_u_latest) wait for the handle's launches in flight first. */

/* bytes of LDS one problem instance occupies (one 64-lane workgroup) */
int mmpc_lds_bytes(mmpc_handle h);
/* problem instances (workgroups) the runtime keeps resident per compute unit for the kernel this handle launches
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor: registers allow 4 - one wave per SIMD -, LDS may allow fewer) */
int mmpc_problems_per_cu(mmpc_handle h);
/* 1 when the handle's next launch runs a specialised kernel, 0 when it runs the generic one.  Decided per launch: dense weights
 * (mmpc_set_weights) and the terminal equality (mmpc_set_terminal_xy_equality) move a handle that has specialised kernels to the
 * generic one and back. */
int mmpc_runs_specialised(mmpc_handle h);

/* Shape libraries: specialised kernels for a (kind, N, M) outside the four built-in shapes, built on demand (build.py:
 * build_shape_library compiles csrc/mmpc_shape.hip for one shape into csrc/shapes/libmmpc_shape_<kind>_<N>_<M>.so, one to two
 * minutes of hipcc) and loaded into the running process.
 * mmpc_shape_supported: 1 when (kind, N, M) lies inside the envelope of the specialised template, 0 otherwise - kinds 0 and 1;
 * whole-body N in 1..20 or 23..31, base N in 1..55 (the number of box slacks a lane multiplies);
 * whole-body M <= 11 up to N = 20 and M <= 16 beyond, base M <= 16 up to N = 31 and M <= 15 beyond; at most 64 KiB of LDS per
 * problem in every obstacle mode.  THE GAP: whole-body N = 21 and 22 have no specialised kernel (the gain ring that the horizons
 * from 21 on keep in LDS during the roll-out does not fit there) - such a config runs the generic kernel, with or without
 * cfg.specialise.  The answer is arithmetic on the template's own bounds; of the shapes it admits, the test suite compiles and
 * runs both upper edges of N, (0, 31, 8) and (1, 55, 1), on the GPU.
 * mmpc_load_shape_library: opens the file at `path` and registers its six kernels ([one launch, budgeted / continuation] x
 * obs_per_stage 0, 1, 2) for the process; handles created AFTERWARDS with cfg.specialise = 1 and that shape run them, budgets,
 * continuations, list launches, the obstacle clock and the objective scaling included.  Handles created earlier keep their
 * kernels; a library is never unloaded; loading a shape that is already there is a no-op that returns MMPC_OK.  MMPC_E_ARG when
 * the file cannot be opened, is not a shape library, was built from other kernel sources than this library (the kernels'
 * parameter block and argument list are no stable ABI: build.py hands both builds a tag of the sources' contents), or holds a
 * shape outside the envelope; the text comes through mmpc_last_error with a NULL handle.  No GPU is needed to load.  Thread-safe. */
int mmpc_shape_supported(int kind, int N, int M);
int mmpc_load_shape_library(const char *path);
const char *mmpc_last_error(mmpc_handle h);
const char *mmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif
