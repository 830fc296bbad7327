"""Device-resident receding-horizon loop over a fleet of B robots with moving obstacles (BASELINE config C5).

The per-robot loop is the reference's (interface_wholebody_qref.py:100-143 with physical_sim=False): local reference
window from the robot's global plan (:353-396), controller.solve(x, traj_ref, u_ref) (:134), plant step x <- f(x, u0)
(:143), warm start per mpc_wholebody_qref.py:301-310 (U init = U_last = the robot's previous optimum, unshifted; X init =
tile(x_init)).  Obstacle j of robot b sits at c_j + v_j (tick + k) dt at stage k of tick `tick` (the build's definition of
the moving-obstacle scenario: README.md:57,85-88 only names the branch).  Everything stays in HBM between ticks; PyTorch
owns the memory and the streams, every solve goes through the C ABI.

Two drivers over the same robots, with bitwise equal per-robot results (tests/test_gpu_parity.py):
  * run_lockstep: all robots solve tick t together, one launch per tick - a tick lasts as long as its slowest robot
    (one wave solves one instance: 200-450 iterations for one robot in 8192 against a mean of 34);
  * run_async: every launch gives a robot at most `budget` iterations (mmpc_set_iteration_budget).  The robots that
    converge within it take their plant step and are launched again in the next round (mmpc_solve_list_device: a device-side
    list of the robots that are ready, longest previous solve first); the few that were suspended are continued on a side
    stream (mmpc_resume_batch_device) while the others move on, and rejoin two rounds later, one tick behind.  Two handles /
    buffer sets alternate, so that a continuation never shares state with the launch beside it.  Robots do not interact, so
    a robot's sequence of solves - and with it every number it produces - is the same as in lock step.

fused=True (lock step and groups): everything between two solves is one HIP kernel (mmpc_tick_prepare_device, csrc/mmpc_tick.h:
plant step, clip, nearest plan point, window, obstacle table) instead of the torch expressions of plant() / inputs(); two output
sets alternate, so the previous optimum is never copied.  warm_start="shifted" (fused only) starts every solve from tick 1 on at
the previous optimum shifted one stage and its roll-out, which the same kernel writes, with mu_0 = 0.1 (mmpc_set_warm_start):
the NLP of every tick is unchanged (U_last stays the previous optimum), the iteration counts are less than half.

obstacles="motion": the handles take the motion record (B, M, 5) = (c_x, c_y, r, v_x, v_y), built once from obs0 and vel, and
a clock of per-robot tick counts (mmpc_set_obstacle_clock) instead of the (B, N+1, M, 3) table of every tick: the solver kernels
form the table's centres where they read them, so every number is the table mode's, bit for bit, and no table is allocated,
written or streamed anywhere.  The clock is the tick tensor the drivers advance anyway (in place; run_async keeps one per buffer
set, filled next to x_in, so that a continuation on the side stream reads the ticks of its own launch).

nlp_scaling="gradient-based" (with nlp_scaling_max_gradient, default 100): IPOPT's objective scaling on every handle of the fleet
(mmpc_set_objective_scaling; sub-fleets of run_groups and the handles of run_async included).  None: the engine's default, off.

run_mission: the reference's task state machine per robot (interface_wholebody_qref.py:146-197: move -> approach -> rotate -> move
finish) instead of a fixed number of 'move' ticks.  A tick is one HIP kernel (mmpc_mission_prepare_device, csrc/mmpc_mission.h: plant
step, state machine, the phase's reference, and per phase a device-side list of the robots in it) and three list launches
(mmpc_solve_rows_device) on three handles - move as created, approach with the terminal-xy equality, rotate with the equality and the
weights diag(5,5,5,0,0,1,1,1,1) - into one output set at disjoint rows.  No host synchronisation; a finished robot is frozen.
manipulate=dict(pose=..., t_manipulate=...) takes the mission on from 'move finish' (:204-226): a second HIP kernel per tick
(mmpc_manipulate_prepare_device, csrc/mmpc_manipulate.h: the endpoint target in the arm frame, the arm's inverse kinematics and the
joint-space plan at the transition, then the finish test and the plan's window in the joint columns) and a fourth list launch on a
fourth handle - the equality and the weights diag(500,500,500,0,0,1,1,1,1) - until the endpoint is within 1 cm of its pose target.
run_mission(..., warm_start="shifted"): the shifted warm start of the lock step in a mission.  From tick 1 on a third HIP kernel per
tick (mmpc_shift_guess_device, csrc/mmpc_guess.h) writes, for the robots the tick solves, the previous optimum shifted one stage and
its roll-out from the tick's x_in; every list launch starts there, with mu_0 = 0.1 on every handle of the mission.  The NLP of every
tick is unchanged (U_last stays the previous optimum).  It is a keyword of run_mission, not of the fleet: it needs no fused=True.

specialise=False / "cached" / True: every handle of the fleet (sub-fleets of run_groups and the handles of run_async included) is
created with this value (_capi.prepare_shape): an unlisted (N, M) then runs the specialised kernels of its shape library - which
also gives it iteration budgets, and with them run_async.  True builds a missing library first: one to two minutes of hipcc.

generic_budget=True: every handle of the fleet (sub-fleets of run_groups, the handles of run_async and the mission handles included)
is created with mmpc_config.generic_budget: iteration budgets and continuation also where a handle runs the generic kernel.  run_async
then works at an unlisted (N, M) without a shape library - no hipcc run -, with the per-robot results of run_lockstep bit for bit.  The
handles run the run-time-sized generic kernel (not the static-LDS instantiation of a listed configuration).

run_mission(..., budget=b, sets=k) on such a fleet: the mission under iteration budgets.  A tick of the lock step lasts as long as its
slowest solve; here a solve that uses up its b iterations is continued on a side stream and its robot rejoins k rounds later, one or
more ticks behind, while every other robot goes on.  The glue between two solves is per robot and stays on the device: a hold word
per robot (MMPC_HOLD_*), the mission and manipulate kernels under it (mmpc_mission_round_device, mmpc_manipulate_round_device), and a
commit kernel that takes a round's solves into U_last and the per-tick histories (mmpc_mission_commit_device; csrc/mmpc_round.h).
k groups of budgeted phase handles alternate; the per-robot results are those of run_mission without a budget, bit for bit.  The
default stays budget=0.  With resume_budget=0 (the default) mmpc_resume_batch_device runs to the end, so a 2 000-iteration solve holds its
handle set until it is through and the main stream waits for it when the set's turn comes round again.

run_mission(..., budget=b, sets=k, resume_budget=c): a continuation gives a solve at most c further iterations (mmpc_set_resume_budget) and
parks it again; its robot stays held on its set (mmpc_mission_rejoin_device), the set's next list launch carries it in the handle's list
of suspended instances and the next continuation goes on with it.  No round waits for more than c iterations of anybody; a carried solve
advances c iterations per k rounds.  Same per-robot results, bit for bit.
"""
import numpy as np


class DeviceFleet:
    def __init__(self, mm, x0, glob, obs0, vel, N=30, device=0, dt=0.1, handles=3, fused=False, warm_start="reference", obstacles="table",
                 nlp_scaling=None, nlp_scaling_max_gradient=100.0, specialise=False, generic_budget=False):
        import torch
        self.nlp_scaling, self.nlp_scaling_max_gradient = nlp_scaling, nlp_scaling_max_gradient
        self.specialise = specialise
        self.generic_budget = bool(generic_budget)
        if obstacles not in ("table", "motion"):
            raise ValueError("obstacles must be 'table' or 'motion', not %r" % (obstacles,))
        self.obstacles = obstacles
        self.motion = obstacles == "motion"
        if warm_start not in ("reference", "shifted"):
            raise ValueError("warm_start must be 'reference' or 'shifted', not %r" % (warm_start,))
        if warm_start == "shifted" and not fused:
            raise ValueError("warm_start='shifted' needs fused=True: the shifted guess and its roll-out are written by the tick kernel")
        self.fused, self.warm_start = bool(fused), warm_start
        self.torch = torch
        self.B, self.N, self.M, self.dt = int(x0.shape[0]), int(N), int(obs0.shape[1]), float(dt)
        self.dev = torch.device("cuda", device)
        B, M = self.B, self.M
        mk = lambda: mm.MPCWholeBody(mm.MobileManipulator(dt), [], [], N=N, max_batch=max(B, 1), device=device, n_obstacles=M,
                                     obs_per_stage="motion" if self.motion else True, nlp_scaling=nlp_scaling,
                                     nlp_scaling_max_gradient=nlp_scaling_max_gradient, specialise=specialise,
                                     generic_budget=self.generic_budget)
        # [0]: lock step (plain kernel); [1], [2]: the two alternating handles of run_async, created on its first call.  A handle owns
        # max_batch rows of device state: staging, warm start, the second-order-correction scratch and - long horizons - the gain
        # blocks (mmpc_create: about 0.5 MB per robot at N = 30, M = 8)
        self._mk = mk
        self.ctrls = [mk()]
        self.engs = [c._engine for c in self.ctrls]
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.f64 = f64
        as_t = lambda a: a.to(self.dev) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.x0, self.glob, self.obs0, self.vel = as_t(x0), as_t(glob), as_t(obs0), as_t(vel)
        self.nglob = self.glob.shape[1]
        self.xlo = torch.from_numpy(self.ctrls[0].xlim[0]).to(self.dev); self.xhi = torch.from_numpy(self.ctrls[0].xlim[1]).to(self.dev)
        self.uref = torch.zeros((B, N, 5), **f64)
        self.karr = torch.arange(N + 1, **f64)
        self.rows = torch.arange(B, device=self.dev)
        if self.motion:
            # the record, once; the lock-step clock: max_batch rows, registered once on the lock-step handle, advanced in place
            self.rec = torch.cat([self.obs0, self.vel], dim=2).contiguous()
            self._clock0 = torch.zeros(max(B, 1), dtype=torch.int64, device=self.dev)
            self.engs[0].set_obstacle_clock(self._clock0)

    # ---- per-robot pieces (torch ops on the device)
    def plant(self, x, u):
        torch = self.torch
        xc = torch.minimum(torch.maximum(x, self.xlo), self.xhi)             # solve() clips x_init (:290-291); the driver steps the clipped state
        c, s, dt = torch.cos(xc[:, 2]), torch.sin(xc[:, 2]), self.dt
        return torch.stack([xc[:, 0] + dt * xc[:, 3], xc[:, 1] + dt * xc[:, 4], xc[:, 2] + dt * xc[:, 5],
                            xc[:, 3] + dt * (u[:, 0] * c - xc[:, 4] * xc[:, 5]),
                            xc[:, 4] + dt * (u[:, 0] * s + xc[:, 3] * xc[:, 5]), xc[:, 5] + dt * u[:, 1],
                            xc[:, 6] + dt * u[:, 2], xc[:, 7] + dt * u[:, 3], xc[:, 8] + dt * u[:, 4]], dim=1)

    def inputs(self, x, tick, loc_out=None, obs_out=None):
        """local reference window (nearest point of the global plan, tail padded: interface_wholebody_qref.py:377-389) and the
        per-stage obstacle table of every robot at ITS tick (a (B,) tensor); obstacles="motion": the record in the table's place
        (the tick reaches the solve through the handle's clock)."""
        torch = self.torch
        B, N = self.B, self.N
        d = torch.linalg.norm(x[:, None, :2] - self.glob[:, :, :2], dim=2)
        start = torch.argmin(d, dim=1)
        idx = torch.clamp(start[:, None] + torch.arange(N + 1, device=self.dev)[None, :], max=self.nglob - 1)
        loc = torch.gather(self.glob, 1, idx[:, :, None].expand(B, N + 1, 9))
        if self.motion:
            if loc_out is not None:
                loc_out.copy_(loc)
                return loc_out, self.rec
            return loc.contiguous(), self.rec
        obs = self.obs0[:, None, :, :].repeat(1, N + 1, 1, 1)
        tk = (tick.to(torch.float64)[:, None] + self.karr[None, :]) * self.dt                   # (B, N+1)
        obs[..., :2] += self.vel[:, None, :, :] * tk[:, :, None, None]
        if loc_out is not None:
            loc_out.copy_(loc); obs_out.copy_(obs)
            return loc_out, obs_out
        return loc.contiguous(), obs.contiguous()

    # ---- lock step
    def run_lockstep(self, T):
        res = {}
        for _ in self._lockstep_ticks(T, res):
            pass
        return res

    def _lockstep_ticks(self, T, res, on_tick=None):
        """run_lockstep as a generator: one tick's work is queued on the current stream per next(); the result lands in `res`.
        on_tick(t, u0): called after tick t's solve is queued, on the stream it runs on, with the (B, 5) first inputs - where a
        multi-rank run issues its all-gather of u0 (bench.py --config c5)"""
        if self.fused:
            return self._fused_ticks(T, res, on_tick)
        return self._torch_ticks(T, res, on_tick)

    def _torch_ticks(self, T, res, on_tick=None):
        torch = self.torch
        B, N = self.B, self.N
        eng = self.engs[0]
        eng.set_iteration_budget(0); eng.reset()
        x = self.x0.clone(); ul = torch.zeros((B, N, 5), **self.f64)
        hist = torch.zeros((B, T, 5), **self.f64); its = torch.zeros((B, T), dtype=torch.int32, device=self.dev)
        tick = self._clock0.zero_()[:B] if self.motion else torch.zeros(B, dtype=torch.int64, device=self.dev)
        out = None
        ok = torch.ones((), dtype=torch.bool, device=self.dev)
        for t in range(T):
            loc, obs = self.inputs(x, tick)
            out = eng.solve_batch_device(x, loc, self.uref, ul, obs, out=out)
            ok = ok & (out["status"] == 0).all()
            ul = out["U"].clone()
            u0 = out["U"][:, 0]
            hist[:, t] = u0; its[:, t] = out["iters"]
            if on_tick is not None:
                on_tick(t, u0)
            x = self.plant(x, u0)
            tick += 1
            res.update(u0=hist, x=x, iters=its, all_converged=ok, rounds=T)
            yield t

    def _fused_ticks(self, T, res, on_tick=None):
        """The same ticks with one mmpc_tick_prepare_device and one solve queued per tick.  x and the tick counters are advanced in
        place by the kernel of the NEXT tick (after the last one by an advance-only call): res["x"] and res["all_converged"] are those of
        the whole run and are there once the generator has yielded T - 1."""
        torch = self.torch
        B, N, M = self.B, self.N, self.M
        dev = self.dev
        eng = self.engs[0]
        shifted = self.warm_start == "shifted"
        if not hasattr(self, "_fsets"):
            mkout = lambda: dict(X=torch.zeros((B, N + 1, 9), **self.f64), U=torch.zeros((B, N, 5), **self.f64), s=torch.zeros((B, N + 1), **self.f64),
                                 status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev),
                                 cost=torch.zeros(B, **self.f64), err=torch.zeros(B, **self.f64))
            self._fsets = [mkout(), mkout()]
            self._fin = dict(x_in=torch.zeros((B, 9), **self.f64), loc=torch.zeros((B, N + 1, 9), **self.f64),
                             obs=self.rec if self.motion else torch.zeros((B, N + 1, M, 3), **self.f64), zero=torch.zeros((B, N, 5), **self.f64))
            if shifted:
                self._fin.update(ug=torch.zeros((B, N, 5), **self.f64), xg=torch.zeros((B, N + 1, 9), **self.f64))
        F = self._fin
        eng.set_iteration_budget(0); eng.reset()
        x = self.x0.clone()
        tick = self._clock0.zero_()[:B] if self.motion else torch.zeros(B, dtype=torch.int64, device=dev)
        # (motion: no table - the tick kernel only advances the clock the solve reads)
        tab = dict() if self.motion else dict(obs0=self.obs0, vel=self.vel, obs=F["obs"])
        hist = torch.zeros((B, T, 5), **self.f64); its = torch.zeros((B, T), dtype=torch.int32, device=dev)
        sts = torch.zeros((B, T), dtype=torch.int32, device=dev)
        ug, xg = (F["ug"], F["xg"]) if shifted else (None, None)
        prev = None
        try:
            for t in range(T):
                out = self._fsets[t & 1]
                warm = shifted and prev is not None
                eng.tick_prepare(x, tick, U_prev=prev, glob=self.glob, x_in=F["x_in"], traj_ref=F["loc"],
                                 u_guess=ug if warm else None, x_guess=xg if warm else None, **tab)
                if warm and t == 1:
                    eng.set_warm_start(ug, 0.1)          # (waits for tick 0's solve: the one host synchronisation of a run)
                eng.solve_batch_device(F["x_in"], F["loc"], self.uref, prev if prev is not None else F["zero"], F["obs"],
                                       x_guess=xg if warm else None, out=out)
                prev = out["U"]
                u0 = prev[:, 0]
                hist[:, t] = u0; its[:, t] = out["iters"]; sts[:, t] = out["status"]
                if on_tick is not None:
                    on_tick(t, u0)
                if t == T - 1:
                    eng.tick_prepare(x, tick, U_prev=prev)                             # the plant step after the last tick
                    res.update(all_converged=(sts == 0).all())
                res.update(u0=hist, x=x, iters=its, rounds=T)
                yield t
        finally:
            if shifted:
                eng.set_warm_start(None, 1.0)

    # ---- missions: the task state machine per robot
    def _mission_handles(self, manipulate=False):
        """[move, approach, rotate]: the states of the reference's one controller in the three phases (:166-167, :175-178; the
        equality is never dropped again).  In motion mode all three read the lock-step clock.  manipulate: and a fourth, the
        controller's state in 'manipulate' (:211-215) - the equality still on, the weights diag(500,500,500,0,0,1,1,1,1)."""
        if not hasattr(self, "_mission_ctrls"):
            N = self.N
            app, rot = self._mk(), self._mk()
            for c in (app, rot):
                c.opti.subject_to(c.X[N, :2] == c.X_ref[N, :2])
                if self.motion:
                    c._engine.set_obstacle_clock(self._clock0)
            W = np.diag([5, 5, 5, 0, 0, 1, 1, 1, 1])
            rot.setWeight(P=W, Q=W)
            self._mission_ctrls = [self.ctrls[0], app, rot]
        if manipulate and len(self._mission_ctrls) < 4:
            N = self.N
            man = self._mk()
            man.opti.subject_to(man.X[N, :2] == man.X_ref[N, :2])
            if self.motion:
                man._engine.set_obstacle_clock(self._clock0)
            W = np.diag([500, 500, 500, 0, 0, 1, 1, 1, 1])
            man.setWeight(P=W, Q=W)
            self._mission_ctrls.append(man)
        return [c._engine for c in self._mission_ctrls[:4 if manipulate else 3]]

    def _mission_set_handles(self, sets, manipulate=False):
        """The handles of a mission under a budget: `sets` groups of [move, approach, rotate(, manipulate)], each group the
        controller states of _mission_handles on controllers of its own (a continuation belongs to the budgeted launch directly before
        it on its handle, so a group is not launched on again before its continuations are back; the lock-step handle runs the glue
        and no solve).  In motion mode every handle reads the lock-step clock: a held robot's tick does not move."""
        if not hasattr(self, "_mission_sets"):
            self._mission_sets = []
        N = self.N
        while len(self._mission_sets) < sets:
            self._mission_sets.append([])
        for grp in self._mission_sets[:sets]:
            while len(grp) < (4 if manipulate else 3):
                p = len(grp)
                c = self._mk()
                if p >= 1:
                    c.opti.subject_to(c.X[N, :2] == c.X_ref[N, :2])
                if p >= 2:
                    W = np.diag([5, 5, 5, 0, 0, 1, 1, 1, 1] if p == 2 else [500, 500, 500, 0, 0, 1, 1, 1, 1])
                    c.setWeight(P=W, Q=W)
                if self.motion:
                    c._engine.set_obstacle_clock(self._clock0)
                grp.append(c)
        return [[c._engine for c in grp[:4 if manipulate else 3]] for grp in self._mission_sets[:sets]]

    def run_mission(self, T, streams=3, on_tick=None, manipulate=None, warm_start="reference", budget=0, sets=2, max_rounds=None, on_round=None, resume_budget=0):
        """T mission ticks.  streams=1: everything on the current stream; streams=3 (default: 0.5 % faster at B = 8192,
        profiles/fleet_mission.txt): the three list launches of a tick on three streams, forked after the mission kernel and joined
        before the next one; the results are bitwise the same.  Returns u0 (B,T,5), iters, status (B,T) - zero
        where a robot was not solved at a tick -, phase (B,T) int32 (the phase a robot was solved in at a tick; 3: not solved),
        counts (T,4) robots per phase, x and final_phase after the plant step that follows the last tick, all_converged over the
        solved rows, rounds.  A failed solve does not raise: the robot goes on with what the solve left.
        on_tick(t, s): called after tick t's solves are queued (and joined), with the tensors of the tick - x, phase, x_in, loc, obs,
        u_last, U; they are rewritten by the next tick, so a caller that keeps them clones them there.
        manipulate=dict(pose=(B,4) array, t_manipulate=2.0): the mission goes on from 'move finish' (phase 3) through 'manipulate' (4)
        to 'manipulate finish' (5, frozen): pose is the endpoint's pose target x, y, z, psi per robot, the joint-space plan has
        int(t_manipulate / dt) + 1 rows.  A tick is then the mission kernel, the manipulate kernel and four list launches (streams=3:
        the fourth on a side stream of its own); a robot counts as solved where phase < 3 or phase == 4.  Returned in addition:
        mcounts (T,2) robots in phases 4 and 5 per tick, qgoal (B,3) and ik_status (B,) int32 of the IK at each robot's transition
        (-1: no transition yet; a failed IK does not raise, the plan goes to the point the solver returned), plan (B,nplan,9); phase
        and final_phase carry the codes 4 and 5, counts stays what the mission kernel writes (column 3: every phase >= 3); on_tick
        also gets plan.
        warm_start="reference" (default): every solve starts by the reference's protocol.  "shifted": tick 0 is the reference protocol's;
        from tick 1 on one more kernel per tick (mmpc_shift_guess_device, after the mission and manipulate kernels, before the
        launches fork) writes the previous optimum shifted one stage and its roll-out from x_in for the robots the tick solves, every
        list launch starts there and every handle of the mission runs with mu_0 = 0.1 (set at tick 1 - each handle waits once for its
        launches in flight, the only host waits of a run - and put back when the run ends, also when on_tick raises).  u_last stays
        the previous optimum, so the NLP of every tick is the same; the returned dict has the same entries; on_tick also gets u_guess
        and x_guess (meaningful from tick 1 on, in the rows of the robots solved at that tick).
        budget=0 (default): the lock step above, unchanged.  budget > 0 (needs a fleet constructed with generic_budget=True; no
        on_tick; `streams` is not used): every list launch gives a solve at most `budget` iterations.  A robot whose solve uses it up is
        continued on a side stream (mmpc_resume_batch_device) and rejoins `sets` rounds later, one or more ticks behind; every other
        robot goes on.  Round r runs on handle set r % sets (sets in 2..4, _mission_set_handles): commit of the set's continuations
        that are back (mmpc_mission_commit_device, rejoin), the mission and manipulate kernels per robot under a hold word
        (mmpc_mission_round_device, mmpc_manipulate_round_device: csrc/mmpc_round.h), the guess kernel on the robots the round solves,
        the list launches, their commit, and the set's continuations on side streams of their own.  All glue runs on the lock-step
        handle, which solves nothing here.  One input set and one output set serve every handle set: the rows of a held robot are
        written by nobody but its continuation.  Robots do not interact, so every number a robot produces is the lock step's, bit
        for bit, indexed by the robot's own tick; phase[b][t] of a tick after a robot froze is its frozen code, counts and mcounts are
        formed from the phase history and equal the lock step's.  The loop ends when no robot has work left (the commit kernel's live
        counter, read on the host from round T on) or after max_rounds (default (sets + 2) T + 8) rounds - then all_converged is
        false.  shifted: set 0 is cold in round 0; every set gets mu_0 = 0.1 before its first warm round (a host wait per handle).
        Returned in addition: rounds, and suspended - the number of solves that used up their budget.  on_round(r, s): called after
        round r is queued, on the main stream, with the tensors counts (4,), counters (4,) = committed, suspended, failed, live of the
        round's commit and, with manipulate, mcounts (2,); the next round rewrites them, so a caller that keeps them clones them.
        resume_budget=0 (default): the above, unchanged.  resume_budget=c > 0 (needs budget > 0): the set's handles get
        mmpc_set_resume_budget(c) for the run - every continuation gives a solve at most c further iterations and parks it again.  A
        round on set s is then: wait for the set's continuations; mmpc_mission_rejoin_device in place of the rejoining commit - a robot
        whose solve is still suspended stays held on set s, every other one rejoins; the round and guess kernels, which skip held
        robots (so the inputs of a carried solve stay what it was launched with); the list launches, which keep the carried rows in
        the handles' lists of suspended instances; their commit; the continuations, of carried and new rows alike.  Returned in
        addition: resuspended - how often a continuation came back still suspended (the sum of counters[1] over the rejoin calls; a
        solve of I > b iterations contributes ceil((I - b) / c) - 1).  A carried solve advances c iterations per `sets` rounds, so a
        solve takes at most sets * ceil(max_iter / c) rounds beyond its first and the default max_rounds becomes
        (sets + 2) T + 8 + T * sets * ceil(max_iter / c): a run whose solves all end cannot stop at the cap."""
        torch = self.torch
        if budget < 0:
            raise ValueError("budget must be >= 0, not %r" % (budget,))
        if sets not in (2, 3, 4):
            raise ValueError("sets must be 2, 3 or 4, not %r" % (sets,))
        if budget > 0 and not self.generic_budget:
            raise ValueError("run_mission(budget=...) needs a fleet constructed with generic_budget=True: the approach, rotate and "
                             "manipulate handles run the generic kernel, which takes a budget only then")
        if resume_budget < 0:
            raise ValueError("resume_budget must be >= 0, not %r" % (resume_budget,))
        if resume_budget > 0 and budget == 0:
            raise ValueError("resume_budget=%r needs budget > 0: only a solve that was suspended is continued" % (resume_budget,))
        if budget == 0 and on_round is not None:
            raise ValueError("on_round belongs to a run under a budget; the lock step calls on_tick")
        if budget > 0 and on_tick is not None:
            raise ValueError("on_tick has no meaning under a budget: the robots of a round are at different ticks (use budget=0)")
        if self.warm_start != "reference":
            raise ValueError("a fleet constructed with warm_start='shifted' runs its lock step that way; a mission takes the switch as "
                             "its own keyword: run_mission(..., warm_start='shifted') on a fleet constructed with the default")
        if warm_start not in ("reference", "shifted"):
            raise ValueError("warm_start must be 'reference' or 'shifted', not %r" % (warm_start,))
        shifted = warm_start == "shifted"
        if streams not in (1, 3):
            raise ValueError("streams must be 1 or 3, not %r" % (streams,))
        B, N, M = self.B, self.N, self.M
        dev = self.dev
        manip = manipulate is not None
        if manip:
            pose = np.ascontiguousarray(manipulate["pose"].cpu().numpy() if torch.is_tensor(manipulate["pose"]) else manipulate["pose"], np.float64)
            if pose.shape != (B, 4):
                raise ValueError("manipulate['pose'] must have shape %r (x, y, z, psi of the endpoint per robot), not %r" % ((B, 4), pose.shape))
            t_man = float(manipulate.get("t_manipulate", 2.0))
            if not t_man >= self.dt:
                raise ValueError("manipulate['t_manipulate'] must be at least dt = %g (a plan of two rows), not %r" % (self.dt, t_man))
            nplan = int(t_man / self.dt) + 1
            if nplan > 1 << 16:
                raise ValueError("manipulate['t_manipulate'] gives a plan of %d rows; at most 65536" % nplan)
        engs = self._mission_handles(manip) if budget == 0 else None
        f64, i32 = self.f64, dict(dtype=torch.int32, device=dev)
        if not hasattr(self, "_msets"):
            mkout = lambda: dict(X=torch.zeros((B, N + 1, 9), **f64), U=torch.zeros((B, N, 5), **f64), s=torch.zeros((B, N + 1), **f64),
                                 status=torch.zeros(B, **i32), iters=torch.zeros(B, **i32), cost=torch.zeros(B, **f64), err=torch.zeros(B, **f64))
            self._msets = [mkout(), mkout()]
            self._min = dict(x_in=torch.zeros((B, 9), **f64), loc=torch.zeros((B, N + 1, 9), **f64),
                             obs=self.rec if self.motion else torch.zeros((B, N + 1, M, 3), **f64), zero=torch.zeros((B, N, 5), **f64),
                             phase=torch.zeros(B, **i32), lists=torch.zeros((3, B), **i32), counts=torch.zeros(4, **i32))
            self._mside = [torch.cuda.Stream(device=dev) for _ in range(3)]
        F = self._min
        if shifted and "ug" not in F:
            F.update(ug=torch.zeros((B, N, 5), **f64), xg=torch.zeros((B, N + 1, 9), **f64))
        ug, xg = (F["ug"], F["xg"]) if shifted else (None, None)
        if manip:
            if len(self._mside) < 4:
                self._mside.append(torch.cuda.Stream(device=dev))
            if getattr(self, "_manip", None) is None or self._manip["plan"].shape[1] != nplan:
                self._manip = dict(plan=torch.zeros((B, nplan, 9), **f64), pose=torch.zeros((B, 4), **f64), qgoal=torch.zeros((B, 3), **f64),
                                   ik_status=torch.zeros(B, **i32), list=torch.zeros(B, **i32), counts=torch.zeros(2, **i32))
            G = self._manip
            G["pose"].copy_(torch.from_numpy(pose)); G["plan"].zero_(); G["qgoal"].zero_(); G["ik_status"].fill_(-1)
            mcnts = torch.zeros((T, 2), **i32)
            mkw = dict(pose=G["pose"], plan=G["plan"], lst=G["list"], counts=G["counts"], qgoal=G["qgoal"], ik_status=G["ik_status"])
        if budget > 0:
            return self._mission_rounds(T, int(budget), sets, max_rounds, shifted, F, G if manip else None, mkw if manip else None, on_round, int(resume_budget))
        for e in engs:
            e.set_iteration_budget(0); e.reset()
        x = self.x0.clone()
        tick = self._clock0.zero_()[:B] if self.motion else torch.zeros(B, dtype=torch.int64, device=dev)
        phase, lists, counts = F["phase"].zero_(), F["lists"], F["counts"]
        tab = dict() if self.motion else dict(obs0=self.obs0, vel=self.vel, obs=F["obs"])
        hist = torch.zeros((B, T, 5), **f64)
        its, sts, phs = torch.zeros((B, T), **i32), torch.zeros((B, T), **i32), torch.zeros((B, T), **i32)
        cnts = torch.zeros((T, 4), **i32)
        main = torch.cuda.current_stream(dev)
        prev = None
        try:
            for t in range(T):
                out = self._msets[t & 1]
                engs[0].mission_prepare(x, tick, phase, lists, counts, U_prev=prev, glob=self.glob, x_in=F["x_in"], traj_ref=F["loc"], **tab)
                if manip:
                    engs[0].manipulate_prepare(x, tick, phase, U_prev=prev, x_in=F["x_in"], traj_ref=F["loc"], **mkw, **tab)
                ul = prev if prev is not None else F["zero"]
                warm = shifted and prev is not None
                if warm:
                    engs[0].shift_guess(phase, prev, F["x_in"], ug, xg)
                    if t == 1:
                        for e in engs:
                            e.set_warm_start(ug, 0.1)        # (waits for the handle's launches in flight: the host waits of a run)
                kw = dict(x_guess=xg) if warm else {}
                if streams == 3:
                    ev = torch.cuda.Event(); ev.record(main)
                for p, e in enumerate(engs):
                    rows = (lists[p], counts[p:p + 1]) if p < 3 else (G["list"], G["counts"][0:1])
                    if streams == 3:
                        side = self._mside[p]
                        side.wait_event(ev)
                        e.solve_rows_device(rows, F["x_in"], F["loc"], self.uref, ul, F["obs"], out, stream=side.cuda_stream, **kw)
                        evp = torch.cuda.Event(); evp.record(side); main.wait_event(evp)
                    else:
                        e.solve_rows_device(rows, F["x_in"], F["loc"], self.uref, ul, F["obs"], out, **kw)
                prev = out["U"]
                solved = (phase < 3) | (phase == 4) if manip else phase < 3
                hist[:, t] = torch.where(solved[:, None], prev[:, 0], hist[:, t])
                its[:, t] = torch.where(solved, out["iters"], its[:, t]); sts[:, t] = torch.where(solved, out["status"], sts[:, t])
                phs[:, t] = phase; cnts[t] = counts
                if manip:
                    mcnts[t] = G["counts"]
                if on_tick is not None:
                    s = dict(x=x, phase=phase, x_in=F["x_in"], loc=F["loc"], obs=F["obs"], u_last=ul, U=prev)
                    if manip:
                        s["plan"] = G["plan"]
                    if shifted:
                        s.update(u_guess=ug, x_guess=xg)
                    on_tick(t, s)
        finally:
            if shifted:
                for e in engs:
                    e.set_warm_start(None, 1.0)
        if prev is not None:
            engs[0].mission_prepare(x, tick, phase, lists, counts, U_prev=prev, glob=self.glob)     # the plant step after the last tick
            if manip:
                engs[0].manipulate_prepare(x, tick, phase, U_prev=prev, **mkw)                     # ... of the robots in 'manipulate'
        res = dict(u0=hist, iters=its, status=sts, phase=phs, counts=cnts, x=x, final_phase=phase.clone(), all_converged=(sts == 0).all(), rounds=T)
        if manip:
            res.update(mcounts=mcnts, qgoal=G["qgoal"].clone(), ik_status=G["ik_status"].clone(), plan=G["plan"].clone())
        return res

    def _mission_rounds(self, T, budget, sets, max_rounds, shifted, F, G, mkw, on_round=None, resume_budget=0):
        """run_mission under a budget (its docstring): F, G the input buffers and the manipulate state run_mission has set up."""
        torch = self.torch
        B, N = self.B, self.N
        dev = self.dev
        manip = G is not None
        f64, i32 = self.f64, dict(dtype=torch.int32, device=dev)
        glue = self.engs[0]
        groups = self._mission_set_handles(sets, manip)
        if not hasattr(self, "_mround"):
            self._mround = dict(U_last=torch.zeros((B, N, 5), **f64), hold=torch.zeros(B, **i32), solve_phase=torch.zeros(B, **i32),
                                counters=torch.zeros(4, **i32), sides=[])
        R = self._mround
        while len(R["sides"]) < sets:
            R["sides"].append([])
        for sd in R["sides"][:sets]:
            while len(sd) < len(groups[0]):
                sd.append(torch.cuda.Stream(device=dev))
        out = self._msets[0]
        for grp in groups:
            for e in grp:
                e.set_iteration_budget(budget); e.reset()
                if resume_budget > 0:
                    e.set_resume_budget(resume_budget)
        x = self.x0.clone()
        tick = self._clock0.zero_()[:B] if self.motion else torch.zeros(B, dtype=torch.int64, device=dev)
        phase, lists, counts = F["phase"].zero_(), F["lists"], F["counts"]
        hold, sp, U_last, counters = R["hold"].zero_(), R["solve_phase"].fill_(-1), R["U_last"].zero_(), R["counters"]
        tab = dict() if self.motion else dict(obs0=self.obs0, vel=self.vel, obs=F["obs"])
        ug, xg = (F["ug"], F["xg"]) if shifted else (None, None)
        hist = torch.zeros((B, T, 5), **f64)
        its, sts, phs = torch.zeros((B, T), **i32), torch.zeros((B, T), **i32), torch.full((B, T), -1, **i32)
        nsusp, nagain = torch.zeros((), dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        main = torch.cuda.current_stream(dev)
        back = [None] * sets                 # per set: the events of its continuations in flight
        warm_set = [False] * sets
        cap = max_rounds if max_rounds is not None else (sets + 2) * T + 8
        if max_rounds is None and resume_budget > 0:
            # (a carried solve advances resume_budget iterations per `sets` rounds and ends at max_iter at the latest)
            cap += T * sets * -(-max(int(e.max_iter) for e in groups[0]) // resume_budget)
        commit = lambda s, rejoin: glue.mission_commit(hold, sp, s, rejoin, out, tick, phase, U_last, hist, its, sts, phs, counters)
        r, live = 0, -1
        try:
            while True:
                s = r % sets
                engs = groups[s]
                if back[s] is not None:
                    # the continuations of round r - sets (same handles) are finished: their robots rejoin
                    for ev in back[s]:
                        main.wait_event(ev)
                    back[s] = None
                    if resume_budget > 0:
                        # (a robot whose solve is still suspended stays held on this set: the list launches below carry it)
                        glue.mission_rejoin(hold, sp, s, out, tick, phase, U_last, hist, its, sts, phs, counters)
                        nagain += counters[1]
                    else:
                        commit(s, 1)
                glue.mission_round(x, tick, phase, lists, counts, U_last, hold, sp, T, glob=self.glob, x_in=F["x_in"], traj_ref=F["loc"], **tab)
                if manip:
                    glue.manipulate_round(x, tick, phase, U_last=U_last, hold=hold, solve_phase=sp, tick_limit=T, x_in=F["x_in"],
                                          traj_ref=F["loc"], **mkw, **tab)
                warm = shifted and r >= 1        # (only round 0 solves robots that have no optimum yet)
                if warm:
                    glue.shift_guess(sp, U_last, F["x_in"], ug, xg)
                    if not warm_set[s]:
                        for e in engs:
                            e.set_warm_start(ug, 0.1)        # (waits for the handle's launches in flight)
                        warm_set[s] = True
                kw = dict(x_guess=xg) if warm else {}
                for p, e in enumerate(engs):
                    rows = (lists[p], counts[p:p + 1]) if p < 3 else (G["list"], G["counts"][0:1])
                    e.solve_rows_device(rows, F["x_in"], F["loc"], self.uref, U_last, F["obs"], out, **kw)
                commit(s, 0)
                nsusp += counters[1]
                ev = torch.cuda.Event(); ev.record(main)
                back[s] = []
                for p, e in enumerate(engs):
                    side = R["sides"][s][p]
                    side.wait_event(ev)
                    e.resume_batch_device(F["x_in"], F["loc"], self.uref, U_last, F["obs"], out, stream=side.cuda_stream, **kw)
                    evp = torch.cuda.Event(); evp.record(side)
                    back[s].append(evp)
                if on_round is not None:
                    on_round(r, dict(counts=counts, counters=counters, **(dict(mcounts=G["counts"]) if manip else {})))
                r += 1
                if r >= T:
                    live = int(counters[3])
                    if live == 0 or r >= cap:
                        break
        finally:
            for s in range(sets):
                for ev in back[s] or ():
                    ev.synchronize()
                for e in groups[s]:
                    e.set_iteration_budget(0)
                    if resume_budget > 0:
                        e.set_resume_budget(0)
                    if warm_set[s]:
                        e.set_warm_start(None, 1.0)
        final = phase.clone()
        phs = torch.where(phs < 0, final[:, None], phs)          # a tick after a robot froze: its frozen code
        drive = torch.stack([(phs == p).sum(dim=0) for p in range(3)], dim=1).to(torch.int32)
        cnts = torch.cat([drive, (B - drive.sum(dim=1, keepdim=True)).to(torch.int32)], dim=1)
        res = dict(u0=hist, iters=its, status=sts, phase=phs, counts=cnts, x=x, final_phase=final,
                   all_converged=(sts == 0).all() & torch.tensor(live == 0, device=dev), rounds=r, suspended=int(nsusp), resuspended=int(nagain))
        if manip:
            res.update(mcounts=torch.stack([(phs == 4).sum(dim=0), (phs == 5).sum(dim=0)], dim=1).to(torch.int32), qgoal=G["qgoal"].clone(),
                       ik_status=G["ik_status"].clone(), plan=G["plan"].clone())
        return res

    # ---- groups in lock step, out of phase
    def run_groups(self, T, groups=2, priority=True, on_tick=None):
        """The fleet as `groups` contiguous groups of robots, each in lock step on its own HIP stream and handle, the streams at
        descending priority: the workgroup dispatcher serves the first group's launch first and fills the slots its tail leaves
        empty - a tick lasts as long as its slowest robot, 200-450 iterations against a mean of 34 - with the other group's
        launch, so the groups run out of phase and one group's tail overlaps the other's bulk.  Robots do not interact: every
        robot's numbers are those of run_lockstep (tests/test_gpu_parity.py).  Same reference protocol per robot.
        on_tick(g, lo, hi, t, u0): called per group and tick on the group's stream (see _lockstep_ticks) - a multi-rank run gathers
        the first inputs of group g's robots [lo, hi) there, so that a tick's exchange waits for the slowest robot of ONE group of
        one rank, not of the whole node."""
        torch = self.torch
        G = int(groups)
        if not hasattr(self, "_groups") or len(self._groups) != G or getattr(self, "_groups_pr", True) != bool(priority):
            self._groups_pr = bool(priority)
            from . import sharding
            import sys
            mm = sys.modules[__package__]
            lo_pr, hi_pr = torch.cuda.Stream.priority_range() if hasattr(torch.cuda.Stream, "priority_range") else (0, -1)
            self._groups = []
            for g in range(G):
                lo, hi = sharding.shard_bounds(self.B, G, g)
                sub = DeviceFleet(mm, self.x0[lo:hi], self.glob[lo:hi], self.obs0[lo:hi], self.vel[lo:hi], N=self.N, device=self.dev.index, dt=self.dt,
                                  handles=1, fused=self.fused, warm_start=self.warm_start, obstacles=self.obstacles,
                                  nlp_scaling=self.nlp_scaling, nlp_scaling_max_gradient=self.nlp_scaling_max_gradient,
                                  specialise=self.specialise, generic_budget=self.generic_budget)
                # (priority: lower number = served first; the last group runs at the default priority)
                pr = (max(hi_pr, min(lo_pr, 0 - (G - 1 - g))) if hi_pr < 0 else 0) if priority else 0
                self._groups.append((lo, hi, sub, torch.cuda.Stream(device=self.dev, priority=pr)))
        main = torch.cuda.current_stream(self.dev)
        ev0 = torch.cuda.Event(); ev0.record(main)
        res = [dict() for _ in range(G)]
        gens = []
        for g, (lo, hi, sub, st) in enumerate(self._groups):
            st.wait_event(ev0)
            with torch.cuda.stream(st):
                cb = None if on_tick is None else (lambda t, u0, g=g, lo=lo, hi=hi: on_tick(g, lo, hi, t, u0))
                gens.append(sub._lockstep_ticks(T, res[g], cb))
        try:
            for t in range(T):
                for g, (lo, hi, sub, st) in enumerate(self._groups):
                    with torch.cuda.stream(st):
                        next(gens[g])
        finally:
            for gen in gens:             # (a fused sub-fleet puts its handle's warm start back when its generator ends)
                gen.close()
        for g, (lo, hi, sub, st) in enumerate(self._groups):
            ev = torch.cuda.Event(); ev.record(st); main.wait_event(ev)
            for v in res[g].values():        # (allocated on the group's stream, read on the caller's from here on)
                if torch.is_tensor(v):
                    v.record_stream(main)
        ok = res[0]["all_converged"]
        for r_ in res[1:]:
            ok = ok & r_["all_converged"]
        return dict(u0=torch.cat([r_["u0"] for r_ in res]), x=torch.cat([r_["x"] for r_ in res]), iters=torch.cat([r_["iters"] for r_ in res]),
                    all_converged=ok, rounds=T, groups=G)

    # ---- asynchronous
    def run_async(self, T, budget=48, max_rounds=None):
        if self.fused:
            raise ValueError("run_async has no fused form: its robots advance under per-robot masks, the tick kernel steps a whole "
                             "batch (use run_lockstep / run_groups, or fused=False)")
        torch = self.torch
        B, N, M = self.B, self.N, self.M
        dev = self.dev
        main = torch.cuda.current_stream(dev)
        while len(self.ctrls) < 3:
            self.ctrls.append(self._mk()); self.engs.append(self.ctrls[-1]._engine)
        if not hasattr(self, "_sets"):
            self._sides = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
            self._sets = []
            for s in range(2):
                o = dict(X=torch.zeros((B, N + 1, 9), **self.f64), U=torch.zeros((B, N, 5), **self.f64), s=torch.zeros((B, N + 1), **self.f64),
                         status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev),
                         cost=torch.zeros(B, **self.f64), err=torch.zeros(B, **self.f64))
                self._sets.append(dict(out=o, x_in=torch.zeros((B, 9), **self.f64), loc=torch.zeros((B, N + 1, 9), **self.f64),
                                       obs=self.rec if self.motion else torch.zeros((B, N + 1, M, 3), **self.f64),
                                       ul_in=torch.zeros((B, N, 5), **self.f64),
                                       list=torch.zeros(B, dtype=torch.int32, device=dev), count=torch.zeros(1, dtype=torch.int32, device=dev),
                                       susp=torch.zeros(B, dtype=torch.bool, device=dev), ev=None))
                if self.motion:
                    # the clock of this buffer set, registered once on the set's handle: a launch and its continuation read these
                    # ticks, whatever the robots of the other set do meanwhile
                    self._sets[s]["tick"] = torch.zeros(max(B, 1), dtype=torch.int64, device=dev)
                    self.engs[1 + s].set_obstacle_clock(self._sets[s]["tick"])
        for s in range(2):
            self.engs[1 + s].set_iteration_budget(budget); self.engs[1 + s].reset()
            self._sets[s]["ev"] = None; self._sets[s]["susp"].zero_()
        x = self.x0.clone(); ul = torch.zeros((B, N, 5), **self.f64)
        hist = torch.zeros((B, T, 5), **self.f64); its = torch.zeros((B, T), dtype=torch.int32, device=dev)
        tick = torch.zeros(B, dtype=torch.int64, device=dev)
        inflight = torch.zeros(B, dtype=torch.bool, device=dev)
        prev_it = torch.zeros(B, **self.f64)
        failed = torch.zeros((), dtype=torch.bool, device=dev)
        nsusp = torch.zeros((), dtype=torch.int64, device=dev)
        state = dict(x=x, ul=ul, tick=tick, prev_it=prev_it)

        def advance(mask, out):
            # the robots of `mask` take the solution in `out`: u_latest <- U*, plant step with u0, next tick
            u0 = out["U"][:, 0]
            t_idx = state["tick"].clamp(max=T - 1)
            hist[self.rows, t_idx] = torch.where(mask[:, None], u0, hist[self.rows, t_idx])
            its[self.rows, t_idx] = torch.where(mask, out["iters"], its[self.rows, t_idx])
            state["x"] = torch.where(mask[:, None], self.plant(state["x"], u0), state["x"])
            state["ul"] = torch.where(mask[:, None, None], out["U"], state["ul"])
            state["prev_it"] = torch.where(mask, out["iters"].to(torch.float64), state["prev_it"])
            state["tick"] = state["tick"] + mask.to(torch.int64)

        r = 0
        cap = max_rounds if max_rounds is not None else 4 * T + 8
        while True:
            s = r & 1
            S = self._sets[s]
            eng = self.engs[1 + s]
            if S["ev"] is not None:
                # the continuation of round r-2 (same handle, same buffers) is finished: its robots rejoin, one tick behind
                main.wait_event(S["ev"]); S["ev"] = None
                m = S["susp"]
                failed = failed | (m & (S["out"]["status"] != 0)).any()
                advance(m, S["out"])
                inflight = inflight & ~m
            ready = (~inflight) & (state["tick"] < T)
            S["x_in"].copy_(state["x"]); S["ul_in"].copy_(state["ul"])
            if self.motion:
                S["tick"][:B].copy_(state["tick"])
            self.inputs(state["x"], state["tick"], S["loc"], S["obs"])
            score = torch.where(ready, state["prev_it"] + 1.0, torch.zeros_like(state["prev_it"]))
            S["list"].copy_(torch.argsort(score, descending=True, stable=True).to(torch.int32))
            S["count"].copy_(ready.sum().to(torch.int32).reshape(1))
            eng.solve_batch_device(S["x_in"], S["loc"], self.uref, S["ul_in"], S["obs"], out=S["out"], rows=(S["list"], S["count"]))
            # (snapshots before the continuation on the side stream starts rewriting the rows of the suspended robots: advance() below
            #  reads whole columns on the main stream)
            snap = S["out"]["status"].clone()
            snap_out = dict(U=S["out"]["U"].clone(), iters=S["out"]["iters"].clone())
            evm = torch.cuda.Event(); evm.record(main)
            side = self._sides[s]
            side.wait_event(evm)
            eng.resume_batch_device(S["x_in"], S["loc"], self.uref, S["ul_in"], S["obs"], S["out"], stream=side.cuda_stream)
            S["ev"] = torch.cuda.Event(); S["ev"].record(side)
            conv = ready & (snap == 0)
            susp = ready & (snap == 3)
            failed = failed | (ready & (snap != 0) & (snap != 3)).any()
            nsusp = nsusp + susp.sum()
            advance(conv, snap_out)
            inflight = inflight | susp
            S["susp"] = susp
            r += 1
            if r >= T and (r >= cap or not bool(((state["tick"] < T) | inflight).any())):
                break
        for s in range(2):
            if self._sets[s]["ev"] is not None:
                self._sets[s]["ev"].synchronize(); self._sets[s]["ev"] = None
            self.engs[1 + s].set_iteration_budget(0)
        done = bool((state["tick"] >= T).all())
        return dict(u0=hist, x=state["x"], iters=its, all_converged=(~failed) & torch.tensor(done, device=dev), rounds=r, suspended=nsusp)
