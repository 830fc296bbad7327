"""GPU (MI355X): the persistent plain launch of the specialised kernels (mmpc_set_persistent_grid) - a grid of resident workgroups
that draw their launch positions from the handle's ticket and solve several instances in turn on one LDS block - against the
launch form it replaces (one workgroup per instance, persistent_grid < 0) on the same handle.  The two forms run the same solver
text on the same inputs, so every comparison is exact equality of all seven outputs, bit for bit.

What can go wrong only in the new form: state of the previous instance left in LDS or in registers (grid 2 at B = 5 makes every
workgroup reuse its block at least once; a NaN instance in the middle is the worst predecessor), the constants block after an
instance that scaled its weights, a ticket that is not back at 0 for the next launch, a position drawn twice or never (the
sentinel in the fresh output set shows a row that nobody wrote), and the launch orders (which only apply above B = 256)."""
import numpy as np
import pytest

from oracle import nlp, synth

pytestmark = pytest.mark.gpu
KEYS = ("X", "U", "s", "status", "iters", "cost", "err")
SHAPES = {(0, 20, 5): dict(kind="wholebody", config_id=3), (1, 15, 3): dict(kind="base", config_id=2),
          (0, 30, 8): dict(kind="wholebody", config_id=5)}


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


class _Run:
    """a handle of a listed shape with a seeded batch on the device"""

    def __init__(self, mm, shape, B, nan_row=None):
        import torch
        k, N, M = shape
        par = nlp.BaseParams(N=N) if k == 1 else nlp.WholeBodyParams(N=N)
        d = synth.make_batch(B, N=N, M=M, **SHAPES[shape])
        x_init = np.array(d["x_init"])
        if nan_row is not None:
            x_init[nan_row, 0] = np.nan
        self.B, self.N, self.nx, self.nu, self.torch = B, N, par.nx, par.nu, torch
        self.eng = mm._capi.Engine(k, N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=B)
        assert self.eng.runs_specialised
        self.t = [_dev(x_init), _dev(d["traj_ref"]), _dev(d["u_ref"]), _dev(np.zeros((B, N, par.nu))), _dev(d["obs"])]

    def solve(self, grid):
        """one launch with `grid` into an output set filled with a sentinel: a row that no workgroup wrote cannot pass"""
        f = lambda *s: self.torch.full(s, -7.0, dtype=self.torch.float64, device="cuda:0")
        i = lambda *s: self.torch.full(s, -7, dtype=self.torch.int32, device="cuda:0")
        B, N = self.B, self.N
        out = dict(X=f(B, N + 1, self.nx), U=f(B, N, self.nu), s=f(B, N + 1), status=i(B), iters=i(B), cost=f(B), err=f(B))
        self.eng.set_persistent_grid(grid)
        self.eng.solve_batch_device(*self.t, out=out)
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_bitwise(new, old, what, rows=None):
    for k in KEYS:
        a, b = new[k], old[k]
        if rows is not None:
            a, b = a[rows], b[rows]
        a = np.ascontiguousarray(a).reshape(len(a), -1)
        b = np.ascontiguousarray(b).reshape(len(b), -1)
        same = (a.view(np.uint8) == b.view(np.uint8)).all(axis=1)
        assert same.all(), "%s: %s differs in rows %s" % (what, k, np.nonzero(~same)[0].tolist())


def test_c4_one_instance(mm):
    run = _Run(mm, (0, 20, 5), 1)
    old = run.solve(-1)
    assert old["status"][0] == 0 and old["iters"][0] > 0
    _assert_bitwise(run.solve(0), old, "B = 1, automatic grid")


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_workgroup_reuses_its_block(mm, shape):
    """B = 5 on 2 workgroups, twice on one handle (the second launch needs the ticket back at 0)"""
    run = _Run(mm, shape, 5)
    old = run.solve(-1)
    assert (old["status"] == 0).all() and (old["iters"] > 0).all()
    _assert_bitwise(run.solve(2), old, "%s, B = 5, grid 2" % (shape,))
    _assert_bitwise(run.solve(2), old, "%s, B = 5, grid 2, second launch" % (shape,))
    _assert_bitwise(run.solve(1), old, "%s, B = 5, grid 1" % (shape,))
    _assert_bitwise(run.solve(0), old, "%s, B = 5, automatic grid after the small ones" % (shape,))


def test_c4_nan_instance_leaves_its_successors_alone(mm):
    run, clean = _Run(mm, (0, 20, 5), 5, nan_row=1), _Run(mm, (0, 20, 5), 5)
    others = np.array([0, 2, 3, 4])
    old, ref = run.solve(-1), clean.solve(-1)
    assert old["status"][1] == 2 and (old["status"][others] == 0).all()
    _assert_bitwise(old, ref, "one workgroup per instance, beside a NaN instance", rows=others)
    for grid in (2, 1):      # (grid 1: every later instance runs behind the NaN one on the same workgroup)
        new = run.solve(grid)
        assert new["status"][1] == 2
        _assert_bitwise(new, ref, "grid %d, rows behind and beside the NaN instance" % grid, rows=others)


def test_c4_objective_scaling_restores_the_constants(mm):
    run = _Run(mm, (0, 20, 5), 5)
    plain = run.solve(-1)
    scale = run.torch.ones(5, dtype=run.torch.float64, device="cuda:0")
    run.eng.set_objective_scaling(100.0, scale)
    old = run.solve(-1)
    assert (old["status"] == 0).all()
    assert (scale.cpu().numpy() < 1.0).sum() >= 2      # (the option acts on this batch: instances that scale their weights have successors)
    _assert_bitwise(run.solve(2), old, "objective scaling, grid 2")
    _assert_bitwise(run.solve(1), old, "objective scaling, grid 1")
    run.eng.set_objective_scaling(0.0)
    _assert_bitwise(run.solve(2), plain, "grid 2 after the option is off again")


@pytest.mark.parametrize("B,grid", [(70, 0), (300, 64)])
def test_c4_launch_orders(mm, B, grid):
    """batch order, history order (the second launch of mode 1 sorts by the first one's iteration counts) and key order; the orders
    only apply above B = 256, where the small grid makes every workgroup draw several positions of the order"""
    run = _Run(mm, (0, 20, 5), B)
    run.eng.set_schedule_hint(0)
    old = run.solve(-1)
    assert (old["status"] == 0).all()
    _assert_bitwise(run.solve(grid), old, "B = %d, batch order" % B)
    for mode, launches in ((1, 3), (2, 2)):
        run.eng.set_schedule_hint(mode)
        for n in range(launches):
            _assert_bitwise(run.solve(grid), old, "B = %d, schedule hint %d, launch %d" % (B, mode, n))
        _assert_bitwise(run.solve(-1), old, "B = %d, schedule hint %d, one workgroup per instance" % (B, mode))
