"""CPU: the linear-motion obstacle mode (obs_per_stage = 2) of both solver kernels in the host emulation
(tests/emu_motion/mmpc_emu_motion.cpp) against its table twin - the same solve with the per-stage table c + v ((tick + k) dt)
built in numpy.  Both runs see identical centres and run the same iteration, so every comparison is bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nlp

import emu_helper
import motion_helper as mh

GENERIC = [("wb", 6, 2), ("base", 5, 1), ("pose", 6, 2)]
FAST = [(0, 20, 5), (0, 30, 8), (0, 20, 3), (1, 15, 3)]


def _par(kind, N):
    return {"wb": nlp.WholeBodyParams, "base": nlp.BaseParams, "pose": nlp.pose_ref_params}[kind](N=N)


def _inputs(kind, B, N, M):
    d = mh.motion_inputs(B, N, M, kind="base" if kind == "base" else "wholebody")
    if kind != "pose":
        # short horizons never reach the generator's obstacles: the first one goes right in front of the robot, where the
        # robot's own speed carries it into the inflated disc within the horizon
        tick_t = (d["tick"].astype(np.float64) * 0.1)[:, None]
        v = d["x_init"][:, 3:5]
        ahead = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9)
        d["rec"][:, 0, 2] = 0.3
        d["rec"][:, 0, :2] = d["x_init"][:, :2] + ahead * 0.75 - d["rec"][:, 0, 3:] * tick_t
    if kind == "pose":
        x, ref, _ = emu_helper.pose_batch(B, N, seed=N)
        d["x_init"], d["traj_ref"] = x, ref
        # the generator's obstacles belong to another path: two discs beside this one, drifting across it
        E0 = ref[:, 0, :2]; E1 = ref[:, -1, :2]
        d["rec"][:, 0, :2] = E0 + 0.5 * (E1 - E0) + [0.0, 0.45]; d["rec"][:, 0, 2] = 0.3
        d["rec"][:, 1, :2] = E0 + 0.8 * (E1 - E0) - [0.0, 0.6]; d["rec"][:, 1, 2] = 0.2
        d["rec"][..., :2] -= d["rec"][..., 3:] * (d["tick"].astype(np.float64) * 0.1)[:, None, None]
    return d


def test_centre_helpers_are_the_table_definition():
    """mmpc_tick_centre(mmpc_tick_time) = numpy's c + v * ((tick + k) * dt), and the kernels' (double)tick + (double)k form gives
    the same bits, up to the documented 2^52"""
    rng = np.random.default_rng(1)
    for tick in (0, 1, 250, 2 ** 31 + 5, 2 ** 40 + 3, 2 ** 52 - 64):
        for _ in range(8):
            c, v, dt = rng.uniform(-5, 5), rng.uniform(-0.5, 0.5), (0.1, 0.05, 1.0 / 3.0)[rng.integers(3)]
            a, b = mh.centres(c, v, tick, dt, 64)
            ref = c + v * ((np.int64(tick) + np.arange(64, dtype=np.int64)).astype(np.float64) * dt)
            assert a.tobytes() == ref.tobytes() and b.tobytes() == ref.tobytes()


@pytest.mark.parametrize("kind,N,M", GENERIC)
def test_generic_motion_equals_table_twin(kind, N, M):
    B = 8
    par = _par(kind, N)
    d = _inputs(kind, B, N, M)
    assert (d["rec"][..., 3:] < 0).any() and len(set(d["tick"])) == B and 0 in d["tick"] and 2 ** 31 + 5 in d["tick"]
    ul = np.zeros((B, N, par.nu))
    tab = mh.table_twin(d["rec"], d["tick"], N, par.dt)
    args = (par, d["x_init"], d["traj_ref"], d["u_ref"], ul)
    t = mh.solve(*args, tab)
    m = mh.solve(*args, d["rec"], tick=d["tick"], mode=2)
    assert (t["status"] == 0).all()
    mh.assert_bitwise(m, t, what="motion vs table")
    mh.assert_bitwise(mh.solve(*args, d["rec"], tick=d["tick"], mode=2, reverse=True), t, what="reversed lanes")
    # the obstacles matter: without them the solution is another one
    far = tab.copy(); far[..., :2] += 100.0
    assert np.abs(mh.solve(*args, far)["X"] - t["X"]).max() > 1e-6
    # no clock registered = tick 0
    z = mh.solve(*args, d["rec"], tick=None, mode=2)
    mh.assert_bitwise(z, mh.solve(*args, mh.table_twin(d["rec"], np.zeros(B, np.int64), N, par.dt)), what="null clock")


_ASAN_CODE = """
import sys; sys.path[:0] = [%r, %r]
import numpy as np
from oracle import nlp
import motion_helper as mh
import test_motion_cpu as T
kind, N, M = T.GENERIC[0]
par = T._par(kind, N)
d = T._inputs(kind, 3, N, M)
args = (par, d["x_init"], d["traj_ref"], d["u_ref"], np.zeros((3, N, par.nu)))
a = mh.solve(*args, d["rec"], tick=d["tick"], mode=2, asan=True)
mh.assert_bitwise(a, mh.solve(*args, mh.table_twin(d["rec"], d["tick"], N, par.dt), asan=True), what="generic")
z = mh.solve(*args, np.zeros((3, 0, 5)), tick=d["tick"], mode=2, asan=True)
assert (z["status"] == 0).all()
for k, N, M in ((0, 30, 8),):
    f = mh.motion_inputs(2, N, M)
    argf = (nlp.WholeBodyParams(N=N), f["x_init"], f["traj_ref"], f["u_ref"], np.zeros((2, N, 5)))
    af = mh.solve(*argf, f["rec"], tick=f["tick"], mode=2, fast=True, asan=True, budget=5)
    assert af["launches"] == 2
    mh.assert_bitwise(af, mh.solve(*argf, mh.table_twin(f["rec"], f["tick"], N, 0.1), fast=True, asan=True), what="specialised")
print("ASAN-OK")
"""


def test_motion_under_asan():
    """the record, the tick and the slab are exact-size heap blocks: one generic shape, M = 0, and the specialised N = 30
    kernel (budgeted: record in LDS, gains in their global block) in the sanitizer build, which build() of the repository compiles"""
    here = os.path.dirname(os.path.abspath(__file__))
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    pre = os.environ.get("LD_PRELOAD")
    env = dict(os.environ, LD_PRELOAD=libasan + (":" + pre if pre else ""), ASAN_OPTIONS="detect_leaks=0")
    p = subprocess.run([sys.executable, "-c", _ASAN_CODE % (os.path.dirname(here), here)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "ASAN-OK" in p.stdout, (p.stdout + p.stderr)[-3000:]


@pytest.mark.parametrize("kind,N", [("wb", 6), ("base", 5), ("pose", 6)])
def test_generic_motion_without_obstacles_equals_static(kind, N):
    B = 4
    par = _par(kind, N)
    d = _inputs(kind, B, N, 2)
    ul = np.zeros((B, N, par.nu))
    args = (par, d["x_init"], d["traj_ref"], d["u_ref"], ul)
    m = mh.solve(*args, np.zeros((B, 0, 5)), tick=d["tick"][:B], mode=2)
    mh.assert_bitwise(m, mh.solve(*args, np.zeros((B, 0, 3))), what="M = 0")


@pytest.mark.parametrize("k,N,M", FAST)
def test_fast_motion_equals_table_twin_and_continues(k, N, M):
    B = 4
    par = nlp.WholeBodyParams(N=N) if k == 0 else nlp.BaseParams(N=N)
    d = mh.motion_inputs(B, N, M, kind="wholebody" if k == 0 else "base")
    ul = np.zeros((B, N, par.nu))
    args = (par, d["x_init"], d["traj_ref"], d["u_ref"], ul)
    t = mh.solve(*args, mh.table_twin(d["rec"], d["tick"], N, par.dt), fast=True)
    m = mh.solve(*args, d["rec"], tick=d["tick"], mode=2, fast=True)
    assert (t["status"] == 0).all() and (t["iters"] > 5).all()
    mh.assert_bitwise(m, t, what="motion vs table")
    bud = mh.solve(*args, d["rec"], tick=d["tick"], mode=2, fast=True, budget=5)
    assert bud["launches"] == 2
    mh.assert_bitwise(bud, m, what="budget 5 + continuation")


def test_fast_layout_fits_four_problems_per_cu():
    """the record in LDS: at most 5120 doubles (40 KB, four problems per CU) for the three whole-body shapes"""
    for N, M in ((20, 5), (20, 3), (30, 8)):
        n2 = mh.fast_lds_doubles(0, N, M, 2)
        assert 0 < n2 <= 5120, (N, M, n2)
        assert n2 - mh.fast_lds_doubles(0, N, M, 0) == ((5 * M + 2) & ~1) - ((3 * M + 1) & ~1)
    assert mh.fast_lds_doubles(1, 15, 3, 2) <= mh.fast_lds_doubles(1, 15, 3, 1)


# largest N whose generic slab fits 160 KiB in mode 2, per kind and M (include/mmpc.h): from the layout's
# arithmetic - the mode-0 slab plus the record's 2 M + 1 words - and checked here at both edges
ENVELOPE = {0: {0: 49, 16: 35}, 1: {16: 59}, 2: {0: 55, 16: 38}}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_generic_envelope_of_motion_mode(kind):
    cap = 160 * 1024 // 8
    for M, nmax in ENVELOPE[kind].items():
        assert mh.lds_doubles(kind, nmax, M, 2) <= cap, (kind, M, nmax)
        if nmax < 63:
            assert mh.lds_doubles(kind, nmax + 1, M, 2) > cap, (kind, M, nmax + 1)
        # between the static record and the table
        assert mh.lds_doubles(kind, nmax, M, 0) <= mh.lds_doubles(kind, nmax, M, 2) <= mh.lds_doubles(kind, nmax, M, 1) + 2
    if kind == 1:
        assert mh.lds_doubles(1, 63, 13, 2) <= cap
