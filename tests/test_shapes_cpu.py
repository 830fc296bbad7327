"""CPU: shape libraries - the specialised template at shapes outside the four built-in ones (host emulation against the C oracle
and the generic kernel's emulation), the envelope predicate, and building / loading a library without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shape_helper as H
import motion_helper as MH

TOL = 1e-6      # the project's standing parity tolerance


@pytest.mark.parametrize("shape", H.SHAPE_LIST, ids=H.shape_id)
def test_emulated_shape_against_oracle_and_generic(shape):
    """every instance converges, X / U / s agree with the C oracle to 1e-6, iteration counts within one of the generic emulation's"""
    r, g, o = H.emulated(shape), H.emulated(shape, fast=False), H.oracle(shape)
    dX, dU, ds = H.max_dev(r, o)
    gX, gU, gs = H.max_dev(r, g)
    print("%s: vs oracle |dX| %.2e |dU| %.2e |ds| %.2e; vs generic emulation %.2e %.2e %.2e; iteration differences %s"
          % (H.shape_id(shape), dX, dU, ds, gX, gU, gs, np.flatnonzero(r["iters"] != g["iters"]).tolist()))
    assert (r["status"] == 0).all() and (g["status"] == 0).all() and (o["status"] == 0).all()
    assert dX <= TOL and dU <= TOL and ds <= TOL
    assert np.abs(r["iters"] - g["iters"]).max() <= 1


@pytest.mark.parametrize("shape", H.SHAPE_LIST, ids=H.shape_id)
def test_reverse_lane_order_same_bits(shape):
    par, d = H.inputs(shape)
    rev = H.solve(shape, par, d, reverse=True)
    H.assert_bitwise(H.emulated(shape), rev, keys=H.BIT_KEYS + ("err",), what="reverse lane order")


@pytest.mark.parametrize("shape", [(0, 24, 6), (1, 25, 4)], ids=H.shape_id)
def test_continuation_same_bits(shape):
    par, d = H.inputs(shape)
    full = H.emulated(shape)
    assert full["iters"].max() > 5
    cut = H.solve(shape, par, d, budget=5)
    assert cut["launches"] == 2
    H.assert_bitwise(full, cut, what="budget 5 + continuation")


def test_motion_record_solves_its_table_twin():
    shape = (0, 24, 6)
    k, N, M = shape
    B = 32
    par = H.par_of(k, N)
    m = MH.motion_inputs(B, N, M)
    d = dict(x_init=np.clip(m["x_init"], par.xlim[0], par.xlim[1]), traj_ref=m["traj_ref"], u_ref=m["u_ref"], u_last=np.zeros((B, N, 5)))
    tab = MH.table_twin(m["rec"], m["tick"], N, par.dt)
    a = H.solve(shape, par, d, obs=m["rec"], tick=m["tick"], mode=2)
    b = H.solve(shape, par, d, obs=tab, mode=1)
    assert (b["status"] == 0).all() and b["iters"].max() > 8
    H.assert_bitwise(b, a, what="motion record against its table")
    assert np.abs(m["rec"][..., 3:]).max() > 0 and (m["tick"] > 0).any()


def test_slim_horizons_take_the_plain_pair_map():
    """the padded pair map is not written for the slim layout (N >= 21); the short whole-body horizons from N = NX on keep it"""
    for shape in H.SHAPE_LIST:
        pad = H.lib(shape).mmpc_emush_padmap()
        if shape[1] >= 21:
            assert pad == 0, shape
        if shape in ((0, 12, 4), (0, 20, 10)):
            assert pad == 1, shape
    assert H.lib((0, 5, 3)).mmpc_emush_padmap() == 0


# True / False at the edges of the envelope.  The issue derived them from the MmpcLogAcc bounds (2 NPASS <= 15 factors, rows + NSELF
# <= 15): whole-body N <= 31, base N <= 55, whole-body M <= 11 at N <= 20.  Where the template's other static assertions put an
# edge elsewhere, they decide: whole-body N = 21 and 22 are OUTSIDE, because the gain ring of the device roll-out (four slots of
# NU NX + NU = 50 doubles) does not fit the stage-matrix extras (192 and 198 doubles) at those horizons - N = 23 (204) is the first.
EDGES_TRUE = [(0, 31, 8), (0, 20, 11), (1, 55, 1), (0, 1, 0), (0, 23, 0), (0, 30, 16), (1, 21, 0), (0, 20, 0), (1, 15, 16)]
EDGES_FALSE = [(0, 32, 0), (0, 20, 12), (1, 56, 0), (2, 20, 5), (2, 5, 0), (3, 5, 0), (-1, 5, 0), (0, 0, 0), (0, 64, 0), (0, 20, -1), (0, 20, 17),
               (1, 63, 0), (0, 21, 2), (0, 22, 0)]


def test_predicate_edges_host():
    for s in EDGES_TRUE:
        assert H.shape_ok(*s), s
    for s in EDGES_FALSE:
        assert not H.shape_ok(*s), s
    for s in H.SHAPE_LIST + [(0, 20, 5), (0, 30, 8), (0, 20, 3), (1, 15, 3)]:
        assert H.shape_ok(*s), s


def test_predicate_edges_c_abi(mm):
    L = mm._capi.lib()
    for s in EDGES_TRUE:
        assert L.mmpc_shape_supported(*s) == 1, s
    for s in EDGES_FALSE:
        assert L.mmpc_shape_supported(*s) == 0, s
    # the library and the host build state one envelope
    for kind in (0, 1):
        for N in (1, 8, 20, 21, 23, 31, 32, 55, 56):
            for M in (0, 8, 11, 12, 16):
                assert bool(L.mmpc_shape_supported(kind, N, M)) == H.shape_ok(kind, N, M), (kind, N, M)


def _build_mod(mm):
    return sys.modules[mm.__name__ + ".build"]


def test_build_and_load_a_shape_library(mm):
    b = _build_mod(mm)
    L = mm._capi.lib()
    err = lambda: (L.mmpc_last_error(None) or b"").decode()
    path = mm.build_shape_library(0, 5, 3)
    assert path == b.shape_library_path(0, 5, 3) and os.path.dirname(path).endswith(os.path.join("csrc", "shapes"))
    data = open(path, "rb").read()
    assert b"gfx950" in data and b"mmpc_fast_kernelILi0ELi5ELi3E" in data
    assert b.shape_library_current(0, 5, 3)
    assert L.mmpc_load_shape_library(os.fsencode(path)) == 0, err()
    assert L.mmpc_load_shape_library(os.fsencode(path)) == 0, err()
    E_ARG = -1
    assert L.mmpc_load_shape_library(os.fsencode(path + ".missing")) == E_ARG
    assert "cannot open" in err() and ".missing" in err()
    assert L.mmpc_load_shape_library(os.fsencode(mm._capi.LIB_PATH)) == E_ARG
    assert "not a shape library" in err()
    assert L.mmpc_load_shape_library(os.fsencode(H.wrong_tag_library(mm))) == E_ARG
    assert "other kernel sources" in err() and ("%016x" % H.WRONG_TAG) in err() and ("%016x" % b.source_tag()) in err()
    assert L.mmpc_load_shape_library(None) == E_ARG
    with pytest.raises(RuntimeError, match="other kernel sources"):
        b.load_shape_library(H.wrong_tag_library(mm))


def test_unsupported_shapes_raise_before_anything_is_compiled(mm, monkeypatch):
    b = _build_mod(mm)
    calls = []
    monkeypatch.setattr(b.subprocess, "check_call", lambda *a, **k: calls.append(a))
    for s in ((0, 32, 0), (0, 20, 12), (1, 56, 0), (2, 20, 5), (0, 21, 2)):
        with pytest.raises(ValueError, match="outside the envelope"):
            mm.build_shape_library(*s)
    assert not calls


def test_specialise_keyword_before_the_handle(mm, monkeypatch):
    """what _capi.prepare_shape decides without a GPU: the value of mmpc_config.specialise, and what it refuses"""
    cap, b = mm._capi, _build_mod(mm)
    built = []
    monkeypatch.setattr(b, "build_shape_library", lambda *a, **k: built.append(a) or b.shape_library_path(*a[:3]))
    assert cap.prepare_shape(0, 12, 4, False) == 0
    for s in cap.LISTED_SHAPES:                      # a listed shape ignores the argument
        assert cap.prepare_shape(*s, True) == 0 and cap.prepare_shape(*s, "cached") == 0
    assert cap.prepare_shape(0, 11, 4, "cached") == 0 and not built        # no library of that shape: the generic kernel
    assert cap.prepare_shape(0, 5, 3, "cached") == 1                        # built by the entry point's build()
    for args, why in (((0, 32, 0, True), "outside the envelope"), ((2, 12, 4, True), "pose-reference"), ((0, 12, 4, True, 2), "half-space")):
        with pytest.raises(ValueError, match=why):
            cap.prepare_shape(*args)
    assert cap.prepare_shape(0, 32, 0, "cached") == 0 and cap.prepare_shape(0, 12, 4, "cached", 2) == 0 and not built
    with pytest.raises(ValueError, match="specialise must be"):
        cap.prepare_shape(0, 12, 4, "yes")
    assert cap.prepare_shape(0, 5, 3, True) == 1 and built == [(0, 5, 3)]


@pytest.mark.parametrize("shape", H.ASAN_SHAPES, ids=H.shape_id)
def test_sanitized_program_ends_clean(shape, tmp_path):
    """a stand-alone program (its own main; nothing sanitized is loaded into python) under AddressSanitizer and UBSan: two instances,
    both lane orders"""
    exe = H.build(shape, asan_main=True)
    case = H.write_case(str(tmp_path / "case.bin"), shape, B=2)
    r = subprocess.run([exe, case], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count("status 0") == 4
