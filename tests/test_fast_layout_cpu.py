"""CPU: the LDS layout of the specialised kernels of every listed shape (MMPC_FAST_LIST), from the kernels' own mmpc_fast_layout on
the host.  The persistent launch sizes its grid by the resident problems per CU, which the LDS block decides: a layout that grows
past a quarter of a CU's 160 KB where it fitted before halves nothing visibly but costs a fourth of the occupancy.  The strides
of the layout are those of the parent commit (the launch work left them alone), so the totals are pinned; and the offset of a
suspended solve's scalars that the tests read is the one the save-area layout implies."""
import ctypes as C

import pytest

import emu_helper

QUARTER = 160 * 1024 // 4
# (kind, N, M) -> bytes per obs_per_stage 0, 1, 2 on the parent commit (code object metadata of mmpc_fast_kernel<kind, N, M, ., false, ops>)
PARENT = {(0, 20, 5): (39600, 42000, 39680), (0, 30, 8): (40768, 40576, 40912), (0, 20, 3): (39552, 40992, 39600),
          (1, 15, 3): (16848, 17920, 16896)}


@pytest.mark.parametrize("shape", sorted(PARENT))
def test_layout_total_of_listed_shapes(shape):
    lib = C.CDLL(emu_helper.build())
    k, N, M = shape
    for ops, parent in enumerate(PARENT[shape]):
        total = 8 * lib.mmpc_emu_fast_lds_doubles(k, N, M, ops)
        assert total > 0
        if parent <= QUARTER:
            assert total <= QUARTER, (shape, ops, total)
        assert total == parent, (shape, ops, total)      # (strides unchanged; a re-stride edits this table and keeps the line above)


@pytest.mark.parametrize("kind,N", [(0, 20), (0, 30), (1, 15)])
def test_exported_scalar_offset_is_the_one_the_save_area_implies(kind, N):
    nx, nu = (9, 5) if kind == 0 else (6, 2)
    ns = N + 1
    assert emu_helper.fast_state_scal_offset(kind, N) == ns * (nx + nu) + ns + ns * nx + 2 * emu_helper.fcap()
