"""The relation that the shared row step (add_rows) and the shared block sum (block_sums28) of
k_align and k_refine make structural (DESIGN.md §Dense map, Refining, "One text"), on the scenes
and with the map and pose helpers of tests/test_gpu_refine.py."""
import numpy as np
import pytest

import test_gpu_refine as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _module(fmx_mod):
    TR._FMX["mod"] = fmx_mod


@TR.FORMS
@pytest.mark.parametrize("m", [1, 64, 65, 256])
def test_one_tile_is_the_one_block_system_bit_for_bit(fmx_mod, form, m):
    """Up to one tile of kept points is one k_refine item and one k_align block.  Both build
    their rows with the one row step and sum them with the one block sum: the same wave sums
    added in the same wave order; every later stage of either path (k_align's last block, the
    finisher) only adds exact zeros.  So the record's system is fmx_align_system's /
    fmx_plane_system's at that pose to the bit, not within a measure."""
    reps, q, ref, first = TR._scene(form)
    assert fmx_mod.refine_plan(m, 1, 1)["tiles"] == 1 and m <= 256  # (one block of 256 lanes, one point each)
    ctx, _ = TR._map(fmx_mod, form)
    plane = form == "plane"
    three = TR._poses(3, seed=7, spread=0.3 if plane else 0.6, turn=0.05 if plane else 0.5, first=first)
    got = ctx.refine_systems(q[:m], three, reach=1, sigma=0.5, plane=plane)
    call = ctx.plane_system if plane else ctx.align_system
    for k, T in enumerate(three):
        S, cnt = call(q[:m], T, reach=1, sigma=0.5)
        assert np.array_equal(got["system"][k], S), (k, np.abs(got["system"][k] - S).max())
        assert {c: int(got[c][k]) for c in TR.CLASSES} == {c: cnt.get(c, 0) for c in TR.CLASSES}, k
        assert int(got["lookups"][k]) == cnt["lookups"], k
    assert m < 64 or got["found"].sum() > 0
