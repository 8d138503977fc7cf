"""The lock-step layer's kernel choice, checked without running a kernel: runtime.inc:wide_plan (through clstm_debug_wide_plan, which
needs no net and no device) against test_wide_layer_sweep.wide_geometry, the hand-written restatement of the rule, for every cell count
129..576, the sweep's line counts, one and two directions, the sweep's five modes and chips of 104, 256, 264 and 304 CUs -- the
8 * ntile <= ncu gate at every tile count and the ntile <= 32 gate, which needs more CUs than an MI355X has, included."""
import pytest

from common import emu_lib
from test_wide_layer_sweep import LINE_COUNTS, MODES, assert_plan_agrees, wide_geometry

CU_COUNTS = [104, 256, 264, 304]
TMAX = 9


@pytest.mark.parametrize("ncu", CU_COUNTS)
def test_the_library_plan_is_the_restated_rule(ncu):
    lib, seen = emu_lib(), set()
    for name, m in MODES.items():
        precision, strict, rec = m["precision"], m.get("strict", False), m.get("rec", True)
        for ni in (48, 64) if precision == 2 else (48,):          # 64 inputs: whole 32-k groups, the folded input projection is asked for
            for ndir in (1, 2):
                for nlines in LINE_COUNTS:
                    for no in range(129, 577):
                        geo = wide_geometry(no, ni, ndir, nlines, TMAX, precision, strict, "hip", rec, ncu=ncu)
                        assert_plan_agrees(lib, geo, no, ni, ndir, nlines, TMAX, precision, strict, ncu, rec)
                        seen.add((geo["fwd"], geo["bwd"]))
    kernels = {k for pair in seen for k in pair}
    # every kernel of the rule was met on a chip of this size, with every parameter the default options reach (fx<4>, fx<8> need fuse_wx = 2)
    assert kernels == {"xcd_fwd_f32", "xcd_fwd_bf16<1>", "xcd_fwd_bf16<2>", "xcd_fwd_bf16<4>", "xcd_fwd_bf16_fx<1>", "xcd_bwd_x3", "xcd_bwd_f32",
                       "xcd_bwd_bf16_c32<1>", "xcd_bwd_bf16_c32<2>", "xcd_bwd_bf16_c32<4>", "xcd_bwd_bf16<1>", "xcd_bwd_bf16<2>", "xcd_bwd_bf16<4>",
                       "fwd_step<1>", "fwd_step<2>", "fwd_step<4>", "fwd_step16_bf16", "bwd_step", "bwd_step16_bf16"}, sorted(kernels)
    # ... and both gates bite: 33 cell tiles never fit, 32 fit from 256 CUs on, 14 tiles (112 workgroups) not on 104 CUs
    assert wide_geometry(513, 48, 2, 16, TMAX, 0, False, "hip", ncu=304)["fwd"] == "fwd_step<1>"
    assert [wide_geometry(512, 48, 2, 16, TMAX, 0, False, "hip", ncu=n)["fwd"] for n in CU_COUNTS] == ["fwd_step<1>", "xcd_fwd_f32", "xcd_fwd_f32", "xcd_fwd_f32"]
    assert [wide_geometry(no, 48, 2, 16, TMAX, 0, False, "hip", ncu=104)["fwd"] for no in (208, 209)] == ["xcd_fwd_f32", "fwd_step<1>"]
