"""The narrow layer's kernel choice, checked without running a kernel: runtime.inc:narrow_plan (through clstm_debug_narrow_plan, which needs
no net and no device) against narrow_rule.plan, the hand-written restatement of the rule, for every cell count 1..128, one and two
directions, one and two layers, overlap 0 / 1 / 2, strict on and off, the emulator flag on and off and chips of 16, 104, 256 and 304 CUs --
and, crossed with the cell counts, at both sides of every bound of the rule: the three CU-count bounds of each chip, the 640-, 900- and
2048-line crossovers, the tmax / frames gate of overlap = 1, 96 / 97 classes, 48 / 49 inputs, every option at each of its values and the
32-bit offset limits.  The literal facts at the end pin the restatement itself."""
import pytest

from common import emu_lib
from narrow_rule import (BWD, FWD_NOSAVE, FWD_SAVE, LIM, NB_BWD_DW, NB_LINE, NB_MFMA, NB_MFMA_DW, NB_MFMA_THEN_DW, NF_FUSED, NF_LINE, NF_MFMA, assert_plan_agrees,
                         fused_forward, plan, shape, xd_form)

CU_COUNTS = [16, 104, 256, 304]
PASSES = (FWD_SAVE, FWD_NOSAVE, BWD)
CELLS = range(1, 129)
# (lines, longest line): a small minibatch, one the overlap = 1 rule admits (64 x 200), the headline shapes from the MFMA crossover on
MINIBATCHES = [(7, 37), (64, 200), (640, 100)]


def nets(no):
    """one layer; the top and the first layer of two"""
    return ([no], 0), ([50, no], 1), ([no, 50], 0)


@pytest.mark.parametrize("emu", [0, 1], ids=["gpu_build", "emulator_build"])
@pytest.mark.parametrize("ncu", CU_COUNTS)
def test_the_library_plan_is_the_restated_rule(ncu, emu):
    lib = emu_lib()
    for no in CELLS:
        for nh, layer in nets(no):
            for uni in (False, True):
                for overlap in (0, 1, 2):
                    for strict in (False, True):
                        for nlines, tmax in MINIBATCHES:
                            for pass_ in PASSES:
                                assert_plan_agrees(lib, shape(pass_, nh, layer=layer, uni=uni, nlines=nlines, tmax=tmax, overlap=overlap, strict=strict, ncu=ncu, emu=emu))


def bounds(ncu, ndir):
    """keyword sets for shape(): both sides of every bound of the rule (the cell counts are crossed with each, not the bounds with each other)"""
    out = []
    # lines x directions at the three CU-count bounds: W.d rides the launch (x 4 <= 3 CUs), the producer form (x 2 <= CUs), the fused forward
    for limit in (3 * ncu // (4 * ndir), ncu // (2 * ndir), (ncu - max(8, ncu // 8)) // ndir):
        out += [dict(nlines=n, tmax=20, overlap=2) for n in (limit, limit + 1) if n > 0]
    # the line-count crossovers: batched MFMA from 640, its one-launch backward below 900, progress words up to 2048
    for n in (639, 640, 899, 900, 2048, 2049):
        out += [dict(nlines=n, tmax=70, overlap=ov) for ov in (1, 2)]
    # overlap = 1: tmax >= 64 and 2048 frames
    out += [dict(nlines=40, tmax=t, frames=f, overlap=1) for t, f in ((63, 2400), (64, 2400), (64, 2047), (64, 2048))]
    out += [dict(nlines=7, tmax=37, overlap=2, nc=nc) for nc in (96, 97)]
    out += [dict(nlines=640, tmax=70, ni=ni) for ni in (48, 49)]
    # every option at each of its values: where the rule decides by itself (640 and 900 lines) and forced onto a small minibatch
    for base in (dict(nlines=7, tmax=37, overlap=2), dict(nlines=640, tmax=70), dict(nlines=900, tmax=70)):
        for opt in ("fwd_mfma", "bwd_mfma", "bwd_mfma_fused", "xd_prologue"):
            out += [dict(base, **{opt: v}) for v in (0, 1, 2)]
        out += [dict(base, bwd_mfma=2, bwd_mfma_fused=v) for v in (0, 2)]
        out += [dict(base, fwd_mfma=2, bwd_mfma=2, strict=True), dict(base, dw_x3=0), dict(base, split_terms=2), dict(base, bwd_mfma=2, split_terms=2),
                dict(base, bf16_gemm=True), dict(base, fwd_mfma=2, bwd_mfma=2, bf16_gemm=True)]
    # 32-bit offsets: a buffer of just under / just over 2147483000 bytes
    for cap in (int(LIM) // 4 - 1, int(LIM) // 4):
        out += [dict(nlines=7, tmax=37, overlap=2, h_cap=cap), dict(nlines=7, tmax=37, overlap=2, d_cap=cap)]
    return out


@pytest.mark.parametrize("ncu", CU_COUNTS)
def test_both_sides_of_every_bound(ncu):
    lib, fwd, bwd, xd = emu_lib(), set(), set(), set()
    for no in CELLS:
        for uni in (False, True):
            ndir = 1 if uni else 2
            cases = bounds(ncu, ndir)
            # ... and frames whose gate pre-activations (N x ndir x 4 no x 4 bytes) just fit / just do not, under the forced MFMA options
            n32 = int(LIM) // (ndir * 16 * no)
            cases += [dict(nlines=7, tmax=37, frames=f, fwd_mfma=2, bwd_mfma=2, overlap=0) for f in (n32 - 1, n32, n32 + 1)]
            for kw in cases:
                for emu in (0, 1):
                    for pass_ in PASSES:
                        p = assert_plan_agrees(lib, shape(pass_, [no], uni=uni, ncu=ncu, emu=emu, **kw))
                        fwd.add(p["fwd"]); bwd.add(p["bwd"]); xd.add(p["xd"])
    # every forward family, every launch form and every x.d form of the rule was met on a chip of this size
    assert fwd == {0, NF_LINE, NF_FUSED, NF_MFMA} and bwd == set(range(8)) and xd == {0, 1, 2}, (fwd, bwd, xd)


def test_literal_facts_of_the_rule():
    """what the restatement answers at the shapes DESIGN.md and EXPERIMENTS.md quote -- and the library with it"""
    lib = emu_lib()
    # the fused forward: bidirectional exactly 81..111 (never a size whose last lane owns a cell), one direction up to 120, on 256 CUs
    assert [no for no in range(1, 129) if fused_forward([no], False, 83, 7, 2, "hip")] == [no for no in range(81, 112) if no % 16 != 0]
    assert [no for no in range(1, 129) if fused_forward([no], True, 83, 7, 2, "hip")] == [no for no in range(81, 121) if no % 16 != 0]
    # x.d: 64 bidirectional lines take the producer form, 65..96 the whole prologue, 97 the launch of its own, on 256 CUs
    assert [xd_form([100], False, 83, n, 2, "hip") for n in (64, 65, 96, 97)] == [2, 1, 1, 0]
    # the headline net at the crossovers, by the default rule
    def bwd(no, nlines):
        return assert_plan_agrees(lib, shape(BWD, [no], nlines=nlines, tmax=200, ncu=256, emu=0))
    assert bwd(100, 640)["bwd"] == NB_MFMA_DW and bwd(100, 899)["bwd"] == NB_MFMA_DW      # MFMA rows + items, one launch
    assert bwd(100, 900)["bwd"] == NB_MFMA_THEN_DW                                         # ... two launches
    assert bwd(100, 639)["bwd"] == NB_BWD_DW and bwd(100, 639)["xd"] == 0                  # the per-line one-launch form; 1278 workgroups: x.d apart
    assert bwd(64, 640) == dict(bwd(64, 640), overlapped=0, bwd=NB_MFMA)                   # 64 cells: the last lane owns a cell -> MFMA rows, family Narrow
    assert bwd(64, 639)["bwd"] == NB_LINE and bwd(128, 640)["bwd"] == NB_LINE              # (128 cells have no batched backward)
    for no, saves in ((64, 0), (100, 0), (128, 1)):                                        # (... and no no-save forward: the training form runs)
        p = assert_plan_agrees(lib, shape(FWD_NOSAVE, [no], nlines=640, tmax=200, ncu=256, emu=0))
        assert (p["fwd"], p["saves"]) == (NF_MFMA, saves)
    assert plan(shape(FWD_SAVE, [100], nlines=64, tmax=200, ncu=256, emu=0))["fwd"] == NF_FUSED    # 64 x 200: the fused forward by the default rule
