"""The kernel choice of the matrix products around the recurrences, checked without running a kernel: runtime.inc:product_plan (through
clstm_debug_product_plan, which needs no net and no device) against its one Python restatement, tests/product_rule.py -- for every precision
mode, strict and not, one and two layers and directions, want_dx0 on and off, every combination of the fact flags, chips of 16, 104, 256 and
304 CUs, and both sides of every bound of the rule.  And the property the two passes rest on: the rows and the tile height of the
bf16-source weight gradient, and whether the x block may stay external, do not depend on any fact."""
import itertools

import pytest

import product_rule as pr
from common import emu_lib
from product_rule import BWD, FWD

CHIPS = (16, 104, 256, 304)
FACT_SETS = list(itertools.product((0, 1), repeat=len(pr.FACTS)))


def first_r_without_256_tiles(cn):
    """the first R >= 192 at which 256-tiles lose the 25 % padding rule against 128-tiles"""
    return next(r for r in range(192, 4096) if not pr.tile256(r, cn))


# (ni of the net, cells per layer, frames, classes): every bound of the rule from both sides
GEOMETRIES = [
    (70, [24], 200, 83), (71, [24], 200, 83), (71, [23], 200, 83),               # product rows 95 | 96 at 96 columns; 92 columns
    (142, [48], 200, 83), (143, [48], 200, 83), (143, [47], 200, 83),            # rows 191 | 192 at 192 columns; 188 columns
    (127, [128], 300, 83), (128, [128], 300, 83),                                # rows 256 | 257 at 512 columns: the 25 % padding rule (below)
    (319, [256], 400, 83), (320, [256], 400, 83), (321, [256], 400, 83),         # 576 | 577 | 578 rows: 192- against 256-row tiles
    (16, [256, 384], 149, 7),                                                    # 896 rows without the bias row: 192-row tiles, 512 % 192 != 0 -> copied
    (16, [256, 128], 149, 7), (16, [512, 512], 149, 7),                          # 1537 rows: 256-row tiles, external
    (64, [256, 512], 6400, 83), (64, [512, 512], 25600, 83),                     # the configs[4] layers: 577 and 1537 rows
    (16, [96, 64], 200, 6), (12, [32, 32], 24, 6), (12, [64, 32], 24, 6),        # the merged launch; the small nets of the parity tests
    (48, [160], 100, 96), (48, [160], 100, 97), (48, [160], 96, 97), (48, [160], 95, 97),   # classes 96 | 97; frames 95 | 96 of the big-tile logits
    (48, [100], 63, 83), (48, [100], 64, 83), (48, [100], 65, 83), (48, [9], 4096, 5), (48, [9], 4097, 5), (48, [9], 4032, 5),   # slab clamps: 1, 64, 63
    (44, [32], 200, 83), (48, [36], 200, 83), (48, [33], 200, 83), (47, [33, 34], 200, 83),   # ni % 8, no % 8, no odd / even
]


def test_the_geometries_sit_on_the_bounds():
    assert first_r_without_256_tiles(512) == 257 and pr.tile256(256, 512) and 1 + 127 + 128 == 256
    assert pr.mc_tile_rows(576) == 192 and pr.mc_tile_rows(577) == 256 and 1 + 319 + 256 == 576
    assert (pr.big(95, 96), pr.big(96, 96), pr.big(96, 95)) == (False, True, False)
    assert (pr.tile256(191, 192), pr.tile256(192, 192), pr.tile256(192, 191)) == (False, True, False)
    # [256, 384]: with the bias row 897 rows, without it 896: both 192-row tiles here, and the 512 x columns fill no whole number of them
    p = pr.plan(pr.shape(BWD, [256, 384], ni=16, precision=2, frames=149))
    assert (p["dw16_rows"], p["dw16_tile"], p["x_external"], p["a2_rows"]) == (896, 192, 0, 0) and p["dw"][0] == pr.PK_B16MC
    # configs[4]: 577 rows -> 576 in 192-row tiles, first layer; 1537 -> 1536 in 256-row tiles, the 1024 x rows external, one launch with x.d
    p = pr.plan(pr.shape(BWD, [512, 512], layer=0, ni=64, precision=2, frames=25600))
    assert (p["dw16_rows"], p["dw16_tile"], p["bias_out"], p["a2_rows"]) == (576, 192, 1, 0)
    p = pr.plan(pr.shape(BWD, [512, 512], ni=64, precision=2, frames=25600))
    assert (p["dw16_rows"], p["dw16_tile"], p["x_external"], p["a2_rows"], p["merged"]) == (1536, 256, 1, 1024, 1)
    assert p["moves"] == sum(1 << c for c in (3, 4, 8, 13, 14))
    # the slab clamps
    assert pr.plan(pr.shape(BWD, [100], frames=64))["dw"][3] == 1 and pr.plan(pr.shape(BWD, [100], frames=65))["dw"][3] == 2
    assert pr.plan(pr.shape(BWD, [9], frames=4096, nc=5))["dw"][3] == 64 and pr.plan(pr.shape(BWD, [9], frames=4032, nc=5))["dw"][3] == 63


@pytest.mark.parametrize("uni", [False, True], ids=["bidi", "uni"])
@pytest.mark.parametrize("strict", [False, True], ids=["", "strict"])
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_the_library_plans_what_the_rule_says(precision, strict, uni):
    """every geometry x layer x pass x fact set x chip x want_dx0 x forced-wide: the library's plan is the restated one"""
    n, lib = 0, emu_lib()
    for ni, nh, frames, nc in GEOMETRIES:
        for layer, pass_, facts, force_wide in itertools.product(range(len(nh)), (FWD, BWD), FACT_SETS, (False, True)):
            for ncu, dx0 in ((16, False), (104, True), (256, False), (304, True), (256, True)):
                h = pr.shape(pass_, nh, layer=layer, ni=ni, uni=uni, nc=nc, frames=frames, precision=precision, strict=strict, ncu=ncu, want_dx0=dx0,
                             force_wide=force_wide, **dict(zip(pr.FACTS, facts)))
                pr.assert_plan_agrees(lib, h)
                n += 1
    assert n > 25000


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_options_and_recurrence_plans(precision):
    """the options the rule reads, and the answers of the narrow plans it depends on, at the geometries where each of them matters"""
    lib = emu_lib()
    opts = [dict(gemm_x3=0), dict(split_terms=2), dict(gemm_b16mc=0), dict(gemm_stag=1), dict(gemm_stag=0), dict(pack_tiles=0), dict(fuse_wx=0), dict(fuse_wx=2),
            dict(fwd_family=1), dict(fwd_family=pr.NF_FUSED), dict(fwd_family=pr.NF_MFMA), dict(overlapped=1, dw_slabs_per_dir=17),
            dict(overlapped=1, dw_slabs_per_dir=9, dwx=1, dwx_nslabs=5), dict(overlapped=1, dw_slabs_per_dir=9, dwx=1, dwx_nslabs=5, xd=1),
            dict(overlapped=1, dw_slabs_per_dir=9, dwx=1, dwx_nslabs=3, xd=2)]
    for (ni, nh, frames, nc), kw, pass_, ncu in itertools.product(GEOMETRIES, opts, (FWD, BWD), CHIPS):
        for layer in range(len(nh)):
            for facts in ((0,) * 5, (1,) * 5, None):
                f = dict(zip(pr.FACTS, facts)) if facts else {}
                pr.assert_plan_agrees(lib, pr.shape(pass_, nh, layer=layer, ni=ni, nc=nc, frames=frames, precision=precision, ncu=ncu, **kw, **f))


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_one_answer_across_passes(precision):
    """dw_rows, the tile height and x_external do not change when the fact flags do, nor with the pass: the forward pass may leave the x block
    external exactly where the backward pass will launch with tiles it fills"""
    lib = emu_lib()
    for (ni, nh, frames, nc), uni, force_wide in itertools.product(GEOMETRIES, (False, True), (False, True)):
        for layer in range(len(nh)):
            seen = set()
            for pass_, facts in itertools.product((FWD, BWD), FACT_SETS):
                h = pr.shape(pass_, nh, layer=layer, ni=ni, uni=uni, nc=nc, frames=frames, precision=precision, force_wide=force_wide, **dict(zip(pr.FACTS, facts)))
                p = pr.library_plan(lib, h)
                seen.add(tuple(p[k] for k in pr.ACROSS_PASSES))
                # what a pass does with them: an external block fills whole tiles of the launch it is external to
                if p["a2_rows"]:
                    assert p["x_external"] and p["a2_rows"] == h.ni and h.ni % p["dw16_tile"] == 0
                if pass_ == BWD and p["dw"][0] in (pr.PK_B16MC, pr.PK_DW_DX):
                    assert p["dw"][1:3] == (p["dw16_tile"], p["dw16_rows"])
            assert len(seen) == 1, (ni, nh, layer, seen)
