"""The rule of the matrix products around the recurrences -- the input projection W_x.x, the softmax layer's logits, its W.d and x.d, a
layer's weight gradient and its input deltas -- restated ONCE in Python: clstm_amd/csrc/runtime.inc:product_plan from the shape
clstm_amd/csrc/net.inc:Net::product_shape fills.  test_product_plan.py compares it with the library's own answer
(clstm_debug_product_plan: host arithmetic, no net, no device) for every mode, fact and chip size and at both sides of every bound;
test_wide_layer_sweep.py and the bf16 cases of test_net_parity.py predict the path counters 2, 3, 4, 8, 13, 14 of their cases from it.

shape() lays a ProductShape out as Net::product_shape does for one layer of a net; plan() is the rule; library_plan() asks the library;
step_moves() is what one forward + backward of a net moves given which recurrences ran persistent, net_moves() the same with that
question put to the library's own lock-step rule (clstm_debug_wide_plan) layer by layer, as Net::forward_pass and Net::backward do."""
import ctypes
from types import SimpleNamespace

FWD, BWD = 0, 1                                                                   # runtime.inc:ProductPass
(PK_NONE, PK_F32, PK_BF16, PK_B16KK, PK_B16MC, PK_DW_DX, PK_X3, PK_X3_BIG, PK_X3_PAIR, PK_F32_PAIR, PK_SOFTMAX_FUSED) = range(11)   # ProductKernel
PW_SBF, PW_HBF, PW_DBF = 1, 2, 4                                                  # ProductWrites
PS_H, PS_S, PS_D = 1, 2, 4                                                        # ProductSkips
PN_SOURCE, PN_DELTA_F32, PN_H_BELOW = 1, 2, 4                                     # ProductNeeds
NF_FUSED, NF_MFMA = 2, 3                                                          # runtime.inc:NarrowFwd
PC_WX_FROM_BF16, PC_DX_FROM_BF16, PC_DW_FROM_BF16, PC_DW_X_EXTERNAL, PC_DW_BIAS_OUT, PC_DW_DX_ONE_LAUNCH = 2, 3, 4, 8, 13, 14
PRODUCT_COUNTERS = (2, 3, 4, 8, 13, 14)
SMX_COLS, GB_BK = 96, 32                                                          # softmax_fused.h, gemm_bf16.h
SHAPE_FIELDS = ("pass_", "ni", "no", "ndir", "wide", "first", "top", "nlayers", "bwd_exact", "kp16f_is_no", "N", "bs", "nclasses", "sm_ni", "precision",
                "gemm_x3_on", "split_terms", "strict", "gemm_b16mc", "gemm_stag", "pack_tiles", "fuse_wx", "ncu", "want_dx0", "fwd_family", "overlapped",
                "dwx", "xd", "dw_slabs_per_dir", "dwx_nslabs", "below_hbf", "fwd_sbf", "bwd_persistent", "packs", "above_packs")
FACTS = ("below_hbf", "fwd_sbf", "bwd_persistent", "packs", "above_packs")
PRODUCTS = ("wx", "logits", "sm_wd", "sm_xd", "dw", "dx")
SCALARS = ("merged", "bias_out", "dw16_rows", "dw16_tile", "x_external", "a2_rows", "x_copy", "fx_mode", "tiled_pack", "stag", "terms", "writes", "skips",
           "needs", "moves")
ACROSS_PASSES = ("dw16_rows", "dw16_tile", "x_external")                          # functions of the shape and the mode alone


def big(r, c):
    """gemm_bf16_big: shapes that fill 128 x 128 tiles reasonably"""
    return r >= 96 and c >= 96


def tile256(r, c):
    """gemm_tile256: 256 x 256 tiles where their padding costs at most 25 % more work than 128 x 128 tiles do"""
    if r < 192 or c < 192:
        return False
    w256, w128 = ((r + 255) // 256) * ((c + 255) // 256) * 4, ((r + 127) // 128) * ((c + 127) // 128)
    return 4 * w256 <= 5 * w128


def mc_tile_rows(r):
    """gemm_mc_tile_rows: 192 rows where that pads r less than 256 do"""
    return 192 if (r + 191) // 192 * 192 < (r + 255) // 256 * 256 else 256


def mc_rows_per_tile(r, c):
    return mc_tile_rows(r) if tile256(r, c) else 128


def shape(pass_, nh, layer=None, ni=48, uni=False, nc=83, frames=64, nlines=4, precision=0, strict=False, gemm_x3=1, split_terms=3, gemm_b16mc=1,
          gemm_stag=2, pack_tiles=1, fuse_wx=1, ncu=256, want_dx0=False, force_wide=False, fwd_family=0, overlapped=0, dwx=0, xd=0, dw_slabs_per_dir=0,
          dwx_nslabs=0, below_hbf=None, fwd_sbf=None, bwd_persistent=None, packs=None, above_packs=None):
    """The ProductShape of layer `layer` (default: the top one) of a net of len(nh) layers as net.inc:Net::product_shape fills it.  The facts
    default to what a net of wide layers leaves when every persistent kernel ran (None): pass 0 / 1 explicitly for the other outcomes."""
    layer = len(nh) - 1 if layer is None else layer
    ndir, no = 1 if uni else 2, nh[layer]
    wide = lambda n: n > 128 or force_wide                                        # runtime.inc:narrow_class, CLSTM_FORCE_WIDE
    x_ni = ni if layer == 0 else ndir * nh[layer - 1]
    exact = (4 * no + 127) // 128 * 128 == 4 * no                                 # net.inc:Net::build, wide_kp16_bwd
    rec = precision == 2
    h = SimpleNamespace(
        pass_=pass_, ni=x_ni, no=no, ndir=ndir, wide=int(wide(no)), first=int(layer == 0), top=int(layer == len(nh) - 1), nlayers=len(nh),
        bwd_exact=int(exact), kp16f_is_no=int((no + 127) // 128 * 128 == no), N=frames, bs=nlines, nclasses=nc, sm_ni=ndir * nh[-1], precision=precision,
        gemm_x3_on=0 if strict else gemm_x3, split_terms=split_terms, strict=int(strict), gemm_b16mc=gemm_b16mc, gemm_stag=gemm_stag, pack_tiles=pack_tiles,
        fuse_wx=fuse_wx, ncu=ncu, want_dx0=int(want_dx0), fwd_family=fwd_family, overlapped=overlapped, dwx=dwx, xd=xd, dw_slabs_per_dir=dw_slabs_per_dir,
        dwx_nslabs=dwx_nslabs)
    # what the launches leave when every persistent kernel runs: Net::forward_pass (run_wide), Net::repack
    writes_hbf = lambda l: rec and wide(nh[l]) and nh[l] % 2 == 0 and l + 1 < len(nh)
    sbf = rec and wide(no) and gemm_b16mc and x_ni % 8 == 0 and no % 8 == 0 and exact
    h.below_hbf = int(layer > 0 and writes_hbf(layer - 1)) if below_hbf is None else below_hbf
    h.fwd_sbf = int(pass_ == BWD and sbf) if fwd_sbf is None else fwd_sbf
    h.bwd_persistent = int(pass_ == BWD and bool(wide(no))) if bwd_persistent is None else bwd_persistent
    h.packs = int(rec and wide(no)) if packs is None else packs
    h.above_packs = int(rec and layer + 1 < len(nh) and wide(nh[layer + 1])) if above_packs is None else above_packs
    return h


def plan(h):
    """runtime.inc:product_plan, as a dict: PRODUCTS -> (kernel, tile, rows, slabs), SCALARS -> int"""
    p = dict.fromkeys(SCALARS, 0)
    p.update({k: (PK_NONE, 0, 0, 0) for k in PRODUCTS})
    bf16_gemm, bf16_rec, x3 = h.precision >= 1, h.precision == 2, bool(h.gemm_x3_on and not h.strict)
    N, M, R, Cn, nc = h.N, h.ndir * 4 * h.no, 1 + h.ni + h.no, 4 * h.no, h.nclasses
    sq = lambda r, c: 128 if big(r, c) else 64
    kk = lambda r, c: 256 if tile256(r, c) else 128
    clamp = lambda want: max(1, min(want, (N + 63) // 64, 64))                    # at least 64 frames per slab, 1..64 slabs

    def split(r, c, nbatch, tile):                                                # 640 workgroups of 64 x 64 tiles, 480 of 128 x 128
        tiles = ((r + tile - 1) // tile) * ((c + tile - 1) // tile) * nbatch
        return clamp(((640 if tile == 64 else 480) + tiles - 1) // tiles)

    def split_mc(r, c, nbatch):                                                   # one workgroup per CU, never a second round
        th = mc_tile_rows(r)
        return clamp(h.ncu // (((r + th - 1) // th) * ((c + 255) // 256) * nbatch))
    p["stag"], p["terms"] = h.gemm_stag, 3 if h.split_terms >= 3 else 2
    p["dw16_rows"] = R - 1 if h.bwd_exact and big(R - 1, Cn) else R
    p["dw16_tile"] = mc_rows_per_tile(p["dw16_rows"], Cn)
    p["x_external"] = int(bf16_rec and not h.first and h.ni % p["dw16_tile"] == 0)
    x_from_hbf = bool(bf16_rec and not h.first and h.below_hbf and h.packs and h.ni % 2 == 0)
    if h.pass_ == FWD:
        p["tiled_pack"] = int(bool(h.wide and bf16_rec and h.no % 128 == 0 and h.ni % 32 == 0 and h.kp16f_is_no and h.bwd_exact and h.pack_tiles))
        if h.wide and bf16_rec:
            if h.gemm_b16mc and h.ni % 8 == 0 and h.no % 8 == 0 and h.bwd_exact:
                p["writes"] |= PW_SBF
                p["skips"] |= PS_S
            if h.no % 2 == 0 and not h.top:
                p["writes"] |= PW_HBF
                if h.above_packs:
                    p["skips"] |= PS_H
        p["fx_mode"] = h.fuse_wx if h.wide and bf16_rec and h.packs and (h.first or x_from_hbf) else 0
        if not h.first and not x_from_hbf:
            p["needs"] |= PN_H_BELOW
        if h.fwd_family == NF_FUSED:
            return p
        if h.fwd_family == NF_MFMA:
            pass
        elif x_from_hbf:
            p["wx"] = (PK_B16KK, kk(N, M), N, 1)
        elif bf16_rec and h.first and h.wide and h.packs and h.ni % 8 == 0 and tile256(N, M):
            p["wx"], p["x_copy"] = (PK_B16KK, 256, N, 1), 1
        elif bf16_gemm:
            p["wx"] = (PK_BF16, sq(N, M), N, 1)
        else:
            p["wx"] = (PK_F32, 64, N, 1)
        if p["wx"][0] == PK_B16KK:
            p["moves"] |= 1 << PC_WX_FROM_BF16
        p["a2_rows"] = h.ni if x_from_hbf and p["x_external"] else 0
        if h.top:
            p["logits"] = (PK_SOFTMAX_FUSED, 0, N, 1) if nc <= SMX_COLS else (PK_X3_BIG, 128, N, 1) if bf16_gemm and x3 and big(N, nc) else (PK_F32, 64, N, 1)
        return p
    if h.wide and bf16_rec and h.bwd_exact:
        p["writes"] |= PW_DBF
        if bf16_gemm:
            p["skips"] |= PS_D
    if h.top:
        sR = 1 + h.sm_ni
        sm_big = bf16_gemm and x3 and big(sR, nc) and big(N, h.sm_ni)
        ns = h.dwx_nslabs if h.dwx else split(sR, nc, 1, 128 if sm_big else 64)
        pair = PK_X3_PAIR if x3 else PK_F32_PAIR
        p["sm_wd"] = (PK_NONE, 64, sR, ns) if h.dwx else (PK_X3_BIG, 128, sR, ns) if sm_big else (pair, 64, sR, ns)
        p["sm_xd"] = (PK_NONE if h.xd else PK_X3, 64, N, 1) if h.dwx else (PK_X3_BIG, 128, N, 1) if sm_big else (pair, 64, N, 1)
    dw16 = bool(bf16_rec and h.bwd_persistent and h.fwd_sbf and h.bwd_exact and big(R, Cn))
    rows = p["dw16_rows"] if dw16 else R
    p["bias_out"] = int(rows < R)
    x3_big = not bf16_gemm and h.wide and x3 and big(R, Cn)
    if h.overlapped:
        ns = h.dw_slabs_per_dir
    elif p["bias_out"] and tile256(rows, Cn):
        ns = split_mc(rows, Cn, h.ndir)
    elif dw16 and tile256(R, Cn):
        ns = split_mc(R, Cn, h.ndir)
    elif (bf16_gemm or x3_big) and big(R, Cn):
        ns = split(R, Cn, h.ndir, 128)
    else:
        ns = split(R, Cn, h.ndir, 64)
    has_dx = not h.first or h.want_dx0
    dx16 = bool(bf16_rec and h.bwd_persistent and h.bwd_exact and h.packs)
    p["merged"] = int(bool(dw16 and p["bias_out"] and not h.first and dx16 and h.gemm_stag == 2 and tile256(rows, Cn) and tile256(N, h.ni)
                           and M % GB_BK == 0 and M >= 2 * GB_BK))
    if h.overlapped:
        p["dw"] = (PK_NONE, 64, R, ns)
    elif dw16:
        p["dw"] = (PK_DW_DX if p["merged"] else PK_B16MC, p["dw16_tile"], rows, ns)
    elif bf16_gemm:
        p["dw"] = (PK_BF16, sq(R, Cn), R, ns)
    else:
        p["dw"] = (PK_X3_BIG, 128, R, ns) if x3_big else (PK_F32, 64, R, ns)
    if has_dx:
        if p["merged"]:
            p["dx"] = (PK_DW_DX, 256, N, 1)
        elif dx16:
            p["dx"] = (PK_B16KK, kk(N, h.ni), N, 1)
        elif bf16_gemm:
            p["dx"] = (PK_BF16, sq(N, h.ni), N, 1)
        else:
            p["dx"] = (PK_X3_BIG, 128, N, 1) if h.wide and x3 and big(N, h.ni) else (PK_F32, 64, N, 1)
    p["a2_rows"] = h.ni if dw16 and x_from_hbf and p["x_external"] else 0
    if not dw16:
        p["needs"] |= PN_SOURCE | PN_DELTA_F32
    if has_dx and p["dx"][0] not in (PK_DW_DX, PK_B16KK):
        p["needs"] |= PN_DELTA_F32
    p["moves"] = ((1 << PC_DW_FROM_BF16 if dw16 else 0) | (1 << PC_DW_BIAS_OUT if p["bias_out"] else 0) | (1 << PC_DW_X_EXTERNAL if p["a2_rows"] else 0)
                  | (1 << PC_DW_DX_ONE_LAUNCH if p["merged"] else 0) | (1 << PC_DX_FROM_BF16 if p["dx"][0] in (PK_DW_DX, PK_B16KK) else 0))
    return p


def library_plan(lib, h):
    """clstm_debug_product_plan (include/clstm_abi.h) for the same shape"""
    ints = (ctypes.c_int * len(SHAPE_FIELDS))(*(int(getattr(h, f)) for f in SHAPE_FIELDS))
    out = (ctypes.c_int * (4 * len(PRODUCTS) + len(SCALARS)))()
    lib.call("clstm_debug_product_plan", ctypes.addressof(ints), ctypes.addressof(out))
    got = {k: tuple(out[4 * i:4 * i + 4]) for i, k in enumerate(PRODUCTS)}
    got.update(zip(SCALARS, out[4 * len(PRODUCTS):]))
    return got


def assert_plan_agrees(lib, h):
    got, want = library_plan(lib, h), plan(h)
    assert got == want, (vars(h), {k: (got[k], want[k]) for k in got if got[k] != want[k]})
    return want


def step_moves(lib, nh, ni, nlines, frames, precision, persistent_fwd, persistent_bwd, fx=(), **kw):
    """{counter: moves} among PRODUCT_COUNTERS of one forward + backward of a net whose layers are all wide, every plan checked against the
    library's.  persistent_fwd / persistent_bwd: per layer, whether the persistent kernel of that pass ran (the caller's wide rule says);
    fx: the layers whose input projection ran inside the forward kernel (counter 6): their hoisted product, and its counter 2, do not run."""
    total, hbf = dict.fromkeys(PRODUCT_COUNTERS, 0), 0
    sbf = []
    for layer in range(len(nh)):
        f = assert_plan_agrees(lib, shape(FWD, nh, layer=layer, ni=ni, frames=frames, nlines=nlines, precision=precision, below_hbf=hbf,
                                          fwd_sbf=0, bwd_persistent=0, **kw))
        ran = precision == 2 and persistent_fwd[layer]
        hbf = int(ran and bool(f["writes"] & PW_HBF))
        sbf.append(int(ran and bool(f["writes"] & PW_SBF)))
        moves = 0 if layer in fx else f["moves"]
        for c in PRODUCT_COUNTERS:
            total[c] += moves >> c & 1
    for layer in range(len(nh)):
        below = layer > 0 and precision == 2 and persistent_fwd[layer - 1]
        f = shape(FWD, nh, layer=layer - 1, ni=ni, frames=frames, nlines=nlines, precision=precision, **kw) if layer else None
        b = assert_plan_agrees(lib, shape(BWD, nh, layer=layer, ni=ni, frames=frames, nlines=nlines, precision=precision,
                                          below_hbf=int(below and bool(plan(f)["writes"] & PW_HBF)), fwd_sbf=sbf[layer],
                                          bwd_persistent=int(persistent_bwd[layer]), **kw))
        for c in PRODUCT_COUNTERS:
            total[c] += b["moves"] >> c & 1
    return {c: n for c, n in total.items() if n}


def wide_plan(lib, fwd, no, x_ni, ndir, nlines, tmax, frames, ncu, precision, strict, fx_mode, sbf):
    """(kernel, moves) of clstm_debug_wide_plan for the shape net.inc:Net::wide_shape fills (CLSTM_XCD_REC on, no placement failure, bwd_c32 = 1)"""
    up = lambda n, q: (n + q - 1) // q * q
    shape = (ctypes.c_int * 20)(fwd, no, x_ni, ndir, nlines, tmax, frames, up(no, 64) if fwd else up(4 * no, 64), up(no, 128) if fwd else up(4 * no, 128),
                                precision == 2, not fwd and precision == 0 and not strict, fx_mode, ncu, 1, 0, 1, sbf, x_ni + no + 8, up(1 + x_ni + no, 16),
                                up(4 + ndir * no, 16))
    out = (ctypes.c_int * 14)()
    lib.call("clstm_debug_wide_plan", ctypes.addressof(shape), ctypes.addressof(out))
    return out[0], out[12]


def net_moves(lib, nh, ni, T, precision, ncu, uni=False, strict=False, **kw):
    """{counter: moves} among PRODUCT_COUNTERS of one forward + backward of the net on lines of T frames: every layer's product plans (checked
    against the library's) with the facts its lock-step plans leave -- a planned persistent kernel runs"""
    ndir, frames, wide = 1 if uni else 2, sum(T), lambda n: n > 128 or kw.get("force_wide", False)
    total, hbf, sbf = dict.fromkeys(PRODUCT_COUNTERS, 0), [0] * (len(nh) + 1), []
    args = dict(ni=ni, uni=uni, frames=frames, nlines=len(T), precision=precision, strict=strict, ncu=ncu, **kw)
    for layer, no in enumerate(nh):
        h = shape(FWD, nh, layer=layer, below_hbf=hbf[layer], fwd_sbf=0, bwd_persistent=0, **args)
        f = assert_plan_agrees(lib, h)
        kernel = wide_plan(lib, 1, no, h.ni, ndir, len(T), max(T), frames, ncu, precision, strict, f["fx_mode"], f["writes"] & PW_SBF)[0] if wide(no) else 0
        ran = precision == 2 and kernel != 0
        hbf[layer + 1] = int(ran and bool(f["writes"] & PW_HBF))
        sbf.append(int(ran and bool(f["writes"] & PW_SBF)))
        for c in PRODUCT_COUNTERS:
            total[c] += 0 if kernel == 3 else f["moves"] >> c & 1                  # (3: the input projection ran inside lstm_xcd_fwd_bf16_fx)
    for layer, no in enumerate(nh):
        h = shape(BWD, nh, layer=layer, below_hbf=hbf[layer], fwd_sbf=sbf[layer], bwd_persistent=0, **args)
        h.bwd_persistent = int(wide(no) and wide_plan(lib, 0, no, h.ni, ndir, len(T), max(T), frames, ncu, precision, strict, 0, 0)[0] != 0)
        b = assert_plan_agrees(lib, h)
        for c in PRODUCT_COUNTERS:
            total[c] += b["moves"] >> c & 1
    return {c: n for c, n in total.items() if n}
