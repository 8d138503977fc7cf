"""The narrow (register-resident, nhidden <= 128) layer's launch rule, restated ONCE in Python: clstm_amd/csrc/runtime.inc:narrow_class /
narrow_plan from the shape clstm_amd/csrc/net.inc:Net::narrow_shape fills.  test_cell_count_sweep.py, test_xd_producers.py and
test_predict.py predict the path counters of their cases from it -- which form ran follows from the rule, never from the result -- and
test_narrow_plan.py compares it with the library's own answer (clstm_debug_narrow_plan: host arithmetic, no net, no device) for every cell
count, option and chip size and at both sides of every bound, so the restatement cannot drift from the rule unnoticed.

shape() lays a NarrowShape out as Net::narrow_shape does for one layer of a net; plan() is the rule; library_plan() asks the library.
geometry / overlapped / fused_forward / xd_form are the questions the parity tests ask, answered by plan()."""
import ctypes
import os
from types import SimpleNamespace

LIM = 2147483000.0                                   # 32-bit byte offsets inside one descriptor
PROG_LINES, PROG_WORDS = 2048, 2 * 2048 * 32         # runtime.inc:PROG_LINES, net.inc:Net::PROG_WORDS (devintrin.h:PROG_STRIDE = 32)
FWD_CW, FWD_JW, FWD_CG, SMX_COLS, XD_MAX_K = 6, 5, 14, 96, 96   # lstm_fwd_fused.h, softmax_fused.h, lstm_xd_prologue.h
FWD_SAVE, FWD_NOSAVE, BWD = 0, 1, 2                  # runtime.inc:NarrowPass
NF_LINE, NF_FUSED, NF_MFMA = 1, 2, 3                 # runtime.inc:NarrowFwd
NB_LINE, NB_LINE_DW, NB_LINE_XD_DW, NB_BWD_DW, NB_MFMA, NB_MFMA_THEN_DW, NB_MFMA_DW = 1, 2, 3, 4, 5, 6, 7   # runtime.inc:NarrowBwd
PC_FWD_FUSED, PC_MFMA_NOSAVE, PC_MFMA_FWD, PC_MFMA_BWD, PC_MFMA_BWD_DW, PC_LINE_NOSAVE, PC_FUSED_NOSAVE, PC_XD_PROLOGUE, PC_XD_PRODUCERS = 5, 15, 16, 17, 18, 22, 23, 26, 27
MFMA_FWD_CELLS, MFMA_NOSAVE_CELLS, MFMA_BWD_CELLS = (64, 100, 128), (64, 100), (64, 100)        # runtime.inc:MFMA_GEOMS
SHAPE_FIELDS = ("pass_", "no", "ni", "ndir", "nlayers", "first", "top", "bs", "tmax", "N", "nc", "ldh", "lds", "ldx", "h_cap", "d_cap", "wk", "wk_njp",
                "w1k_kps", "overlap", "bf16_gemm", "strict_f32", "dw_x3", "split_terms", "fwd_mfma", "bwd_mfma", "bwd_mfma_fused", "xd_prologue", "ncu", "emu")
PLAN_FIELDS = ("nk4", "ku", "waves", "fwd", "saves", "overlapped", "bwd", "terms", "dwx", "xd", "moves")


def geometry(no):
    """(nk4, ku, waves, waves in group B, last lane owns a cell) of a layer of `no` cells; nk4 = ku = None where no register-resident
    instantiation exists (the layer is wide)"""
    need = ((no + 3) // 4 + 3) // 4                                               # runtime.inc:narrow_class: the first class that holds the k-quads
    nk4 = next((v for v in (1, 2, 4, 7, 8) if v >= need), None)                   # runtime.inc:NARROW_CLASSES
    if nk4 is None:
        return None, None, 1, 0, False                                            # net.inc:Net::build: wide layers launch one wave per workgroup role
    ku = 25 if nk4 == 7 and (no + 3) // 4 == 25 else 4 * nk4                      # ... KU exact for 97..100 cells, padded elsewhere
    waves = (no + 15) // 16                                                       # net.inc:Net::build, y.nthreads = 64 * waves
    group_b = waves - 4 if nk4 >= 5 else 0                                        # devintrin.h:stag_on, group A = waves 0..3
    return nk4, ku, waves, group_b, no % 16 == 0


def klass(no):
    return geometry(no)[:3]


def narrow(no):
    return geometry(no)[0] is not None


def cus(kind):
    """runtime.inc:device_cu_count"""
    return 256 if kind == "hip" else int(os.environ.get("CLSTM_EMU_CUS", 16))


def grown(n):
    """runtime.inc:DevBuf::reserve of n elements into an empty buffer"""
    return n + n // 4 + 64


def shape(pass_, nh, layer=None, ni=48, uni=False, nc=83, nlines=1, tmax=1, frames=None, overlap=None, strict=False, bf16_gemm=False, kind="hip",
          ncu=None, emu=None, dw_x3=1, split_terms=3, fwd_mfma=1, bwd_mfma=1, bwd_mfma_fused=1, xd_prologue=2, h_cap=None, d_cap=None):
    """The NarrowShape of layer `layer` (default: the top one) of a net of len(nh) layers as net.inc:Net::narrow_shape fills it: `nlines` lines
    of at most `tmax` frames, `frames` in all (default nlines * tmax); overlap None: the library's default, 1; strict: clstm_net_set_strict_f32,
    which clears dw_x3 (abi.inc); the buffer capacities default to what a fresh net's first minibatch reserves (Net::reserve_batch)."""
    layer = len(nh) - 1 if layer is None else layer
    ndir, no = 1 if uni else 2, nh[layer]
    ldh = lambda n: (4 + ndir * n + 15) // 16 * 16                                # net.inc:Net::build
    x_ni = ni if layer == 0 else ndir * nh[layer - 1]
    n = nlines * tmax if frames is None else frames
    wk = len(nh) == 1 and narrow(no) and nc <= SMX_COLS                           # net.inc:Net::build: the fused forward's packed operands
    h = SimpleNamespace(
        pass_=pass_, no=no, ni=x_ni, ndir=ndir, nlayers=len(nh), first=int(layer == 0), top=int(layer == len(nh) - 1), bs=nlines, tmax=tmax, N=n, nc=nc,
        ldh=ldh(no), lds=(1 + x_ni + no + 15) // 16 * 16, ldx=ni if layer == 0 else ldh(nh[layer - 1]),
        h_cap=grown(n * ldh(no) + 64 + (PROG_WORDS if wk else 0)) if h_cap is None else h_cap,
        d_cap=grown(n * ndir * 4 * no + PROG_WORDS + 64) if d_cap is None else d_cap,
        wk=int(wk), wk_njp=(4 * no + 15) // 16 if wk else 0, w1k_kps=(ndir * no + 15) // 16 * 16 if wk else 0,
        overlap=1 if overlap is None else overlap, bf16_gemm=int(bf16_gemm), strict_f32=int(strict), dw_x3=0 if strict else dw_x3, split_terms=split_terms,
        fwd_mfma=fwd_mfma, bwd_mfma=bwd_mfma, bwd_mfma_fused=bwd_mfma_fused, xd_prologue=xd_prologue,
        ncu=cus(kind) if ncu is None else ncu, emu=int(kind == "emu") if emu is None else int(emu))
    h.h_cap, h.d_cap = min(h.h_cap, 2 ** 31 - 1), min(h.d_cap, 2 ** 31 - 1)
    return h


def plan(h):
    """runtime.inc:narrow_plan, as a dict of PLAN_FIELDS"""
    nk4, ku, waves, _, owns = geometry(h.no)
    assert nk4 is not None, "a wide layer has no narrow plan"
    p = dict.fromkeys(PLAN_FIELDS, 0)
    p.update(nk4=nk4, ku=ku, waves=waves)
    gates32 = h.N * h.ndir * 4 * h.no * 4 < LIM
    big_enough = h.overlap != 1 or (h.tmax >= 64 and h.N >= 2048)               # overlap = 1 (the rule): only minibatches large enough to profit
    if h.pass_ != BWD:
        mfma = bool(not h.emu and h.fwd_mfma and not h.bf16_gemm and not (h.strict_f32 and h.fwd_mfma < 2) and h.no in MFMA_FWD_CELLS and h.ni == 48
                    and gates32 and h.N * h.ldh * 4 < LIM and h.N * h.lds * 4 < LIM and h.N * h.ldx * 4 < LIM and (h.fwd_mfma >= 2 or h.bs >= 640))
        fused = bool(not mfma and h.overlap and h.nlayers == 1 and not h.bf16_gemm and h.wk and waves >= FWD_CW and not owns
                     and h.wk_njp <= FWD_JW * FWD_CW and h.w1k_kps <= 16 * FWD_CG and h.nc <= SMX_COLS and h.bs <= PROG_LINES and h.bs < 1 << 18
                     and h.tmax < 1 << 16 and big_enough and h.h_cap * 4 < LIM and h.bs * h.ndir <= h.ncu - max(8, h.ncu // 8))
        p["fwd"] = NF_MFMA if mfma else NF_FUSED if fused else NF_LINE
        p["saves"] = int(h.pass_ == FWD_SAVE or (mfma and h.no not in MFMA_NOSAVE_CELLS))
        if mfma:
            p["moves"] = 1 << (PC_MFMA_FWD if p["saves"] else PC_MFMA_NOSAVE)
        elif fused:
            p["moves"] = 1 << (PC_FWD_FUSED if p["saves"] else PC_FUSED_NOSAVE)
        elif not p["saves"]:
            p["moves"] = 1 << PC_LINE_NOSAVE
        return p
    over = bool(not h.bf16_gemm and h.overlap and not owns and h.bs <= PROG_LINES and big_enough and h.d_cap * 4 < LIM and (h.overlap == 2 or waves >= 4))
    mfma = bool(not h.emu and h.bwd_mfma and not h.bf16_gemm and not (h.strict_f32 and h.bwd_mfma < 2) and h.no in MFMA_BWD_CELLS and gates32
                and (h.bwd_mfma >= 2 or h.bs >= 640))
    terms = 0 if not h.dw_x3 else 3 if h.split_terms >= 3 else 2
    dwx = bool(h.top and h.dw_x3 and over and h.bs * h.ndir * 4 <= 3 * h.ncu)
    one_launch = not h.emu and waves >= 4 and not mfma
    xd = 0
    if dwx and not mfma and h.nc <= XD_MAX_K and h.xd_prologue != 0:
        xd = 2 if h.xd_prologue >= 2 and one_launch and h.bs * h.ndir * 2 <= h.ncu else 1
    if not over:
        bwd = NB_MFMA if mfma else NB_LINE
    elif mfma:
        bwd = NB_MFMA_DW if h.bwd_mfma_fused and terms == 3 and (h.bwd_mfma_fused >= 2 or h.bs < 900) else NB_MFMA_THEN_DW
    else:
        bwd = NB_BWD_DW if one_launch else NB_LINE_XD_DW if xd else NB_LINE_DW
    moves = (1 << PC_MFMA_BWD if mfma else 0) | (1 << PC_MFMA_BWD_DW if bwd == NB_MFMA_DW else 0)
    moves |= 1 << PC_XD_PRODUCERS if xd == 2 else 1 << PC_XD_PROLOGUE if xd else 0
    p.update(overlapped=int(over), bwd=bwd, terms=terms, dwx=int(dwx), xd=xd, moves=moves)
    return p


def library_plan(lib, h):
    """clstm_debug_narrow_plan (include/clstm_abi.h) for the same shape"""
    ints = (ctypes.c_int * len(SHAPE_FIELDS))(*(int(getattr(h, f)) for f in SHAPE_FIELDS))
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    lib.call("clstm_debug_narrow_plan", ctypes.addressof(ints), ctypes.addressof(out))
    return dict(zip(PLAN_FIELDS, out))


def assert_plan_agrees(lib, h):
    got, want = library_plan(lib, h), plan(h)
    assert got == want, (vars(h), got, want)
    return want


def assert_net_plans_agree(lib, nh, **kw):
    """every narrow layer of the net `nh`, every pass: the library's plan is the restated one"""
    for layer, no in enumerate(nh):
        if narrow(no):
            for pass_ in (FWD_SAVE, FWD_NOSAVE, BWD):
                assert_plan_agrees(lib, shape(pass_, nh, layer=layer, **kw))


# ---- what the parity tests ask -----------------------------------------------------------------------------------------------------
def overlapped(no, overlap, **kw):
    """the backward pass of a layer of `no` cells runs Overlapped (for the small minibatches shape() defaults to: only when forced --
    mode 1 wants tmax >= 64 and 2048 frames)"""
    return narrow(no) and bool(plan(shape(BWD, [no], overlap=overlap, **kw))["overlapped"])


def fused_forward(nh, uni, nc, nlines, overlap, kind, **kw):
    """the forward pass is the fused launch"""
    return len(nh) == 1 and narrow(nh[0]) and plan(shape(FWD_SAVE, nh, uni=uni, nc=nc, nlines=nlines, overlap=overlap, kind=kind, **kw))["fwd"] == NF_FUSED


def xd_form(nh, uni, nc, nlines, overlap, kind, strict=False, **kw):
    """NarrowPlan::xd of the top layer with the default option (2): 0 the separate launch, 1 the whole prologue (counter 26), 2 the producer
    form (counter 27).  The softmax layer's W.d rides the top layer's launch where that runs the split products (not strict f32) for lines x
    directions x 4 <= 3 CUs; form 2 needs the one-launch form -- four or more waves on a real GPU -- and lines x directions x 2 <= CUs."""
    if not narrow(nh[-1]):
        return 0
    return plan(shape(BWD, nh, uni=uni, nc=nc, nlines=nlines, overlap=overlap, kind=kind, strict=strict, **kw))["xd"]
