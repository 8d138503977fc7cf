"""Parity sweep over the hidden sizes, line counts, input widths and precisions of wide layers (lstm_wide.h: every layer of more than
128 cells, BASELINE configs[4]).

Seven persistent and four per-step kernels carry these layers; which one runs is decided on the host (runtime.inc:wide_plan from
net.inc:Net::wide_shape; the weight packs: Net::repack) from the cell count -- the padded contraction lengths wide_kp_fwd / wide_kp_bwd
(multiples of 64) and wide_kp16_fwd / wide_kp16_bwd (multiples of 128), the cell tiles (4 forward, 16 backward, 32 for
lstm_xcd_bwd_bf16_c32), no % 32, no % 128, no % 4, ntile <= 32 -- and from the line count: 16-line blocks, mt = 1 / 2 / 4 and ept =
1 / 2 / 4 at 8 / 16 line-block x direction groups, chunks of 8 / ndir blocks per launch, mts of the per-step forward at 16 / 32 lines.
wide_geometry() restates that rule ONCE in Python; every case asserts the path counters 0, 1, 6, 9, 11 it predicts -- which kernel
ran follows from the rule, never from the result -- and the counters 2, 3, 4, 8, 13, 14 of the products around the recurrence as
product_rule.py predicts them for the same shape (runtime.inc:product_plan), every plan compared with the library's.

f32 modes (default: persistent forward + x3 backward; strict_f32: the f32 MFMA backward; CLSTM_XCD_REC=0: the per-step kernels) are
test_net_parity.run_case at its default bars, weights init x scale_for(no), lr lr_for(no); test_the_inputs_are_adequate proves from
the oracle alone (f32 against f64) that these inputs sit within half of every bar.

Precision 2 (bf16 MFMA operands) has no parity bar; its bar is measured on the reference alone.  The gauge D_q of a case is the largest
difference between the f32 oracle on (params, lines) and the f32 oracle on (bf16(params), bf16(lines)), round to nearest even, per
quantity: softmax outputs and each saved activation absolute, the minibatch gradient relative to its largest entry.  The kernels must
stay within min(4 D_q, cap) of the UNROUNDED f32 oracle, cap = the 3e-2 / 8 % of the forced small-size tests.  The margin of 4: the
gauge rounds two of the operand kinds the kernels round (weights, inputs); the kernels also round h, the gate deltas and the hoisted
products' operands at every step.  A frame whose oracle top-two margin exceeds twice the output bar must decode as the oracle does.

Hidden-size axis: bidirectional, T = [37, 16, 1, 20, 6, 2, 17] (tmax >= 8: the per-step launches replay a captured graph), 48 inputs,
83 classes on the MI355X.  Line-count axis: 144 cells (16-cell bf16 backward kernel, mt) and 160 cells (c32, ept) at 1 .. 257 lines.
Input-width axis: the tiled weight pack (k_pack_wide_tiles) and the input projection inside the forward kernel (lstm_xcd_fwd_bf16_fx).
The host emulator's default 16 CUs never admit a persistent kernel at these widths: in-process it runs the per-step kernels, and one
child process with CLSTM_EMU_CUS=104 the persistent ones up to 192 cells, 65 lines (two launches of the f32 kernels) included.

Each case prints `SWEEP <case> class=(kp_fwd, kp16_fwd, persistent) fwd=<kernel>x<launches> bwd=<kernel>x<launches> moved=<counters>`
and `worst=<largest error / bar>` (f32) or `ratio=<largest kernel error / D_q>` (bf16) with the per-quantity figures.
`python tests/test_wide_layer_sweep.py [pytest output of a GPU run]` prints the table of DESIGN.md 4.6 from wide_geometry()."""
import contextlib
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from common import ATOL, ROOT, RTOL, oracle_minibatch, synth_lines
if ROOT not in sys.path:          # (run as a script for the table: no conftest.py has put the package on the path)
    sys.path.insert(0, ROOT)
import product_rule
import test_net_parity
from test_net_parity import DELTAS, STATES, run_case, _forget_debug_options, _path_count  # noqa: F401  (autouse fixture)
from test_cell_count_sweep import QUANTITIES, T_ORACLE, both, cus, ids, only_gpu, recording

PC_FWD_PERSISTENT, PC_BWD_PERSISTENT, PC_FWD_FUSED_WX, PC_BWD_C32, PC_BWD_X3 = 0, 1, 6, 9, 11
COUNTERS = (PC_FWD_PERSISTENT, PC_BWD_PERSISTENT, PC_FWD_FUSED_WX, PC_BWD_C32, PC_BWD_X3) + product_rule.PRODUCT_COUNTERS
SIZES = [129, 130, 143, 144, 145, 148, 159, 160, 161, 191, 192, 193, 255, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512, 513, 528, 576]
LINE_COUNTS = [1, 16, 17, 32, 33, 64, 65, 128, 129, 257]
EMU_CHILD_CUS = 104               # 8 x 13 cell tiles: the persistent kernels up to 208 cells


def scale_for(no):
    """weights = the oracle's seeded init x this: keeps the f32 oracle well inside run_case's bars (test_the_inputs_are_adequate)"""
    return 12.0 if no <= 160 else 8.0 if no <= 256 else 5.0 if no <= 320 else 3.0


def lr_for(no):
    return 1e-3 if no <= 160 else 1e-4


def line_lengths(nlines):
    return [9] + [1 + (7 * i) % 6 for i in range(1, nlines)]


# ---- 1. the rule, restated once ---------------------------------------------------------------------------------------------------
WIDE_NW, WIDE_WPAD, WIDE_LDW = 4, 4, 20                                           # lstm_wide.h


def kp_fwd(no):
    return (no + 63) // 64 * 64                                                   # lstm_wide.h:wide_kp_fwd, 16 k x WIDE_NW waves


def kp_bwd(no):
    return (4 * no + 63) // 64 * 64                                               # wide_kp_bwd


def kp16_fwd(no):
    return (no + 127) // 128 * 128                                                # wide_kp16_fwd, 32 k x WIDE_NW waves


def kp16_bwd(no):
    return (4 * no + 127) // 128 * 128                                            # wide_kp16_bwd


def tiled_pack(no, ni, precision):
    """net.inc:Net::repack: every bf16 copy of the layer by k_pack_wide_tiles (pack_tiles = 1) instead of k_pack_wide_bf16 + k_pack_layer
    + k_to_bf16 + k_transpose_to_bf16"""
    return precision == 2 and no % 128 == 0 and ni % 32 == 0 and kp16_fwd(no) == no and kp16_bwd(no) == 4 * no


def wide_geometry(no, ni, ndir, nlines, tmax, precision, strict, kind, xcd_rec=True, ncu=None):
    """What the C++ derives for the first (wide) layer of a net in one forward + backward: the cell tiles, the padded contraction
    lengths, whether the persistent kernels may run, per pass the kernel and its number of launches, and the path-counter moves.
    ncu: a chip of that many CUs instead of the backend's."""
    assert no > 128 and precision in (0, 2) and not (strict and precision)
    bf16 = precision == 2
    ncu = cus(kind) if ncu is None else ncu
    ntile, nzb16 = (no + 15) // 16, (nlines + 15) // 16                           # runtime.inc:wide_plan
    mt = 1 if not bf16 else 4 if nzb16 * ndir > 16 else 2 if nzb16 * ndir > 8 else 1
    nzb, zb_per = (nlines + 16 * mt - 1) // (16 * mt), max(1, 8 // ndir)
    chunks = (nzb + zb_per - 1) // zb_per
    fits = xcd_rec and tmax > 1 and ntile <= 32 and 8 * ntile <= max(ncu, 16)
    g = {"ntile": ntile, "ntile_fwd": (no + 3) // 4, "kp_fwd": kp_fwd(no), "kp_bwd": kp_bwd(no), "kp16_fwd": kp16_fwd(no), "kp16_bwd": kp16_bwd(no),
         "fits": fits, "mt": mt, "tiled_pack": tiled_pack(no, ni, precision)}
    moves = {}
    # forward (net.inc:Net::forward_pass, fuse_wx = 1: first layer, bf16 GEMMs + recurrence, up to 128 inputs in whole 32-k groups)
    fx_asked = bf16 and ni <= 128 and ni % 32 == 0
    if fx_asked and fits and mt == 1 and kp16_fwd(no) <= 512 and no % 4 == 0:
        g["fwd"], g["fwd_launches"] = "xcd_fwd_bf16_fx<1>", chunks
        moves[PC_FWD_PERSISTENT] = moves[PC_FWD_FUSED_WX] = 1
    elif fits and not bf16 and (64 * (kp_fwd(no) + WIDE_WPAD) + WIDE_NW * 16 * 68 + 16) * 4 <= 160 * 1024:      # xcd_fwd_f32_lds_bytes
        g["fwd"], g["fwd_launches"] = "xcd_fwd_f32", chunks
        moves[PC_FWD_PERSISTENT] = 1
    elif fits and bf16 and kp16_fwd(no) <= 512:
        g["fwd"], g["fwd_launches"] = "xcd_fwd_bf16<%d>" % mt, chunks
        moves[PC_FWD_PERSISTENT] = 1
    else:
        mts = 4 if nlines > 32 else 2 if nlines > 16 else 1
        g["fwd"], g["fwd_launches"] = "fwd_step16_bf16" if bf16 else "fwd_step<%d>" % mts, tmax
    # backward (net.inc:Net::rec_x3: f32 mode, not strict)
    if fits and not bf16 and not strict and kp16_bwd(no) <= 2048:
        g["bwd"], g["bwd_launches"] = "xcd_bwd_x3", chunks
        moves[PC_BWD_PERSISTENT] = moves[PC_BWD_X3] = 1
    elif fits and not bf16 and max((16 * (kp_bwd(no) + WIDE_WPAD) + WIDE_NW * 16 * WIDE_LDW + 16) * 4, 84 * 1024) <= 160 * 1024:   # xcd_bwd_f32_lds_bytes
        g["bwd"], g["bwd_launches"] = "xcd_bwd_f32", chunks
        moves[PC_BWD_PERSISTENT] = 1
    elif fits and bf16 and kp16_bwd(no) <= 2048 and no % 32 == 0 and ndir <= 2:   # bwd_c32 = 1
        per = 16 // ndir
        ept = 1 if nlines <= 8 * per else 2 if nlines <= 16 * per else 4
        ng = (nlines + 8 * ept - 1) // (8 * ept)
        g["bwd"], g["bwd_launches"] = "xcd_bwd_bf16_c32<%d>" % ept, (ng + per - 1) // per
        moves[PC_BWD_PERSISTENT] = moves[PC_BWD_C32] = 1
    elif fits and bf16 and kp16_bwd(no) <= 2048:
        g["bwd"], g["bwd_launches"] = "xcd_bwd_bf16<%d>" % mt, chunks
        moves[PC_BWD_PERSISTENT] = 1
    else:
        g["bwd"], g["bwd_launches"] = "bwd_step16_bf16" if bf16 else "bwd_step", tmax
    g["moves"] = moves
    return g


# clstm_debug_wide_plan (include/clstm_abi.h): what the library's own rule (runtime.inc:wide_plan) answers for the same shape.  The shape is
# laid out here as net.inc:Net::wide_shape fills it for the first layer of a net in its default options.
PLAN_KERNELS = {1: "xcd_fwd_f32", 2: "xcd_fwd_bf16<%d>", 3: "xcd_fwd_bf16_fx<%d>", 4: "xcd_bwd_x3", 5: "xcd_bwd_f32", 6: "xcd_bwd_bf16_c32<%d>",
                7: "xcd_bwd_bf16<%d>", 8: "fwd_step<%d>", 9: "fwd_step16_bf16", 10: "bwd_step", 11: "bwd_step16_bf16"}


def library_plan(lib, no, ni, ndir, nlines, tmax, precision, strict, ncu, xcd_rec=True, frames=None):
    """{fwd, fwd_launches, bwd, bwd_launches, moves} as wide_geometry names them, from the library's plans of the two passes"""
    bf16, out, moves = precision == 2, {}, 0
    sbf = bf16 and ni % 8 == 0 and no % 8 == 0 and kp16_bwd(no) == 4 * no                     # runtime.inc:product_plan, PW_SBF
    for fwd in (1, 0):
        shape = (ctypes.c_int * 20)(fwd, no, ni, ndir, nlines, tmax, nlines * tmax if frames is None else frames,
                                    kp_fwd(no) if fwd else kp_bwd(no), kp16_fwd(no) if fwd else kp16_bwd(no), bf16,
                                    not fwd and not bf16 and not strict,                       # x3: net.inc:Net::rec_x3, R2b packed with it
                                    1 if fwd and bf16 else 0,                                  # fuse_wx = 1: a first layer in precision 2 has the operands
                                    ncu, xcd_rec, 0, 1, fwd and sbf, ni + no + 8, (1 + ni + no + 15) // 16 * 16, (4 + ndir * no + 15) // 16 * 16)
        plan = (ctypes.c_int * 14)()
        lib.call("clstm_debug_wide_plan", ctypes.addressof(shape), ctypes.addressof(plan))
        kernel, param, launches, step_kernel, step_param = plan[0], plan[1], plan[5], plan[7], plan[8]
        name = PLAN_KERNELS[kernel or step_kernel]
        side = "fwd" if fwd else "bwd"
        out[side] = name % (param if kernel else step_param) if "%" in name else name
        out[side + "_launches"] = launches
        assert launches == ((plan[3] + plan[4] - 1) // plan[4] if kernel else tmax), list(plan)
        if kernel:
            moves |= plan[12]
    out["moves"] = {c: 1 for c in range(31) if moves >> c & 1}
    return out


def assert_plan_agrees(lib, geo, *shape, **kw):
    got = library_plan(lib, *shape, **kw)
    assert got == {k: geo[k] for k in got}, (shape, kw, got, {k: geo[k] for k in got})


def klass(no):
    """(kp_fwd, kp16_fwd, persistent-eligible on a 256-CU chip)"""
    return kp_fwd(no), kp16_fwd(no), (no + 15) // 16 <= 32


def classes():
    """{class: [cell counts]} for 129..576 cells"""
    out = {}
    for no in range(129, 577):
        out.setdefault(klass(no), []).append(no)
    return out


def test_the_sweep_covers_every_class_at_both_ends():
    """for every (kp_fwd, kp16_fwd, persistent-eligible) class the rule yields for 129..576 cells: its lowest and its highest cell
    count are swept, and the list holds the residues the kernels branch on -- a later change to the tables makes the gap visible here"""
    assert list(classes()) == [(192, 256, True), (256, 256, True), (320, 384, True), (384, 384, True), (448, 512, True), (512, 512, True), (576, 640, False)]
    for k, members in classes().items():
        swept = [no for no in SIZES if klass(no) == k]
        assert members[0] in swept and members[-1] in swept, (k, members[0], members[-1], swept)
    assert any(no % 4 for no in SIZES) and any(no % 16 and not no % 4 for no in SIZES)
    assert any(no % 32 == 0 and no % 128 for no in SIZES) and any(no % 128 == 0 for no in SIZES) and any(no % 32 == 16 for no in SIZES)
    # both sides of every 16-cell backward tile edge (kp_bwd) and 32-cell c32 edge (kp16_bwd == 4 no) in 143..161, of ntile <= 32 at 512 / 513
    assert {143, 144, 145, 159, 160, 161, 512, 513} <= set(SIZES)
    geo = lambda no, precision=0, strict=False, **kw: wide_geometry(no, 48, 2, 7, 37, precision, strict, "hip", **kw)
    for no in SIZES:
        want = "xcd_fwd_f32 xcd_bwd_x3" if no <= 512 else "fwd_step<1> bwd_step"
        assert "%(fwd)s %(bwd)s" % geo(no) == want, no
        assert geo(no, strict=True)["bwd"] == ("xcd_bwd_f32" if no <= 512 else "bwd_step"), no
        assert "%(fwd)s %(bwd)s" % geo(no, xcd_rec=False) == "fwd_step<1> bwd_step" and not geo(no, xcd_rec=False)["moves"], no
        want = "fwd_step16_bf16 bwd_step16_bf16" if no > 512 else "xcd_fwd_bf16<1> " + ("xcd_bwd_bf16_c32<1>" if no % 32 == 0 else "xcd_bwd_bf16<1>")
        assert "%(fwd)s %(bwd)s" % geo(no, 2) == want, no
    # the line-count edges: 64 | 65 and 128 | 129 lines of two directions
    for no, kernel in ((144, "xcd_bwd_bf16<%d>"), (160, "xcd_bwd_bf16_c32<%d>")):
        got = [wide_geometry(no, 48, 2, n, 9, 2, False, "hip") for n in LINE_COUNTS]
        assert [g["bwd"] for g in got] == [kernel % m for m in (1, 1, 1, 1, 1, 1, 2, 2, 4, 4)]
        assert [g["fwd"] for g in got] == ["xcd_fwd_bf16<%d>" % m for m in (1, 1, 1, 1, 1, 1, 2, 2, 4, 4)]
        assert [g["fwd_launches"] for g in got] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2]
    assert [wide_geometry(144, 48, 2, n, 9, 0, False, "hip")["fwd_launches"] for n in LINE_COUNTS] == [1, 1, 1, 1, 1, 1, 2, 2, 3, 5]
    assert [wide_geometry(144, 48, 2, n, 9, 0, False, "hip", xcd_rec=False)["fwd"][-2] for n in (16, 17, 32, 33)] == ["1", "2", "2", "4"]
    # one direction: 16 groups per launch; one-frame lines never take a persistent kernel; the emulator's 16 CUs admit none at these widths
    assert wide_geometry(160, 48, 1, 7, 37, 2, False, "hip")["bwd"] == "xcd_bwd_bf16_c32<1>" and wide_geometry(257, 48, 1, 7, 37, 0, False, "hip")["moves"] == {0: 1, 1: 1, 11: 1}
    assert not wide_geometry(160, 48, 2, 3, 1, 0, False, "hip")["moves"]
    if "CLSTM_EMU_CUS" not in os.environ:
        assert not any(wide_geometry(no, 6, 2, 4, 37, p, False, "emu")["moves"] for no in SIZES for p in (0, 2))
    # the input-width axis (section 4): tiled pack and the fused input projection
    assert [tiled_pack(256, ni, 2) for ni in (48, 64, 160)] == [False, True, True] and not any(tiled_pack(160, ni, 2) for ni in (48, 64, 160))
    assert [wide_geometry(no, ni, 2, 7, 37, 2, False, "hip")["moves"].get(6, 0) for no in (256, 160) for ni in (48, 64, 160)] == [0, 1, 0, 0, 1, 0]


# ---- the shared reference -----------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


class Updated:
    """stands where run_case expects the oracle's net: the one update of the shared result was applied when it was made"""

    def __init__(self, net):
        net.update()
        self._params, self._derivs = net.get_params(), net.get_derivs()

    def update(self):
        pass

    def get_params(self):
        return self._params

    def get_derivs(self):
        return self._derivs


_INPUTS, _RESULTS = {}, {}


def case_inputs(ora32, ni, no, nc, T, uni, scale):
    """(params, lines, transcripts) as run_case makes them from its default seeds"""
    key = (ni, no, nc, tuple(T), uni, scale)
    if key not in _INPUTS:
        rng = np.random.default_rng(1)
        params = test_net_parity.OracleNet(ora32, ni, no, nc, unidirectional=uni, seed=0.222).get_params() * scale
        lines = synth_lines(rng, T, ni)
        trs = [rng.integers(1, nc, max(1, t // 3)).astype(np.int32) for t in T]
        _INPUTS[key] = (params, lines, trs)
    return _INPUTS[key]


def reference(ora, ora32, ni, no, nc, T, uni, scale, lr, rounded=False, dx=False):
    """one minibatch on the oracle `ora`, computed once per process and shared by every mode that compares with it, read-only;
    rounded: on bf16(params), bf16(lines) -- the gauge's second run"""
    key = (ora.prec, ni, no, nc, tuple(T), uni, scale, lr, rounded, dx)
    if key not in _RESULTS:
        params, lines, trs = case_inputs(ora32, ni, no, nc, T, uni, scale)
        if rounded:
            params, lines = bf16_round(params), [bf16_round(x) for x in lines]
        skeys = [(0, d, w) for d in ((0,) if uni else (0, 1)) for w in STATES + DELTAS]
        want = oracle_minibatch(ora, test_net_parity.OracleNet, params, ni, no, nc, lines, trs, unidirectional=uni, states=skeys, lr=lr, mom=0.9)
        if dx:      # the first layer's input deltas, line by line
            net = test_net_parity.OracleNet(ora, ni, no, nc, unidirectional=uni, init=False)
            net.set_params(params)
            want["dx"] = []
            for x, tr in zip(lines, trs):
                net.set_inputs(x); net.forward(); net.ctc_deltas(tr); net.backward()
                want["dx"].append(net.input_deltas()[:, 0, :].copy())
        want["net"] = Updated(want["net"])
        want["params_after"], want["derivs_after"] = want["net"].get_params(), want["net"].get_derivs()
        for a in [want["derivs"], want["params_after"], want["derivs_after"]] + want["outputs"] + want["aligned"] + [s for v in want["states"].values() for s in v]:
            a.setflags(write=False)
        _RESULTS[key] = want
    return _RESULTS[key]


@contextlib.contextmanager
def oracle_from(want, params):
    """run_case takes the shared result instead of running the oracle again"""
    real = test_net_parity.oracle_minibatch

    def shared(ora, OracleNet, p, *a, **k):
        assert np.array_equal(p, params)
        return dict(want)
    test_net_parity.oracle_minibatch = shared
    try:
        yield
    finally:
        test_net_parity.oracle_minibatch = real


@contextlib.contextmanager
def xcd_rec_env(on):
    """CLSTM_XCD_REC is read per pass (net.inc:Net::wide_shape)"""
    old = os.environ.get("CLSTM_XCD_REC")
    os.environ["CLSTM_XCD_REC"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CLSTM_XCD_REC"]
        else:
            os.environ["CLSTM_XCD_REC"] = old


def frac(a, b, rtol=RTOL, atol=ATOL, scale_atol=0.0):
    """max |a - b| / bar, the bar as common.assert_close has it"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    if not b.size:
        return 0.0
    bar = atol + scale_atol * float(np.abs(b).max()) + rtol * np.abs(b)
    return float(np.nan_to_num(np.abs(a - b) / bar, nan=np.inf).max())


def fractions(got, want, lr, grad_tol=1e-4):
    """{quantity: largest error / bar} of one oracle result against another, at the bars run_case sets for a backend"""
    n = len(want["outputs"])
    out = {"softmax outputs": max(frac(got["outputs"][b], want["outputs"][b]) for b in range(n)),
           "state": max(frac(got["states"][k][b], want["states"][k][b]) for k in want["states"] if k[2] in STATES for b in range(n)),
           "aligned": max(frac(got["aligned"][b], want["aligned"][b], 1e-4, 1e-6) for b in range(n)),
           "delta": max(frac(got["states"][k][b], want["states"][k][b], grad_tol, 1e-9, grad_tol) for k in want["states"] if k[2] in DELTAS for b in range(n)),
           "minibatch gradient": frac(got["derivs"], want["derivs"], grad_tol, 1e-9, grad_tol),
           "params after update": frac(got["params_after"], want["params_after"], 1e-5, 1e-7 + lr * grad_tol * float(np.abs(want["derivs"]).max())),
           "momentum buffer": frac(got["derivs_after"], want["derivs_after"], grad_tol, 1e-9, grad_tol)}
    if "dx" in want:
        out["input deltas"] = max(frac(got["dx"][b], want["dx"][b], grad_tol, 1e-9, grad_tol) for b in range(n))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
MODES = {"f32": dict(precision=0), "strict": dict(precision=0, strict=True), "steps": dict(precision=0, rec=False),
         "bf16": dict(precision=2), "bf16_steps": dict(precision=2, rec=False)}
CAP_ACT, CAP_GRAD, MARGIN = 3e-2, 8e-2, 4.0           # the forced small-size bf16 tests' bars stay as the cap


def shape(backend, no, ni=None, T=None, scale=None, lr=None):
    emu = backend.kind == "emu"
    return ((6 if emu else 48) if ni is None else ni, 9 if emu else 83, (T_ORACLE[:4] if emu else T_ORACLE) if T is None else T,
            scale_for(no) if scale is None else scale, lr_for(no) if lr is None else lr)


def counters(backend):
    return {c: _path_count(backend, c) for c in COUNTERS}


def moved_since(backend, before):
    return {c: _path_count(backend, c) - before[c] for c in COUNTERS if _path_count(backend, c) != before[c]}


def product_moves(backend, geo, no, ni, uni, T, precision, strict, check_dx=False):
    """what the products of one forward + backward of the one-layer net move (product_rule.step_moves), given the recurrence kernels the
    wide rule names; with every plan the library's own"""
    return product_rule.step_moves(backend.lib, [no], ni, len(T), sum(T), precision, ["xcd" in geo["fwd"]], ["xcd" in geo["bwd"]],
                                   fx=(0,) if geo["moves"].get(PC_FWD_FUSED_WX) else (), uni=uni, nc=shape(backend, no)[1], strict=strict,
                                   ncu=cus(backend.kind), want_dx0=check_dx)


def head(name, no, geo, moved):
    return "SWEEP %s class=%r fwd=%sx%d bwd=%sx%d moved=%r" % (name, klass(no), geo["fwd"], geo["fwd_launches"], geo["bwd"], geo["bwd_launches"], moved)


def f32_case(backend, ora32, name, no, mode, uni=False, check_dx=False, **shape_kw):
    """run_case at its default bars against the shared oracle result; the counters must move as the rule says"""
    m = MODES[mode]
    ni, nc, T, scale, lr = shape(backend, no, **shape_kw)
    geo = wide_geometry(no, ni, 1 if uni else 2, len(T), max(T), 0, m.get("strict", False), backend.kind, m.get("rec", True))
    assert_plan_agrees(backend.lib, geo, no, ni, 1 if uni else 2, len(T), max(T), 0, m.get("strict", False), cus(backend.kind), m.get("rec", True), frames=sum(T))
    params, lines, trs = case_inputs(ora32, ni, no, nc, T, uni, scale)
    want = reference(ora32, ora32, ni, no, nc, T, uni, scale, lr, dx=check_dx)
    before, moved = counters(backend), None
    with recording() as worst, oracle_from(want, params), xcd_rec_env(m.get("rec", True)):
        try:
            net, _ = run_case(backend, ora32, ni, no, nc, T, uni=uni, scale=scale, lr=lr, check_dx=check_dx, strict_f32=m.get("strict", False),
                              params=params, lines=lines, trs=trs)
            if check_dx:
                dx = net.split(net.input_deltas())
                worst["input deltas"] = max(frac(dx[b], want["dx"][b], 1e-4, 1e-9, 1e-4) for b in range(len(T)))
        finally:
            moved = moved_since(backend, before)
            print("%s worst=%.3f %s" % (head(name, no, geo, moved), max(worst.values()) if worst else 0.0,
                                        " ".join("%s=%.3f" % (q.replace(" ", "_"), f) for q, f in worst.items())))
    assert moved == {**geo["moves"], **product_moves(backend, geo, no, ni, uni, T, 0, m.get("strict", False), check_dx)}, (moved, geo["moves"])
    assert set(worst) == set(QUANTITIES) | ({"input deltas"} if check_dx else set())
    assert worst.get("input deltas", 0.0) <= 1.0, worst


def gauge(ora32, ni, no, nc, T, uni, scale, lr):
    """(want, D_q): the f32 oracle's result and, per quantity, its largest distance from the f32 oracle on bf16-rounded weights and
    inputs -- outputs and every saved activation absolute, the gradient relative to its largest entry"""
    want = reference(ora32, ora32, ni, no, nc, T, uni, scale, lr)
    q = reference(ora32, ora32, ni, no, nc, T, uni, scale, lr, rounded=True)
    n = len(T)
    dq = {"outputs": max(float(np.abs(q["outputs"][b] - want["outputs"][b]).max()) for b in range(n)),
          "gradient": float(np.abs(q["derivs"] - want["derivs"]).max() / np.abs(want["derivs"]).max())}
    for k in want["states"]:
        if k[2] in STATES:
            dq[k] = max(float(np.abs(q["states"][k][b] - want["states"][k][b]).max()) for b in range(n))
    return want, dq


def bf16_case(backend, ora32, name, no, mode, uni=False, **shape_kw):
    """precision 2 against the unrounded f32 oracle within min(4 D_q, cap) per quantity; the counters must move as the rule says"""
    from clstm_amd.net import Network
    m = MODES[mode]
    ni, nc, T, scale, lr = shape(backend, no, **shape_kw)
    geo = wide_geometry(no, ni, 1 if uni else 2, len(T), max(T), 2, False, backend.kind, m.get("rec", True))
    assert_plan_agrees(backend.lib, geo, no, ni, 1 if uni else 2, len(T), max(T), 2, False, cus(backend.kind), m.get("rec", True), frames=sum(T))
    params, lines, trs = case_inputs(ora32, ni, no, nc, T, uni, scale)
    want, dq = gauge(ora32, ni, no, nc, T, uni, scale, lr)
    assert all(v > 0 for v in dq.values()), dq
    bar = {k: min(MARGIN * v, CAP_GRAD if k == "gradient" else CAP_ACT) for k, v in dq.items()}
    before, moved, err = counters(backend), None, {}
    with xcd_rec_env(m.get("rec", True)):
        try:
            net = Network(ni, no, nc, unidirectional=uni, lib=backend.lib)
            net.set_params(params)
            net.setLearningRate(lr, 0.9)
            net.set_gemm_precision(2)
            net.set_inputs(lines)
            net.forward()
            got = net.split(net.outputs())
            err["outputs"] = max(float(np.abs(got[b] - want["outputs"][b]).max()) for b in range(len(T)))
            for k in want["states"]:
                if k[2] in STATES:
                    s = net.split(net.state(*k))
                    err[k] = max(float(np.abs(s[b] - want["states"][k][b]).max()) for b in range(len(T)))
            judged = wrong = 0
            for b in range(len(T)):
                top2 = np.sort(want["outputs"][b].astype(np.float64), axis=1)[:, -2:]
                clear = top2[:, 1] - top2[:, 0] > 2 * bar["outputs"]
                judged += int(clear.sum())
                wrong += int((got[b].argmax(1) != want["outputs"][b].argmax(1))[clear].sum())
            net.ctc(trs)
            net.backward()
            g = net.get_grads()
            err["gradient"] = float(np.abs(g - want["derivs"]).max() / np.abs(want["derivs"]).max())
        finally:
            moved = moved_since(backend, before)
            ratio = {k: err[k] / dq[k] for k in err}
            states = [k for k in ratio if isinstance(k, tuple)]
            print("%s ratio=%.3f outputs=%.3f states=%.3f gradient=%.3f D_q=%.1e/%.1e/%.1e error=%.1e/%.1e/%.1e" % (
                head(name, no, geo, moved), max(ratio.values(), default=0.0), ratio.get("outputs", 0.0), max((ratio[k] for k in states), default=0.0),
                ratio.get("gradient", 0.0), dq["outputs"], max(dq[k] for k in dq if isinstance(k, tuple)), dq["gradient"],
                err.get("outputs", 0.0), max((err[k] for k in states), default=0.0), err.get("gradient", 0.0)))
    assert moved == {**geo["moves"], **product_moves(backend, geo, no, ni, uni, T, 2, False)}, (moved, geo["moves"])
    assert set(err) == set(dq) and np.isfinite(list(err.values())).all()
    over = {k: (err[k], bar[k]) for k in err if not err[k] <= bar[k]}
    assert not over, "kernel error beyond min(4 D_q, cap) (error, bar): %r" % over
    assert judged > 0 and wrong == 0, "%d of %d frames with a clear oracle margin decode differently" % (wrong, judged)
    assert not np.array_equal(g, want["derivs"])          # the switch really changed the arithmetic


def sweep_case(backend, ora32, name, no, mode, **kw):
    (bf16_case if MODES[mode]["precision"] == 2 else f32_case)(backend, ora32, "%s %s" % (name, mode), no, mode, **kw)


# ---- 2. the hidden-size axis ----------------------------------------------------------------------------------------------------------
EMU_F32, EMU_BF16 = [129, 145, 160, 193, 257, 513], [145, 160]


@pytest.mark.parametrize("backend,no", both(SIZES, EMU_F32), indirect=["backend"], ids=ids)
def test_default_f32(backend, ora32, no):
    """persistent f32 forward, x3 backward up to 512 cells; beyond, and on the emulator's 16 CUs, the per-step kernels"""
    sweep_case(backend, ora32, "bidi %d" % no, no, "f32")


@pytest.mark.parametrize("backend,no", only_gpu(SIZES), indirect=["backend"], ids=ids)
def test_strict_f32(backend, ora32, no):
    """clstm_net_set_strict_f32: the backward recurrence on the f32 MFMA (lstm_xcd_bwd_f32), weights resident up to kp_bwd = 2048"""
    sweep_case(backend, ora32, "bidi %d" % no, no, "strict")


@pytest.mark.parametrize("backend,no", only_gpu(SIZES), indirect=["backend"], ids=ids)
def test_per_step_f32(backend, ora32, no):
    """CLSTM_XCD_REC=0: lstm_wide_fwd_step<1> / lstm_wide_bwd_step as a replayed graph of 37 launches each; no persistent counter moves"""
    sweep_case(backend, ora32, "bidi %d" % no, no, "steps")


@pytest.mark.parametrize("backend,no", both(SIZES, EMU_BF16), indirect=["backend"], ids=ids)
def test_bf16(backend, ora32, no):
    """precision 2: lstm_xcd_fwd_bf16<1>, the c32 backward kernel where no % 32 == 0 and the 16-cell one elsewhere; above 512 cells
    (and on the emulator) *_step16_bf16"""
    sweep_case(backend, ora32, "bidi %d" % no, no, "bf16")


@pytest.mark.parametrize("backend,no", only_gpu(SIZES), indirect=["backend"], ids=ids)
def test_per_step_bf16(backend, ora32, no):
    """precision 2 with CLSTM_XCD_REC=0: lstm_wide_fwd_step16_bf16 / lstm_wide_bwd_step16_bf16 at every width"""
    sweep_case(backend, ora32, "bidi %d" % no, no, "bf16_steps")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("backend,no", only_gpu([160, 257]), indirect=["backend"], ids=ids)
def test_unidirectional(backend, ora32, no, mode):
    """one direction: 16 groups of one direction per launch, per = 16 line groups for c32"""
    sweep_case(backend, ora32, "uni %d" % no, no, mode, uni=True)


# ---- 3. the line-count axis -----------------------------------------------------------------------------------------------------------
LINES_SCALE, LINES_LR = 8.0, 1e-3      # as test_lockstep_persistent_chunks: with many lines of gradient sums the update check's floor is below lr x the gradient's bar


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("nlines", LINE_COUNTS)
@pytest.mark.parametrize("backend,no", only_gpu([144, 160]), indirect=["backend"], ids=ids)
def test_line_counts(backend, ora32, no, nlines, mode):
    """16-line blocks whole and plus one; mt / ept = 1 | 2 at 64 | 65 lines and 2 | 4 at 128 | 129; 257 lines walk two (bf16) and five
    (f32) chunks; ragged lines of 1..6 frames drop out of lock-step in every block"""
    sweep_case(backend, ora32, "lines %d x %d" % (no, nlines), no, mode, T=line_lengths(nlines), scale=LINES_SCALE, lr=LINES_LR)


@pytest.mark.parametrize("nlines", [16, 17, 32, 33])
@pytest.mark.parametrize("backend,no", only_gpu([144, 160]), indirect=["backend"], ids=ids)
def test_line_counts_per_step(backend, ora32, no, nlines):
    """lstm_wide_fwd_step<mts>: mts = 1 | 2 at 16 | 17 lines, 2 | 4 at 32 | 33"""
    sweep_case(backend, ora32, "lines %d x %d" % (no, nlines), no, "steps", T=line_lengths(nlines), scale=LINES_SCALE, lr=LINES_LR)


@pytest.mark.parametrize("backend", [pytest.param("hip", marks=pytest.mark.gpu)], indirect=True)
def test_one_frame_lines_take_the_per_step_kernels(backend, ora32):
    """tmax == 1: nothing to keep resident for -- by rule the per-step kernels, and the persistent counters stay put"""
    assert not wide_geometry(160, 48, 2, 3, 1, 0, False, backend.kind)["moves"]
    sweep_case(backend, ora32, "one-frame lines 160", 160, "f32", T=[1, 1, 1], scale=LINES_SCALE, lr=LINES_LR)


@pytest.mark.parametrize("backend", [pytest.param("hip", marks=pytest.mark.gpu)], indirect=True)
def test_input_deltas_of_a_wide_first_layer(backend, ora32):
    """96 inputs, 192 cells, enable_input_deltas: dX of layer 0 from the wide backward pass's deltas, against the oracle's"""
    sweep_case(backend, ora32, "dx 192", 192, "f32", ni=96, check_dx=True)


# ---- 4. the input-width axis of the bf16 forward ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ni", [48, 64, 160])
@pytest.mark.parametrize("backend,no", only_gpu([256, 160]), indirect=["backend"], ids=ids)
def test_bf16_input_widths(backend, ora32, no, ni):
    """256 cells: k_pack_wide_tiles from 64 inputs on (ni % 32 == 0); 160 cells: never.  lstm_xcd_fwd_bf16_fx<1> (counter 6) at 64
    inputs only: 48 is no whole 32-k group, 160 is beyond fuse_wx = 1's 128 inputs -- the hoisted bf16 product runs there"""
    assert wide_geometry(no, ni, 2, len(T_ORACLE), max(T_ORACLE), 2, False, backend.kind)["moves"].get(PC_FWD_FUSED_WX, 0) == (ni == 64)
    assert tiled_pack(no, ni, 2) == (no == 256 and ni != 48)
    sweep_case(backend, ora32, "ni %d -> %d" % (ni, no), no, "bf16", ni=ni)


# ---- 5. the inputs prove themselves adequate (oracle only) ------------------------------------------------------------------------------
def f32_inputs():
    """every (ni, no, nc, T, uni, scale, lr, dx) an f32 mode of this file compares at"""
    out = []
    for ni, nc, T, sizes in ((48, 83, T_ORACLE, SIZES), (6, 9, T_ORACLE[:4], sorted(set(EMU_F32 + [145, 160, 192])))):
        out += [(ni, no, nc, T, False, scale_for(no), lr_for(no), False) for no in sizes]
    out += [(48, no, 83, T_ORACLE, True, scale_for(no), lr_for(no), False) for no in (160, 257)]
    out += [(6, 145, 9, CHILD_LINES["T"], False, LINES_SCALE, LINES_LR, False)]
    out += [(48, no, 83, line_lengths(n), False, LINES_SCALE, LINES_LR, False) for no in (144, 160) for n in LINE_COUNTS]
    out += [(48, 160, 83, [1, 1, 1], False, LINES_SCALE, LINES_LR, False), (96, 192, 83, T_ORACLE, False, scale_for(192), lr_for(192), True)]
    return out


def test_the_inputs_are_adequate(ora32, ora64):
    """at every swept (size, scale) the f32 oracle lies within HALF of each of run_case's bars of the f64 oracle, decodes equal: a
    kernel that misses a bar is wrong, not unlucky with an ill-conditioned net"""
    worst = {}
    for ni, no, nc, T, uni, scale, lr, dx in f32_inputs():
        a = reference(ora32, ora32, ni, no, nc, T, uni, scale, lr, dx=dx)
        b = reference(ora64, ora32, ni, no, nc, T, uni, scale, lr, dx=dx)
        assert [d.tolist() for d in a["decode"]] == [d.tolist() for d in b["decode"]], (ni, no, len(T))
        f = fractions(a, b, lr)
        print("ADEQUATE ni=%d no=%d lines=%d uni=%d scale=%g worst=%.3f %s" % (ni, no, len(T), uni, scale, max(f.values()), " ".join("%s=%.3f" % (q.replace(" ", "_"), v) for q, v in f.items())))
        worst[(ni, no, len(T), uni)] = max(f.values())
    over = {k: v for k, v in worst.items() if not v <= 0.5}
    assert not over, over


# ---- 6. the persistent kernels on a larger emulated chip ----------------------------------------------------------------------------------
CHILD_CASES = [(no, mode, {}) for no in (145, 160, 192) for mode in ("f32", "strict", "bf16")]
CHILD_LINES = dict(T=line_lengths(65), scale=LINES_SCALE, lr=LINES_LR)      # five line blocks x two directions: two launches of the f32 kernels, mt = 2 in bf16
CHILD_CASES += [(145, "f32", CHILD_LINES), (145, "bf16", CHILD_LINES)]


def child_main():
    """in a fresh process whose emulator was given EMU_CHILD_CUS CUs: every CHILD_CASES case, counters asserted"""
    from common import Backend
    from oracle.oracle import Oracle
    backend, ora32 = Backend("emu"), Oracle("f32")
    assert cus("emu") == EMU_CHILD_CUS
    for no, mode, kw in CHILD_CASES:
        want = {"f32": {0: 1, 1: 1, 11: 1}, "strict": {0: 1, 1: 1}, "bf16": {0: 1, 1: 1, 9: 1} if no % 32 == 0 else {0: 1, 1: 1}}[mode]
        geo = wide_geometry(no, 6, 2, len(kw.get("T", T_ORACLE[:4])), 37, MODES[mode]["precision"], mode == "strict", "emu")
        assert geo["moves"] == want, (no, mode)
        if kw:
            assert (geo["fwd"], geo["fwd_launches"]) == (("xcd_fwd_f32", 2) if mode == "f32" else ("xcd_fwd_bf16<2>", 1)), geo
        sweep_case(backend, ora32, "emu%d bidi %d x %d" % (EMU_CHILD_CUS, no, len(kw.get("T", T_ORACLE[:4]))), no, mode, **kw)
    print("CHILD PASSED %d" % len(CHILD_CASES))


def test_persistent_kernels_on_a_larger_emulated_chip():
    """The emulator's default 16 CUs admit no persistent kernel above 32 cells.  A child process with CLSTM_EMU_CUS=104 (the count is
    read once per process) runs lstm_xcd_fwd_f32 + lstm_xcd_bwd_x3, lstm_xcd_bwd_f32, lstm_xcd_fwd_bf16<1> + lstm_xcd_bwd_bf16<1> (145
    cells) / lstm_xcd_bwd_bf16_c32<1> (160, 192) with every workgroup of a launch live at once."""
    code = textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        import test_wide_layer_sweep
        test_wide_layer_sweep.child_main()
    """ % (ROOT, ROOT))
    env = dict(os.environ, CLSTM_EMU_CUS=str(EMU_CHILD_CUS))
    env.pop("CLSTM_XCD_REC", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "CHILD PASSED %d" % len(CHILD_CASES) in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- 7. the table of DESIGN.md ------------------------------------------------------------------------------------------------------------
def kernels(no, precision, strict=False, xcd_rec=True):
    g = wide_geometry(no, 48, 2, len(T_ORACLE), max(T_ORACLE), precision, strict, "hip", xcd_rec)
    return g["fwd"], g["bwd"]


def table(log=None):
    worst, ratio = {}, {}
    if log:
        text = open(log).read()
        for m in re.finditer(r"^\W*SWEEP .* class=\((\d+), (\d+), (True|False)\) .* (worst|ratio)=([0-9.]+|inf|nan)", text, re.M):
            k = (int(m.group(1)), int(m.group(2)), m.group(3) == "True")
            d = worst if m.group(4) == "worst" else ratio
            d[k] = max(d.get(k, 0.0), float(m.group(5)))
    rows = ["| cells | kp_fwd / kp16_fwd / kp16_bwd | f32 | strict f32 | precision 2 | `CLSTM_XCD_REC=0`, f32 / precision 2 | worst error / bar, f32 modes (MI355X) | worst kernel error / `D_q`, precision 2 (MI355X) |",
            "|---|---|---|---|---|---|---|---|"]
    for k, members in classes().items():
        each = lambda f: " + ".join(" or ".join(dict.fromkeys(f(no)[i] for no in members)) for i in (0, 1))      # (c32 where no % 32 == 0)
        kb = sorted({kp16_bwd(no) for no in members})
        fmt = lambda d: "%.2f" % d[k] if k in d else "-"
        rows.append("| %d..%d | %d / %d / %d..%d | %s | %s | %s | %s / %s | %s | %s |" % (
            members[0], members[-1], k[0], k[1], kb[0], kb[-1], each(lambda no: kernels(no, 0)), each(lambda no: kernels(no, 0, strict=True)),
            each(lambda no: kernels(no, 2)), each(lambda no: kernels(no, 0, xcd_rec=False)), each(lambda no: kernels(no, 2, xcd_rec=False)), fmt(worst), fmt(ratio)))
    return "\n".join(rows)


if __name__ == "__main__":
    print(table(sys.argv[1] if len(sys.argv) > 1 else None))
