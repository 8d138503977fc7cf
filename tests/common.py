"""Shared helpers for the parity tests (oracle <-> HIP path)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "hipemu")

# gate activations / states: 1e-4 relative (BASELINE.json north_star) with an absolute floor for
# values that are themselves ~0.
RTOL = 1e-4
ATOL = 2e-6


def assert_close(a, b, rtol=RTOL, atol=ATOL, what="", scale_atol=0.0):
    """|a-b| <= atol + scale_atol*max|b| + rtol*|b|.  `scale_atol` is for quantities that are sums
    with cancellation (deltas, gradients): float32 summation-order noise is relative to the
    magnitude of the terms (~ the largest entries), not of each small result."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if scale_atol:
        atol = atol + scale_atol * float(np.abs(b).max()) if b.size else atol
    err = np.abs(a - b) - (atol + rtol * np.abs(b))
    if not (err <= 0).all():
        i = np.unravel_index(np.argmax(err), err.shape)
        raise AssertionError("%s mismatch at %s: got %r want %r (max excess %g)" % (what, i, a[i], b[i], err[i]))


def emu_lib():
    """Build (if needed) and load the TEST-ONLY host emulation of the kernels."""
    subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
    from clstm_amd import abi
    return abi.load(os.path.join(EMU_DIR, "build", "libclstm_emu.so"))


def synth_lines(rng, T_list, ni):
    """Normalised-line-like inputs: clip(N(0.2,0.3),0,1), 3-tap smoothed along t."""
    out = []
    for T in T_list:
        x = np.clip(rng.normal(0.2, 0.3, (T + 2, ni)), 0, 1)
        x = (x[:-2] + x[1:-1] + x[2:]) / 3.0
        out.append(x.astype(np.float32))
    return out


def synth_labels(rng, n, L, nc):
    return [rng.integers(1, nc, L).astype(np.int32) for _ in range(n)]


def oracle_minibatch(ora, OracleNet, params, ninput, nhidden, nclasses, lines, transcripts,
                     unidirectional=False, derivs0=None, lr=None, mom=None, states=()):
    """Reference semantics of one minibatch: every line is an independent bs=1 fwd/CTC/bwd
    (clstmhl.h:201-217) accumulating into the same Params.d.  Returns dict of results."""
    net = OracleNet(ora, ninput, nhidden, nclasses, unidirectional=unidirectional, init=False)
    net.set_params(params)
    if derivs0 is not None:
        net.set_derivs(derivs0)
    if lr is not None:
        net.set_lr(lr, mom)
    res = {"outputs": [], "aligned": [], "deltas": [], "decode": [], "states": {k: [] for k in states}}
    for x, tr in zip(lines, transcripts):
        net.set_inputs(x)
        out = net.forward()[:, 0, :]
        res["outputs"].append(out.copy())
        res["decode"].append(net.decode())
        if tr is not None:
            al = net.ctc_deltas(tr)
            res["aligned"].append(al.copy())
            res["deltas"].append(net.get_output_deltas()[:, 0, :].copy())
            net.backward()
        for k in states:
            layer, direction, which = k
            plane = 1 if which.startswith("d_") else 0
            s = net.state(layer, direction, which[2:] if plane else which, plane)[:, 0, :]
            if direction == 1:
                s = s[::-1]          # the NPLSTM inside Reversed runs on reversed frames
            res["states"][k].append(s.copy())
    res["derivs"] = net.get_derivs()
    res["net"] = net
    return res


# ---- the SGD update, stated exactly (tests/test_update_rule.py, tests/test_distributed.py) ---------------------------------------
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def fma_f32(a, b, c):
    """round_to_float32(a * b + c) with ONE rounding, elementwise, for float32 inputs.
    The product of two float32 is exact in float64 (48 significant bits).  s = p + c is rounded once to float64 and the TwoSum
    error term e (s + e == p + c exactly) is exact.  Rounding s to float32 is then wrong only when s lies exactly half way between
    two neighbouring float32 values while e != 0: the true sum lies on e's side of the tie."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(F32)
        r64 = r.astype(np.float64)
        diff = s - r64                                    # exact: r is within half a float32 ulp of s
        nb = np.nextafter(r, np.where(diff > 0, F32(np.inf), F32(-np.inf)).astype(F32))
        tie = np.isfinite(s) & np.isfinite(nb) & (diff != 0) & (diff == (nb.astype(np.float64) - r64) / 2)
        beyond = tie & (e != 0) & ((e > 0) == (diff > 0))
    return np.where(beyond, nb, r).astype(F32)


def update_of_clamped(v0, di, lr, mom):
    """what `v += lr * di ; d = di * mom` leaves, for the already clamped di = clip(d0 + g), in numpy float32 with one operation per
    rounding: (d', v' unfused, v' as the single-rounding fused multiply-add -- the compilers may contract `v += di * lr`)"""
    v0, di, lr, mom = np.asarray(v0, F32), np.asarray(di, F32), F32(lr), F32(mom)
    with np.errstate(invalid="ignore"):                    # (inf * 0: test_update_rule.py feeds +-inf to the per-operator entry points)
        return (di * mom).astype(F32), (v0 + (di * lr).astype(F32)).astype(F32), fma_f32(di, lr, v0)


def assert_update_bits(v1, d1, want, what, **inputs):
    """the acceptance rule of the update tests: d' bit for bit, v' bit for bit the unfused or the fused value.  want: what
    update_of_clamped returned; inputs: arrays quoted at the first differing entry"""
    ed, ev, evf = want
    at = lambda i: " ".join("%s %r" % (k, np.asarray(a).ravel()[i]) for k, a in inputs.items())
    bad = np.flatnonzero(bits(d1) != bits(ed))
    assert bad.size == 0, "%s: d' differs at %d of %d entries, first %d: got %r want %r (%s)" % (
        what, bad.size, d1.size, bad[0], d1[bad[0]], ed[bad[0]], at(bad[0]))
    bad = np.flatnonzero((bits(v1) != bits(ev)) & (bits(v1) != bits(evf)))
    assert bad.size == 0, "%s: v' differs at %d of %d entries, first %d: got %r want %r or %r (%s)" % (
        what, bad.size, v1.size, bad[0], v1[bad[0]], ev[bad[0]], evf[bad[0]], at(bad[0]))


def pm200(n):
    """derivs of +-200, the sign by index parity"""
    return np.where(np.arange(n) % 2 == 0, 200.0, -200.0).astype(F32)


def assert_every_entry_once(v0, d0, g, v1, d1, lr, mom, what):
    """d0 = pm200, |g| < 100, clip 100: d0 + g lies beyond the clip whatever the gradient arithmetic did, so the clamped sum is
    +-100, d' = +-f32(100 mom) and v' = v0 +- 100 lr exactly -- an entry the update missed, or visited twice, stands out.
    Returns max |g|."""
    assert np.isfinite(g).all() and np.abs(g).max() < 100.0, "inconclusive: max |g| = %g (%s)" % (np.abs(g).max(), what)
    assert np.array_equal(d0, pm200(d0.size))
    assert_update_bits(v1, d1, update_of_clamped(v0, d0 / F32(2.0), lr, mom), what, v0=v0, d0=d0, g=g)
    return float(np.abs(g).max())


class Backend:
    """Where the C ABI runs: 'emu' = host-thread emulator build of the kernel sources (CPU
    tests), 'hip' = the real libclstm_hip.so on an MI355X (-m gpu tests)."""

    def __init__(self, kind):
        self.kind = kind
        if kind == "emu":
            self.lib = emu_lib()
        else:
            import torch
            assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
            from clstm_amd import abi
            self.lib = abi.load()          # raises loudly if the HIP extension is missing
            self.torch = torch

    def up(self, a, dtype=np.float32):
        a = np.ascontiguousarray(a, dtype=dtype)
        if self.kind == "emu":
            return a.copy()
        return self.torch.from_numpy(a).cuda()

    def zeros(self, shape, dtype=np.float32):
        return self.up(np.zeros(shape, dtype), dtype)

    def down(self, d):
        if self.kind == "emu":
            return np.array(d, copy=True)
        self.lib.call("clstm_synchronize")
        return d.cpu().numpy()

    def sync(self):
        self.lib.call("clstm_synchronize")
