#!/usr/bin/env python3
"""Rate of the CTC prefix beam search launch (clstm_net_beam, csrc/ctc_beam.h).  Writes profiles/beam_rate.txt.  Needs a GPU.

Shape: 64 lines x T = 200, 83 classes, on the outputs of a BiLSTM(100) forward pass; beam = nbest = 1 / 4 / 8 / 16 / 32; then 1024
lines at beam 8.  Beside them, alternating in the same process (so drift hits all alike): the CTC alignment launch on the same
lines (transcripts of 25 labels) and the trivial decode of the same outputs.
Two figures per configuration, medians of REPEATS alternating repeats:
    kernel  the launch's own time between the pair of events it carries (clstm_net_enable_timing / clstm_net_kernel_time_ms);
            the decode's two small launches sit in no timing bracket, so it has none
    call    host wall clock of the whole library call, results on the host (timing off): what a caller waits for
No threshold: the first measurement of this kernel."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NI, NH, NC, T, L = 48, 100, 83, 200, 25
REPEATS = 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_rate.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_beam_rate.py needs a GPU")
    from clstm_amd import abi
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    lib = abi.load()
    rng = np.random.default_rng(0)
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    def measure(nlines, beams, repeats):
        net = Network(NI, [NH], NC, lib=lib)
        net.set_params(init_params(NI, NH, NC, seed=0.222) * 10.0)
        net.set_inputs([np.clip(rng.normal(0.2, 0.3, (T, NI)), 0, 1).astype(np.float32) for _ in range(nlines)])
        net.forward()
        trs = [rng.integers(1, NC, L).astype(np.int32) for _ in range(nlines)]
        cfg = {}
        for w in beams:
            cfg["beam %d" % w] = ("ctc_beam", lambda w=w: net.beam(w))
        cfg["ctc_align_kernel"] = ("ctc_align", lambda: net.ctc(trs))
        cfg["trivial decode"] = (None, lambda: net.decode())
        for _, fn in cfg.values():      # warm every configuration (allocations, LDS attribute, code upload)
            fn(); fn()
        kern, call = {name: [] for name in cfg}, {name: [] for name in cfg}
        for timed in (True, False):
            net.enable_timing(timed)
            for _ in range(repeats):
                for name, (kname, fn) in cfg.items():
                    if timed and kname:
                        net.reset_timing()
                        fn()
                        lib.call("clstm_synchronize")
                        ms, n = net.kernel_time_ms(kname)
                        assert n == 1, (name, n)
                        kern[name].append(ms * 1e3)
                    elif not timed:
                        lib.call("clstm_synchronize")
                        t0 = time.perf_counter()
                        fn()
                        lib.call("clstm_synchronize")
                        call[name].append((time.perf_counter() - t0) * 1e6)
        for name in cfg:
            k, c = np.array(kern[name]), np.array(call[name])
            ks = "%9.1f us  (spread %4.1f %%)  %11.0f lines/s" % (np.median(k), 100 * (k.max() - k.min()) / np.median(k),
                                                                   nlines / (np.median(k) * 1e-6)) if len(k) else "%45s" % "-"
            say("%5d lines  %-18s kernel %s   call %9.1f us  %11.0f lines/s" % (nlines, name, ks, np.median(c), nlines / (np.median(c) * 1e-6)))

    say("# CTC prefix beam search launch, nbest = beam; T = %d, %d classes; %s; medians of %d alternating repeats"
        % (T, NC, torch.cuda.get_device_name(0), REPEATS))
    measure(64, (1, 4, 8, 16, 32), REPEATS)
    say("# 1024 lines")
    measure(1024, (8,), 7)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
