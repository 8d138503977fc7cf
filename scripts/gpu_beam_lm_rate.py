#!/usr/bin/env python3
"""Rate of the beam search launch with a character n-gram language model (clstm_net_beam_lm, csrc/ctc_beam.h, second part).
Writes profiles/beam_lm_rate.txt.  Needs a GPU.

Shape: gpu_beam_rate.py's -- 64 lines x T = 200, 83 classes, on the outputs of a BiLSTM(100) forward pass; then 1024 lines.
beam = nbest = 4 / 8 / 16 (1024 lines: 8), a random table of order 2 and of order 3 with an end table, weight 0.5.  Beside each
width, alternating in the same process (so drift hits all alike), the launch without a model (clstm_net_beam).
Per configuration the median kernel time of REPEATS alternating repeats (the launch's own pair of events: clstm_net_enable_timing /
clstm_net_kernel_time_ms) and the host wall clock of the whole call, as gpu_beam_rate.py takes them; for the 64-line launches (one
line per CU, all at once) also the time per frame.  With a model every class is a candidate of every entry -- beam (1 + nc - 1)
keys per frame against beam (1 + min(nc - 1, 2 beam)) without --, the sorted class list lies in the workspace, the table in global
memory (through L2; 27 KB at order 2, 2.3 MB at order 3).
No threshold: the first measurement of this form."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NI, NH, NC, T = 48, 100, 83, 200
REPEATS = 15
WEIGHT = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_lm_rate.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_beam_lm_rate.py needs a GPU")
    from clstm_amd import abi
    from clstm_amd.init import init_params
    from clstm_amd.lm import CharLM
    from clstm_amd.net import Network
    lib = abi.load()
    rng = np.random.default_rng(0)
    lms = {o: CharLM(o, NC, rng.normal(-3.0, 1.5, (NC ** (o - 1), NC)).astype(np.float32),
                     rng.normal(-3.0, 1.5, NC ** (o - 1)).astype(np.float32), lib=lib) for o in (2, 3)}
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    def measure(nlines, beams, repeats):
        net = Network(NI, [NH], NC, lib=lib)
        net.set_params(init_params(NI, NH, NC, seed=0.222) * 10.0)
        net.set_inputs([np.clip(rng.normal(0.2, 0.3, (T, NI)), 0, 1).astype(np.float32) for _ in range(nlines)])
        net.forward()
        cfg = {}
        for w in beams:
            cfg["beam %d" % w] = ("ctc_beam", w * (1 + min(NC - 1, 2 * w)), lambda w=w: net.beam(w))
            for o in (2, 3):
                cfg["beam %d order %d" % (w, o)] = ("ctc_beam_lm", w * NC, lambda w=w, o=o: net.beam_lm(lms[o], WEIGHT, beam=w))
        for _, _, fn in cfg.values():      # warm every configuration (allocations, LDS attribute, code upload)
            fn(); fn()
        kern, call = {name: [] for name in cfg}, {name: [] for name in cfg}
        for timed in (True, False):
            net.enable_timing(timed)
            for _ in range(repeats):
                for name, (kname, _, fn) in cfg.items():
                    if timed:
                        net.reset_timing()
                        fn()
                        lib.call("clstm_synchronize")
                        ms, n = net.kernel_time_ms(kname)
                        assert n == 1, (name, n)
                        kern[name].append(ms * 1e3)
                    else:
                        lib.call("clstm_synchronize")
                        t0 = time.perf_counter()
                        fn()
                        lib.call("clstm_synchronize")
                        call[name].append((time.perf_counter() - t0) * 1e6)
        for name, (_, keys, _) in cfg.items():
            k, c = np.array(kern[name]), np.array(call[name])
            frame = "%6.2f us/frame" % (np.median(k) / T) if nlines <= 64 else "%15s" % ""
            say("%5d lines  %-16s %5d keys/frame  kernel %9.1f us  (spread %4.1f %%)  %s  %9.0f lines/s   call %9.1f us"
                % (nlines, name, keys, np.median(k), 100 * (k.max() - k.min()) / np.median(k), frame, nlines / (np.median(k) * 1e-6), np.median(c)))

    say("# beam search launch with and without a character n-gram model, nbest = beam, weight %.1f; T = %d, %d classes; %s; medians of %d alternating repeats"
        % (WEIGHT, T, NC, torch.cuda.get_device_name(0), REPEATS))
    say("# with a model: every class a candidate of every entry, class list in the workspace, table in global memory")
    measure(64, (4, 8, 16), REPEATS)
    say("# 1024 lines")
    measure(1024, (8,), 7)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
