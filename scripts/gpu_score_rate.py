#!/usr/bin/env python3
"""Kernel time of the score launches (clstm_net_score, csrc/ctc_score.h) against the alignment launch (ctc_align_kernel) on the same
lattices, alternating in one process.  Writes profiles/score_rate.txt.  Needs a GPU.

Shape: 64 lines x T = 200, transcripts of 25 labels (S = 51), 101 classes, on the outputs of a BiLSTM(100) forward pass.
Measured per repeat, round robin over the configurations (so drift hits them alike), REPEATS times each; a figure is the kernel
time of ONE call's launches between the pair of events each launch carries (clstm_net_enable_timing / clstm_net_kernel_time_ms):
    sum form at K = 1, 8, 32 candidates per line;  max-plus form with paths at K = 1;  ctc_align_kernel on the same 64 lattices.
Reported: median, spread (max - min) / median, lattices per second.  Then the same at 2048 lines x 1 candidate.
Two comparisons decide the exit status:
    (1) at K = 1 the sum form is no slower than the alignment launch (it does a strict subset of that launch's work);
    (2) lattices per second at K = 32 are no lower than at K = 1 (batching candidates must not cost)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NI, NH, NC, T, L = 48, 100, 101, 200, 25
REPEATS = 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_rate.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_score_rate.py needs a GPU")
    from clstm_amd import abi
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    lib = abi.load()
    rng = np.random.default_rng(0)
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    def measure(nlines, ks, repeats):
        net = Network(NI, [NH], NC, lib=lib)
        net.set_params(init_params(NI, NH, NC, seed=0.222) * 10.0)
        net.set_inputs([np.clip(rng.normal(0.2, 0.3, (T, NI)), 0, 1).astype(np.float32) for _ in range(nlines)])
        net.forward()
        trs = [rng.integers(1, NC, L).astype(np.int32) for _ in range(nlines)]
        cfg = {}
        for k in ks:
            cands = [rng.integers(1, NC, L).astype(np.int32) for _ in range(nlines * k)]
            cl = [b for b in range(nlines) for _ in range(k)]
            cfg["score sum K=%d" % k] = ("ctc_score", nlines * k, lambda c=cands, l=cl: net.score(c, lines=l))
        cfg["score max-plus + paths K=1"] = ("ctc_score", nlines, lambda: net.align(trs))
        cfg["ctc_align_kernel"] = ("ctc_align", nlines, lambda: net.ctc(trs))
        net.enable_timing(True)
        for _, _, fn in cfg.values():      # warm every configuration (allocations, LDS attribute, code upload)
            fn(); fn()
        times = {name: [] for name in cfg}
        for _ in range(repeats):
            for name, (kname, _, fn) in cfg.items():
                net.reset_timing()
                fn()
                lib.call("clstm_synchronize")
                ms, n = net.kernel_time_ms(kname)
                assert n == 1, (name, n)
                times[name].append(ms * 1e3)
        res = {}
        for name, (_, nlat, _) in cfg.items():
            t = np.array(times[name])
            med = float(np.median(t))
            res[name] = (med, nlat / (med * 1e-6))
            say("%5d lines  %-28s %9.1f us  (spread %4.1f %%)  %6d lattices  %12.0f lattices/s  %7.1f ns per lattice frame"
                % (nlines, name, med, 100 * (t.max() - t.min()) / med, nlat, res[name][1], med * 1e3 / (nlat * T)))
        return res

    say("# score launches vs the alignment launch, kernel time per call; T = %d, S = %d, %d classes; %s; median of %d alternating repeats"
        % (T, 2 * L + 1, NC, torch.cuda.get_device_name(0), REPEATS))
    r64 = measure(64, (1, 8, 32), REPEATS)
    say("# the large_minibatch shape")
    measure(2048, (1,), 20)
    ok1 = r64["score sum K=1"][0] <= r64["ctc_align_kernel"][0]
    ok2 = r64["score sum K=32"][1] >= r64["score sum K=1"][1]
    say("# (1) sum form at K = 1 no slower than the alignment launch: %s (%.1f vs %.1f us)"
        % ("yes" if ok1 else "NO", r64["score sum K=1"][0], r64["ctc_align_kernel"][0]))
    say("# (2) lattices/s at K = 32 no lower than at K = 1: %s (%.0f vs %.0f)"
        % ("yes" if ok2 else "NO", r64["score sum K=32"][1], r64["score sum K=1"][1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    if not (ok1 and ok2):
        sys.exit(1)


if __name__ == "__main__":
    main()
