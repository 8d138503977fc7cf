#!/usr/bin/env python3
"""Line degradation on one MI355X against the host degrade_line.  Writes profiles/degrade_rate.txt.  Needs a GPU.

(1) The degrader alone on 64 and 1024 copies of the fixture line (tests/golden/textline.bin.png, 819 x 88), parameters drawn at the
    default ranges (clstm_degrade_draw, seed 0, key = position, visit 0): device lines/s of clstm_degrader_run_d (pixels resident),
    of the same call with only the warp (maxdelta = 0, blur = 0), and of clstm_normalizer_run_d alone on the same lines, in
    alternating windows -- a window runs whole calls until MIN_WINDOW_S have passed and ends with a synchronise -- with the spread
    (max - min over the windows, relative to the median); the host degrade_line on the same lines and parameters on 1 and on 16
    threads (`clstm_hosttool degrade-bench`) on the same box.
(2) `clstmocrtrain batch=64 gpu_prep=1` on the 512-line rendered corpus (scripts/make_corpus.py): degrade=0 cache=0 against degrade=1
    (both normalise every line on the device), three alternations, whole-process wall time, lines/s.

--profile-run: a few run_d calls on 64 copies and nothing else -- the workload for
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/gpu_degrade_rate.py --profile-run
--kernel-table DIR: append the kernel rows of that run's statistics, with each kernel's share, to the output file."""
import argparse
import csv
import glob
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "clstm_amd", "bin")
FIXTURE = os.path.join(ROOT, "tests", "golden", "textline.bin.png")
MIN_WINDOW_S, ALTERNATIONS = 1.0, 3
PROFILE_CALLS = 10


def fixture_line(tmp):
    raw = os.path.join(tmp, "fixture.raw")
    subprocess.run([os.path.join(BIN, "clstm_hosttool"), "png2raw", FIXTURE, raw], check=True)
    data = open(raw, "rb").read()
    w, h = struct.unpack("<ii", data[:8])
    return np.ascontiguousarray(np.float32(1.0) - np.frombuffer(data[8:], np.float32).reshape(w, h))


def spread(r):
    return (max(r) - min(r)) / float(np.median(r))


def setup(n, tmp, lib):
    import torch
    from clstm_amd.net import Normalizer, degrade_line, draw
    img = fixture_line(tmp)
    pix, w, h = Normalizer.pack([img] * n)
    lines = [draw(0, k, 0, img.shape[0], img.shape[1], lib=lib) for k in range(n)]
    warp_only = [degrade_line(tuple(d.m), d.tx, d.ty) for d in lines]
    return img, torch.from_numpy(pix).cuda(), w, h, lines, warp_only


def degrader_rates(say, tmp):
    from clstm_amd import abi
    from clstm_amd.net import Degrader, Normalizer
    lib = abi.load()
    for n in (64, 1024):
        img, pix_d, w, h, lines, warp_only = setup(n, tmp, lib)
        dg, nz = Degrader(lib=lib), Normalizer(48, lib=lib)

        def window(fn):
            done, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < MIN_WINDOW_S:
                fn()
                done += n
            lib.call("clstm_synchronize")
            return done / (time.perf_counter() - t0)
        calls = [("degrader run_d, every stage", lambda: dg.run_device_pixels(pix_d, w, h, lines)),
                 ("degrader run_d, warp only", lambda: dg.run_device_pixels(pix_d, w, h, warp_only)),
                 ("normalizer run_d alone", lambda: nz.run_device_pixels(pix_d, w, h)),
                 ("degrader + normalizer", lambda: nz.run_device_pixels(dg.run_device_pixels(pix_d, w, h, lines), w, h))]
        for _, fn in calls:
            fn(); fn()
        rates = [[] for _ in calls]
        for _ in range(ALTERNATIONS):
            for r, (_, fn) in zip(rates, calls):
                r.append(window(fn))
        for r, (name, _) in zip(rates, calls):
            say("%4d copies of the fixture line   %-30s %9.0f lines/s (spread %4.1f %%)" % (n, name, np.median(r), 100 * spread(r)))
        say("%4d copies: device bytes degrader %d, normalizer %d" % (n, dg.device_bytes(), nz.device_bytes()))
        del dg, nz
        if n > 64:
            continue
        raws = os.path.join(tmp, "copies%d.raw" % n)
        with open(raws, "wb") as f:
            for _ in range(n):
                f.write(struct.pack("<ii", img.shape[0], img.shape[1]))
                f.write(img.tobytes())
        for threads in (1, 16):
            r = []
            for _ in range(ALTERNATIONS):
                out = subprocess.run([os.path.join(BIN, "clstm_hosttool"), "degrade-bench", raws, str(threads)], check=True,
                                     capture_output=True, text=True).stdout.split()
                r.append(float(out[out.index("lines/s") - 1]))
            say("%4d copies, host degrade_line on %2d thread(s) %9.0f lines/s (spread %4.1f %%)" % (n, threads, np.median(r), 100 * spread(r)))


def cli_rates(say):
    from make_corpus import make_corpus
    d = tempfile.mkdtemp(prefix="degrade_cli_")
    names, _ = make_corpus(d, n=512, seed=0)
    base = dict(os.environ, batch="64", ntrain="4096", lrate="1e-4", nhidden="100", seed="0.222", save_name="", gpu_prep="1",
                report_every="1000000", test_every="100000000")
    rates = {0: [], 1: []}
    for _ in range(3):
        for g in (0, 1):
            env = dict(base, degrade=str(g))
            if g == 0:
                env["cache"] = "0"
            t0 = time.perf_counter()
            subprocess.run([os.path.join(BIN, "clstmocrtrain"), os.path.join(d, "list.txt")], env=env, check=True, capture_output=True, timeout=600)
            rates[g].append(4096 / (time.perf_counter() - t0))
    say("# clstmocrtrain batch=64 gpu_prep=1 ntrain=4096 on the 512-line rendered corpus, wall time of the whole process (start-up, PNG decoding included), lines/s")
    for g, name in ((0, "degrade=0 cache=0"), (1, "degrade=1        ")):
        say("clstmocrtrain %s  %s   median %.0f (spread %.1f %%)" % (name, " ".join("%.0f" % r for r in rates[g]), float(np.median(rates[g])), 100 * spread(rates[g])))
    say("degrade=1 / degrade=0 cache=0: %.2f" % (float(np.median(rates[1])) / float(np.median(rates[0]))))


def kernel_table(say, d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Name"].startswith(("k_dg_", "k_nz_")):
                rows.append((r["Name"].split("(")[0], int(r["Calls"]), float(r["TotalDurationNs"])))
    total = sum(r[2] for r in rows)
    say("# device time per kernel (rocprofv3 --kernel-trace --stats of --profile-run: run_d, every stage, on 64 copies of the fixture line;")
    say("# k_nz_filter_rows serves the noise fields and the blur, k_nz_filter_run the blur's column pass)")
    for name, calls, ns in sorted(rows, key=lambda r: -r[2]):
        say("%-18s %5d launches  %9.1f us per call of 64 lines  %5.1f %%" % (name, calls, ns / 1e3 / PROFILE_CALLS, 100 * ns / total if total else 0.0))
    say("all kernels: %.1f us per call of 64 lines" % (total / 1e3 / PROFILE_CALLS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-table")
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_rate.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)
    if args.kernel_table:
        kernel_table(say, args.kernel_table)
        with open(args.out, "a") as f:
            f.write("\n".join(out) + "\n")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_degrade_rate.py needs a GPU")
    tmp = tempfile.mkdtemp(prefix="degrade_rate_")
    if args.profile_run:
        from clstm_amd import abi
        from clstm_amd.net import Degrader
        lib = abi.load()
        _, pix_d, w, h, lines, _ = setup(64, tmp, lib)
        dg = Degrader(lib=lib)
        for _ in range(PROFILE_CALLS):
            dg.run_device_pixels(pix_d, w, h, lines)
        lib.call("clstm_synchronize")
        return
    say("# line degradation: device (clstm_degrader_run_d) against the host degrade_line; %s" % torch.cuda.get_device_name(0))
    degrader_rates(say, tmp)
    if not args.skip_cli:
        cli_rates(say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
