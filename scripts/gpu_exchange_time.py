#!/usr/bin/env python3
"""The peer gradient exchange in its two forms, timed with 2, 4 and 8 rank processes that share device 0 (a communicator without
RCCL: CLSTM_COMM_NO_RCCL=1).  Writes profiles/exchange_two_phase.txt.  Needs a GPU.

SAME-DEVICE figures: every "peer" read is a read of the same HBM through another process's mapping, and the rank processes
time-share one GPU.  They show that both forms run at every size and what the kernels cost there; they say NOTHING about xGMI, and
no threshold is tuned from them.

Nets: B1 (BiLSTM(100), 48 inputs, 83 classes: 0.54 MB of gradient) and configs[4] (2 x BiLSTM(512), 64 inputs, 100 classes: 35 MB)
on a few short lines per rank.  Per net, rank count and form (CLSTM_DEBUG=peer_two_phase=0 / 2) rank 0 reports, per step, from
clstm_net_kernel_time_ms:
  allreduce_grads  barrier A [+ k_peer_reduce_scatter + barrier B], the launches' own durations: a barrier's is the time its
                   workgroup waits for the slowest rank's queued device work, and the ranks time-share the device
  sgd_update       k_peer_allreduce_update / k_peer_gather_update
  backward         every launch of the backward pass (lstm_bwd, gemm_*, reduce_scatter: the slab reductions that leave the
                   gradient in the fine-grained exchange slot)
and, per net, the same backward pass in a single-rank run through separate calls, which writes the local gradient buffer.

Every GPU step is a child process under `timeout -k 10`; the script stops at the first one that fails."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NETS = {"B1": (48, [100], 83, 10.0), "configs4": (64, [512, 512], 100, 3.0)}      # ninput, hidden layers, classes, weight scale
LINES_T = [24, 17, 9, 20]        # per rank
WARMUP, STEPS = 3, 10
BACKWARD = ("lstm_bwd", "gemm_gates_dw", "gemm_gates_dx", "gemm_softmax_dw_dx", "reduce_scatter")


def rank_main(rank, world, port, net_name, out):
    os.environ["CLSTM_COMM_NO_RCCL"] = "1"
    os.environ["CLSTM_XCD_REC"] = "0"           # the persistent wide kernels assume one process per device
    os.environ["CLSTM_REPLICA_CHECK_EVERY"] = "0"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    from clstm_amd import abi
    from clstm_amd.init import init_params
    from clstm_amd.net import Comm, Network
    from common import synth_lines
    torch.cuda.set_device(0)
    lib = abi.load()
    ni, nh, nc, scale = NETS[net_name]
    net = Network(ni, nh, nc, lib=lib)
    net.set_params(init_params(ni, nh, nc, seed=0.222) * scale)
    net.setLearningRate(1e-4, 0.9)
    rng = np.random.default_rng(7 + rank)
    lines = synth_lines(rng, LINES_T, ni)
    trs = [rng.integers(1, nc, max(1, t // 3)).astype(np.int32) for t in LINES_T]
    x = torch.from_numpy(np.ascontiguousarray(np.concatenate(lines, 0), np.float32)).cuda()
    comm = None
    if world > 1:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)

        def exchange(ident):
            box = [ident]
            dist.broadcast_object_list(box, src=0)
            return box[0]
        comm = Comm(rank, world, exchange, lib=lib)
        net.set_comm(comm)

    def step():
        if comm is not None:
            net.train_step(LINES_T, x, trs)
        else:                                   # single rank, separate calls: the reductions write the local gradient buffer
            net.set_inputs(lines); net.forward(); net.ctc(trs); net.backward(); net.update()
    for _ in range(WARMUP):
        step()
    lib.call("clstm_synchronize")
    net.enable_timing(True)
    net.reset_timing()
    for _ in range(STEPS):
        step()
    lib.call("clstm_synchronize")
    if rank == 0:
        t = {k: net.kernel_time_ms(k)[0] / STEPS for k in ("allreduce_grads", "sgd_update") + BACKWARD}
        res = {"net": net_name, "world": world, "nparams": int(net.nparams), "allreduce_grads": t["allreduce_grads"], "sgd_update": t["sgd_update"],
               "backward": sum(t[k] for k in BACKWARD), "reduce_scatter": t["reduce_scatter"],
               "capacity": comm.peer_capacity() if comm is not None else 0, "device": torch.cuda.get_device_name(0)}
        with open(out, "w") as f:
            json.dump(res, f)
    if comm is not None:
        net.set_comm(None)
        comm.close()
        dist.destroy_process_group()


def child(args):
    if args.world == 1:
        return rank_main(0, 1, 0, args.net, args.out)
    import torch.multiprocessing as mp
    mp.spawn(rank_main, args=(args.world, 23456 + os.getpid() % 2000, args.net, args.out), nprocs=args.world, join=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--net", default="B1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exchange_two_phase.txt"))
    ap.add_argument("--step-timeout", type=int, default=150)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import tempfile
    tmp = tempfile.mkdtemp(prefix="exchange_time_")
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    def run(net, world, form):
        res = os.path.join(tmp, "%s_%d_%s.json" % (net, world, form))
        env = dict(os.environ)
        env.pop("CLSTM_DEBUG", None)
        if form is not None:
            env["CLSTM_DEBUG"] = "peer_two_phase=%d" % form
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--world", str(world), "--net", net,
               "--out", res]
        r = subprocess.run(cmd, env=env)
        if r.returncode != 0 or not os.path.exists(res):
            say("# FAILED (exit %d): %s net, %d ranks, form %s -- stopping here" % (r.returncode, net, world, form))
            finish(1)
        return json.load(open(res))

    def finish(code):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")
        sys.exit(code)

    say("# peer gradient exchange, one-shot (peer_two_phase=0) against two-phase (peer_two_phase=2); ms per step on rank 0, mean of %d steps "
        "after %d; %d lines of T = %s per rank" % (STEPS, WARMUP, len(LINES_T), LINES_T))
    say("# SAME-DEVICE figures: the rank processes share device 0 (no RCCL) and time-share it; nothing here says anything about xGMI,")
    say("# and no threshold is tuned from it.  Durations of the launches themselves; a barrier's is its wait for the slowest rank's device work.")
    for net in ("B1", "configs4"):
        single = run(net, 1, None)
        say("%-8s %9d parameters (%.2f MB)  %s" % (net, single["nparams"], single["nparams"] * 4 / 1e6, single["device"]))
        say("  single rank, separate calls, local gradient buffer:      backward %8.3f  (slab reductions %7.3f)" % (single["backward"], single["reduce_scatter"]))
        for world in (2, 4, 8):
            for form, name in ((0, "one-shot "), (2, "two-phase")):
                r = run(net, world, form)
                say("  %d ranks %s  allreduce_grads %8.3f  sgd_update %8.3f  backward %8.3f  (slab reductions into the slot %7.3f)  capacity %d floats"
                    % (world, name, r["allreduce_grads"], r["sgd_update"], r["backward"], r["reduce_scatter"], r["capacity"]))
    finish(0)


if __name__ == "__main__":
    main()
