"""The peer gradient exchange above 4 MB and its two-phase form (comm.h, ops.h: k_peer_reduce_scatter / k_peer_gather_update).

Both forms of the exchange add the ranks' gradients in rank order 0..R-1 starting from rank 0's value, so the two-phase result must be
BIT-identical to the one-shot result on every rank: most checks here are byte comparisons of everything a run saves, between a run
under the default rule and a run with the experiment option peer_two_phase forced (CLSTM_DEBUG in the rank processes' environment),
plus the path counters -- 7 counts every fused peer exchange + update, 24 the two-phase ones.  CPU: the host emulator's rank
processes; GPU: rank processes that share device 0 through a communicator without RCCL."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from test_distributed import (SAT_SHAPE, _check_replicas_and_oracle, _driver_fixture, _port, gpu_worker, make_data, oracle_after,  # noqa: F401
                              worker)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PHASE = 24            # clstm_debug_path_count: fused peer exchanges that took the two-phase form
TINY_SHAPE = (1, 1, 2)    # 30 parameters: at 8 ranks the segments hold 4 floats, segment 6 holds 2 and segment 7 is empty
BIG_SHAPE = (8, 512, 5)   # 2,139,141 parameters > 2^20: beyond the exchange slots' first capacity
BIG_SCALE = 3.0           # weight scale of the big net (the x3 of test_stacked_bilstm512_shape_vs_oracle: the gates do not saturate)
BIG_LR, BIG_MOM = 1e-4, 0.9


def _count(lib, which):
    c = ctypes.c_longlong(0)
    lib.call("clstm_debug_path_count", which, ctypes.byref(c))
    return int(c.value)


def _write_counts(lib, outdir, rank):
    open(os.path.join(outdir, "counts_%d.txt" % rank), "w").write("%d %d" % (_count(lib, 7), _count(lib, TWO_PHASE)))


def counting_worker(rank, world, port, outdir, *args):
    """test_distributed.worker, then path counters 7 and 24 of this rank process (they are process-global) into a file"""
    worker(rank, world, port, outdir, *args)
    from common import emu_lib
    _write_counts(emu_lib(), outdir, rank)


def counting_gpu_worker(rank, world, port, outdir, *args):
    gpu_worker(rank, world, port, outdir, *args)
    from clstm_amd import abi
    _write_counts(abi.load(), outdir, rank)


def _counts(outdir, world):
    return [tuple(int(x) for x in open(os.path.join(str(outdir), "counts_%d.txt" % r)).read().split()) for r in range(world)]


def _saved(outdir, world, names=("v1", "d1", "g")):
    """every array a pm200 run saved, keyed by (name, step, rank); the ranks must agree byte for byte"""
    out = {}
    for step in range(2):
        for name in names:
            for r in range(world):
                a = np.load(os.path.join(str(outdir), "%s_%d_%d.npy" % (name, step, r)))
                out[name, step, r] = a
                assert a.tobytes() == out[name, step, 0].tobytes(), "%s of step %d: rank %d differs from rank 0" % (name, step, r)
    return out


def _assert_same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), "%s: %s of step %d, rank %d differs between the two forms" % ((what,) + k)


def _both_forms(monkeypatch, tmp_path, spawn, world, fused):
    """spawn(outdir) once under the default rule and once with the two-phase form forced: everything saved byte-equal between the
    runs and across ranks; counter 7 counts both steps in both runs where the exchange is fused into the update (else 0: the
    exchange is the plain all-reduce and k_update follows), counter 24 only in the forced run"""
    got = {}
    for tag, opt in (("default", None), ("forced", "peer_two_phase=2")):
        if opt:
            monkeypatch.setenv("CLSTM_DEBUG", opt)
        else:
            monkeypatch.delenv("CLSTM_DEBUG", raising=False)
        (tmp_path / tag).mkdir()
        spawn(str(tmp_path / tag))
        got[tag] = _saved(tmp_path / tag, world)
        n = 2 if fused else 0
        assert _counts(tmp_path / tag, world) == [(n, n if opt else 0)] * world, (tag, _counts(tmp_path / tag, world))
    _assert_same_bytes(got["default"], got["forced"], "%d ranks" % world)


# ---- CPU suite: the host emulator ------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,shape", [(2, SAT_SHAPE), (4, SAT_SHAPE), (8, SAT_SHAPE), (8, TINY_SHAPE)],
                         ids=["2_ranks_455", "4_ranks_455", "8_ranks_455_partial_last_segment", "8_ranks_30_empty_segment"])
def test_two_phase_is_bit_identical_to_one_shot(tmp_path, monkeypatch, world, shape):
    """455 parameters (455 % 4 == 3): at 8 ranks the segments are 60 floats, the last holds 35 and ends in a partial 16-byte group.
    30 parameters on 8 ranks: segments of 4 floats, segment 6 holds 2 and segment 7 is empty."""
    import torch.multiprocessing as mp
    from common import emu_lib
    emu_lib()
    _both_forms(monkeypatch, tmp_path,
                lambda out: mp.spawn(counting_worker, args=(world, _port(22000), out, "one_call", 0.0, False, None, "pm200", shape), nprocs=world, join=True),
                world, True)


def flat_worker(rank, world, port, outdir, gpu, lengths):
    """clstm_allreduce_flat over buffers of the given lengths; each rank saves what it got"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if gpu:
        os.environ["CLSTM_COMM_NO_RCCL"] = "1"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clstm_amd.net import Comm
    if gpu:
        from clstm_amd import abi
        torch.cuda.set_device(0)
        lib = abi.load()
    else:
        from common import emu_lib
        lib = emu_lib()

    def exchange(ident):
        box = [ident]
        dist.broadcast_object_list(box, src=0)
        return box[0]
    comm = Comm(rank, world, exchange, lib=lib)
    for n in lengths:
        buf = torch.from_numpy(flat_input(rank, n))
        if gpu:
            buf = buf.cuda()
            torch.cuda.synchronize()
        comm.allreduce(buf, n)
        lib.call("clstm_synchronize")
        np.save(os.path.join(outdir, "flat_%d_%d.npy" % (n, rank)), buf.cpu().numpy())
    comm.close()
    dist.destroy_process_group()


def flat_input(rank, n):
    return np.random.default_rng(1000 * rank + n).normal(0, 1, n).astype(np.float32)


FLAT_LENGTHS = (1, 5, 455, 4097)


def _check_flat(outdir, world):
    for n in FLAT_LENGTHS:
        want = flat_input(0, n)
        for r in range(1, world):
            want = want + flat_input(r, n)          # float32, in rank order from rank 0's value
        assert want.dtype == np.float32
        for r in range(world):
            got = np.load(os.path.join(str(outdir), "flat_%d_%d.npy" % (n, r)))
            assert got.tobytes() == want.tobytes(), "length %d, rank %d of %d" % (n, r, world)


@pytest.mark.parametrize("world", [2, 4])
def test_allreduce_flat_two_phase_is_the_rank_ordered_sum(tmp_path, monkeypatch, world):
    """lengths 1 (one segment of one float, the others empty), 5, 455 and 4097 (all end in a partial group)"""
    import torch.multiprocessing as mp
    from common import emu_lib
    emu_lib()
    monkeypatch.setenv("CLSTM_DEBUG", "peer_two_phase=2")
    mp.spawn(flat_worker, args=(world, _port(21000), str(tmp_path), False, FLAT_LENGTHS), nprocs=world, join=True)
    _check_flat(tmp_path, world)


def test_two_phase_run_matches_the_oracle(tmp_path, monkeypatch, ora32):
    """the bars of test_distributed (they hold for the one-shot form, and the bytes are identical) on a forced run of four ranks"""
    import torch.multiprocessing as mp
    from common import emu_lib
    emu_lib()
    monkeypatch.setenv("CLSTM_DEBUG", "peer_two_phase=2")
    mp.spawn(counting_worker, args=(4, _port(20000), str(tmp_path), "one_call"), nprocs=4, join=True)
    assert _counts(tmp_path, 4) == [(2, 2)] * 4
    _check_replicas_and_oracle(tmp_path, ora32, 4, "4 ranks, two-phase")


def test_peer_capacity_binding_before_set_up():
    """clstm_comm_peer_capacity / Comm.peer_capacity(): 0 on a communicator that has set nothing up"""
    from clstm_amd.net import Comm
    from common import emu_lib
    comm = Comm(0, 1, lambda ident: ident, lib=emu_lib())
    assert comm.peer_capacity() == 0
    comm.close()


# ---- GPU suite: rank processes that share device 0 -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("one_call", [True, False], ids=["train_step_fused_update", "separate_calls_plain_allreduce"])
@pytest.mark.parametrize("world,shape", [(2, SAT_SHAPE), (4, SAT_SHAPE), (8, SAT_SHAPE), (8, TINY_SHAPE)],
                         ids=["2_ranks_455", "4_ranks_455", "8_ranks_455_partial_last_segment", "8_ranks_30_empty_segment"])
def test_gpu_two_phase_is_bit_identical_to_one_shot(tmp_path, monkeypatch, world, shape, one_call):
    """test_two_phase_is_bit_identical_to_one_shot on the MI355X, through clstm_net_train_step (the fused kernels) and through
    separate calls (the same kernels as the plain all-reduce of Comm::allreduce, then k_update)"""
    import torch.multiprocessing as mp
    _both_forms(monkeypatch, tmp_path,
                lambda out: mp.spawn(counting_gpu_worker, args=(world, _port(36000), out, True, one_call, 0.0, None, "pm200", shape), nprocs=world, join=True),
                world, one_call)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_gpu_allreduce_flat_two_phase_is_the_rank_ordered_sum(tmp_path, monkeypatch, world):
    import torch.multiprocessing as mp
    monkeypatch.setenv("CLSTM_DEBUG", "peer_two_phase=2")
    mp.spawn(flat_worker, args=(world, _port(37000), str(tmp_path), True, FLAT_LENGTHS), nprocs=world, join=True)
    _check_flat(tmp_path, world)


def _big_params(shape, scale):
    from clstm_amd.init import init_params
    return init_params(*shape, seed=0.222) * scale


def _gpu_rank_setup(rank, world, port):
    os.environ["CLSTM_COMM_NO_RCCL"] = "1"
    os.environ["CLSTM_REPLICA_CHECK_EVERY"] = "1"
    os.environ["CLSTM_XCD_REC"] = "0"           # the persistent wide kernels assume one process per device
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clstm_amd import abi
    lib = abi.load()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    lib.call("clstm_set_stream", stream.cuda_stream)

    def exchange(ident):
        box = [ident]
        dist.broadcast_object_list(box, src=0)
        return box[0]
    return torch, dist, lib, exchange


def _gpu_net(torch, lib, shape, scale, lr, mom):
    from clstm_amd.net import Network
    dev = torch.device("cuda", 0)
    params = torch.from_numpy(_big_params(shape, scale).copy()).to(dev)
    derivs, grads = torch.zeros_like(params), torch.zeros_like(params)
    net = Network(*shape, lib=lib, params=params, derivs=derivs, grads=grads)
    net.params_changed()
    net.setLearningRate(lr, mom)
    return net, (params, derivs, grads)


def _gpu_step(torch, net, step, rank, world, shape):
    from clstm_amd.parallel import shard
    lines, trs = make_data(step, world, shape)
    mine_l, mine_t = shard(lines, rank, world), shard(trs, rank, world)
    x = torch.from_numpy(np.ascontiguousarray(np.concatenate(mine_l, 0), np.float32)).to(torch.device("cuda", 0))
    net.train_step([len(l) for l in mine_l], x, mine_t)


def big_worker(rank, world, port, outdir):
    """two one-call steps of the big net on make_data's lines; saves parameters, derivs and gradient of every step, the
    exchange capacity and the path counters"""
    torch, dist, lib, exchange = _gpu_rank_setup(rank, world, port)
    from clstm_amd.net import Comm
    comm = Comm(rank, world, exchange, lib=lib)
    net, bufs = _gpu_net(torch, lib, BIG_SHAPE, BIG_SCALE, BIG_LR, BIG_MOM)
    net.set_comm(comm)
    for step in range(2):
        _gpu_step(torch, net, step, rank, world, BIG_SHAPE)
        lib.call("clstm_synchronize")            # (also the verdict of the replica check behind the update)
        for name, t in zip(("v1", "d1", "g"), bufs):
            np.save(os.path.join(outdir, "%s_%d_%d.npy" % (name, step, rank)), t.cpu().numpy())
    open(os.path.join(outdir, "cap_%d.txt" % rank), "w").write("%d %d" % (comm.peer_capacity(), lib.call("clstm_comm_peer_active", comm.h)))
    _write_counts(lib, outdir, rank)
    net.set_comm(None)
    comm.close()
    dist.destroy_process_group()


BIG_NPARAMS = 2139141


def _big_oracle(ora32, world):
    """oracle_after's steps for the big net at its own weight scale and learning rate"""
    from oracle.oracle import OracleNet
    ref = OracleNet(ora32, *BIG_SHAPE, init=False)
    ref.set_params(_big_params(BIG_SHAPE, BIG_SCALE))
    ref.set_lr(BIG_LR, BIG_MOM)
    for step in range(2):
        lines, trs = make_data(step, world, BIG_SHAPE)
        for x, t in zip(lines, trs):
            ref.set_inputs(x); ref.forward(); ref.ctc_deltas(t); ref.backward()
        ref.update()
    return ref


def _run_big(tmp_path, monkeypatch, tag, world, opt):
    import torch.multiprocessing as mp
    if opt:
        monkeypatch.setenv("CLSTM_DEBUG", opt)
    else:
        monkeypatch.delenv("CLSTM_DEBUG", raising=False)
    (tmp_path / tag).mkdir()
    mp.spawn(big_worker, args=(world, _port(38000), str(tmp_path / tag)), nprocs=world, join=True)
    caps = [tuple(int(x) for x in open(tmp_path / tag / ("cap_%d.txt" % r)).read().split()) for r in range(world)]
    assert all(c >= BIG_NPARAMS and active == 1 for c, active in caps) and len(set(caps)) == 1, caps
    return _saved(tmp_path / tag, world), _counts(tmp_path / tag, world)


def _check_big_oracle(got, ora32, world):
    from common import assert_close
    ref = _big_oracle(ora32, world)
    assert ref.get_params().size == BIG_NPARAMS
    for name, a, b, rtol, atol in (("params", got["v1", 1, 0], ref.get_params(), 2e-5, 2e-7),
                                   ("derivs", got["d1", 1, 0], ref.get_derivs(), 1e-4, 1e-9 + 2e-4 * float(np.abs(ref.get_derivs()).max()))):
        a, b = a.astype(np.float64), b.astype(np.float64)
        print("big net, %d ranks, %s: max |got - oracle| = %.3g, largest error / bar = %.3g" % (world, name, np.abs(a - b).max(), (np.abs(a - b) / (atol + rtol * np.abs(b))).max()))
    # the bars of tests/test_net_parity.py:222-223
    assert_close(got["v1", 1, 0], ref.get_params(), rtol=2e-5, atol=2e-7, what="params after 2 DP steps, %d ranks" % world)
    assert_close(got["d1", 1, 0], ref.get_derivs(), rtol=1e-4, atol=1e-9, scale_atol=2e-4, what="momentum buffer after 2 DP steps, %d ranks" % world)


@pytest.mark.gpu
def test_gpu_gradient_above_4mb_two_ranks_one_shot(tmp_path, monkeypatch, ora32):
    """Network(8, 512, 5): 2,139,141 parameters, 8.6 MB of gradient, weights x3, lr 1e-4.  Two ranks under the default rule: the
    exchange slots are set up at a capacity that holds the gradient and the one-shot form runs at full size (counter 7 is 2,
    counter 24 is 0) -- where the communicator without RCCL used to raise "the ranks could not map each other's exchange buffers"."""
    got, counts = _run_big(tmp_path, monkeypatch, "default", 2, None)
    assert counts == [(2, 0)] * 2, counts
    _check_big_oracle(got, ora32, 2)


@pytest.mark.gpu
def test_gpu_gradient_above_4mb_four_ranks_two_phase(tmp_path, monkeypatch, ora32):
    """The same net on four ranks: the default rule takes the two-phase form (counter 24 is 2); with peer_two_phase=0 the one-shot
    form at full size leaves the same bytes in parameters, derivs and gradient, on every rank."""
    got, counts = _run_big(tmp_path, monkeypatch, "default", 4, None)
    assert counts == [(2, 2)] * 4, counts
    one, counts1 = _run_big(tmp_path, monkeypatch, "one_shot", 4, "peer_two_phase=0")
    assert counts1 == [(2, 0)] * 4, counts1
    _assert_same_bytes(got, one, "big net, 4 ranks")
    _check_big_oracle(got, ora32, 4)


def growth_worker(rank, world, port, outdir):
    """small net, big net, small net again: once over ONE communicator, whose exchange slots must grow for the big net and stay
    grown, and once over a fresh communicator per net"""
    torch, dist, lib, exchange = _gpu_rank_setup(rank, world, port)
    from clstm_amd.net import Comm
    order = [("small", SAT_SHAPE, 30.0, 5e-2), ("big", BIG_SHAPE, BIG_SCALE, BIG_LR), ("small", SAT_SHAPE, 30.0, 5e-2)]
    results, caps = {}, []
    for mode in ("shared", "fresh"):
        comm = Comm(rank, world, exchange, lib=lib) if mode == "shared" else None
        nets = {}
        for i, (name, shape, scale, lr) in enumerate(order):
            if mode == "fresh":
                comm = Comm(rank, world, exchange, lib=lib)
            if name not in nets:
                nets[name] = _gpu_net(torch, lib, shape, scale, lr, 0.9)
            net, bufs = nets[name]
            net.set_comm(comm)
            _gpu_step(torch, net, i, rank, world, shape)
            lib.call("clstm_synchronize")
            results[mode, i] = [t.cpu().numpy().copy() for t in bufs]
            if mode == "shared":
                caps.append(comm.peer_capacity())
            net.set_comm(None)
            if mode == "fresh":
                comm.close()
        if mode == "shared":
            comm.close()
    for i in range(len(order)):
        for a, b in zip(results["shared", i], results["fresh", i]):
            assert a.tobytes() == b.tobytes(), "exchange %d (%s net) over the grown communicator differs from a fresh one" % (i, order[i][0])
        np.save(os.path.join(outdir, "params_%d_%d.npy" % (i, rank)), results["shared", i][0])
    open(os.path.join(outdir, "caps_%d.txt" % rank), "w").write(" ".join(str(c) for c in caps))
    _write_counts(lib, outdir, rank)
    dist.destroy_process_group()


@pytest.mark.gpu
def test_gpu_exchange_slots_grow_on_one_communicator(tmp_path, monkeypatch):
    """One communicator of four ranks serves the 455-parameter net for a step (one-shot, slots of 2^20 floats), then the big net
    (the slots are set up again at a larger capacity; two-phase), then the small net again: byte-equal to fresh communicators,
    identical on every rank, and the capacity grew and did not shrink."""
    import torch.multiprocessing as mp
    monkeypatch.delenv("CLSTM_DEBUG", raising=False)
    world = 4
    mp.spawn(growth_worker, args=(world, _port(39000), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        caps = [int(c) for c in open(tmp_path / ("caps_%d.txt" % r)).read().split()]
        assert caps[0] == 1 << 20 and caps[1] >= BIG_NPARAMS and caps[2] == caps[1], caps
        for i in range(3):
            assert np.load(tmp_path / ("params_%d_%d.npy" % (i, r))).tobytes() == np.load(tmp_path / ("params_%d_0.npy" % i)).tobytes()
    assert _counts(tmp_path, world) == [(6, 2)] * world      # six fused exchanges per rank process, the two of the big net two-phase


@pytest.mark.gpu
def test_gpu_cpp_driver_two_phase_saves_the_same_model(tmp_path):
    """clstmocrtrain ngpu=2 on one GPU (test_cpp_driver_ngpu2_two_rank_processes_on_one_gpu) with CLSTM_DEBUG=peer_two_phase=2:
    the saved model is byte-equal to the same run without the option"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])
    exe = os.path.join(ROOT, "clstm_amd", "bin", "clstmocrtrain")
    lst = _driver_fixture(tmp_path)
    models = {}
    for tag, opt in (("a", None), ("b", "peer_two_phase=2")):
        env = dict(os.environ, ngpu="2", batch="2", ntrain="40", nhidden="20", lrate="1e-2", report_every="10", save_every="1000",
                   save_name=str(tmp_path / tag), HSA_ENABLE_IPC_MODE_LEGACY="0", CLSTM_NGPU_SHARE_DEVICE="1", CLSTM_COMM_NO_RCCL="1",
                   CLSTM_REPLICA_CHECK_EVERY="1")
        env.pop("CLSTM_DEBUG", None)
        if opt:
            env["CLSTM_DEBUG"] = opt
        r = subprocess.run([exe, str(lst)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
        models[tag] = open(tmp_path / ("%s-38.clstm" % tag), "rb").read()
    assert len(models["a"]) > 0 and models["a"] == models["b"]
