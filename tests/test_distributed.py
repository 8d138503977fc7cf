"""world_size-2 data-parallel step on CPU through the LIBRARY's communicator entry points (clstm_comm_create,
clstm_net_set_comm; the emulator build backs them with a shared-memory all-reduce between the rank processes, the GPU
build with RCCL): the in-library order all-reduce of g -> d += g -> update is what runs, the kernels through the host
emulator; gloo only carries the 128-byte communicator id.  A second case keeps the torch.distributed fallback of
clstm_amd/parallel.py alive.  Checks (a) both ranks end bit-identical, (b) the
result equals the single-process oracle minibatch over ALL lines, including the second step where
the carried momentum (Params.d, clstm_compute.cc:560-563) must NOT be multiplied by the replica
count (the share_deltas artefact, clstm.cc:731-744 / SURVEY.md §8e)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NI, NH, NC = 4, 5, 4
SAT_SHAPE = (4, 5, 5)     # 455 parameters, 455 % 4 == 3: the four-wide loop of k_peer_allreduce_update ends in a partial group


def make_data(step, world=2, shape=None):
    """four lines for two ranks (the original case); world lines + 3 beyond that: uneven shards, every rank owns a line"""
    from common import synth_lines
    ni, _, nc = shape or (NI, NH, NC)
    rng = np.random.default_rng(100 + step)
    T = [5, 3, 4, 6] if world <= 2 else [3 + (7 * i + step) % 4 for i in range(world + 3)]
    lines = synth_lines(rng, T, ni)
    trs = [rng.integers(1, nc, 2).astype(np.int32) for _ in T]
    return lines, trs


def oracle_after(ora32, nsteps, world, shape=None, clip=None, shares=None):
    """clip: the oracle's gradient clip (None: its default of 100); shares (a list): takes, per step, the share of the entries of
    derivs (carried momentum + minibatch gradient) that lie beyond the clip before update() clamps them"""
    from clstm_amd.init import init_params
    from oracle.oracle import OracleNet
    ni, nh, nc = shape or (NI, NH, NC)
    ref = OracleNet(ora32, ni, nh, nc, init=False)
    ref.set_params(init_params(ni, nh, nc, seed=0.222) * 30)
    ref.set_lr(5e-2, 0.9)
    if clip is not None:
        ref.set_gradient_clip(clip)
    for step in range(nsteps):
        lines, trs = make_data(step, world, shape)
        for x, t in zip(lines, trs):
            ref.set_inputs(x); ref.forward(); ref.ctc_deltas(t); ref.backward()
        if shares is not None:
            shares.append(float((np.abs(ref.get_derivs()) > (100.0 if clip is None else clip)).mean()))
        ref.update()
    return ref


def worker(rank, world, port, outdir, use_lib_comm, slow_rank0_s=0.0, sabotage=False, clip=None, derivs0=None, shape=None):
    """clip: clstm_net_set_gradient_clip (None: the library's default); derivs0 "pm200": the derivs are preloaded with +-200 before
    EVERY step and parameters / derivs / gradient around every step are saved for the exact check; shape: (ni, nh, nc)"""
    ni, nh, nc = shape or (NI, NH, NC)
    if slow_rank0_s:
        os.environ["CLSTM_PEER_TIMEOUT_S"] = "1"      # far below the time rank 0 stays away: the HOST wait must cover it
    os.environ["CLSTM_REPLICA_CHECK_EVERY"] = "1" if use_lib_comm else "0"
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    from clstm_amd.parallel import Trainer, shard
    from common import emu_lib
    lib = emu_lib()
    p0 = init_params(ni, nh, nc, seed=0.222) * 30
    params = torch.from_numpy(p0.copy())
    derivs = torch.zeros_like(params)
    grads = torch.zeros_like(params)
    net = Network(ni, nh, nc, lib=lib, params=params, derivs=derivs, grads=grads)
    net.params_changed()
    net.setLearningRate(5e-2, 0.9)
    if clip is not None:
        net.set_gradient_clip(clip)
    if use_lib_comm:
        from clstm_amd.net import Comm

        def exchange(ident):
            box = [ident]
            dist.broadcast_object_list(box, src=0)
            return box[0]
        comm = Comm(rank, world, exchange, lib=lib)
        assert lib.call("clstm_comm_size", comm.h) == world and lib.call("clstm_comm_rank", comm.h) == rank
        tr = Trainer(net, comm=comm)
        assert tr.dist is None            # nothing goes through torch.distributed in the step
    else:
        tr = Trainer(net, grads_tensor=grads)
        assert tr.world_size() == world
    import ctypes
    import time
    for step in range(2):
        lines, trs = make_data(step, world, shape)
        if derivs0 == "pm200":
            from common import pm200
            derivs.copy_(torch.from_numpy(pm200(derivs.numel())))
            np.save(os.path.join(outdir, "v0_%d_%d.npy" % (step, rank)), params.numpy())
        if slow_rank0_s and rank == 0 and step == 1:
            time.sleep(slow_rank0_s)       # clstmocrtrain's rank 0 in its test / save phase: the others are already at the next exchange
        if sabotage and rank == world - 1 and step == 1:
            params.view(-1)[3] += 1e-3     # one replica's parameters silently change (what a skipped update / a bit flip leaves)
            net.params_changed()
        if use_lib_comm == "one_call":    # clstm_net_train_step: the peer-read all-reduce fused into the update
            mine_l, mine_t = shard(lines, rank, world), shard(trs, rank, world)
            net.train_step([len(l) for l in mine_l], np.ascontiguousarray(np.concatenate(mine_l, 0), np.float32), mine_t)
        else:
            tr.train(shard(lines, rank, world), shard(trs, rank, world))
        if derivs0 == "pm200":
            lib.call("clstm_synchronize")
            for name, t in (("v1", params), ("d1", derivs), ("g", grads)):
                np.save(os.path.join(outdir, "%s_%d_%d.npy" % (name, step, rank)), t.numpy())
    if sabotage:                          # every rank must be told, with the step number
        try:
            lib.call("clstm_synchronize")
            verdict = "no error"
        except Exception as e:            # noqa: BLE001
            verdict = str(e)
        open(os.path.join(outdir, "verdict_%d.txt" % rank), "w").write(verdict)
    if use_lib_comm == "one_call":
        cnt = ctypes.c_longlong(0)
        lib.call("clstm_debug_path_count", 7, ctypes.byref(cnt))
        assert cnt.value == 2, "the fused peer-read all-reduce + update did not run (%d)" % cnt.value
    if use_lib_comm and not sabotage:
        cnt = ctypes.c_longlong(0)
        lib.call("clstm_debug_path_count", 12, ctypes.byref(cnt))
        assert cnt.value == 2, "the replica check did not run after every update (%d)" % cnt.value
        lib.call("clstm_synchronize")     # ... and found the replicas identical (a mismatch would raise here)
    np.save(os.path.join(outdir, "params_%d.npy" % rank), params.numpy())
    np.save(os.path.join(outdir, "derivs_%d.npy" % rank), derivs.numpy())
    if use_lib_comm:
        net.set_comm(None)
        comm.close()
    dist.destroy_process_group()


def _port(base):
    _port.n = getattr(_port, "n", 0) + 1
    return base + (os.getpid() % 1500) + 13 * _port.n


def _check_replicas_and_oracle(tmp_path, ora32, world, what, ref=None):
    """ref: the oracle net to compare with (default: oracle_after two steps at the module's shape and the default clip)"""
    from common import assert_close
    p = [np.load(tmp_path / ("params_%d.npy" % r)) for r in range(world)]
    d = [np.load(tmp_path / ("derivs_%d.npy" % r)) for r in range(world)]
    for r in range(1, world):
        assert np.array_equal(p[0], p[r]) and np.array_equal(d[0], d[r]), "rank %d differs from rank 0" % r    # replicas stay identical
    if ref is None:
        ref = oracle_after(ora32, 2, world)
    # (the minibatch gradient is summed shard by shard, then over ranks in rank order: with more shards the float32 sum is
    #  grouped differently from the oracle's line-by-line accumulation -- lr x 1e-5 of a gradient entry of order 1)
    assert_close(p[0], ref.get_params(), rtol=2e-5, atol=2e-7 if world <= 2 else 1e-6, what="params after 2 DP steps, " + what)
    assert_close(d[0], ref.get_derivs(), rtol=1e-4, atol=1e-9, scale_atol=2e-4, what="momentum buffer after 2 DP steps, " + what)


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("use_lib_comm", [True, "one_call", False], ids=["library_communicator", "library_communicator_one_call_peer_allreduce", "torch_distributed_fallback"])
def test_two_rank_data_parallel_matches_single_process(tmp_path, ora32, use_lib_comm, world):
    """(the name is historical: world sizes 2, 4 and 8 -- VERDICT r4 'Missing 2': PEER_MAX_RANKS is 16, k_peer_barrier uses one
    lane per rank, the rendezvous counts to nranks, and none of it had seen more than two)"""
    import torch.multiprocessing as mp
    from common import emu_lib
    if world > 2 and use_lib_comm is False:
        pytest.skip("the torch.distributed fallback has no world-size-dependent code of its own")
    emu_lib()                                   # build once, before the workers race for it
    mp.spawn(worker, args=(world, _port(29500), str(tmp_path), use_lib_comm), nprocs=world, join=True)
    _check_replicas_and_oracle(tmp_path, ora32, world, "%d ranks" % world)


def test_slow_rank_does_not_trip_the_device_barrier(tmp_path, ora32):
    """ADVICE r4 (medium) / VERDICT r4 weak 7: in clstmocrtrain ngpu=N only rank 0 runs the test set and saves while the others
    are already at the next step's exchange.  The device-side barrier used to give up after 2^24 polls and every later update
    was skipped.  Now the HOSTS announce an exchange to each other before any of them enqueues the device barrier
    (Comm::peer_barrier): rank 0 stays away for far longer than the device time-out (forced down to 1 s here) and the run
    must still end with identical replicas that match the oracle."""
    import torch.multiprocessing as mp
    from common import emu_lib
    emu_lib()
    mp.spawn(worker, args=(2, _port(27500), str(tmp_path), "one_call", 6.0), nprocs=2, join=True)
    _check_replicas_and_oracle(tmp_path, ora32, 2, "rank 0 late by 6 s")


@pytest.mark.parametrize("use_lib_comm", [True, "one_call"], ids=["separate_calls", "one_call_peer_allreduce"])
def test_replica_check_reports_a_diverged_rank(tmp_path, use_lib_comm):
    """VERDICT r4 'Missing 2': nothing ever compared the replicas.  One of four ranks has a parameter changed behind the
    library's back before the second step: the check that follows that step's update (CLSTM_REPLICA_CHECK_EVERY=1) must make
    EVERY rank's next synchronisation fail with the step number (reference: distribute_weights re-syncs, clstm.cc:718-729)."""
    import torch.multiprocessing as mp
    from common import emu_lib
    emu_lib()
    world = 4
    mp.spawn(worker, args=(world, _port(26000), str(tmp_path), use_lib_comm, 0.0, True), nprocs=world, join=True)
    verdicts = [open(tmp_path / ("verdict_%d.txt" % r)).read() for r in range(world)]
    told = [("replicas diverged" in v and "training step 2" in v) for v in verdicts]
    # sum == nranks * own fails on every rank whose checksum differs from the mean: with one odd rank out of four, all of them
    assert all(told), verdicts


def _check_pm200(outdir, world, what, lr=5e-2, mom=0.9):
    """common.assert_every_entry_once (the exact check of tests/test_update_rule.py (b)) on what worker(derivs0="pm200") saved:
    with derivs of +-200, a summed gradient below 100 and the default clip of 100, every entry of derivs ends at +-f32(100 mom)
    and every parameter moves by +-100 lr -- whatever the number of ranks, because the gradient drops out.  Both steps, every rank."""
    from common import assert_every_entry_once, pm200
    for step in range(2):
        for r in range(world):
            v0, v1, d1, g = (np.load(os.path.join(outdir, "%s_%d_%d.npy" % (n, step, r))) for n in ("v0", "v1", "d1", "g"))
            assert_every_entry_once(v0, pm200(v0.size), g, v1, d1, lr, mom, "%s, step %d rank %d" % (what, step, r))
            if r:
                assert np.array_equal(g, g0) and np.array_equal(v1, v10), "rank %d differs from rank 0" % r
            else:
                g0, v10 = g, v1


def _saturating_clip(ora32, world, shape):
    """a clip that bites in a two-step run from zero derivs: the median of |derivs| the oracle holds before its first update.
    Returns it with the oracle after two steps under it; the share of entries beyond it is asserted for both steps."""
    from oracle.oracle import OracleNet
    from clstm_amd.init import init_params
    ni, nh, nc = shape
    first = OracleNet(ora32, ni, nh, nc, init=False)
    first.set_params(init_params(ni, nh, nc, seed=0.222) * 30)
    lines, trs = make_data(0, world, shape)
    for x, t in zip(lines, trs):
        first.set_inputs(x); first.forward(); first.ctc_deltas(t); first.backward()
    clip = float(np.median(np.abs(first.get_derivs())))
    shares = []
    ref = oracle_after(ora32, 2, world, shape, clip, shares)
    assert clip > 0 and all(0.1 <= s <= 0.9 for s in shares), "inconclusive: clip %g, shares beyond it %r" % (clip, shares)
    return clip, ref


@pytest.mark.parametrize("use_lib_comm,world", [(True, 2), (True, 4), ("one_call", 2), ("one_call", 4), (False, 2)],
                         ids=["library_communicator-2", "library_communicator-4", "one_call_peer_allreduce-2", "one_call_peer_allreduce-4",
                              "torch_distributed_fallback-2"])
def test_data_parallel_update_where_the_clip_saturates(tmp_path, ora32, use_lib_comm, world):
    """The update behind an exchange -- all-reduce then k_update (library communicator, torch fallback), or k_peer_allreduce_update
    (one call; the worker holds path count 7 to the number of steps) -- where the clamp is not the identity, on a net of 455
    parameters (455 % 4 == 3: the four-wide loop ends in a partial group and its last load reaches past the end of the buffer).
    (1) derivs of +-200: exact, see _check_pm200.  (2) two steps from zero derivs under a clip at the median of the first step's
    gradient, against the oracle with the same clip: tolerances of _check_replicas_and_oracle, replicas bit-identical."""
    import torch.multiprocessing as mp
    from common import emu_lib
    emu_lib()
    what = "%d ranks, %s" % (world, use_lib_comm)
    (tmp_path / "pm200").mkdir()
    mp.spawn(worker, args=(world, _port(24000), str(tmp_path / "pm200"), use_lib_comm, 0.0, False, None, "pm200", SAT_SHAPE), nprocs=world, join=True)
    _check_pm200(str(tmp_path / "pm200"), world, what)
    clip, ref = _saturating_clip(ora32, world, SAT_SHAPE)
    (tmp_path / "sat").mkdir()
    mp.spawn(worker, args=(world, _port(24000), str(tmp_path / "sat"), use_lib_comm, 0.0, False, clip, None, SAT_SHAPE), nprocs=world, join=True)
    _check_replicas_and_oracle(tmp_path / "sat", ora32, world, "clip %g, %s" % (clip, what), ref=ref)


def test_shard_covers_everything():
    from clstm_amd.parallel import shard
    items = list(range(11))
    for world in (1, 2, 3, 4, 8):
        parts = [shard(items, r, world) for r in range(world)]
        assert sum(parts, []) == items
        assert min(len(p) for p in parts) >= 1 and max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    # n = 5, world = 4 used to leave rank 3 empty (-> "empty batch" on that rank while the others wait in the all-reduce)
    assert [len(shard(list(range(5)), r, 4)) for r in range(4)] == [2, 1, 1, 1]
    import pytest
    with pytest.raises(ValueError):
        shard([1, 2], 0, 4)


def gpu_worker(rank, world, port, outdir, share_device=False, one_call=False, slow_rank0_s=0.0, clip=None, derivs0=None, shape=None):
    """one rank per GPU: the library's RCCL communicator (clstm_comm_create + clstm_net_set_comm), gloo for the id.
    share_device: every rank on GPU 0 with a communicator WITHOUT RCCL (CLSTM_COMM_NO_RCCL=1: RCCL refuses duplicate GPUs) --
    the exchange is the peer-read path over HIP IPC mappings alone.  one_call: clstm_net_train_step (the fused path).
    clip / derivs0 / shape: as in worker()."""
    ni, nh, nc = shape or (NI, NH, NC)
    if share_device:
        os.environ["CLSTM_COMM_NO_RCCL"] = "1"
    if slow_rank0_s:
        os.environ["CLSTM_PEER_TIMEOUT_S"] = "5"
    os.environ["CLSTM_REPLICA_CHECK_EVERY"] = "1"
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0 if share_device else rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clstm_amd import abi
    from clstm_amd.init import init_params
    from clstm_amd.net import Comm, Network
    from clstm_amd.parallel import Trainer, shard
    lib = abi.load()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    lib.call("clstm_set_stream", stream.cuda_stream)
    dev = torch.device("cuda", 0 if share_device else rank)
    p0 = init_params(ni, nh, nc, seed=0.222) * 30
    params = torch.from_numpy(p0.copy()).to(dev)
    derivs = torch.zeros_like(params)
    grads = torch.zeros_like(params)
    net = Network(ni, nh, nc, lib=lib, params=params, derivs=derivs, grads=grads)
    net.params_changed()
    net.setLearningRate(5e-2, 0.9)
    if clip is not None:
        net.set_gradient_clip(clip)

    def exchange(ident):
        box = [ident]
        dist.broadcast_object_list(box, src=0)
        return box[0]
    comm = Comm(rank, world, exchange, lib=lib)
    tr = Trainer(net, comm=comm)
    import ctypes
    import time
    for step in range(2):
        lines, trs = make_data(step, world, shape)
        mine_l, mine_t = shard(lines, rank, world), shard(trs, rank, world)
        if derivs0 == "pm200":
            from common import pm200
            lib.call("clstm_synchronize")
            derivs.copy_(torch.from_numpy(pm200(derivs.numel())).to(dev))
            torch.cuda.current_stream().synchronize()
            np.save(os.path.join(outdir, "v0_%d_%d.npy" % (step, rank)), params.cpu().numpy())
        if slow_rank0_s and rank == 0 and step == 1:
            time.sleep(slow_rank0_s)
        if one_call:
            x = torch.from_numpy(np.ascontiguousarray(np.concatenate(mine_l, 0), np.float32)).to(dev)
            net.train_step([len(l) for l in mine_l], x, mine_t)
        else:
            tr.train(mine_l, mine_t)
        if derivs0 == "pm200":
            lib.call("clstm_synchronize")
            for name, t in (("v1", params), ("d1", derivs), ("g", grads)):
                np.save(os.path.join(outdir, "%s_%d_%d.npy" % (name, step, rank)), t.cpu().numpy())
    lib.call("clstm_synchronize")         # (also the verdict of the replica checks that followed both updates)
    if one_call:
        cnt = ctypes.c_longlong(0)
        lib.call("clstm_debug_path_count", 7, ctypes.byref(cnt))
        open(os.path.join(outdir, "peer_%d.txt" % rank), "w").write(str(cnt.value))
    cnt = ctypes.c_longlong(0)
    lib.call("clstm_debug_path_count", 12, ctypes.byref(cnt))
    assert cnt.value == 2, "the replica check did not run after every update (%d)" % cnt.value
    np.save(os.path.join(outdir, "params_%d.npy" % rank), params.cpu().numpy())
    np.save(os.path.join(outdir, "derivs_%d.npy" % rank), derivs.cpu().numpy())
    net.set_comm(None)
    comm.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_gpus_library_communicator_matches_single_process(tmp_path, ora32):
    """The same two-rank step on two MI355X through RCCL inside the library (ncclCommInitRank from clstm_comm_create,
    ncclAllReduce on the library stream in front of k_update): replicas bit-identical, result = the oracle's
    single-process minibatch.  Skips on a one-GPU box; lights up by itself where the driver has several."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (this box has %d)" % torch.cuda.device_count())
    import torch.multiprocessing as mp
    mp.spawn(gpu_worker, args=(2, _port(31500), str(tmp_path)), nprocs=2, join=True)
    _check_replicas_and_oracle(tmp_path, ora32, 2, "2 GPUs")


@pytest.mark.gpu
@pytest.mark.parametrize("world", [4, 8])
def test_all_gpus_one_call_step_matches_single_process(tmp_path, ora32, world):
    """world ranks on world GPUs through clstm_net_train_step (RCCL communicator + the peer-read exchange where the ranks can
    map each other): skips unless the box has that many GPUs."""
    import torch
    if torch.cuda.device_count() < world:
        pytest.skip("needs %d GPUs (this box has %d)" % (world, torch.cuda.device_count()))
    import torch.multiprocessing as mp
    mp.spawn(gpu_worker, args=(world, _port(30500), str(tmp_path), False, True), nprocs=world, join=True)
    _check_replicas_and_oracle(tmp_path, ora32, world, "%d GPUs" % world)


@pytest.mark.gpu
@pytest.mark.parametrize("world,one_call", [(2, True), (2, False), (4, True), (8, True), (8, False)],
                         ids=["2_train_step_fused_update", "2_separate_calls_plain_allreduce", "4_train_step_fused_update",
                              "8_train_step_fused_update", "8_separate_calls_plain_allreduce"])
def test_two_processes_on_one_gpu_peer_read_allreduce(tmp_path, ora32, world, one_call):
    """VERDICT r3 'Missing 3' / r4 'Missing 2': the one-shot peer-read all-reduce (each rank maps the others' fresh-gradient
    buffers through HIP IPC, a flag handshake replaces ncclAllReduce, the sum is formed in rank order inside the update kernel)
    exercised on ONE GPU with 2, 4 and 8 rank processes that share device 0 (a communicator without RCCL, which refuses
    duplicate GPUs).  Replicas bit-identical, result = the oracle's single-process minibatch; in the one-call form the fused
    kernel must have run twice; the replica check runs after every update."""
    import torch.multiprocessing as mp
    mp.spawn(gpu_worker, args=(world, _port(33500), str(tmp_path), True, one_call), nprocs=world, join=True)
    if one_call:
        assert [open(tmp_path / ("peer_%d.txt" % r)).read() for r in range(world)] == ["2"] * world
    _check_replicas_and_oracle(tmp_path, ora32, world, "%d processes on one GPU" % world)


@pytest.mark.gpu
@pytest.mark.parametrize("one_call", [True, False], ids=["train_step_fused_update", "separate_calls_plain_allreduce"])
def test_two_processes_on_one_gpu_update_where_the_clip_saturates(tmp_path, ora32, one_call):
    """test_data_parallel_update_where_the_clip_saturates on the MI355X: two rank processes on device 0, the peer-read exchange
    over HIP IPC, 455 parameters.  Which clamp each mode covers: in the one-call form (clstm_net_train_step) k_peer_allreduce_update
    sums the ranks' gradients AND applies the update, so the clamp under test is its own, partial last group included (path count 7
    is held to the number of steps).  With separate calls the same kernel runs only as the plain all-reduce (no parameters handed
    to it, nothing clamped there), and the clamp under test is k_update's, on the sum that all-reduce left."""
    import torch.multiprocessing as mp
    what = "2 processes on one GPU, one_call=%s" % one_call
    (tmp_path / "pm200").mkdir()
    mp.spawn(gpu_worker, args=(2, _port(35500), str(tmp_path / "pm200"), True, one_call, 0.0, None, "pm200", SAT_SHAPE), nprocs=2, join=True)
    if one_call:
        assert [open(tmp_path / "pm200" / ("peer_%d.txt" % r)).read() for r in range(2)] == ["2"] * 2
    _check_pm200(str(tmp_path / "pm200"), 2, what)
    clip, ref = _saturating_clip(ora32, 2, SAT_SHAPE)
    (tmp_path / "sat").mkdir()
    mp.spawn(gpu_worker, args=(2, _port(35500), str(tmp_path / "sat"), True, one_call, 0.0, clip, None, SAT_SHAPE), nprocs=2, join=True)
    if one_call:
        assert [open(tmp_path / "sat" / ("peer_%d.txt" % r)).read() for r in range(2)] == ["2"] * 2
    _check_replicas_and_oracle(tmp_path / "sat", ora32, 2, "clip %g, %s" % (clip, what), ref=ref)


@pytest.mark.gpu
def test_rank_30_s_late_on_one_gpu(tmp_path, ora32):
    """rank 0 sleeps 30 s between the steps (clstmocrtrain's test / save phase) while rank 1 is already
    at the next exchange; the device-side barrier's time-out is forced down to 5 s.  The hosts' announce handshake keeps rank 1
    from enqueuing the barrier until rank 0 is there: no time-out, identical replicas, the oracle's result."""
    import torch.multiprocessing as mp
    mp.spawn(gpu_worker, args=(2, _port(34500), str(tmp_path), True, True, 30.0), nprocs=2, join=True)
    _check_replicas_and_oracle(tmp_path, ora32, 2, "rank 0 late by 30 s")


# ---- the C++ driver with ngpu=N: rank processes forked by clstmocrtrain itself ---------------------------------------
def _driver_fixture(tmp_path, n=2):
    """two short text lines cut from the reference's fixture image (so the emulator finishes in seconds)"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    im = Image.open(os.path.join(root, "tests", "golden", "textline.bin.png"))
    names = []
    for i, (x0, x1, gt) in enumerate([(0, 70, "pe"), (60, 150, "rf")][:n]):
        p = tmp_path / ("l%d.bin.png" % i)
        im.crop((x0, 0, x1, im.size[1])).save(p)
        (tmp_path / ("l%d.gt.txt" % i)).write_text(gt + "\n", encoding="utf-8")
        names.append(str(p))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(names) + "\n")
    return lst


def _model_params(tool, path, tmp_path, tag):
    out = tmp_path / ("params_%s.bin" % tag)
    subprocess.run([tool, "params", str(path), str(out)], check=True, capture_output=True)
    return np.fromfile(out, np.float32)


@pytest.mark.parametrize("nranks", [2, 4])
def test_cpp_driver_ngpu2_equals_single_process(tmp_path, nranks):
    """clstmocrtrain ngpu=2 batch=2 (the driver forks a second rank, both join the library communicator through
    clstm_comm_unique_id / clstm_comm_create, every rank trains on its half of each minibatch, update() all-reduces the
    gradient) must leave the model of ngpu=1 batch=2 -- same draws, same summed gradient, two summation orders.
    CPU run: the driver is linked against the host emulator, whose communicator is a shared-memory all-reduce between
    the rank processes (CLSTM_NGPU_SHARE_DEVICE: there is no device to bind)."""
    from common import emu_lib
    emu_lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "clstm_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", os.path.join(root, "clstm_amd", "host"), "-s", "all"])
    emu_dir = os.path.join(root, "tests", "hipemu", "build")
    exe = tmp_path / "clstmocrtrain_emu"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(root, "clstm_amd", "host", "clstmocrtrain.cc"),
                           "-L" + emu_dir, "-lclstm_emu", "-Wl,-rpath," + emu_dir, "-lz", "-pthread"])
    lst = _driver_fixture(tmp_path)
    tool = os.path.join(root, "clstm_amd", "bin", "clstm_hosttool")
    got = {}
    # (nranks = 4, VERDICT r4 next 3(a): minibatches of four lines, one per rank; the replica check after every update)
    for ngpu in (1, nranks):
        env = dict(os.environ, ngpu=str(ngpu), batch=str(nranks), ntrain=str(3 * nranks), nhidden="6", target_height="12", lrate="1e-2",
                   report_every=str(nranks), save_every="1000", save_name=str(tmp_path / ("m%d" % ngpu)), CLSTM_NGPU_SHARE_DEVICE="1",
                   CLSTM_REPLICA_CHECK_EVERY="1")
        r = subprocess.run([str(exe), str(lst)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
        if ngpu > 1:
            assert "ranks %d x 1 lines" % nranks in r.stdout
        assert r.stdout.count("TRU ") == 3, r.stdout          # only rank 0 reports
        model = tmp_path / ("m%d-%d.clstm" % (ngpu, 2 * nranks))
        assert model.exists(), r.stdout[-800:]
        got[ngpu] = _model_params(tool, model, tmp_path, str(ngpu))
    assert got[1].size == got[nranks].size and np.abs(got[1]).max() > 0
    assert np.allclose(got[1], got[nranks], rtol=1e-5, atol=1e-7), np.abs(got[1] - got[nranks]).max()


@pytest.mark.gpu
def test_cpp_driver_ngpu2_on_two_gpus(tmp_path):
    """the same through RCCL on a box with two GPUs (skips on one)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "clstm_amd", "host"), "-s", "all"])
    exe = os.path.join(root, "clstm_amd", "bin", "clstmocrtrain")
    tool = os.path.join(root, "clstm_amd", "bin", "clstm_hosttool")
    lst = _driver_fixture(tmp_path)
    got = {}
    for ngpu in (1, 2):
        env = dict(os.environ, ngpu=str(ngpu), batch="2", ntrain="40", nhidden="20", lrate="1e-2", report_every="10",
                   save_every="1000", save_name=str(tmp_path / ("g%d" % ngpu)), HSA_ENABLE_IPC_MODE_LEGACY="0")
        r = subprocess.run([exe, str(lst)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
        got[ngpu] = _model_params(tool, tmp_path / ("g%d-38.clstm" % ngpu), tmp_path, "g%d" % ngpu)
    assert np.allclose(got[1], got[2], rtol=1e-4, atol=1e-6), np.abs(got[1] - got[2]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("nranks", [2, 4])
def test_cpp_driver_ngpu2_two_rank_processes_on_one_gpu(tmp_path, nranks):
    """clstmocrtrain ngpu=2 on a ONE-GPU box: both rank processes bind device 0 (CLSTM_NGPU_SHARE_DEVICE), the communicator
    carries no RCCL (CLSTM_COMM_NO_RCCL=1) and every update goes through the one-shot peer-read all-reduce over HIP IPC
    mappings (clstm_net_train_step_h / clstm_net_update); the model must equal ngpu=1 batch=2 up to the summation order."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "clstm_amd", "host"), "-s", "all"])
    exe = os.path.join(root, "clstm_amd", "bin", "clstmocrtrain")
    tool = os.path.join(root, "clstm_amd", "bin", "clstm_hosttool")
    lst = _driver_fixture(tmp_path)
    got = {}
    for ngpu in (1, nranks):
        env = dict(os.environ, ngpu=str(ngpu), batch=str(nranks), ntrain=str(20 * nranks), nhidden="20", lrate="1e-2", report_every=str(5 * nranks),
                   save_every="1000", save_name=str(tmp_path / ("s%d" % ngpu)), HSA_ENABLE_IPC_MODE_LEGACY="0",
                   CLSTM_NGPU_SHARE_DEVICE="1", CLSTM_COMM_NO_RCCL="1", CLSTM_REPLICA_CHECK_EVERY="1")
        r = subprocess.run([exe, str(lst)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
        got[ngpu] = _model_params(tool, tmp_path / ("s%d-%d.clstm" % (ngpu, 19 * nranks)), tmp_path, "s%d" % ngpu)
    assert np.abs(got[1]).max() > 0 and np.allclose(got[1], got[nranks], rtol=1e-4, atol=1e-6), np.abs(got[1] - got[nranks]).max()


def test_shard_by_length_balances_the_longest_lines():
    """VERDICT r3 #3b: the deal is a partition, every rank gets n // world (+1) lines, and the ranks' longest lines are
    neighbours in the sorted order (equal +-1 position), for ragged lengths U{150..250} and for ties."""
    from clstm_amd.parallel import shard_by_length
    rng = np.random.default_rng(3)
    for world in (2, 4, 8):
        for n in (world, 64, 67):
            T = [int(t) for t in rng.integers(150, 251, n)]
            parts = [shard_by_length(T, r, world) for r in range(world)]
            assert sorted(i for p in parts for i in p) == list(range(n))
            assert {len(p) for p in parts} <= {n // world, n // world + 1}
            srt = sorted(T, reverse=True)
            for r, p in enumerate(parts):
                assert max(T[i] for i in p) == srt[r]            # rank r's longest line is the r-th longest of the minibatch
                assert p == sorted(p)
    assert [shard_by_length([5, 5, 5, 5], r, 2) for r in range(2)] == [[0, 2], [1, 3]]   # ties keep their order
    with pytest.raises(ValueError):
        shard_by_length([1, 2], 0, 4)
