"""What one training step launches, by the library's own account: the exact increase of EVERY path counter
(clstm_debug_path_count, include/clstm_abi.h) and of the overlapped-launch count (clstm_net_overlap_stats) over one
clstm_net_train_step, for one small net per backward plan of Net::backward (clstm_amd/csrc/net.inc: backward_family, the
per-layer plan, the weight-gradient forms).  The expected numbers are those of the commit BEFORE the backward scheduler was
restated (713e76c), recorded on each backend: the host emulator has 16 CUs and no batched-MFMA kernels, so the persistent
recurrences of the 136-cell layers (nine cell tiles: 72 workgroups) and case 8 exist on the GPU only.  A change that moves a
number here has changed which kernels a step launches.
What these small nets do NOT reach: the weight gradient and x.d as ONE launch (gemm_dw_dx, counter 14) needs 256 x 256 tiles for
both products -- wide_bf16_c32 takes the bf16-source weight gradient with the bias row outside (4, 13) and x.d as a product of its
own (3); the one-launch branch is covered by test_net_parity.py::test_weight_gradient_and_input_deltas_as_one_launch (BiLSTM(96, 64),
counter 14 asserted on both backends) and the configs[4] tests of test_gpu_e2e.py.  On the emulator the
two 136-cell cases run per-step launches: what they pin there is that no counter moves.
Sizes: those of the parity tests of the same paths (test_states_and_step.py, test_net_parity.py, test_mfma_recurrence.py)."""
import numpy as np
import pytest

from common import synth_lines
from test_net_parity import set_opt, _forget_debug_options, _path_count  # noqa: F401  (autouse fixture)

NCOUNTERS = 26      # indices 0..25 (include/clstm_abi.h)

# id: (ni, nh, nc, T, what to set)        set: precision / overlap / input_deltas / force_wide / opts (dbgopt.h)
T20 = [8 + (5 * i) % 9 for i in range(20)]
CASES = {
    "overlapped_single_layer": (6, [9], 5, [21, 13, 17], dict(overlap=2)),
    "overlapped_stacked": (6, [7, 5], 5, [18, 11], dict(overlap=2)),
    "narrow_bf16_gemms": (8, [10], 7, [12, 7], dict(precision=1)),
    "wide_f32_rec_x3": (12, [136], 6, [12, 1, 8], dict(opts={"rec_x3": 1})),
    "wide_f32_rec_f32": (12, [136], 6, [12, 1, 8], dict(opts={"rec_x3": 0})),
    "wide_bf16_c32": (12, [32, 32], 6, [9, 5, 7, 3], dict(precision=2, force_wide=True)),
    "wide_bf16_c16": (8, [136, 132], 7, [9, 5, 7], dict(precision=2)),
    "overlapped_input_deltas": (6, [9], 5, [21, 13, 17], dict(overlap=2, input_deltas=True)),
    "mfma_bwd_fused": (48, [100], 83, T20, dict(overlap=2, opts={"bwd_mfma": 2, "bwd_mfma_fused": 2})),
    "mfma_bwd_separate": (48, [100], 83, T20, dict(overlap=2, opts={"bwd_mfma": 2, "bwd_mfma_fused": 0})),
}
GPU_ONLY = ("mfma_bwd_fused", "mfma_bwd_separate")      # the batched-MFMA recurrences exist for gfx950 only

# {case: {backend kind: ({counter: increase, all others 0}, overlapped launches)}}
EXPECTED = {
    "overlapped_single_layer": {"emu": ({10: 1}, 1), "hip": ({10: 1}, 1)},
    "overlapped_stacked": {"emu": ({}, 2), "hip": ({}, 2)},
    "narrow_bf16_gemms": {"emu": ({10: 1}, 0), "hip": ({10: 1}, 0)},
    "wide_f32_rec_x3": {"emu": ({}, 0), "hip": ({0: 1, 1: 1, 11: 1}, 0)},
    "wide_f32_rec_f32": {"emu": ({}, 0), "hip": ({0: 1, 1: 1}, 0)},
    "wide_bf16_c32": {"emu": ({0: 2, 1: 2, 3: 1, 4: 1, 6: 1, 9: 2, 13: 1}, 0), "hip": ({0: 2, 1: 2, 3: 1, 4: 1, 6: 1, 9: 2, 13: 1}, 0)},
    "wide_bf16_c16": {"emu": ({}, 0), "hip": ({0: 2, 1: 2, 2: 1}, 0)},
    "overlapped_input_deltas": {"emu": ({10: 1}, 1), "hip": ({10: 1}, 1)},
    "mfma_bwd_fused": {"hip": ({5: 1, 10: 1, 17: 1, 18: 1}, 1)},
    "mfma_bwd_separate": {"hip": ({5: 1, 10: 1, 17: 1}, 1)},
}


def run_step(backend, monkeypatch, case):
    """one clstm_net_train_step of the case's net -> ([increase of counter 0..25], increase of the overlapped-launch count)"""
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    ni, nh, nc, T, cfg = CASES[case]
    if cfg.get("force_wide"):
        monkeypatch.setenv("CLSTM_FORCE_WIDE", "1")
    else:
        monkeypatch.delenv("CLSTM_FORCE_WIDE", raising=False)
    monkeypatch.setenv("CLSTM_XCD_REC", "1")
    backend.lib.call("clstm_debug_set_device_error", 5, 0)      # (a placement failure an earlier test provoked is forgotten)
    for name, value in cfg.get("opts", {}).items():
        set_opt(backend, name, value)
    rng = np.random.default_rng(7)
    wide = max(nh) >= 100
    net = Network(ni, nh, nc, lib=backend.lib)
    net.set_params(init_params(ni, nh, nc, seed=0.222) * (1 if wide else 20))
    net.setLearningRate(1e-4 if wide else 1e-2, 0.9)
    if "precision" in cfg:
        net.set_gemm_precision(cfg["precision"])
    if "overlap" in cfg:
        net.set_overlap(cfg["overlap"])
    if cfg.get("input_deltas"):
        net.enable_input_deltas(True)
    x = backend.up(np.concatenate(synth_lines(rng, T, ni), 0))
    trs = [rng.integers(1, nc, max(1, t // 3)).astype(np.int32) for t in T]
    before = [_path_count(backend, i) for i in range(NCOUNTERS)]
    launches0, _ = net.overlap_stats()
    net.train_step(T, x, trs)
    backend.sync()
    launches, timeouts = net.overlap_stats()
    assert timeouts == 0
    assert np.isfinite(net.get_params()).all()
    return [_path_count(backend, i) - before[i] for i in range(NCOUNTERS)], launches - launches0


def check(backend, monkeypatch, case):
    got, launches = run_step(backend, monkeypatch, case)
    got = {i: n for i, n in enumerate(got) if n}
    print("%s on %s: counters %r, overlapped launches %d" % (case, backend.kind, got, launches))
    want, want_launches = EXPECTED[case][backend.kind]
    assert got == want
    assert launches == want_launches


@pytest.mark.parametrize("case", [c for c in CASES if c not in GPU_ONLY])
def test_one_training_step_launches_what_it_launched_before(backend, monkeypatch, case):
    check(backend, monkeypatch, case)


@pytest.fixture(scope="module")
def hip_backend():
    from common import Backend
    return Backend("hip")


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_ONLY)
def test_one_training_step_on_the_batched_backward_kernels(hip_backend, monkeypatch, case):
    try:
        check(hip_backend, monkeypatch, case)
    finally:
        hip_backend.lib.call("clstm_debug_set_option", None, 0)
