"""degrade=1 in `clstmocrtrain`: every visit of a training line is degraded afresh on the device (CLSTMOCR::set_degrade: clstm_degrader_run_h
in front of clstm_normalizer_run_d).  The driver is linked against the host emulator for the CPU suite and is the real one under gpu.
Four short lines cut from the fixture image, four updates of four lines; every subprocess has a timeout."""
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO_RANGES = dict(degrade_angle="0", degrade_scale="0", degrade_aniso="0", degrade_translate="0", degrade_sigma="0,0", degrade_maxdelta="0,0",
                   degrade_blur="0,0")


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def driver(request, tmp_path_factory):
    """-> (clstmocrtrain, directory with list.txt)"""
    from PIL import Image
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "csrc"), "-s", "all"], timeout=1800)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"], timeout=900)
    d = tmp_path_factory.mktemp("degrade_host_" + request.param)
    exe = os.path.join(ROOT, "clstm_amd", "bin", "clstmocrtrain")
    if request.param == "emu":
        from common import emu_lib
        emu_lib()
        emu_dir = os.path.join(ROOT, "tests", "hipemu", "build")
        exe = str(d / "clstmocrtrain_emu")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "clstm_amd", "host", "clstmocrtrain.cc"),
                               "-L" + emu_dir, "-lclstm_emu", "-Wl,-rpath," + emu_dir, "-lz", "-pthread"], timeout=900)
    im = Image.open(os.path.join(ROOT, "tests", "golden", "textline.bin.png"))
    names = []
    for i, (x0, x1, gt) in enumerate([(0, 70, "pe"), (60, 150, "rf"), (140, 230, "or"), (220, 300, "me")]):
        p = d / ("l%d.bin.png" % i)
        im.crop((x0, 0, x1, im.size[1])).save(p)
        (d / ("l%d.gt.txt" % i)).write_text(gt + "\n", encoding="utf-8")
        names.append(str(p))
    (d / "list.txt").write_text("\n".join(names) + "\n")
    return exe, str(d)


_RUNS = {}


def train(driver, tag, expect_ok=True, **opts):
    """one run of `clstmocrtrain batch=4 ntrain=16` -> (stdout with the run's own name taken out, bytes of the saved model, stderr);
    run once per tag"""
    exe, d = driver
    if (exe, tag) not in _RUNS:
        env = dict(os.environ, batch="4", ntrain="16", lrate="1e-2", nhidden="6", seed="0.222", CLSTM_OVERLAP="0", save_name=os.path.join(d, tag),
                   save_every="100000000", report_every="4", test_every="100000000")
        env.update(opts)
        lst = os.path.join(d, "list.txt")
        r = subprocess.run([exe, lst], env=env, capture_output=True, text=True, timeout=600)
        if not expect_ok:
            return r
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
        models = sorted(glob.glob(os.path.join(d, tag + "-*.clstm")))
        assert len(models) == 1, (models, r.stdout[-2000:])
        _RUNS[(exe, tag)] = (r.stdout.replace(tag, "_run"), open(models[0], "rb").read(), r.stderr)
    return _RUNS[(exe, tag)]


def test_same_seed_prints_and_saves_the_same(driver):
    a = train(driver, "s3a", degrade="1", degrade_seed="3")
    b = train(driver, "s3b", degrade="1", degrade_seed="3")
    assert a[0].count("TRU ") == 4 and "saving" in a[0], a[0][-2000:]
    assert a[0] == b[0] and a[1] == b[1]


def test_another_seed_saves_another_model(driver):
    a = train(driver, "s3a", degrade="1", degrade_seed="3")
    c = train(driver, "s4", degrade="1", degrade_seed="4")
    assert a[1] != c[1]
    assert a[1] != train(driver, "plain", degrade="0", gpu_prep="1")[1]       # ... and degrading changes what is trained on


def test_zero_ranges_save_what_no_degradation_saves(driver):
    z = train(driver, "zero", degrade="1", degrade_seed="3", **ZERO_RANGES)
    p = train(driver, "plain", degrade="0", gpu_prep="1")
    assert z[0] == p[0] and z[1] == p[1]


def test_degrade_without_gpu_prep_is_refused_by_name(driver):
    r = train(driver, "refused", expect_ok=False, degrade="1", gpu_prep="0")
    assert r.returncode != 0 and "degrade=1 gpu_prep=0" in r.stderr, r.stderr[-2000:]
    assert not glob.glob(os.path.join(driver[1], "refused-*.clstm"))
    r = train(driver, "refused1", expect_ok=False, degrade="1", batch="1")
    assert r.returncode != 0 and "degrade=1 needs batch > 1" in r.stderr, r.stderr[-2000:]
    r = train(driver, "refused2", expect_ok=False, degrade="1", degrade_sigma="3,2")
    assert r.returncode != 0 and "LO <= HI" in r.stderr, r.stderr[-2000:]


def test_two_ranks_stay_replicas(driver):
    """ngpu=2 on one device: every rank draws the same keys and visits from the lrand48 sequence the ranks share; the replica check after
    every update finds the ranks' parameters equal"""
    out, model, err = train(driver, "two", degrade="1", degrade_seed="3", ngpu="2", CLSTM_NGPU_SHARE_DEVICE="1", CLSTM_COMM_NO_RCCL="1",
                            CLSTM_REPLICA_CHECK_EVERY="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    assert "ranks 2 x 2 lines" in out and out.count("TRU ") == 4
    assert "diverged" not in err and "replica" not in err.lower(), err[-2000:]
    # ... and they trained on the lines one process trains on: the same model up to the order in which the gradient is summed (the
    # tolerance of tests/test_distributed.py for the same comparison without degradation)
    one = train(driver, "s3a", degrade="1", degrade_seed="3")[1]
    tool = os.path.join(ROOT, "clstm_amd", "bin", "clstm_hosttool")
    got = []
    for tag, blob in (("one", one), ("two", model)):
        src, dst = os.path.join(driver[1], "cmp_%s.clstm" % tag), os.path.join(driver[1], "cmp_%s.bin" % tag)
        open(src, "wb").write(blob)
        subprocess.run([tool, "params", src, dst], check=True, capture_output=True, timeout=60)
        got.append(np.fromfile(dst, np.float32))
    assert got[0].size == got[1].size and np.abs(got[0]).max() > 0
    assert np.allclose(got[0], got[1], rtol=1e-4, atol=1e-6), np.abs(got[0] - got[1]).max()
