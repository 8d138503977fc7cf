"""gpu_prep=1 in the drop-in tools: `clstmocr` and `clstmocrtrain` with CenterNormalizer on the device (clstm_normalizer_run_h) must
print and write, byte for byte, what they print and write with the host normaliser (gpu_prep=0, the default).  Both sides of every
comparison set CLSTM_OVERLAP=0 (the fused launches off: with them the training loop itself is not reproducible to the last decode,
see tests/test_predict_host.py).  24 rendered lines, a few dozen updates; every subprocess has a timeout."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "clstm_amd", "bin")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

N_LINES, BATCH, UPDATES = 24, 8, 36


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from make_corpus import make_corpus
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"], timeout=900)
    d = str(tmp_path_factory.mktemp("normalize_host"))
    names, _ = make_corpus(d, n=N_LINES, seed=2)
    return d, names


def train(d, gpu_prep):
    tag = "_g%d" % gpu_prep
    env = dict(os.environ, batch=str(BATCH), test_batch=str(BATCH), ntrain=str(BATCH * UPDATES), lrate="1e-3", nhidden="20", seed="0.222",
               gpu_prep=str(gpu_prep), CLSTM_OVERLAP="0", save_name=os.path.join(d, tag), save_every="100000000",
               report_every=str(BATCH * 6), test_every=str(BATCH * 12))
    lst = os.path.join(d, "list.txt")
    r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), lst, lst], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    models = sorted(glob.glob(os.path.join(d, tag + "-*.clstm")))
    assert len(models) == 1, (models, r.stdout[-2000:])
    return r.stdout.replace(tag, "_g"), models[0]


@pytest.fixture(scope="module")
def trained(corpus):
    d, names = corpus
    return {g: train(d, g) for g in (0, 1)}


@pytest.mark.gpu
def test_clstmocrtrain_gpu_prep_prints_and_saves_the_same(trained):
    (out0, model0), (out1, model1) = trained[0], trained[1]
    assert out0.count("ERROR ") >= 2 and out0.count("TRU ") >= 3, out0[-2000:]
    assert out1 == out0
    assert open(model1, "rb").read() == open(model0, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [0, 1])
def test_clstmocr_gpu_prep_prints_the_same(corpus, trained, conf):
    d, names = corpus
    outs = []
    for gpu_prep in (0, 1):
        env = dict(os.environ, load=trained[0][1], batch="16", gpu_prep=str(gpu_prep), conf=str(conf), save_text="0", CLSTM_OVERLAP="0")
        r = subprocess.run([os.path.join(BIN, "clstmocr"), os.path.join(d, "list.txt")], env=env, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0].count(b"\n") >= len(names)
    assert outs[1] == outs[0]
