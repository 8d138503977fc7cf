"""Line degradation on the device (clstm_degrader_*, clstm_amd/csrc/degrade.h): raw line images in, degraded images of the same
sizes out.  The acceptance property is identity with degrade_line of clstm_amd/host/degrade.h: the referee everywhere is
`clstm_hosttool degrade-raw`, one image at a time, and images are compared AS BYTES.  Every case runs on the host emulator (CPU
suite) and, marked gpu, on the MI355X."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from common import synth_labels
from test_normalize_gpu import FIXTURE, TOOL, count, grey, read_raw, same_bytes, write_raw
from test_normalize_gpu import referee as normalize_referee

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEGRADED = 33        # clstm_debug_path_count: lines degraded on the device
NORMALIZED = 25
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def build_tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("degrade"))


# ---- parameters ------------------------------------------------------------------------------------------------------------------
def params(m=(1.0, 0.0, 0.0, 1.0), tx=0.0, ty=0.0, sigma=0.0, maxdelta=0.0, blur=0.0, seed=0):
    """a line's parameters as a tuple of float32 values (and the integer seed): the key of the referee's cache"""
    return tuple(F32(v) for v in m) + (F32(tx), F32(ty), F32(sigma), F32(maxdelta), F32(blur), int(seed))


IDENTITY = params()


def as_line(p):
    from clstm_amd.net import degrade_line
    return degrade_line(p[0:4], p[4], p[5], p[6], p[7], p[8], p[9])


def affine(k):
    a, sx, sy = 0.03 - 0.01 * (k % 5), 1.04 - 0.01 * (k % 3), 0.97 + 0.01 * (k % 4)
    return dict(m=(sx * math.cos(a), -sy * math.sin(a), sx * math.sin(a), sy * math.cos(a)), tx=0.7 - 0.3 * (k % 3), ty=-0.4 + 0.25 * (k % 4))


def distortion(k):
    return dict(sigma=1.5 + 0.5 * (k % 6), maxdelta=1.5 + 0.25 * (k % 3), seed=1000 + 7 * k)


def blurring(k):
    return dict(blur=0.8 + 0.1 * (k % 3))


MODES = {
    "all": lambda k: params(**affine(k), **distortion(k), **blurring(k)),
    "distortion": lambda k: params(**distortion(k)),
    "affine": lambda k: params(**affine(k)),
    "blur": lambda k: params(**blurring(k)),
    # a whole border (for the narrow shapes: the whole image) reads taps outside the image
    "shift": lambda k: params(**dict(affine(k), tx=2.5, ty=-1.5), **distortion(k), **blurring(k)),
}
# (1,1) (1,7) (9,1); the row tile is 64 x 8; an item is 256 outputs: a column-pass item spans several columns and splits one
SHAPES = [(1, 1), (1, 7), (9, 1), (63, 5), (64, 8), (65, 9), (255, 3), (256, 1), (257, 48), (300, 31)]

_IMAGES = {}


def image(k):
    if k not in _IMAGES:
        w, h = SHAPES[k]
        _IMAGES[k] = grey(np.random.default_rng(100 + k), w, h)
    return _IMAGES[k]


@pytest.fixture(scope="module")
def fixture_line(tmp):
    raw = os.path.join(tmp, "fixture.raw")
    subprocess.run([TOOL, "png2raw", FIXTURE, raw], check=True)
    img = np.float32(1.0) - read_raw(raw)             # ink = 1
    assert img.shape == (819, 88)
    return img


def all_images(backend, fixture_line):
    """the shapes above and the fixture line (its first 160 columns on the emulator, to bound its time)"""
    return [image(k) for k in range(len(SHAPES))] + [fixture_line if backend.kind == "hip" else np.ascontiguousarray(fixture_line[:160])]


# ---- the referee -----------------------------------------------------------------------------------------------------------------
_REFEREE = {}


def referee(tmp, img, p, what=None):
    """degrade_line on one image -> image; computed once per (image, parameters).  what = "noise0" / "noise1": the unsmoothed field"""
    img = np.ascontiguousarray(img, F32)
    key = (img.shape, img.tobytes(), tuple(repr(v) for v in p), what)
    if key not in _REFEREE:
        src, dst = os.path.join(tmp, "in.raw"), os.path.join(tmp, "out.raw")
        write_raw(src, img)
        args = [TOOL, "degrade-raw", src, dst] + [repr(float(v)) for v in p[:9]] + [str(p[9])] + ([what] if what else [])
        subprocess.run(args, check=True, capture_output=True, text=True)
        _REFEREE[key] = read_raw(dst)
        assert _REFEREE[key].shape == img.shape
    return _REFEREE[key]


def check(tmp, dg, images, ps):
    """one call on `images` with the parameters `ps`: every line's bytes against the referee"""
    got = dg.run(images, [as_line(p) for p in ps])
    assert len(got) == len(images)
    for b, (img, p) in enumerate(zip(images, ps)):
        want = referee(tmp, img, p)
        assert same_bytes(got[b], want), "line %d (%d x %d, %r): %d of %d values differ, max |d| %g" % (
            b, img.shape[0], img.shape[1], p, int((got[b] != want).sum()), want.size, float(np.abs(got[b] - want).max()))
    return got


# ---- 1. bytes against the referee ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_bytes_against_the_referee(backend, tmp, fixture_line, mode):
    """every shape and the fixture line, one image per call"""
    from clstm_amd.net import Degrader
    dg = Degrader(lib=backend.lib)
    for k, img in enumerate(all_images(backend, fixture_line)):
        got = check(tmp, dg, [img], [MODES[mode](k)])
        if img.size > 64:
            assert not same_bytes(got[0], img)           # (something was done to it)


def test_wide_sigma(backend, tmp):
    """sigma = 20 on 40 x 30: the mask (reach 61) is wider than the image in both directions -- clamping dominates both passes"""
    from clstm_amd.net import Degrader
    img = grey(np.random.default_rng(7), 40, 30)
    check(tmp, Degrader(lib=backend.lib), [img], [params(**affine(1), sigma=20.0, maxdelta=2.0, seed=5, blur=0.5)])


# ---- 2. identity -----------------------------------------------------------------------------------------------------------------
def test_identity_returns_the_input_and_lines_are_counted(backend, tmp, fixture_line):
    from clstm_amd.net import Degrader
    images = all_images(backend, fixture_line)
    dg = Degrader(lib=backend.lib)
    c0 = count(backend, DEGRADED)
    got = dg.run(images, [as_line(IDENTITY)] * len(images))
    assert count(backend, DEGRADED) == c0 + len(images)
    for b, img in enumerate(images):
        assert same_bytes(got[b], img), b
        assert same_bytes(referee(tmp, img, IDENTITY), img), b      # ... and the specification says so too


# ---- 3. hi == lo -----------------------------------------------------------------------------------------------------------------
def test_single_pixel_field_gives_no_displacement(backend, tmp):
    """a 1 x 1 image: each field has one value, hi == lo, the displacement is zero and the result is the affine-only result"""
    from clstm_amd.net import Degrader
    dg = Degrader(lib=backend.lib)
    img = np.full((1, 1), 0.75, F32)
    a = dict(m=(0.9, 0.1, -0.1, 1.1), tx=0.25, ty=-0.125)
    got = check(tmp, dg, [img], [params(**a, sigma=2.0, maxdelta=3.0, seed=9)])
    want = check(tmp, dg, [img], [params(**a)])
    assert same_bytes(got[0], want[0]) and got[0][0, 0] != 0.0


# seeds (found by exhaustive search over all 2^32) whose field 0 / field 1 has the same value at pixels 0 and 1: on a two-pixel image that
# field is constant after smoothing -- both outputs are the same chain over the same values -- while the other field is not.  No seed
# makes both fields of a two-pixel image constant.
CONSTANT_FIELD = {0: 625966222, 1: 564309925}


@pytest.mark.parametrize("f", [0, 1])
@pytest.mark.parametrize("shape", [(2, 1), (1, 2)])
def test_constant_field_gives_no_displacement(backend, tmp, f, shape):
    """hi == lo with more than one pixel: that field's displacement is zero (the division 0 / 0 is not evaluated into the result), the
    other field's is not; the bytes are the referee's.  With only the constant field acting -- the other axis has nothing to sample but
    equal rows / columns -- the result is the affine-only result."""
    from clstm_amd.net import Degrader
    dg = Degrader(lib=backend.lib)
    img = np.array([0.25, 1.0], F32).reshape(shape)
    a = dict(m=(1.0, 0.0, 0.0, 1.0), tx=0.25, ty=-0.25)
    p = params(**a, sigma=1.0, maxdelta=0.75, seed=CONSTANT_FIELD[f])
    u = [referee(tmp, img, p, "noise%d" % g) for g in (0, 1)]
    assert u[f].ravel()[0] == u[f].ravel()[1] and u[1 - f].ravel()[0] != u[1 - f].ravel()[1]
    got = check(tmp, dg, [img], [p])
    assert np.isfinite(got[0]).all()
    assert not same_bytes(got[0], check(tmp, dg, [img], [params(**a)])[0])     # (the other field does displace)


# ---- 4. batch independence -------------------------------------------------------------------------------------------------------
def mixed_batch(backend, fixture_line):
    images = all_images(backend, fixture_line)
    modes = list(MODES) + ["identity"]
    ps = [IDENTITY if modes[k % len(modes)] == "identity" else MODES[modes[k % len(modes)]](k) for k in range(len(images))]
    return images, ps


def test_batch_independence(backend, tmp, fixture_line):
    """all shapes in one call with per-line parameters (every mode and the identity among them): each line's bytes are those of its
    single-line result; the same batch reversed; then a smaller batch on the same degrader (the buffers are grow-only)"""
    from clstm_amd.net import Degrader
    images, ps = mixed_batch(backend, fixture_line)
    dg = Degrader(lib=backend.lib)
    check(tmp, dg, images, ps)
    b0 = dg.device_bytes()
    check(tmp, dg, images[::-1], ps[::-1])
    assert dg.device_bytes() == b0 > 0
    check(tmp, dg, images[3:6], ps[3:6])
    assert dg.device_bytes() == b0
    # pixels resident on the device: the same bytes
    from clstm_amd.net import Normalizer
    pix, w, h = Normalizer.pack(images[3:6])
    pix_d = backend.up(pix)
    dg.run_device_pixels(pix_d, w, h, [as_line(p) for p in ps[3:6]])
    for got, img, p in zip(dg.pixels(), images[3:6], ps[3:6]):
        assert same_bytes(got, referee(tmp, img, p))


# ---- 5. clstm_degrade_draw -------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def splitmix(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def draw_restated(seed, key, visit, rg, h):
    """the generator of clstm_degrade_draw (csrc/degrade_run.inc) restated: -> (angle, log-scale, anisotropy) in double and the line"""
    stream = splitmix(splitmix(splitmix(seed) ^ key) ^ visit)
    bits = lambda k: splitmix((stream + (k + 1) * 0x9e3779b97f4a7c15) & M64)
    u = lambda k: float(bits(k) >> 11) * 2.0 ** -53
    sym = lambda k, a: -a + (2.0 * a) * u(k)
    within = lambda k, iv: float(iv[0]) + (float(iv[1]) - float(iv[0])) * u(k)
    angle, ls, an = sym(0, float(rg.angle)), sym(1, float(rg.scale)), sym(2, float(rg.aniso))
    sx, sy, c, s = math.exp(ls + an), math.exp(ls - an), math.cos(angle), math.sin(angle)
    t = float(rg.translate) * h
    line = params((c * sx, 0.0 - s * sy, s * sx, c * sy), sym(3, t), sym(4, t), within(5, rg.sigma), within(6, rg.maxdelta), within(7, rg.blur),
                  bits(8) >> 32)
    return (angle, ls, an), line


def line_tuple(d):
    return tuple(F32(v) for v in d.m) + (F32(d.tx), F32(d.ty), F32(d.sigma), F32(d.maxdelta), F32(d.blur), int(d.seed))


def line_bits(d):
    return bytes(d)


def test_draw_is_a_function_of_seed_key_visit(backend):
    from clstm_amd.net import draw
    lib = backend.lib
    a = draw(3, 17, 2, 300, 48, lib=lib)
    assert line_bits(a) == line_bits(draw(3, 17, 2, 300, 48, lib=lib))
    assert line_bits(a) == line_bits(draw(3, 17, 2, 555, 48, lib=lib))         # the width has no part in it
    for other in ((4, 17, 2), (3, 18, 2), (3, 17, 3), (17, 3, 2), (3, 2, 17)):
        b = draw(*other, 300, 48, lib=lib)
        assert line_bits(a) != line_bits(b) and a.seed != b.seed, other
    assert line_bits(draw(2 ** 64 - 1, 2 ** 63, 2 ** 40, 300, 48, lib=lib)) != line_bits(a)


def test_draw_stays_inside_its_ranges_and_m_is_the_rounded_double_expression(backend):
    from clstm_amd.net import default_ranges, draw
    lib = backend.lib
    rg = default_ranges(lib)
    assert rg.angle > 0 and rg.scale > 0 and rg.aniso > 0 and rg.translate > 0
    for iv in (rg.sigma, rg.maxdelta, rg.blur):
        assert 0 <= iv[0] < iv[1]
    h = 48
    seen = {name: [] for name in ("angle", "ls", "an", "tx", "sigma", "maxdelta", "blur")}
    for key in range(1000):
        d = draw(11, key, key % 7, 300, h, lib=lib)
        (angle, ls, an), want = draw_restated(11, key, key % 7, rg, h)
        assert line_tuple(d) == want, key                                      # m: the float rounding of the double expression
        assert abs(angle) <= rg.angle and abs(ls) <= rg.scale and abs(an) <= rg.aniso
        t = F32(float(rg.translate) * h)
        assert abs(d.tx) <= t and abs(d.ty) <= t
        assert rg.sigma[0] <= d.sigma <= rg.sigma[1] and rg.maxdelta[0] <= d.maxdelta <= rg.maxdelta[1] and rg.blur[0] <= d.blur <= rg.blur[1]
        # the matrix itself: its determinant is sx sy = exp(2 ls), the angle of its first column is the rotation
        det = float(d.m[0]) * d.m[3] - float(d.m[1]) * d.m[2]
        assert abs(math.log(det)) <= 2 * rg.scale + 1e-6 and abs(math.atan2(d.m[2], d.m[0])) <= rg.angle + 1e-6
        for name, v in zip(seen, (angle, ls, an, d.tx, d.sigma, d.maxdelta, d.blur)):
            seen[name].append(v)
    for name, lo, hi in (("angle", -rg.angle, rg.angle), ("ls", -rg.scale, rg.scale), ("an", -rg.aniso, rg.aniso), ("tx", -rg.translate * h, rg.translate * h),
                         ("sigma", *rg.sigma), ("maxdelta", *rg.maxdelta), ("blur", *rg.blur)):
        v = np.array(seen[name])                                               # ... and the range is used: 1000 uniform draws leave
        assert v.min() < lo + 0.05 * (hi - lo) and v.max() > hi - 0.05 * (hi - lo), name   # 5% at an end empty with probability 2 * 0.95^1000


def test_draw_with_zero_width_ranges_is_the_identity(backend):
    from clstm_amd.abi import DegradeRanges
    from clstm_amd.net import draw
    rg = DegradeRanges()
    for key in range(20):
        d = draw(5, key, 1, 200, 40, ranges=rg, lib=backend.lib)
        assert line_tuple(d)[:9] == IDENTITY[:9]
        assert bytes(d)[:36] == bytes(as_line(IDENTITY))[:36]                 # +0.0 everywhere, not -0.0
    rg.sigma[0] = rg.sigma[1] = 2.5
    rg.blur[0] = rg.blur[1] = 0.5
    d = draw(5, 3, 1, 200, 40, ranges=rg, lib=backend.lib)
    assert d.sigma == 2.5 and d.blur == 0.5 and d.maxdelta == 0.0


def test_draw_refuses_bad_ranges(backend):
    from clstm_amd.abi import ClstmError, DegradeRanges
    from clstm_amd.net import draw
    rg = DegradeRanges()
    rg.sigma[0], rg.sigma[1] = 3.0, 2.0
    with pytest.raises(ClstmError, match="LO <= HI"):
        draw(0, 0, 0, 10, 10, ranges=rg, lib=backend.lib)
    rg = DegradeRanges()
    rg.angle = float("nan")
    with pytest.raises(ClstmError, match="finite"):
        draw(0, 0, 0, 10, 10, ranges=rg, lib=backend.lib)


def test_drawn_lines_at_the_default_ranges_against_the_referee(backend, tmp, fixture_line):
    """what training does: parameters from clstm_degrade_draw at the default ranges, keyed by the line"""
    from clstm_amd.net import Degrader, draw
    images = all_images(backend, fixture_line)[3:]
    lines = [draw(1, key, 0, img.shape[0], img.shape[1], lib=backend.lib) for key, img in enumerate(images)]
    got = Degrader(lib=backend.lib).run(images, lines)
    for b, img in enumerate(images):
        assert same_bytes(got[b], referee(tmp, img, line_tuple(lines[b]))), b


# ---- 6. the noise (host arithmetic: the emulator run only) -----------------------------------------------------------------------
def test_noise_statistics(tmp):
    """the unsmoothed fields of a 64 x 64 image, from the referee.  The bounds follow from the sample size: the mean of 4096 uniform
    values has standard error 0.289/64 (6.6 of them: 0.03); a lag-1 correlation has standard error 1/64 (6 of them: below 0.1)"""
    img = np.zeros((64, 64), F32)
    p = params(sigma=1.0, maxdelta=1.0, seed=12345)
    fields = [referee(tmp, img, p, "noise%d" % f).astype(np.float64) for f in (0, 1)]
    for u in fields:
        assert u.min() >= 0.0 and u.max() < 1.0
        assert 0.47 <= u.mean() <= 0.53, u.mean()
        for a, b in ((u[1:, :], u[:-1, :]), (u[:, 1:], u[:, :-1])):
            r = np.corrcoef(a.ravel(), b.ravel())[0, 1]
            assert abs(r) < 0.1, r
    assert not np.array_equal(fields[0], fields[1])
    assert abs(np.corrcoef(fields[0].ravel(), fields[1].ravel())[0, 1]) < 0.1
    assert not np.array_equal(fields[0], referee(tmp, img, params(sigma=1.0, maxdelta=1.0, seed=12346), "noise0"))   # the seed has a part in it


# ---- 7. refusals, each by its text, the degrader usable afterwards ---------------------------------------------------------------
def raw_run(backend, dg, pix, w, h, bs, lines, out=True):
    from clstm_amd.abi import DegradeLine, i32, ptr
    wa, ha = i32(w), i32(h)
    arr = (DegradeLine * len(lines))(*lines)
    res = ctypes.c_void_p()
    backend.lib.call("clstm_degrader_run_h", dg.h, ptr(pix), ptr(wa), ptr(ha), bs, ctypes.cast(arr, ctypes.c_void_p), ctypes.byref(res) if out else None)


@pytest.fixture()
def used_degrader(backend, tmp):
    """a degrader after a good call -> (degrader, its image, its parameters, its output)"""
    from clstm_amd.net import Degrader
    dg = Degrader(lib=backend.lib)
    img, p = image(3), MODES["all"](3)
    return dg, img, p, check(tmp, dg, [img], [p])[0]


def refused(backend, tmp, used, match, w, h, bs, lines, pix=True, out=True):
    """the call is refused by its text; nothing was counted or allocated, the last good call's output is still there (the refused call
    produced nothing), and the next good call is right"""
    from clstm_amd.abi import ClstmError, f32
    dg, img, p, first = used
    state = (dg.device_bytes(), count(backend, DEGRADED))
    with pytest.raises(ClstmError, match=match):
        raw_run(backend, dg, f32(np.ones(64)) if pix else None, w, h, bs, lines, out)
    assert (dg.device_bytes(), count(backend, DEGRADED)) == state
    assert same_bytes(dg.pixels()[0], first)
    check(tmp, dg, [img], [p])


def test_refuses_an_empty_batch(backend, tmp, used_degrader):
    refused(backend, tmp, used_degrader, "bs must be positive", [4], [4], 0, [as_line(IDENTITY)])


def test_refuses_a_zero_width(backend, tmp, used_degrader):
    refused(backend, tmp, used_degrader, "line 1 has width 0", [4, 0], [4, 4], 2, [as_line(IDENTITY)] * 2)


def test_refuses_nan_in_m(backend, tmp, used_degrader):
    refused(backend, tmp, used_degrader, "line 0: m, tx and ty must be finite", [4], [4], 1, [as_line(params(m=(1.0, float("nan"), 0.0, 1.0)))])


def test_refuses_a_negative_maxdelta(backend, tmp, used_degrader):
    refused(backend, tmp, used_degrader, "maxdelta must be finite and not negative", [4], [4], 1, [as_line(params(sigma=2.0, maxdelta=-1.0))])


def test_refuses_sigma_zero_with_distortion(backend, tmp, used_degrader):
    refused(backend, tmp, used_degrader, "sigma must be positive where maxdelta > 0", [4], [4], 1, [as_line(params(sigma=0.0, maxdelta=1.0))])


def test_refuses_a_sigma_beyond_the_reach_limit(backend, tmp, used_degrader):
    refused(backend, tmp, used_degrader, "mask of sigma .* NZ_MAXRANGE = 800", [4], [4], 1, [as_line(params(sigma=267.0, maxdelta=1.0))])
    refused(backend, tmp, used_degrader, "mask of blur .* NZ_MAXRANGE = 800", [4], [4], 1, [as_line(params(blur=1e30))])
    # ... and the largest admitted reach is admitted: 1 + int(3 * 266.3) = 799
    used_degrader[0].run([image(0)], [as_line(params(sigma=266.3, maxdelta=1.0))])


def test_get_pixels_before_any_call_is_refused(backend):
    from clstm_amd.abi import ClstmError
    from clstm_amd.net import Degrader
    dg = Degrader(lib=backend.lib)
    with pytest.raises(ClstmError, match="produced nothing"):
        backend.lib.call("clstm_degrader_get_pixels_h", dg.h, np.zeros(4, np.float32).ctypes.data)


def test_refuses_a_null_argument(backend, tmp, used_degrader):
    refused(backend, tmp, used_degrader, "null argument", [4], [4], 1, [as_line(IDENTITY)], pix=False)
    refused(backend, tmp, used_degrader, "null argument", [4], [4], 1, [as_line(IDENTITY)], out=False)


# ---- 8. chaining on the device ---------------------------------------------------------------------------------------------------
def chain_images(rng):
    return [grey(rng, w, 30) for w in (61, 118, 90)]


def chain_params(step):
    return [MODES["all"](k + 3 * step) for k in range(3)]


def test_degrade_normalize_train_step_on_the_device(backend, tmp):
    """Degrader.run_device -> Normalizer.run_device_pixels -> Network.train_step, no host copy in between: T, r and the frames are
    those of referee-degrade followed by normalize-raw, the trained parameters those of a step fed the same frames from the host"""
    from clstm_amd.init import init_params
    from clstm_amd.net import Degrader, Network, Normalizer
    ni, nh, nc = 48, [8], 11
    rng = np.random.default_rng(61)
    p0 = init_params(ni, nh, nc, seed=0.222) * 20
    host, dev = Network(ni, nh, nc, lib=backend.lib), Network(ni, nh, nc, lib=backend.lib)
    for n in (host, dev):
        n.set_params(p0)
        n.setLearningRate(1e-2, 0.9)
    dg, nz = Degrader(lib=backend.lib), Normalizer(ni, lib=backend.lib)
    for step in range(2):
        images, ps = chain_images(rng), chain_params(step)
        want = [normalize_referee(tmp, referee(tmp, img, p)) for img, p in zip(images, ps)]
        lines = [f for _, _, f in want]
        T = [len(x) for x in lines]
        trs = synth_labels(rng, len(T), 5, nc)
        x = backend.up(np.concatenate(lines, 0))      # (kept alive until the sync below: the step is asynchronous)
        host.train_step(T, x, trs)
        c0 = (count(backend, DEGRADED), count(backend, NORMALIZED))
        pix_d = dg.run_device(images, [as_line(p) for p in ps])
        Td, rd, frames_d = nz.run_device_pixels(pix_d, [a.shape[0] for a in images], [a.shape[1] for a in images])
        assert (count(backend, DEGRADED), count(backend, NORMALIZED)) == (c0[0] + 3, c0[1] + 3)
        assert Td.tolist() == T and [float(v) for v in rd] == [r for _, r, _ in want]
        dev.train_step(T, frames_d, trs)
        backend.sync()
        assert same_bytes(nz.frames(), np.concatenate(lines, 0)), step
        assert same_bytes(dev.get_params(), host.get_params()), step
        assert same_bytes(dev.get_derivs(), host.get_derivs()), step
    assert not np.array_equal(host.get_params(), p0.astype(np.float32))


def test_degrade_normalize_predict_on_the_device(backend, tmp):
    from clstm_amd.abi import i32, ptr
    from clstm_amd.net import Degrader, Normalizer
    from test_predict import make_net, raw_predict, varied_params
    ni, nh, nc = 48, [8], 11
    rng = np.random.default_rng(59)
    images, ps = chain_images(rng), chain_params(0)
    lines = [normalize_referee(tmp, referee(tmp, img, p))[2] for img, p in zip(images, ps)]
    prm = varied_params(backend, ni, nh, nc, lines)
    host, dev = make_net(backend, ni, nh, nc, prm), make_net(backend, ni, nh, nc, prm)
    cls_h, loc_h, conf_h, cnt_h = raw_predict(host, lines)
    z_h = host.outputs()
    dg, nz = Degrader(lib=backend.lib), Normalizer(ni, lib=backend.lib)
    pix_d = dg.run_device(images, [as_line(p) for p in ps])
    T, _, frames_d = nz.run_device_pixels(pix_d, [a.shape[0] for a in images], [a.shape[1] for a in images])
    assert T.tolist() == [len(x) for x in lines]
    N = int(T.sum())
    cls, loc = np.full(N, -7, np.int32), np.full(N, -7, np.int32)
    conf, cnt = np.full(N, -7.0, np.float32), np.full(len(T), -7, np.int32)
    backend.lib.call("clstm_net_predict", dev.h, ptr(i32(T)), len(T), frames_d, ptr(cls), ptr(loc), ptr(conf), ptr(cnt))
    dev.T, dev.N = [int(t) for t in T], N
    assert same_bytes(dev.outputs(), z_h) and np.array_equal(cnt, cnt_h) and cnt.sum() > 0
    off = np.concatenate([[0], np.cumsum(T)])
    for b in range(len(T)):
        o, k = off[b], cnt[b]
        assert np.array_equal(cls[o:o + k], cls_h[o:o + k]) and np.array_equal(loc[o:o + k], loc_h[o:o + k])
        assert same_bytes(conf[o:o + k], conf_h[o:o + k])
