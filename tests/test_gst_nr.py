"""GPU tests of bayer2rgb denoise / noise-read / noise-shot: a gst-launch pipeline over a 258 x 37 stream, 8-bit and
12-bit, compared byte for byte with the CPU oracle (the deep strip model) applied to the model-denoised mosaic
(tests/nr_model.py) under the curve of the same noise model."""
import numpy as np
import pytest

import nr_model as nm
import strip_cases as sc
from test_gpu_shading import DEEP_12_TO_16
import colour_model as cm
from test_gst_colour import PROPS as COLOUR, file_pipeline, stage
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, needs_gst]

W, H = 258, 37


@pytest.mark.parametrize("extra", ["", "inflight=3 devices=0,0"])
def test_bayer2rgb_denoise_equals_the_model_8bit(plugin, gpu_pkg, oracle, tmp_path, extra):
    n, stride = 3, 260
    rng = np.random.default_rng(2581)
    src = np.full((n, H, stride), 0x5A, np.uint8)
    src[:, :, :W] = np.clip(rng.normal(0, 5, (n, H, W)) + np.linspace(20, 230, W), 0, 255).astype(np.uint8)
    r, g, b = gpu_pkg.FORMATS["BGRx"]
    for k, (strength, read, shot, black) in enumerate(((1.5, 4.0, 0.0, 0), (2.0, 2.0, 0.25, 16), (1.0, 2.0, 0.0, 0))):
        props = "denoise=%r noise-read=%r noise-shot=%r %s" % (strength, read, shot, extra)
        if k == 1:
            props += " " + COLOUR % black       # the shot noise counts from the colour stage's black level
        if k == 2:
            props = "denoise=1 " + extra        # the defaults of the other two
        curve = nm.noise_curve(8, black, read, shot, strength)
        if k == 1:
            assert curve != nm.noise_curve(8, 0, read, shot, strength)
        got = file_pipeline(tmp_path, src, W, H, "grbg", "BGRx", 4, " ".join(props.split()), "nr%d" % k)
        for i in range(n):
            clean = nm.denoise_raw(src[i], src[i], W, H, stride, 0, False, curve).reshape(H, stride)
            assert not np.array_equal(clean, src[i])
            if black:
                want = cm.bayer2rgb_colour(clean, W, H, "grbg", "BGRx", method="bilinear", stride=stride, **stage(gpu_pkg, black))
            else:
                want = oracle.bayer2rgb(clean, W, "grbg", r, g, b)
            assert np.array_equal(got[i], want), (extra, k, i)
    # denoise=0: the reference's bytes, whatever the noise model says
    plain = file_pipeline(tmp_path, src, W, H, "grbg", "BGRx", 4, "denoise=0 noise-read=9 noise-shot=3 " + extra, "plain")
    for i in range(n):
        assert np.array_equal(plain[i], oracle.bayer2rgb(src[i], W, "grbg", r, g, b))


def test_bayer2rgb_denoise_equals_the_model_12bit(plugin, gpu_pkg, tmp_path):
    n = 2
    rng = np.random.default_rng(2582)
    S = np.clip(rng.normal(0, 40, (n, H, W)) + np.linspace(300, 3800, W), 0, 4095).astype(np.int64)
    src = np.stack([sc.frame_bytes(S[i], 12, rng) for i in range(n)])
    stride = src.shape[2]
    curve = nm.noise_curve(12, 0, 20.0, 0.4, 1.25)
    got = file_pipeline(tmp_path, src, W, H, "rggb12le", "ARGB64", 8, "denoise=1.25 noise-read=20 noise-shot=0.4", "nr12")
    case = sc.Case(W, H, "rggb", "ARGB64", False, False)
    for i in range(n):
        clean = nm.denoise_raw(src[i], src[i], W, H, stride, 12, False, curve).reshape(H, stride)
        assert not np.array_equal(clean, src[i])
        assert np.array_equal(got[i], sc.expect(DEEP_12_TO_16.arm, clean, case).reshape(H, -1)), i
    plain = file_pipeline(tmp_path, src, W, H, "rggb12le", "ARGB64", 8, "denoise=0", "plain12")
    for i in range(n):
        assert np.array_equal(plain[i], sc.expect(DEEP_12_TO_16.arm, src[i], case).reshape(H, -1)), i
