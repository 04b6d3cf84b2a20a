"""tray_racing_hip --png --light ...: the image is trx_render_image_lit's - the composition tests/test_gpu_light.py holds to the
twin - the options that do not go together are refused, and without --light the program does what it did."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tray_racing_amd", "tray_racing_hip")
W, H = 96, 64
BASE = ["-i", "standin:cornell", "--render-time", "0", "--width", str(W), "--height", str(H), "--passes", "1", "--png", "--cpu-semantics"]


def _png(path, w, h):
    data = open(path, "rb").read()
    pos, idat = 8, b""
    while pos < len(data):
        size, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if tag == b"IDAT":
            idat += data[pos + 8:pos + 8 + size]
        pos += 12 + size
    return np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)[:, 1:].reshape(h, w, 4)


def _run(tmp_path, *extra):
    r = subprocess.run([CLI] + BASE + list(extra), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    return _png(str(tmp_path / "cornell_rend.png"), W, H).copy()


def test_cli_png_with_lights_is_the_lit_frame(trx, tmp_path):
    assert trx.load().trx_device_count() > 0, "no HIP device visible to libtrx.so"
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    eye, look, fov = trx.scene_camera("cornell")
    view = trx.view_from_camera(eye, look, fov, W, H)
    sc = trx.Scene(flat)
    point = trx.light(trx.LIGHT_POINT, (0.0, 1.8, 0.0), intensity=2.0)
    rect = trx.light(trx.LIGHT_RECT, (-0.4, 1.9, -0.4), (0.8, 0.0, 0.0), (0.0, 0.0, 0.8))
    sun = trx.light(trx.LIGHT_DIRECTIONAL, (0.3, 1.0, 0.4), intensity=0.5)
    try:
        # the defaults: one sample, unmasked, shadow_eps 0.01, ambient 0.1, no AO term (the command line's ao_eps is 0.0001)
        img = _run(tmp_path, "--light", "point:0,1.8,0:2")
        want, _ = sc.render_image_lit(view, W, H, [point], sem=3, shadow_eps=0.01, ambient=0.1)
        assert (img == want).all(), "%d pixels differ from trx_render_image_lit" % (img != want).any(2).sum()
        assert (img[..., 3] == 255).all() and np.unique(img[..., 0]).size >= 8
        # every option, three lights, the ambient under the filtered AO term
        img3 = _run(tmp_path, "--light", "point:0,1.8,0:2", "--light", "rect:-0.4,1.9,-0.4:0.8,0,0:0,0,0.8", "--light", "dir:0.3,1,0.4:0.5",
                    "--light-samples", "8", "--light-mask", "3", "--shadow-eps", "0.001", "--ambient", "0.25", "--ao-samples", "4", "--ao-radius", "1.4",
                    "--ao-filter", "2", "--ao-depth-tol", "0.05", "--ao-normal-cos", "0.5")
        want3, _ = sc.render_image_lit(view, W, H, [point, rect, sun], sem=3, ray_mask=3, light_samples=8, shadow_eps=0.001, ambient=0.25, ao_samples=4,
                                       ao_eps=0.0001, ao_radius=1.4, filter_radius=2, depth_tol=0.05, normal_cos=0.5)
        assert (img3 == want3).all(), "%d pixels differ from trx_render_image_lit" % (img3 != want3).any(2).sum()
        assert (img3 != img).any()
        # --ao-samples without --ao-filter: the term at radius 0
        img4 = _run(tmp_path, "--light", "dir:0.3,1,0.4:0.5", "--ao-samples", "4")
        want4, _ = sc.render_image_lit(view, W, H, [sun], sem=3, ambient=0.1, ao_samples=4, ao_eps=0.0001, filter_radius=0)
        assert (img4 == want4).all()
        # without --light the program does what it did: the reference's image, another one
        assert (_run(tmp_path) != img).any()
        sc.check()
    finally:
        sc.close()


def test_cli_refuses_the_options_that_do_not_go_with_lights(tmp_path):
    def run(*extra):
        return subprocess.run([CLI] + BASE + list(extra), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    light = ("--light", "point:0,1.8,0")
    for extra, msg in (((*light, "--profile-rt", "tris"), "not together"), ((*light, "--ao-samples", "4", "--ao-stride", "2"), "not together"),
                       (("--light-samples", "4"), "go with --light"), (("--light", "rect:0,0,0:1,0,0"), "--light takes"), ((*light * 9,), "at most 8")):
        r = run(*extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "cornell_rend.png").exists()
