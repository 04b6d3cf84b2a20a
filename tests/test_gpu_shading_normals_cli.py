"""The command line's --smooth on the GPU (include/trx.h, "vertex normals and the shading normal"): `--png --light ... --smooth`
and `--png --colour --smooth` on standin:cornell write the images the binding's host forms give for the same arguments with
trx_compute_vertex_normals' table (by tri_source) - at the default crease of 45 degrees and at --smooth-crease 180, where every
corner is welded and the image differs from the faceted one."""
import math
import subprocess

import numpy as np
import pytest

from test_gpu_emitters_cli import CLI, _read_png
from test_gpu_light import limit

pytestmark = pytest.mark.gpu
LIGHT = (0.0, 1.8, 0.0)


@pytest.mark.parametrize("colour,crease", [(False, None), (False, 180.0), (True, None), (True, 180.0)])
def test_the_command_line_writes_the_smooth_host_forms_image(trx, tmp_path, colour, crease):
    w, h = 72, 48
    args = ["-i", "standin:cornell", "--render-time", "0", "--width", str(w), "--height", str(h), "--passes", "1", "--png", "--light",
            "point:%g,%g,%g:1.5" % LIGHT, "--smooth"]
    args += ["--smooth-crease", "%g" % crease] if crease is not None else []
    args += ["--colour", "--bounce-samples", "2"] if colour else []
    with limit(300):
        r = subprocess.run([CLI] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-800:]
    img = _read_png(str(tmp_path / "cornell_rend.png"))
    assert img.shape == (h, w, 4)
    # the same call through the binding: the command line's scene, camera, tables (by tri_source) and defaults
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    eye, look, fov = trx.scene_camera("cornell")
    view = trx.view_from_camera(eye, look, fov, w, h)
    lights = [trx.light(trx.LIGHT_POINT, LIGHT, intensity=1.5)]
    crease_cos = float(np.float32(math.cos((45.0 if crease is None else crease) * 3.14159265358979323846 / 180.0)))
    normals = trx.compute_vertex_normals(verts, crease_cos)
    sc = trx.Scene(flat)
    try:
        sc.set_vertex_normals(normals[flat.tri_source])
        kw = dict(ambient=0.1, frame0=0, ao_eps=0.0001)               # (the command line's defaults; the frame counter stands still)
        with limit():
            if colour:
                mats, idx = trx.standin_materials("cornell", verts, counts)
                sc.set_materials(mats, idx[flat.tri_source])
                want, _ = sc.render_image_colour_smooth(view, w, h, lights, bounce_samples=2, **kw)
                faceted, _ = sc.render_image_colour(view, w, h, lights, bounce_samples=2, **kw)
            else:
                want, _ = sc.render_image_lit_smooth(view, w, h, lights, **kw)
                faceted, _ = sc.render_image_lit(view, w, h, lights, **kw)
    finally:
        sc.close()
    assert (img == want).all(), int((img != want).sum())
    if crease is not None:
        assert (img != faceted).sum() > 50                              # welded across the box's edges: not the faceted image


def test_the_refusals_hold_on_a_real_run(tmp_path):
    """What tests/test_shading_normals.py asks of a --dry-run, without it: refused before a scene is built or a device touched."""
    light = ["--light", "point:0,1.8,0"]
    for extra, msg in ((["--png", "--smooth", "--bounce-samples", "2"] + light, "grey --bounce-samples"), (["--png", "--smooth", "--benchmark"] + light, "--benchmark"),
                       (["--png", "--smooth", "--profile-rt", "tris"], "--profile-rt"), (["--smooth"] + light, "--png"), (["--png", "--smooth"], "--smooth")):
        r = subprocess.run([CLI, "-i", "standin:cornell", "--render-time", "0", "--passes", "1", "--width", "16", "--height", "16"] + extra, cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not list(tmp_path.iterdir())
