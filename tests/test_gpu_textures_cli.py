"""The command line's --textures on the GPU (include/trx.h, "texture coordinates and albedo textures"): on standin:cornell the PNG
is trx_render_image_colour_textured's with the stand-in tables permuted by tri_source - plain, with --emitters and with --smooth;
on the fixture OBJ (tests/golden/quad_tex.obj) it is the binding's host form fed the loaders' tables and the fixture's texels
(decoded here by tests/texture_twin.py's PPM reader, rows flipped, sRGB, bilinear) - once per image fixture, so the command
line's PPM decoder and its PNG decoder (RGB and RGBA, all five scanline filters between them) give the same image for the same
texels."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import texture_twin as TT
from test_gpu_light import limit
from test_gpu_light_cli import BASE, CLI, H, W, _png, _run

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("extra,kw", [([], {}), (["--emitters", "2"], {"emitter_samples": 2}), (["--smooth"], {"smooth": True})],
                         ids=["plain", "emitters", "smooth"])
def test_cli_textures_on_the_standin_is_the_textured_host_form(trx, tmp_path, extra, kw):
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    mats, idx = trx.standin_materials("cornell", verts, counts)
    eye, look, fov = trx.scene_camera("cornell")
    view = trx.view_from_camera(eye, look, fov, W, H)
    point = trx.light(trx.LIGHT_POINT, (0.0, 1.8, 0.0), intensity=2.0)
    with limit(300):
        img = _run(tmp_path, "--light", "point:0,1.8,0:2", "--colour", "--textures", "--bounce-samples", "2", *extra)
    sc = trx.Scene(flat)
    try:
        sc.set_materials(mats, idx[flat.tri_source])
        if kw.get("smooth"):
            sc.set_vertex_normals(trx.compute_vertex_normals(verts, float(f32(np.cos(45.0 * 3.14159265358979323846 / 180.0))))[flat.tri_source])
        args = dict(bounce_samples=2, bounce_eps=0.01, sem=3, shadow_eps=0.01, ambient=0.1, **kw)
        with limit():
            plain, _ = sc.render_image_colour_textured(view, W, H, [point], **args)
        sc.set_texcoords(trx.standin_texcoords("cornell", verts)[flat.tri_source])
        sc.set_textures(*trx.standin_textures("cornell", mats.shape[0]))
        with limit():
            want, _ = sc.render_image_colour_textured(view, W, H, [point], **args)
        assert (img == want).all(), "%d pixels differ from trx_render_image_colour_textured" % (img != want).any(2).sum()
        assert (want != plain).any(2).sum() > 200                      # (the checker shows on the grey material)
        sc.check()
    finally:
        sc.close()


@pytest.mark.parametrize("image", ["checker_4x3.ppm", "checker_4x3.png", "checker_4x3_rgba.png"])
def test_cli_decoders_give_the_fixtures_texels(trx, tmp_path, image):
    for name in ("quad_tex.obj", image):
        shutil.copy(os.path.join(GOLDEN, name), str(tmp_path / name))
    (tmp_path / "quad_tex.mtl").write_text(open(os.path.join(GOLDEN, "quad_tex.mtl")).read().replace("checker_4x3.ppm", image))
    obj = str(tmp_path / "quad_tex.obj")
    args = [CLI, "-i", obj] + BASE[2:] + ["--light", "dir:0.2,0.3,1", "--colour", "--textures"]
    with limit(300):
        r = subprocess.run(args, capture_output=True, text=True, timeout=280, cwd=str(tmp_path))
    assert r.returncode == 0 and "untextured" not in r.stderr, r.stderr
    img = _png(str(tmp_path / "quad_tex_rend.png"), W, H)
    verts, counts, mats, idx = trx.load_model_materials(obj)
    _, _, uvs, has = trx.load_model_texcoords(obj)
    maps = trx.load_model_material_maps(obj)
    assert has and maps == ["", image, ""] and idx.tolist() == [1, 1, 2, 1]
    texels = TT.read_ppm(os.path.join(GOLDEN, "checker_4x3.ppm"))[::-1]          # (top-down file: row 0 of the texture is the bottom row)
    flat = trx.flat_build(verts, counts)
    # the command line's camera for a model file: from +z, a box diagonal away from the box's centre, 60 degrees (binary32)
    pts = verts.reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    centre = (f32(0.5) * (lo + hi)).astype(np.float32)
    ext = (hi - lo).astype(np.float32)
    diag = f32(0.0)
    for c in range(3):
        diag = f32(diag + f32(ext[c] * ext[c]))
    eye = centre.copy()
    eye[2] = f32(eye[2] + np.sqrt(diag))
    view = trx.view_from_camera(eye.tolist(), centre.tolist(), 60.0, W, H)
    light = [trx.light(trx.LIGHT_DIRECTIONAL, (0.2, 0.3, 1.0))]
    sc = trx.Scene(flat)
    try:
        sc.set_materials(mats, idx[flat.tri_source])
        with limit():
            plain, _ = sc.render_image_colour_textured(view, W, H, light, sem=3, shadow_eps=0.01, ambient=0.1)
        sc.set_texcoords(uvs[flat.tri_source])
        sc.set_textures([[4, 3, trx.TEX_RGBA8_SRGB, trx.TEX_BILINEAR]], np.ascontiguousarray(texels).reshape(-1), [trx.NO_TEXTURE, 0, trx.NO_TEXTURE])
        with limit():
            want, _ = sc.render_image_colour_textured(view, W, H, light, sem=3, shadow_eps=0.01, ambient=0.1)
        assert (img == want).all(), "%s: %d pixels differ from trx_render_image_colour_textured" % (image, (img != want).any(2).sum())
        assert (want != plain).any(2).sum() > 100                      # (the texture shows on the quad)
        sc.check()
    finally:
        sc.close()
