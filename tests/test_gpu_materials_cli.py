"""tray_racing_hip --png --light ... --colour: on standin:cornell the image is trx_render_image_colour's with the stand-in table
permuted by tri_source - a red and a green wall that tint the floor beside them - with every --bounce-*, --ao-* and --light
option; on -i <file.obj> the table is the mtl files'; the options that do not go together are refused."""
import subprocess

import numpy as np
import pytest

from test_gpu_light_cli import BASE, CLI, H, W, _png, _run

pytestmark = pytest.mark.gpu
f32 = np.float32


def _cornell(trx):
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    mats, idx = trx.standin_materials("cornell", verts, counts)
    eye, look, fov = trx.scene_camera("cornell")
    sc = trx.Scene(flat)
    sc.set_materials(mats, idx[flat.tri_source])
    return sc, trx.view_from_camera(eye, look, fov, W, H)


def test_cli_png_with_colour_is_the_colour_frame(trx, tmp_path):
    assert trx.load().trx_device_count() > 0, "no HIP device visible to libtrx.so"
    sc, view = _cornell(trx)
    point = trx.light(trx.LIGHT_POINT, (0.0, 1.8, 0.0), intensity=2.0)
    rect = trx.light(trx.LIGHT_RECT, (-0.4, 1.9, -0.4), (0.8, 0.0, 0.0), (0.0, 0.0, 0.8))
    try:
        # direct light only: compose without an indirect term
        direct = _run(tmp_path, "--light", "point:0,1.8,0:2", "--colour")
        want, _ = sc.render_image_colour(view, W, H, [point], sem=3, shadow_eps=0.01, ambient=0.1)
        assert (direct == want).all(), "%d pixels differ from trx_render_image_colour" % (direct != want).any(2).sum()
        # one bounce: the walls tint the floor
        img = _run(tmp_path, "--light", "point:0,1.8,0:2", "--colour", "--bounce-samples", "16")
        want, _ = sc.render_image_colour(view, W, H, [point], bounce_samples=16, bounce_eps=0.01, sem=3, shadow_eps=0.01, ambient=0.1)
        assert (img == want).all(), "%d pixels differ from trx_render_image_colour" % (img != want).any(2).sum()
        assert (img != direct).any()
        px = img.astype(int)
        red, green = (px[..., 0] > px[..., 1] + 20) & (px[..., 1] == px[..., 2]), (px[..., 1] > px[..., 0] + 20) & (px[..., 0] == px[..., 2])
        # a red wall on the left, a green one on the right (white surfaces under a wall's bleed alone can pass for it: a few pixels)
        assert red[:, :W // 2].sum() > 100 and green[:, W // 2:].sum() > 100, (red.sum(), green.sum())
        assert red[:, :W // 2].sum() > 10 * red[:, W // 2:].sum() and green[:, W // 2:].sum() > 10 * green[:, :W // 2].sum(), (red.sum(0), green.sum(0))
        grey = (px[..., 0] == px[..., 1]).mean()
        tint_l, tint_r = px[:, :W // 2][~red[:, :W // 2]].sum(0), px[:, W // 2:][~green[:, W // 2:]].sum(0)
        print("red - green over what is not a wall: left half %d, right half %d; grey pixels %.2f" % (tint_l[0] - tint_l[1], tint_r[0] - tint_r[1], grey))
        assert tint_l[0] - tint_l[1] > tint_r[0] - tint_r[1] and grey < 0.9, (tint_l, tint_r, grey)      # what is not a wall leans toward the nearer wall's tint
        # every option, two lights, the ambient under the filtered AO term, the sparse bounce upsampled and filtered
        img2 = _run(tmp_path, "--light", "point:0,1.8,0:2", "--light", "rect:-0.4,1.9,-0.4:0.8,0,0:0,0,0.8", "--light-samples", "8", "--light-mask", "3",
                    "--shadow-eps", "0.001", "--ambient", "0.25", "--ao-samples", "4", "--ao-radius", "1.4", "--ao-filter", "2", "--bounce-samples", "3",
                    "--bounce-eps", "0.002", "--bounce-stride", "3", "--bounce-phase", "8", "--bounce-upsample", "2", "--bounce-filter", "2",
                    "--bounce-filter-tol", "0.05", "--bounce-filter-cos", "0.5", "--colour")
        want2, _ = sc.render_image_colour(view, W, H, [point, rect], bounce_samples=3, bounce_stride=3, bounce_phase=8, bounce_upsample_radius=2,
                                          bounce_filter_levels=2, bounce_depth_tol=0.05, bounce_normal_cos=0.5, bounce_eps=0.002, sem=3, ray_mask=3,
                                          light_samples=8, shadow_eps=0.001, ambient=0.25, ao_samples=4, ao_eps=0.0001, ao_radius=1.4, filter_radius=2)
        assert (img2 == want2).all(), "%d pixels differ from trx_render_image_colour" % (img2 != want2).any(2).sum()
        # without the option: the grey images as before
        grey = _run(tmp_path, "--light", "point:0,1.8,0:2", "--bounce-samples", "4")
        want_grey, _ = sc.render_image_gi(view, W, H, [point], 4, bounce_eps=0.01, bounce_albedo=0.5, sem=3, shadow_eps=0.01, ambient=0.1)
        assert (grey == want_grey).all() and (grey[..., 0] == grey[..., 1]).all()
        sc.check()
    finally:
        sc.close()


OBJ = """mtllib two.mtl
v -1 -1 0
v 1 -1 0
v 1 1 0
v -1 1 0
v -1 -1 -1
v 1 -1 -1
usemtl left
f 1 2 3
usemtl right
f 1 3 4
f 1 2 6 5
"""
MTL = "newmtl left\nKd 0.9 0.1 0.1\nnewmtl right\nKd 0.1 0.2 0.9\nKe 0.1 0.1 0.1\n"


def test_cli_takes_the_mtl_of_an_obj(trx, tmp_path):
    (tmp_path / "two.obj").write_text(OBJ)
    (tmp_path / "two.mtl").write_text(MTL)
    args = [CLI, "-i", str(tmp_path / "two.obj")] + BASE[2:] + ["--light", "dir:0.2,0.3,1", "--colour", "--bounce-samples", "2"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    img = _png(str(tmp_path / "two_rend.png"), W, H)
    verts, counts, mats, idx = trx.load_model_materials(str(tmp_path / "two.obj"))
    assert idx.tolist() == [1, 2, 2, 2] and mats.shape[0] == 3
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
    sc = trx.Scene(flat)
    try:
        sc.set_materials(mats, idx[flat.tri_source])
        want, _ = sc.render_image_colour(view, W, H, [trx.light(trx.LIGHT_DIRECTIONAL, (0.2, 0.3, 1.0))], bounce_samples=2, bounce_eps=0.01, sem=3,
                                         shadow_eps=0.01, ambient=0.1)
        assert (img == want).all(), "%d pixels differ from trx_render_image_colour" % (img != want).any(2).sum()
        px = img.astype(int)
        assert (px[..., 0] > px[..., 2] + 20).mean() > 0.05 and (px[..., 2] > px[..., 0] + 20).mean() > 0.05     # a red and a blue triangle
        sc.check()
    finally:
        sc.close()


def test_cli_refuses_what_does_not_go_with_colour(tmp_path):
    def run(*extra):
        return subprocess.run([CLI] + BASE + list(extra), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    light = ("--light", "point:0,1.8,0")
    for extra, msg in ((("--colour",), "--light"), ((*light, "--colour", "--bounce-samples", "4", "--bounce-albedo", "0.5"), "--bounce-albedo"),
                       ((*light, "--colour", "--bounce-stride", "2"), "--bounce-samples")):
        r = run(*extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "cornell_rend.png").exists()
