"""tray_racing_hip --png --light ... --bounce-samples N --bounce-stride S [--bounce-filter L]: the image is
trx_render_image_gi_sparse's - the composition tests/test_gpu_indirect_sparse.py holds to the twin - the options that do not
go together are refused, and without --bounce-stride the program writes the images it wrote before."""
import subprocess

import pytest

from test_gpu_light_cli import BASE, CLI, H, W, _run

pytestmark = pytest.mark.gpu


def test_cli_png_with_a_bounce_stride_is_the_sparse_gi_frame(trx, tmp_path):
    assert trx.load().trx_device_count() > 0, "no HIP device visible to libtrx.so"
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    eye, look, fov = trx.scene_camera("cornell")
    view = trx.view_from_camera(eye, look, fov, W, H)
    sc = trx.Scene(flat)
    point = trx.light(trx.LIGHT_POINT, (0.0, 1.8, 0.0), intensity=2.0)
    rect = trx.light(trx.LIGHT_RECT, (-0.4, 1.9, -0.4), (0.8, 0.0, 0.0), (0.0, 0.0, 0.8))
    try:
        # the defaults: phase 0, upsample radius 1, depth tolerance 0.1, cosine 0.9 on top of the filtered GI image's
        img = _run(tmp_path, "--light", "point:0,1.8,0:2", "--bounce-samples", "4", "--bounce-stride", "2", "--bounce-filter", "3")
        want, _ = sc.render_image_gi_sparse(view, W, H, [point], 4, 2, bounce_phase=0, bounce_upsample_radius=1, bounce_filter_levels=3,
                                            bounce_depth_tol=0.1, bounce_normal_cos=0.9, bounce_eps=0.01, bounce_albedo=0.5, sem=3, shadow_eps=0.01,
                                            ambient=0.1)
        assert (img == want).all(), "%d pixels differ from trx_render_image_gi_sparse" % (img != want).any(2).sum()
        # without the option: the filtered GI image as before, and another image
        dense = _run(tmp_path, "--light", "point:0,1.8,0:2", "--bounce-samples", "4", "--bounce-filter", "3")
        want_dense, _ = sc.render_image_gi_filtered(view, W, H, [point], 4, 3, bounce_depth_tol=0.1, bounce_normal_cos=0.9, bounce_eps=0.01,
                                                    bounce_albedo=0.5, sem=3, shadow_eps=0.01, ambient=0.1)
        assert (dense == want_dense).all() and (img[..., 0] != dense[..., 0]).mean() > 0.05
        # without a filter: the upsample adds the term itself
        plain = _run(tmp_path, "--light", "point:0,1.8,0:2", "--bounce-samples", "4", "--bounce-stride", "2")
        want_plain, _ = sc.render_image_gi_sparse(view, W, H, [point], 4, 2, bounce_eps=0.01, bounce_albedo=0.5, sem=3, shadow_eps=0.01, ambient=0.1)
        assert (plain == want_plain).all() and (plain != img).any()
        # every option, two lights, the ambient under the filtered AO term
        img2 = _run(tmp_path, "--light", "point:0,1.8,0:2", "--light", "rect:-0.4,1.9,-0.4:0.8,0,0:0,0,0.8", "--light-samples", "8", "--light-mask", "3",
                    "--shadow-eps", "0.001", "--ambient", "0.25", "--ao-samples", "4", "--ao-radius", "1.4", "--ao-filter", "2", "--bounce-samples", "3",
                    "--bounce-albedo", "0.8", "--bounce-eps", "0.002", "--bounce-stride", "3", "--bounce-phase", "8", "--bounce-upsample", "2",
                    "--bounce-filter", "2", "--bounce-filter-tol", "0.05", "--bounce-filter-cos", "0.5")
        want2, _ = sc.render_image_gi_sparse(view, W, H, [point, rect], 3, 3, bounce_phase=8, bounce_upsample_radius=2, bounce_filter_levels=2,
                                             bounce_depth_tol=0.05, bounce_normal_cos=0.5, bounce_eps=0.002, bounce_albedo=0.8, sem=3, ray_mask=3,
                                             light_samples=8, shadow_eps=0.001, ambient=0.25, ao_samples=4, ao_eps=0.0001, ao_radius=1.4, filter_radius=2)
        assert (img2 == want2).all(), "%d pixels differ from trx_render_image_gi_sparse" % (img2 != want2).any(2).sum()
        assert (img2 != img).any()
        sc.check()
    finally:
        sc.close()


def test_cli_refuses_the_options_that_do_not_go_with_the_bounce_stride(tmp_path):
    def run(*extra):
        return subprocess.run([CLI] + BASE + list(extra), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    light = ("--light", "point:0,1.8,0")
    for extra, msg in (((*light, "--bounce-stride", "2"), "--bounce-samples"), ((*light, "--bounce-samples", "4", "--bounce-stride", "5"), "1..4"),
                       ((*light, "--bounce-samples", "4", "--bounce-stride", "2", "--bounce-phase", "4"), "S*S-1"),
                       ((*light, "--bounce-samples", "4", "--bounce-phase", "1"), "--bounce-stride"),
                       ((*light, "--bounce-samples", "4", "--bounce-stride", "2", "--bounce-upsample", "3"), "0..2")):
        r = run(*extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "cornell_rend.png").exists()
