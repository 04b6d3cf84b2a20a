"""tray_racing_hip --png --ao-samples N --ao-stride S [--ao-phase P] [--ao-upsample R]: the image is trx_render_image_sparse's -
the composition tests/test_gpu_ao_sparse.py holds to the twin - and without --ao-stride the program does what it did."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from ao_sparse_twin import ao_upsample, lo_size, sparse_counts
from image_twin import shade_term

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tray_racing_amd", "tray_racing_hip")
W, H, N, RADIUS = 96, 64, 4, 1.4


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
    r = subprocess.run([CLI, "-i", "standin:cornell", "--render-time", "0", "--width", str(W), "--height", str(H), "--passes", "1",
                        "--png", "--cpu-semantics", "--ao-samples", str(N), "--ao-radius", str(RADIUS)] + list(extra),
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    return _png(str(tmp_path / "cornell_rend.png"), W, H).copy()


def test_cli_png_with_ao_stride_is_the_sparse_frame(trx, tmp_path):
    import torch
    assert trx.load().trx_device_count() > 0, "no HIP device visible to libtrx.so"
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    eye, look, fov = trx.scene_camera("cornell")
    view = trx.view_from_camera(eye, look, fov, W, H)
    sc = trx.Scene(flat)
    try:
        # the records the twin is fed: the device's own, as in tests/test_gpu_ao_sparse.py (the command line's ao_eps is 0.0001)
        n = W * H
        d_prim = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
        d_attr = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(n, dtype=torch.uint8, device="cuda")
        sc.trace_primary_dev(view, W, H, d_prim.data_ptr(), sem=3)
        sc.hit_attributes_primary_dev(view, W, H, d_prim.data_ptr(), d_attr.data_ptr())
        sc.trace_ao_visibility_dev(view, W, H, d_prim.data_ptr(), d_cnt.data_ptr(), N, RADIUS, sem=3, frame0=0, ao_eps=0.0001)
        torch.cuda.synchronize()
        prim, attr, cnt = d_prim.cpu().numpy().view(trx.HIT_DTYPE), d_attr.cpu().numpy().view(trx.HIT_ATTR_DTYPE), d_cnt.cpu().numpy()
        images = {}
        for stride, phase, r, flags in ((2, 0, 1, ("--ao-stride", "2")), (2, 3, 2, ("--ao-stride", "2", "--ao-phase", "3", "--ao-upsample", "2")),
                                        (3, 4, 0, ("--ao-stride", "3", "--ao-phase", "4", "--ao-upsample", "0", "--ao-depth-tol", "0.05",
                                                   "--ao-normal-cos", "0.5"))):
            tol, cos = (0.05, 0.5) if stride == 3 else (0.02, 0.9)
            img = _run(tmp_path, *flags)
            want, _ = sc.render_image_sparse(view, W, H, N, stride, ao_phase=phase, upsample_radius=r, sem=3, frame0=0, ao_eps=0.0001,
                                             ao_radius=RADIUS, depth_tol=tol, normal_cos=cos)
            assert (img == want).all(), "stride %d phase %d: %d pixels differ from trx_render_image_sparse" % (stride, phase, (img != want).any(2).sum())
            lo = sparse_counts(cnt, W, H, stride, phase)
            assert lo.size == lo_size(W, H, stride)[0] * lo_size(W, H, stride)[1]
            twin = shade_term(ao_upsample(prim, attr["normal"], lo, W, H, stride, phase, N, r, tol, cos))
            assert (img.reshape(-1, 4) == twin).all(), "stride %d phase %d: differs from the twin" % (stride, phase)
            assert (img[..., 3] == 255).all() and np.unique(img[..., 0]).size >= 4
            images[(stride, phase)] = img
        assert (images[(2, 0)] != images[(2, 3)]).any()
        # stride 1 without a window is the dense pass's own image: {count, N} per pixel, the counts shade of --ao-filter 0
        dense = _run(tmp_path, "--ao-filter", "0")
        assert (_run(tmp_path, "--ao-stride", "1", "--ao-upsample", "0") == dense).all()
        assert (dense != images[(2, 0)]).any()
        # without --ao-stride the program does what it did: the host loop over trx_trace_ao_visibility's counts
        plain = _run(tmp_path)
        col = np.where(cnt == 0xFF, 0.0, cnt / float(N))
        assert (plain[..., 0].reshape(-1) == (np.power(col, 2.2) * 255.0).astype(np.uint8)).all()
        sc.check()
    finally:
        sc.close()
