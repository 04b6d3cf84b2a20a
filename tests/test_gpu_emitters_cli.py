"""The command line's --emitters on the GPU (include/trx.h, "emitters"): `--png --colour --emitters 4` on standin:cornell without a
--light writes the image the binding's host form gives for the same arguments; the floor's codes are above 0 there and above what
trx_render_image_colour gives under the same ambient with a light of intensity 0, which with no ambient leaves it black; and the new refusals."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_gpu_light import limit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")


def _read_png(path):
    """[h, w, 4] uint8 of the 8-bit RGBA, filter 0 image the command line writes."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, w, h = 8, b"", 0, 0
    while at < len(raw):
        n, tag = struct.unpack(">I4s", raw[at:at + 8])
        body = raw[at + 8:at + 8 + n]
        if tag == b"IHDR":
            w, h, depth, kind = struct.unpack(">IIBB", body[:10])
            assert (depth, kind) == (8, 6)
        elif tag == b"IDAT":
            idat += body
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, w * 4 + 1)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 4)


def test_the_command_line_writes_the_host_forms_image(trx, tmp_path):
    w, h = 96, 64
    args = ["-i", "standin:cornell", "--render-time", "0", "--width", str(w), "--height", str(h), "--passes", "1", "--png", "--colour", "--emitters", "4",
            "--bounce-samples", "2", "--emitter-eps", "0.002"]
    with limit(300):
        r = subprocess.run([CLI] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-800:]
    img = _read_png(str(tmp_path / "cornell_rend.png"))
    assert img.shape == (h, w, 4)
    # the same call through the binding: the command line's scene, camera, table (by tri_source) and defaults
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    mats, idx = trx.standin_materials("cornell", verts, counts)
    eye, look, fov = trx.scene_camera("cornell")
    view = trx.view_from_camera(eye, look, fov, w, h)
    sc = trx.Scene(flat)
    try:
        sc.set_materials(mats, idx[flat.tri_source])
        with limit():
            frame0 = 0                                                  # (the frame counter stands still without --animate)
            want, _ = sc.render_image_colour_emitters(view, w, h, emitter_samples=4, emitter_eps=0.002, bounce_samples=2, ambient=0.1, frame0=frame0,
                                                      ao_eps=0.0001)                   # (0.1: the command line's default ambient)
            assert sc.get_emitters()[0].shape[0] == 2
            none = [trx.light(trx.LIGHT_POINT, (0.0, 1.0, 0.0), intensity=0.0)]
            # the same ambient without the emitters sampled (the existing image, a light of intensity 0): the floor gets less ...
            plain, _ = sc.render_image_colour(view, w, h, none, ambient=0.1, frame0=frame0)
            direct, _ = sc.render_image_colour_emitters(view, w, h, emitter_samples=4, emitter_eps=0.002, ambient=0.1, frame0=frame0)
            # ... and with no ambient it is black there
            dark, _ = sc.render_image_colour(view, w, h, none, ambient=0.0, frame0=frame0)
            prim, _ = sc.trace_primary(view, w, h)
    finally:
        sc.close()
    assert (img == want).all(), int((img != want).sum())
    v = flat.tri_verts.reshape(-1, 3, 3)
    floor = (v[:, :, 1] == 0.0).all(1)
    hit = prim["prim"] != 0xFFFFFFFF
    on_floor = (hit & floor[np.where(hit, prim["prim"], 0)]).reshape(h, w)
    assert on_floor.sum() > 200
    # (the shade's code is about 255 v^2.2: the quad's light alone - 0.03 to 0.08 on the floor - stays below code 1, on top of the ambient it shows)
    assert img[on_floor][:, :3].mean() > 0 and dark[on_floor][:, :3].max() == 0
    a, b = direct[on_floor][:, :3].astype(int), plain[on_floor][:, :3].astype(int)
    assert (a >= b).all() and (a > b).mean() > 0.25, ((a > b).mean(), a.mean(), b.mean())


def test_the_new_refusals():
    def run(*args):
        return subprocess.run([CLI, "-i", "standin:cornell", "--dry-run", "--passes", "1"] + list(args), capture_output=True, text=True, timeout=120)
    for extra, msg in ((("--png", "--emitters", "4"), "--colour"), (("--png", "--colour", "--emitters", "4", "--emitter-eps", "1.0"), "--emitter-eps"),
                       (("--png", "--colour", "--emitters", "4", "--emitter-eps", "-1"), "--emitter-eps"), (("--png", "--colour", "--emitter-eps", "0.01"), "--emitters"),
                       (("--png", "--colour", "--emitters", "65"), "--emitters")):
        r = run(*extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert run("--png", "--colour", "--emitters", "4").returncode == 0
