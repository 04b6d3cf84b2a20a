"""tray_racing_hip: the reference's command line (src/main.rs:65-171) over the C ABI."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")


def run(*args, cwd=None):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=600, cwd=cwd)


def test_cli_is_built_and_links_only_the_abi():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tray_racing_amd", "csrc"), "all"])
    needed = subprocess.check_output(["readelf", "-d", CLI]).decode()
    assert "libtrx.so" in needed and "liboracle" not in needed
    assert run("--help").returncode == 0


def test_cli_rejects_what_the_reference_rejects():
    r = run("-i", "standin:cornell", "--max-prims-per-leaf", "4")
    assert r.returncode != 0 and "CWBVH only supports a maximum of 3 primitives per leaf." in r.stderr  # src/main.rs:176-178
    r = run("-i", "standin:cornell", "--build", "nope")
    assert r.returncode != 0 and "NO BVH BUILDER SPECIFIED" in r.stderr                                   # src/cwbvh.rs:99
    for flag, msg in (("--cpu", "no CPU traversal"), ("--hardware", "ray-tracing hardware")):
        r = run("-i", "standin:cornell", flag)
        assert r.returncode != 0 and msg in r.stderr
    r = run("-i", "standin:cornell", "--preset", "warp_speed", "--dry-run")
    assert r.returncode != 0 and "unknown preset" in r.stderr
    assert run("-i", "standin:cornell", "--preset", "very_fast_build", "--dry-run", "--passes", "1").returncode == 0
    assert run().returncode != 0


def parse_table(text):
    lines = [l for l in text.splitlines() if l.strip()]
    hdr = lines[0].split()
    assert hdr == ["name", "traversal_ms", "blas_build_time_s", "tlas_build_time_ms"]  # src/main.rs:634-640
    return {l.split()[0]: [float(x) for x in l.split()[1:]] for l in lines[1:]}


@pytest.mark.gpu
def test_cli_benchmark_table(tmp_path):
    r = run("-i", "standin:cornell,standin:kitchen", "--benchmark", "--render-time", "0.05", "--width", "320", "--height",
            "184", "--passes", "2", "--tlas")
    assert r.returncode == 0, r.stderr
    rows = parse_table(r.stdout)
    assert set(rows) == {"cornell", "kitchen", "Avg"}
    assert all(v[0] > 0 for v in rows.values())
    assert abs(rows["Avg"][0] - 0.5 * (rows["cornell"][0] + rows["kitchen"][0])) < 1e-3 * rows["Avg"][0] + 1e-6
    assert rows["cornell"][2] > 0  # a TLAS was built


@pytest.mark.gpu
def test_cli_overlapped_frame_loop_and_device_preset_build(tmp_path):
    """Round 6: --overlap keeps the frame loop on the device with frame i's AO pass under frame i + 1's primary pass
    (trx_frame_loop), --gpu-build --preset builds the preset with every stage on the device
    (trx_flat_build_preset_device); the table keeps the reference's shape."""
    r = run("-i", "standin:kitchen", "--benchmark", "--overlap", "--render-time", "0.05", "--width", "320", "--height", "184",
            "--passes", "1", "--animate")
    assert r.returncode == 0, r.stderr
    rows = parse_table(r.stdout)
    assert set(rows) == {"kitchen", "Avg"} and rows["kitchen"][0] > 0
    serial = run("-i", "standin:kitchen", "--benchmark", "--render-time", "0.05", "--width", "320", "--height", "184", "--passes", "1")
    assert serial.returncode == 0 and parse_table(serial.stdout)["kitchen"][0] > 0
    r = run("-i", "standin:kitchen", "--gpu-build", "--preset", "medium_build", "--render-time", "0", "--width", "64", "--height", "64",
            "--passes", "1")
    assert r.returncode == 0, r.stderr
    rows = parse_table(r.stdout)
    assert rows["kitchen"][0] > 0 and rows["kitchen"][1] > 0


@pytest.mark.gpu
def test_bench_takes_a_real_scene_file(tmp_path):
    """Round 6 (review item 6): `bench.py --input <scene.ron>` runs the frame of a scene file of the reference - model through
    trx_load_scene, camera from the file - and says `data: "real"`.  Here a small scene written on the spot."""
    import json
    import subprocess
    import sys
    (tmp_path / "assets" / "scenes").mkdir(parents=True)
    (tmp_path / "assets" / "obj").mkdir(parents=True)
    (tmp_path / "assets" / "obj" / "quad.obj").write_text(
        "o quad\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nf 1 2 3 4\no tri\nv -1 -1 -1\nv 1 -1 -1\nv 0 1 -1\nf 5 6 7\n")
    scene = str(tmp_path / "assets" / "scenes" / "quad.ron")
    open(scene, "w").write('(\n model_path: "assets/obj/quad.obj",\n camera: (\n eye: (0.0, 0.0, 3.0),\n look_at: (0.0, 0.0, 0.0),\n'
                           ' fov: 60.0,\n exposure: 0.0,\n ),\n sun_direction: (0.5, -0.24, 0.5),\n)')
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--input", scene, "--steps", "5", "--warmup", "2", "--width", "256",
                          "--height", "144", "--full", "--no-legs", "--no-pmc", "--cpu-seconds", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["data"] == "real" and os.path.basename(scene) in d["config"]["workload"] and d["value"] > 0
    assert d["parity_vs_oracle_full_frame"] is True and d["build"]["lib_sha16"]


@pytest.mark.gpu
def test_cli_ron_scene_with_relative_model_path(tmp_path):
    """RON subset + the reference's path rule: a relative model path is resolved against the scene
    file's great-grandparent directory (src/main.rs:271-284)."""
    root = tmp_path
    (root / "assets" / "scenes").mkdir(parents=True)
    (root / "assets" / "obj").mkdir(parents=True)
    (root / "assets" / "obj" / "quad.obj").write_text(
        "o quad\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nf 1 2 3 4\no tri\nv -1 -1 -1\nv 1 -1 -1\nv 0 1 -1\nf 5 6 7\n")
    (root / "assets" / "scenes" / "quad.ron").write_text("""(
    model_path: "assets/obj/quad.obj",
    camera: (
        eye: (0.0, 0.0, 3.0),
        look_at: (0.0, 0.0, 0.0),
        fov: 60.0,
        exposure: 0.0,
    ),
    sun_direction: (0.5, -0.24, 0.5),
    //sun_direction: (-0.27, -0.24, 1.0),
)""")
    r = run("-i", "assets/scenes/quad.ron", "--render-time", "0", "--width", "64", "--height", "64", "--passes", "1",
            "--verbose", cwd=str(root))
    assert r.returncode == 0, r.stderr
    assert re.search(r"2 objects \"quad\"\s+triangles 3", r.stdout)
    rows = parse_table(r.stdout[r.stdout.index(" name"):])
    assert set(rows) == {"quad", "Avg"} and rows["quad"][0] > 0
    r = run("-i", "assets/scenes/missing.ron", cwd=str(root))
    assert r.returncode != 0 and "Failed to load config" in r.stderr


@pytest.mark.gpu
def test_cli_png_is_the_reference_shading(tmp_path):
    """--png: `<name>_rend.png`, AO term of the primary hit (1/t on a miss), gamma 2.2 to u8
    (src/rt_cpu/rt_cpu.rs:57-85,102-112), checked against the oracle's primary + AO pass."""
    import struct
    import sys
    import zlib

    import numpy as np
    sys.path.insert(0, ROOT)
    import tray_racing_amd as T
    from oracle import binding as O

    w, h = 96, 64
    r = run("-i", "standin:cornell", "--render-time", "0", "--width", str(w), "--height", str(h), "--passes", "1", "--png",
            "--cpu-semantics", cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    data = (tmp_path / "cornell_rend.png").read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert zlib.crc32(tag + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        if tag == b"IDAT":
            idat += body
        pos += 12 + n
    assert ihdr == (w, h, 8, 6, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    assert (raw[:, 0] == 0).all()
    img = raw[:, 1:].reshape(h, w, 4)
    assert (img[..., 3] == 255).all() and (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all()

    verts, counts = T.gen_scene("cornell", 0, 1)
    flat = T.flat_build(verts, counts)
    eye, look, fov = T.scene_camera("cornell")
    ov = O.view_from_bytes(T.view_from_camera(eye, look, fov, w, h))
    osc = O.Scene.from_flat(flat)
    prim, _ = osc.trace_primary(ov, w, h, sem=3)
    ao, _ = osc.trace_ao(ov, w, h, prim, sem=3, frame=0, ao_eps=0.0001)
    fmax = np.float32(3.4028234663852886e38)
    with np.errstate(divide="ignore"):
        col = np.where(prim["t"] < fmax, np.where(ao["t"] < fmax, ao["t"] / (np.float32(1) + ao["t"]), np.float32(1)),
                       np.float32(1) / prim["t"]).astype(np.float32)
    want = (np.power(col.astype(np.float64), 2.2) * 255.0).astype(np.uint32).astype(np.uint8).reshape(h, w)
    diff = np.abs(img[..., 0].astype(int) - want.astype(int))
    assert diff.max() <= 1 and (diff != 0).mean() < 0.01   # powf rounding may move a value across an integer
    assert 0.05 < (img[..., 0] > 0).mean()


def test_cli_reads_the_scene_files_the_reference_ships(tmp_path):
    """--dry-run (scene file + model + build, no device): the RON subset and the relative-model-path rule
    (src/main.rs:262-284) on a tree laid out like the reference's assets/, run from its root: scene files in the layout of
    its assets/scenes/*.ron with their cameras, in-repo stand-ins for its two small models (helpers.obj_text), and scene
    files whose models are absent, as most of the reference's are."""
    from helpers import obj_text
    (tmp_path / "assets" / "scenes").mkdir(parents=True)
    (tmp_path / "assets" / "obj").mkdir(parents=True)
    (tmp_path / "assets" / "obj" / "cornell_box.obj").write_text(obj_text("cornell_box"))
    (tmp_path / "assets" / "obj" / "box.obj").write_text(obj_text("box"))
    scenes = {"cornell_box": ("assets/obj/cornell_box.obj", "(0.0, 1.0, 2.1)", "(0.0, 1.0, 0.0)", "90.0"),
              "box": ("assets/obj/box.obj", "(3.0, 1.5, 1.4)", "(-3.9438584, 1.5, -1.7303504)", "90.0"),
              "bistro": ("assets/large_obj/bistro/bistro.obj", "(-10.5, 1.7, -1.0)", "(12.5, 1.7, -2.0)", "100.0"),
              "hairball": ("assets/large_obj/hairball.obj", "(0.0, 0.0, 7.0)", "(0.0, 0.0, 0.0)", "90.0")}
    for name, (model, eye, look, fov) in scenes.items():
        (tmp_path / "assets" / "scenes" / (name + ".ron")).write_text(
            '(\n    model_path: "%s",\n    camera: (\n        eye: %s,\n        look_at: %s,\n        fov: %s,\n'
            '        exposure: 1.0,\n    ),\n    sun_direction: (-1.0, -0.24, -0.28),\n    //sun_direction: (-0.27, -0.24, 1.0),\n)\n'
            % (model, eye, look, fov))
    import tray_racing_amd as T
    _, cornell_counts = T.gen_scene("cornell", 0, 1)
    r = run("-i", "assets/scenes/cornell_box.ron,assets/scenes/box.ron", "--dry-run", "--verbose", "--passes", "1", "--tlas",
            cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert re.search(r"%d objects \"cornell_box\"\s+triangles %d" % (len(cornell_counts), int(cornell_counts.sum())), r.stdout)
    assert re.search(r"2 objects \"box\"\s+triangles 14", r.stdout)
    assert "camera eye 0 1 2.1 look_at 0 1 0 fov 90" in r.stdout              # cornell_box.ron
    assert "camera eye 3 1.5 1.4 look_at -3.94386 1.5 -1.73035 fov 90" in r.stdout  # box.ron
    rows = parse_table(r.stdout[r.stdout.index(" name"):])
    assert set(rows) == {"cornell_box", "box", "Avg"} and rows["box"][2] > 0
    # every scene file parses; the ones whose models are absent fail on the model only
    for f in sorted(os.listdir(tmp_path / "assets" / "scenes")):
        r = run("-i", "assets/scenes/" + f, "--dry-run", "--passes", "1", cwd=str(tmp_path))
        ok_model = f in ("cornell_box.ron", "box.ron")
        assert (r.returncode == 0) == ok_model, (f, r.stderr)
        if not ok_model:
            assert "Failed to load config" not in r.stderr, f   # the scene file itself parsed; only the model is missing
