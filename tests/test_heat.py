"""The PROFILE_RT heat map without a GPU: the colour rule's published anchors, the record type, every refusal (decided before a
device is touched) and the twin of the per-ray counts (tests/heat_twin.py) against the oracle's pass totals.  The GPU side is
tests/test_gpu_heat.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import heat_twin as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")
IMAGE_FIXTURES = ("soup_52x44", "cornell_64", "cornell_tlas_48", "kitchen_tlas_f16_56x40")
ALL_COUNTS = np.arange(65536)


@pytest.fixture(scope="module")
def ramps():
    return {H.HEAT_NODES: H.heat_rgba(ALL_COUNTS, H.HEAT_NODES, H.SCALE_NODES),
            H.HEAT_TRIS: H.heat_rgba(ALL_COUNTS, H.HEAT_TRIS, H.SCALE_TRIS)}


def test_anchors_of_the_colour_rule(ramps):
    """Nodes mode at the reference scale, counts 0 / 6 / 12 / 25 / 50 / 62 (include/trx.h states the rule; the anchors were
    published with it).  Alpha is 255 everywhere.  (No monotonicity: the palette is not monotone.)"""
    img = ramps[H.HEAT_NODES]
    want = {0: (0, 2, 91), 6: (0, 51, 165), 12: (0, 156, 238), 25: (153, 237, 0), 50: (209, 11, 42), 62: (145, 0, 65)}
    for count, rgb in want.items():
        assert tuple(int(v) for v in img[count, :3]) == rgb, count
    for img in ramps.values():
        assert (img[:, 3] == 255).all()


def test_saturation_points_and_colour_counts(ramps):
    """At the reference scales the image is constant from n_node = 61 on (61 distinct colours) and from n_tri = 98 on (97)."""
    for which, first_constant, colours in ((H.HEAT_NODES, 61, 61), (H.HEAT_TRIS, 98, 97)):
        img = ramps[which]
        assert (img[first_constant:] == img[65535]).all(), which
        assert (img[first_constant - 1] != img[65535]).any(), which
        assert np.unique(img, axis=0).shape[0] == colours, which
        assert tuple(int(v) for v in img[65535, :3]) == (145, 0, 65)


def test_scale_zero_and_an_overflowing_scale_are_defined():
    """x = 0 is the first palette row; a finite scale whose product overflows to +inf is the last one."""
    assert (H.heat_rgba(ALL_COUNTS[:100], H.HEAT_TRIS, 0.0)[:, :3] == (0, 2, 91)).all()
    big = H.heat_rgba(np.array([0, 1, 65535]), H.HEAT_NODES, 3.0e38)
    assert tuple(big[0, :3]) == (0, 2, 91) and (big[1:, :3] == (145, 0, 65)).all()


def test_record_type_is_four_bytes(trx):
    from tray_racing_amd import _lib
    assert C.sizeof(_lib.RayCost) == 4 and trx.RAY_COST_DTYPE.itemsize == 4 and H.COST_DTYPE == trx.RAY_COST_DTYPE
    assert _lib.RayCost.n_node.offset == 0 and _lib.RayCost.n_tri.offset == 2
    src = (b'#include "trx.h"\n_Static_assert(sizeof(trx_ray_cost) == 4, "size");\n'
           b'_Static_assert(TRX_HEAT_NODES == 0u && TRX_HEAT_TRIS == 1u, "modes");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)
    assert (_lib.HEAT_NODES, _lib.HEAT_TRIS) == (0, 1)
    assert np.float32(_lib.HEAT_SCALE_NODES) == H.SCALE_NODES and np.float32(_lib.HEAT_SCALE_TRIS) == H.SCALE_TRIS


def test_every_refusal_is_decided_before_a_device_is_touched(trx):
    """No scene exists without a device, so every call here carries a null scene: the argument checks come first and name
    what they refuse; with good arguments the null scene is what is refused.  Nothing is enqueued, nothing crashes."""
    from tray_racing_amd import _lib as L
    lib = trx.load()
    view, st = L.View(), L.Stats()
    cost = (L.RayCost * 4)()
    rgba = (C.c_uint8 * 20)()
    shard = L.Shard(0, 1, 0, 0)
    P = C.c_void_p

    def refused(rc, word):
        assert rc == L.TRX_ERR_INVALID and word in lib.trx_last_error(), (rc, lib.trx_last_error())

    refused(lib.trx_count_primary_per_ray(None, C.byref(view), 8, 8, shard, 0, None, None, C.byref(st)), b"d_cost")
    refused(lib.trx_count_primary_per_ray(None, C.byref(view), 8, 8, shard, 0, None, cost, C.byref(st)), b"null scene")
    refused(lib.trx_count_ao_per_ray(None, C.byref(view), 8, 8, shard, 0, 0, 0.01, cost, None, None, C.byref(st)), b"d_cost")
    refused(lib.trx_count_ao_per_ray(None, C.byref(view), 8, 8, shard, 0, 0, 0.01, cost, None, cost, C.byref(st)), b"null")
    refused(lib.trx_count_rays_per_ray(None, cost, 1, 0, None, None, C.byref(st)), b"d_cost")
    refused(lib.trx_count_rays_per_ray(None, cost, 1, 0, None, cost, C.byref(st)), b"bad ray batch")
    for which, scale, word in ((2, 0.002, b"TRX_HEAT_NODES"), (0xFFFFFFFF, 0.002, b"TRX_HEAT_NODES"), (0, float("nan"), b"scale"),
                               (0, -1.0, b"scale"), (1, float("inf"), b"scale"), (1, -0.0, b"null scene")):
        refused(lib.trx_shade_heat_dev(None, cost, 4, which, scale, rgba, None), word)
        refused(lib.trx_render_heat_image(None, C.byref(view), 8, 8, 0, which, scale, rgba, None), word if word != b"null scene" else b"null")
    refused(lib.trx_shade_heat_dev(None, cost, 4, 0, 0.002, P(C.addressof(rgba) + 2), None), b"aligned")
    refused(lib.trx_shade_heat_dev(None, cost, 0, 0, 0.002, rgba, None), b"null scene")
    refused(lib.trx_render_heat_image(None, C.byref(view), 0, 8, 0, 0, 0.002, rgba, None), b"image")
    refused(lib.trx_render_heat_image(None, C.byref(view), 8, 8, 8, 0, 0.002, rgba, None), b"semantics")
    refused(lib.trx_render_heat_image(None, None, 8, 8, 0, 0, 0.002, rgba, None), b"null")
    assert bytes(rgba) == bytes(20) and bytes(cost) == bytes(16)


def test_cli_lists_and_checks_profile_rt():
    def run(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=120)
    usage = run("--help")
    assert usage.returncode == 0 and "--profile-rt nodes|tris" in usage.stdout and "--profile-rt-scale" in usage.stdout
    base = ("-i", "standin:cornell", "--dry-run", "--passes", "1")
    for extra, msg in ((("--profile-rt", "nodes", "--ao-samples", "4"), "not together"),
                       (("--profile-rt", "tris", "--ao-samples", "4", "--ao-filter", "1"), "not together"),
                       (("--profile-rt", "boxes"), "nodes or tris"),
                       (("--profile-rt-scale", "0.5"), "--profile-rt nodes|tris"),
                       (("--profile-rt", "nodes", "--profile-rt-scale", "-1"), "finite"),
                       (("--profile-rt", "nodes", "--profile-rt-scale", "inf"), "finite")):
        r = run(*base, *extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert run(*base, "--profile-rt", "tris", "--profile-rt-scale", "0.02", "--png").returncode == 0


@pytest.mark.parametrize("name", IMAGE_FIXTURES)
def test_per_ray_twin_sums_to_the_pass_totals_and_is_not_vacuous(orc, name):
    """Per-ray counts of the primary frame sum to trace_primary's n_node / n_tri under TRX_SEM_HLSL and semantics word 3, and
    the frame is a heat map worth the name - asserted on the oracle's output alone: at least 10 distinct n_node values, at
    least 10 distinct n_tri values, a largest n_node of at least 15 (a flat image would pass any comparison)."""
    g, osc, ov, w, h = H.golden(orc, name)
    for sem in (orc.SEM_HLSL, 3):
        cost = H.primary_cost(osc, ov, w, h, sem)
        _, st = osc.trace_primary(ov, w, h, sem=sem)
        assert int(cost["n_node"].sum(dtype=np.int64)) == st.n_node and int(cost["n_tri"].sum(dtype=np.int64)) == st.n_tri, (name, sem)
        assert cost["n_node"].max() < 65535 and cost["n_tri"].max() < 65535
        assert np.unique(cost["n_node"]).size >= 10 and np.unique(cost["n_tri"]).size >= 10 and cost["n_node"].max() >= 15, (
            name, sem, np.unique(cost["n_node"]).size, np.unique(cost["n_tri"]).size, int(cost["n_node"].max()))


def test_one_ray_at_a_time_equals_the_per_ray_counters(orc):
    """trace_rays over the frame's primary rays, one ray per call, gives count_per_ray's records: the method the explicit-ray
    and AO twins rest on."""
    g, osc, ov, w, h = H.golden(orc, "cornell_tlas_48")
    rays = osc.primary_rays(ov, w, h)
    for sem in (orc.SEM_HLSL, 3):
        assert (H.rays_cost(osc, rays, sem) == H.primary_cost(osc, ov, w, h, sem)).all(), sem


@pytest.mark.parametrize("name", ("soup_52x44", "cornell_tlas_48"))
def test_ao_twin_sums_to_the_ao_pass_totals(orc, name):
    """The AO rays of tests/ao_visibility_twin.py at tmax = FLT_MAX, each walked alone, sum to trace_ao's n_node / n_tri and
    number its n_rays - so the GPU test may pin AO records one by one - with surface and no-surface pixels both present."""
    g, osc, ov, w, h = H.golden(orc, name)
    for sem in (orc.SEM_HLSL, 3):
        prim, _ = osc.trace_primary(ov, w, h, sem=sem)
        for frame, eps in ((3, 0.01), (7, 0.0001)):
            cost, surface = H.ao_cost(orc, osc, ov, w, h, prim, sem, frame, eps)
            _, st = osc.trace_ao(ov, w, h, prim, sem=sem, frame=frame, ao_eps=eps)
            assert 0 < surface.sum() < w * h and int(surface.sum()) == st.n_rays
            assert int(cost["n_node"].sum(dtype=np.int64)) == st.n_node and int(cost["n_tri"].sum(dtype=np.int64)) == st.n_tri
            assert (cost[~surface] == np.zeros(1, dtype=H.COST_DTYPE)).all() and cost["n_node"][surface].min() >= 1
